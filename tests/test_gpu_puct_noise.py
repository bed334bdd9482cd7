"""GPU checks of the two random steps of the PUCT searches against their specification
(tests/puct_noise_ref.py): the root priors with Dirichlet noise (ps.prior) and the move sampled
in proportion to N^(1/T), replayed exactly from the device's own logits, visit counts, seed,
game index and search number — chess roots in all four 64-move chunks, Connect4 with a full
column, distinct search numbers per game, a sub-range of the engine's games, split streams,
graph replays, a kept (re-rooted) Connect4 root, and T = 0.01.

Noise tolerance: the float64 specification against the device's float32 arithmetic.  The floor
is max |spec32 - spec64| on the same games (the specification run in float32); the device may
differ from spec64 by 8 floors (its logf / cospif / powf / expf are not numpy's, but of the
same accuracy class).  Games holding a draw whose acceptance margin is below 1e-5 are left out
(rounding may flip that accept), at most 3 % of a case's games.

Measured on an MI355X (max over a case's kept games and moves; 256 games a case):

    chess  device - spec64 3.1e-8 .. 1.3e-7   floor 3.1e-8 .. 1.3e-7   left out 0 or 1 of 256
    c4     device - spec64 8.1e-8 .. 1.3e-7   floor 8.2e-8 .. 1.5e-7   left out 0 of 256

The device error never passed 1.2 floors (in most cases the two are the same number: the worst
element is one where the device and spec32 agree to the bit).  The one chess game left out is
at alpha = 0.03; the launch-path cases (128 games) left out 1 game in one case (chess,
first_game = 5), the kept-root case none.  The temperature replays left out no game at any T.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import puct_ref
import puct_noise_ref as ref

pytestmark = pytest.mark.gpu

G = 256
SEED = 0x9E3779B97F4A7C15   # both key words in use
MARGIN, MAX_OUT = 1e-5, 0.03
FLOOR_CAP = 1e-4   # a prior <= 1 through a dozen float32 roundings errs by 1e-7..1e-6; a floor
#                    above this means spec32 itself took another branch than spec64

WIDE = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"
CHESS_ROOTS = [(WIDE, 218), ("R6R/3Q4/1Q4Q1/4Q3/2Q5/5Q2/pp1Q4/kBNN1KB1 w - - 0 1", 194),
               ("R6R/3Q4/1Q4Q1/4Q3/8/5Q2/pp1Q4/kBNN1KB1 w - - 0 1", 171),
               ("R6R/3Q4/1Q6/8/8/5Q2/pp1Q4/kBNN1KB1 w - - 0 1", 131),
               ("R6R/8/1Q6/8/8/5Q2/pp1Q4/kBNN1KB1 w - - 0 1", 112),
               ("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", 20),
               ("r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1", 46)]


def _mix(h):
    h = h ^ (h >> np.uint64(29))
    h = h * np.uint64(0xBF58476D1CE4E5B9)
    return h ^ (h >> np.uint64(32))


@functools.lru_cache(maxsize=None)
def _logits(rows, width, f16):
    """A hash of (row, move) in [-3, 3], as the tensor the network returns."""
    r = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(0x9E3779B97F4A7C15)
    m = np.arange(width, dtype=np.uint64)[None, :] * np.uint64(0xC2B2AE3D27D4EB4F)
    lg = (_mix(r + m) % np.uint64(6001)).astype(np.float32) / np.float32(1000) - np.float32(3)
    t = torch.from_numpy(lg).cuda()
    return t.half() if f16 else t


def _values(leaves):
    """hash_net-style values: a fixed pseudo-random function of the leaf's bytes."""
    b = leaves.cpu().numpy().view(np.uint8).reshape(leaves.shape[0], -1).astype(np.uint64)
    w = _mix(np.arange(1, b.shape[1] + 1, dtype=np.uint64) * np.uint64(0x165667B19E3779F9))
    h = _mix((b * w[None, :]).sum(axis=1, dtype=np.uint64))
    return torch.from_numpy(((h % np.uint64(200001)).astype(np.float64) - 100000.0) / 100003.0).cuda()


def _host_net(logits):
    return lambda leaves, planes, counts: (_values(leaves), logits)


def _device_net(logits, lo=0, hi=None):
    """Values from the planes on the device (capturable); rows [lo, hi) of the logits."""
    lg, w = logits[lo:hi], {}

    def fn(leaves, planes, counts):
        x = planes.reshape(planes.shape[0], -1).float()
        if x.shape[1] not in w:   # first made by the warm-up call, outside any capture
            w[x.shape[1]] = torch.linspace(-9.0, 9.0, x.shape[1], device=x.device).cos_()
        return torch.tanh(x @ w[x.shape[1]] * 0.37).double(), lg
    return fn


class Chess:
    name, width = "chess", 4096

    def __init__(self):
        from zeroclone_amd._native import NativeEngine
        self.eng = NativeEngine(max_games=G + 8, max_sims=400, max_batch=16)
        self.moves = {}
        for fen, count in CHESS_ROOTS:
            self.moves[fen] = oracle.chess_moves(oracle.chess_from_fen(fen))
            assert len(self.moves[fen]) == count
        counts = sorted(c for _, c in CHESS_ROOTS)
        for lo, hi in ((1, 64), (65, 128), (129, 192), (193, 256)):   # every chunk of 64 moves
            assert any(lo <= c <= hi for c in counts)

    def positions(self, n):
        return [CHESS_ROOTS[i % len(CHESS_ROOTS)][0] for i in range(n)]

    def roots(self, pos):
        from zeroclone_amd._native import CHESS_STATE_DTYPE, chess_from_fen
        a = np.array([chess_from_fen(f) for f in pos], CHESS_STATE_DTYPE)
        return torch.from_numpy(a.view(np.uint8).reshape(len(pos), 72).copy()).cuda()

    def search(self, n, bs, **kw):
        from zeroclone_amd.valued import ChessPuctSearch
        return ChessPuctSearch(self.eng, n, bs, **kw)

    def logit_index(self, p):
        return [(fr * 8 + fc) * 64 + tr * 8 + tc for fr, fc, tr, tc, _ in self.moves[p]]

    def in_list_order(self, row, p):
        return row[:len(self.moves[p])]

    def index_of(self, mv, p):
        from zeroclone_amd._native import unpack_chess_move
        (fr, fc, tr, tc), v = unpack_chess_move(int(mv) & 0xFFFF)
        return self.moves[p].index((fr, fc, tr, tc, v))


class C4:
    name, width = "c4", 7

    def __init__(self, max_games=G + 8, max_sims=400):
        from zeroclone_amd._native import NativeEngine
        self.eng = NativeEngine(max_games=max_games, max_sims=max_sims, max_batch=16)
        b, t = "." * 42, 0
        for col in [0, 0, 0, 0, 0, 0, 1, 2]:   # column 0 full
            b, t = oracle.play(b, t, col)
        self.pos = [("." * 42, 0), (b, t)]
        assert len(self.cols(self.pos[0])) == 7 and len(self.cols(self.pos[1])) == 6

    def positions(self, n):
        return [self.pos[i % 2] for i in range(n)]

    def roots(self, pos):
        from zeroclone_amd._native import c4_from_rows
        rows = np.array([c4_from_rows(b, t) for b, t in pos])
        return torch.from_numpy(rows.view(np.int64).reshape(len(pos), 3).copy()).cuda()

    def search(self, n, bs, **kw):
        from zeroclone_amd.valued import C4PuctSearch
        return C4PuctSearch(self.eng, n, bs, **kw)

    @staticmethod
    def cols(p):
        return puct_ref.C4Rules.moves(p)

    logit_index = cols

    def in_list_order(self, row, p):
        return row[self.cols(p)]

    def index_of(self, mv, p):
        return self.cols(p).index(int(mv))


@pytest.fixture(scope="module")
def games():
    g = {"chess": Chess(), "c4": C4()}
    yield g
    for x in g.values():
        x.eng.close()


def _listed(game, rows, pos):
    """Per-move device rows [n, *] -> [n, K] in each game's move-list order, and nm [n]."""
    per = [game.in_list_order(rows[i], p) for i, p in enumerate(pos)]
    nm = np.array([len(x) for x in per])
    out = np.zeros((len(pos), nm.max()), dtype=rows.dtype)
    for i, x in enumerate(per):
        out[i, :len(x)] = x
    return out, nm


def check_noise(game, prior, pos, root_logits, alpha, eps, sno, first=0, sm=None, what=""):
    """prior [n, *]: the device's root priors; root_logits [n, width]: the logits of each game's
    root row, as the device read them; sm: the priors under the noise where they are not the
    softmax of root_logits (a kept root).  Returns (device error, floor, games left out)."""
    n = len(pos)
    dev, nm = _listed(game, prior.astype(np.float64), pos)
    lg = np.zeros(dev.shape)
    for i, p in enumerate(pos):
        lg[i, :nm[i]] = root_logits[i, game.logit_index(p)]
    games_ix = first + np.arange(n)
    if sm is None:
        sm64, sm32 = ref.softmax(lg, nm), ref.softmax(lg, nm, np.float32)
    else:
        sm64, sm32 = sm[:, :dev.shape[1]], sm[:, :dev.shape[1]].astype(np.float32)
    p64, margin = ref.root_prior(sm64, alpha, eps, SEED, games_ix, nm, sno)
    p32, _ = ref.root_prior(sm32, alpha, eps, SEED, games_ix, nm, sno, np.float32)
    keep = margin >= MARGIN
    out = int((~keep).sum())
    err = float(np.abs(dev - p64)[keep].max())
    floor = float(np.abs(p32.astype(np.float64) - p64)[keep].max())
    print(f"noise {game.name} {what}: device-spec64 {err:.3e} floor {floor:.3e} left out {out}/{n}")
    assert out <= MAX_OUT * n
    assert 0 < floor < FLOOR_CAP
    assert err <= 8 * floor, (err, floor)
    np.testing.assert_allclose(dev.sum(axis=1), 1.0, atol=1e-5)
    return err, floor, out


def check_sample(game, mv, na, pos, T, sno, first=0, exact=True, visits=None, what=""):
    """The device's move is sample_index of its own counts."""
    na_l, nm = _listed(game, na, pos)
    out = 0
    for i, p in enumerate(pos):
        if visits is not None:
            assert int(na_l[i].sum()) == visits
        idx, dist = ref.sample_index(na_l[i, :nm[i]], T, SEED, first + i, int(sno[i]))
        if not exact and dist < 1e-9:
            out += 1
            continue
        assert game.index_of(mv[i], p) == int(idx), (game.name, what, i, T)
    print(f"sample {game.name} {what} T={T}: left out {out}/{len(pos)}")
    assert out <= 0.01 * len(pos)
    return out


def _set_search_numbers(ps):
    sno = 3 + 7 * np.arange(ps.n, dtype=np.int32)
    ps.search_no.copy_(torch.from_numpy(sno))
    return sno


def _root_rows(logits, n, bs):
    return logits.view(n, bs, -1)[:, 0].double().cpu().numpy()


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("eps", [0.25, 1.0])
@pytest.mark.parametrize("alpha", [0.3, 1.0, 0.03])
@pytest.mark.parametrize("name", ["chess", "c4"])
def test_root_noise_replays_the_specification(games, name, alpha, eps, f16):
    game, bs, sims = games[name], 8, 9
    pos = game.positions(G)
    logits = _logits(G * bs, game.width, f16)
    ps = game.search(G, bs, dirichlet_alpha=alpha, dirichlet_eps=eps, seed=SEED)
    sno = _set_search_numbers(ps)
    mv, na, st = ps.run(game.roots(pos), sims, _host_net(logits))
    assert (st[:, 5] == 0).all()
    check_noise(game, ps.prior.cpu().numpy(), pos, _root_rows(logits, G, bs), alpha, eps, sno,
                what=f"alpha={alpha} eps={eps} {'f16' if f16 else 'f32'}")
    assert ps.search_no.cpu().numpy().tolist() == (sno + 1).tolist()


@pytest.mark.parametrize("T", [0.25, 0.5, 1.0, 1.7, 2.0])
@pytest.mark.parametrize("name", ["chess", "c4"])
def test_temperature_sample_replays_the_specification(games, name, T):
    game, bs, sims = games[name], 16, 129
    pos = game.positions(G)
    logits = _logits(G * bs, game.width, False)
    ps = game.search(G, bs, seed=SEED)
    sno = _set_search_numbers(ps)
    mv, na, st = ps.run(game.roots(pos), sims, _host_net(logits), temperature=T)
    assert (st[:, 5] == 0).all()
    mv, na = mv.cpu().numpy(), na.cpu().numpy()
    check_sample(game, mv, na, pos, T, sno, exact=T in (0.25, 0.5, 1.0), visits=sims - 1)
    na_l, _ = _listed(game, na, pos)
    assert all(na_l[i, game.index_of(mv[i], p)] > 0 for i, p in enumerate(pos))


@pytest.mark.parametrize("mode", ["plain", "first_game", "split", "graph"])
@pytest.mark.parametrize("name", ["chess", "c4"])
def test_counter_words_through_every_launch_path(games, name, mode):
    """Distinct search numbers per game; a search over games [5, 5 + n) of the engine; two parts
    on two streams (the second part's launches index search_no from their own first game); a
    captured graph replayed twice (searches sno and sno + 1)."""
    game, n, bs, sims, alpha, eps, T = games[name], 128, 16, 65, 0.3, 0.25, 1.0
    pos = game.positions(n)
    roots = game.roots(pos)
    logits = _logits(G * bs, game.width, True)[:n * bs]
    rows = _root_rows(logits, n, bs)
    ps = game.search(n, bs, dirichlet_alpha=alpha, dirichlet_eps=eps, seed=SEED)
    sno = _set_search_numbers(ps)
    first = 5 if mode == "first_game" else 0
    fn = [_device_net(logits, 0, n // 2 * bs), _device_net(logits, n // 2 * bs, n * bs)] if mode == "split" \
        else _device_net(logits)
    if mode == "graph":
        g = ps.capture(roots, sims, fn, temperature=T)
        assert ps.search_no.cpu().numpy().tolist() == sno.tolist()   # capturing runs no search
        replays = 2
    else:
        replays = 1
    for r in range(replays):
        if mode == "graph":
            g.replay()
            torch.cuda.synchronize()
        else:
            ps.run(roots, sims, fn, temperature=T, first_game=first)
        assert (ps.stats[:, 5] == 0).all()
        check_noise(game, ps.prior.cpu().numpy(), pos, rows, alpha, eps, sno + r, first=first, what=f"{mode} {r}")
        check_sample(game, ps.move.cpu().numpy(), ps.na.cpu().numpy(), pos, T, sno + r, first=first,
                     visits=sims - 1, what=f"{mode} {r}")
    assert ps.search_no.cpu().numpy().tolist() == (sno + replays).tolist()


def test_c4_kept_root_takes_the_next_search_numbers_noise(games):
    """C4PuctSearch(reuse=True), two consecutive searches: the second one's root is the first
    one's chosen child; its kept priors take the noise of the game's next search number, and
    the sample runs over the kept visits plus the new ones."""
    game, n, bs, sims, alpha, eps, T = games["c4"], 64, 16, 129, 0.3, 0.25, 1.0
    eng = game.eng
    pos = game.positions(n)
    logits = _logits(G * bs, 7, False)[:n * bs]
    rows = _root_rows(logits, n, bs)
    ps = game.search(n, bs, dirichlet_alpha=alpha, dirichlet_eps=eps, seed=SEED, reuse=True)
    sno = _set_search_numbers(ps)
    mv, na, st = ps.run(game.roots(pos), sims, _host_net(logits), temperature=T)
    assert (st[:, 5] == 0).all() and (ps.kept == 0).all()
    mv = mv.cpu().numpy()
    check_noise(game, ps.prior.cpu().numpy(), pos, rows, alpha, eps, sno, what="fresh")
    check_sample(game, mv, na.cpu().numpy(), pos, T, sno, visits=sims - 1, what="fresh")
    nxt, kept_pr, kept_na = [], np.zeros((n, 7)), np.zeros(n, dtype=np.int64)
    for i, p in enumerate(pos):
        d = eng.debug_c4_puct_tree(i)
        c = int(d["child"][0][game.index_of(mv[i], p)])
        assert c != 0xFFFF and int(d["evaluated"][c]) and int(d["nmoves"][c]) > 0
        q = oracle.play(p[0], p[1], int(mv[i]))
        nxt.append(q)
        k = int(d["nmoves"][c])
        assert [(int(d["order"][c]) >> (3 * s)) & 7 for s in range(k)] == game.cols(q)
        kept_pr[i, :k] = d["pr"][c][:k]
        kept_na[i] = int(d["na"][c][:k].sum())
    mv2, na2, st2 = ps.run(game.roots(nxt), sims, _host_net(logits), temperature=T)
    assert (st2[:, 5] == 0).all() and (ps.kept.cpu().numpy() > 0).all()
    assert ps.search_no.cpu().numpy().tolist() == (sno + 2).tolist()
    check_noise(game, ps.prior.cpu().numpy(), nxt, rows, alpha, eps, sno + 1, sm=kept_pr, what="kept root")
    na2 = na2.cpu().numpy()
    assert (na2.sum(axis=1) == kept_na + sims - 1).all()
    check_sample(game, mv2.cpu().numpy(), na2, nxt, T, sno + 1, what="kept root")


def test_low_temperature_is_the_argmax():
    """T = 0.01 on root counts above 1210: unscaled, 1210^100 overflows a double, the total and
    the target are inf, no running sum exceeds the target and the kernel returns the last move
    of the list whatever the visits.  With the scaled weights the move is the most visited."""
    n, bs, sims, T = 8, 16, 2049, 0.01
    game = C4(max_games=n, max_sims=2100)
    try:
        pos = [("." * 42, 0)] * n
        logits = _logits(n * bs, 7, False).clone()
        logits[:, 2] = 8.0   # column 2: in no game the last move of the list
        assert all(game.cols(p)[-1] != 2 for p in pos)
        # c_puct 4 and values in (-0.1, 0.1): the prior, not the hash values, decides the visits
        ps = game.search(n, bs, c_puct=4.0, seed=SEED)
        sno = _set_search_numbers(ps)
        net = lambda leaves, planes, counts: (_values(leaves) * 0.1, logits)  # noqa: E731
        mv, na, st = ps.run(game.roots(pos), sims, net, temperature=T)
        mv, na = mv.cpu().numpy(), na.cpu().numpy()
        assert (st[:, 5] == 0).all() and (na.sum(axis=1) == sims - 1).all()
        assert (na.max(axis=1) > 1210).all(), na.max(axis=1)
        # no runner-up within reach: the other moves' weights together stay below 2^-25 of the
        # top one's, the smallest value of the uniform
        second = np.sort(na, axis=1)[:, -2]
        assert ((second / na.max(axis=1)) ** 100 * 7 < 2.0 ** -25).all()
        assert mv.tolist() == na.argmax(axis=1).tolist() == [2] * n
        check_sample(game, mv, na, pos, T, sno, visits=sims - 1, what="low")
    finally:
        game.eng.close()
