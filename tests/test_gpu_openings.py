"""A book of openings on the device: zc_traj_openings_async against tests/traj_openings_ref.py on
scripted tables, then the self-play pools and the arenas with openings= against the same pools
without it, seeded by the test in torch (tests/openings_ref.py) — the same games bit for bit,
every game's first row its opening."""
import ctypes

import numpy as np
import pytest
import torch

import arena_ref
import openings_ref
import oracle
import test_gpu_traj_scripted as scripted
import traj_ref as tr
from arena_nets import integer_net, integer_pv_net
from traj_openings_ref import OpeningsModel, opening_of
from zeroclone_amd import _native
from zeroclone_amd.arena import ArenaResult, C4Arena, ChessArena
from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
SIMS, BS = 32, 8


def same_games(got, want):
    for name, x, y in zip(("rows", "labels", "moves", "games"), got, want):
        assert torch.equal(x, y), name


# ------------------------------------------------------------------ 1. the kernel against the model
def book_rows(n: int, words: int) -> list[tuple]:
    return [tuple(0x2222000000000000 + (r + 1) * 0x100 + w for w in range(words)) for r in range(n)]


class SeededDev(scripted.Dev):
    """test_gpu_traj_scripted's hand-built recorder with a book and the roots beside it, both
    between guard rows."""

    def __init__(self, c, book, share):
        super().__init__(c)
        self.share = share
        self.big["book"], self.book = scripted.guarded(len(book), c.words, torch.int64)
        self.book[:] = torch.tensor(book, dtype=torch.int64)
        self.sent_book = self.book.clone()
        self.big["roots"], self.roots = scripted.guarded(c.n, c.words, torch.int64)
        self.roots[:] = self.init[0]

    def seed(self):
        _native.check(self.lib.zc_traj_openings_async(self.c.n, ctypes.byref(self.buf), VP(self.book.data_ptr()),
                                                      self.book.shape[0], self.share, VP(self.roots.data_ptr()),
                                                      self.stream))
        torch.cuda.synchronize()

    def check_seeded(self, m, roots):
        self.check(m)
        assert [tuple(r) for r in self.roots.tolist()] == roots, "d_roots"
        assert torch.equal(self.book, self.sent_book), "the book was written"


def run_seeded(n, words, lengths, steps, n_book, share, quota=None, max_len=6):
    chess = words == 9
    t = tr.scripted(n, steps, 8 * words, lengths, chess=chess)
    c = scripted.Cfg(n, words, max_len, 3 * n * steps + 8, n * steps + 4, quota=quota)
    book = book_rows(n_book, words)
    m = OpeningsModel(n, tr.init_row(words), max_len, c.pool_cap, c.games_cap, quota, book=book, share=share)
    d = SeededDev(c, book, share)
    roots = m.seed(m.start_roots())
    d.seed()
    d.check_seeded(m, roots)
    for k in range(steps):
        left = d.single(t, k, k + 1, chess=chess)
        d.roots.copy_(left["states"][0])           # what the play kernel leaves: d_init where the record restarted
        d.seed()
        states = [tuple(int(x) for x in r) for r in t["states"][k]]
        kw = dict(flags=t["flags"][k], rep=t["rep"][k]) if chess else {}
        m.step_seeded(states, t["moves"][k], [int(x) for x in t["results"][k]], roots, **kw)
        d.check_seeded(m, roots)
    d.seed()                                       # once more: nothing changes
    d.check_seeded(m, roots)
    assert m.overflow == 0
    for rec in m.games:
        if rec:
            assert m.pool[rec[3]] == book[opening_of(rec[0], n_book, share)]
    return m


@pytest.mark.parametrize("share", [1, 2])
@pytest.mark.parametrize("n_book", [1, 3])
@pytest.mark.parametrize("row_bytes", [24, 72])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_kernel_against_the_model(n, row_bytes, n_book, share):
    steps = 4
    lengths = [[2 + (g * 7 // 3 + i) % 3 for i in range(8)] for g in range(n)]   # 2, 3 and 4 mixed along the slots
    m = run_seeded(n, row_bytes // 8, lengths, steps, n_book, share)
    assert m.finished >= n


@pytest.mark.parametrize("share", [1, 2])
@pytest.mark.parametrize("quota,n_book", [(3, 3), (6, 3), (7, 1), (5, 8), (0, 3)])
def test_kernel_under_a_quota(quota, n_book, share):
    """Five slots.  Quota 3: two slots idle from the start; 6: the quota runs out inside the step in
    which all five finish; 5 with 8 rows: a book larger than the quota; 0: every slot idle."""
    m = run_seeded(5, 3, [[2, 2, 3], [2, 3, 2], [2, 2, 2], [2, 4], [2, 2, 2]], 6, n_book, share, quota=quota)
    assert m.finished == quota and all(s == [1, -1] for s in m.slot)


def test_openings_call_refuses_bad_arguments():
    c = scripted.Cfg(3, 3, 4, 20, 8)
    d = SeededDev(c, book_rows(2, 3), 1)
    lib = d.lib

    def call(n=3, buf=d.buf, book=d.book.data_ptr(), rows=2, share=1, roots=d.roots.data_ptr()):
        return lib.zc_traj_openings_async(n, ctypes.byref(buf) if buf is not None else None, VP(book), rows, share,
                                          VP(roots), d.stream)
    bad = _native.TrajBuffers.from_buffer_copy(d.buf)
    bad.d_hist = 0
    for rc in (call(book=None), call(roots=None), call(book=d.book.data_ptr() + 4), call(roots=d.roots.data_ptr() + 4),
               call(rows=0), call(rows=-1), call(share=0), call(share=-3), call(n=-1), call(buf=None), call(buf=bad)):
        assert rc == _native.ZC_EINVAL
    assert call(n=0) == 0
    torch.cuda.synchronize()
    m = OpeningsModel(3, tr.init_row(3), 4, 20, 8, book=book_rows(2, 3))
    d.check_seeded(m, m.start_roots())              # the refused and the empty calls wrote nothing


# ------------------------------------------------------------------ 2. the Connect4 pool
def c4_row(cols: str) -> list[int]:
    stones, height = [0, 0], [0] * 7
    for i, ch in enumerate(cols):
        c = int(ch)
        stones[i & 1] |= 1 << (7 * c + height[c])
        height[c] += 1
    return [stones[0], stones[1], len(cols) & 1]


C4_BOOK = torch.tensor([c4_row("33"), c4_row("3"), c4_row("3342")], dtype=torch.int64)   # one at an odd ply
C4_BOOK4 = torch.cat([C4_BOOK, torch.tensor([c4_row("2")])])
_nets = {}


def net(kind, seed):
    if (kind, seed) not in _nets:
        _nets[kind, seed] = (integer_net(2, seed) if kind == "c4_value" else integer_pv_net(2, 6, 7, 7, seed)
                             if kind == "c4_puct" else integer_net(17, seed))
    return _nets[kind, seed]


def c4_pool_kw(mode):
    if mode == "value":
        return dict(net=net("c4_value", 5))
    return dict(puct_net=net("c4_puct", 5), reuse_tree=True, record_policy=True, temperature=1.0)


def policy(pool):
    b = pool.last_batch
    return (b.pi_off.cpu(), b.pi.cpu()) if b.pi is not None else ()


@pytest.mark.parametrize("mode", ["value", "puct-reuse-policy"])
def test_c4_pool_with_a_book(mode):
    kw = dict(batch_size=BS, seed=3, **c4_pool_kw(mode))
    pool = C4SelfPlay(8, SIMS, openings=C4_BOOK, **kw)
    ref = C4SelfPlay(8, SIMS, **kw)
    kept_fresh = []

    def on_search(p, fresh):           # a game's first search starts afresh: nothing kept
        if p.ps is not None and p.ps.kept is not None:
            kept_fresh.append(p.ps.kept[fresh].clone())
    got = openings_ref.play(pool, 20, on_search=on_search)
    want = openings_ref.play(ref, 20, after_step=lambda p: openings_ref.seed(p, C4_BOOK, 1))
    same_games(got, want)
    for x, y in zip(policy(pool), policy(ref)):
        assert torch.equal(x, y)
    games = got[3]
    assert games[:, 0].tolist() == list(range(20))
    assert torch.equal(openings_ref.first_rows(got), C4_BOOK[games[:, 0] % 3])
    if mode != "value":
        kept = torch.cat(kept_fresh)
        assert kept.numel() >= 20 and int(kept.abs().sum()) == 0
        assert pool.last_batch.pi is not None
    pool.check()
    # an idle slot (quota spent) is held at the empty board
    idle = pool.traj.slot[:, 1] < 0
    assert bool(idle.all()) and int(pool.roots.abs().sum()) == 0
    pool.close()
    ref.close()


def _deep_row(cls, kw, root_row):
    """Four games at `root_row`, one step without noise at temperature 0: the position every game
    is at afterwards, one ply below the searched root and inside its tree."""
    probe = cls(4, SIMS, **kw)
    _put(probe, root_row)
    probe.step()
    row = probe.roots[:1].cpu().clone()
    assert bool((probe.results == 2).all()) and bool((probe.roots == probe.roots[:1]).all())
    probe.close()
    return row


def _put(pool, root_row):
    """Every slot in the middle of a game (two positions recorded) at `root_row`."""
    pool.roots.copy_(root_row.to(pool.dev).expand_as(pool.roots))
    pool.traj.slot[:, 0] = 2


@pytest.mark.parametrize("game", ["c4", "chess"])
def test_a_refilled_slot_drops_its_tree_though_its_opening_lies_below_the_old_root(game):
    """A book row one ply below a game's last searched root (Connect4: 7 stones under a root of
    6).  Slots 0 and 1 go on with their game and re-root into the kept tree; slots 2 and 3 are
    refilled, take the same position from the book, and must start afresh: kept == 0.  Without
    the forget in the pool's seeding step the re-root, which goes by position equality alone,
    keeps the old game's subtree in all four."""
    if game == "c4":
        cls, root = C4SelfPlay, torch.tensor([c4_row("303142")], dtype=torch.int64)
        kw = dict(batch_size=BS, seed=3, puct_net=net("c4_puct", 5), temperature=0.0,
                  puct_args=dict(dirichlet_eps=0.0))
    else:
        cls = ChessSelfPlay
        root = torch.from_numpy(np.frombuffer(_native.chess_from_fen("8/8/4k3/8/8/8/3QK3/8 w - - 0 1").tobytes(),
                                              np.uint8).reshape(1, 72).copy())
        kw = dict(batch_size=BS, seed=5, puct_net=integer_pv_net(17, 8, 8, 4096, 5, "conv"), temperature=0.0,
                  puct_args=dict(dirichlet_eps=0.0), hist_cap=16)
    deep = _deep_row(cls, kw, root)
    if game == "c4":
        assert bin(int(deep[0, 0])).count("1") + bin(int(deep[0, 1])).count("1") == 7
    pool = cls(4, SIMS, reuse_tree=True, openings=deep, **kw)
    _put(pool, root)
    pool.step()                                          # every game now stands at the deep row, its tree kept
    assert torch.equal(pool.roots.cpu(), deep.expand(4, -1)) and int(pool.ps.kept.abs().sum()) == 0
    pool.traj.slot[2:, 0] = 1                            # as the record leaves a refilled slot
    pool.roots[2:] = 0
    pool._seed_openings(pool._stream(None))
    assert torch.equal(pool.roots.cpu(), deep.expand(4, -1))
    pool.step_search()
    kept = pool.ps.kept.cpu().tolist()
    assert kept[0] > 0 and kept[1] > 0, "the games in progress kept nothing: the case shows nothing"
    assert kept[2:] == [0, 0]
    pool.close()


def test_c4_pool_with_a_book_replays_from_a_graph():
    """The same pool stepped and replayed from its captured step: the same roots, histories and
    pooled games (the unlimited quota: a graph's case), past the first refills."""
    kw = dict(batch_size=BS, seed=3, net=net("c4_value", 5), openings=C4_BOOK)
    a, b = C4SelfPlay(8, SIMS, **kw), C4SelfPlay(8, SIMS, **kw)
    assert torch.equal(a.roots.cpu(), C4_BOOK[torch.arange(8) % 3])       # seeded at construction
    g = b.capture_step()
    for _ in range(40):
        a.step()
        g.replay()
    torch.cuda.synchronize()
    for name in ("hist", "hmoves", "slot", "ctl", "pool", "labels", "pool_moves", "games"):
        assert torch.equal(getattr(a.traj, name), getattr(b.traj, name)), name
    assert torch.equal(a.roots, b.roots)
    ba, bb = a.take(), b.take()
    assert ba.games.shape[0] >= 4, "no game finished: play more steps"
    assert torch.equal(ba.rows, bb.rows) and torch.equal(ba.games, bb.games)
    assert torch.equal(ba.rows[ba.games[:, 3]].cpu(), C4_BOOK[ba.games[:, 0].cpu() % 3])
    a.close()
    b.close()


def test_c4_pool_adopts_games_by_their_numbers_and_takes_a_network():
    """adopt(): the slots go on by their game numbers; set_network: the book stays."""
    from zeroclone_amd.nets import ValueNetwork
    kw = dict(batch_size=BS, seed=3, openings=C4_BOOK)
    a = C4SelfPlay(8, SIMS, net=net("c4_value", 5), **kw)
    for _ in range(12):
        a.step()
    b = C4SelfPlay(8, SIMS, net=net("c4_value", 6), **kw)
    b.adopt(a)
    torch.manual_seed(0)
    b.set_network(ValueNetwork(128, 2, in_planes=2))
    for _ in range(45):
        b.step()
    batch = b.take()
    assert batch.games.shape[0] >= 8 and int(batch.games[:, 0].max()) >= 8
    assert torch.equal(batch.rows[batch.games[:, 3]].cpu(), C4_BOOK[batch.games[:, 0].cpu() % 3])
    a.close()
    b.close()


def test_c4_pool_refuses_a_bad_row_on_the_device():
    bad = C4_BOOK.clone().cuda()
    bad[1, 0] |= 1 << 23            # a stone in the air: column 3, two above its only stone
    with pytest.raises(ValueError, match="row 1: a gap"):
        C4SelfPlay(8, SIMS, openings=bad)


# ------------------------------------------------------------------ 3. the chess pool
# The engine's fifty-move rule (check_draw) ends a game when the counter reaches 50 plies, so these
# clocks leave three, two and one plies; a capture of the rook leaves king against king, where
# the move generator has no move: a draw as well.
FENS = ["8/8/4k3/8/8/8/R3K3/8 w - - 47 60", "8/8/4k3/8/8/8/R3K3/8 b - - 48 60", "4k3/8/8/8/8/8/3QK3/8 w - - 49 70"]
HIST_CAP = 4     # moves per side: a game has at most 3


def _longest_line(s, d=0):
    if oracle.chess_win(s) or oracle.chess_draw(s):
        return d
    moves = oracle.chess_moves(s)
    assert moves
    return max(_longest_line(oracle.chess_play(s, m), d + 1) for m in moves)


def chess_book():
    rows = np.stack([np.frombuffer(_native.chess_from_fen(f).tobytes(), np.uint8) for f in FENS])
    return torch.from_numpy(rows.copy())


def test_chess_pool_with_a_book():
    for f in FENS:                    # legal, not finished, and every line ends inside the histories
        s = oracle.chess_from_fen(f)
        assert oracle.chess_moves(s) and not oracle.chess_win(s) and not oracle.chess_draw(s)
        assert 1 <= _longest_line(s) <= 3 < 2 * HIST_CAP
    assert oracle.chess_from_fen(FENS[1]).turn == 1
    kw = dict(batch_size=BS, seed=5, hist_cap=HIST_CAP)
    pool = ChessSelfPlay(4, 16, openings=FENS, **kw)
    ref = ChessSelfPlay(4, 16, **kw)
    book = chess_book()
    assert torch.equal(pool.roots.cpu(), book[torch.arange(4) % 3])
    got = openings_ref.play(pool, 6)
    want = openings_ref.play(ref, 6, after_step=lambda p: openings_ref.seed(p, book, 1))
    same_games(got, want)
    games = got[3]
    assert games[:, 0].tolist() == list(range(6)) and int(games[:, 4].max()) <= 4
    assert torch.equal(openings_ref.first_rows(got), book.view(torch.int64)[games[:, 0] % 3])
    assert set(games[:, 2].tolist()) == {0}          # the fifty-move rule: draws
    pool.check()
    assert bool((pool.traj.slot[:, 1] < 0).all()) and torch.equal(pool.roots, ref.roots)   # idle slots: as without a book
    pool.close()
    ref.close()
    tensor_pool = ChessSelfPlay(4, 16, openings=book, **kw)                   # the tensor form of the same book
    same_games(openings_ref.play(tensor_pool, 6), got)
    tensor_pool.close()


@pytest.mark.parametrize("fen,why", [("8/8/4k3/8/8/8/R3K3/8 w - - 50 60", "fifty"),
                                     ("7k/5Q2/6K1/8/8/8/8/8 b - - 0 1", "no legal move"),
                                     ("7k/6Q1/6K1/8/8/8/8/8 b - - 0 1", "mated")])
def test_chess_pool_refuses_a_finished_opening(fen, why):
    with pytest.raises(ValueError, match=rf"row 1 .*{why}"):
        ChessSelfPlay(4, 16, openings=[FENS[0], fen, FENS[1]], hist_cap=HIST_CAP)


# ------------------------------------------------------------------ 4. the arenas
ENTRIES = 1 << 16
_arena_games = {}


def c4_arena(a, b, **kw):
    return C4Arena(8, SIMS, batch_size=BS, seed=3, net_a=a, net_b=b, openings=C4_BOOK4, **kw)


def plain_arena_games():
    """The plain arena with the book, networks 5 against 6, 16 games: played once."""
    if "ab" not in _arena_games:
        arena = c4_arena(net("c4_value", 5), net("c4_value", 6))
        res = arena.play(16, max_steps=2000)
        b = arena.last_batch
        _arena_games["ab"] = ((b.rows.cpu(), b.labels.cpu(), b.moves.cpu(), b.games.cpu()), res, arena.mixed_steps)
        arena.check()
        arena.close()
    return _arena_games["ab"]


def mirrored(r: ArenaResult) -> ArenaResult:
    """The same games with the networks' names swapped: A's games as the first mover are B's,
    wins and losses change places."""
    return ArenaResult(tuple(reversed(r.second)), tuple(reversed(r.first)))


def test_c4_arena_with_a_book_equals_the_reference_arena():
    got, res, mixed = plain_arena_games()
    a, b = net("c4_value", 5), net("c4_value", 6)
    ref = arena_ref.reference_arena("c4", 8, SIMS, a, b, False, batch_size=BS, seed=3)
    want = openings_ref.play(ref, 16, after_step=lambda p: openings_ref.seed(p, C4_BOOK4, 2))
    ref.close()
    same_games(got, want)
    games = got[3]
    assert games[:, 0].tolist() == list(range(16))
    assert torch.equal(openings_ref.first_rows(got), C4_BOOK4[(games[:, 0] // 2) % 4])   # 2k and 2k + 1: book[k % 4]
    assert res == ArenaResult.tally(games[:, 2].tolist(), games[:, 0].tolist()) and res.games == 16
    assert sum(res.first) == 8 and sum(res.second) == 8 and mixed > 0
    # the pairs differ: not the two games an arena without a book plays over and over
    moves = {tuple(got[2][o:o + n].tolist()) for _, _, _, o, n in games.tolist()}
    assert len(moves) > 4


def test_cached_c4_arena_with_a_book_stepped_and_captured():
    want, res, _ = plain_arena_games()
    a, b = net("c4_value", 5), net("c4_value", 6)
    arena = c4_arena(a, b, eval_cache=ENTRIES, eval_merge=True)
    assert arena.play(16, max_steps=2000) == res
    bt = arena.last_batch
    same_games((bt.rows.cpu(), bt.labels.cpu(), bt.moves.cpu(), bt.games.cpu()), want)
    # No cross-network hit: the two networks differ, so a value served from the other network's table
    # would change a search, and the games above are the plain arena's bit for bit.  The counters
    # below only show that both tables were in use and account for every row they were asked for.
    for s in arena.eval_cache_stats(by_network=True):
        assert s["probed"] == s["hits"] + s["merged"] + s["inserts"] + s["dropped"] and s["probed"] > 0
    arena.close()
    # the captured step against the stepped one, both new arenas without a quota
    arena, twin = (c4_arena(a, b, eval_cache=ENTRIES, eval_merge=True) for _ in range(2))
    g = arena.capture_step()
    for _ in range(20):
        twin.step()
        g.replay()
    torch.cuda.synchronize()
    for name in ("hist", "hmoves", "slot", "ctl", "pool", "labels", "pool_moves", "games"):
        assert torch.equal(getattr(arena.traj, name), getattr(twin.traj, name)), name
    assert torch.equal(arena.roots, twin.roots)
    bt = twin.take()
    assert bt.games.shape[0] >= 4, "no game finished: play more steps"
    assert torch.equal(bt.rows[bt.games[:, 3]].cpu(), C4_BOOK4[(bt.games[:, 0].cpu() // 2) % 4])
    arena.close()
    twin.close()


@pytest.mark.parametrize("cached", [False, True], ids=["plain", "cached"])
def test_set_networks_swaps_the_colours(cached):
    _, res, _ = plain_arena_games()
    a, b = net("c4_value", 5), net("c4_value", 6)
    kw = dict(eval_cache=ENTRIES, eval_merge=True) if cached else {}
    arena = c4_arena(a, b, **kw)
    assert arena.play(16, max_steps=2000) == res
    before = arena.eval_cache_stats(by_network=True) if cached else None
    arena.set_networks(b, a)
    if cached:   # both tables empty: the 64-byte header and every entry's meta word (0 = empty) are zero, so
        # no entry of the old networks is left to serve the new ones
        torch.cuda.synchronize()
        cache = arena._caches[0]
        meta = 64 + 4 * _native.EVALCACHE_WAYS * cache.sets
        assert len(cache.tables) == 2 and all(int(t[:meta].count_nonzero()) == 0 for t in cache.tables)
        assert all(int(t[meta:].count_nonzero()) > 0 for t in cache.tables)   # they were in use
    swapped = arena.play(16, max_steps=2000)
    assert swapped == mirrored(res) and swapped.score == 1.0 - res.score
    if cached:   # the counters go on counting, by the rows a new arena of (b, a) probes; both tables hit again
        fresh = c4_arena(b, a, **kw)
        assert fresh.play(16, max_steps=2000) == swapped
        after, alone = arena.eval_cache_stats(by_network=True), fresh.eval_cache_stats(by_network=True)
        for x, y, z in zip(before, after, alone):
            assert y["probed"] - x["probed"] == z["probed"] > 0 and y["hits"] > x["hits"]
        fresh.close()
    with pytest.raises(ValueError, match="value search"):
        arena.set_networks(net("c4_puct", 5), net("c4_puct", 6))
    arena.close()


def test_set_networks_swaps_the_colours_across_widths():
    """The cached arena handed a 64-channel network against a 128-channel one, then the same two
    with the names swapped: the first pair plays the plain arena's games of that pair, the second
    the mirrored result.  After each call both tables are empty (the header and every meta word
    zero), so the counters of the games that follow are those of tables filled from nothing: the
    rows a new arena of that pair probes, and new inserts in both."""
    x64, y128 = integer_net(2, 5, 64), net("c4_value", 6)
    assert (x64.channels, y128.channels) == (64, 128)
    kw = dict(eval_cache=ENTRIES, eval_merge=True)
    arena = c4_arena(net("c4_value", 5), y128, **kw)

    def empty_tables():
        torch.cuda.synchronize()
        cache = arena._caches[0]
        meta = 64 + 4 * _native.EVALCACHE_WAYS * cache.sets
        return len(cache.tables) == 2 and all(int(t[:meta].count_nonzero()) == 0 for t in cache.tables)

    def used_tables():
        cache = arena._caches[0]
        meta = 64 + 4 * _native.EVALCACHE_WAYS * cache.sets
        return all(int(t[:meta].count_nonzero()) > 0 for t in cache.tables)

    results = []
    for pair in ((x64, y128), (y128, x64)):
        arena.set_networks(*pair)
        assert empty_tables()
        assert [n.channels for n in arena.routed.nets] == [n.channels for n in pair]
        before = arena.eval_cache_stats(by_network=True)
        results.append(arena.play(16, max_steps=2000))
        assert used_tables()
        bt = arena.last_batch
        games = (bt.rows.cpu(), bt.labels.cpu(), bt.moves.cpu(), bt.games.cpu())
        after = arena.eval_cache_stats(by_network=True)
        fresh = c4_arena(*pair) if pair[0] is x64 else c4_arena(*pair, **kw)
        assert fresh.play(16, max_steps=2000) == results[-1]
        fb = fresh.last_batch
        same_games(games, (fb.rows.cpu(), fb.labels.cpu(), fb.moves.cpu(), fb.games.cpu()))
        if pair[0] is not x64:   # the counters against a new cached arena's, which start at zero
            for x, y, z in zip(before, after, fresh.eval_cache_stats(by_network=True)):
                assert y["probed"] - x["probed"] == z["probed"] > 0
        for x, y in zip(before, after):
            assert y["probed"] > x["probed"] and y["inserts"] > x["inserts"] and y["hits"] > x["hits"]
        fresh.check()
        fresh.close()
    assert results[1] == mirrored(results[0]) and results[1].score == 1.0 - results[0].score
    arena.check()
    arena.close()


def test_chess_arena_with_a_book():
    a, b = net("chess_value", 5), net("chess_value", 6)
    kw = dict(batch_size=BS, seed=5, hist_cap=HIST_CAP)
    arena = ChessArena(4, 16, net_a=a, net_b=b, openings=FENS, **kw)
    res = arena.play(4, max_steps=200)
    bt = arena.last_batch
    got = (bt.rows.cpu(), bt.labels.cpu(), bt.moves.cpu(), bt.games.cpu())
    ref = arena_ref.reference_arena("chess", 4, 16, a, b, False, **kw)
    book = chess_book()
    same_games(got, openings_ref.play(ref, 4, after_step=lambda p: openings_ref.seed(p, book, 2)))
    assert torch.equal(openings_ref.first_rows(got), book.view(torch.int64)[[0, 0, 1, 1]])
    assert res.games == 4 and res.score == 0.5
    arena.check()
    arena.close()
    ref.close()
