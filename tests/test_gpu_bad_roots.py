"""Roots that no game produces, through every Connect4 search and self-play entry point: 8 games,
32 simulations, batch 8 (one self-play case at batch 64 x 64 simulations, the kernel instance
without the planned flush).

Every launch holds good and bad roots together, flagged ones at row 0, inside the workgroup and
at the last row.  Outputs are pre-filled with a pattern.  The expected status comes from a plain
restatement of the rules (expected_status below), the good games' outputs from a twin engine with
the same seeds that runs the same launch with valid roots in the flagged rows: games are
independent, so the good games' moves, visit rows, stats and MT19937 states must match bit for
bit, and a flagged game must have consumed no random word.

Pinned as they are: an already-won root with free columns is searched by the rollout and value
searches (status 0) and is ZC_STATUS_NO_MOVES for PUCT."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from c4_raw_pool import (BAD_STATE, FILL32, FILL64, NO_MOVES, SKIP, RawPool, c4_rows, raw_state)
from zeroclone_amd import _native

pytestmark = pytest.mark.gpu

N, SIMS, BS, C, MOVES = 8, 32, 8, 1.4, 3
SEEDS = [31 * g + 5 for g in range(N)]
FULL = sum(0x3F << (7 * c) for c in range(7))
M64 = (1 << 64) - 1


def has_four(b):
    return any(b & (b >> d) & (b >> 2 * d) & (b >> 3 * d) for d in (1, 6, 7, 8))


def expected_status(s0, s1, turn):
    """include/zeroclone.h: stones inside the 42 cells, no overlap, stacked from the bottom,
    turn 0 or 1 — else BAD_STATE; a valid board without a free column: NO_MOVES."""
    occ = s0 | s1
    if (s0 & s1) or (occ & ~FULL & M64) or turn not in (0, 1):
        return BAD_STATE
    for c in range(7):
        col = (occ >> (7 * c)) & 0x3F
        if col & (col + 1):
            return BAD_STATE
    return NO_MOVES if occ == FULL else 0


def _played(cols, reserved=0):
    b, t = "." * 42, 0
    for col in cols:
        b, t = oracle.play(b, t, col)
    s = _native.c4_from_rows(b, t)
    return raw_state(int(s["stones"][0]), int(s["stones"][1]), int(s["turn"]), reserved)


def _full_board():
    """42 stones, no four in a row: cell (column c, height h) is O's where (c + h // 2) is odd."""
    s = [0, 0]
    for c in range(7):
        for h in range(6):
            s[(c + h // 2) & 1] |= 1 << (7 * c + h)
    assert s[0] | s[1] == FULL and not has_four(s[0]) and not has_four(s[1])
    return raw_state(s[0], s[1], 0)


RESERVED_COLS = [3, 3, 2, 4, 1]
CASES = {
    "overlap": raw_state(1, 1, 0),
    "sentinel": raw_state(1 << 6, 0, 1),             # column 0's sentinel bit
    "above48": raw_state(1, 1 << 55, 0),             # past the seven columns
    "floating": raw_state(1 << 15, 0, 1),            # column 2, height 1, nothing under it
    "turn2": raw_state(0, 0, 2),
    "turn_neg": raw_state(0, 0, -1),
    "full": _full_board(),
    "won": _played([3, 2, 3, 2, 3, 2, 3]),           # X has four in column 3; six columns free
    "reserved": _played(RESERVED_COLS, reserved=0x7777),
    "empty": _played([]),
    "mid1": _played([3, 3, 2, 4]),
    "mid2": _played([0, 0, 0, 0, 0, 0, 1, 2]),       # column 0 full
    "mid3": _played([1, 1, 2, 2, 4, 4, 5, 6, 6, 5, 0]),
}
LAYOUTS = {
    "A": ["overlap", "mid1", "sentinel", "reserved", "above48", "won", "mid2", "floating"],
    "B": ["turn2", "mid2", "full", "empty", "turn_neg", "won", "mid1", "full"],
}


def _fields(s):
    return int(s["stones"][0]), int(s["stones"][1]), int(s["turn"])


class Layout:
    """The launch's roots, the twin's (valid roots in the flagged rows, reserved = 0 everywhere)
    and the status each row must report; puct: a won root has no moves there."""

    def __init__(self, name, puct=False):
        names = LAYOUTS[name]
        self.exp = []
        for k in names:
            s0, s1, t = _fields(CASES[k])
            st = expected_status(s0, s1, t)
            if puct and not st and (has_four(s0) or has_four(s1)):
                st = NO_MOVES
            self.exp.append(st)
        assert self.exp[0] and self.exp[-1] and any(self.exp[1:-1]) and not all(self.exp)
        assert {BAD_STATE, NO_MOVES} <= set(self.exp) or name == "A"
        self.roots = np.array([CASES[k] for k in names], _native.C4_STATE_DTYPE)
        self.twin = np.array([CASES["mid3"] if e else _played(RESERVED_COLS) if k == "reserved" else CASES[k]
                              for k, e in zip(names, self.exp)], _native.C4_STATE_DTYPE)
        self.bad = [i for i, e in enumerate(self.exp) if e]
        self.good = [i for i, e in enumerate(self.exp) if not e]


def test_the_root_cases_are_what_they_claim():
    want = dict(overlap=2, sentinel=2, above48=2, floating=2, turn2=2, turn_neg=2, full=1)
    for k, s in CASES.items():
        assert expected_status(*_fields(s)) == want.get(k, 0), k
    s0, s1, _ = _fields(CASES["won"])
    assert has_four(s0) and not has_four(s1) and (s0 | s1) != FULL


def pools(max_batch=16, steps=MOVES):
    return (RawPool(N, 128, max_batch, SEEDS, steps), RawPool(N, 128, max_batch, SEEDS, steps))


def assert_rows(lay, got, ref):
    """got / ref: (move [n], visits [n, 7], stats [n, 8]) of the launch and of the twin's."""
    mv, na, st = (np.asarray(x) for x in got)
    rmv, rna, rst = (np.asarray(x) for x in ref)
    for i, e in enumerate(lay.exp):
        if e:
            assert int(mv[i]) == -1, i
            assert na[i].tolist() == [0] * 7, i
            assert st[i].tolist() == [0, 0, 0, 0, 0, e, 0, 0], i
        else:
            assert int(mv[i]) == int(rmv[i]) and 0 <= int(mv[i]) < 7, i
            assert na[i].tolist() == rna[i].tolist() and st[i].tolist() == rst[i].tolist(), i
            assert int(st[i][5]) == 0


def assert_streams(lay, a, b, before, games=None):
    """Flagged games drew nothing; the others stand where the twin's stand."""
    games = list(range(N)) if games is None else games
    for i, e in enumerate(lay.exp):
        g = games[i]
        assert a.rng(g) == (before[g] if e else b.rng(g)), (i, g)
    assert any(a.rng(games[i]) != before[games[i]] for i in lay.good)   # the comparison is not vacuous


def _raw_search(eng, roots, games=None):
    """zc_c4_search / zc_c4_search_games into pre-filled host outputs: (rc, message, outputs)."""
    L = _native.lib()
    n = len(roots)
    mv = np.full(n, FILL32, np.int32)
    na = np.full((n, 7), FILL32, np.int32)
    st = np.full((n, 8), FILL64, np.int64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    if games is None:
        rc = L.zc_c4_search(eng.handle, 0, n, p(roots), SIMS, C, BS, p(mv), p(na), p(st))
    else:
        ids = np.ascontiguousarray(games, np.int32)
        rc = L.zc_c4_search_games(eng.handle, n, p(ids), p(roots), SIMS, C, BS, p(mv), p(na), p(st))
    return rc, L.zc_last_error().decode(), (mv, na, st)


def _message(e):
    return "root has no legal move" if e == NO_MOVES else "invalid Connect4 state (status 2)"


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_c4_search_names_the_first_flagged_game(name):
    lay = Layout(name)
    a, b = pools()
    before = [a.rng(g) for g in range(N)]
    rc, msg, got = _raw_search(a.eng, lay.roots)
    rc_b, _, ref = _raw_search(b.eng, lay.twin)
    assert rc_b == 0 and rc == _native.ZC_EINVAL
    assert msg.startswith(f"game {lay.bad[0]}: ") and _message(lay.exp[lay.bad[0]]) in msg
    assert_rows(lay, got, ref)
    assert_streams(lay, a, b, before)
    with pytest.raises(ValueError, match=f"game {lay.bad[0]}: "):       # the Python entry raises it
        a.eng.c4_search(lay.roots, SIMS, C, BS)
    a.close()
    b.close()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_c4_search_games_names_the_engine_game_not_the_row(name):
    lay = Layout(name)
    games = [5, 2, 7, 0, 3, 6, 1, 4]
    a, b = pools()
    before = [a.rng(g) for g in range(N)]
    rc, msg, got = _raw_search(a.eng, lay.roots, games)
    rc_b, _, ref = _raw_search(b.eng, lay.twin, games)
    assert rc_b == 0 and rc == _native.ZC_EINVAL
    assert msg.startswith(f"game {games[lay.bad[0]]}: ")
    assert_rows(lay, got, ref)
    assert_streams(lay, a, b, before, games)
    a.close()
    b.close()


def _device_outputs():
    return (torch.full((N,), FILL32, dtype=torch.int32, device="cuda"),
            torch.full((N, 7), FILL32, dtype=torch.int32, device="cuda"),
            torch.full((N, 8), FILL64, dtype=torch.int64, device="cuda"))


def _host(outs):
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in outs)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_c4_search_async_flags_on_the_device(name):
    lay = Layout(name)
    a, b = pools()
    before = [a.rng(g) for g in range(N)]
    res = []
    for p, roots in ((a, lay.roots), (b, lay.twin)):
        d_roots, outs = c4_rows(roots), _device_outputs()
        p.eng.c4_search_async(d_roots.data_ptr(), N, SIMS, C, BS, *(x.data_ptr() for x in outs))
        res.append(_host(outs))
        assert torch.equal(d_roots, c4_rows(roots))
    assert_rows(lay, *res)
    assert_streams(lay, a, b, before)
    a.close()
    b.close()


def _leaf_values(leaves):
    """A value in {-1, -0.5, 0, 0.5, 1} from the leaf's stones (any deterministic function does)."""
    return ((leaves[:, 0] ^ (leaves[:, 1] * 3)) % 5).to(torch.float64) / 2 - 1


def _stepwise(p, roots):
    """begin, [select, backup] per flush, end, by hand; the leaf counts of every flush."""
    e = p.eng
    d_roots, outs = c4_rows(roots), _device_outputs()
    leaves = torch.zeros((N * BS, 3), dtype=torch.int64, device="cuda")
    counts = torch.empty(N, dtype=torch.int32, device="cuda")
    seen = []
    e.c4_ext_begin(0, N, d_roots.data_ptr(), SIMS, C, BS)
    for f in range((SIMS + BS - 1) // BS):
        counts.fill_(FILL32)
        e.c4_ext_select(0, N, f, leaves.data_ptr(), 0, True, counts.data_ptr())
        values = _leaf_values(leaves).contiguous()
        e.c4_ext_backup(0, N, f, values.data_ptr())
        seen.append(counts.cpu().tolist())
    e.c4_ext_end(0, N, *(x.data_ptr() for x in outs))
    return _host(outs), seen


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_c4_stepwise_value_search_gives_a_flagged_game_no_leaves(name):
    lay = Layout(name)
    a, b = pools()
    before = [a.rng(g) for g in range(N)]
    got, seen = _stepwise(a, lay.roots)
    ref, seen_b = _stepwise(b, lay.twin)
    for f, (row, row_b) in enumerate(zip(seen, seen_b)):
        nb = min(BS, SIMS - f * BS)
        assert row_b == [nb] * N
        assert row == [0 if e else nb for e in lay.exp], f
    assert_rows(lay, got, ref)
    assert_streams(lay, a, b, before)
    a.close()
    b.close()


def _net(leaves, planes, counts):
    return _leaf_values(leaves), torch.zeros((leaves.shape[0], 7), dtype=torch.float32, device=leaves.device)


@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_c4_puct_begin_flags_and_leaves_the_others_alone(name, reuse):
    from zeroclone_amd.valued import C4PuctSearch
    lay = Layout(name, puct=True)
    assert lay.exp[LAYOUTS[name].index("won")] == NO_MOVES
    a, b = pools()
    before = [a.rng(g) for g in range(N)]
    res = []
    for p, roots in ((a, lay.roots), (b, lay.twin)):
        ps = C4PuctSearch(p.eng, N, BS, dirichlet_eps=0.25, seed=11, reuse=reuse)
        if reuse:   # a first search of valid roots, so that the flagged begin meets kept trees
            ps.run(c4_rows(lay.twin), SIMS, _net)
        ps.move.fill_(FILL32)
        ps.na.fill_(FILL32)
        ps.stats.fill_(FILL64)
        ps.prior.fill_(7.0)
        mv, na, st = ps.run(c4_rows(roots), SIMS, _net)
        res.append((mv.cpu().numpy(), na.cpu().numpy(), st.cpu().numpy(), ps.prior.cpu().numpy()))
    assert_rows(lay, res[0][:3], res[1][:3])
    for i, e in enumerate(lay.exp):
        assert res[0][3][i].tolist() == ([0.0] * 7 if e else res[1][3][i].tolist()), i
    for g in range(N):   # the PUCT search draws nothing from the games' MT19937 streams
        assert a.rng(g) == before[g]
    a.close()
    b.close()


SELFPLAY = [("free", "exact", 8, 32), ("pooled", "exact", 8, 32), ("carry", "exact", 8, 32),
            ("pooled", "philox", 8, 32), ("carry", "philox", 8, 32), ("free", "exact", 64, 64)]


@pytest.mark.parametrize("form,mode,bs,sims", SELFPLAY)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_c4_selfplay_launch_skips_a_flagged_game(name, form, mode, bs, sims):
    lay = Layout(name)
    a, b = pools(max_batch=64 if bs == 64 else 16)   # the batch-64 engine for the one case that needs it
    out = []
    before = [a.rng(g) for g in range(N)]
    for p, roots in ((a, lay.roots), (b, lay.twin)):
        p.eng.c4_rollout_mode(mode, 99)
        p.roots.copy_(c4_rows(roots))
        seq = p.launch(form, MOVES, sims=sims, bs=bs, c=C)     # pooled: a budget of n x moves_cap
        tabs, stats, ticket = p.tables(MOVES, N), p.stats.cpu().clone(), p.ticket.cpu().tolist()
        if form == "carry":
            # the twin's 8 good games spend the whole budget, so its last moves may be suspended (the
            # launch with flagged games never spends it): the drain finishes them, and the games'
            # finished moves and summed counters are compared
            seq = [x + y for x, y in zip(seq, p.launch("pooled", 1, sims=sims, bs=bs, c=C, budget=0))]
            stats = stats + p.stats.cpu()
        out.append((seq, tabs, stats, p.roots.cpu(), ticket))
    (seq, (res, mv, st), stats, roots, ticket), (rseq, _, rstats, rroots, _) = out
    given = c4_rows(lay.roots).cpu()
    for i, e in enumerate(lay.exp):
        if e:
            assert res[:, i].tolist() == [SKIP] * MOVES and mv[:, i].tolist() == [-1] * MOVES, i
            assert bool((st[:, i] == FILL64).all()), i                    # no state row written
            assert seq[i] == []
            assert stats[i].tolist() == [0, 0, 0, 0, 0, e, 0, 0], i       # reserved (games finished) 0 too
            assert torch.equal(roots[i], given[i]), i
        else:
            assert SKIP not in res[:, i].tolist(), i                      # all its moves in the one launch
            assert len(seq[i]) == MOVES and seq[i] == rseq[i], i          # (result, move, state) per move
            assert torch.equal(roots[i], rroots[i]), i
            assert stats[i].tolist() == rstats[i].tolist() and int(stats[i, 5]) == 0, i
            assert int(stats[i, 2]) == sims * MOVES
            assert int(roots[i, 2]) >> 32 == 0                            # reserved is written as 0
    if form != "free":
        assert ticket[1] == MOVES
        assert ticket[0] >= len(lay.good) * MOVES + len(lay.bad)          # one ticket per flagged game
    else:
        assert ticket == [FILL32, FILL32]
    assert_streams(lay, a, b, before)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- chess
# 6 games, 16 simulations, batch 8: a mated and a stalemated root (ZC_STATUS_NO_MOVES), the
# 257-move board and the queen ring (more legal moves than a move list holds:
# ZC_STATUS_CAPACITY), ordinary positions between them.  The expected status comes from the
# oracle's move count; the ordinary games are compared with a twin engine as above.  A flagged
# game: its status, move 0xFFFF, a zero visit row, no expansion, an untouched MT19937 stream.
from test_gpu_chess import CAPACITY_BOARDS, ORDINARY, PROBE_FENS   # noqa: E402

CN, CSIMS, CBS = 6, 16, 8
CAPACITY = 4


def _chess_row(board64: str, turn=0, fifty=0, castle=0):
    a = np.zeros((), _native.CHESS_STATE_DTYPE)
    a["board"] = np.frombuffer(board64.encode("latin-1"), np.uint8)
    a["turn"], a["fifty"], a["castle"] = turn, fifty, castle
    return a, oracle.chess_move_count(oracle.chess_state(board64, turn, fifty, castle))


def _chess_fen(fen):
    return _native.chess_from_fen(fen).reshape(()), oracle.chess_move_count(oracle.chess_from_fen(fen))


def _chess_layout(names):
    """(rows [6, 72] uint8 on the device, the twin's rows, expected statuses)."""
    src = {"mated": _chess_fen(PROBE_FENS[0]), "stalemate": _chess_fen(PROBE_FENS[1]),
           "257": _chess_row(CAPACITY_BOARDS["257"][0]), "ring": _chess_row(CAPACITY_BOARDS["ring"][0]),
           "o0": _chess_fen(ORDINARY[0]), "o1": _chess_fen(ORDINARY[1]), "o2": _chess_fen(ORDINARY[2])}
    exp = [NO_MOVES if src[k][1] == 0 else CAPACITY if src[k][1] > _native.CHESS_MAX_MOVES else 0 for k in names]
    assert exp[0] and exp[-1] and any(exp[1:-1]) and not all(exp)
    rows = [src[k][0] for k in names]
    twin = [src["o2"][0] if e else r for r, e in zip(rows, exp)]
    dev = lambda rs: torch.from_numpy(np.frombuffer(   # noqa: E731
        np.array(rs, _native.CHESS_STATE_DTYPE).tobytes(), np.uint8).reshape(len(rs), 72).copy()).cuda()
    return dev(rows), dev(twin), exp


CHESS_LAYOUTS = {"all": ["mated", "o0", "257", "o1", "stalemate", "ring"],
                 "no moves": ["mated", "o0", "stalemate", "o1", "o0", "stalemate"],
                 "capacity": ["257", "o0", "ring", "o1", "o0", "257"]}


def test_the_chess_root_cases_are_what_they_claim():
    assert _chess_layout(CHESS_LAYOUTS["all"])[2] == [NO_MOVES, 0, CAPACITY, 0, NO_MOVES, CAPACITY]
    assert _chess_layout(CHESS_LAYOUTS["no moves"])[2] == [NO_MOVES, 0, NO_MOVES, 0, 0, NO_MOVES]
    assert _chess_layout(CHESS_LAYOUTS["capacity"])[2] == [CAPACITY, 0, CAPACITY, 0, 0, CAPACITY]


def _chess_engines():
    out = []
    for _ in range(2):
        e = _native.NativeEngine(max_games=CN, max_sims=64, max_batch=CBS)
        e.seed(0, [77 * g + 1 for g in range(CN)])
        e.chess_reserve()
        out.append(e)
    return out


def _rng(e, g):
    mt, idx = e.get_rng_state(g)
    return mt.tolist(), idx


def assert_chess_rows(exp, got, ref, a, b, before, puct=False):
    """got / ref: (move [n] int16, visits [n, 256], stats [n, 8]) on the host."""
    (mv, na, st), (rmv, rna, rst) = got, ref
    for i, e in enumerate(exp):
        if e:
            assert int(st[i][5]) == e, i
            assert int(mv[i]) & 0xFFFF == 0xFFFF, i
            assert not na[i].any(), i
            assert int(st[i][0]) == 0 and int(st[i][1]) == 0 and int(st[i][4]) == 0, i   # no expansion, no draw
            if puct and e == NO_MOVES:
                assert int(st[i][2]) == 0, i
            assert _rng(a, i) == before[i], i
        else:
            assert int(st[i][5]) == 0 and int(mv[i]) & 0xFFFF != 0xFFFF, i
            assert int(mv[i]) == int(rmv[i]) and na[i].tolist() == rna[i].tolist(), i
            assert st[i].tolist() == rst[i].tolist(), i
            assert _rng(a, i) == _rng(b, i), i


def _chess_outputs():
    return (torch.full((CN,), 0x5A5A, dtype=torch.int16, device="cuda"),
            torch.full((CN, _native.CHESS_MAX_MOVES), FILL32, dtype=torch.int32, device="cuda"),
            torch.full((CN, 8), FILL64, dtype=torch.int64, device="cuda"))


def test_chess_search_async_flags_a_root_without_moves_or_room():
    rows, twin, exp = _chess_layout(CHESS_LAYOUTS["all"])
    a, b = _chess_engines()
    before = [_rng(a, g) for g in range(CN)]
    res = []
    for e, r in ((a, rows), (b, twin)):
        given, outs = r.clone(), _chess_outputs()
        e.chess_search_async(0, CN, r.data_ptr(), CSIMS, C, CBS, _native.ZC_POLICY_IMMEDIATE_VALUE, 3.0,
                             *(x.data_ptr() for x in outs))
        res.append(_host(outs))
        assert torch.equal(r, given)
    assert_chess_rows(exp, res[0], res[1], a, b, before)
    assert any(_rng(a, i) != before[i] for i in range(CN) if not exp[i])
    a.close()
    b.close()


def _chess_leaf_values(leaves):
    return (leaves[:, :64].to(torch.int64).sum(1) % 5).to(torch.float64) / 2 - 1


def test_chess_stepwise_value_search_gives_a_flagged_game_no_leaves():
    from zeroclone_amd.valued import ChessValuedSearch
    rows, twin, exp = _chess_layout(CHESS_LAYOUTS["all"])
    a, b = _chess_engines()
    before = [_rng(a, g) for g in range(CN)]
    res, seen = [], []
    for e, r in ((a, rows), (b, twin)):
        vs = ChessValuedSearch(e, CN, CBS, planes=False)
        vs.move.fill_(0x5A5A)
        vs.na.fill_(FILL32)
        vs.stats.fill_(FILL64)
        counts = []

        def value_fn(leaves, planes, cv, counts=counts):
            counts.append(cv.cpu().tolist())
            return _chess_leaf_values(leaves)

        mv, na, st = vs.run(r, CSIMS, C, value_fn)
        res.append((mv.cpu().numpy(), na.cpu().numpy(), st.cpu().numpy()))
        seen.append(counts)
    assert len(seen[0]) == CSIMS // CBS
    for row, row_b in zip(*seen):
        assert row_b == [CBS] * CN and row == [0 if e else CBS for e in exp]
    assert_chess_rows(exp, res[0], res[1], a, b, before)
    a.close()
    b.close()


def _chess_net(leaves, planes, counts):
    return (_chess_leaf_values(leaves),
            torch.zeros((leaves.shape[0], 4096), dtype=torch.float32, device=leaves.device))


@pytest.mark.parametrize("reuse", [False, True])
def test_chess_puct_begin_flags_and_leaves_the_others_alone(reuse):
    from zeroclone_amd.valued import ChessPuctSearch
    rows, twin, exp = _chess_layout(CHESS_LAYOUTS["all"])
    a, b = _chess_engines()
    before = [_rng(a, g) for g in range(CN)]
    res = []
    for e, r in ((a, rows), (b, twin)):
        ps = ChessPuctSearch(e, CN, CBS, dirichlet_eps=0.25, seed=3, reuse=reuse)
        if reuse:   # a first search of valid roots, so that the flagged begin meets kept trees
            ps.run(twin, CSIMS, _chess_net)
        ps.move.fill_(0x5A5A)
        ps.na.fill_(FILL32)
        ps.stats.fill_(FILL64)
        ps.prior.fill_(7.0)
        mv, na, st = ps.run(r, CSIMS, _chess_net)
        res.append((mv.cpu().numpy(), na.cpu().numpy(), st.cpu().numpy(), ps.prior.cpu().numpy()))
    for g in range(CN):   # the PUCT search draws nothing from the MT19937 streams
        assert _rng(a, g) == before[g] == _rng(b, g)
    assert_chess_rows(exp, res[0][:3], res[1][:3], a, b, before, puct=True)
    for i, e in enumerate(exp):
        assert res[0][3][i].tolist() == ([0.0] * _native.CHESS_MAX_MOVES if e else res[1][3][i].tolist()), i
    a.close()
    b.close()


@pytest.mark.parametrize("name,err,message", [("no moves", [0, 0, 1], "no move for a live game"),
                                              ("capacity", [0, 1, 0], "child-slot pool"),
                                              ("all", [0, 1, 1], "child-slot pool")])
def test_chess_selfplay_launch_raises_the_documented_err_words(name, err, message):
    """chess_selfplay_kernel: a root without moves raises bit 2 of its flags (the third err
    word), one without room the capacity word; ChessSelfPlay.check() names the condition."""
    from zeroclone_amd.selfplay import ChessSelfPlay
    rows, twin, exp = _chess_layout(CHESS_LAYOUTS[name])
    moves = 2
    out = []
    for r in (rows, twin):
        sp = ChessSelfPlay(CN, CSIMS, batch_size=CBS, seed=9, hist_cap=64)
        sp.roots.copy_(r)
        before = [_rng(sp.eng, g) for g in range(CN)]
        res = sp.run(moves).cpu()
        torch.cuda.synchronize()
        out.append((sp, before, res, sp._run_moves.cpu(), sp._run_states.cpu(), sp.stats.cpu(), sp.roots.cpu()))
    (a, before, res, mv, st, stats, roots), (b, _, rres, rmv, rst, rstats, rroots) = out
    assert a.err.cpu().tolist() == err and b.err.cpu().tolist() == [0, 0, 0]
    with pytest.raises(RuntimeError, match=message):
        a.check()
    b.check()
    given = rows.cpu()
    for i, e in enumerate(exp):
        if e:
            assert res[:, i].tolist() == [SKIP] * moves and mv[:, i].tolist() == [-1] * moves, i
            assert not st[:, i].any(), i                                   # no state row written
            assert stats[i].tolist() == [0, 0, 0, 0, 0, e, 0, 0], i
            assert torch.equal(roots[i], given[i]) and _rng(a.eng, i) == before[i], i
        else:
            assert SKIP not in res[:, i].tolist(), i
            assert torch.equal(res[:, i], rres[:, i]) and torch.equal(mv[:, i], rmv[:, i]), i
            assert torch.equal(st[:, i], rst[:, i]) and torch.equal(roots[i], rroots[i]), i
            assert stats[i].tolist() == rstats[i].tolist() and int(stats[i, 5]) == 0, i
            assert _rng(a.eng, i) == _rng(b.eng, i) != before[i], i
            assert torch.equal(a.hist[i], b.hist[i]) and torch.equal(a.hlen[i], b.hlen[i]), i
    a.close()
    b.close()
