"""GPU checks of the two PUCT searches (chess_puct.hip, c4_puct.hip) under non-uniform priors,
against their specification (oracle/puct_ref.py through tests/puct_prior_cases.py; the cases and
what each is there for: test_puct_priors_cpu.py).

Priors: every evaluated node of every game against the float64 softmax of the logits the host
callback supplied for that position, over the node's moves in list order; the error within 8
floors (the float32 restatement's own error, absolute and relative), bit equality where the
restatement is exact, masked moves exactly 0 (puct_prior_cases.check_priors).  Search: the
device's own priors replayed into the specification, then the whole tree node by node in creation
order — position, parent, edge, move list, every edge's N, every edge's W bit for bit, child
presence, the evaluated flag — and the move at temperature 0 (compare_trees).  Reuse: sequences
of five reused searches under moderate hash logits.  Limits: the chess kernel's depth limit and
slot pool end a search exactly where the specification's max_level = 62 and slot_cap say, a
failed game keeps nothing and disturbs no other game.  Non-finite network outputs end the game
with ZC_STATUS_INTERNAL and touch nothing else.

Measured on an MI355X (max over a case's games and nodes, device - float64 softmax against the
float32 restatement's floor): see DESIGN.md §5."""
import numpy as np
import pytest
import torch

import oracle
import chess_puct_reuse_ref as chess_spec
import puct_prior_cases as pc
import puct_reuse_ref as c4_spec

pytestmark = pytest.mark.gpu

MAX_SIMS = 260
NODE_FIELDS = ("st", "base", "nmoves", "nu", "parent", "pact", "depth", "material", "check", "evaluated")
SLOT_FIELDS = ("mv", "prior", "na", "w", "child")
STATUS_INTERNAL, STATUS_CAPACITY = 3, 4


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=16, max_sims=MAX_SIMS, max_batch=32)
    yield e
    e.close()


class HostNet:
    """A search's net_fn from a case's Logits: per flush, the value and the logit row of each
    pending leaf's position; every other row of the buffers holds a filler no position owns.
    roots_only: flush 0 comes without leaves, one row a game (valued.PolicyNet's path).
    tamper(flush, values, logits, keys): edits the host arrays before they go to the device.
    counts: the leaves selected per flush and game, as the device reported them."""

    def __init__(self, logits, root_keys, bs, roots_only=False, tamper=None):
        self.lg, self.root_keys, self.bs, self.roots_only, self.tamper = logits, root_keys, bs, roots_only, tamper
        self.counts, self._fill, self.roots_flush = [], {}, False

    def __call__(self, leaves, planes, counts):
        g, lg = self.lg.game, self.lg
        cnt = counts.cpu().numpy().copy()
        f = len(self.counts)
        self.counts.append(cnt)
        n = len(cnt)
        if leaves is None:
            assert f == 0 and self.roots_only
            self.roots_flush = True
            per, keys = 1, [[k][:int(c)] for k, c in zip(self.root_keys, cnt)]
        else:
            rows = leaves.cpu().numpy()
            per = self.bs
            keys = [[g.row_key(rows[i * per + j]) for j in range(int(cnt[i]))] for i in range(n)]
        L = n * per
        if L not in self._fill:
            self._fill[L] = np.stack([lg.filler(0x9E37 + r) for r in range(L)])
        v, x = np.full(L, 0.123), self._fill[L].copy()
        for i, ks in enumerate(keys):
            for j, k in enumerate(ks):
                v[i * per + j] = lg.value(k)
                x[i * per + j] = lg.row(k)
        if self.tamper is not None:
            self.tamper(f, v.reshape(n, per), x.reshape(n, per, g.width), keys)
        dev = counts.device
        t = torch.from_numpy(x).to(dev)
        return torch.from_numpy(v).to(dev), (t.half() if lg.half else t)


def _chess_rows(keys):
    r = np.zeros((len(keys), 72), np.uint8)
    for i, (board, turn, fifty, castle) in enumerate(keys):
        r[i, :64] = np.frombuffer(board, np.uint8)
        r[i, 64:67] = (turn, fifty, castle)
    return torch.from_numpy(r).cuda()


def _c4_rows(keys):
    return torch.tensor([list(k) for k in keys], dtype=torch.int64).cuda()   # (stones fit in 49 bits)


def _search(eng, game, n, bs, c, reuse=False):
    from zeroclone_amd.valued import C4PuctSearch, ChessPuctSearch
    cls = ChessPuctSearch if game is pc.Chess else C4PuctSearch
    return cls(eng, n, bs, c_puct=c, dirichlet_eps=0.0, reuse=reuse)


def _roots(game, keys):
    return _chess_rows(keys) if game is pc.Chess else _c4_rows(keys)


def _dump(eng, game, g):
    if game is pc.Chess:
        d = eng.debug_chess_tree(g, max_nodes=512, max_slots=1 << 15)
        return {f: v.copy() for f, v in d.items()}
    return eng.debug_c4_puct_tree(g, max_nodes=512).copy()


def _tree(game, dump):
    return pc.chess_dump_tree(dump) if game is pc.Chess else pc.c4_dump_tree(dump)


def _same_dump(game, a, b):
    """Two dumps byte for byte (the records' padding aside)."""
    if game is pc.Chess:
        assert len(a["nodes"]) == len(b["nodes"])
        for f in NODE_FIELDS:
            assert np.ascontiguousarray(a["nodes"][f]).tobytes() == np.ascontiguousarray(b["nodes"][f]).tobytes(), f
        for f in SLOT_FIELDS:
            assert a[f].tobytes() == b[f].tobytes(), f
    else:
        assert len(a) == len(b)
        for f in a.dtype.names:
            if not f.startswith("pad"):
                assert np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes(), f


def _move(game, m):
    if game is pc.C4:
        return int(m)
    if int(m) & 0xFFFF == 0xFFFF:
        return -1
    from zeroclone_amd._native import unpack_chess_move
    sq, val = unpack_chess_move(int(m) & 0xFFFF)
    return sq + (val,)


def _root_visits(game, na_row, moves):
    return [int(na_row[col]) for col in moves] if game is pc.C4 else [int(x) for x in na_row[:len(moves)]]


def _against_the_spec(eng, game, lg, g, state, sims, bs, c, mv, na, what, masked_unvisited=False, **kw):
    """Game g's dump: its priors against the logits, then the whole tree and the move against the
    specification on those priors.  Returns (check_priors' figures, the SpecRun)."""
    tree = _tree(game, _dump(eng, game, g))
    fig = pc.check_priors(tree, lg, f"{what} game {g}", masked_unvisited)
    run = pc.SpecRun(lg, state, sims, bs, c, priors=pc.device_priors(game, tree), **kw)
    assert run.capacity is None
    pc.compare_trees(tree, run.tree, f"{what} game {g}")
    assert _root_visits(game, na[g], run.moves) == run.N and _move(game, mv[g]) == run.moves[run.best]
    return fig, run


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_priors_and_whole_tree_match_the_specification(eng, case):
    game, lg, roots = case.game, case.logits(), case.roots()
    keys = [game.key(s) for s in roots]
    ps = _search(eng, game, len(roots), case.bs, case.c)
    net = HostNet(lg, keys, case.bs, case.roots_only)   # (roots_only: what valued._puct_backup looks for)
    mv, na, st = ps.run(_roots(game, keys), case.sims, net)
    mv, na, st = mv.cpu().numpy(), na.cpu().numpy(), st.cpu().numpy()
    assert (st[:, 5] == 0).all() and (na.sum(axis=1) == case.sims - 1).all()
    assert net.roots_flush == case.roots_only   # the backup's rows = 1 path ran where the case asks for it
    figs = []
    for g, s in enumerate(roots):   # no game is left out
        fig, run = _against_the_spec(eng, game, lg, g, s, case.sims, case.bs, case.c, mv, na, case.name,
                                     case.masked_unvisited)
        figs.append(fig)
        assert [int(cnt[g]) for cnt in net.counts] == run.flush_counts(case.sims, case.bs)
    err, floor, rerr, rfloor = (max(f[k] for f in figs) for k in range(4))
    print(f"case {case.name}: abs {err:.3e} / floor {floor:.3e}, rel {rerr:.3e} / floor {rfloor:.3e}, "
          f"worst game {max((f[0] / f[1] if f[1] else 0) for f in figs):.2f} abs floors, "
          f"{max((f[2] / f[3] if f[3] else 0) for f in figs):.2f} rel floors, {sum(f[4] for f in figs)} nodes")


def _subtree(root):
    out, todo = set(), [root]
    while todo:
        n = todo.pop()
        out.add(id(n))
        todo += [ch for ch in n.child if ch is not None]
    return out


@pytest.mark.parametrize("game", [pc.Chess, pc.C4], ids=["chess", "c4"])
def test_reused_search_sequences_under_moderate_logits(eng, game):
    """Five searches of two games, each keeping the played move's subtree: kept nodes, the whole
    tree (the kept part compacted in creation order, then this search's nodes), visits and move."""
    sims, bs, c, n = 65, 8, 1.5, 2
    lg = pc.Logits(game, "hash", 3)
    states = [oracle.chess_from_fen(pc.START), oracle.chess_from_fen(pc.KIWIPETE)] if game is pc.Chess else \
        [pc.c4_board([]), pc.c4_board([3, 3, 2, 4])]
    ps = _search(eng, game, n, bs, c, reuse=True)
    trees = [(None, [])] * n
    reused = 0
    for t in range(5):
        keys = [game.key(s) for s in states]
        mv, na, st = ps.run(_roots(game, keys), sims, HostNet(lg, keys, bs))
        mv, na, st = mv.cpu().numpy(), na.cpu().numpy(), st.cpu().numpy()
        assert (st[:, 5] == 0).all()
        for g in range(n):
            old, order = trees[g]
            if game is pc.Chess:
                root, kept = chess_spec.next_root(old, states[g], sims, MAX_SIMS + 1)
            else:
                root, kept = c4_spec.next_root(old, states[g], sims, MAX_SIMS + 1)
            inside = _subtree(root)
            order = [x for x in order if id(x) in inside] if kept else [root]
            assert len(order) == (kept or 1) and int(ps.kept[g]) == kept, (t, g)
            _, run = _against_the_spec(eng, game, lg, g, states[g], sims, bs, c, mv, na, f"reuse {game.name} search {t}",
                                       root=root, order=order, reused=kept > 0)
            assert int(st[g, 2]) == (sims - 1 if kept else sims)
            trees[g] = (root, run.order)
            reused += kept > 1
            states[g] = game.rules.play(states[g], run.moves[run.best])
    assert reused >= 4


LINE = pc.Logits(pc.Chess, "line", 40)


@pytest.mark.parametrize("bs,last_ok", [(1, 63), (4, 249)])
def test_the_depth_limit_is_where_the_specification_puts_it(eng, bs, last_ok):
    """The line logits grow one level a flush.  The last simulation count that ends with status 0
    holds a leaf at level 62; one more stands a walk on it: ZC_STATUS_CAPACITY, no move, and the
    flush of that walk selects nothing."""
    states = [oracle.chess_from_fen(f) for f in pc.LINE_FENS]
    keys = [pc.Chess.key(s) for s in states]
    ps = _search(eng, pc.Chess, len(keys), bs, 1.5)
    for sims, ok in ((last_ok, True), (last_ok + 1, False)):
        net = HostNet(LINE, keys, bs)
        mv, na, st = ps.run(_chess_rows(keys), sims, net)
        mv, na, st = mv.cpu().numpy(), na.cpu().numpy(), st.cpu().numpy()
        for g, s in enumerate(states):
            if ok:
                assert st[g, 5] == 0
                _, run = _against_the_spec(eng, pc.Chess, LINE, g, s, sims, bs, 1.5, mv, na, f"depth {sims}x{bs}",
                                           max_level=pc.MAX_LEVEL)
                assert max(pc.levels(run.tree)) == pc.MAX_LEVEL
            else:
                run = pc.SpecRun(LINE, s, sims, bs, 1.5, max_level=pc.MAX_LEVEL)
                assert run.capacity is not None and run.capacity.kind == "depth"
                assert st[g, 5] == STATUS_CAPACITY and _move(pc.Chess, mv[g]) == -1
            assert [int(cnt[g]) for cnt in net.counts] == run.flush_counts(sims, bs)


def test_slot_overrun_and_a_failed_game_beside_healthy_ones():
    """sims = max_sims = 128 on the many-queens position overruns the 64 * 129 slots in the flush
    the specification names: status ZC_STATUS_CAPACITY and no move for that game; the other games
    of the launch hold the trees of a launch without it, byte for byte; with reuse on, the failed
    game's next search keeps nothing and is a fresh search."""
    from zeroclone_amd._native import NativeEngine
    sims, bs, c = 128, 8, 1.5
    lg = pc.Logits(pc.Chess, "hash", 3)
    e = NativeEngine(max_games=4, max_sims=sims, max_batch=bs)
    try:
        states = [oracle.chess_from_fen(f) for f in (pc.SLOT_FEN, pc.START, pc.KIWIPETE)]
        keys = [pc.Chess.key(s) for s in states]
        ps = _search(e, pc.Chess, 3, bs, c, reuse=True)
        net = HostNet(lg, keys, bs)
        mv, na, st = ps.run(_chess_rows(keys), sims, net)
        mv, na, st = mv.cpu().numpy().copy(), na.cpu().numpy().copy(), st.cpu().numpy().copy()
        bad = pc.SpecRun(lg, states[0], sims, bs, c, slot_cap=64 * (sims + 1))
        assert bad.capacity is not None and bad.capacity.kind == "slots"
        assert st[0, 5] == STATUS_CAPACITY and _move(pc.Chess, mv[0]) == -1
        assert [int(cnt[0]) for cnt in net.counts] == bad.flush_counts(sims, bs)   # the spec's flush
        assert list(st[1:, 5]) == [0, 0]
        beside = [_dump(e, pc.Chess, g) for g in (1, 2)]
        for g in (1, 2):
            _against_the_spec(e, pc.Chess, lg, g, states[g], sims, bs, c, mv, na, "beside a failed game",
                              slot_cap=64 * (sims + 1))
        # the failed game's next search: a position its tree holds one ply down, yet nothing is kept
        k = next(j for j, ch in enumerate(bad.root.child) if ch is not None and ch.evaluated and len(ch.moves))
        nxt = [oracle.chess_play(states[0], bad.root.moves[k]), states[1], states[2]]
        nkeys = [pc.Chess.key(s) for s in nxt]
        mv2, na2, st2 = ps.run(_chess_rows(nkeys), 33, HostNet(lg, nkeys, bs))
        mv2, na2, st2 = mv2.cpu().numpy(), na2.cpu().numpy(), st2.cpu().numpy()
        assert int(ps.kept[0]) == 0 and st2[0, 5] == 0 and st2[0, 2] == 33
        _against_the_spec(e, pc.Chess, lg, 0, nxt[0], 33, bs, c, mv2, na2, "after a failed search")
        # the same launch with a healthy game in the failed one's place
        keys[0] = keys[1]
        plain = _search(e, pc.Chess, 3, bs, c)
        _, _, st3 = plain.run(_chess_rows(keys), sims, HostNet(lg, keys, bs))
        assert (st3.cpu().numpy()[:, 5] == 0).all()
        for g, d in zip((1, 2), beside):
            _same_dump(pc.Chess, _dump(e, pc.Chess, g), d)
    finally:
        e.close()


@pytest.mark.parametrize("game", [pc.Chess, pc.C4], ids=["chess", "c4"])
def test_non_finite_network_outputs_end_the_game_and_nothing_else(eng, game):
    """Six games in one launch: a NaN value at flush 3, +inf on a legal move, NaN on every ILLEGAL
    entry (never read: no effect), -inf on a subset of the legal moves (priors exactly 0 there,
    status 0, the specification's tree) and two clean games.  The first two end with
    ZC_STATUS_INTERNAL and no move; every other game's tree is the clean launch's byte for byte."""
    sims, bs, c = 41, 8, 1.5
    lg = pc.Logits(game, "hash", 3)
    masked = pc.Logits(game, "mask", 3)   # the same hash with -inf on a subset: game 3's rows
    if game is pc.Chess:
        states = [oracle.chess_from_fen(f) for f in pc.LINE_FENS + [pc.CHESS_FENS[6], pc.START, pc.KIWIPETE]]
    else:
        states = [pc.c4_board(cols) for cols in ([], [3, 3, 2, 4], [0, 0, 0, 0, 0, 0, 1, 2], [3], [], [3, 3, 2, 4])]
    keys = [game.key(s) for s in states]

    def tamper(f, v, x, ks):
        if f == 3 and ks[0]:
            v[0, 0] = np.nan
        if f == 0:
            x[1, 0, game.index(lg.moves(ks[1][0])[-1])] = np.inf
        for j, k in enumerate(ks[2]):
            legal = np.zeros(game.width, bool)
            legal[[game.index(m) for m in lg.moves(k)]] = True
            if game is pc.C4 and legal.all():
                continue   # seven legal columns: no illegal entry in the row
            x[2, j, ~legal] = np.nan
        for j, k in enumerate(ks[3]):
            x[3, j] = masked.row(k)

    ps = _search(eng, game, 6, bs, c)
    clean_net = HostNet(lg, keys, bs)
    ps.run(_roots(game, keys), sims, clean_net)
    clean = [_dump(eng, game, g) for g in range(6)]
    net = HostNet(lg, keys, bs, tamper=tamper)
    mv, na, st = ps.run(_roots(game, keys), sims, net)
    mv, na, st = mv.cpu().numpy(), na.cpu().numpy(), st.cpu().numpy()
    assert list(st[:, 5]) == [STATUS_INTERNAL, STATUS_INTERNAL, 0, 0, 0, 0]
    assert _move(game, mv[0]) == -1 and _move(game, mv[1]) == -1
    # the NaN value stops game 0 in flush 3's backup, the +inf logit game 1 in flush 0's
    assert [int(cnt[0]) for cnt in net.counts] == [1, 8, 8, 8, 0, 0] and [int(cnt[1]) for cnt in net.counts] == [1] + [0] * 5
    for g in (2, 4, 5):
        _same_dump(game, _dump(eng, game, g), clean[g])
    _against_the_spec(eng, game, masked, 3, states[3], sims, bs, c, mv, na, "masked rows")
    assert np.isneginf(masked.listed(keys[3])).any()   # the root itself has masked moves
