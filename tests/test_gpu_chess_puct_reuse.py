"""GPU checks of the chess PUCT search's tree reuse (zc_chess_puct_begin_reuse, chess_puct.hip's
re-root kernel) against its specification in tests/chess_puct_reuse_ref.py: the re-rooted tree
is exactly the subtree (node records and slot arrays), sequences of reused searches, both
halves of the room rule, the fresh-start rules, root noise on a kept root, the self-play
pool's options, and the option off."""
import numpy as np
import pytest
import torch

import oracle
from oracle import puct_ref
import chess_puct_reuse_ref as spec
from test_gpu_puct import FENS, decode, hash_net, hv, roots_of

pytestmark = pytest.mark.gpu

M = 401          # nodes per tree of the shared engine (max_sims + 1)
S = 64 * M       # and its child slots
NODE_FIELDS = ("st", "base", "nmoves", "nu", "parent", "pact", "depth", "material", "check", "evaluated")
SLOT_FIELDS = ("mv", "prior", "na", "w", "child")
SLOT_FEN = "kr6/pp1Q1q2/2Q2q2/3Q1q2/2Q1q3/1Q2q3/5QPP/6RK w - - 0 1"


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=64, max_sims=400, max_batch=32)
    yield e
    e.close()


def _hv(s):
    return hv(bytes(bytearray(s.board)[:64]), int(s.turn))


def _uniform(node):
    return [float(np.float32(1.0) / np.float32(len(node.moves)))] * len(node.moves)


def hash_logit_net(leaves, planes, counts):
    """hash_net's values with logits that depend on the position (non-uniform priors)."""
    v, _ = hash_net(leaves, planes, counts)
    j = torch.arange(4096, dtype=torch.float64, device="cuda")
    return v, (3.0 * torch.sin(v[:, None] * 977.0 + j[None, :] * 0.37)).float()


def _row(board, turn, fifty, castle):
    r = np.zeros(72, np.uint8)
    r[:64] = np.frombuffer(board, np.uint8)
    r[64:67] = (turn, fifty, castle)
    return r


def _rows(keys):
    """[(board bytes, turn, fifty, castle)] -> zc_chess_state rows on the device."""
    return torch.from_numpy(np.stack([_row(*k) for k in keys])).cuda()


def _dump(eng, g):
    d = eng.debug_chess_tree(g, max_nodes=512, max_slots=1 << 15)
    return {f: v.copy() for f, v in d.items()}


def _kids(d, i):
    """[(slot index, child id)] of node i's expanded moves."""
    b, n = int(d["nodes"]["base"][i]), int(d["nodes"]["nmoves"][i])
    return [(k, int(c)) for k, c in enumerate(d["child"][b:b + n]) if int(c) != 0xFFFF]


def _child_by_move(d, mv):
    b, n = int(d["nodes"]["base"][0]), int(d["nodes"]["nmoves"][0])
    k = [int(m) for m in d["mv"][b:b + n]].index(int(mv) & 0xFFFF)
    return int(d["child"][b + k])


def _subtree_ids(d, r):
    keep = [r]
    for i in range(r + 1, len(d["nodes"])):
        if int(d["nodes"]["parent"][i]) in keep:
            keep.append(i)
    return keep


def _begin_reuse(eng, ps, roots, sims):
    """The re-root alone (no select follows): kept [n] on the host."""
    kept = torch.full((ps.n,), -1, dtype=torch.int32, device="cuda")
    eng.chess_puct_begin_reuse(0, ps.n, roots.data_ptr(), sims, ps.c, ps.bs, ps.alpha, ps.eps, ps.seed,
                               ps.search_no.data_ptr(), kept.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return kept.cpu().numpy()


def _same_tree(got, want):
    assert len(got["nodes"]) == len(want["nodes"])
    for f in NODE_FIELDS:
        assert np.ascontiguousarray(got["nodes"][f]).tobytes() == np.ascontiguousarray(want["nodes"][f]).tobytes(), f
    for f in SLOT_FIELDS:   # na, w and prior bit for bit
        assert got[f].tobytes() == want[f].tobytes(), f


def _is_fresh(d, key):
    nd = d["nodes"]
    assert len(nd) == 1 and spec.dump_key(d, 0) == key
    assert int(nd["parent"][0]) == 0xFFFF and int(nd["pact"][0]) == 0xFFFF and not int(nd["evaluated"][0])
    assert int(nd["base"][0]) == 0 and len(d["mv"]) == int(nd["nmoves"][0])
    assert (d["child"] == 0xFFFF).all() and (d["na"] == 0).all() and (d["w"] == 0).all()


def _room(want, sims, m=M):
    return len(want["nodes"]) + sims - 1 <= m and len(want["mv"]) + 64 * (sims - 1) <= 64 * m


def _check_reroot(eng, sims, bs, plies, net, next_sims):
    """A search of FENS * 2, then the re-root alone (for a search of next_sims) at the chosen
    move's child, or at that child's most visited reply: the trees against spec.compact.
    Returns the nodes kept per game and the old ids they span."""
    from zeroclone_amd.valued import ChessPuctSearch
    fens = FENS * 2
    n = len(fens)
    ps = ChessPuctSearch(eng, n, bs, dirichlet_eps=0.0, reuse=True)
    mv, _, st = ps.run(roots_of(fens), sims, net)
    mv = mv.cpu().numpy()
    assert (st[:, 5] == 0).all() and (ps.kept == 0).all()
    dumps = [_dump(eng, g) for g in range(n)]
    targets = []
    for g, d in enumerate(dumps):
        t = _child_by_move(d, mv[g])   # the chosen move's child
        assert t != 0xFFFF
        if plies == 2:   # and its most visited reply that was expanded (ply 1 where there is none)
            b = int(d["nodes"]["base"][t])
            ch = [(int(d["na"][b + k]), -k, c) for k, c in _kids(d, t)]
            if ch:
                t = max(ch)[2]
        targets.append(t)
    kept = _begin_reuse(eng, ps, _rows([spec.dump_key(d, t) for d, t in zip(dumps, targets)]), next_sims)
    moved, span = 0, []
    for g, (d, t) in enumerate(zip(dumps, targets)):
        after = _dump(eng, g)
        r = spec.find(d, spec.dump_key(d, t))
        if r is None:   # the move ended the game (or its node was never evaluated): nothing to keep
            assert int(d["nodes"]["nmoves"][t]) == 0 or not int(d["nodes"]["evaluated"][t])
            assert kept[g] == 0
            _is_fresh(after, spec.dump_key(d, t))
            continue
        assert r == t and int(d["nodes"]["depth"][t]) == plies
        want = spec.compact(d, r)
        assert _room(want, next_sims)
        assert kept[g] == len(want["nodes"])
        _same_tree(after, want)
        moved += len(want["nodes"]) > 1
        span.append(_subtree_ids(d, r)[-1] - r)
    # Most games keep a real subtree.  By the spec on the CPU (uniform priors): FENS[0..3] one ply
    # down at sims 65, FENS[0..2] one and two plies down at sims 200 and 400 (there the searches
    # of FENS[3] and FENS[4] play their mates, which keep nothing): 6 games of 10 or more.  Two
    # plies down at sims 65 the most visited replies hold 3, 1, 6 and 1 nodes: 4 games of 10.
    assert moved >= (4 if (sims, plies) == (65, 2) else 6)
    if net is hash_logit_net:
        p = dumps[0]["prior"][:int(dumps[0]["nodes"]["nmoves"][0])]
        assert p.max() > 2 * p.min()   # the kept priors are not uniform
    return kept, span


@pytest.mark.parametrize("sims,bs,plies,net", [(65, 8, 1, hash_net), (65, 8, 2, hash_net), (200, 32, 1, hash_net),
                                               (200, 32, 2, hash_net), (200, 32, 1, hash_logit_net)])
def test_reroot_is_exactly_the_subtree(eng, sims, bs, plies, net):
    kept, span = _check_reroot(eng, sims, bs, plies, net, sims)
    if sims == 200:
        assert max(span) > 64   # kept nodes from more than one 64-node chunk of the old tree


@pytest.mark.parametrize("net", [hash_net, hash_logit_net])
def test_reroot_of_more_than_64_kept_nodes(eng, net):
    """A full tree (sims = max_sims = 400) re-rooted for a search of 2 simulations, so that the
    room rule lets a subtree of more than 64 nodes through: more than one window of the slot
    move.  (With hash_net the spec keeps 62, 40 and 75 nodes for FENS[0..2].)"""
    kept, _ = _check_reroot(eng, 400, 32, 1, net, 2)
    assert max(kept) > 64


@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("sims,bs,c", [(65, 8, 1.5), (129, 16, 2.5), (40, 32, 1.0)])
def test_reused_search_sequence_matches_its_specification(eng, sims, bs, c, start):
    from zeroclone_amd.valued import ChessPuctSearch
    ps = ChessPuctSearch(eng, 1, bs, c_puct=c, dirichlet_eps=0.0, reuse=True)
    state, root, reused_searches = oracle.chess_from_fen(FENS[start]), None, 0
    for t in range(5):
        root, kept = spec.next_root(root, state, sims, M)
        kept_visits = sum(root.N)
        moves, N, best = spec.search(root, sims, bs, c, _hv, _uniform, rules=puct_ref.ChessRules, reused=kept > 0)
        mv, na, st = ps.run(_rows([spec.key(state)]), sims, hash_net)
        na, st = na.cpu().numpy(), st.cpu().numpy()
        assert st[0, 5] == 0
        assert int(ps.kept[0]) == kept, t
        assert list(na[0, :len(moves)]) == N, t
        assert decode(mv.cpu().numpy()[0]) == moves[best]
        assert int(na[0].sum()) == kept_visits + sims - 1 == sum(N)
        assert st[0, 2] == (sims - 1 if kept else sims)
        d = _dump(eng, 0)
        assert len(d["nodes"]) == spec.count_nodes(root) == (kept or 1) + st[0, 0]
        assert len(d["mv"]) == spec.count_slots(root)
        reused_searches += kept > 0
        state = oracle.chess_play(state, moves[best])
    assert reused_searches >= 2


def test_slot_half_of_the_room_rule():
    """A position of many queens: 65 nodes take 4780 slots, the chosen child's subtree 11 nodes
    and 822 slots.  With max_sims = 74 (M 75, S 4800) the node half holds (75 <= 75) and the
    slot half does not (822 + 64 * 64 = 4918 > 4800); with max_sims = 76 (S 4928) both hold."""
    from zeroclone_amd._native import NativeEngine
    from zeroclone_amd.valued import ChessPuctSearch
    sims, bs, c = 65, 8, 1.5
    s0 = oracle.chess_from_fen(SLOT_FEN)
    root = puct_ref.Node(s0, puct_ref.ChessRules)
    moves, N, best = spec.search(root, sims, bs, c, _hv, _uniform, rules=puct_ref.ChessRules)
    child = root.child[best]
    numbers = (spec.count_nodes(root), spec.count_slots(root), spec.count_nodes(child), spec.count_slots(child))
    assert numbers == (65, 4780, 11, 822)   # the inputs have not drifted
    s1 = oracle.chess_play(s0, moves[best])
    assert spec.next_root(root, s1, sims, 75)[1] == 0 and spec.next_root(root, s1, sims, 77)[1] == 11
    r0, r1 = _rows([spec.key(s0)]), _rows([spec.key(s1)])
    for max_sims, want_kept in ((74, 0), (76, 11)):
        e = NativeEngine(max_games=4, max_sims=max_sims, max_batch=32)
        ps = ChessPuctSearch(e, 1, bs, c_puct=c, dirichlet_eps=0.0, reuse=True)
        mv, _, st = ps.run(r0, sims, hash_net)
        assert st[0, 5] == 0 and decode(mv.cpu().numpy()[0]) == moves[best]
        d = _dump(e, 0)
        assert (len(d["nodes"]), len(d["mv"])) == numbers[:2]
        if want_kept:   # the re-root alone: nodes of more than 64 moves, slot for slot
            t = _child_by_move(d, mv.cpu().numpy()[0])
            want = spec.compact(d, t)
            assert (len(want["nodes"]), len(want["mv"])) == numbers[2:] and (want["nodes"]["nmoves"] > 64).any()
            assert _begin_reuse(e, ps, r1, sims)[0] == want_kept
            _same_tree(_dump(e, 0), want)
        else:   # a fresh start: the plain begin's search
            out = [x.cpu().clone() for x in ps.run(r1, sims, hash_net)] + [ps.prior.cpu().clone()]
            # (on S = 4800 slots this search may itself run out of slots, as the plain one does:
            # the status is the plain search's, whatever it is)
            assert int(ps.kept[0]) == 0
            plain = ChessPuctSearch(e, 1, bs, c_puct=c, dirichlet_eps=0.0)
            ref = [x.cpu().clone() for x in plain.run(r1, sims, hash_net)] + [plain.prior.cpu().clone()]
            for x, y in zip(out, ref):
                assert torch.equal(x, y)
        e.close()


def test_no_headroom_means_a_fresh_search():
    """max_sims = sims: a tree has sims + 1 nodes, so any kept subtree of 3 nodes or more leaves
    no room for the search's own and the game starts afresh: the plain begin's results."""
    from zeroclone_amd._native import NativeEngine
    from zeroclone_amd.valued import ChessPuctSearch
    sims, bs = 65, 8
    e = NativeEngine(max_games=64, max_sims=sims, max_batch=32)
    fens = FENS * 2
    n = len(fens)
    ps = ChessPuctSearch(e, n, bs, dirichlet_eps=0.0, reuse=True)
    mv, _, _ = ps.run(roots_of(fens), sims, hash_net)
    nxt, big = [], []
    for g, m in enumerate(mv.cpu().numpy()):
        d = _dump(e, g)
        t = _child_by_move(d, m)
        big.append(int(d["nodes"]["nmoves"][t]) > 0 and len(spec.compact(d, t)["nodes"]) >= 3)
        nxt.append(spec.dump_key(d, t))
    assert sum(big) >= 6
    r = _rows(nxt)
    out = [x.cpu().clone() for x in ps.run(r, sims, hash_net)] + [ps.prior.cpu().clone()]
    kept = ps.kept.cpu().numpy()
    plain = ChessPuctSearch(e, n, bs, dirichlet_eps=0.0)
    ref = [x.cpu().clone() for x in plain.run(r, sims, hash_net)] + [plain.prior.cpu().clone()]
    for g in range(n):
        if big[g]:
            assert kept[g] == 0
        if kept[g] == 0:
            for x, y in zip(out, ref):
                assert torch.equal(x[g], y[g]), g
    e.close()


def test_fresh_start_rules(eng):
    """sims 3, bs 2: the root and two walks, into the root's slots 0 and 1."""
    from zeroclone_amd import _native
    from zeroclone_amd.valued import ChessPuctSearch
    ps = ChessPuctSearch(eng, 1, 2, dirichlet_eps=0.0, reuse=True)
    s0 = oracle.chess_from_fen(FENS[0])
    r0 = roots_of([FENS[0]])

    def searched():
        ps.run(r0, 3, hash_net)
        d = _dump(eng, 0)
        assert len(d["nodes"]) == 3 and [int(c) for c in d["child"][:3]] == [1, 2, 0xFFFF]
        return d

    d = searched()
    bare = spec.key(oracle.chess_play(s0, oracle.chess_moves(s0)[2]))   # slot 2 was never walked
    assert _begin_reuse(eng, ps, _rows([bare]), 3)[0] == 0
    _is_fresh(_dump(eng, 0), bare)

    searched()
    assert _begin_reuse(eng, ps, roots_of([FENS[4]]), 3)[0] == 0       # not in the tree
    assert len(_dump(eng, 0)["nodes"]) == 1

    searched()
    assert _begin_reuse(eng, ps, r0, 3)[0] == 0                        # the same position again
    assert len(_dump(eng, 0)["nodes"]) == 1

    d = searched()
    ps.forget()
    assert _begin_reuse(eng, ps, _rows([spec.dump_key(d, 1)]), 3)[0] == 0   # forgotten
    _is_fresh(_dump(eng, 0), spec.dump_key(d, 1))

    d = searched()   # a crude search of the game in between: the arena is no longer the PUCT tree
    mv = torch.zeros(1, dtype=torch.int16, device="cuda")
    na = torch.zeros((1, _native.CHESS_MAX_MOVES), dtype=torch.int32, device="cuda")
    st = torch.zeros((1, _native.STATS_FIELDS), dtype=torch.int64, device="cuda")
    eng.chess_search_async(0, 1, r0.data_ptr(), 8, 1.4, 4, _native.ZC_POLICY_RANDOM, 0.0, mv.data_ptr(), na.data_ptr(),
                           st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert _begin_reuse(eng, ps, _rows([spec.dump_key(d, 1)]), 3)[0] == 0
    _is_fresh(_dump(eng, 0), spec.dump_key(d, 1))

    d = searched()
    assert _begin_reuse(eng, ps, _rows([spec.dump_key(d, 1)]), 3)[0] == 1   # and the same root, kept
    _same_tree(_dump(eng, 0), spec.compact(d, 1))
    # a search that never reached end leaves nothing to keep
    assert _begin_reuse(eng, ps, _rows([spec.dump_key(d, 1)]), 3)[0] == 0

    with pytest.raises((_native.ZeroCloneError, ValueError)):
        _begin_reuse(eng, ps, r0, 1)                                   # sims < 2


def test_noise_on_a_kept_root(eng):
    from zeroclone_amd.valued import ChessPuctSearch
    n, sims, bs = 64, 33, 8
    kw = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25, seed=9)
    ps = ChessPuctSearch(eng, n, bs, reuse=True, **kw)
    states = [oracle.chess_from_fen(FENS[0])] * n
    seen = []
    for t in range(3):
        r = _rows([spec.key(s) for s in states])
        mv, _, st = ps.run(r, sims, hash_net)
        assert (st[:, 5] == 0).all()
        seen.append((r, ps.prior.cpu().numpy().copy(), ps.kept.cpu().numpy().copy(),
                     [len(oracle.chess_moves(s)) for s in states]))
        states = [oracle.chess_play(s, next(x for x in oracle.chess_moves(s) if x == decode(m)))
                  for s, m in zip(states, mv.cpu().numpy())]
    assert (seen[0][2] == 0).all() and (seen[1][2] > 0).all() and (seen[2][2] > 0).all()
    assert ps.search_no.cpu().tolist() == [3] * n
    # the reused search 1 against a fresh search of the same roots as search 1
    fresh = ChessPuctSearch(eng, n, bs, **kw)
    fresh.search_no.fill_(1)
    fresh.run(seen[1][0], sims, hash_net)
    np.testing.assert_allclose(seen[1][1], fresh.prior.cpu().numpy(), rtol=0, atol=1e-6)
    p = seen[1][1].astype(np.float64)
    np.testing.assert_allclose(p.sum(axis=1), 1.0, atol=1e-5)
    nm = np.array(seen[1][3])
    assert (np.sort(p, axis=1)[np.arange(n), 256 - nm] >= 0.75 / nm - 1e-6).all()   # uniform kept priors
    assert ((p > 0).sum(axis=1) == nm).all()
    # two consecutive reused searches of a game draw different noise
    assert all(not np.array_equal(seen[1][1][i], seen[2][1][i]) for i in range(n))


def _pool_steps(pool, steps, advance):
    """Per step: moves, root visits, kept, results, stats."""
    out = []
    for _ in range(steps):
        advance()
        torch.cuda.synchronize()
        out.append((pool.moves.cpu().clone(), pool.ps.na.cpu().clone(),
                    pool.ps.kept.cpu().clone() if pool.ps.kept is not None else None,
                    pool.results.cpu().clone(), pool.stats.cpu().clone()))
    return out


def _conv_net(seed):
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, PolicyValueNetwork
    torch.manual_seed(seed)
    return MfmaPolicyValueNetwork(PolicyValueNetwork(head="conv").eval())


G, SIMS, B, STEPS = 16, 33, 8, 8


def _reuse_pool(net, **kw):
    from zeroclone_amd.selfplay import ChessSelfPlay
    return ChessSelfPlay(G, SIMS, batch_size=B, seed=4, puct_net=net, reuse_tree=True, record_policy=True,
                         hist_cap=128, **kw)


@pytest.fixture(scope="module")
def eager_pool_run():
    """The reference run of the option tests: NHWC planes (the conv head's default), one
    stream, eager steps."""
    from zeroclone_amd import _native
    from zeroclone_amd.selfplay import ONGOING
    net = _conv_net(7)
    a = _reuse_pool(net)
    assert a.eng.max_sims == 2 * SIMS and a.ps.planes_nhwc and a.ps.reuse
    ea = _pool_steps(a, STEPS, a.step)
    for t, (mv, na, kept, res, st) in enumerate(ea):
        assert (st[:, 5] == 0).all()
        for s in range(G):
            if t == 0 or int(ea[t - 1][3][s]) != ONGOING:
                assert int(kept[s]) == 0
            assert int(st[s, 2]) == (SIMS - 1 if int(kept[s]) else SIMS)
            assert int(na[s].sum()) >= SIMS - 1 and (int(na[s].sum()) == SIMS - 1) == (int(kept[s]) <= 1)
    assert sum(int((k > 1).sum()) for _, _, k, _, _ in ea[1:]) >= G   # subtrees are kept
    assert int(a.traj.pctl[_native.ZC_TRAJ_PI_OVERFLOW]) & 4 == 0     # no count saturated
    final = (a.traj.slot_pi.cpu().clone(), a.traj.slot_off.cpu().clone(), a.roots.cpu().clone())
    a.close()
    return net, ea, final


def _equals_the_eager_run(b, advance, eager_pool_run):
    from zeroclone_amd import _native
    _, ea, final = eager_pool_run
    eb = _pool_steps(b, STEPS, advance)
    for x, y in zip(ea, eb):
        for u, v in zip(x, y):
            assert torch.equal(u, v)
    for u, v in zip(final, (b.traj.slot_pi.cpu(), b.traj.slot_off.cpu(), b.roots.cpu())):
        assert torch.equal(u, v)
    assert int(b.traj.pctl[_native.ZC_TRAJ_PI_OVERFLOW]) & 4 == 0
    b.close()


def test_selfplay_reuse_nchw_planes_equal_nhwc(eager_pool_run, monkeypatch):
    monkeypatch.setenv("ZC_PUCT_NHWC", "0")
    b = _reuse_pool(eager_pool_run[0])
    assert not b.ps.planes_nhwc
    _equals_the_eager_run(b, b.step, eager_pool_run)


def test_selfplay_reuse_two_streams_equal_one(eager_pool_run):
    b = _reuse_pool(eager_pool_run[0], puct_streams=2)
    assert isinstance(b.net_fn, list) and len(b.net_fn) == 2
    _equals_the_eager_run(b, b.step, eager_pool_run)


def test_selfplay_reuse_graph_equals_eager(eager_pool_run):
    b = _reuse_pool(eager_pool_run[0])
    g = b.capture_step()
    _equals_the_eager_run(b, g.replay, eager_pool_run)


def test_reuse_off_is_the_plain_pool():
    """reuse_tree=False against a pool built without the option: the same engine shape, launches
    and outputs (the begin and end kernels are shared with the reuse path)."""
    from zeroclone_amd.selfplay import ChessSelfPlay
    net = _conv_net(7)
    kw = dict(batch_size=B, seed=4, puct_net=net, record_policy=True, hist_cap=128)
    a = ChessSelfPlay(G, SIMS, reuse_tree=False, **kw)
    b = ChessSelfPlay(G, SIMS, **kw)
    assert a.eng.max_sims == SIMS and a.ps.kept is None and not a.ps.reuse
    ea, eb = _pool_steps(a, STEPS, a.step), _pool_steps(b, STEPS, b.step)
    for x, y in zip(ea, eb):
        assert (x[4][:, 2] == SIMS).all() and (x[1].sum(1) == SIMS - 1).all()
        for u, v in zip(x, y):
            assert u is v is None or torch.equal(u, v)
    assert torch.equal(a.traj.slot_pi, b.traj.slot_pi) and torch.equal(a.roots, b.roots)
    a.close()
    b.close()
