"""GPU checks of the Connect4 PUCT search's tree reuse (zc_c4_puct_begin_reuse, c4_puct.hip's
re-root kernel) against its specification in tests/puct_reuse_ref.py: the re-rooted tree is
exactly the subtree, sequences of reused searches, the fresh-start rules, root noise on a kept
root, self-play eager = graph, and the option off."""
import numpy as np
import pytest
import torch

import oracle
from oracle import puct_ref
import puct_reuse_ref as spec
from test_gpu_c4_puct import POSITIONS, _c4_net, _hash_net, _hv, _roots

pytestmark = pytest.mark.gpu

M = 401   # nodes per tree of the shared engine (max_sims + 1)
FIELDS = ("s0", "s1", "order", "turn", "nmoves", "evaluated", "won", "parent", "pact", "depth", "child", "na", "pr",
          "w")


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=64, max_sims=400, max_batch=32)
    yield e
    e.close()


def _uniform(node):
    return [float(np.float32(1.0) / np.float32(len(node.moves)))] * len(node.moves)


def _rows(states):
    """[(s0, s1, turn)] -> zc_c4_state rows on the device."""
    a = np.array([[s0, s1, t] for s0, s1, t in states], dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).cuda()


def _state(d, i):
    return int(d["s0"][i]), int(d["s1"][i]), int(d["turn"][i])


def _slot_of(d, i, col):
    return [(int(d["order"][i]) >> (3 * k)) & 7 for k in range(int(d["nmoves"][i]))].index(col)


def _begin_reuse(eng, ps, roots, sims):
    """The re-root alone (no select follows): kept [n] on the host."""
    kept = torch.full((ps.n,), -1, dtype=torch.int32, device="cuda")
    eng.c4_puct_begin_reuse(0, ps.n, roots.data_ptr(), sims, ps.c, ps.bs, ps.alpha, ps.eps, ps.seed,
                            ps.search_no.data_ptr(), kept.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return kept.cpu().numpy()


def _same_records(got, want):
    assert len(got) == len(want)
    for f in FIELDS:   # na, w and pr bit for bit
        assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes(), f


def _is_fresh(d, state):
    assert len(d) == 1 and _state(d, 0) == state
    assert int(d["parent"][0]) == 0xFFFF and not int(d["evaluated"][0])
    assert (d["child"][0] == 0xFFFF).all() and (d["na"][0] == 0).all()


def _subtree_ids(d, r):
    """The old ids of r's subtree in a dump, ascending (a parent's id is below its child's)."""
    ids = []
    for i in range(r, len(d)):
        if i == r or int(d["parent"][i]) in ids:
            ids.append(i)
    return ids


def _check_reroot(eng, sims, bs, plies, next_sims):
    """A search of POSITIONS * 2, then the re-root alone (for a search of next_sims) at the chosen
    column's child, or at that child's most visited reply: the trees against spec.compact.
    Returns the nodes kept per game and the old ids they span."""
    from zeroclone_amd.valued import C4PuctSearch
    pos = POSITIONS * 2
    n = len(pos)
    ps = C4PuctSearch(eng, n, bs, dirichlet_eps=0.0, reuse=True)
    mv, _, st = ps.run(_roots(pos), sims, _hash_net)
    mv = mv.cpu().numpy()
    assert (st[:, 5] == 0).all() and (ps.kept == 0).all()
    dumps = [eng.debug_c4_puct_tree(g).copy() for g in range(n)]
    targets = []
    for g, d in enumerate(dumps):
        t = int(d["child"][0][_slot_of(d, 0, int(mv[g]))])   # the chosen column's child
        assert t != 0xFFFF
        if plies == 2:   # and its most visited reply that was expanded (ply 1 where there is none)
            ch = [(int(d["na"][t][k]), -k, int(c)) for k, c in enumerate(d["child"][t]) if int(c) != 0xFFFF]
            if ch:
                t = max(ch)[2]
        targets.append(t)
    kept = _begin_reuse(eng, ps, _rows([_state(d, t) for d, t in zip(dumps, targets)]), next_sims)
    moved, span = 0, []
    for g, (d, t) in enumerate(zip(dumps, targets)):
        after = eng.debug_c4_puct_tree(g)
        r = spec.find(d, *_state(d, t))
        if r is None:   # the move ended the game: nothing to keep
            assert int(d["nmoves"][t]) == 0 and kept[g] == 0
            _is_fresh(after, _state(d, t))
            continue
        assert r == t and int(d["depth"][t]) == plies
        want = spec.compact(d, r)
        assert len(want) + next_sims - 1 <= M
        assert kept[g] == len(want)
        _same_records(after, want)
        moved += len(want) > 1
        span.append(_subtree_ids(d, r)[-1] - r)
    assert moved >= 6   # most games kept a real subtree
    return kept, span


@pytest.mark.parametrize("plies", [1, 2])
@pytest.mark.parametrize("sims,bs", [(65, 8), (200, 32)])
def test_reroot_is_exactly_the_subtree(eng, sims, bs, plies):
    """By the spec on the CPU (c_puct 1.5, uniform priors) the searches of 200 simulations keep 58,
    43, 72, 25 and 58 nodes one ply down and 22, 18, 30, 0 and 11 two plies down, from old ids
    that span 83 or more: the kept records come from more than one 64-node chunk of the old tree."""
    kept, span = _check_reroot(eng, sims, bs, plies, sims)
    if sims == 200:
        assert max(span) > 64


def test_reroot_of_more_than_64_kept_nodes(eng):
    """A full tree (sims = max_sims = 400) re-rooted for a search of 2 simulations, so that the
    room rule lets a subtree of more than 64 nodes through: more than one chunk of new ids in the
    record move and the link pass.  By the spec on the CPU (c_puct 1.5, uniform priors) the five
    positions keep 109, 166, 184, 103 and 176 nodes one ply down."""
    kept, _ = _check_reroot(eng, 400, 32, 1, 2)
    assert max(kept) > 64


@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("sims,bs,c", [(65, 8, 1.5), (200, 32, 2.5), (40, 16, 0.7)])
def test_reused_search_sequence_matches_its_specification(eng, sims, bs, c, start):
    from zeroclone_amd.valued import C4PuctSearch
    ps = C4PuctSearch(eng, 1, bs, c_puct=c, dirichlet_eps=0.0, reuse=True)
    state, root, reused_searches = POSITIONS[start], None, 0
    for t in range(6):
        if not puct_ref.C4Rules.moves(state):
            break
        root, kept = spec.next_root(root, state, sims, M)
        kept_visits = sum(root.N)
        moves, N, best = spec.search(root, sims, bs, c, _hv, _uniform, reused=kept > 0)
        mv, na, st = ps.run(_roots([state]), sims, _hash_net)
        na, st = na.cpu().numpy(), st.cpu().numpy()
        assert st[0, 5] == 0
        assert int(ps.kept[0]) == kept, t
        assert [int(na[0, col]) for col in moves] == N, t
        assert int(mv[0]) == moves[best]
        assert int(na[0].sum()) == kept_visits + sims - 1 == sum(N)
        assert st[0, 2] == (sims - 1 if kept else sims)
        assert len(eng.debug_c4_puct_tree(0)) == spec.count_nodes(root) == (kept or 1) + st[0, 0]
        reused_searches += kept > 0
        state = oracle.play(state[0], state[1], moves[best])
    assert t >= 3 and reused_searches >= 2


def test_no_headroom_means_a_fresh_search():
    """max_sims = sims: a tree has sims + 1 nodes, so any kept subtree of 3 nodes or more leaves
    no room for the search's own and the game starts afresh: the plain begin's results."""
    from zeroclone_amd._native import NativeEngine
    from zeroclone_amd.valued import C4PuctSearch
    sims, bs = 65, 8
    e = NativeEngine(max_games=64, max_sims=sims, max_batch=32)
    pos = POSITIONS * 2
    n = len(pos)
    ps = C4PuctSearch(e, n, bs, dirichlet_eps=0.0, reuse=True)
    mv, _, _ = ps.run(_roots(pos), sims, _hash_net)
    nxt, big = [], []
    for g, (s, col) in enumerate(zip(pos, mv.cpu().tolist())):
        d = e.debug_c4_puct_tree(g)
        t = int(d["child"][0][_slot_of(d, 0, col)])
        big.append(int(d["nmoves"][t]) > 0 and len(spec.compact(d, t)) >= 3)
        nxt.append(oracle.play(s[0], s[1], col))
    assert sum(big) >= 6
    r = _roots(nxt)
    out = [x.cpu().clone() for x in ps.run(r, sims, _hash_net)] + [ps.prior.cpu().clone()]
    kept = ps.kept.cpu().numpy()
    plain = C4PuctSearch(e, n, bs, dirichlet_eps=0.0)
    ref = [x.cpu().clone() for x in plain.run(r, sims, _hash_net)] + [plain.prior.cpu().clone()]
    for g in range(n):
        if big[g]:
            assert kept[g] == 0
        if kept[g] == 0:
            for x, y in zip(out, ref):
                assert torch.equal(x[g], y[g]), g
    e.close()


def test_unvisited_move_unrelated_root_and_forget(eng):
    """sims 3, bs 2: the root and two walks, into the root's slots 0 and 1."""
    from zeroclone_amd.valued import C4PuctSearch
    ps = C4PuctSearch(eng, 1, 2, dirichlet_eps=0.0, reuse=True)
    r0 = _roots([POSITIONS[0]])

    def searched():
        ps.run(r0, 3, _hash_net)
        d = eng.debug_c4_puct_tree(0).copy()
        assert len(d) == 3 and [int(c) for c in d["child"][0][:3]] == [1, 2, 0xFFFF]
        return d

    d = searched()
    col = (int(d["order"][0]) >> (3 * 2)) & 7   # slot 2 was never walked
    bare = oracle.play(POSITIONS[0][0], POSITIONS[0][1], col)
    assert _begin_reuse(eng, ps, _roots([bare]), 3)[0] == 0
    after = eng.debug_c4_puct_tree(0)
    _is_fresh(after, _state(after, 0))
    assert _state(after, 0)[2] == 1 and bin(_state(after, 0)[0]).count("1") == 1

    searched()
    assert _begin_reuse(eng, ps, _roots([POSITIONS[4]]), 3)[0] == 0    # not in the tree
    assert len(eng.debug_c4_puct_tree(0)) == 1

    d = searched()
    assert _begin_reuse(eng, ps, r0, 3)[0] == 0                        # the same position again
    assert len(eng.debug_c4_puct_tree(0)) == 1

    d = searched()
    ps.forget()
    assert _begin_reuse(eng, ps, _rows([_state(d, 1)]), 3)[0] == 0     # forgotten
    _is_fresh(eng.debug_c4_puct_tree(0), _state(d, 1))

    d = searched()
    assert _begin_reuse(eng, ps, _rows([_state(d, 1)]), 3)[0] == 1     # and the same root, kept
    _same_records(eng.debug_c4_puct_tree(0), spec.compact(d, 1))
    # a search that never reached end leaves nothing to keep
    assert _begin_reuse(eng, ps, _rows([_state(d, 1)]), 3)[0] == 0

    from zeroclone_amd._native import ZeroCloneError
    with pytest.raises((ZeroCloneError, ValueError)):
        _begin_reuse(eng, ps, r0, 1)                                   # sims < 2


def test_noise_on_a_kept_root(eng):
    from zeroclone_amd.valued import C4PuctSearch
    n, sims, bs = 64, 33, 8
    kw = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25, seed=9)
    ps = C4PuctSearch(eng, n, bs, reuse=True, **kw)
    states = [POSITIONS[0]] * n
    seen = []
    for t in range(3):
        r = _roots(states)
        mv, _, st = ps.run(r, sims, _hash_net)
        assert (st[:, 5] == 0).all()
        seen.append((r, ps.prior.cpu().numpy().copy(), ps.kept.cpu().numpy().copy()))
        states = [oracle.play(b, s, int(col)) for (b, s), col in zip(states, mv.cpu().tolist())]
    assert (seen[0][2] == 0).all() and (seen[1][2] > 0).all() and (seen[2][2] > 0).all()
    assert ps.search_no.cpu().tolist() == [3] * n
    # the reused search 1 against a fresh search of the same roots as search 1
    fresh = C4PuctSearch(eng, n, bs, **kw)
    fresh.search_no.fill_(1)
    fresh.run(seen[1][0], sims, _hash_net)
    np.testing.assert_allclose(seen[1][1], fresh.prior.cpu().numpy(), rtol=0, atol=1e-6)
    p = seen[1][1].astype(np.float64)
    np.testing.assert_allclose(p.sum(axis=1), 1.0, atol=1e-5)
    assert (p.min(axis=1) >= 0.75 / 7 - 1e-6).all()       # seven legal columns, uniform kept priors
    # two consecutive reused searches of a game draw different noise (both over seven columns)
    assert all(not np.array_equal(seen[1][1][i], seen[2][1][i]) for i in range(n))


def _pool_steps(pool, steps, advance, played=None):
    """Per step: moves, root visits, kept, results, stats.  `played` (a list) also takes, per
    step and slot, the visits that the played move's node holds below it in the step's tree:
    what the next search of that game keeps at its root."""
    out = []
    for _ in range(steps):
        advance()
        torch.cuda.synchronize()
        out.append((pool.moves.cpu().clone(), pool.ps.na.cpu().clone(),
                    pool.ps.kept.cpu().clone() if pool.ps.kept is not None else None,
                    pool.results.cpu().clone(), pool.stats.cpu().clone()))
        if played is not None:
            row = []
            for s, col in enumerate(out[-1][0].tolist()):
                d = pool.eng.debug_c4_puct_tree(s, max_nodes=128)
                t = int(d["child"][0][_slot_of(d, 0, col)])
                row.append(int(d["na"][t][: int(d["nmoves"][t])].sum()) if t != 0xFFFF else 0)
            played.append(row)
    return out


def _slot_sums(traj):
    """Per slot, the visit sums of its game in progress' recorded positions."""
    slot, off, pi = traj.slot.cpu().numpy(), traj.slot_off.cpu().numpy(), traj.slot_pi.cpu().numpy().view(np.uint32)
    sums = []
    for g in range(traj.n):
        L = int(slot[g, 0])
        sums.append([int((pi[g, (off[g, i] if i else 0):off[g, i + 1]] >> 16).sum()) for i in range(L - 1)])
    return sums


def test_selfplay_reuse_graph_equals_eager():
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    from zeroclone_amd.selfplay import C4SelfPlay, ONGOING
    G, S, B, steps = 16, 33, 8, 12
    pnet = MfmaPolicyValueNetwork(_c4_net(seed=7))
    kw = dict(batch_size=B, seed=4, puct_net=pnet, reuse_tree=True, record_policy=True)
    a, b = C4SelfPlay(G, S, **kw), C4SelfPlay(G, S, **kw)
    assert a.eng.max_sims == 2 * S
    played = []
    ea = _pool_steps(a, steps, a.step, played)
    g = b.capture_step()
    eb = _pool_steps(b, steps, g.replay)
    for x, y in zip(ea, eb):
        for u, v in zip(x, y):
            assert torch.equal(u, v)
    assert torch.equal(a.traj.slot_pi, b.traj.slot_pi) and torch.equal(a.traj.slot_off, b.traj.slot_off)
    assert torch.equal(a.roots, b.roots)
    want = [[] for _ in range(G)]   # per slot: the visit sums of the game in progress
    for t, (mv, na, kept, res, st) in enumerate(ea):
        assert (st[:, 5] == 0).all()
        for s in range(G):
            refilled = t == 0 or int(ea[t - 1][3][s]) != ONGOING
            if refilled:
                assert int(kept[s]) == 0
                carried = 0
            else:
                assert int(kept[s]) > 0, (t, s)
                carried = played[t - 1][s]
                # at most the played move's visits less the node's own evaluation
                assert 0 <= carried <= int(ea[t - 1][1][s, int(ea[t - 1][0][s])]) - 1
            assert int(na[s].sum()) == carried + S - 1
            want[s].append(int(na[s].sum()))
            if int(res[s]) != ONGOING:
                want[s] = []
    assert _slot_sums(a.traj) == want
    if a.traj.finished():
        ba, bb = a.take(), b.take()
        for f in ("rows", "labels", "moves", "games", "pi_off", "pi"):
            assert torch.equal(getattr(ba, f), getattr(bb, f)), f
    a.close()
    b.close()


def test_reuse_off_is_the_plain_pool():
    """reuse_tree=False against a pool built without the option: the same engine shape, launches
    and outputs (the begin and end kernels are shared with the reuse path)."""
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    from zeroclone_amd.selfplay import C4SelfPlay
    G, S, B, steps = 16, 33, 8, 12
    pnet = MfmaPolicyValueNetwork(_c4_net(seed=7))
    a = C4SelfPlay(G, S, batch_size=B, seed=4, puct_net=pnet, record_policy=True, reuse_tree=False)
    b = C4SelfPlay(G, S, batch_size=B, seed=4, puct_net=pnet, record_policy=True)
    assert a.eng.max_sims == S and a.ps.kept is None and not a.ps.reuse
    ea, eb = _pool_steps(a, steps, a.step), _pool_steps(b, steps, b.step)
    for x, y in zip(ea, eb):
        assert (x[4][:, 2] == S).all() and (x[1].sum(1) == S - 1).all()
        for u, v in zip(x, y):
            assert u is v is None or torch.equal(u, v)
    assert torch.equal(a.traj.slot_pi, b.traj.slot_pi) and torch.equal(a.roots, b.roots)
    a.close()
    b.close()
