"""Root visit counts recorded with the self-play trajectories (zc_traj_policy_*): the sparse
per-position records against a recorder written here in plain Python, fed only with what a
caller sees — the slot table before each step, the search's `na` after it, the results (and,
for chess, the legal-move lists of the roots before the move)."""
import ctypes

import numpy as np
import pytest
import torch

from zeroclone_amd import _native
from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay, ONGOING, TrajBatch, simulate_games

pytestmark = pytest.mark.gpu

FIFTY_NEXT = "4k3/8/8/8/8/8/8/4K2R w K - 49 30"   # tests/test_gpu_chess_selfplay.py's
KQK = "8/8/4k3/8/8/8/3QK3/8 w - - 0 1"


class Recorder:
    """What the device recorder must hold: per game number, one list of (move id, Na) per
    position — the non-zero counts of the step's `na` row in row order, nothing for the last
    position."""

    def __init__(self, n_slots):
        self.cur = [[] for _ in range(n_slots)]
        self.done = {}

    def step(self, slot_before, na, results, root_moves=None):
        slot_before, na, results = slot_before.cpu().numpy(), na.cpu().numpy(), results.cpu().numpy()
        mv = root_moves.cpu().numpy().view(np.uint16) if root_moves is not None else None
        for g in range(len(self.cur)):
            game = int(slot_before[g, 1])
            if game < 0:
                continue
            self.cur[g].append([(int(mv[g, j]) if mv is not None else j, int(na[g, j]))
                                for j in range(na.shape[1]) if na[g, j] > 0])
            if int(results[g]) != ONGOING:
                self.done[game] = self.cur[g] + [[]]
                self.cur[g] = []


def entries(batch: TrajBatch):
    """Per row of a taken batch: [(move id, count)], from pi_off / pi."""
    off = batch.pi_off.cpu().numpy()
    pi = batch.pi.cpu().numpy().view(np.uint32)
    assert off.dtype == np.int64 and off.shape == (batch.rows.shape[0] + 1,)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(pi)
    return [[(int(e & 0xFFFF), int(e >> 16)) for e in pi[off[i]:off[i + 1]]] for i in range(len(off) - 1)]


def check_batch(batch: TrajBatch, rec: Recorder, sums=None):
    rows = entries(batch)
    games = batch.games.cpu().numpy().tolist()
    assert games
    for gno, _slot, _res, off, n in games:
        want = rec.done[gno]
        assert len(want) == n
        for i in range(n):
            assert rows[off + i] == want[i], (gno, i)
        assert rows[off + n - 1] == []
        if sums is not None:
            assert all(sum(c for _, c in rows[off + i]) == sums for i in range(n - 1))
    return rows


def same_batch(x: TrajBatch, y: TrajBatch):
    for f in ("rows", "labels", "moves", "games", "pi_off", "pi"):
        assert torch.equal(getattr(x, f), getattr(y, f)), f


# ---------------------------------------------------------------- Connect4, rollout search
@pytest.fixture(scope="module")
def c4_run():
    G, S, B, steps = 70, 32, 8, 42
    a = C4SelfPlay(G, S, batch_size=B, seed=11, record_policy=True)
    b = C4SelfPlay(G, S, batch_size=B, seed=11)
    rec = Recorder(G)
    for _ in range(steps):
        slot = a.traj.slot.clone()
        a.step_search()
        na = a.na.clone()
        rec.step(slot, na, a.step_finish().clone())
        b.step()
    torch.cuda.synchronize()
    out = {"a": a, "b": b, "rec": rec, "ba": a.take(), "bb": b.take(), "G": G, "S": S}
    yield out
    a.close()
    b.close()


def test_c4_rollout_entries_equal_the_na_rows(c4_run):
    """Every pooled position's entries are the non-zero (column, Na) pairs of the step's na
    row in column order; the row's sum is kept (the rollout search spends all its
    simulations at the root's moves); the last position of a game has none."""
    ba, rec = c4_run["ba"], c4_run["rec"]
    assert ba.games.shape[0] >= c4_run["G"]   # 42 steps: every slot finished a game
    rows = check_batch(ba, rec)
    assert max(sum(c for _, c in r) for r in rows) <= c4_run["S"]
    assert ba.pi.dtype == torch.int32 and ba.pi_off.dtype == torch.int64
    # dense targets of the same rows: count / sum per column
    dense = ba.policy_targets(7).cpu().numpy()
    for i, r in enumerate(rows):
        want = np.zeros(7, np.float32)
        tot = np.float32(sum(c for _, c in r))
        for m, c in r:
            want[m] = np.float32(c) / tot
        assert np.array_equal(dense[i], want)


def test_recording_off_is_unchanged(c4_run):
    """The twin pool without record_policy: identical trajectories, roots and RNG streams,
    and no policy fields."""
    a, b, ba, bb = c4_run["a"], c4_run["b"], c4_run["ba"], c4_run["bb"]
    for f in ("rows", "labels", "moves", "games"):
        assert torch.equal(getattr(ba, f), getattr(bb, f)), f
    assert bb.pi is None and bb.pi_off is None
    assert torch.equal(a.roots, b.roots)
    for g in (0, c4_run["G"] - 1):
        (ma, ia), (mb, ib) = a.eng.get_rng_state(g), b.eng.get_rng_state(g)
        assert ia == ib and np.array_equal(ma, mb)
    with pytest.raises(ValueError):
        bb.policy_targets(7)


def test_fused_launches_refuse_policy_recording(c4_run):
    a = c4_run["a"]
    with pytest.raises(ValueError):
        a.run(2)
    with pytest.raises(ValueError):
        a.run_pooled(8, 2)


# ---------------------------------------------------------------- chess
def chess_steps(sp: ChessSelfPlay, rec: Recorder, steps: int, na_of):
    mv = torch.zeros((sp.G, _native.CHESS_MAX_MOVES), dtype=torch.int16, device=sp.dev)
    cnt = torch.zeros(sp.G, dtype=torch.int32, device=sp.dev)
    for _ in range(steps):
        slot, roots = sp.traj.slot.clone(), sp.roots.clone()
        sp.eng.chess_legal_moves_async(sp.G, roots.data_ptr(), mv.data_ptr(), cnt.data_ptr(),
                                       torch.cuda.current_stream(sp.dev).cuda_stream)
        res = sp.step().clone()
        rec.step(slot, na_of(sp).clone(), res, mv.clone())


@pytest.mark.parametrize("fen,steps", [(KQK, 110), (FIFTY_NEXT, 3)])
def test_chess_crude_score_entries(fen, steps):
    """(packed move, Na > 0) in the order of zc_chess_legal_moves_async on the pre-move roots."""
    G, S, B = 6, 24, 8
    sp = ChessSelfPlay(G, S, batch_size=B, seed=3, init_fen=fen, hist_cap=128, record_policy=True)
    rec = Recorder(G)
    chess_steps(sp, rec, steps, lambda p: p.na)
    batch = sp.take()
    rows = check_batch(batch, rec)
    lens = batch.games[:, 4].cpu().numpy()
    if fen == FIFTY_NEXT:   # over after one move: exactly one searched position each
        assert batch.games.shape[0] == G * steps and (lens == 2).all()
        assert all(len(rows[2 * k]) > 0 and rows[2 * k + 1] == [] for k in range(G * steps))
    # the dense targets put each entry at from * 64 + to and nothing elsewhere
    dense = batch.policy_targets(4096).cpu().numpy()
    for i, r in enumerate(rows):
        want = np.zeros(4096, np.float32)
        tot = np.float32(sum(c for _, c in r))
        for m, c in r:
            want[(m & 63) * 64 + ((m >> 6) & 63)] = np.float32(c) / tot
        assert np.array_equal(dense[i], want), i
    sp.close()


# ---------------------------------------------------------------- PUCT pools, graphs
def _chess_pv_net(seed=0):
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, PolicyValueNetwork
    torch.manual_seed(seed)
    return MfmaPolicyValueNetwork(PolicyValueNetwork().eval())


def test_chess_puct_pool_and_graph_replay():
    net = _chess_pv_net(2)
    G, S, B = 16, 33, 16
    kw = dict(batch_size=B, seed=5, init_fen=FIFTY_NEXT, puct_net=net, hist_cap=128, record_policy=True)
    a, b = ChessSelfPlay(G, S, **kw), ChessSelfPlay(G, S, **kw)
    rec = Recorder(G)
    chess_steps(a, rec, 3, lambda p: p.ps.na)
    g = b.capture_step()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ba, bb = a.take(), b.take()
    check_batch(ba, rec, sums=None)
    assert ba.pi.numel() > 0
    same_batch(ba, bb)
    a.close()
    b.close()


def test_c4_puct_pool_and_graph_replay():
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, PolicyValueNetwork
    torch.manual_seed(0)
    pnet = MfmaPolicyValueNetwork(PolicyValueNetwork(in_planes=2, board=(6, 7), n_logits=7).eval())
    G, S, B = 32, 33, 16
    a = C4SelfPlay(G, S, batch_size=B, seed=4, puct_net=pnet, record_policy=True)
    b = C4SelfPlay(G, S, batch_size=B, seed=4, puct_net=pnet, record_policy=True)
    rec = Recorder(G)
    for _ in range(30):
        slot = a.traj.slot.clone()
        a.step_search()
        na = a.ps.na.clone()
        rec.step(slot, na, a.step_finish().clone())
    g = b.capture_step()
    for _ in range(30):
        g.replay()
    torch.cuda.synchronize()
    # the games in progress hold the same visit counts too
    assert torch.equal(a.traj.slot, b.traj.slot) and torch.equal(a.traj.slot_off, b.traj.slot_off)
    ba, bb = a.take(), b.take()
    check_batch(ba, rec)
    same_batch(ba, bb)
    a.close()
    b.close()


def test_c4_value_network_pool_adopts_a_rollout_pool():
    """The value-network search mode records its na too, and adopt() brings the visit counts of
    the games in progress along: their records continue across the hand-over."""
    from zeroclone_amd.nets import ValueNetwork, for_inference
    torch.manual_seed(0)
    vnet = for_inference(ValueNetwork(32, 2, in_planes=2).eval(), torch.device("cuda"), torch.float16)
    G, S, B = 16, 33, 16
    r = C4SelfPlay(G, S, batch_size=B, seed=6, record_policy=True)
    a = C4SelfPlay(G, S, batch_size=B, seed=6, net=vnet, record_policy=True)
    rec = Recorder(G)
    for pool, na_of, steps in ((r, lambda p: p.na, 5), (a, lambda p: p.vs.na, 40)):
        if pool is a:
            a.adopt(r)
        for _ in range(steps):
            slot = pool.traj.slot.clone()
            pool.step_search()
            na = na_of(pool).clone()
            rec.step(slot, na, pool.step_finish().clone())
    batch = a.take()
    rows = check_batch(batch, rec)
    lens = batch.games[:, 4].cpu().numpy()
    assert (lens > 6).all()   # the first games were 5 moves old when adopted
    assert all(len(rows[i]) > 0 for i in range(5))
    r.close()
    a.close()


# ---------------------------------------------------------------- quota, capacity
def test_simulate_games_grows_the_entry_pool():
    G, S, B, total = 8, 16, 8, 24
    sp = C4SelfPlay(G, S, batch_size=B, seed=9, games_cap=4, record_policy=True, pi_pool_cap=64)
    rec = Recorder(G)
    step = sp.step

    def recorded_step():
        slot = sp.traj.slot.clone()
        res = step()
        rec.step(slot, sp.na.clone(), res.clone())
        return res

    sp.step = recorded_step
    res = simulate_games(sp, total, max_steps=500)
    assert len(res) == total
    batch = sp.last_batch
    assert sorted(rec.done) == list(range(total))
    check_batch(batch, rec)
    assert batch.pi.numel() > 64 and sp.traj.pi_pool_cap >= batch.pi.numel()   # it had to grow
    sp.close()


def test_a_slot_history_too_small_is_flagged_not_overrun():
    G, S, B, cap = 8, 32, 8, 10
    sp = C4SelfPlay(G, S, batch_size=B, seed=2, record_policy=True, pi_slot_cap=cap)
    for _ in range(12):
        sp.step()
    torch.cuda.synchronize()
    assert sp.traj.slot_pi.shape == (G, cap)
    assert int(sp.traj.slot_off.max()) <= cap and int(sp.traj.slot_off.min()) >= 0
    assert int(sp.traj.pctl[_native.ZC_TRAJ_PI_OVERFLOW]) & 1
    with pytest.raises(RuntimeError, match="policy"):
        sp.take()
    sp.close()


# ---------------------------------------------------------------- dense kernel
def _dense(first, count, ent, width, dtype, n=None):
    dev = torch.device("cuda")
    f = torch.tensor(first, dtype=torch.int64, device=dev)
    c = torch.tensor(count, dtype=torch.int32, device=dev)
    e = torch.from_numpy(np.asarray(ent, np.uint32).view(np.int32)).to(dev)
    n = len(first) if n is None else n
    out = torch.full((n, width), 7.0, dtype=dtype, device=dev)   # not zeros: the kernel fills every cell
    rc = _native.lib().zc_traj_policy_dense_async(
        n, ctypes.c_void_p(f.data_ptr()), ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(e.data_ptr()), width,
        _native.ZC_F16 if dtype == torch.float16 else _native.ZC_F32, ctypes.c_void_p(out.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _move(fr, to, cap=0):
    return fr | (to << 6) | (cap << 12)


@pytest.mark.parametrize("width", [7, 4096])
def test_dense_targets_exact(width):
    """A hand-built CSR of 5 rows (one empty, rows out of storage order): f32 = float32(count)
    / float32(sum) exactly, f16 its round-to-nearest, every other cell exactly 0."""
    if width == 7:
        rows = [[(3, 5)], [], [(0, 1), (1, 2), (6, 30)], [(2, 65535), (4, 1)], [(c, c + 1) for c in range(7)]]
        index = lambda m: m  # noqa: E731
    else:
        rows = [[(_move(12, 28), 7), (_move(6, 21), 3)],
                [],
                [(_move(52, 36, 9), 11), (_move(36, 52, 5), 2), (_move(63, 0, 3), 1)],   # from != to, captures
                [(_move(0, 63), 65535), (_move(1, 2, 1), 1)],
                # more entries than a wave has lanes
                [(_move(k % 64, (k * 7 + 1 + 3 * (k // 64)) % 64, k % 10), k + 1) for k in range(70)]]
        index = lambda m: (m & 63) * 64 + ((m >> 6) & 63)  # noqa: E731
        assert len({index(m) for m, _ in rows[4]}) == 70
    order = [3, 0, 4, 1, 2]   # storage order of the rows' entries
    ent, first, count = [], [0] * 5, [0] * 5
    for r in order:
        first[r], count[r] = len(ent), len(rows[r])
        ent += [m | (c << 16) for m, c in rows[r]]
    want = np.zeros((5, width), np.float32)
    for i, r in enumerate(rows):
        tot = np.float32(sum(c for _, c in r))
        for m, c in r:
            want[i, index(m)] = np.float32(c) / tot
    rc, out = _dense(first, count, ent, width, torch.float32)
    assert rc == _native.ZC_OK and out.dtype == np.float32
    assert np.array_equal(out, want)
    assert (out[1] == 0).all() and np.count_nonzero(out) == sum(len(r) for r in rows)
    rc, out16 = _dense(first, count, ent, width, torch.float16)
    assert rc == _native.ZC_OK and out16.dtype == np.float16
    assert np.array_equal(out16, want.astype(np.float16))


def test_dense_targets_refuse_other_widths():
    rc, out = _dense([0], [1], [1 << 16], 8, torch.float32)
    assert rc == _native.ZC_EINVAL
    assert (out == 7.0).all()   # nothing was launched
