"""Root visit counts recorded by the fused self-play launches (fused_policy=True:
zc_c4_selfplay_visits / zc_chess_selfplay_visits + zc_traj_policy_record_steps_async) against
the same moves played and recorded with step(): whole batches bit for bit where the schedules
agree (run()), per slot and game where they do not (run_pooled(), carry, drain())."""
import ctypes

import numpy as np
import pytest
import torch

from zeroclone_amd import _native
from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay, TrajBatch

pytestmark = pytest.mark.gpu

FIFTY_NEXT = "4k3/8/8/8/8/8/8/4K2R w K - 49 30"   # tests/test_gpu_chess_selfplay.py's
KQK = "8/8/4k3/8/8/8/3QK3/8 w - - 0 1"
C4 = dict(batch_size=8, seed=11)
CHESS = dict(batch_size=8, seed=3, hist_cap=128)
G, S, STEPS = 70, 16, 90


def same_batch(x: TrajBatch, y: TrajBatch):
    for f in ("rows", "labels", "moves", "games", "pi_off", "pi"):
        assert torch.equal(getattr(x, f), getattr(y, f)), f


def csr(pool):
    """The slots' policy records as the device holds them: slot table, offsets, each slot's
    entries up to its game's fill, the counters."""
    t = pool.traj
    torch.cuda.synchronize()
    slot, off, pi = t.slot.cpu().numpy(), t.slot_off.cpu().numpy(), t.slot_pi.cpu().numpy()
    fill = [int(off[g, slot[g, 0] - 1]) for g in range(t.n)]
    return {"slot": slot[:, :2].copy(), "off": off, "pi": [pi[g, :fill[g]].copy() for g in range(t.n)],
            "pctl": t.pctl.cpu().numpy().copy(), "ctl": t.ctl.cpu().numpy().copy()}


def same_csr(x, y):
    assert np.array_equal(x["slot"], y["slot"])
    assert np.array_equal(x["off"], y["off"])
    assert all(np.array_equal(a, b) for a, b in zip(x["pi"], y["pi"]))
    assert np.array_equal(x["pctl"], y["pctl"]) and np.array_equal(x["ctl"], y["ctl"])


def slot_games(pool, batches):
    """Per slot, the games it played in order: (rows, moves, result, entries per position) of
    every finished game of `batches` (taken in order), then its game in progress (result None,
    entries of the searched positions only)."""
    out = [[] for _ in range(pool.G)]
    for b in batches:
        rows, moves, labels = b.rows.cpu().numpy(), b.moves.cpu().numpy(), b.labels.cpu().numpy()
        off, pi = b.pi_off.cpu().numpy(), b.pi.cpu().numpy()
        for _gno, slot, res, first, n in b.games.cpu().numpy().tolist():
            ents = [pi[off[i]:off[i + 1]] for i in range(first, first + n)]
            assert len(ents[-1]) == 0   # a game's last position was never searched
            out[slot].append((rows[first:first + n], moves[first:first + n], (res, labels[first:first + n]), ents))
    t = pool.traj
    torch.cuda.synchronize()
    slot, hist, hmv = t.slot.cpu().numpy(), t.hist.cpu().numpy(), t.hmoves.cpu().numpy()
    off, pi = t.slot_off.cpu().numpy(), t.slot_pi.cpu().numpy()
    for g in range(pool.G):
        n = int(slot[g, 0])
        ents = [pi[g, (off[g, i] if i else 0):off[g, i + 1]] for i in range(n - 1)]
        out[g].append((hist[g, :n], hmv[g, :n - 1], None, ents))
    return out


def same_per_slot(got, want):
    """Every game a slot finished equals the twin's game of the same place in that slot; its
    game in progress is a prefix of the twin's next one."""
    finished = 0
    for g, (mine, twin) in enumerate(zip(got, want)):
        assert len(mine) <= len(twin), g
        for j, (rows, moves, res, ents) in enumerate(mine):
            trows, tmoves, tres, tents = twin[j]
            if res is not None:
                assert tres is not None, (g, j)   # the twin played long enough to finish it too
                assert res[0] == tres[0] and np.array_equal(res[1], tres[1]), (g, j)
                assert np.array_equal(rows, trows) and np.array_equal(moves, tmoves), (g, j)
                assert len(ents) == len(tents) and all(np.array_equal(a, b) for a, b in zip(ents, tents)), (g, j)
                finished += 1
            else:
                n = len(rows)
                assert j == len(mine) - 1 and n <= len(trows), (g, j)
                assert np.array_equal(rows, trows[:n]) and np.array_equal(moves, tmoves[:n - 1]), (g, j)
                assert all(np.array_equal(a, b) for a, b in zip(ents, tents[:n - 1])), (g, j)
    return finished


# ---------------------------------------------------------------- Connect4
@pytest.fixture(scope="module")
def c4_twin():
    """The lockstep twin: 90 x step() (batch and CSR kept), then 40 more steps so that it
    finishes every game a pooled schedule of the tests below can finish."""
    b = C4SelfPlay(G, S, record_policy=True, **C4)
    for _ in range(STEPS):
        b.step()
    out = {"csr": csr(b), "roots": b.roots.clone(), "rng": [b.eng.get_rng_state(g) for g in (0, G - 1)]}
    out["batch"] = b.take()
    for _ in range(40):
        b.step()
    out["games"] = slot_games(b, [out["batch"], b.take()])
    b.close()
    return out


def test_c4_run_equals_steps(c4_twin):
    a = C4SelfPlay(G, S, record_policy=True, fused_policy=True, **C4)
    a.run(STEPS)
    same_csr(csr(a), c4_twin["csr"])
    assert torch.equal(a.roots, c4_twin["roots"])
    ba = a.take()
    same_batch(ba, c4_twin["batch"])
    per_slot = np.bincount(ba.games[:, 1].cpu().numpy(), minlength=G)
    assert per_slot.min() >= 2   # a game has at most 42 moves: the multi-finish path in every slot
    assert ba.pi.numel() > 0 and int(a.traj.pctl[_native.ZC_TRAJ_PI_OVERFLOW]) == 0
    a.close()


def test_c4_steps_and_runs_interleave(c4_twin):
    a = C4SelfPlay(G, S, record_policy=True, fused_policy=True, **C4)
    a.run(7)
    for _ in range(3):
        a.step()
    a.run(80)
    same_csr(csr(a), c4_twin["csr"])
    same_batch(a.take(), c4_twin["batch"])
    a.close()


def test_c4_pooled_equals_steps_per_slot(c4_twin):
    a = C4SelfPlay(G, S, record_policy=True, fused_policy=True, **C4)
    a.run_pooled(G * 30, STEPS)
    ba = a.take()
    got = slot_games(a, [ba])
    # every ticket below the budget is a move played (70 x 90 > the budget: no slot runs out of steps)
    assert sum(len(rows) - 1 for games in got for rows, _, _, _ in games) == G * 30
    assert same_per_slot(got, c4_twin["games"]) == ba.games.shape[0] > 0
    assert int(a.traj.ctl[_native.ZC_TRAJ_OVERFLOW]) == 0 and int(a.traj.pctl[_native.ZC_TRAJ_PI_OVERFLOW]) == 0
    a.close()


def test_c4_carry_and_drain_equal_steps_per_slot(c4_twin):
    a = C4SelfPlay(G, S, record_policy=True, fused_policy=True, **C4)
    batches = []
    for _ in range(3):
        a.run_pooled(G * 10, 40, carry=True)
        batches.append(a.take())
    a.drain()
    batches.append(a.take())
    got = slot_games(a, batches)
    played = sum(len(rows) - 1 for games in got for rows, _, _, _ in games)
    # every ticket below a budget is a move played: finished in its launch, or suspended and
    # finished by the next launch or the drain, which starts none
    assert played == 3 * G * 10
    assert same_per_slot(got, c4_twin["games"]) == sum(b.games.shape[0] for b in batches) > 0
    assert int(a.traj.pctl[_native.ZC_TRAJ_PI_OVERFLOW]) == 0
    a.close()


def test_c4_switch_off_is_inert(c4_twin):
    """A pool without record_policy plays and records run(90) exactly as the fused-policy pool
    and the lockstep twin do: positions, games, roots, RNG streams."""
    x = C4SelfPlay(G, S, **C4)
    a = C4SelfPlay(G, S, record_policy=True, fused_policy=True, **C4)
    rx, ra = x.run(STEPS).clone(), a.run(STEPS).clone()
    assert torch.equal(rx, ra)
    assert torch.equal(x.roots, a.roots) and torch.equal(x.roots, c4_twin["roots"])
    assert torch.equal(x.stats, a.stats)
    bx, ba = x.take(), a.take()
    for f in ("rows", "labels", "moves", "games"):
        assert torch.equal(getattr(bx, f), getattr(ba, f)), f
        assert torch.equal(getattr(bx, f), getattr(c4_twin["batch"], f)), f
    assert bx.pi is None and bx.pi_off is None
    for k, g in enumerate((0, G - 1)):
        (mx, ix), (ma, ia), (mt, it) = x.eng.get_rng_state(g), a.eng.get_rng_state(g), c4_twin["rng"][k]
        assert ix == ia == it and np.array_equal(mx, ma) and np.array_equal(mx, mt)
    x.close()
    a.close()


def test_a_launch_longer_than_the_staging_is_refused():
    """Raw ABI: moves > steps_cap returns ZC_EINVAL and nothing is enqueued; NULL switches the
    output off again."""
    n, moves = 8, 3
    a = C4SelfPlay(n, S, **C4)
    dev = a.dev
    na = torch.full((2, n, 7), -7, dtype=torch.int32, device=dev)
    states = torch.zeros((moves, n, 3), dtype=torch.int64, device=dev)
    mv = torch.full((moves, n), -5, dtype=torch.int16, device=dev)
    res = torch.full((moves, n), -5, dtype=torch.int32, device=dev)
    ticket = torch.zeros(2, dtype=torch.int32, device=dev)
    a.eng.c4_selfplay_visits(na.data_ptr(), 2)
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    head = (a.eng._h, 0, n, ctypes.c_void_p(a.roots.data_ptr()), S, 1.4, 8, moves)
    outs = (ctypes.c_void_p(states.data_ptr()), ctypes.c_void_p(mv.data_ptr()), ctypes.c_void_p(res.data_ptr()),
            ctypes.c_void_p(a.stats.data_ptr()), s)
    L = _native.lib()
    assert L.zc_c4_selfplay_async(*head, *outs) == _native.ZC_EINVAL
    for fn in (L.zc_c4_selfplay_pooled_async, L.zc_c4_selfplay_carry_async):
        assert fn(*head, n, ctypes.c_void_p(ticket.data_ptr()), *outs) == _native.ZC_EINVAL
    torch.cuda.synchronize()
    assert (na == -7).all() and (mv == -5).all() and (res == -5).all() and not a.roots.any()
    a.eng.c4_selfplay_visits(None)
    assert L.zc_c4_selfplay_async(*head, *outs) == _native.ZC_OK
    torch.cuda.synchronize()
    assert (na == -7).all() and (res != -5).all()
    a.close()


def test_c4_more_slots_than_a_scan_workgroup():
    """1100 slots: the recorder's row scans walk the slots 1024 at a time, so a step's games
    take their places across two rounds of the workgroup."""
    n, steps = 1100, 50
    kw = dict(batch_size=8, seed=5, record_policy=True)
    a, b = C4SelfPlay(n, 8, fused_policy=True, **kw), C4SelfPlay(n, 8, **kw)
    a.run(steps)
    for _ in range(steps):
        b.step()
    same_csr(csr(a), csr(b))
    ba, bb = a.take(), b.take()
    same_batch(ba, bb)
    assert np.bincount(ba.games[:, 1].cpu().numpy(), minlength=n).min() >= 1   # 50 > 42 moves
    a.close()
    b.close()


def test_a_game_the_trajectory_pool_drops_reserves_no_entries():
    """games_cap 4 with 8 slots: the position pool overflows in both schedules, and the entry
    pool holds the same entries at the same places for the games that were taken."""
    kw = dict(batch_size=8, seed=7, record_policy=True, games_cap=4)
    a, b = C4SelfPlay(8, S, fused_policy=True, **kw), C4SelfPlay(8, S, **kw)
    a.run(60)
    for _ in range(60):
        b.step()
    ca, cb = csr(a), csr(b)
    assert cb["ctl"][_native.ZC_TRAJ_OVERFLOW] & 1 and cb["ctl"][_native.ZC_TRAJ_GAMES] > 4   # games were dropped
    same_csr(ca, cb)
    for f in ("pool_pi", "pool_first", "pool_count", "games", "labels", "pool_moves"):
        assert torch.equal(getattr(a.traj, f), getattr(b.traj, f)), f
    with pytest.raises(RuntimeError, match="overflow"):
        a.take()
    a.close()
    b.close()


# ---------------------------------------------------------------- chess
@pytest.fixture(scope="module")
def kqk_twin():
    b = ChessSelfPlay(6, 32, init_fen=KQK, record_policy=True, **CHESS)
    for _ in range(12):
        b.step()
    out = {"csr": csr(b), "roots": b.roots.clone()}
    out["batch"] = b.take()
    out["games"] = slot_games(b, [out["batch"]])
    b.check()
    b.close()
    return out


def test_chess_run_equals_steps(kqk_twin):
    a = ChessSelfPlay(6, 32, init_fen=KQK, record_policy=True, fused_policy=True, **CHESS)
    a.run(12)
    same_csr(csr(a), kqk_twin["csr"])
    assert torch.equal(a.roots, kqk_twin["roots"])
    assert sum(len(p) for p in kqk_twin["csr"]["pi"]) > 0   # games in progress hold entries
    ba = a.take()
    same_batch(ba, kqk_twin["batch"])
    if ba.rows.shape[0]:
        assert torch.equal(ba.policy_targets(4096), kqk_twin["batch"].policy_targets(4096))
    a.close()


def test_chess_every_slot_finishes_at_every_step():
    kw = dict(init_fen=FIFTY_NEXT, record_policy=True, **CHESS)
    a, b = ChessSelfPlay(6, 32, fused_policy=True, **kw), ChessSelfPlay(6, 32, **kw)
    a.run(5)
    for _ in range(5):
        b.step()
    same_csr(csr(a), csr(b))
    ba, bb = a.take(), b.take()
    assert ba.games.shape[0] == 6 * 5 and (ba.games[:, 4] == 2).all()
    same_batch(ba, bb)
    assert ba.pi.numel() > 0
    dense = ba.policy_targets(4096)
    assert torch.equal(dense, bb.policy_targets(4096))
    assert torch.equal(dense.sum(1) > 0, ba.moves >= 0)   # targets exactly at the searched positions
    a.close()
    b.close()


def test_chess_pooled_equals_steps_per_slot(kqk_twin):
    a = ChessSelfPlay(6, 32, init_fen=KQK, record_policy=True, fused_policy=True, **CHESS)
    a.run_pooled(40, 12)
    got = slot_games(a, [a.take()])
    same_per_slot(got, kqk_twin["games"])
    assert sum(len(rows) - 1 for games in got for rows, _, _, _ in games) == 40
    assert int(a.traj.pctl[_native.ZC_TRAJ_PI_OVERFLOW]) == 0
    a.check()
    a.close()


def test_chess_launch_longer_than_the_staging_is_refused():
    a = ChessSelfPlay(6, 32, init_fen=KQK, **CHESS)
    na = torch.full((2, 6, _native.CHESS_MAX_MOVES), -7, dtype=torch.int32, device=a.dev)
    mv = torch.zeros((2, 6, _native.CHESS_MAX_MOVES), dtype=torch.int16, device=a.dev)
    a.eng.chess_selfplay_visits(na.data_ptr(), mv.data_ptr(), 2)
    roots = a.roots.clone()
    for launch in (lambda: a.run(3), lambda: a.run_pooled(6, 3)):
        with pytest.raises(ValueError, match="staging"):
            launch()
    torch.cuda.synchronize()
    assert (na == -7).all() and torch.equal(a.roots, roots)
    a.run(2)   # fits: the rows of both steps are written
    torch.cuda.synchronize()
    assert (na.sum(2) > 0).all() and (na >= 0).all() and (mv[na > 0] != 0).all()
    a.eng.chess_selfplay_visits(None)
    a.run(3)
    a.check()
    a.close()


# ---------------------------------------------------------------- overflow
def test_entry_pool_too_small_raises_at_take():
    a = C4SelfPlay(G, S, record_policy=True, fused_policy=True, pi_pool_cap=64, **C4)
    a.run(STEPS)
    torch.cuda.synchronize()
    assert int(a.traj.pctl[_native.ZC_TRAJ_PI_OVERFLOW]) & 2
    with pytest.raises(RuntimeError, match="policy"):
        a.take()
    a.close()


def test_slot_history_too_small_is_flagged_not_overrun():
    cap = 10
    a = C4SelfPlay(8, 32, batch_size=8, seed=2, record_policy=True, fused_policy=True, pi_slot_cap=cap)
    a.run(12)
    torch.cuda.synchronize()
    assert a.traj.slot_pi.shape == (8, cap)
    assert int(a.traj.slot_off.max()) <= cap and int(a.traj.slot_off.min()) >= 0
    assert int(a.traj.pctl[_native.ZC_TRAJ_PI_OVERFLOW]) & 1
    with pytest.raises(RuntimeError, match="policy"):
        a.take()
    a.close()
