"""step() is step_search() then step_finish(): for both games and each of the three search
modes, two pools with the same seed played 3 moves, one by step() and one by the two halves,
hold the same positions, results, statistics, totals and trajectories."""
import pytest
import torch

from test_gpu_pool_replay import make_pool

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["c4_rollout", "c4_net", "c4_puct_temperature",
                                  "chess_crude", "chess_net", "chess_puct"])
def test_step_is_its_two_halves(name):
    a, b = make_pool(name), make_pool(name)
    try:
        for _ in range(3):
            ra = a.step()
            b.step_search()
            rb = b.step_finish()
            for f in ("roots", "results", "stats", "totals"):
                assert torch.equal(getattr(a, f), getattr(b, f)), f
            assert torch.equal(ra, rb)
        ta, tb = a.take(), b.take()
        for f in ("rows", "labels", "moves", "games"):
            assert torch.equal(getattr(ta, f), getattr(tb, f)), f
        for f in ("hist", "hmoves", "slot"):   # no Connect4 game ends in 3 moves: the histories in progress
            assert torch.equal(getattr(a.traj, f), getattr(b.traj, f)), f
    finally:
        a.close()
        b.close()
