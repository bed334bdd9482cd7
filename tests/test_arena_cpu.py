"""The arena's host side: the route kernel's executable specification, the tally of a match and
the pools' refusals (raised before an engine exists, so no GPU is needed)."""
import numpy as np
import pytest

from zeroclone_amd.arena import ArenaResult, C4Arena, ChessArena, route_ref

SIZES = (1, 64, 65, 1000)


def keys(pattern: str, n: int) -> np.ndarray:
    if pattern == "zeros":
        return np.zeros(n, np.int32)
    if pattern == "ones":
        return np.ones(n, np.int32)
    if pattern == "alternating":
        return (np.arange(n) & 1).astype(np.int32)
    return np.random.default_rng(n).integers(0, 2, n).astype(np.int32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", ["zeros", "ones", "alternating", "random"])
def test_route_ref_is_the_stable_partition(pattern, n):
    key = keys(pattern, n)
    perm, counts = route_ref(key)
    assert perm.dtype == np.int32 and counts.dtype == np.int32
    assert sorted(perm.tolist()) == list(range(n))                      # a permutation
    n0 = int((key == 0).sum())
    assert counts.tolist() == [n0, n - n0]                             # the counts
    assert (key[perm[:n0]] == 0).all() and (key[perm[n0:]] == 1).all()  # the groups
    assert (np.diff(perm[:n0]) > 0).all() and (np.diff(perm[n0:]) > 0).all()   # stable


def test_route_ref_reads_bit_0_only():
    key = keys("random", 1000)
    junk = key | (np.random.default_rng(1).integers(0, 1 << 30, 1000).astype(np.int32) << 1)
    junk[::7] |= np.int32(-2)   # the sign bit too
    assert (junk & 1 == key).all()
    for got, want in zip(route_ref(junk), route_ref(key)):
        assert np.array_equal(got, want)


def test_tally_of_an_odd_number_of_games():
    """Games 0..6: A moves first in the odd ones (1, 3, 5: N // 2 = 3) and second in the even
    ones (0, 2, 4, 6: N - N // 2 = 4).  +1 = the first mover won."""
    #          game 0   1   2   3   4   5   6
    results = [+1, +1, -1, 0, 0, -1, +1]
    r = ArenaResult.tally(results)
    assert r.first == (1, 1, 1)     # games 1 (+1: won), 3 (draw), 5 (-1: lost)
    assert r.second == (1, 1, 2)    # games 2 (-1: won), 4 (draw), 0 and 6 (+1: lost)
    assert sum(r.first) == 7 // 2 and sum(r.second) == 7 - 7 // 2 and r.games == 7
    assert r.score == (2 + 0.5 * 2) / 7


def test_tally_of_draws_is_one_half():
    r = ArenaResult.tally([0] * 9)
    assert r.first == (0, 4, 0) and r.second == (0, 5, 0) and r.score == 0.5


def test_the_same_result_is_a_win_in_one_colour_and_a_loss_in_the_other():
    assert ArenaResult.tally([+1, +1]) == ArenaResult((1, 0, 0), (0, 0, 1))
    assert ArenaResult.tally([-1, -1]) == ArenaResult((0, 0, 1), (1, 0, 0))
    assert ArenaResult.tally([+1, +1]).score == 0.5 == ArenaResult.tally([-1, -1]).score
    # the colours go by game number, not by the list's order
    assert ArenaResult.tally([+1, +1], game_numbers=[3, 5]) == ArenaResult((2, 0, 0), (0, 0, 0))
    assert ArenaResult.tally([+1, +1], game_numbers=[4, 2]).score == 0.0
    with pytest.raises(ValueError):
        ArenaResult.tally([2])


def test_score_is_evaluate_pairs_weighted_mean():
    """evaluate_pair: (wr_first * g_first + wr_second * g_second) / games, each colour's
    win rate (wins + 0.5 * draws) / its games."""
    r = ArenaResult((5, 2, 3), (4, 4, 3))
    wr_first, wr_second = (5 + 1.0) / 10, (4 + 2.0) / 11
    assert r.score == pytest.approx((wr_first * 10 + wr_second * 11) / 21, rel=1e-15)


NETS = [dict(net_a=object(), net_b=object()), dict(puct_net_a=object(), puct_net_b=object())]


@pytest.mark.parametrize("arena", [C4Arena, ChessArena])
@pytest.mark.parametrize("nets", NETS, ids=["value", "puct"])
def test_refusals_need_no_engine(arena, nets):
    streams = "streams" if arena is C4Arena or "net_a" in nets else "puct_streams"
    for bad in ({"reuse_tree": True}, {"record_policy": True}, {streams: 2}):
        with pytest.raises(ValueError):
            arena(8, 20, batch_size=8, **nets, **bad)


@pytest.mark.parametrize("arena", [C4Arena, ChessArena])
def test_an_arena_needs_two_networks_of_one_search(arena):
    for nets in ({}, {"net_a": object()}, {"puct_net_b": object()},
                 {"net_a": object(), "net_b": object(), "puct_net_a": object(), "puct_net_b": object()},
                 {"net_a": object(), "puct_net_b": object()}):
        with pytest.raises(ValueError):
            arena(8, 20, batch_size=8, **nets)
