"""The arena pools against a reference arena built from the self-play pools alone
(tests/arena_ref.py: both networks on every row, selected with torch.where): the same games,
position for position, and the same tally; and an arena of one network against itself plays
exactly that network's self-play games."""
import pytest
import torch

import arena_ref
from arena_nets import ExactModel, integer_net, integer_pv_net
from zeroclone_amd.arena import ArenaResult, C4Arena, ChessArena
from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay, simulate_games

pytestmark = pytest.mark.gpu

KQK = "8/8/4k3/8/8/8/3QK3/8 w - - 0 1"   # short games: mates, stalemates, repetitions
SIMS, BS = 20, 8


def batch(pool):
    b = pool.last_batch
    return b.rows.cpu(), b.labels.cpu(), b.moves.cpu(), b.games.cpu()


def same_games(got, want):
    for name, x, y in zip(("rows", "labels", "moves", "games"), got, want):
        assert torch.equal(x, y), name


def check_against_reference(arena, ref, total):
    res = arena.play(total, max_steps=2000)
    want = arena_ref.play(ref, total)
    same_games(batch(arena), want)
    games = want[3]
    assert res == ArenaResult.tally(games[:, 2].tolist(), games[:, 0].tolist())
    assert games[:, 0].tolist() == list(range(total))
    assert sum(res.first) == total // 2 and sum(res.second) == total - total // 2 and res.games == total
    assert arena.mixed_steps > 0, "no step had games of both networks: the comparison shows nothing"
    arena.check()
    arena.close()
    ref.close()
    return res


@pytest.mark.parametrize("puct", [False, True], ids=["value", "puct"])
def test_c4_arena_equals_the_reference_arena(puct):
    nl = 7 if puct else 0
    a, b = ExactModel(11, nl), ExactModel(23, nl)
    nets = dict(puct_net_a=a, puct_net_b=b) if puct else dict(net_a=a, net_b=b)
    arena = C4Arena(8, SIMS, batch_size=BS, seed=3, **nets)
    ref = arena_ref.reference_arena("c4", 8, SIMS, a, b, puct, batch_size=BS, seed=3)
    res = check_against_reference(arena, ref, 20)
    assert sum(res.first) == 10 and sum(res.second) == 10


@pytest.mark.parametrize("puct", [False, True], ids=["value", "puct"])
def test_chess_arena_equals_the_reference_arena(puct):
    nl = 4096 if puct else 0
    a, b = ExactModel(11, nl), ExactModel(23, nl)
    nets = dict(puct_net_a=a, puct_net_b=b) if puct else dict(net_a=a, net_b=b)
    kw = dict(batch_size=BS, seed=5, init_fen=KQK, hist_cap=128)
    arena = ChessArena(4, SIMS, **nets, **kw)
    ref = arena_ref.reference_arena("chess", 4, SIMS, a, b, puct, **kw)
    check_against_reference(arena, ref, 8)


def test_c4_arena_of_one_network_plays_its_self_play_games():
    net = integer_net(2, 5)
    arena = C4Arena(8, SIMS, batch_size=BS, seed=9, net_a=net, net_b=net)
    pool = C4SelfPlay(8, SIMS, batch_size=BS, seed=9, net=net)
    arena.play(20, max_steps=2000)
    simulate_games(pool, 20, max_steps=2000)
    same_games(batch(arena), batch(pool))
    assert arena.mixed_steps > 0
    arena.close()
    pool.close()


def test_chess_puct_arena_of_one_network_plays_its_self_play_games():
    """The convolutional head: the planes in the tower's layout (4096-byte rows) and 8192-byte
    logit rows through the gather and the scatter; temperature and root noise as the pool's."""
    net = integer_pv_net(17, 8, 8, 4096, 5, "conv")
    kw = dict(batch_size=BS, seed=7, init_fen=KQK, hist_cap=128)
    arena = ChessArena(4, SIMS, puct_net_a=net, puct_net_b=net, temperature=1.0, dirichlet_eps=0.25, **kw)
    pool = ChessSelfPlay(4, SIMS, puct_net=net, temperature=1.0, **kw)
    assert arena.ps.planes_nhwc and arena.ps.eps == pool.ps.eps == 0.25 and arena.ps.c == pool.ps.c
    arena.play(8, max_steps=2000)
    simulate_games(pool, 8, max_steps=2000)
    same_games(batch(arena), batch(pool))
    assert arena.mixed_steps > 0
    arena.check()
    arena.close()
    pool.close()


def test_puct_arena_defaults_and_capture_refusal():
    a, b = ExactModel(1, 7), ExactModel(2, 7)
    arena = C4Arena(4, SIMS, batch_size=BS, puct_net_a=a, puct_net_b=b)
    assert arena.temperature == 0.0 and arena.ps.eps == 0.0
    with pytest.raises(ValueError):
        arena.capture_step()
    with pytest.raises(ValueError):
        arena.run(2)
    arena.close()
    over = C4Arena(4, SIMS, batch_size=BS, puct_net_a=a, puct_net_b=b, temperature=0.5, dirichlet_eps=0.1, c_puct=2.0)
    assert over.temperature == 0.5 and over.ps.eps == 0.1 and over.ps.c == 2.0
    over.close()
