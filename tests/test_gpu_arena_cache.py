"""The arena pools with an evaluation cache per network (arena.py eval_cache= / eval_merge=,
evalcache.RoutedCachedValue / RoutedCachedPolicy): the cached arena plays the plain arena's games
bit for bit — the networks are integer MFMA networks, exact whatever batch they see — each
network hits its own table alone, and a step of the cached arena replays from a graph.

The plain arena's games are played once per configuration and shared (PLAIN below)."""
import pytest
import torch

from arena_nets import integer_net, integer_pv_net
from test_gpu_arena_pool import BS, KQK, SIMS, batch, same_games
from test_gpu_eval_cache import _pool_state
from zeroclone_amd.arena import C4Arena, ChessArena
from zeroclone_amd.selfplay import C4SelfPlay, simulate_games

pytestmark = pytest.mark.gpu

SEEDS = (5, 6)              # the two integer networks of every configuration
ENTRIES = 1 << 16           # nothing is evicted at these sizes
KINDS = ["c4_value", "c4_puct", "chess_value", "chess_puct"]
SWITCHES = {"cache": dict(eval_cache=ENTRIES), "merge": dict(eval_merge=True),
            "both": dict(eval_cache=ENTRIES, eval_merge=True)}
TOTAL = {"c4": 20, "chess": 8}


def _net(kind, seed, channels=128):
    if kind == "c4_value":
        return integer_net(2, seed, channels)
    if kind == "c4_puct":
        return integer_pv_net(2, 6, 7, 7, seed, channels=channels)
    if kind == "chess_value":
        return integer_net(17, seed, channels)
    return integer_pv_net(17, 8, 8, 4096, seed, "conv", channels)


def _arena(kind, a, b, **kw):
    nets = dict(puct_net_a=a, puct_net_b=b) if kind.endswith("puct") else dict(net_a=a, net_b=b)
    if kind.startswith("c4"):
        return C4Arena(8, SIMS, batch_size=BS, seed=3, **nets, **kw)
    return ChessArena(4, SIMS, batch_size=BS, seed=5, init_fen=KQK, hist_cap=128, **nets, **kw)


def _play(kind, a, b, **kw):
    arena = _arena(kind, a, b, **kw)
    res = arena.play(TOTAL[kind.split("_")[0]], max_steps=2000)
    out = dict(games=batch(arena), result=res, mixed=arena.mixed_steps, steps=arena.steps)
    if kw:
        out["stats"] = arena.eval_cache_stats(by_network=True)
        out["sum"] = arena.eval_cache_stats()
    arena.check()
    arena.close()
    return out


_nets, _plain = {}, {}


SAME = (128, 128)           # the channels of networks A and B


def nets_of(kind, widths=SAME):
    if (kind, widths) not in _nets:
        _nets[kind, widths] = tuple(_net(kind, s, c) for s, c in zip(SEEDS, widths))
    return _nets[kind, widths]


def plain(kind, widths=SAME):
    """The plain arena's games of network A against network B: played once."""
    if (kind, widths) not in _plain:
        _plain[kind, widths] = _play(kind, *nets_of(kind, widths))
    return _plain[kind, widths]


def _identity(s, table):
    if table:
        assert s["probed"] == s["hits"] + s.get("merged", 0) + s["inserts"] + s["dropped"], s
    else:
        assert s["hits"] == s["inserts"] == s["dropped"] == 0 <= s["merged"] <= s["probed"], s


def _cached_plays_plain(kind, switch, widths):
    want = plain(kind, widths)
    got = _play(kind, *nets_of(kind, widths), **SWITCHES[switch])
    same_games(got["games"], want["games"])
    assert got["result"] == want["result"]
    assert got["mixed"] > 0 and got["mixed"] == want["mixed"] and got["steps"] == want["steps"]
    a, b = got["stats"]
    print(f"{kind} {switch} {widths}: A {a}  B {b}")
    table = "eval_cache" in SWITCHES[switch]
    for s in (a, b):
        assert ("merged" in s) == ("eval_merge" in SWITCHES[switch])
        _identity(s, table)
        assert s["probed"] > 0
        if table:   # game k + 2 opens as game k did, for both sides
            assert s["hits"] > 0, s
    assert got["sum"] == {k: a[k] + b[k] for k in a}


def _other_pairings_play_other_games(kind, widths):
    a, b = nets_of(kind, widths)
    ab = plain(kind, widths)["games"]
    for x, y in ((a, a), (b, b), (b, a)):
        other = _play(kind, x, y)["games"]
        assert any(p.shape != q.shape or not torch.equal(p, q) for p, q in zip(ab, other)), (kind, widths, "same games")


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("kind", KINDS)
def test_cached_arena_plays_the_plain_arenas_games(kind, switch):
    _cached_plays_plain(kind, switch, SAME)


@pytest.mark.parametrize("kind", KINDS)
def test_the_two_networks_play_other_games_than_one_network_alone(kind):
    """The guard of the equality above: were the routes swapped or one network used for both
    sides, the games would be those of another pairing — and those differ at this shape."""
    _other_pairings_play_other_games(kind, SAME)


# a 64-channel network against a 128-channel one in every search, and two 64-channel networks in
# the two searches that tests/test_gpu_net_width_pools.py does not run at that width
ACROSS = [(k, (64, 128)) for k in KINDS] + [("c4_puct", (64, 64)), ("chess_value", (64, 64))]
ACROSS_IDS = [f"{k}-{a}v{b}" for k, (a, b) in ACROSS]


@pytest.mark.parametrize("kind,widths", ACROSS, ids=ACROSS_IDS)
def test_cached_arena_plays_the_plain_arenas_games_across_widths(kind, widths):
    """Cache and merged flush together, the two networks' towers of different widths or both 64
    channels wide: each network's table and flush runs its own tower, and the games are the plain
    arena's, which tests/test_gpu_arena_search.py ties to the two single-network searches."""
    a, b = nets_of(kind, widths)
    assert tuple((n.tower if kind.endswith("puct") else n).channels for n in (a, b)) == widths
    _cached_plays_plain(kind, "both", widths)


@pytest.mark.parametrize("kind,widths", ACROSS, ids=ACROSS_IDS)
def test_the_two_networks_play_other_games_than_one_network_alone_across_widths(kind, widths):
    _other_pairings_play_other_games(kind, widths)


def test_cached_c4_arena_of_one_network_plays_its_self_play_games():
    net = integer_net(2, 5)
    arena = C4Arena(8, SIMS, batch_size=BS, seed=9, net_a=net, net_b=net, eval_cache=ENTRIES)
    pool = C4SelfPlay(8, SIMS, batch_size=BS, seed=9, net=net)
    arena.play(20, max_steps=2000)
    simulate_games(pool, 20, max_steps=2000)
    same_games(batch(arena), batch(pool))
    assert arena.mixed_steps > 0
    a, b = arena.eval_cache_stats(by_network=True)
    assert a["probed"] > 0 and b["probed"] > 0 and a["hits"] > 0 and b["hits"] > 0   # two tables all the same
    arena.close()
    pool.close()


def test_cached_arena_replays_its_step_from_a_graph():
    """Twelve replays, past the first refill, against twelve step() calls of a twin: the same
    roots, trajectories and cache counters; the warm-up before the capture leaves no trace."""
    a, _ = _replayed_and_stepped("c4_value", SAME)
    assert int(a.traj.slot[:, 1].max()) >= 8, "no slot was refilled: play more steps"
    assert all(s["hits"] > 0 for s in a.eval_cache_stats(by_network=True))
    a.close()


def test_cached_chess_puct_arena_of_two_widths_replays_its_step_from_a_graph():
    """The same with the routed policy cache in the graph: the convolutional head, network A 64
    channels wide and network B 128 (one logits width, two towers).  Twelve steps end no game
    of king and queen against king, so no slot is refilled; what is asked of the counters
    beyond their equality in the two arenas is that both tables were probed and took entries."""
    a, nets = _replayed_and_stepped("chess_puct", (64, 128))
    assert all(n.conv_head for n in nets) and [n.tower.channels for n in nets] == [64, 128]
    stats = a.eval_cache_stats(by_network=True)
    print(f"chess_puct (64, 128), captured: A {stats[0]}  B {stats[1]}")
    for s in stats:
        _identity(s, True)
        assert s["probed"] > 0 and s["inserts"] > 0, s
    a.close()


def _replayed_and_stepped(kind, widths):
    na, nb = nets_of(kind, widths)
    a = _arena(kind, na, nb, eval_cache=ENTRIES)
    b = _arena(kind, na, nb, eval_cache=ENTRIES)
    g = b.capture_step()
    assert b.eval_cache_stats() == a.eval_cache_stats() and b.steps == 0
    for i in range(12):
        a.step()
        g.replay()
    sa, sb = _pool_state(a), _pool_state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert a.eval_cache_stats(by_network=True) == b.eval_cache_stats(by_network=True)
    assert (a.steps, a.mixed_steps) == (b.steps, b.mixed_steps) == (12, b.mixed_steps) and b.mixed_steps > 0
    a.check()
    b.check()
    b.close()
    return a, (na, nb)


def test_plain_arena_still_refuses_the_capture():
    na, nb = nets_of("c4_value")
    arena = _arena("c4_value", na, nb)
    with pytest.raises(ValueError, match="cannot be captured"):
        arena.capture_step()
    with pytest.raises(ValueError, match="without eval_cache"):
        arena.eval_cache_stats()
    arena.close()
