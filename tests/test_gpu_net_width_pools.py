"""A 64-channel network everywhere a 128-channel one runs: the self-play pools with the
evaluation cache and the merged flush, the arena's routed cache and its captured step, and
set_network.  Every network here is built from its trainable module by learner.inference_form,
as set_network and the training loop build it: where the 64-channel tower is missing that is a
torch module, which the caches refuse.  The smallest pools that reach every path."""
import pytest
import torch

from test_gpu_eval_cache import _bn, _pool_state

pytestmark = pytest.mark.gpu

ENTRIES = 256


def value_model(seed, channels=64):
    from zeroclone_amd.nets import ValueNetwork
    torch.manual_seed(seed)
    return _bn(ValueNetwork(channels, 1, in_planes=2))


def integer_policy_model(seed, head):
    """PolicyValueNetwork(64, 1 block) with tests/arena_nets.py's integer weights (density 0.004
    for the 64 -> 64 convs): its outputs are exact in any summation order, so the linear head's
    GEMM gives a row the same logits whichever rows stand beside it."""
    from zeroclone_amd.nets import PolicyValueNetwork
    g = torch.Generator().manual_seed(seed)
    net = PolicyValueNetwork(64, 1, head=head).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            dens = 0.004 if m.in_channels == 64 and m.kernel_size == (3, 3) else 0.02
            keep = torch.rand(m.weight.shape, generator=g) < dens
            m.weight.data = torch.randint(-2, 3, m.weight.shape, generator=g).float() * keep
        elif isinstance(m, torch.nn.BatchNorm2d):
            m.eps = 0.0
            m.running_mean.zero_()
            m.running_var.fill_(1.0)
            m.weight.data.fill_(1.0)
            m.bias.data = torch.randint(-1, 3, m.bias.shape, generator=g).float()
        elif isinstance(m, torch.nn.Linear) and m.out_features == 1:
            m.weight.data = torch.randint(-2, 3, m.weight.shape, generator=g).float() / 64.0
            m.bias.data.zero_()
        elif isinstance(m, torch.nn.Linear):
            keep = torch.rand(m.weight.shape, generator=g) < 0.004
            m.weight.data = torch.randint(-1, 2, m.weight.shape, generator=g).float() * keep
            m.bias.data = torch.randint(-4, 5, m.bias.shape, generator=g).float()
    return net


def form(model):
    from zeroclone_amd import learner
    return learner.inference_form(model, "cuda")


def same_state(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def test_c4_pool_with_cache_and_merge_plays_the_plain_pools_games():
    from zeroclone_amd.nets import MfmaValueNetwork
    from zeroclone_amd.selfplay import C4SelfPlay
    net = form(value_model(seed=41))
    assert isinstance(net, MfmaValueNetwork) and net.channels == 64
    states = []
    for kw in ({}, dict(eval_cache=ENTRIES, eval_merge=True)):
        pool = C4SelfPlay(8, 16, batch_size=4, seed=31, net=net, **kw)
        for _ in range(12):
            pool.step()
        pool.check()
        states.append(_pool_state(pool))
        if kw:
            s = pool.eval_cache_stats()
            print(f"c4 value, 64 channels: {s}")
            assert s["hits"] > 0 and s["probed"] > 0
        pool.close()
    same_state(states[0], states[1], "c4 value")
    assert int(states[0]["traj.hmoves"].abs().sum()) + int(states[0]["traj.pool_moves"].abs().sum()) > 0


@pytest.mark.parametrize("head", ["conv", "linear"])
def test_chess_puct_pool_with_the_cache_plays_the_plain_pools_games(head):
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    from zeroclone_amd.selfplay import ChessSelfPlay
    net = form(integer_policy_model(seed=43, head=head))
    assert isinstance(net, MfmaPolicyValueNetwork) and net.tower.channels == 64 and net.fused
    states = []
    for kw in ({}, dict(eval_cache=ENTRIES)):
        pool = ChessSelfPlay(4, 16, batch_size=4, seed=35, temperature=1.0, puct_net=net, **kw)
        for _ in range(6):
            pool.step()
        pool.check()
        states.append(_pool_state(pool))
        if kw:
            s = pool.eval_cache_stats()
            print(f"chess puct ({head}), 64 channels: {s}")
            assert s["probed"] > 0 and s["probed"] == s["hits"] + s["inserts"] + s["dropped"]
        pool.close()
    same_state(states[0], states[1], ("chess puct", head))
    assert int(states[0]["moves"].abs().sum()) > 0


def test_c4_arena_of_two_64_channel_networks_replays_its_step_from_a_graph():
    from zeroclone_amd.arena import C4Arena
    na, nb = form(value_model(seed=45)), form(value_model(seed=46))

    def arena():
        return C4Arena(8, 16, batch_size=4, seed=3, net_a=na, net_b=nb, eval_cache=ENTRIES)
    a, b = arena(), arena()
    g = b.capture_step()
    for _ in range(12):
        a.step()
        g.replay()
    same_state(_pool_state(a), _pool_state(b), "arena")
    # a table of 256 entries drops rows, and which of two rows that claim one slot in the same
    # flush gets it is not fixed: the games are, the split of the probes into hits and inserts is not
    for sa, sb in zip(a.eval_cache_stats(by_network=True), b.eval_cache_stats(by_network=True)):
        assert sa["probed"] == sb["probed"] > 0
        for s in (sa, sb):
            assert s["probed"] == s["hits"] + s["inserts"] + s["dropped"], s
    assert (a.steps, a.mixed_steps) == (b.steps, b.mixed_steps) and a.steps == 12 and a.mixed_steps > 0
    a.check()
    b.check()
    a.close()
    b.close()


def test_set_network_takes_a_64_channel_model_and_then_a_128_channel_one():
    """set_network builds the model's inference form anew, so the width may change between
    calls: a 64-channel model puts the 64-channel MFMA tower in place, a 128-channel one the
    128-channel tower, and the pool (with its cache, emptied each time) goes on playing."""
    from zeroclone_amd.nets import MfmaValueNetwork
    from zeroclone_amd.selfplay import C4SelfPlay
    pool = C4SelfPlay(8, 16, batch_size=4, seed=31, net=form(value_model(seed=47)), eval_cache=ENTRIES)
    for _ in range(2):
        pool.step()
    for channels in (64, 128):
        pool.set_network(value_model(seed=48, channels=channels))
        net = pool.value_fn.nets[0]
        assert isinstance(net, MfmaValueNetwork) and net.channels == channels
        before = pool.eval_cache_stats()
        for _ in range(3):
            pool.step()
        pool.check()
        after = pool.eval_cache_stats()
        assert after["probed"] > before["probed"] and after["inserts"] > before["inserts"]
    pool.close()
