"""A 64-channel network everywhere a 128-channel one runs: the self-play pools with the
evaluation cache and the merged flush, the arena's routed cache and its captured step,
set_network, the searches split over streams on replicas and the short last flush.  Every network here is built from its trainable module by learner.inference_form,
as set_network and the training loop build it: where the 64-channel tower is missing that is a
torch module, which the caches refuse.  The smallest pools that reach every path."""
import pytest
import torch

from test_gpu_eval_cache import _bn, _pool_state

pytestmark = pytest.mark.gpu

ENTRIES = 256


def value_model(seed, channels=64, in_planes=2):
    from zeroclone_amd.nets import ValueNetwork
    torch.manual_seed(seed)
    return _bn(ValueNetwork(channels, 1, in_planes=in_planes))


def integer_policy_model(seed, head, c4=False):
    """PolicyValueNetwork(64, 1 block) with tests/arena_nets.py's integer weights (density 0.004
    for the 64 -> 64 convs): its outputs are exact in any summation order, so the linear head's
    GEMM gives a row the same logits whichever rows stand beside it.  c4: the Connect4 network
    (2 planes, 6x7, 32 policy planes, 7 logits) instead of the chess one."""
    from zeroclone_amd.nets import PolicyValueNetwork
    g = torch.Generator().manual_seed(seed)
    shape = dict(in_planes=2, board=(6, 7), n_logits=7) if c4 else {}
    net = PolicyValueNetwork(64, 1, head=head, **shape).eval()
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


def test_c4_puct_pool_with_the_cache_plays_the_plain_pools_games():
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    from zeroclone_amd.selfplay import C4SelfPlay
    net = form(integer_policy_model(seed=49, head="linear", c4=True))
    assert isinstance(net, MfmaPolicyValueNetwork) and net.tower.channels == 64 and net.fused
    assert net.pw.shape[0] == 2 and net.logits_width == 7   # 32 policy planes: two M tiles of 16
    states = []
    for kw in ({}, dict(eval_cache=ENTRIES)):
        pool = C4SelfPlay(8, 16, batch_size=4, seed=33, temperature=1.0, puct_net=net, **kw)
        for _ in range(12):
            pool.step()
        pool.check()
        states.append(_pool_state(pool))
        if kw:
            s = pool.eval_cache_stats()
            print(f"c4 puct, 64 channels: {s}")
            assert s["probed"] > 0 and s["probed"] == s["hits"] + s["inserts"] + s["dropped"]
        pool.close()
    same_state(states[0], states[1], "c4 puct")
    assert int(states[0]["traj.hmoves"].abs().sum()) + int(states[0]["traj.pool_moves"].abs().sum()) > 0


def test_chess_value_pool_with_cache_and_merge_plays_the_plain_pools_games():
    from zeroclone_amd.nets import MfmaValueNetwork
    from zeroclone_amd.selfplay import ChessSelfPlay
    net = form(value_model(seed=51, in_planes=17))
    assert isinstance(net, MfmaValueNetwork) and net.channels == 64
    states = []
    for kw in ({}, dict(eval_cache=ENTRIES, eval_merge=True)):
        pool = ChessSelfPlay(4, 16, batch_size=4, seed=37, net=net, **kw)
        for _ in range(6):
            pool.step()
        pool.check()
        states.append(_pool_state(pool))
        if kw:
            s = pool.eval_cache_stats()
            print(f"chess value, 64 channels: {s}")
            assert s["probed"] > 0 and s["probed"] == s["hits"] + s["merged"] + s["inserts"] + s["dropped"]
        pool.close()
    same_state(states[0], states[1], "chess value")
    assert int(states[0]["moves"].abs().sum()) > 0


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=64, max_sims=128, max_batch=32)
    yield e
    e.close()


def test_split_stream_chess_search_equals_the_single_stream_search(eng):
    """tests/test_gpu_puct.py:test_split_stream_search_equals_the_single_stream_search at 64
    channels, k = 2: the 37 games in two parts on two streams, each part on a replica() of the
    network (shared weights, its own buffers; the replica carries the width).  Moves, root
    visits, priors and counters equal the one-stream search's, eagerly and replayed from a graph."""
    from test_gpu_puct import FENS, roots_of
    from zeroclone_amd.valued import ChessPuctSearch
    net = form(integer_policy_model(seed=53, head="linear"))
    rep = net.replica()
    assert rep.tower.channels == net.tower.channels == 64 and rep.tower.wall.data_ptr() == net.tower.wall.data_ptr()
    assert rep.tower._bufs is not net.tower._bufs and rep._pout is not net._pout
    fens = (FENS * 8)[:37]
    roots = roots_of(fens)
    outs = []
    for split in (False, True):
        ps = ChessPuctSearch(eng, len(fens), 32, seed=9)
        fn = [(lambda l, p, c, m=net.replica(): m(p)) for _ in range(2)] if split else (lambda l, p, c: net(p))
        mv, na, st = ps.run(roots, 97, fn, temperature=1.0)
        assert (st[:, 5] == 0).all()
        first = (mv.cpu().clone(), na.cpu().clone(), ps.prior.cpu().clone(), st[:, :3].cpu().clone())
        g = ps.capture(roots, 97, fn, temperature=1.0)
        g.replay()
        torch.cuda.synchronize()
        second = (ps.move.cpu().clone(), ps.na.cpu().clone(), ps.prior.cpu().clone())
        assert ps.search_no.cpu().tolist() == [2] * len(fens)
        outs.append((first, second))
    (a1, a2), (b1, b2) = outs
    for x, y in zip(a1 + a2, b1 + b2):
        assert torch.equal(x, y)
    assert (a1[1].sum(dim=1) == 96).all()


def test_split_stream_c4_search_equals_the_single_stream_search(eng):
    """tests/test_gpu_c4_puct.py:test_c4_split_stream_search_equals_the_single_stream_search at 64
    channels, k = 2."""
    from test_gpu_c4_puct import POSITIONS, _roots
    from zeroclone_amd.valued import C4PuctSearch
    net = form(integer_policy_model(seed=55, head="linear", c4=True))
    assert net.replica().tower.channels == 64
    pos = (POSITIONS * 8)[:37]
    r = _roots(pos)
    outs = []
    for split in (False, True):
        ps = C4PuctSearch(eng, len(pos), 16, seed=5)
        fn = [(lambda l, p, c, m=net.replica(): m(p)) for _ in range(2)] if split else (lambda l, p, c: net(p))
        mv, na, st = ps.run(r, 97, fn, temperature=1.0)
        outs.append((mv.cpu().clone(), na.cpu().clone(), ps.prior.cpu().clone(), st[:, :3].cpu().clone()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert int(outs[0][1].sum()) > 0


def test_short_last_flush_runs_the_network_on_its_leaves_only(eng):
    """tests/test_gpu_chess_search.py's test of that name with a 64-channel value network: sims
    is not a multiple of the batch, NetValue.rows evaluates the last flush's n * 4 boards only,
    and the search equals the one that evaluates all n * 32 slots."""
    from test_gpu_puct import FENS, roots_of
    from zeroclone_amd.nets import MfmaValueNetwork, ValueNetwork
    from zeroclone_amd.valued import ChessValuedSearch, NetValue
    torch.manual_seed(3)
    mnet = MfmaValueNetwork(ValueNetwork(64, 2).eval(), "cuda")
    assert mnet.channels == 64
    net = NetValue(mnet)
    fens = FENS * 3
    n, sims, bs = len(fens), 100, 32   # the last flush holds 4 leaves a game
    seeds = [40 + i for i in range(n)]
    calls = []

    def full(leaves, planes, counts):
        calls.append(planes.shape[0])
        return net(leaves, planes, counts)

    outs = []
    for fn in (net, full):
        eng.seed(0, seeds)
        vs = ChessValuedSearch(eng, n, bs)
        outs.append([x.cpu().numpy().copy() for x in vs.run(roots_of(fens), sims, 1.4, fn)])
    assert calls == [n * bs] * 4
    for a, b in zip(*outs):
        assert (a == b).all()
    assert (outs[0][2][:, 5] == 0).all() and (outs[0][2][:, 0] == sims).all()
