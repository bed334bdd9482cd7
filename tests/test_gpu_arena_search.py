"""A routed search equals the two single-network searches: each game's move, root visit counts,
stats and final RNG state are those of the search whose network its key names, bit for bit, in
each of the four stepwise searches (12 Connect4 games, 6 chess games, batch 8, 20 simulations:
flushes of 8, 8 and 4 leaves, and the PUCT searches' roots flush of one row a game).  The networks
are callables exact on the planes, integer MFMA networks of 128 channels, of 64, and one of 64
against one of 128."""
import random

import numpy as np
import pytest
import torch

import oracle
from arena_nets import Exact, integer_net, integer_pv_net
from c4_positions import EMPTY, states
from zeroclone_amd import _native, valued

pytestmark = pytest.mark.gpu

BS, SIMS, C = 8, 20, 1.4
# neither constant nor the slot halves
KEY12 = [0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0]
KEY6 = [1, 0, 0, 1, 1, 0]
# positions of the chess goldens (chess_get_move.json, the self-play tests' KQK) with few root
# moves, so that 20 simulations return to the root's children and the values steer the counts
CHESS_FENS = ["4k3/8/8/8/8/8/8/4K2R b K - 0 1",
              "8/P6k/8/8/8/8/6Kp/8 w - - 0 1",
              "8/P6k/8/8/8/8/6Kp/8 b - - 0 1",
              "6k1/5ppp/8/8/8/8/5PPP/3R2K1 b - - 0 1",
              "8/8/4k3/8/8/8/3QK3/8 b - - 0 1",
              "4k3/8/8/8/8/8/8/4K2R w K - 0 1"]


def c4_roots():
    """12 live positions 3 to 14 plies deep, both sides to move."""
    rng, boards = random.Random(41), []
    while len(boards) < 12:
        b, t = EMPTY, 0
        for _ in range(3 + len(boards)):
            b, t = oracle.play(b, t, rng.choice([col for col in range(7) if b[col] == "."]))
            if oracle.check_win(b, t) or oracle.check_draw(b):
                break
        else:
            boards.append((b, t))
    assert {t for _, t in boards} == {0, 1}
    return torch.from_numpy(states(boards).view(np.int64).reshape(12, 3).copy()).cuda()


def chess_roots():
    a = np.array([_native.chess_from_fen(f) for f in CHESS_FENS], _native.CHESS_STATE_DTYPE)
    assert set(a["turn"].tolist()) == {0, 1}
    return torch.from_numpy(a.view(np.uint8).reshape(len(CHESS_FENS), 72).copy()).cuda()


# the channels of networks A and B: two 64-channel towers, and a 64-channel one against a
# 128-channel one (the routed callables need the same head and logits width, not the same tower)
WIDTHS = {"integer_net": (128, 128), "integer_net_64": (64, 64), "integer_net_mixed": (64, 128)}


def value_fns(kind, planes):
    if kind == "exact":
        return Exact(11), Exact(23)
    ca, cb = WIDTHS[kind]
    return valued.NetValue(integer_net(planes, 5, ca)), valued.NetValue(integer_net(planes, 6, cb))


def policy_fns(kind, planes, h, w, nl, head="linear"):
    if kind == "exact":
        return Exact(11, nl), Exact(23, nl)
    ca, cb = WIDTHS[kind]
    return (valued.PolicyNet(integer_pv_net(planes, h, w, nl, 5, head, ca)),
            valued.PolicyNet(integer_pv_net(planes, h, w, nl, 6, head, cb)))


# search: (class, roots, keys, constructor arguments, the two callables of a kind)
SEARCHES = {
    "c4_value": (valued.C4ValuedSearch, c4_roots, KEY12, {}, lambda k: value_fns(k, 2)),
    "chess_value": (valued.ChessValuedSearch, chess_roots, KEY6, {}, lambda k: value_fns(k, 17)),
    "c4_puct": (valued.C4PuctSearch, c4_roots, KEY12, {"seed": 3}, lambda k: policy_fns(k, 2, 6, 7, 7)),
    "chess_puct": (valued.ChessPuctSearch, chess_roots, KEY6, {"seed": 3},
                   lambda k: policy_fns(k, 17, 8, 8, 4096)),
    "chess_puct_nhwc": (valued.ChessPuctSearch, chess_roots, KEY6, {"seed": 3, "planes_nhwc": True},
                        lambda k: policy_fns(k, 17, 8, 8, 4096, "conv")),
}


@pytest.mark.parametrize("kind", ["exact", "integer_net", "integer_net_64", "integer_net_mixed"])
@pytest.mark.parametrize("name", list(SEARCHES))
def test_routed_search_equals_the_single_network_searches(name, kind):
    cls, roots_fn, key, kw, fns = SEARCHES[name]
    n, puct = len(key), "puct" in name
    eng = _native.NativeEngine(max_games=n, max_sims=SIMS, max_batch=BS)
    try:
        eng.seed(0, [900 + 17 * g for g in range(n)])
        search = cls(eng, n, BS, leaves=False, **kw)
        roots = roots_fn()
        fn_a, fn_b = fns(kind)
        stream = torch.cuda.current_stream().cuda_stream
        snap = torch.zeros(n * (4096 * 4 + 16), dtype=torch.uint8, device="cuda")
        eng.rng_copy(0, n, snap.data_ptr(), False, stream)

        def run(fn):
            eng.rng_copy(0, n, snap.data_ptr(), True, stream)
            if puct:
                search.search_no.zero_()   # the root noise's counter word: the same search again
                search.run(roots, SIMS, fn, 0.0)
            else:
                search.run(roots, SIMS, C, fn)
            out = [search.move.cpu().numpy().copy(), search.na.cpu().numpy().copy(), search.stats.cpu().numpy().copy()]
            assert (out[2][:, 5] == 0).all(), "a search failed"
            rng = [eng.get_rng_state(g) for g in range(n)]
            return out + [[(mt.tolist(), i) for mt, i in rng]]

        single = [run(fn_a), run(fn_b)]
        # the cap against a vacuous pass: a routing error shows only where the two searches differ
        differ = sum(not np.array_equal(single[0][1][g], single[1][1][g]) for g in range(n))
        print(f"{name} {kind}: the all-A and all-B root visit counts differ in {differ} of {n} games")
        assert 4 * differ >= 3 * n, (differ, n)

        routed = (valued.RoutedPolicy if puct else valued.RoutedValue)(fn_a, fn_b)
        d_key = torch.tensor(key, dtype=torch.int32, device="cuda")
        perm = torch.zeros(n, dtype=torch.int32, device="cuda")
        count = torch.zeros(2, dtype=torch.int32, device="cuda")
        _native.arena_route(n, d_key.data_ptr(), perm.data_ptr(), count.data_ptr(), stream)
        routed.set_route(perm, int(count[0]))
        assert int(count[0]) == key.count(0)
        mark_a, mark_b = len(fn_a.calls) if kind == "exact" else 0, len(fn_b.calls) if kind == "exact" else 0
        got = run(routed)
        for g in range(n):
            want = single[key[g]]
            assert got[0][g] == want[0][g], (g, "move")
            assert np.array_equal(got[1][g], want[1][g]), (g, "root visit counts")
            assert np.array_equal(got[2][g], want[2][g]), (g, "stats")
            assert got[3][g] == want[3][g], (g, "RNG state")
        if kind == "exact":   # each network saw the rows of its own group only, in one call a flush
            for calls, m in ((fn_a.calls[mark_a:], key.count(0)), (fn_b.calls[mark_b:], key.count(1))):
                if puct:   # the roots flush: one row a game
                    assert calls[0] == m and len(calls) > 1 and set(calls[1:]) == {m * BS}
                else:      # the short last flush: its 4 leaves a game
                    assert calls == [m * BS, m * BS, m * (SIMS - 2 * BS)]
    finally:
        eng.close()


def test_empty_groups_call_no_network_and_logits_must_agree():
    n = 4
    planes = (torch.rand((n * BS, 2, 6, 7), device="cuda") < 0.3).half()
    counts = torch.full((n,), BS, dtype=torch.int32, device="cuda")
    perm = torch.arange(n, dtype=torch.int32, device="cuda")
    a, b = Exact(1), Exact(2)
    routed = valued.RoutedValue(a, b)
    with pytest.raises(ValueError):
        routed(None, planes, counts)          # no route yet
    routed.set_route(perm, n)
    va = routed(None, planes, counts).clone()
    assert a.calls == [n * BS] and b.calls == []
    assert torch.equal(va, Exact(1)(None, planes, counts))
    routed.set_route(perm, 0)
    vb = routed(None, planes, counts).clone()
    assert a.calls == [n * BS] and b.calls == [n * BS]
    assert torch.equal(vb, Exact(2)(None, planes, counts))
    out = torch.full((n * BS,), 7.0, dtype=torch.float64, device="cuda")
    routed.set_route(torch.tensor([2, 0, 3, 1], dtype=torch.int32, device="cuda"), 2)
    routed.rows(planes, n, BS, 3, out)
    o, ea, eb = out.view(n, BS), va.view(n, BS), vb.view(n, BS)
    assert bool((o[:, 3:] == 7.0).all())
    assert torch.equal(o[[0, 2], :3], ea[[0, 2], :3]) and torch.equal(o[[1, 3], :3], eb[[1, 3], :3])
    # logits of two widths: refused at the first call that shows it
    pol = valued.RoutedPolicy(Exact(1, 7), Exact(2, 9))
    pol.set_route(perm, 2)
    with pytest.raises(ValueError):
        pol(None, planes, counts)
