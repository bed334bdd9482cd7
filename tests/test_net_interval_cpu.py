"""The one-layer float64 reference and its derived bound (tests/nn_check.py: conv_interval,
pointwise_interval, value_head_reference) on the CPU.  A torch fp32 convolution stands in for a
correct kernel: it must lie wholly inside the accepted interval, and four subtly wrong kernels
(the conv rounded to fp16 before the residual add, one tap dropped at one pixel, the bias
added in fp16, ReLU before the residual) must fall outside it for at least 100 elements.
The generator's inputs must leave fewer than half of the intervals holding two fp16 values
(a condition on the inputs: an ambiguous element still rejects every value but those two).
The same for the value head: five subtly wrong heads against the synthetic activations of the
GPU tests of the stand-alone head, at both widths."""
import numpy as np
import pytest
import torch

import nn_check as nc

SHAPES = [(8, 8, 128), (6, 7, 32)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def layer(request):
    h, w, cin = request.param
    x, wt, bias, res = nc.wide_range_layer(h, w, cin, seed=100 * h + cin)
    return x, wt, bias, res, nc.conv_interval(x, wt, bias, res, relu=True)


def test_rn16_rounds_once():
    """1 + 2^-11 + 2^-30 lies above the tie between 1 and 1 + 2^-10; a conversion through
    fp32 lands on the tie and rounds to even (1.0)."""
    v = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -30, 65519.99, 65520.0, -65520.0, 2.0 ** -25, 2.0 ** -25 * 1.0001,
                      float("nan")], dtype=torch.float64)
    got = nc.rn16(v)
    assert got[:6].tolist() == [1 + 2.0 ** -10, 65504.0, float("inf"), float("-inf"), 0.0, 2.0 ** -24]
    assert torch.isnan(got[6])


def test_gamma_is_the_textbook_bound():
    assert nc.gamma(9 * 128 + 2) == pytest.approx(1154 * 2.0 ** -24, rel=1e-4)
    # an fp32 sum of k terms in the worst order stays inside it
    g = torch.Generator().manual_seed(0)
    t = (torch.randn(1154, generator=g) * 10 ** (4 * torch.rand(1154, generator=g))).float()
    exact, A = t.double().sum().item(), t.double().abs().sum().item()
    for order in (torch.arange(1154), torch.argsort(t.abs()), torch.argsort(-t.abs()), torch.randperm(1154, generator=g)):
        s = np.float32(0)
        for v in t[order].numpy():
            s = np.float32(s + v)
        assert abs(float(s) - exact) <= nc.gamma(1154) * A


def test_generator_reaches_the_edges(layer):
    x, wt, bias, res, (lo, hi, s) = layer
    assert x.shape[0] == 13 and x.dtype == wt.dtype == res.dtype == torch.float16 and bias.dtype == torch.float32
    assert nc.has_subnormals(x), "no fp16-subnormal stored activation"
    assert nc.has_subnormals(wt), "no fp16-subnormal weight"
    assert 0.25 < float((x == 0).double().mean()) < 0.4
    assert x.abs().max().item() > 512 and res.abs().max().item() > 1024
    assert nc.ambiguous_share(lo, hi) < 0.5
    assert (s < 0).any() and (s > 0).any()


def test_fp32_stand_in_lies_inside_the_interval(layer):
    x, wt, bias, res, _ = layer
    for use_res, relu in ((False, True), (True, True), (True, False)):
        r = res if use_res else None
        lo, hi, s = nc.conv_interval(x, wt, bias, r, relu=relu)
        got = nc.fp32_layer(x, wt, bias, r, relu=relu)
        bad = nc.outside(got, lo, hi, s)
        assert int(bad.sum()) == 0, (use_res, relu, int(bad.sum()))
        # the cap is on the ReLU'd layer, where the negative half of the sums is exactly 0; without
        # the ReLU both halves count, so the share is twice that of the positive half alone
        share = nc.ambiguous_share(lo, hi)
        assert share < 0.5 if relu else 0.5 * share < 0.5, (use_res, relu, share)


@pytest.mark.parametrize("mutant,least", [("round_before_res", 100), ("drop_tap", 100), ("bias_fp16", 100),
                                          ("relu_before_res", 100)])
def test_mutants_fall_outside(layer, mutant, least):
    x, wt, bias, res, (lo, hi, s) = layer
    got = nc.fp32_layer(x, wt, bias, res, relu=True, mutant=mutant)
    bad = int(nc.outside(got, lo, hi, s).sum())
    print(f"{mutant}: {bad} of {s.numel()} outside")
    assert bad >= least, (mutant, bad)
    if mutant == "drop_tap":   # confined to the one pixel: 13 boards x 128 channels
        mask = torch.zeros(s.shape, dtype=torch.bool)
        mask[:, 2, 3, :] = True
        assert int(nc.outside(got, lo, hi, s)[~mask].sum()) == 0 and int(mask.sum()) == 1664


def head_cases(channels):
    """The inputs of the stand-alone value head's GPU tests (test_gpu_net_range.py at 128 channels,
    test_gpu_net_width.py at 64), drawn as there: (hw, n, cancelling set, spread set)."""
    for hw in (64, 42):
        g = torch.Generator().manual_seed(hw)
        for n in (1, 5):
            yield hw, n, nc.cancelling_head_inputs(g, n, hw, channels), nc.spread_head_inputs(
                1000 * channels + 10 * hw + n, n, hw, channels)


# which set must reject which wrong head ("divide_by_64" is a wrong head on 6x7 alone)
CANCELLING_CATCHES = ("fp16_pixel_sums", "fp16_weights", "divide_by_64")
SPREAD_CATCHES = ("fp16_pixel_sums", "divide_by_64", "pair_weights_swapped", "one_lane_left_out")


@pytest.mark.parametrize("channels", [64, 128])
def test_wrong_value_heads_fall_outside_the_slack(channels):
    """The synthetic activations of the value head's GPU tests tell a wrong head from a right one:
    each of nn_check.HEAD_MUTANTS, computed in float64 from the head's inputs alone, is NaN or
    outside value_head_reference's slack on at least one board of every (hw, n, fcb) case.

    The cancelling set (channel pairs with the same activation under opposite weights) rejects the
    fp16 pixel sums (NaN: inf - inf), the fp16 weights (1.7 to 17 slacks) and the division by 64 on
    6x7 (7 to 17 slacks).  It cannot see the two weights of a pair exchanged (its two channels hold
    the same activation, so the sum is the same) and sees one lane's share of channels 8 .. 15
    left out in a few cases only (the term leaves both channels of a pair and cancels: 0 to 2.4
    slacks).  The spread set (every channel its own activation and weight) was added for those
    two and rejects both in every case, by 40 slacks at the least; with it every named wrong head
    is caught in every case at both widths.  A right head in fp32 (torch's sums) lies inside
    the slack on both sets."""
    assert set(CANCELLING_CATCHES) | set(SPREAD_CATCHES) == set(nc.HEAD_MUTANTS)
    for hw, n, cancelling, spread in head_cases(channels):
        for fcb in nc.HEAD_FCBS:
            for name, (act, fcw), catches in (("cancelling", cancelling, CANCELLING_CATCHES), ("spread", spread, SPREAD_CATCHES)):
                d, slack = nc.value_head_reference(act, fcw, fcb)
                assert 5.0e4 < act.max().item() and torch.isfinite(act).all() and slack.max().item() < 0.5
                assert (d - float(np.float32(fcb))).abs().max().item() < 2.0
                right = ((act.float().sum(dim=1) * fcw).sum(dim=1) / np.float32(hw) + np.float32(fcb)).double()
                assert not nc.head_rejects(right, d, slack).any(), (channels, hw, n, fcb, name)
                for mutant in catches:
                    if mutant == "divide_by_64" and hw == 64:
                        continue
                    wrong = nc.wrong_head(act, fcw, fcb, mutant)
                    bad = nc.head_rejects(wrong, d, slack)
                    print(f"{channels} channels hw {hw} n {n} fcb {fcb} {name} {mutant}: {int(bad.sum())} of {n} boards, "
                          f"{((wrong - d).abs() / slack).max().item():.1f} slacks")
                    assert bad.any(), (channels, hw, n, fcb, name, mutant)
            # the blind spot that the spread set closes, stated so that it stays known
            act, fcw = cancelling
            d, slack = nc.value_head_reference(act, fcw, fcb)
            assert not nc.head_rejects(nc.wrong_head(act, fcw, fcb, "pair_weights_swapped"), d, slack).any()


def test_overflow_set_demands_the_infinities():
    x, wt, bias, res = nc.wide_range_layer(8, 8, 32, seed=7, overflow=True)
    lo, hi, s = nc.conv_interval(x, wt, bias, res, relu=False)
    assert (lo == float("inf")).any() and (hi == float("-inf")).any()
    share = float(((lo == float("inf")) | (hi == float("-inf"))).double().mean())
    assert 0.005 < share < 0.05
    straddle = (lo < float("inf")) & (hi == float("inf"))     # sums the bound cannot place: both accepted
    assert straddle.any()
    got = nc.fp32_layer(x, wt, bias, res, relu=False)
    assert int(nc.outside(got, lo, hi, s).sum()) == 0
    # a kernel that saturates instead of overflowing, and one that stores NaN there, both fail
    sat = got.clone()
    sat[torch.isinf(sat)] = 65504.0
    assert int(nc.outside(sat, lo, hi, s).sum()) >= 100
    lo1, hi1, s1 = nc.conv_interval(x, wt, bias, res, relu=True)
    assert (hi1[hi == float("-inf")] == 0).all()              # -inf becomes 0 under ReLU


def test_nan_in_the_sum_demands_nan():
    x, wt, bias, res = nc.wide_range_layer(6, 7, 32, seed=3)
    bias = bias.clone()
    bias[5] = float("nan")
    lo, hi, s = nc.conv_interval(x, wt, bias, res, relu=True)
    assert torch.isnan(s[..., 5]).all() and not torch.isnan(s[..., :5]).any()
    got = nc.fp32_layer(x, wt, bias, res, relu=True)                       # torch.relu keeps the NaN
    assert int(nc.outside(got, lo, hi, s).sum()) == 0
    swallowed = torch.nan_to_num(got, nan=0.0)                             # fmaxf(NaN, 0) = 0
    assert int(nc.outside(swallowed, lo, hi, s).sum()) == 13 * 6 * 7


def test_pointwise_and_value_head_references():
    g = torch.Generator().manual_seed(11)
    a = (torch.randn(5, 42, 128, generator=g).abs() * 2.0 ** torch.randint(-8, 15, (128,), generator=g)).half()
    w = (torch.randn(32, 128, generator=g) * 0.05).half()
    b = torch.randn(32, generator=g)
    lo, hi, s = nc.pointwise_interval(a, w, b, relu=True)
    got = torch.relu(a.float() @ w.float().t() + b).half()
    assert int(nc.outside(got, lo, hi, s).sum()) == 0
    in_fp16 = torch.relu((a.float() @ w.float().t()).half() + b.half())          # the bias added in fp16
    assert int(nc.outside(in_fp16, lo, hi, s).sum()) >= 100
    fcw = (torch.randn(128, generator=g) * 1e-3).float()
    d, slack = nc.value_head_reference(a, fcw, 0.25)
    d32 = ((a.float().sum(dim=1) * fcw).sum(dim=1) / 42 + np.float32(0.25)).double()
    assert ((d32 - d).abs() <= slack).all() and (slack < 0.05 * d.abs().max()).all()
    assert ((a.float().sum(dim=1) * fcw).sum(dim=1).double() / 42 - d).abs().max() > slack.max()   # no bias: caught


def test_emulation_heads_track_float64():
    """fp16_emulation_heads restates both heads' storage points: close to the float64 network on
    a random-init network, and not equal to it."""
    from zeroclone_amd.nets import PolicyValueNetwork
    torch.manual_seed(2)
    for kind, nl in (("linear", 7), ("conv", 42 * 42)):
        net = PolicyValueNetwork(blocks=1, in_planes=2, board=(6, 7), n_logits=nl, head=kind).eval()
        x = (torch.rand(4, 2, 6, 7) < 0.3).half()
        v64, l64 = nc.network64(net, x)
        v16, l16 = nc.fp16_emulation_heads(net, x)
        assert v16.shape == v64.shape and l16.shape == l64.shape
        assert 0 < (v16 - v64).abs().max().item() < 1e-3
        assert 0 < (l16 - l64).abs().max().item() < 2e-2
