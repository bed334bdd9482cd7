"""The network kernels (csrc/net_conv.hip) on wide-range floats and non-finite values.

Every comparison of a layer is the interval of tests/nn_check.py: the kernel's exact fp16 /
fp32 inputs in float64, the worst-case error of an fp32 sum of k terms in any order, and the
fp16 values that interval rounds to — nothing measured on the code under test.  Along a chain
of layers each reference starts from the kernel's own previous output, so no error accumulates.
A NaN in the exact sum demands a NaN in the output (every ReLU keeps it), a sum far past
65520 demands the infinity, and -inf becomes 0 under ReLU."""
import functools

import numpy as np
import pytest
import torch

import nn_check as nc

pytestmark = pytest.mark.gpu

INF = float("inf")
BOARDS = [(17, 8, 8), (2, 6, 7)]


@pytest.fixture
def net_sw():
    """Set the network launches' switches (zc_debug_net_switch) for one test; restored after."""
    from zeroclone_amd import _native
    saved = {}

    def set_(name, value):
        old = _native.net_switch(name, value)
        saved.setdefault(name, old)
    yield set_
    for name, old in saved.items():
        _native.net_switch(name, old)


def same_bits(a, b) -> bool:
    """NaN at the same positions, every other element bit for bit."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(torch.equal(na, nb) and torch.equal(a.view(ints)[~na], b.view(ints)[~nb]))


def kernel_weights(wt):
    """[128, cin, 3, 3] fp16 -> the staged kernels' [9, 128, cin] and the packed form, on the GPU."""
    from zeroclone_amd import _native
    cin = wt.shape[1]
    wk = wt.permute(2, 3, 0, 1).reshape(9, 128, cin).contiguous().cuda()
    wp = torch.empty_like(wk)
    _native.check(_native.lib().zc_net_conv3x3_pack_async(cin, wk.data_ptr(), wp.data_ptr(), None))
    return wk, wp


def conv_weight_of(wk):
    """The inverse of the kernels' [9, 128, cin] layout: [128, cin, 3, 3] on the CPU."""
    return wk.cpu().reshape(3, 3, 128, wk.shape[2]).permute(2, 3, 0, 1).contiguous()


def run_layer(packed, x, w, bias, res, relu):
    """One launch of zc_net_conv3x3_packed_async / zc_net_conv3x3_async: x [n, h, w, cin] fp16 on
    the GPU, w that entry point's weights; returns the output on the CPU."""
    from zeroclone_amd import _native
    L = _native.lib()
    n, h, wd, cin = x.shape
    out = torch.full((n, h, wd, 128), 777.0, dtype=torch.float16, device="cuda")
    fn = L.zc_net_conv3x3_packed_async if packed else L.zc_net_conv3x3_async
    _native.check(fn(n, h, wd, cin, x.data_ptr(), w.data_ptr(), bias.data_ptr(), res.data_ptr() if res is not None else None,
                     out.data_ptr(), 1 if relu else 0, None))
    torch.cuda.synchronize()
    return out.cpu()


VARIANTS = [(False, True), (True, True), (True, False)]   # (residual, ReLU)


@functools.lru_cache(maxsize=None)
def layer_case(h, w, cin, overflow):
    """One generated layer and its three variants' intervals, computed once for every form."""
    x, wt, bias, res = nc.wide_range_layer(h, w, cin, seed=1000 * h + cin + (7 if overflow else 0), overflow=overflow)
    assert nc.has_subnormals(wt), "no fp16-subnormal weight"
    assert nc.has_subnormals(x), "no fp16-subnormal stored activation"
    refs = {}
    for use_res, relu in VARIANTS:
        lo, hi, s = nc.conv_interval(x, wt, bias, res if use_res else None, relu=relu)
        share = nc.ambiguous_share(lo, hi)
        assert (share if relu else 0.5 * share) < 0.5   # without the ReLU both halves of the sums count
        if overflow:   # about 1 % of the sums past 65520 each way: +inf, and -inf (0 under ReLU)
            assert 0.005 < float((lo == INF).double().mean()) < 0.03
            assert 0.005 < float((s < -70000).double().mean()) < 0.03
            assert (hi == (0.0 if relu else -INF))[s < -70000].all()
            at = int((bias == 65520.0).nonzero()[0])   # this channel's sums lie on both sides of 65520
            assert (lo[..., at] == INF).any() and (hi[..., at] < INF).any()
        refs[(use_res, relu)] = (lo, hi, s)
    return x, wt, bias, res, refs


@pytest.mark.parametrize("mf", [32, 16])
@pytest.mark.parametrize("shape", [(8, 8, 128), (6, 7, 128), (8, 8, 32), (6, 7, 32)], ids=lambda s: "x".join(map(str, s)))
def test_single_layer_within_the_interval(shape, mf, net_sw):
    """zc_net_conv3x3_async and zc_net_conv3x3_packed_async (both MFMA forms) on 13 boards of the
    wide-range generator and on its overflow set: every element inside the interval."""
    net_sw("tower_mf", mf)
    h, w, cin = shape
    for overflow in (False, True):
        x, wt, bias, res, refs = layer_case(h, w, cin, overflow)
        wk, wp = kernel_weights(wt)
        xg, bg, rg = x.cuda(), bias.cuda(), res.cuda()
        for (use_res, relu), (lo, hi, s) in refs.items():
            for packed in (False, True):
                got = run_layer(packed, xg, wp if packed else wk, bg, rg if use_res else None, relu)
                bad = nc.outside(got, lo, hi, s)
                assert int(bad.sum()) == 0, (shape, mf, overflow, use_res, relu, packed, int(bad.sum()),
                                             got[bad][:4].tolist(), s[bad][:4].tolist())
                if overflow:
                    assert torch.isposinf(got).any() and (relu or torch.isneginf(got).any())


# ---- the wide-range networks ------------------------------------------------------------------

def planes(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, c, h, w, generator=g) < 0.3).half()


def nhwc32(x):
    """state_to_tensor planes [n, c, h, w] -> the tower's input [n, h, w, 32] (zero padded)."""
    n, c, h, w = x.shape
    out = torch.zeros(n, h, w, 32, dtype=torch.float16)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out


@functools.lru_cache(maxsize=None)
def wide_value_net(c, h, w):
    """ValueNetwork(128, 2) with a trained network's BN spread, scaled until the float64
    emulation's last activation peaks between 1e3 and 6e4 on the 131 test boards."""
    from zeroclone_amd.nets import FoldedValueNetwork, ValueNetwork
    torch.manual_seed(40 + c)
    net = nc.widen_bn(ValueNetwork(128, 2, in_planes=c), seed=c)
    x = planes(131, c, h, w, seed=9)
    nc.scale_tower(net, x[:16])
    a = nc.fp16_emulation_activation(FoldedValueNetwork(net), x)
    assert torch.isfinite(a).all() and 1e3 <= a.max().item() <= 6e4
    return net


@functools.lru_cache(maxsize=None)
def wide_policy_net(c, h, w, head):
    """PolicyValueNetwork on the wide-range tower (2 blocks), its policy BN widened the same way."""
    from zeroclone_amd.nets import FoldedValueNetwork, PolicyValueNetwork, _fold
    torch.manual_seed(50 + c)
    net = PolicyValueNetwork(blocks=2, in_planes=c, board=(h, w), n_logits=4096 if (h, w) == (8, 8) else 7, head=head)
    nc.widen_bn(net, seed=c + 1)
    x = planes(53, c, h, w, seed=10)
    nc.scale_tower(net, x[:16])
    a = nc.fp16_emulation_activation(FoldedValueNetwork(net.value_network()), x)
    assert torch.isfinite(a).all() and 1e3 <= a.max().item() <= 6e4
    with torch.no_grad():   # the 1x1 conv's outputs up to 3e4 (finite in fp16), but for one channel
        f = _fold(net.policy[0], net.policy[1])          # whose bias sends it to -inf (0 under ReLU)
        peak = torch.nn.functional.conv2d(a, f.weight.double(), f.bias.double()).abs().max().item()
        net.policy[1].weight.mul_(3.0e4 / peak)
        net.policy[1].bias.mul_(3.0e4 / peak)
        net.policy[1].bias[3] = -3.0e5
    return net


def layered(mnet, x0, check=None, staged=False):
    """The tower layer by layer on the packed kernel from x0 [n, h, w, 32] (GPU); check(i, got,
    src, res, wt, bias) sees every layer's output (CPU).  staged: each layer also through
    zc_net_conv3x3_async, which must store the same bits.  Returns the last activation (CPU)."""
    def conv(i, src, res):
        got = run_layer(True, src, mnet.wp[i], mnet.b[i], res, True)
        if staged:
            assert same_bits(run_layer(False, src, mnet.w[i], mnet.b[i], res, True), got), ("staged", i)
        if check is not None:
            check(i, got, src.cpu(), res.cpu() if res is not None else None, conv_weight_of(mnet.w[i]), mnet.b[i].cpu())
        return got.cuda()
    a = conv(0, x0, None)
    for k in range((len(mnet.w) - 1) // 2):
        t = conv(1 + 2 * k, a, None)
        a = conv(2 + 2 * k, t, a)
    return a.cpu()


def interval_check(tag):
    def check(i, got, src, res, wt, bias):
        lo, hi, s = nc.conv_interval(src, wt, bias, res, relu=True)
        bad = nc.outside(got, lo, hi, s)
        assert int(bad.sum()) == 0, (tag, "layer", i, int(bad.sum()), got[bad][:4].tolist(), s[bad][:4].tolist())
    return check


FUSED_FORMS = [32, 16, 0]   # tower_mf; 0 the default pairing


@pytest.mark.parametrize("board", BOARDS, ids=["8x8", "6x7"])
def test_wide_range_tower_layer_by_layer_and_fused(board, net_sw):
    """The wide-range tower: every layer of the layered path inside its interval (from the
    kernel's own previous output), in both MFMA forms bit for bit; every fused form
    bit-identical to the layered activation."""
    from zeroclone_amd.nets import MfmaValueNetwork
    c, h, w = board
    mnet = MfmaValueNetwork(wide_value_net(c, h, w))
    assert any(nc.has_subnormals(wk) for wk in mnet.w)
    x = planes(131, c, h, w, seed=9)
    for n in (1, 5, 131):
        xs = x[:n].contiguous()
        x0 = nhwc32(xs).cuda()
        net_sw("tower_mf", 32)
        want = layered(mnet, x0, interval_check((board, n)))
        assert want.max().item() >= (1e3 if n == 131 else 1.0)
        net_sw("tower_mf", 16)
        assert same_bits(layered(mnet, x0), want), (board, n, "layered, 16x16x32")
        for mf in FUSED_FORMS:
            net_sw("tower_mf", mf)
            a, _ = mnet.tower(xs.cuda(), fused=True)
            torch.cuda.synchronize()
            assert same_bits(a.cpu().reshape(want.shape), want), (board, n, mf)


# ---- the value head ---------------------------------------------------------------------------

def check_values(got, act, fcw, fcb, raw, what):
    d, slack = nc.value_head_reference(act, fcw, fcb)
    got = got.cpu()
    if raw:
        assert ((got - d).abs() <= slack).all(), (what, (got - d).abs().max().item(), slack.max().item())
        return d, slack
    assert ((got - torch.tanh(d)).abs() <= slack + 1e-6).all(), (what, (got - torch.tanh(d)).abs().max().item())
    assert (got.abs() <= 1.0).all(), what
    big = d.abs() > 10
    assert torch.equal(got[big], torch.sign(d[big])), what
    return d, slack


@pytest.mark.parametrize("hw", [64, 42])
def test_value_head_on_synthetic_activations(hw, net_sw):
    """zc_net_value_head_async on activations up to 6e4 whose channels come in pairs with
    opposite Linear weights: the 128-term sum cancels to O(1), so an fp16 or a badly ordered
    accumulation shows.  Pre-tanh within the slack of float64; tanh within slack + 1e-6, never
    past +-1 and exactly +-1 past |d| = 10.  The same on nn_check.spread_head_inputs, every
    channel with an activation and a weight of its own, which shows what cancels in a pair
    (tests/test_net_interval_cpu.py:test_wrong_value_heads_fall_outside_the_slack)."""
    from zeroclone_amd import _native
    L = _native.lib()
    g = torch.Generator().manual_seed(hw)
    for n in (1, 5):
        sets = {"cancelling": nc.cancelling_head_inputs(g, n, hw, 128),
                "spread": nc.spread_head_inputs(1000 * 128 + 10 * hw + n, n, hw, 128)}
        for name, (act, fcw) in sets.items():
            assert act.max().item() > 5.0e4 and torch.isfinite(act).all()
            ag, wg = act.cuda(), fcw.cuda()
            for fcb in nc.HEAD_FCBS:
                d, slack = nc.value_head_reference(act, fcw, fcb)
                assert slack.max().item() < 0.5 and (d - float(np.float32(fcb))).abs().max().item() < 2.0   # it cancels
                for raw in (1, 0):
                    net_sw("head_raw", raw)
                    vals = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
                    _native.check(L.zc_net_value_head_async(n, hw, ag.data_ptr(), wg.data_ptr(), fcb, vals.data_ptr(), None))
                    torch.cuda.synchronize()
                    check_values(vals, act, fcw, fcb, raw, (hw, n, name, fcb, raw))
                if abs(fcb) > 10:
                    assert (d.abs() > 10).all()


@pytest.mark.parametrize("board", BOARDS, ids=["8x8", "6x7"])
def test_fused_value_head_on_the_wide_range_network(board, net_sw):
    """The head inside the tower launch on activations in the thousands: within the slack of
    float64 on the activation the same launch wrote, and the unfused head's bits."""
    from zeroclone_amd.nets import MfmaValueNetwork
    c, h, w = board
    mnet = MfmaValueNetwork(wide_value_net(c, h, w))
    fcw = mnet.fcw.cpu()
    for n in (1, 5):
        x = planes(131, c, h, w, seed=9)[:n].cuda()
        for raw in (1, 0):
            net_sw("head_raw", raw)
            a, vals = mnet.tower(x, head=True)
            fused = vals.clone()
            act = a.cpu().clone()
            assert same_bits(mnet(x).clone(), fused)                      # without writing the activation
            assert same_bits(mnet(x, fused=False).clone(), fused)         # layered tower + zc_net_value_head_async
            check_values(fused, act, fcw, mnet.fcb, raw, (board, n, raw))


# ---- the policy 1x1 conv ----------------------------------------------------------------------

def policy_operands(net):
    from zeroclone_amd.nets import _fold
    f = _fold(net.policy[0], net.policy[1])
    return f.weight.detach().float().reshape(f.out_channels, -1).half(), f.bias.detach().float()


@pytest.mark.parametrize("case", [(17, 8, 8, "linear", 37), (2, 6, 7, "linear", 53), (17, 8, 8, "conv", 37)],
                         ids=["8x8-linear", "6x7-linear", "8x8-conv"])
def test_policy_conv_within_the_interval(case):
    """The 1x1 policy conv of the fused launch (P = 32 with ReLU; P = 64 logits without) on the
    wide-range tower, against float64 of the activation tower(head=True) returns: k = 129.
    One logit channel's bias sends it to -inf (0 under ReLU).  Values: the value-only launch's."""
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    c, h, w, head, n = case
    net = wide_policy_net(c, h, w, head)
    mnet = MfmaPolicyValueNetwork(net)
    assert mnet.fused
    x = planes(53, c, h, w, seed=10)[:n].cuda()
    v, logits = mnet(x)
    v, logits = v.clone(), logits.clone()
    pout = mnet._pout[(n, h * w)].cpu().clone()
    a, _ = mnet.tower.tower(x, head=True)
    act = a.cpu().clone()
    assert same_bits(mnet.tower(x).clone(), v)
    pw, pb = policy_operands(net)
    relu = head == "linear"
    lo, hi, s = nc.pointwise_interval(act, pw, pb, relu=relu)
    assert act.max().item() >= 1e3 and (s < -70000).any()
    bad = nc.outside(pout, lo, hi, s)
    assert int(bad.sum()) == 0, (case, int(bad.sum()), pout[bad][:4].tolist(), s[bad][:4].tolist())
    if relu:
        assert (pout[..., 3] == 0).all() and (pout > 0).any()
    else:
        assert torch.isneginf(pout[..., 3]).all() and torch.isfinite(pout).any()
        assert same_bits(logits.cpu(), pout.reshape(n, -1))      # the conv head's logits are that output


# ---- end to end ---------------------------------------------------------------------------------

@pytest.mark.parametrize("head", ["linear", "conv"])
def test_policy_value_network_tracks_float64(head):
    """MfmaPolicyValueNetwork against the float64 network, with a wide value head (values std
    >= 0.3) and logits of std >= 0.3: Pearson >= 0.999 and max error within 4 x the error of
    the fp16-storage emulation against float64 on the same inputs (computed here, from the
    references alone).  Why 4: the kernels accumulate in fp32, which may flip a storage rounding
    relative to the emulation's exact sums, and flips compound over the 5 layers."""
    from zeroclone_amd.nets import FoldedValueNetwork, MfmaPolicyValueNetwork, PolicyValueNetwork
    torch.manual_seed(0)
    net = PolicyValueNetwork(blocks=2, head=head).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * torch.rand(m.num_features, generator=g) - 0.1)
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    x = planes(37, 17, 8, 8, seed=2)
    cal = planes(64, 17, 8, 8, seed=3)
    wv, bv = nc.wide_head(nc.features64(FoldedValueNetwork(net.value_network()), cal.float()))
    with torch.no_grad():
        net.head[2].weight.copy_(wv.reshape(1, -1))
        net.head[2].bias.fill_(bv)
        _, l64 = nc.network64(net, x)
        last = net.policy[4] if head == "linear" else net.policy[1]   # spread the logits: std 0.5
        last.weight.mul_(0.5 / l64.std().item())
        if head == "linear":
            last.bias.mul_(0.5 / l64.std().item())
    v64, l64 = nc.network64(net, x)
    v16, l16 = nc.fp16_emulation_heads(net, x)
    emu_v, emu_l = (v16 - v64).abs().max().item(), (l16 - l64).abs().max().item()
    v, lg = MfmaPolicyValueNetwork(net)(x.cuda())
    v, lg = v.cpu(), lg.double().cpu()
    err_v, err_l = (v - v64).abs().max().item(), (lg - l64).abs().max().item()
    print(f"{head} head: emulation error values {emu_v:.3e} logits {emu_l:.3e}; kernel error values {err_v:.3e} "
          f"logits {err_l:.3e}; std values {v64.std().item():.3f} logits {l64.std().item():.3f}")
    nc.assert_tracks(v.numpy(), v64.numpy(), 4 * emu_v, min_r=0.999, min_std=0.3, what=f"{head}: values")
    nc.assert_tracks(lg.numpy(), l64.numpy(), 4 * emu_l, min_r=0.999, min_std=0.3, what=f"{head}: logits")


# ---- non-finite values ----------------------------------------------------------------------------

POISON = {2: 60000.0, 5: INF, 8: float("nan")}    # board -> what one of its planes holds
NB = 11                                             # boards: each poisoned one has a clean tile neighbour


def poisoned(c, h, w):
    x = planes(NB, c, h, w, seed=12)
    bad = x.clone()
    bad[2, 0] = 60000.0          # the whole plane: the stem overflows, the next layer forms inf - inf
    bad[5, 1, 3, 3] = INF
    bad[8, c - 1, 2, 4] = float("nan")
    return x, bad


def clean_rows(t):
    return t[[i for i in range(NB) if i not in POISON]]


@pytest.mark.parametrize("board", BOARDS, ids=["8x8", "6x7"])
def test_non_finite_inputs_reach_every_output(board, net_sw):
    """60000, +inf and NaN in a plane of three boards of eleven.  Layer by layer (packed and
    staged kernels) each output is what float64 with ReLU and the fp16 storage rounding demands
    of the kernel's own input: NaN stays NaN through every ReLU store, +inf stays, -inf becomes
    0.  Every fused form stores the layered activation; the value of every poisoned board is
    what float64 makes of its activation (NaN); the clean boards, tile neighbours included,
    hold the bits of a launch without the poison."""
    from zeroclone_amd.nets import MfmaValueNetwork
    c, h, w = board
    mnet = MfmaValueNetwork(wide_value_net(c, h, w))
    x, bad = poisoned(c, h, w)
    seen = {"inf": False}

    def check(i, got, src, res, wt, bias):
        interval_check((board, "poisoned"))(i, got, src, res, wt, bias)
        seen["inf"] |= bool(torch.isposinf(got[2]).any())
        if i >= 1:
            assert all(torch.isnan(got[b]).any() for b in POISON), (board, i)
    net_sw("tower_mf", 32)
    want = layered(mnet, nhwc32(bad).cuda(), check, staged=True)
    clean = layered(mnet, nhwc32(x).cuda())
    assert seen["inf"] and not torch.isnan(clean).any()
    assert same_bits(clean_rows(want), clean_rows(clean))
    fcw = mnet.fcw.cpu()
    d, _ = nc.value_head_reference(want.reshape(NB, h * w, 128), fcw, mnet.fcb)
    assert torch.isnan(d[list(POISON)]).all() and torch.isfinite(clean_rows(d)).all()
    for mf in FUSED_FORMS:
        net_sw("tower_mf", mf)
        a, vals = mnet.tower(bad.cuda(), head=True)
        got_a, got_v = a.cpu().clone().reshape(want.shape), vals.cpu().clone()
        assert same_bits(got_a, want), (board, mf)
        assert torch.equal(torch.isnan(got_v), torch.isnan(d)), (board, mf, got_v.tolist())
        assert same_bits(mnet(bad.cuda()).cpu(), got_v) and same_bits(mnet(bad.cuda(), fused=False).cpu(), got_v)
        a, vals = mnet.tower(x.cuda(), head=True)
        assert same_bits(clean_rows(a.cpu().reshape(want.shape)), clean_rows(want))
        assert same_bits(clean_rows(vals.cpu()), clean_rows(got_v))


@pytest.mark.parametrize("case", [(17, 8, 8, "linear"), (2, 6, 7, "linear"), (17, 8, 8, "conv")],
                         ids=["8x8-linear", "6x7-linear", "8x8-conv"])
def test_non_finite_inputs_reach_pout_and_logits(case):
    """The same three boards through zc_net_tower_policy_ex_async (the conv head from NHWC
    [n, 64, 32] planes): pout is what float64 makes of the activation of tower(head=True), NaN
    on every pixel the activation holds a NaN; the poisoned boards' values and logits are NaN;
    the clean boards hold the bits of the clean launch."""
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    c, h, w, head = case
    net = wide_policy_net(c, h, w, head)
    mnet = MfmaPolicyValueNetwork(net)
    x, bad = poisoned(c, h, w)
    as_input = (lambda t: nhwc32(t).reshape(NB, h * w, 32).cuda()) if head == "conv" else (lambda t: t.cuda())
    v, logits = mnet(as_input(bad))
    v, logits, pout = v.cpu().clone(), logits.cpu().clone(), mnet._pout[(NB, h * w)].cpu().clone()
    a, _ = mnet.tower.tower(bad.cuda(), head=True)
    act = a.cpu().clone()
    pw, pb = policy_operands(net)
    lo, hi, s = nc.pointwise_interval(act, pw, pb, relu=head == "linear")
    assert int(nc.outside(pout, lo, hi, s).sum()) == 0
    for b in POISON:
        assert torch.isnan(act[b]).any() and torch.isnan(pout[b]).any() and torch.isnan(v[b]), (case, b)
        assert torch.isnan(logits[b]).any(), (case, b)
    v0, logits0 = mnet(as_input(x))
    assert not torch.isnan(v0).any() and not torch.isnan(logits0).any()
    assert same_bits(clean_rows(v0.cpu()), clean_rows(v))
    assert same_bits(clean_rows(mnet._pout[(NB, h * w)].cpu()), clean_rows(pout))
    assert same_bits(clean_rows(logits0.cpu()), clean_rows(logits))


@pytest.mark.parametrize("board", BOARDS, ids=["8x8", "6x7"])
def test_counted_launches_with_non_finite_rows(board):
    """zc_net_tower_counted_async and zc_net_tower_policy_counted_async, count = 7 of 11: the
    poisoned boards below the count give the plain launch's outputs (NaN kept), and the rows
    past it — board 7, the last counted board's tile neighbour, holds NaN planes, board 8 too —
    leave their outputs untouched."""
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    c, h, w = board
    mnet = MfmaPolicyValueNetwork(wide_policy_net(c, h, w, "linear"))
    tower = mnet.tower
    _, bad = poisoned(c, h, w)
    bad[7] = float("nan")
    xg = bad.cuda()
    cnt = torch.tensor([7], dtype=torch.int32, device="cuda")
    a, vals = tower.tower(xg, head=True)
    want_a, want_v = a.clone(), vals.clone()
    pout = torch.empty((NB, h * w, 32), dtype=torch.float16, device="cuda")
    want_pv = tower.tower_policy(xg, mnet.pw, mnet.pb, pout).clone()
    want_p = pout.clone()
    assert torch.isnan(want_v[[2, 5]]).all() and torch.isnan(want_p[2]).any() and torch.isnan(want_p[5]).any()
    a.fill_(-3.0)
    vals.fill_(-3.0)
    a2, v2 = tower.tower(xg, head=True, count=cnt)
    torch.cuda.synchronize()
    assert same_bits(a2[:7], want_a[:7]) and same_bits(v2[:7], want_v[:7])
    assert (a2[7:] == -3.0).all() and (v2[7:] == -3.0).all()
    pout.fill_(-3.0)
    vals.fill_(-3.0)
    v3 = tower.tower_policy(xg, mnet.pw, mnet.pb, pout, count=cnt)
    torch.cuda.synchronize()
    assert same_bits(pout[:7], want_p[:7]) and same_bits(v3[:7], want_pv[:7])
    assert (pout[7:] == -3.0).all() and (v3[7:] == -3.0).all()


@pytest.mark.parametrize("count", [0, -1, -2 ** 31])
@pytest.mark.parametrize("board", BOARDS, ids=["8x8", "6x7"])
def test_counted_launches_with_no_rows_to_evaluate(board, count, net_sw):
    """zc_net_tower_counted_async and zc_net_tower_policy_counted_async, capacity 11, in every
    fused form: "a negative count is 0" (include/zeroclone.h), so with -1 and -2^31 as with 0
    every row of a sentinel-filled activation, values and pout keeps its sentinel."""
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    c, h, w = board
    mnet = MfmaPolicyValueNetwork(wide_policy_net(c, h, w, "linear"))
    tower = mnet.tower
    xg = planes(NB, c, h, w, seed=21).cuda()
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    assert int(cnt.item()) == count
    pout = torch.empty((NB, h * w, 32), dtype=torch.float16, device="cuda")
    for mf in FUSED_FORMS:
        net_sw("tower_mf", mf)
        a, vals = tower.tower(xg, head=True)
        tower.tower_policy(xg, mnet.pw, mnet.pb, pout)
        assert a.abs().sum().item() > 0 and pout.abs().sum().item() > 0 and (vals != -3.0).all()   # the plain launches write
        a.fill_(-3.0)
        vals.fill_(-3.0)
        a2, v2 = tower.tower(xg, head=True, count=cnt)
        torch.cuda.synchronize()
        assert a2.data_ptr() == a.data_ptr() and v2.data_ptr() == vals.data_ptr()
        assert (a2 == -3.0).all() and (v2 == -3.0).all(), (board, count, mf)
        pout.fill_(-3.0)
        v3 = tower.tower_policy(xg, mnet.pw, mnet.pb, pout, count=cnt)
        torch.cuda.synchronize()
        assert (pout == -3.0).all() and (v3 == -3.0).all(), (board, count, mf)


@pytest.mark.parametrize("what", ["bias", "weight"])
@pytest.mark.parametrize("board", BOARDS, ids=["8x8", "6x7"])
def test_nan_parameter_reaches_every_output(board, what, net_sw):
    """A NaN folded bias at one channel of block 1's first conv, or one NaN weight (the centre
    tap: no zero padding meets it): that output channel is NaN on every pixel (the layered
    interval check demands it at the first ReLU already), and every board's activation, value,
    pout and logits hold NaN in every fused form."""
    import copy
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    c, h, w = board
    net = copy.deepcopy(wide_policy_net(c, h, w, "linear"))
    with torch.no_grad():
        if what == "bias":
            net.res[0].seq[1].bias[7] = float("nan")
        else:
            net.res[0].seq[0].weight[9, 3, 1, 1] = float("nan")
    mnet = MfmaPolicyValueNetwork(net)
    ch = 7 if what == "bias" else 9
    x = planes(5, c, h, w, seed=13)

    def check(i, got, src, res, wt, bias):
        interval_check((board, what))(i, got, src, res, wt, bias)
        if i == 1:
            assert torch.isnan(got[..., ch]).all() and not torch.isnan(got[..., :ch]).any()
    net_sw("tower_mf", 32)
    want = layered(mnet.tower, nhwc32(x).cuda(), check, staged=True)
    assert torch.isnan(want).any(dim=(1, 2, 3)).all()
    for mf in FUSED_FORMS:
        net_sw("tower_mf", mf)
        a, vals = mnet.tower.tower(x.cuda(), head=True)
        assert same_bits(a.cpu().reshape(want.shape), want), (board, what, mf)
        assert torch.isnan(vals).all()
        v, logits = mnet(x.cuda())
        assert torch.isnan(v).all() and torch.isnan(mnet._pout[(5, h * w)]).any(dim=(1, 2)).all()
        assert torch.isnan(logits).any(dim=1).all()


def test_pool_with_a_nan_bias_stops_every_game():
    """A 4-game Connect4 pool at 8 simulations whose network — the real MFMA tower, value head
    and policy head — has a NaN BN bias in block 1: the search of every game ends with
    ZC_STATUS_INTERNAL (the backup's fence on the NaN value) and check() raises."""
    from zeroclone_amd import _native
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, MfmaValueNetwork, PolicyValueNetwork
    from zeroclone_amd.selfplay import C4SelfPlay
    torch.manual_seed(0)
    net = PolicyValueNetwork(blocks=2, in_planes=2, board=(6, 7), n_logits=7).eval()
    with torch.no_grad():
        net.res[0].seq[1].bias[7] = float("nan")
    pnet = MfmaPolicyValueNetwork(net)
    assert isinstance(pnet.tower, MfmaValueNetwork)
    pool = C4SelfPlay(4, 8, batch_size=8, seed=3, puct_net=pnet)
    try:
        pool.step_search()
        torch.cuda.synchronize()
        assert pool.stats[:, 5].cpu().tolist() == [_native.ZC_STATUS_INTERNAL] * 4
        with pytest.raises(RuntimeError, match="ZC_STATUS_INTERNAL"):
            pool.check()
    finally:
        pool.close()
