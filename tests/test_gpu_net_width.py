"""The 64-channel network kernels (csrc/net_conv64.hip) through the C ABI's _w_ family and
nets.MfmaValueNetwork / MfmaPolicyValueNetwork: one layer inside a derived interval, the fused
tower exact on integers, fused = layered bit for bit, the heads, the counted forms, non-finite
values and the refusals.  The references are tests/nn_check.py's (float64 on the kernel's exact
inputs); nothing here is measured on the code under test."""
import functools

import numpy as np
import pytest
import torch

import nn_check as nc

pytestmark = pytest.mark.gpu

INF = float("inf")
C = 64
BOARDS = [(17, 8, 8), (2, 6, 7)]
BOARD_IDS = ["8x8", "6x7"]


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


def planes(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, c, h, w, generator=g) < 0.3).half()


def nhwc32(x):
    """state_to_tensor planes [n, c, h, w] -> the tower's input [n, h, w, 32] (zero padded)."""
    n, c, h, w = x.shape
    out = torch.zeros(n, h, w, 32, dtype=torch.float16)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out


def kernel_weights(wt):
    """[64, cin, 3, 3] fp16 -> [9, 64, cin] and the packed form (zc_net_conv3x3_pack_w_async), on the GPU."""
    from zeroclone_amd import _native
    cin = wt.shape[1]
    wk = wt.permute(2, 3, 0, 1).reshape(9, C, cin).contiguous().cuda()
    wp = torch.empty_like(wk)
    _native.check(_native.lib().zc_net_conv3x3_pack_w_async(C, cin, wk.data_ptr(), wp.data_ptr(), None))
    return wk, wp


def conv_weight_of(wk):
    """The inverse of [9, 64, cin]: [64, cin, 3, 3] on the CPU."""
    return wk.cpu().reshape(3, 3, C, wk.shape[2]).permute(2, 3, 0, 1).contiguous()


def run_layer(x, wp, bias, res, relu):
    """One launch of zc_net_conv3x3_packed_w_async at 64 channels; the output on the CPU."""
    from zeroclone_amd import _native
    n, h, wd, cin = x.shape
    out = torch.full((n, h, wd, C), 777.0, dtype=torch.float16, device="cuda")
    _native.check(_native.lib().zc_net_conv3x3_packed_w_async(
        C, n, h, wd, cin, x.data_ptr(), wp.data_ptr(), bias.data_ptr(), res.data_ptr() if res is not None else None,
        out.data_ptr(), 1 if relu else 0, None))
    torch.cuda.synchronize()
    return out.cpu()


# ---- 1. one layer inside a derived interval ---------------------------------------------------

VARIANTS = [(False, True), (True, True), (True, False)]   # (residual, ReLU)


@functools.lru_cache(maxsize=None)
def layer_case(h, w, cin, overflow):
    """One generated layer (13 boards, 64 output channels) and its three variants' intervals."""
    x, wt, bias, res = nc.wide_range_layer(h, w, cin, seed=640 * h + cin + (7 if overflow else 0), cout=C,
                                           overflow=overflow)
    assert x.shape[0] == 13
    assert nc.has_subnormals(wt), "no fp16-subnormal weight"
    assert nc.has_subnormals(x), "no fp16-subnormal stored activation"
    refs = {}
    for use_res, relu in VARIANTS:
        lo, hi, s = nc.conv_interval(x, wt, bias, res if use_res else None, relu=relu)
        share = nc.ambiguous_share(lo, hi)
        assert (share if relu else 0.5 * share) < 0.5   # without the ReLU both halves of the sums count
        if overflow:   # five moved channels of 64: about 3 % of the sums past 65520 each way
            assert 0.02 <= float((lo == INF).double().mean()) <= 0.05
            assert 0.02 <= float((s < -70000).double().mean()) <= 0.05
            assert (hi == (0.0 if relu else -INF))[s < -70000].all()
        refs[(use_res, relu)] = (lo, hi, s)
    return x, wt, bias, res, refs


@pytest.mark.parametrize("shape", [(8, 8, 64), (6, 7, 64), (8, 8, 32), (6, 7, 32)], ids=lambda s: "x".join(map(str, s)))
def test_single_layer_within_the_interval(shape):
    """zc_net_conv3x3_packed_w_async at 64 channels on 13 boards of the wide-range generator and
    on its overflow set: every element inside the interval."""
    h, w, cin = shape
    for overflow in (False, True):
        x, wt, bias, res, refs = layer_case(h, w, cin, overflow)
        _, wp = kernel_weights(wt)
        xg, bg, rg = x.cuda(), bias.cuda(), res.cuda()
        for (use_res, relu), (lo, hi, s) in refs.items():
            got = run_layer(xg, wp, bg, rg if use_res else None, relu)
            bad = nc.outside(got, lo, hi, s)
            assert int(bad.sum()) == 0, (shape, overflow, use_res, relu, int(bad.sum()), got[bad][:4].tolist(),
                                         s[bad][:4].tolist())
            if overflow:
                assert torch.isposinf(got).any() and (relu or torch.isneginf(got).any())


# ---- 2. the tower on integers, exactly --------------------------------------------------------

def integer_net(c, blocks, seed):
    """tests/test_gpu_net.py:_integer_net at 64 channels: sparse small-integer convs (density 0.004
    for the 64 -> 64 convs, 0.02 for the stem), identity BN with integer biases."""
    from zeroclone_amd.nets import ValueNetwork
    g = torch.Generator().manual_seed(seed)
    net = ValueNetwork(C, blocks, in_planes=c).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            keep = torch.rand(m.weight.shape, generator=g) < (0.004 if m.in_channels == C else 0.02)
            m.weight.data = torch.randint(-2, 3, m.weight.shape, generator=g).float() * keep
        elif isinstance(m, torch.nn.BatchNorm2d):
            m.eps = 0.0
            m.running_mean.zero_()
            m.running_var.fill_(1.0)
            m.weight.data.fill_(1.0)
            m.bias.data = torch.randint(-1, 3, m.bias.shape, generator=g).float()
    return net


@pytest.mark.parametrize("blocks", [0, 1, 2, 3])
@pytest.mark.parametrize("board", BOARDS, ids=BOARD_IDS)
def test_tower_exact_on_integers(board, blocks):
    """The fused tower on an integer network equals float64 bit for bit: the MFMA operand and
    accumulator layouts, tap shifts, board edges, the in-place residual and ragged tiles (a tile
    is 2 chess or 3 Connect4 boards; 1 and 3 blocks end in the same buffer, through another
    number of swaps).  0 blocks: the stem alone (nconv = 1), a layer with no next layer's weights
    to fetch."""
    from zeroclone_amd.nets import FoldedValueNetwork, MfmaValueNetwork
    c, h, w = board
    vnet = integer_net(c, blocks, seed=h * 10 + blocks)
    net = MfmaValueNetwork(vnet)
    assert net.channels == C
    assert len(net.w) == len(net.wp) == 1 + 2 * blocks and net.ball.shape == (1 + 2 * blocks, C)
    assert net.wall.numel() == 9 * C * 32 + 2 * blocks * 9 * C * C   # 0 blocks: the stem's weights alone
    f = FoldedValueNetwork(vnet).double()
    for n in (1, 5, 12, 13, 131):
        x = planes(n, c, h, w, seed=100 + n)
        got, _ = net.tower(x.cuda(), fused=True)
        torch.cuda.synchronize()
        with torch.no_grad():
            want = f.res(torch.relu(f.stem(x.double()))).permute(0, 2, 3, 1).reshape(n, h * w, C)
        assert want.abs().max().item() < 2048 and want.abs().sum().item() > 0
        assert got.dtype == torch.float16 and got.shape == (n, h * w, C)
        assert torch.equal(got.double().cpu(), want), (board, blocks, n)


# ---- 3. fused = layered, bit for bit ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def wide_value_net(c, h, w):
    """ValueNetwork(64, 2) with a trained network's BN spread, scaled until the float64
    emulation's last activation peaks near 2e4 on the test boards."""
    from zeroclone_amd.nets import FoldedValueNetwork, ValueNetwork
    torch.manual_seed(64 + c)
    net = nc.widen_bn(ValueNetwork(C, 2, in_planes=c), seed=c)
    x = planes(131, c, h, w, seed=9)
    nc.scale_tower(net, x[:16])
    a = nc.fp16_emulation_activation(FoldedValueNetwork(net), x)
    assert torch.isfinite(a).all() and 1e3 <= a.max().item() <= 6e4
    return net


def layered(mnet, x0, check=None):
    """The tower layer by layer on the per-layer kernel from x0 [n, h, w, 32] (GPU); check(i, got,
    src, res, wt, bias) sees every layer's output (CPU).  Returns the last activation (CPU)."""
    def conv(i, src, res):
        got = run_layer(src, mnet.wp[i], mnet.b[i], res, True)
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


@pytest.mark.parametrize("board", BOARDS, ids=BOARD_IDS)
def test_wide_range_tower_layer_by_layer_and_fused(board, net_sw):
    """The wide-range 64-channel tower: every layer of the layered path inside its interval (from
    the kernel's own previous output); the fused activation has the layered path's bits; the
    fused value head has the stand-alone head's."""
    from zeroclone_amd.nets import MfmaValueNetwork
    c, h, w = board
    mnet = MfmaValueNetwork(wide_value_net(c, h, w))
    x = planes(131, c, h, w, seed=9)
    for n in (1, 5, 131):
        xs = x[:n].contiguous()
        want = layered(mnet, nhwc32(xs).cuda(), interval_check((board, n)))
        assert want.max().item() >= (1e3 if n == 131 else 1.0)
        a, _ = mnet.tower(xs.cuda(), fused=False)
        assert same_bits(a.cpu().reshape(want.shape), want), (board, n, "tower(fused=False)")
        a, _ = mnet.tower(xs.cuda(), fused=True)
        torch.cuda.synchronize()
        assert same_bits(a.cpu().reshape(want.shape), want), (board, n)
        for raw in (1, 0):
            net_sw("head_raw", raw)
            a, vals = mnet.tower(xs.cuda(), head=True)
            fused = vals.clone()
            assert same_bits(a.cpu().reshape(want.shape), want)
            assert same_bits(mnet(xs.cuda()).clone(), fused)                    # without writing the activation
            assert same_bits(mnet(xs.cuda(), fused=False).clone(), fused)       # layered + zc_net_value_head_w_async
            assert torch.isfinite(fused).all() and (raw == 0 or fused.abs().sum().item() > 0)


# ---- 4. the heads -----------------------------------------------------------------------------

def check_values(got, act, fcw, fcb, raw, what):
    d, slack = nc.value_head_reference(act, fcw, fcb)
    got = got.cpu()
    if raw:
        assert ((got - d).abs() <= slack).all(), (what, (got - d).abs().max().item(), slack.max().item())
        return
    assert ((got - torch.tanh(d)).abs() <= slack + 1e-6).all(), (what, (got - torch.tanh(d)).abs().max().item())
    assert (got.abs() <= 1.0).all(), what
    big = d.abs() > 10
    assert torch.equal(got[big], torch.sign(d[big])), what


@pytest.mark.parametrize("hw", [64, 42])
def test_value_head_on_synthetic_activations(hw, net_sw):
    """zc_net_value_head_w_async at 64 channels on activations up to 6e4 whose channels come in 32
    pairs with opposite Linear weights (tests/test_gpu_net_range.py's generator at this width):
    the 64-term sum cancels to O(1), so an fp16 or a badly ordered accumulation shows.  Pre-tanh
    within the slack of float64 (k = hw + 64 + 2); tanh within slack + 1e-6, never past +-1 and
    exactly +-1 past |d| = 10.  The same on nn_check.spread_head_inputs, which shows what cancels
    in a pair: tests/test_net_interval_cpu.py:test_wrong_value_heads_fall_outside_the_slack has
    the wrong heads each set rejects."""
    from zeroclone_amd import _native
    L = _native.lib()
    g = torch.Generator().manual_seed(hw)
    for n in (1, 5):
        sets = {"cancelling": nc.cancelling_head_inputs(g, n, hw, C),
                "spread": nc.spread_head_inputs(1000 * C + 10 * hw + n, n, hw, C)}
        for name, (act, fcw) in sets.items():
            assert act.shape == (n, hw, C) and act.max().item() > 5.0e4 and torch.isfinite(act).all()
            ag, wg = act.cuda(), fcw.cuda()
            for fcb in nc.HEAD_FCBS:
                d, slack = nc.value_head_reference(act, fcw, fcb)
                assert slack.max().item() < 0.5 and (d - float(np.float32(fcb))).abs().max().item() < 2.0
                for raw in (1, 0):
                    net_sw("head_raw", raw)
                    vals = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
                    _native.check(L.zc_net_value_head_w_async(C, n, hw, ag.data_ptr(), wg.data_ptr(), fcb, vals.data_ptr(),
                                                              None))
                    torch.cuda.synchronize()
                    check_values(vals, act, fcw, fcb, raw, (hw, n, name, fcb, raw))
                if abs(fcb) > 10:
                    assert (d.abs() > 10).all()


@pytest.mark.parametrize("board", BOARDS, ids=BOARD_IDS)
def test_value_head_within_the_slack(board, net_sw):
    """The value head inside the tower launch and stand-alone, on activations in the thousands:
    the pre-tanh sum within the slack of float64 on the activation the launch wrote."""
    from zeroclone_amd import _native
    from zeroclone_amd.nets import MfmaValueNetwork
    c, h, w = board
    mnet = MfmaValueNetwork(wide_value_net(c, h, w))
    fcw = mnet.fcw.cpu()
    assert fcw.shape == (C,)
    for n in (1, 5, 37):
        x = planes(131, c, h, w, seed=9)[:n].cuda()
        for raw in (1, 0):
            net_sw("head_raw", raw)
            a, vals = mnet.tower(x, head=True)
            act, fused = a.cpu().clone(), vals.clone()
            check_values(fused, act, fcw, mnet.fcb, raw, (board, n, raw, "fused"))
            alone = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
            _native.check(_native.lib().zc_net_value_head_w_async(C, n, h * w, a.data_ptr(), mnet.fcw.data_ptr(),
                                                                  mnet.fcb, alone.data_ptr(), None))
            torch.cuda.synchronize()
            assert same_bits(alone, fused)


@functools.lru_cache(maxsize=None)
def wide_policy_net(c, h, w, head):
    """tests/test_gpu_net_range.py:wide_policy_net's recipe at channels=64."""
    from zeroclone_amd.nets import FoldedValueNetwork, PolicyValueNetwork, _fold
    torch.manual_seed(50 + c)
    net = PolicyValueNetwork(C, blocks=2, in_planes=c, board=(h, w), n_logits=4096 if (h, w) == (8, 8) else 7,
                             head=head)
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


def policy_operands(net):
    from zeroclone_amd.nets import _fold
    f = _fold(net.policy[0], net.policy[1])
    return f.weight.detach().float().reshape(f.out_channels, -1).half(), f.bias.detach().float()


POLICY_CASES = [(17, 8, 8, "linear", 37), (2, 6, 7, "linear", 53), (17, 8, 8, "conv", 37)]
POLICY_IDS = ["8x8-linear", "6x7-linear", "8x8-conv"]


@pytest.mark.parametrize("case", POLICY_CASES, ids=POLICY_IDS)
def test_policy_conv_within_the_interval(case):
    """The 1x1 policy conv of the fused launch (64 -> 32 with ReLU; 64 -> 64 logits without) on the
    wide-range tower, against float64 of the activation tower(head=True) returns: k = 65.  One
    channel's bias sends it to -inf (0 under ReLU).  Values: the value-only launch's."""
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    c, h, w, head, n = case
    net = wide_policy_net(c, h, w, head)
    mnet = MfmaPolicyValueNetwork(net)
    assert mnet.fused and mnet.tower.channels == C
    x = planes(53, c, h, w, seed=10)[:n].cuda()
    v, logits = mnet(x)
    v, logits = v.clone(), logits.clone()
    pout = mnet._pout[(n, h * w)].cpu().clone()
    a, _ = mnet.tower.tower(x, head=True)
    act = a.cpu().clone()
    assert same_bits(mnet.tower(x).clone(), v)
    pw, pb = policy_operands(net)
    assert pw.shape == (32 if head == "linear" else 64, C)
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


def integer_pv_net(c, h, w, nl, seed, head):
    """tests/test_gpu_net.py:_integer_pv_net at 64 channels (density 0.004 for the 64 -> 64 convs)."""
    from zeroclone_amd.nets import PolicyValueNetwork
    g = torch.Generator().manual_seed(seed)
    net = PolicyValueNetwork(C, blocks=2, in_planes=c, board=(h, w), n_logits=nl, head=head).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            dens = 0.004 if m.in_channels == C and m.kernel_size == (3, 3) else 0.02
            keep = torch.rand(m.weight.shape, generator=g) < dens
            m.weight.data = torch.randint(-2, 3, m.weight.shape, generator=g).float() * keep
        elif isinstance(m, torch.nn.BatchNorm2d):
            m.eps = 0.0
            m.running_mean.zero_()
            m.running_var.fill_(1.0)
            m.weight.data.fill_(1.0)
            m.bias.data = torch.randint(-1, 3, m.bias.shape, generator=g).float()
        elif isinstance(m, torch.nn.Linear) and m.out_features == nl:
            keep = torch.rand(m.weight.shape, generator=g) < 0.004
            m.weight.data = torch.randint(-1, 2, m.weight.shape, generator=g).float() * keep
            m.bias.data = torch.randint(-4, 5, m.bias.shape, generator=g).float()
    return net


@pytest.mark.parametrize("case", [(37, 17, 8, 8, 4096, "linear"), (53, 2, 6, 7, 7, "linear"), (37, 17, 8, 8, 4096, "conv")],
                         ids=POLICY_IDS)
def test_policy_heads_exact_on_integers(case):
    """Both fused policy heads on an integer PolicyValueNetwork(64): the 1x1 conv's output (ReLU'd
    64 -> 32; the 64 -> 64 logits in from*64 + to order) and the linear head's logits equal
    float64 exactly, ragged last tiles included."""
    from zeroclone_amd.nets import FoldedValueNetwork, MfmaPolicyValueNetwork
    n, c, h, w, nl, head = case
    net = integer_pv_net(c, h, w, nl, seed=n + len(head), head=head)
    mnet = MfmaPolicyValueNetwork(net)
    assert mnet.fused
    x = planes(n, c, h, w, seed=3)
    _, logits = mnet(x.cuda())
    logits = logits.double().cpu()
    pout = mnet._pout[(n, h * w)].double().cpu()
    fv = FoldedValueNetwork(net.value_network()).double()
    conv, bn = net.policy[0], net.policy[1]
    with torch.no_grad():   # identity BN (eps 0): the folded form is the module's own algebra
        t = fv.res(torch.relu(fv.stem(x.double())))
        p = torch.nn.functional.conv2d(t, conv.weight.double()) + bn.bias.double().reshape(1, -1, 1, 1)
        if head == "conv":
            want = p.flatten(2).transpose(1, 2).reshape(n, 4096)       # [n, from, to]
            assert want.abs().max().item() < 2048 and (want < 0).any() and (want > 0).any()
            assert torch.equal(logits, want)
            return
        p = torch.relu(p)
        lin = net.policy[4]
        want_logits = p.flatten(1) @ lin.weight.double().t() + lin.bias.double()
    want_p = p.permute(0, 2, 3, 1).reshape(n, h * w, 32)
    assert want_p.abs().max().item() < 2048 and want_p.abs().sum().item() > 0
    assert want_logits.abs().max().item() < 2048 and (want_logits != lin.bias.double()).any()
    assert torch.equal(pout, want_p)
    assert torch.equal(logits, want_logits)


@pytest.mark.parametrize("head", ["linear", "conv"])
def test_policy_value_network_tracks_float64(head):
    """MfmaPolicyValueNetwork at 64 channels against the float64 network, as
    tests/test_gpu_net_range.py:test_policy_value_network_tracks_float64 at 128: a wide value
    head (values std >= 0.3), logits of std >= 0.3, Pearson >= 0.999 and max error within 4 x the
    error of the fp16-storage emulation against float64 on the same inputs (computed here, from
    the references alone; why 4: there)."""
    from zeroclone_amd.nets import FoldedValueNetwork, MfmaPolicyValueNetwork, PolicyValueNetwork
    torch.manual_seed(0)
    net = PolicyValueNetwork(C, blocks=2, head=head).eval()
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


# ---- 5. the counted forms ---------------------------------------------------------------------

@pytest.mark.parametrize("count", [0, 1, 7, 11, 40, -1, -2 ** 31])
@pytest.mark.parametrize("board", BOARDS, ids=BOARD_IDS)
def test_counted_forms(board, count):
    """zc_net_tower_counted_w_async and zc_net_tower_policy_counted_w_async at 64 channels, capacity
    11: the rows below min(count, 11) have the bits of the plain call; the rows past it of a
    sentinel-filled activation, values and pout are untouched.  A negative count is 0
    (include/zeroclone.h): every row keeps its sentinel."""
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    c, h, w = board
    n = 11
    k = max(min(count, n), 0)
    mnet = MfmaPolicyValueNetwork(wide_policy_net(c, h, w, "linear"))
    tower = mnet.tower
    xg = planes(n, c, h, w, seed=21).cuda()
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    a, vals = tower.tower(xg, head=True)
    want_a, want_v = a.clone(), vals.clone()
    pout = torch.empty((n, h * w, 32), dtype=torch.float16, device="cuda")
    want_pv = tower.tower_policy(xg, mnet.pw, mnet.pb, pout).clone()
    want_p = pout.clone()
    assert want_a.abs().sum().item() > 0 and want_p.abs().sum().item() > 0
    a.fill_(-3.0)
    vals.fill_(-3.0)
    a2, v2 = tower.tower(xg, head=True, count=cnt)
    torch.cuda.synchronize()
    assert same_bits(a2[:k], want_a[:k]) and same_bits(v2[:k], want_v[:k])
    assert (a2[k:] == -3.0).all() and (v2[k:] == -3.0).all()
    pout.fill_(-3.0)
    vals.fill_(-3.0)
    v3 = tower.tower_policy(xg, mnet.pw, mnet.pb, pout, count=cnt)
    torch.cuda.synchronize()
    assert same_bits(pout[:k], want_p[:k]) and same_bits(v3[:k], want_pv[:k])
    assert (pout[k:] == -3.0).all() and (v3[k:] == -3.0).all()


# ---- 6. non-finite values travel --------------------------------------------------------------

POISON = (2, 5, 8)   # the boards of eleven that hold 60000, +inf and NaN in one plane
NB = 11


def poisoned(c, h, w):
    x = planes(NB, c, h, w, seed=12)
    bad = x.clone()
    bad[2, 0] = 60000.0          # the whole plane: the stem overflows, the next layer forms inf - inf
    bad[5, 1, 3, 3] = INF
    bad[8, c - 1, 2, 4] = float("nan")
    return x, bad


def clean_rows(t):
    return t[[i for i in range(NB) if i not in POISON]]


@pytest.mark.parametrize("board", BOARDS, ids=BOARD_IDS)
def test_non_finite_inputs_reach_every_output(board):
    """60000, +inf and NaN in a plane of three boards of eleven: layer by layer each output is
    inside its interval (NaN stays NaN through every ReLU store); the fused tower stores the
    layered bits; the poisoned boards' values are NaN; the clean boards, tile neighbours included,
    hold the bits of a run without the poison."""
    from zeroclone_amd.nets import MfmaValueNetwork
    c, h, w = board
    mnet = MfmaValueNetwork(wide_value_net(c, h, w))
    x, bad = poisoned(c, h, w)

    def check(i, got, src, res, wt, bias):
        interval_check((board, "poisoned"))(i, got, src, res, wt, bias)
        if i >= 1:
            assert all(torch.isnan(got[b]).any() for b in POISON), (board, i)
    want = layered(mnet, nhwc32(bad).cuda(), check)
    clean = layered(mnet, nhwc32(x).cuda())
    assert not torch.isnan(clean).any()
    assert same_bits(clean_rows(want), clean_rows(clean))
    d, _ = nc.value_head_reference(want.reshape(NB, h * w, C), mnet.fcw.cpu(), mnet.fcb)
    assert torch.isnan(d[list(POISON)]).all() and torch.isfinite(clean_rows(d)).all()
    a, vals = mnet.tower(bad.cuda(), head=True)
    got_a, got_v = a.cpu().clone().reshape(want.shape), vals.cpu().clone()
    assert same_bits(got_a, want), board
    assert torch.equal(torch.isnan(got_v), torch.isnan(d)), (board, got_v.tolist())
    assert same_bits(mnet(bad.cuda()).cpu(), got_v) and same_bits(mnet(bad.cuda(), fused=False).cpu(), got_v)
    a, vals = mnet.tower(x.cuda(), head=True)
    assert same_bits(clean_rows(a.cpu().reshape(want.shape)), clean_rows(want))
    assert same_bits(clean_rows(vals.cpu()), clean_rows(got_v))


@pytest.mark.parametrize("case", [(17, 8, 8, "linear"), (2, 6, 7, "linear"), (17, 8, 8, "conv")], ids=POLICY_IDS)
def test_non_finite_inputs_reach_pout_and_logits(case):
    """The same three boards through zc_net_tower_policy_w_async at 64 channels (the conv head from
    NHWC [n, 64, 32] planes, tower_policy's three-dimensional input): pout is what float64 makes
    of the activation of tower(head=True), NaN on every pixel the activation holds a NaN; the
    poisoned boards' values and logits are NaN; the clean boards hold the bits of the clean
    launch."""
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    c, h, w, head = case
    net = wide_policy_net(c, h, w, head)
    mnet = MfmaPolicyValueNetwork(net)
    assert mnet.fused and mnet.tower.channels == C
    x, bad = poisoned(c, h, w)
    as_input = (lambda t: nhwc32(t).reshape(NB, h * w, 32).cuda()) if head == "conv" else (lambda t: t.cuda())
    assert as_input(bad).dim() == (3 if head == "conv" else 4)
    v, logits = mnet(as_input(bad))
    v, logits, pout = v.cpu().clone(), logits.cpu().clone(), mnet._pout[(NB, h * w)].cpu().clone()
    a, _ = mnet.tower.tower(bad.cuda(), head=True)
    act = a.cpu().clone()
    pw, pb = policy_operands(net)
    assert pw.shape == (32 if head == "linear" else 64, C)
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


@pytest.mark.parametrize("board", BOARDS, ids=BOARD_IDS)
def test_counted_launches_with_non_finite_rows(board):
    """zc_net_tower_counted_w_async and zc_net_tower_policy_counted_w_async at 64 channels, count =
    7 of 11: the poisoned boards below the count give the plain launch's outputs (NaN kept), and
    the rows past it — board 7, all NaN, shares its tile with the last counted board (8x8: boards
    6 and 7; 6x7: boards 6, 7 and 8), board 8 holds a NaN too — keep their sentinel."""
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
    assert torch.isfinite(want_v[[0, 1, 3, 4, 6]]).all() and not torch.isnan(want_a[6]).any()
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


@pytest.mark.parametrize("what", ["bias", "weight"])
@pytest.mark.parametrize("board", BOARDS, ids=BOARD_IDS)
def test_nan_parameter_reaches_every_output(board, what):
    """A NaN folded bias at one channel of block 1's first conv, or one NaN weight (the centre
    tap: no zero padding meets it), at 64 channels: that output channel is NaN on every pixel
    (the layered interval check demands it at the first ReLU already), and every board's
    activation, value, pout and logits hold NaN in the fused tower."""
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
    assert mnet.fused and mnet.tower.channels == C
    ch = 7 if what == "bias" else 9
    x = planes(5, c, h, w, seed=13)

    def check(i, got, src, res, wt, bias):
        interval_check((board, what))(i, got, src, res, wt, bias)
        if i == 1:
            assert torch.isnan(got[..., ch]).all() and not torch.isnan(got[..., :ch]).any()
    want = layered(mnet.tower, nhwc32(x).cuda(), check)
    assert torch.isnan(want).any(dim=(1, 2, 3)).all()
    a, vals = mnet.tower.tower(x.cuda(), head=True)
    assert same_bits(a.cpu().reshape(want.shape), want), (board, what)
    assert torch.isnan(vals).all()
    v, logits = mnet(x.cuda())
    assert torch.isnan(v).all() and torch.isnan(mnet._pout[(5, h * w)]).any(dim=(1, 2)).all()
    assert torch.isnan(logits).any(dim=1).all()


def test_pool_with_a_nan_bias_stops_every_game():
    """A 4-game Connect4 pool at 8 simulations whose 64-channel network — the MFMA tower, value
    head and policy head of csrc/net_conv64.hip — has a NaN BN bias in block 1: the search of every
    game ends with ZC_STATUS_INTERNAL (the backup's fence on the NaN value) and check() raises."""
    from zeroclone_amd import _native
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, MfmaValueNetwork, PolicyValueNetwork
    from zeroclone_amd.selfplay import C4SelfPlay
    torch.manual_seed(0)
    net = PolicyValueNetwork(C, blocks=2, in_planes=2, board=(6, 7), n_logits=7).eval()
    with torch.no_grad():
        net.res[0].seq[1].bias[7] = float("nan")
    pnet = MfmaPolicyValueNetwork(net)
    assert isinstance(pnet.tower, MfmaValueNetwork) and pnet.tower.channels == C and pnet.fused
    pool = C4SelfPlay(4, 8, batch_size=8, seed=3, puct_net=pnet)
    try:
        pool.step_search()
        torch.cuda.synchronize()
        assert pool.stats[:, 5].cpu().tolist() == [_native.ZC_STATUS_INTERNAL] * 4
        with pytest.raises(RuntimeError, match="ZC_STATUS_INTERNAL"):
            pool.check()
    finally:
        pool.close()


# ---- 7. refusals ------------------------------------------------------------------------------

def test_refusals():
    """The _w_ entry points refuse 5x5 boards, cin0 = 64, an even or zero nconv and 96 channels
    (ZC_EINVAL, the message naming the covered widths); the entry points without a width still
    refuse what tests/test_gpu_net.py:test_fused_tower_rejects_unsupported_shapes pins."""
    from zeroclone_amd import _native
    L = _native.lib()
    buf = torch.zeros(4096, dtype=torch.float16, device="cuda")
    bias = torch.zeros(128, dtype=torch.float32, device="cuda")
    vals = torch.zeros(4, dtype=torch.float64, device="cuda")
    cnt = torch.ones(1, dtype=torch.int32, device="cuda")
    p, b, v, k = buf.data_ptr(), bias.data_ptr(), vals.data_ptr(), cnt.data_ptr()

    def calls(ch, h, w, cin0, nconv):
        return {
            "tower": L.zc_net_tower_w_async(ch, 1, h, w, cin0, nconv, p, p, b, p, None, 0.0, None, None),
            "counted": L.zc_net_tower_counted_w_async(ch, 1, h, w, cin0, nconv, p, p, b, p, None, 0.0, None, k, None),
            "policy": L.zc_net_tower_policy_w_async(ch, 1, h, w, cin0, nconv, p, p, b, b, 0.0, v, p, b, 32, 1, p, None),
            "policy counted": L.zc_net_tower_policy_counted_w_async(ch, 1, h, w, cin0, nconv, p, p, b, b, 0.0, v, p, b,
                                                                    32, 1, p, k, None),
        }
    for (h, w, cin0, nconv) in [(5, 5, 32, 5), (8, 8, 64, 5), (8, 8, 32, 4), (8, 8, 32, 0)]:
        for name, rc in calls(C, h, w, cin0, nconv).items():
            assert rc == _native.ZC_EINVAL, (name, h, w, cin0, nconv)
    assert L.zc_net_conv3x3_packed_w_async(C, 1, 5, 5, 64, p, p, b, None, p, 1, None) == _native.ZC_EINVAL
    assert L.zc_net_conv3x3_packed_w_async(C, 1, 8, 8, 128, p, p, b, None, p, 1, None) == _native.ZC_EINVAL
    assert L.zc_net_conv3x3_pack_w_async(C, 128, p, p, None) == _native.ZC_EINVAL
    for ch in (96, 32, 256, 0):
        thunks = {
            "tower": lambda: L.zc_net_tower_w_async(ch, 1, 8, 8, 32, 5, p, p, b, p, None, 0.0, None, None),
            "counted": lambda: L.zc_net_tower_counted_w_async(ch, 1, 8, 8, 32, 5, p, p, b, p, None, 0.0, None, k, None),
            "policy": lambda: L.zc_net_tower_policy_w_async(ch, 1, 8, 8, 32, 5, p, p, b, b, 0.0, v, p, b, 32, 1, p, None),
            "policy counted": lambda: L.zc_net_tower_policy_counted_w_async(ch, 1, 8, 8, 32, 5, p, p, b, b, 0.0, v, p,
                                                                            b, 32, 1, p, k, None),
            "pack": lambda: L.zc_net_conv3x3_pack_w_async(ch, 32, p, p, None),
            "conv": lambda: L.zc_net_conv3x3_packed_w_async(ch, 1, 8, 8, 32, p, p, b, None, p, 1, None),
            "head": lambda: L.zc_net_value_head_w_async(ch, 1, 64, p, b, 0.0, v, None),
        }
        for name, call in thunks.items():
            assert call() == _native.ZC_EINVAL, (name, ch)
            msg = L.zc_last_error().decode(errors="replace")   # the message of that call
            assert "64 and 128" in msg, (name, ch, msg)
    # the width-less entry points and the family at 128: the refusals of before
    for (h, w, cin0, nconv) in [(5, 5, 32, 17), (8, 8, 128, 17), (8, 8, 32, 16), (8, 8, 32, 0)]:
        assert L.zc_net_tower_async(1, h, w, cin0, nconv, p, p, b, p, None, 0.0, None, None) != 0
        assert L.zc_net_tower_w_async(128, 1, h, w, cin0, nconv, p, p, b, p, None, 0.0, None, None) != 0
    assert L.zc_net_conv3x3_pack_async(64, p, p, None) != 0
    assert L.zc_net_conv3x3_packed_async(1, 8, 8, 64, p, p, b, None, p, 1, None) != 0
    torch.cuda.synchronize()
