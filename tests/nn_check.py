"""Helpers for the network numerics tests.

The only floating-point parity in the system is the value/policy network: the search is
exact given its values.  A check therefore has to be able to FAIL on a broken head, so every
comparison here asserts two things:

* max |got - want| <= atol, with atol a small fraction of the outputs' spread (`spread_ok`
  refuses a comparison whose reference outputs barely vary), and
* the Pearson correlation of got and want >= min_r (a near-constant head fails it even when
  the outputs sit inside a loose band).

`fp16_emulation` restates the GPU path's numerics on the CPU in float64: BN folded, weights
rounded to fp16, every layer's activation rounded to fp16 (the tower's epilogue stores fp16),
accumulation exact.  It predicts the fp16-vs-fp32 error a correct kernel must show.

The second half checks ONE layer against float64 with a bound that is derived, not measured
(`conv_interval` and its kin): the kernel's exact fp16 / fp32 inputs widened to float64, the
standard worst-case error of an fp32 sum of k terms in any order around the exact sum, and
the fp16 values that interval rounds to.  `wide_range_layer` draws inputs over the whole fp16
range (subnormal weights and activations, cancellation, sums past 65504).
"""
import numpy as np
import torch


def pearson(a, b) -> float:
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    a = a - a.mean()
    b = b - b.mean()
    return float((a @ b) / np.sqrt((a @ a) * (b @ b)))


def assert_tracks(got, want, atol, min_r=0.999, min_std=None, what=""):
    got = np.asarray(got, np.float64).reshape(-1)
    want = np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, what
    err = float(np.abs(got - want).max())
    assert err <= atol, f"{what}: max |err| {err:.3e} > atol {atol:.1e}"
    if min_std is not None:
        assert want.std() >= min_std, f"{what}: reference outputs span too little ({want.std():.3e})"
    if len(want) > 2:
        r = pearson(got, want)
        assert r >= min_r, f"{what}: Pearson {r:.6f} < {min_r}"
    return err


def fails_tracking(got, want, atol, min_r=0.999) -> bool:
    """True when `assert_tracks` would reject got (the mutation checks: a broken head)."""
    try:
        assert_tracks(got, want, atol, min_r)
    except AssertionError:
        return True
    return False


def fp16_emulation_features(folded, x):
    """Pooled tower features [n, 128] of a FoldedValueNetwork under the GPU path's fp16
    storage points (float64 accumulation)."""
    def h(t):
        return t.half().double()

    def conv(c, t):
        return torch.nn.functional.conv2d(t, h(c.weight.double()), c.bias.double(), padding=1)

    with torch.no_grad():
        a = h(torch.relu(conv(folded.stem, x.double())))
        for b in folded.res:
            t = h(torch.relu(conv(b.c1, a)))
            a = h(torch.relu(a + conv(b.c2, t)))
        return a.mean(dim=(2, 3))


def features64(folded, x):
    with torch.no_grad():
        f = folded.double()
        a = torch.relu(f.stem(x.double()))
        for b in f.res:
            a = torch.relu(a + b.c2(torch.relu(b.c1(a))))
        return a.mean(dim=(2, 3))


def wide_head(features, std=1.2):
    """(weight [128], bias) of a Linear head along the top principal direction of `features`
    [n, 128], scaled so the pre-tanh sum has mean 0 and std `std` over these inputs."""
    f = features.double()
    mu = f.mean(0)
    _, _, vt = torch.linalg.svd(f - mu, full_matrices=False)
    d = vt[0]
    scale = std / ((f - mu) @ d).std().item()
    return (d * scale).float(), float(-(mu @ (d * scale)).item())


# ---- one layer against float64, with a derived bound ---------------------------------------

U32 = 2.0 ** -24          # fp32 unit roundoff
F16_MIN_NORMAL = 2.0 ** -14


def gamma(k: int) -> float:
    """The worst-case relative error of an fp32 sum of k terms, in any order, against the sum
    of their absolute values (Higham, Accuracy and Stability, §4.2): k u / (1 - k u)."""
    return k * U32 / (1.0 - k * U32)


def rn16(t):
    """float64 -> the nearest fp16 (ties to even), as float64.  Through numpy: torch's
    `.half()` of a float64 tensor rounds to fp32 first, and the second rounding can land one
    fp16 ulp off when the first lands on a tie (1 + 2^-11 + 2^-30 -> 1.0)."""
    with np.errstate(over="ignore"):
        return torch.from_numpy(t.double().numpy().astype(np.float16).astype(np.float64))


def _interval(s, A, k, relu):
    slack = gamma(k) * A
    lo, hi = s - slack, s + slack
    exact = torch.isinf(A) & ~torch.isnan(s)   # an infinite input: the sum is that infinity in any order
    lo, hi = torch.where(exact, s, lo), torch.where(exact, s, hi)
    if relu:
        lo, hi = torch.relu(lo), torch.relu(hi)   # torch.relu keeps a NaN
    return rn16(lo), rn16(hi), s


def conv_interval(x, w, bias, res=None, relu=True):
    """out = rn16(relu?(conv3x3(x, w) + bias + res)) for the kernel's exact inputs: x NHWC
    fp16 [n, h, w, cin], w fp16 [cout, cin, 3, 3], bias fp32 [cout], res NHWC fp16 or None.
    Returns (lo16, hi16, s), NHWC float64: the fp16 values the correctly rounded result may
    take when the sum is formed in fp32 in any order (k = 9 cin + 2 terms; the fp16 x fp16
    products are exact in fp32), and the exact sum."""
    assert x.dtype == torch.float16 and w.dtype == torch.float16 and bias.dtype == torch.float32
    xd, wd, bd = x.double().permute(0, 3, 1, 2), w.double(), bias.double()
    s = torch.nn.functional.conv2d(xd, wd, bd, padding=1)
    A = torch.nn.functional.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=1)
    if res is not None:
        assert res.dtype == torch.float16
        rd = res.double().permute(0, 3, 1, 2)
        s, A = s + rd, A + rd.abs()
    return tuple(t.permute(0, 2, 3, 1).contiguous() for t in _interval(s, A, 9 * x.shape[3] + 2, relu))


def pointwise_interval(a, w, bias, relu):
    """The policy 1x1 conv on a [..., 128] fp16 activation: w fp16 [P, 128], bias fp32 [P];
    k = 128 + 1 terms."""
    assert a.dtype == torch.float16 and w.dtype == torch.float16 and bias.dtype == torch.float32
    s = a.double() @ w.double().t() + bias.double()
    A = a.double().abs() @ w.double().abs().t() + bias.double().abs()
    return _interval(s, A, a.shape[-1] + 1, relu)


def outside(got, lo16, hi16, s):
    """Elements of `got` (fp16) outside the accepted interval: where the exact sum is NaN the
    kernel must store NaN; elsewhere a number in [lo16, hi16] (infinite endpoints included: a
    sum far past 65520 demands the infinity)."""
    g = got.double().reshape(s.shape)
    nan = torch.isnan(s)
    assert not (torch.isnan(lo16) | torch.isnan(hi16))[~nan].any(), "the reference inputs must be finite"
    return torch.where(nan, ~torch.isnan(g), ~((g >= lo16) & (g <= hi16)))


def ambiguous_share(lo16, hi16) -> float:
    """The share of elements whose interval holds more than one fp16 value."""
    return float((lo16 != hi16).double().mean())


def value_head_reference(act, fcw, fcb):
    """The value head's pre-tanh sum for act fp16 [n, hw, C], fcw fp32 [C], fcb (an fp32
    value): (d64, slack), with k = hw + C + 2 fp32 operations on any element's path (the
    pixel sum, the product, the channel sum, the division by hw, + fcb)."""
    assert act.dtype == torch.float16 and fcw.dtype == torch.float32
    hw = act.shape[1]
    fb = float(np.float32(fcb))
    d = (act.double().sum(dim=1) @ fcw.double()) / hw + fb
    A = (act.double().abs().sum(dim=1) @ fcw.double().abs()) / hw + abs(fb)
    return d, gamma(hw + act.shape[2] + 2) * A


# ---- synthetic activations for the stand-alone value head, and the wrong heads they must catch ----

HEAD_FCBS = (0.3, 12.5, -12.5)


def cancelling_head_inputs(g, n, hw, channels=128):
    """(act fp16 [n, hw, C], fcw fp32 [C]) from the generator g: C / 2 channel pairs that hold the
    same activation (per-pair scales 1 .. 6e4, the first two 6e4 and 3e4; 30 % zeros) under
    opposite Linear weights (the second off by a relative 2^-9 randn), so the C-term sum cancels
    to O(1) and an fp16 or a badly ordered accumulation shows."""
    pairs = channels // 2
    scale = 6.0e4 ** torch.rand(pairs, generator=g, dtype=torch.float64)
    scale[:2] = torch.tensor([6.0e4, 3.0e4], dtype=torch.float64)
    half = torch.rand(n, hw, pairs, generator=g, dtype=torch.float64) * scale * (torch.rand(n, hw, pairs, generator=g) >= 0.3)
    act = torch.stack([half, half], dim=3).reshape(n, hw, channels).half()
    wpair = torch.randn(pairs, generator=g) * 1e-3
    fcw = torch.stack([wpair, -wpair * (1 + 2.0 ** -9 * torch.randn(pairs, generator=g))], dim=1).reshape(channels).float()
    return act, fcw


def spread_head_inputs(seed, n, hw, channels=128):
    """The second, non-cancelling set: every channel its own activation (the pair's scale, 30 %
    zeros) and its own weight, 0.5 randn / sqrt(C) over the channel's expected pixel mean (0.35
    scale), so every channel adds O(1 / sqrt(C)) to a sum of std ~0.5.  What the cancelling set
    cannot see shows here: a term lost from both channels of a pair alike, or the two weights of a
    pair exchanged (its two channels hold the same activation there)."""
    g = torch.Generator().manual_seed(seed)
    scale = (6.0e4 ** torch.rand(channels // 2, generator=g, dtype=torch.float64)).repeat_interleave(2)
    scale[:4] = torch.tensor([6.0e4, 6.0e4, 3.0e4, 3.0e4], dtype=torch.float64)
    act = torch.rand(n, hw, channels, generator=g, dtype=torch.float64) * scale * (torch.rand(n, hw, channels, generator=g) >= 0.3)
    fcw = (0.5 / channels ** 0.5) * torch.randn(channels, generator=g, dtype=torch.float64) / (0.35 * scale)
    return act.half(), fcw.float()


HEAD_MUTANTS = ("fp16_pixel_sums", "fp16_weights", "divide_by_64", "pair_weights_swapped", "one_lane_left_out")


def wrong_head(act, fcw, fcb, mutant):
    """The pre-tanh sum of a subtly wrong value head, in float64 from the head's inputs alone:
    "fp16_pixel_sums" (each channel's pixel sum accumulated in fp16), "fp16_weights" (fcw rounded
    to fp16), "divide_by_64" (the mean over 64 pixels whatever hw is: wrong on 6x7 only),
    "pair_weights_swapped" (channels 2 i and 2 i + 1 take each other's weight), "one_lane_left_out"
    (channels 8 .. 15 lose one lane's pixels: p = 7 mod 8 of the 64-channel head, where lane l
    sums channels 8 (l & 7) .. + 7 over pixels l / 8, + 8, ...; p = 3 mod 4 of the 128-channel
    head, where lane l sums channels 8 (l & 15) .. + 7 over pixels l / 16, + 4, ...)."""
    assert mutant in HEAD_MUTANTS
    n, hw, C = act.shape
    a, w, div = act.double(), fcw.double(), float(hw)
    fb = float(np.float32(fcb))
    if mutant == "fp16_pixel_sums":
        s = torch.zeros(n, C, dtype=torch.float16)
        for p in range(hw):
            s = s + act[:, p]
        return (s.double() @ w) / div + fb
    if mutant == "fp16_weights":
        w = fcw.half().double()
    elif mutant == "divide_by_64":
        div = 64.0
    elif mutant == "pair_weights_swapped":
        w = w.reshape(-1, 2).flip(1).reshape(-1)
    elif mutant == "one_lane_left_out":
        a = a.clone()
        step, first = (8, 7) if C == 64 else (4, 3)
        a[:, first::step, 8:16] = 0.0
    return (a.sum(dim=1) @ w) / div + fb


def head_rejects(d_wrong, d, slack):
    """Boards on which a wrong head's sum is NaN or outside the slack of the reference."""
    return torch.isnan(d_wrong) | ~((d_wrong - d).abs() <= slack)


def wide_range_layer(h, w, cin, seed, n=13, cout=128, overflow=False):
    """One layer's inputs over the fp16 range (13 boards): per-input-channel activation scales
    2^[-16, 10] x randn with 30 % zeros; weight scales 2^[-18, 1] per (cout, cin), reaching
    fp16 subnormals; bias 4 randn (fp32); residual scales 2^[-10, 11] per channel.
    overflow: the bias of five channels (~1 % of the sums each way) is moved so that the sums
    pass +-65520 (two channels each way) or straddle 65520 (one channel).
    Returns x [n, h, w, cin] fp16, wt [cout, cin, 3, 3] fp16, bias [cout] fp32, res fp16."""
    g = torch.Generator().manual_seed(seed)
    sx = 2.0 ** torch.randint(-16, 11, (cin,), generator=g).double()
    x = torch.randn(n, h, w, cin, generator=g, dtype=torch.float64) * sx
    x = (x * (torch.rand(n, h, w, cin, generator=g) >= 0.3)).half()
    sw = 2.0 ** torch.randint(-18, 2, (cout, cin), generator=g).double()
    wt = (torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * sw[:, :, None, None]).half()
    bias = (4.0 * torch.randn(cout, generator=g)).float()
    sr = 2.0 ** torch.randint(-10, 12, (cout,), generator=g).double()
    res = (torch.randn(n, h, w, cout, generator=g, dtype=torch.float64) * sr).half()
    if overflow:
        ch = torch.randperm(cout, generator=g)[:5]
        bias[ch[0]], bias[ch[1]] = 1.0e5, 2.0e5
        bias[ch[2]], bias[ch[3]] = -1.0e5, -2.0e5
        bias[ch[4]] = 65520.0
    return x, wt, bias, res


def has_subnormals(t) -> bool:
    a = t.double().abs()
    return bool(((a > 0) & (a < F16_MIN_NORMAL)).any())


# ---- the four mutants every interval check must catch (a CPU fp32 stand-in for a kernel) ----

def fp32_layer(x, wt, bias, res=None, relu=True, mutant=None):
    """A correct kernel's stand-in: torch fp32 conv + bias + res, ReLU, one rounding to fp16
    (NHWC).  mutant: "round_before_res" (the conv rounded to fp16 before the residual add),
    "drop_tap" (one tap's products missing at one pixel of every board), "bias_fp16" (the bias
    rounded to fp16 and added in fp16, to the conv rounded to fp16), "relu_before_res" (ReLU
    applied before the residual add)."""
    xf = x.float().permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(xf, wt.float(), None if mutant == "bias_fp16" else bias, padding=1)
    if mutant == "bias_fp16":
        y = (y.half() + bias.half().reshape(1, -1, 1, 1)).float()
    if mutant == "drop_tap":   # tap (0, 2) at pixel (2, 3): input pixel (1, 4)
        y[:, :, 2, 3] -= torch.einsum("nc,oc->no", xf[:, :, 1, 4], wt.float()[:, :, 0, 2])
    if mutant == "round_before_res":
        y = y.half().float()
    if mutant == "relu_before_res" and relu:
        y = torch.relu(y)
    if res is not None:
        y = y + res.float().permute(0, 3, 1, 2)
    if relu and mutant != "relu_before_res":
        y = torch.relu(y)
    return y.half().permute(0, 2, 3, 1).contiguous()


# ---- the wide-range network: BN statistics as a trained network has them --------------------

def widen_bn(net, seed):
    """BN running_var log-uniform in [1e-4, 10], weight in [0.25, 4], bias and running_mean in
    +-1, on every BatchNorm2d of `net` (in place)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.running_var.copy_(10.0 ** (torch.rand(c, generator=g) * 5.0 - 4.0))
                m.weight.copy_(0.25 + 3.75 * torch.rand(c, generator=g))
                m.bias.copy_(2.0 * torch.rand(c, generator=g) - 1.0)
                m.running_mean.copy_(2.0 * torch.rand(c, generator=g) - 1.0)
    return net.eval()


def scale_tower(net, x, target=2.0e4, tries=40):
    """Multiply every tower BN's weight by one factor (bisection on its logarithm) until the
    fp16-storage emulation's last activation on x peaks near `target`; returns that peak.
    Uses the float64 emulation alone."""
    from zeroclone_amd.nets import FoldedValueNetwork
    bns = [m for part in (net.stem, net.res) for m in part.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    base = [m.weight.detach().clone() for m in bns]

    def peak(logf):
        with torch.no_grad():
            for m, b in zip(bns, base):
                m.weight.copy_(b * float(np.exp(logf)))
        a = fp16_emulation_activation(FoldedValueNetwork(_as_value_network(net)), x)
        p = a.max().item()
        return p if np.isfinite(p) else float("inf")

    lo, hi = -12.0, 6.0
    for _ in range(tries):
        mid = 0.5 * (lo + hi)
        p = peak(mid)
        if 0.5 * target <= p <= 1.5 * target:
            return p
        lo, hi = (mid, hi) if p < target else (lo, mid)
    raise AssertionError("no BN scale puts the last activation's peak near the target")


def _as_value_network(net):
    return net.value_network() if hasattr(net, "value_network") else net


def fp16_emulation_activation(folded, x):
    """The tower's last activation [n, 128, h, w] under the fp16 storage points (float64)."""
    def h(t):
        return rn16(t)

    def conv(c, t):
        return torch.nn.functional.conv2d(t, h(c.weight.double()), c.bias.float().double(), padding=1)

    with torch.no_grad():
        a = h(torch.relu(conv(folded.stem, x.double())))
        for b in folded.res:
            t = h(torch.relu(conv(b.c1, a)))
            a = h(torch.relu(a + conv(b.c2, t)))
        return a


def fp16_emulation_heads(net, x):
    """(values [n], logits [n, L]) of a PolicyValueNetwork under the GPU path's storage points,
    float64 arithmetic between them: fp16 tower activations and conv weights, the value head on
    the fp16 activation with fp32 parameters; the policy 1x1 conv (fp16 weights, fp32 bias)
    stored as fp16, and for the linear head an fp16 GEMM's operands and fp16 logits."""
    from zeroclone_amd.nets import FoldedValueNetwork, _fold
    with torch.no_grad():
        f = FoldedValueNetwork(net.value_network())
        a = fp16_emulation_activation(f, x)                       # [n, 128, h, w]
        n = a.shape[0]
        v = torch.tanh(a.mean(dim=(2, 3)) @ f.fc.weight.float().double().reshape(-1) + f.fc.bias.float().double())
        pc = _fold(net.policy[0], net.policy[1])
        p = torch.nn.functional.conv2d(a, rn16(pc.weight.double()), pc.bias.float().double())
        if net.head_kind == "conv":
            return v, rn16(p).flatten(2).transpose(1, 2).reshape(n, -1)
        lin = net.policy[4]
        p = rn16(torch.relu(p))
        return v, rn16(p.flatten(1) @ rn16(lin.weight.double()).t() + rn16(lin.bias.double()))


def network64(net, x):
    """(values, logits) of the PolicyValueNetwork in float64 (eval-mode BN, no fp16 anywhere)."""
    import copy
    with torch.no_grad():
        v, lg = copy.deepcopy(net).double().eval()(x.double())
        return v.reshape(-1), lg
