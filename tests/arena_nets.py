"""Helpers of the arena tests: exact, batch-independent callables and integer networks (the
builder of test_gpu_net.py's _integer_net / _integer_pv_net), so that a routed search can be
compared bit for bit with the single-network searches whatever batch each network saw."""
import torch

PRIME = 1_000_003


class Exact:
    """A value function (n_logits = 0) or a policy + value function over the planes alone, in
    integer arithmetic: value = (planes . w mod PRIME) mapped to [-1, 1] in fp64 (an int64 dot
    product with fixed integer weights), logits = small integers (a matrix product of small
    integers, exact in fp64).  A row's outputs depend on that row alone; `seed` picks the weights."""
    roots_only = True   # as valued.PolicyNet: the roots flush may pass one row a game

    def __init__(self, seed: int, n_logits: int = 0):
        self.seed, self.n_logits = seed, n_logits
        self._w = {}
        self.calls = []   # rows of every call

    def _weights(self, width: int, dev):
        if width not in self._w:
            g = torch.Generator().manual_seed(self.seed * 7919 + width)
            w = torch.randint(1, 1 << 20, (width,), generator=g)
            m = torch.randint(0, 5, (width, self.n_logits), generator=g).double() if self.n_logits else None
            self._w[width] = (w.to(dev), m.to(dev) if m is not None else None)
        return self._w[width]

    def __call__(self, leaves, planes, counts):
        x = planes.reshape(planes.shape[0], -1)
        self.calls.append(x.shape[0])
        w, m = self._weights(x.shape[1], x.device)
        h = (x.to(torch.int64) * w).sum(1) % PRIME
        v = h.to(torch.float64) / (PRIME - 1) * 2.0 - 1.0
        if not self.n_logits:
            return v
        lg = (torch.matmul(x.to(torch.float64), m).to(torch.int64) % 7 - 3).to(torch.float32)
        return v, lg


class ExactModel:
    """`Exact` as a network: model(planes) -> values, or (values, logits) with n_logits, the
    call valued.NetValue / valued.PolicyNet make."""

    def __init__(self, seed: int, n_logits: int = 0):
        self.fn = Exact(seed, n_logits)

    def __call__(self, planes):
        return self.fn(None, planes, None)


def _integers(net, g, nl):
    """test_gpu_net.py's integer weights: sparse small-integer convolutions, identity BN with
    integer biases, a sparse integer policy Linear; and a value head whose weights are small
    multiples of 2^-6, so that its sum is exact in any order and tanh does not saturate."""
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            # the tower's convs: 0.002 at 128 -> 128, 0.004 at 64 -> 64 (the width tests' density)
            dens = {128: 0.002, 64: 0.004}.get(m.in_channels, 0.02) if m.kernel_size == (3, 3) else 0.02
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
        elif isinstance(m, torch.nn.Linear) and m.out_features == nl:
            keep = torch.rand(m.weight.shape, generator=g) < 0.004
            m.weight.data = torch.randint(-1, 2, m.weight.shape, generator=g).float() * keep
            m.bias.data = torch.randint(-4, 5, m.bias.shape, generator=g).float()
    return net


def integer_net(in_planes: int, seed: int, channels: int = 128):
    """MfmaValueNetwork over an integer ValueNetwork(64 or 128 channels, 2 blocks): the MFMA tower."""
    from zeroclone_amd.nets import MfmaValueNetwork, ValueNetwork
    g = torch.Generator().manual_seed(seed)
    net = MfmaValueNetwork(_integers(ValueNetwork(channels, 2, in_planes=in_planes).eval(), g, 0))
    assert net.channels == channels
    return net


def integer_pv_net(in_planes: int, h: int, w: int, n_logits: int, seed: int, head: str = "linear",
                   channels: int = 128):
    """MfmaPolicyValueNetwork over an integer PolicyValueNetwork (64 or 128 channels, 2 blocks)."""
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, PolicyValueNetwork
    g = torch.Generator().manual_seed(seed)
    net = PolicyValueNetwork(channels, in_planes=in_planes, board=(h, w), n_logits=n_logits, head=head).eval()
    net.res = net.res[:2]
    net = MfmaPolicyValueNetwork(_integers(net, g, n_logits))
    assert net.tower.channels == channels and net.fused
    return net
