"""The training step of the reference's loop (scripts/train.py:104-145, 191-244;
models/chess_value/network.py:75-101) on compact device data.

The reference expands every position to fp32 planes on the host and feeds a DataLoader; here
the training set stays as the self-play pools keep it — 24-byte Connect4 rows or 72-byte chess
rows, int32 labels, the sparse root visit counts (`TrajBatch.pi`) — and each minibatch is
decoded on the device (zc_train_batch_async): planes, labels, the positions' legal moves and
the visit counts as targets aligned with them.  The loss (zc_train_loss_async) is the
reference's MSE on the value plus, for a `PolicyValueNetwork`, the cross-entropy between the
visit distribution and the softmax over the position's LEGAL moves — the distribution the PUCT
searches evaluate (puct_common.h softmax_priors), never a [B, 4096] target.  The
convolutions' forward and backward in training mode stay on PyTorch-ROCm.

`device="cpu"` runs the same definitions in torch ops (no native library needed): the host-only
logic and the reference parity are testable without a GPU.  A chess set's legal moves need the
device move generator, so on the CPU a chess minibatch carries no legal lists (enough for a
`ValueNetwork`; a chess set with policy targets refuses).
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import TYPE_CHECKING

import numpy as np
import torch

from . import _native, nets
from .selfplay import TrajBatch, schedule_hyperparams, simulate_games

if TYPE_CHECKING:   # arena.py imports the pools, and a gate only holds one
    from .arena import C4Arena, ChessArena

GAMES = {"c4": (_native.ZC_TRAIN_C4, 3, 7, 7, (2, 6, 7)),                               # code, row words, stride,
         "chess": (_native.ZC_TRAIN_CHESS, 9, _native.CHESS_MAX_MOVES, 4096, (17, 8, 8))}  # logits width, planes


def _csr_select(pi_off: torch.Tensor, pi: torch.Tensor, index: torch.Tensor):
    """The CSR of rows `index` (any order, repeats allowed), rebuilt in that order."""
    cnt = pi_off[index + 1] - pi_off[index]
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=pi_off.device), torch.cumsum(cnt, 0)])
    total = int(off[-1])
    src = torch.repeat_interleave(pi_off[index] - off[:-1], cnt, output_size=total) \
        + torch.arange(total, device=pi_off.device)
    return off, pi[src]


@dataclass
class TrainingSet:
    """Positions to train on, compact (device tensors; CPU tensors work for the host-only logic).

    game    "c4" or "chess"
    rows    [n, 3] / [n, 9] int64     zc_c4_state / zc_chess_state records
    labels  [n] int32                 Engine.get_dataset labels
    pi_off  [n + 1] int64, pi [total] int32: the root visit counts, `TrajBatch`'s CSR and entry
            format (id | count << 16); both None: no policy targets."""
    game: str
    rows: torch.Tensor
    labels: torch.Tensor
    pi_off: torch.Tensor | None = None
    pi: torch.Tensor | None = None

    def __post_init__(self):
        if self.game not in GAMES:
            raise ValueError(f"game must be 'c4' or 'chess' (got {self.game!r})")
        words = GAMES[self.game][1]
        if self.rows.dim() != 2 or self.rows.shape[1] != words or self.rows.dtype != torch.int64:
            raise ValueError(f"{self.game} rows must be int64 [n, {words}]")
        if self.labels.shape != (self.rows.shape[0],) or self.labels.dtype != torch.int32:
            raise ValueError("labels must be int32 [n]")
        if (self.pi_off is None) != (self.pi is None):
            raise ValueError("pi_off and pi go together")
        if self.pi_off is not None and self.pi_off.shape != (self.rows.shape[0] + 1,):
            raise ValueError("pi_off must be [n + 1]")

    @classmethod
    def from_batch(cls, batch: TrajBatch, game: str) -> "TrainingSet":
        """A pool's finished games (`pool.take()` / `pool.last_batch`) as a training set."""
        return cls(game, batch.rows, batch.labels, batch.pi_off, batch.pi)

    @staticmethod
    def cat(sets: list["TrainingSet"]) -> "TrainingSet":
        """The sets' rows one after another; the policy is kept when every set has one."""
        if not sets:
            raise ValueError("nothing to concatenate")
        if len({s.game for s in sets}) != 1:
            raise ValueError("sets of different games")
        out = TrainingSet(sets[0].game, torch.cat([s.rows for s in sets]), torch.cat([s.labels for s in sets]))
        if all(s.pi_off is not None for s in sets):
            offs, base = [sets[0].pi_off[:1] * 0], 0
            for s in sets:
                offs.append(s.pi_off[1:] - s.pi_off[0] + base)
                base += int(s.pi_off[-1] - s.pi_off[0])
            out.pi_off = torch.cat(offs)
            out.pi = torch.cat([s.pi[int(s.pi_off[0]):int(s.pi_off[-1])] for s in sets])
        return out

    def __len__(self) -> int:
        return self.rows.shape[0]

    def select(self, index) -> "TrainingSet":
        """Rows `index` (tensor, array or list; any order, repeats allowed) with their CSR rebuilt."""
        index = torch.as_tensor(np.asarray(index) if not torch.is_tensor(index) else index,
                                dtype=torch.int64).to(self.rows.device)
        out = TrainingSet(self.game, self.rows[index], self.labels[index])
        if self.pi_off is not None:
            out.pi_off, out.pi = _csr_select(self.pi_off, self.pi, index)
        return out

    def to(self, device) -> "TrainingSet":
        mv = lambda t: None if t is None else t.to(device)  # noqa: E731
        return TrainingSet(self.game, mv(self.rows), mv(self.labels), mv(self.pi_off), mv(self.pi))


class ReplaySet:
    """scripts/train.py:_update_replay (:27-50) over compact sets, `selfplay.ReplayBuffer`'s
    semantics: a cycle trains on a uniform sample without replacement of `frac_old` of everything
    seen before — the sampled old rows first — then all new rows.  The sample is the reference's
    call, `np.random.choice(len(old), k, replace=False)` on numpy's GLOBAL generator, so after the
    same `np.random.seed` the same rows are drawn; `seed` gives a private generator instead."""

    def __init__(self, frac_old: float = 0.30, seed: int | None = None):
        self.frac_old = frac_old
        self.sets: list[TrainingSet] = []
        self.rng = np.random.default_rng(seed) if seed is not None else None

    def update(self, new: TrainingSet) -> TrainingSet:
        if not self.sets:
            self.sets.append(new)
            return new
        old = TrainingSet.cat(self.sets)
        self.sets = [old]   # concatenated once, not once per cycle and set
        k = int(self.frac_old * len(old))
        if k > 0:
            idx = (self.rng.choice(len(old), k, replace=False) if self.rng is not None
                   else np.random.choice(len(old), k, replace=False))
        else:
            idx = np.zeros(0, np.int64)
        self.sets.append(new)
        return TrainingSet.cat([old.select(idx), new])


def _raise_status(status: torch.Tensor):
    """Raises what a status word of zc_train_batch_async (or the OR of several) says: one device read."""
    st = int(status.item())
    if st & 1:
        raise RuntimeError("a policy entry names a move that is not legal in its position (the entry was dropped)")
    if st & 2:
        raise RuntimeError("a minibatch index lies outside the training set")
    if st & 4:
        raise RuntimeError(f"a chess position has more than {_native.CHESS_MAX_MOVES} legal moves")


@dataclass
class Minibatch:
    """One decoded minibatch (zc_train_batch_async): planes [B, C, H, W], z [B] float, legal
    [B, stride] int16 (the uint16 move ids) with n_legal [B] int32, target [B, stride] float
    aligned with legal; status: the device's status word (int32 [1])."""
    planes: torch.Tensor
    z: torch.Tensor
    legal: torch.Tensor
    n_legal: torch.Tensor
    target: torch.Tensor
    status: torch.Tensor
    width: int = 7

    def check(self):
        """Raises what the batch kernel flagged (one device read)."""
        _raise_status(self.status)


def _c4_planes_torch(rows: torch.Tensor, mirror: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor]:
    """selfplay.planes in torch ops, and the occupancy of the top cell of each column [n, 7]."""
    r = torch.arange(6, device=rows.device).view(1, 6, 1)
    c = torch.arange(7, device=rows.device).view(1, 1, 7).expand(rows.shape[0], 1, 7)
    if mirror is not None:
        c = torch.where(mirror.view(-1, 1, 1), 6 - c, c)
    bit = 7 * c + (5 - r)
    x = (rows[:, 0].view(-1, 1, 1) >> bit) & 1
    o = (rows[:, 1].view(-1, 1, 1) >> bit) & 1
    turn = (rows[:, 2] & 1).view(-1, 1, 1)
    planes = torch.stack([torch.where(turn == 0, x, o), torch.where(turn == 0, o, x)], dim=1)
    return planes, (x | o)[:, 0, :]


def _chess_planes_torch(rows: torch.Tensor) -> torch.Tensor:
    """state_to_tensor (chess_backend.cpp:461-521) of zc_chess_state rows in torch ops."""
    raw = rows.contiguous().view(torch.uint8).view(rows.shape[0], 72)
    board = raw[:, :64].view(-1, 1, 8, 8)
    pieces = torch.tensor(list(b"PNBRQKpnbrqk"), dtype=torch.uint8).view(1, 12, 1, 1)
    out = torch.zeros((rows.shape[0], 17, 8, 8), dtype=torch.float32)
    out[:, :12] = (board == pieces).float()
    out[:, 12] = (raw[:, 64] == 0).float().view(-1, 1, 1)
    for k in range(4):
        out[:, 13 + k] = ((raw[:, 66] >> k) & 1).float().view(-1, 1, 1)
    return out


def _minibatch_cpu(ts: TrainingSet, index, mirror, planes_dtype) -> Minibatch:
    """The batch's definition in torch ops (tests/learner_ref.py is its numpy spec)."""
    _, _, stride, width, _ = GAMES[ts.game]
    B = index.shape[0]
    rows, z = ts.rows[index], ts.labels[index].float()
    status = torch.zeros(1, dtype=torch.int32)
    legal = torch.zeros((B, stride), dtype=torch.int16)
    target = torch.zeros((B, stride), dtype=torch.float32)
    if ts.game == "chess":
        if ts.pi is not None:
            raise ValueError("a chess set's policy targets need the device move generator: decode it on the GPU")
        return Minibatch(_chess_planes_torch(rows).to(planes_dtype), z, legal, torch.zeros(B, dtype=torch.int32),
                         target, status, width)
    planes, top = _c4_planes_torch(rows, mirror)
    playable = top == 0                                          # [B, 7] in output columns
    n_legal = playable.sum(1).to(torch.int32)
    cols = torch.arange(7).expand(B, 7)
    order = torch.argsort(torch.where(playable, cols, cols + 7), dim=1)   # the playable columns first, ascending
    live = cols < n_legal.view(-1, 1)
    dense = torch.zeros((B, 7), dtype=torch.float32)
    if ts.pi is not None:
        off, ent = _csr_select(ts.pi_off, ts.pi, index)
        owner = torch.repeat_interleave(torch.arange(B), off[1:] - off[:-1])
        ids, cnt = (ent & 0xFFFF).to(torch.int64), ((ent >> 16) & 0xFFFF).to(torch.float32)
        total = torch.zeros(B, dtype=torch.float32).index_add_(0, owner, cnt)
        if mirror is not None:
            ids = torch.where(mirror[owner] & (ids < 7), 6 - ids, ids)
        ok = (ids < 7) & playable[owner, ids.clamp(max=6)]
        if not bool(ok.all()):   # an entry for a full column (or no column): dropped, still in the sum
            status |= 1
        dense[owner[ok], ids[ok]] = cnt[ok] / total[owner[ok]]   # one single-precision division
    legal = torch.where(live, order, torch.zeros_like(order)).to(torch.int16)
    target = torch.where(live, dense.gather(1, order), torch.zeros_like(dense))
    return Minibatch(planes.to(planes_dtype), z, legal, n_legal, target, status, width)


def minibatch(ts: TrainingSet, index: torch.Tensor, mirror: torch.Tensor | None = None,
              planes_dtype: torch.dtype = torch.float32) -> Minibatch:
    """Batch row b = set row index[b], decoded (zc_train_batch_async; a CPU set: the same in
    torch ops).  index: int64, any order, repeats allowed; mirror: bool / uint8 [B], Connect4
    only — a mirrored row is reflected left to right in the planes, the legal list and the
    targets.  Nothing is synchronised: `Minibatch.check()` reads the status word."""
    if planes_dtype not in (torch.float32, torch.float16):
        raise ValueError("planes_dtype must be torch.float32 or torch.float16")
    if mirror is not None and ts.game != "c4":
        raise ValueError("mirror is Connect4's symmetry: a chess position has no mirror image")
    dev = ts.rows.device
    index = index.to(device=dev, dtype=torch.int64).contiguous()
    B = index.shape[0]
    if mirror is not None:
        if mirror.shape != (B,):
            raise ValueError("mirror must be [B]")
        mirror = (mirror.to(dev) != 0)
    if dev.type != "cuda":
        if B and (int(index.min()) < 0 or int(index.max()) >= len(ts)):
            raise IndexError("a minibatch index lies outside the training set")
        return _minibatch_cpu(ts, index, mirror, planes_dtype)
    code, words, stride, width, shape = GAMES[ts.game]
    c = _native.TrainSet()
    c.game, c.row_bytes, c.n_rows = code, 8 * words, len(ts)
    rows, labels = ts.rows.contiguous(), ts.labels.contiguous()
    c.d_rows, c.d_labels = rows.data_ptr(), labels.data_ptr()
    if ts.pi is not None:
        pi_off = ts.pi_off.contiguous()
        pi = ts.pi.contiguous() if ts.pi.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        c.d_pi_off, c.d_pi = pi_off.data_ptr(), pi.data_ptr()
    mb = Minibatch(torch.empty((B, *shape), dtype=planes_dtype, device=dev),
                   torch.empty(B, dtype=torch.float32, device=dev),
                   torch.empty((B, stride), dtype=torch.int16, device=dev),
                   torch.empty(B, dtype=torch.int32, device=dev),
                   torch.empty((B, stride), dtype=torch.float32, device=dev),
                   torch.zeros(1, dtype=torch.int32, device=dev), width)
    flags = mirror.to(torch.uint8).contiguous() if mirror is not None else None
    _native.train_batch(c, B, index.data_ptr(), flags.data_ptr() if flags is not None else 0,
                        planes_dtype == torch.float16, mb.planes.data_ptr(), mb.z.data_ptr(), mb.legal.data_ptr(),
                        mb.n_legal.data_ptr(), mb.target.data_ptr(), mb.status.data_ptr(),
                        torch.cuda.current_stream(dev).cuda_stream)
    return mb


def logit_index(legal: torch.Tensor, width: int) -> torch.Tensor:
    """The logit index of each move id of a legal list (int64): the column (width 7), or
    from * 64 + to of the packed chess move (width 4096)."""
    ids = legal.to(torch.int64) & 0xFFFF
    return ids if width == 7 else (ids & 63) * 64 + ((ids >> 6) & 63)


def loss_torch(v: torch.Tensor, logits: torch.Tensor | None, mb: Minibatch):
    """(Lv, Lp) by torch ops and autograd, the loss's definition (zc_train_loss_async) in the
    tensors' own precision: the masked log_softmax formulation.  The CPU path of
    `policy_value_loss`, and what the kernel is compared against.  The header's rules for rows
    `minibatch` never makes: n_legal outside [0, stride] is clamped, a width-7 id above 6 is in
    neither the softmax nor the target sum, and a policy row is one whose legal slots' targets
    sum to more than 0."""
    v = v.reshape(-1)
    Lv = torch.nn.functional.mse_loss(v, mb.z.to(v.dtype))
    if logits is None:
        return Lv, torch.zeros((), dtype=v.dtype, device=v.device)
    B, stride = mb.legal.shape
    at = logit_index(mb.legal, logits.shape[1])
    live = (torch.arange(stride, device=v.device).view(1, -1) < mb.n_legal.view(-1, 1)) & (at < logits.shape[1])
    x = logits.gather(1, at.clamp(max=logits.shape[1] - 1))
    # (a row without legal moves keeps its slots: a softmax over nothing is NaN, in backward too)
    lsm = torch.log_softmax(x.masked_fill(~(live | ~live.any(1, keepdim=True)), float("-inf")), dim=1)
    t = mb.target.to(x.dtype)
    rows = torch.where(live, t, torch.zeros_like(t)).sum(1) > 0
    P = int(rows.sum())
    if P == 0:
        return Lv, (logits * 0).sum()
    terms = torch.where(live & rows.view(-1, 1), -t * lsm, torch.zeros_like(lsm))
    return Lv, terms.sum() / P


class _FusedLoss(torch.autograd.Function):
    """zc_train_loss_async: both losses and both gradients in one call; backward scales the
    stored gradients by the incoming ones."""

    @staticmethod
    def forward(ctx, v, logits, mb):
        B = v.shape[0]
        dev = v.device
        vf = v.detach().reshape(-1).to(torch.float32).contiguous()
        lg = logits.detach().contiguous() if logits is not None else None
        if lg is not None and lg.dtype not in (torch.float32, torch.float16):
            raise ValueError("logits must be fp32 or fp16")
        need = _native.train_loss_scratch_bytes(B)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        gv = torch.empty(B, dtype=torch.float32, device=dev)
        gl = torch.empty_like(lg) if lg is not None else None
        _native.train_loss(B, lg.shape[1] if lg is not None else 0, mb.legal.shape[1],
                           lg.data_ptr() if lg is not None else 0, lg is not None and lg.dtype == torch.float16,
                           vf.data_ptr(), mb.z.data_ptr(), mb.legal.data_ptr(), mb.n_legal.data_ptr(),
                           mb.target.data_ptr(), scratch.data_ptr(), need, loss.data_ptr(), gv.data_ptr(),
                           gl.data_ptr() if gl is not None else 0, torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(gv, gl)
        ctx.v_shape, ctx.v_dtype = v.shape, v.dtype
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_lv, g_lp):
        gv, gl = ctx.saved_tensors
        grad_v = (gv * g_lv).to(ctx.v_dtype).reshape(ctx.v_shape)
        grad_l = None if gl is None else (gl * g_lp.to(gl.dtype))
        return grad_v, grad_l, None


def policy_value_loss(v: torch.Tensor, logits: torch.Tensor | None, mb: Minibatch):
    """(Lv, Lp): Lv = mean (v - z)^2 (nn.MSELoss, the reference's criterion); Lp = the mean over
    the policy rows (targets summing to more than 0) of the cross-entropy between the targets and
    the softmax of the row's logits over its LEGAL moves; 0 without such rows or with
    logits=None (a `ValueNetwork`).  v: the tanh head's output, [B] or [B, 1]; logits [B, 7] or
    [B, 4096], fp32 or fp16.  On the GPU one call of zc_train_loss_async computes both losses
    and both gradients; on the CPU the same definition in torch ops."""
    if v.numel() != mb.z.shape[0]:
        raise ValueError("v must hold one value per batch row")
    if logits is not None and (logits.dim() != 2 or logits.shape[0] != mb.z.shape[0] or logits.shape[1] != mb.width):
        raise ValueError(f"logits must be [B, {mb.width}]")
    if v.device.type != "cuda":
        return loss_torch(v, logits, mb)
    return _FusedLoss.apply(v, logits, mb)


@dataclass
class TrainResult:
    """epoch_losses: each epoch's loss averaged over the set (batches weighted by their size).

    reference_return: what the reference's `train` (network.py:75-101) actually returns.  Its
    `loss` accumulator is overwritten by every batch's loss tensor, so at the end it holds only
    the LAST batch's loss of the last epoch plus that epoch's average, and the function returns
    that sum (fp32) divided by `epochs` — not the mean of the epoch averages.  Reproduced here
    because scripts/train.py reports it; use epoch_losses for anything else."""
    epoch_losses: list[float] = field(default_factory=list)
    reference_return: float = 0.0
    value_losses: list[float] = field(default_factory=list)
    policy_losses: list[float] = field(default_factory=list)


def train(model, ts: TrainingSet, epochs: int = 10, lr: float = 1e-3, batch_size: int = 32, shuffle: bool = True,
          device=None, generator: torch.Generator | None = None, mirror: bool = False) -> TrainResult:
    """network.py:train (:75-101) behind scripts/train.py:train_and_save_latest's DataLoader
    (:104-145): Adam(model.parameters(), lr), model.train() each epoch, batches of `batch_size`
    with the last partial batch kept, the epoch's loss averaged with the batch sizes as weights.
    The loss is Lv for a `ValueNetwork` and Lv + Lp for a `PolicyValueNetwork`
    (`policy_value_loss`).

    shuffle draws torch.randperm(n, generator=generator) on the host once per epoch; the
    DataLoader's own seeding (a base seed drawn from the global generator, then its sampler's
    private one) is NOT reproduced, so a shuffled run matches the reference in distribution
    only.  mirror (Connect4): each sample of each batch is mirrored with probability 1/2, drawn
    from the same generator.  device: where the model and the set go (default: the set's)."""
    dev = torch.device(device) if device is not None else ts.rows.device
    ts = ts.to(dev)
    model.to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    n = len(ts)
    if n == 0:
        raise ValueError("an empty training set")
    if mirror and ts.game != "c4":
        raise ValueError("mirror is Connect4's symmetry")
    res = TrainResult()
    last = 0.0
    for _ in range(epochs):
        model.train()
        order = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)
        running = running_v = running_p = torch.zeros((), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)   # every batch's status word, OR-ed on the device
        for lo in range(0, n, batch_size):
            idx = order[lo:lo + batch_size]
            flip = (torch.rand(idx.shape[0], generator=generator) < 0.5) if mirror else None
            mb = minibatch(ts, idx, flip)
            status |= mb.status
            opt.zero_grad()
            out = model(mb.planes)
            v, logits = out if isinstance(out, tuple) else (out, None)
            Lv, Lp = policy_value_loss(v, logits, mb)
            loss = Lv if logits is None else Lv + Lp
            loss.backward()
            opt.step()
            last = loss.detach()
            running = running + last.double() * idx.shape[0]
            running_v = running_v + Lv.detach().double() * idx.shape[0]
            running_p = running_p + Lp.detach().double() * idx.shape[0]
        _raise_status(status)
        res.epoch_losses.append(float(running) / n)
        res.value_losses.append(float(running_v) / n)
        res.policy_losses.append(float(running_p) / n)
    if epochs:   # the reference's return value (TrainResult.reference_return)
        res.reference_return = float((last.float().cpu() + res.epoch_losses[-1]) / epochs)
    return res


class FoldedPolicyValueNetwork(torch.nn.Module):
    """Inference form of a `PolicyValueNetwork` of any width on PyTorch-ROCm (the MFMA towers
    cover 64 and 128 channels): eval-mode BatchNorm folded into the convolutions, channels-last;
    returns (values fp64 [n], logits [n, n_logits]) as a PUCT search's network does."""

    def __init__(self, net: nets.PolicyValueNetwork):
        super().__init__()
        import copy
        net = copy.deepcopy(net).eval()
        self.value = nets.FoldedValueNetwork(net.value_network())
        self.conv_head = net.head_kind == "conv"
        self.pconv = nets._fold(net.policy[0], net.policy[1])
        self.plin = None if self.conv_head else net.policy[4]

    @torch.no_grad()
    def forward(self, x):
        x = x.contiguous(memory_format=torch.channels_last)
        t = self.value.res(torch.relu(self.value.stem(x)))
        v = torch.tanh(self.value.fc(t.mean(dim=(2, 3)))).reshape(-1).to(torch.float64)
        p = self.pconv(t)
        if self.conv_head:
            return v, p.flatten(2).transpose(1, 2).reshape(x.shape[0], -1)
        return v, self.plin(torch.relu(p).flatten(1))


def inference_form(model, device, dtype=torch.float16):
    """A trained model as a pool's search evaluates it: `nets.for_inference` of a ValueNetwork;
    `nets.MfmaPolicyValueNetwork` of a PolicyValueNetwork the MFMA towers cover (64 or 128 channels,
    the fused policy heads), else `FoldedPolicyValueNetwork` in `dtype`."""
    dev = torch.device(device)
    if isinstance(model, nets.PolicyValueNetwork):
        conv = model.policy[0]
        fits = (nets.mfma_supported(model) and dev.type == "cuda" and dtype == torch.float16
                and (conv.out_channels == 64 if model.head_kind == "conv" else True))
        if fits:
            return nets.MfmaPolicyValueNetwork(model, dev)
        return FoldedPolicyValueNetwork(model).to(device=dev, dtype=dtype).to(memory_format=torch.channels_last).eval()
    if isinstance(model, nets.ValueNetwork):
        return nets.for_inference(model, dev, dtype)
    raise TypeError("set_network takes a ValueNetwork or a PolicyValueNetwork")


@dataclass
class Gate:
    """The gate of `full_training_run(gate=)`: after a cycle's training the trained network plays
    `games` games against the network it was trained from in `arena` (a `C4Arena` / `ChessArena`
    of the model's search, best with openings= so that the games differ) and replaces it in the
    self-play pool only at a score of at least `threshold` — scripts/evaluate.py:evaluate_pair's
    win rate with draws as one half.  The arena's sims and c are its own, not the schedule's.
    history: one (cycle, ArenaResult, promoted) per cycle."""
    arena: "C4Arena | ChessArena"
    games: int
    threshold: float = 0.55
    history: list = field(default_factory=list)


def full_training_run(pool, model, cycles: int, *, epochs: int = 4, batch_size: int = 256, games_cap: int = 2000,
                      sims_cap: int = 800, init_lr: float = 3e-4, lr_decay: float = 0.95, lr_floor: float = 1e-5,
                      replay: ReplaySet | None = None, game: str | None = None, train_fn=None,
                      gate: Gate | None = None) -> list[TrainResult]:
    """scripts/train.py:full_training_run (:191-244) on a device pool built with `model`'s
    inference form.  Per cycle: `schedule_hyperparams`; the pool's `sims` and `c` (and a PUCT
    search's c_puct) set from it — a schedule beyond the pool's `max_sims` refuses, the trees
    were sized at construction; `simulate_games`; the finished games as a `TrainingSet`;
    `ReplaySet.update`; `train` at the cycle's learning rate; `pool.set_network(model)`.
    With gate= the hand-back is conditional: the model's state_dict is copied before the cycle's
    `train`; afterwards a copy of the model holding that state (the incumbent) plays the trained
    model in `gate.arena` (`set_networks(model, incumbent)`, `play(gate.games)`); at a score of at
    least `gate.threshold` the pool gets the trained network, else the model takes the copied state
    back and the pool goes on playing the incumbent; `gate.history` gets the cycle's entry.
    Returns the cycles' `TrainResult`s.  The reference's log-file tee and checkpoint renaming are
    the caller's.  game: "c4" / "chess" (default: by the pool's row size); train_fn: `train`'s
    stand-in (tests)."""
    replay = replay if replay is not None else ReplaySet()
    train_fn = train_fn or train
    results = []
    for cycle in range(cycles):
        hp = schedule_hyperparams(cycle, games_cap=games_cap, sims_cap=sims_cap, init_lr=init_lr, lr_decay=lr_decay,
                                  lr_floor=lr_floor)
        limit = getattr(pool, "max_sims", None) or pool.eng.max_sims
        if hp["simulations"] > limit:
            raise ValueError(f"cycle {cycle} schedules {hp['simulations']} simulations, the pool was built for "
                             f"{limit} (max_sims): build it for the schedule's cap")
        pool.sims, pool.c = hp["simulations"], hp["c_puct"]
        if getattr(pool, "ps", None) is not None:
            pool.ps.c = hp["c_puct"]
        simulate_games(pool, hp["games"])
        batch = pool.last_batch
        new = TrainingSet.from_batch(batch, game or ("c4" if batch.rows.shape[1] == 3 else "chess"))
        if gate is not None:   # on the model's device: what the incumbent is made of
            snapshot = {k: v.detach().clone() for k, v in model.state_dict().items()}
        results.append(train_fn(model, replay.update(new), epochs=epochs, lr=hp["lr"], batch_size=batch_size))
        if gate is None:
            pool.set_network(model)
            continue
        incumbent = copy.deepcopy(model)
        incumbent.load_state_dict(snapshot)
        gate.arena.set_networks(model, incumbent)
        res = gate.arena.play(gate.games)
        promoted = res.score >= gate.threshold
        if promoted:
            pool.set_network(model)
        else:
            model.load_state_dict(snapshot)
        gate.history.append((cycle, res, promoted))
    return results
