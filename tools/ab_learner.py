#!/usr/bin/env python3
"""What the learner's fused minibatch + loss costs against the same work composed from what the
package had before it, with the arms alternating over several rounds on one device.

  (a) minibatch and loss: one minibatch decoded from the compact set, both losses forward and
      backward down to the gradients of v and of the logits (leaf tensors; no network)
        fused     learner.minibatch (zc_train_batch_async) + learner.policy_value_loss
                  (zc_train_loss_async)
        composed  index_select of the rows and labels; planes by zc_chess_planes_async (chess) or
                  torch ops (Connect4); TrajBatch.policy_targets(width) of the WHOLE set made once
                  outside the timed window, indexed inside it; a legal mask ([B, 4096] from
                  zc_chess_legal_moves_async and a scatter, or the full-column test); masked
                  F.log_softmax, mse_loss and autograd
      at chess B = 256 and 4096 and Connect4 B = 256 and 4096.  The composed arm gets the dense
      targets of the whole set for nothing (8192 x 4096 fp32 = 134 MB here; a real replay set
      would not fit), so its figure is a lower bound.
  (b) one full optimiser step (batch, forward, loss, backward, Adam) of the 128 x 8
      PolicyValueNetwork each way, B = 256, fp32 training-mode convolutions on PyTorch-ROCm.

The sets: 8192 positions with their root visit counts, taken from self-play pools stepped from
the opening (rollout search for Connect4, the crude-score search for chess; 64 simulations).
Times are device events around back-to-back iterations (10 x reps of (a), reps / 2 of (b)), in us
(a) or ms (b) per iteration.

    python tools/ab_learner.py [--rounds 5] [--reps 20]
"""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def build_set(game: str, rows_wanted: int = 8192):
    """(TrainingSet, engine): positions of a stepped pool with the visit counts of their searches."""
    import torch
    from zeroclone_amd import _native
    from zeroclone_amd.learner import TrainingSet
    from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay
    G, steps = (1024, 8) if game == "c4" else (512, 16)
    pool = C4SelfPlay(G, 64, seed=1) if game == "c4" else ChessSelfPlay(G, 64, seed=1)
    rows, offs, pis = [], [], []
    for _ in range(rows_wanted // G):
        roots = pool.roots.clone()
        if game == "chess":
            mv = torch.zeros((G, _native.CHESS_MAX_MOVES), dtype=torch.int16, device=pool.dev)
            cnt = torch.zeros(G, dtype=torch.int32, device=pool.dev)
            pool.eng.chess_legal_moves_async(G, roots.data_ptr(), mv.data_ptr(), cnt.data_ptr())
            ids = mv.to(torch.int32) & 0xFFFF
        else:
            ids = torch.arange(7, dtype=torch.int32, device=pool.dev).expand(G, 7)
        pool.step()
        na = pool.na.clone()
        keep = na > 0
        rows.append(roots.view(torch.int64).reshape(G, -1))
        offs.append(keep.sum(1))
        pis.append((ids | (na << 16))[keep])
    torch.cuda.synchronize()
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=pool.dev), torch.cumsum(torch.cat(offs), 0)])
    rows = torch.cat(rows)
    labels = (torch.arange(rows.shape[0], device=pool.dev) % 3 - 1).to(torch.int32)
    return TrainingSet(game, rows, labels, off, torch.cat(pis).to(torch.int32)), pool


class Composed:
    """The same batch and loss from the package's earlier entry points and torch ops."""

    def __init__(self, ts, pool):
        import torch
        from zeroclone_amd.selfplay import TrajBatch
        self.ts, self.eng, self.chess = ts, pool.eng, ts.game == "chess"
        self.width = 4096 if self.chess else 7
        self.dense = TrajBatch(ts.rows, ts.labels, None, None, ts.pi_off, ts.pi).policy_targets(self.width)
        torch.cuda.synchronize()

    def batch(self, index):
        import torch
        from zeroclone_amd import learner
        rows = self.ts.rows.index_select(0, index)
        z = self.ts.labels.index_select(0, index).float()
        B, dev = rows.shape[0], rows.device
        if self.chess:
            planes = torch.empty((B, 17, 8, 8), dtype=torch.float32, device=dev)
            mv = torch.zeros((B, 256), dtype=torch.int16, device=dev)
            cnt = torch.empty(B, dtype=torch.int32, device=dev)
            s = torch.cuda.current_stream().cuda_stream
            self.eng.chess_planes_async(B, rows.data_ptr(), planes.data_ptr(), False, s)
            self.eng.chess_legal_moves_async(B, rows.data_ptr(), mv.data_ptr(), cnt.data_ptr(), s)
            live = torch.arange(256, device=dev).view(1, -1) < cnt.view(-1, 1)
            mask = torch.zeros((B, 4096), dtype=torch.bool, device=dev)
            # (an idle slot's id 0 is a8 -> a8, no move: its False lands on a cell that stays False)
            mask.scatter_(1, learner.logit_index(mv, 4096), live)
        else:
            planes, top = learner._c4_planes_torch(rows, None)
            planes, mask = planes.float(), top == 0
        return planes, z, mask, self.dense.index_select(0, index)

    @staticmethod
    def loss(v, logits, z, mask, target):
        import torch
        import torch.nn.functional as F
        Lv = F.mse_loss(v.reshape(-1), z)
        lsm = F.log_softmax(logits.float().masked_fill(~mask, float("-inf")), dim=1)
        rows = target.sum(1) > 0
        terms = torch.where(mask & rows.view(-1, 1), -target * lsm, torch.zeros_like(lsm))
        return Lv, terms.sum() / rows.sum().clamp(min=1)


def timed(fn, reps: int) -> float:
    """ms per call of `reps` back-to-back calls (device events)."""
    import torch
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def alternate(arms: dict, rounds: int, reps: int) -> dict:
    for fn in arms.values():   # warm-up: kernels loaded, algorithms picked, the allocator filled
        timed(fn, 3)
    order, res = list(arms), {k: [] for k in arms}
    for rnd in range(rounds):
        for k in order[rnd % len(order):] + order[:rnd % len(order)]:
            res[k].append(timed(arms[k], reps))
    return res


def report(title: str, res: dict, unit: str, scale: float):
    med = {k: statistics.median(v) * scale for k, v in res.items()}
    for k, v in res.items():
        print(f"{title:28s} {k:9s} median {med[k]:10.1f} {unit}  min {min(v) * scale:10.1f}  max {max(v) * scale:10.1f}")
    print(f"{title:28s} fused / composed = {med['fused'] / med['composed']:.3f}", flush=True)


def part_a(game, ts, comp, B, args):
    import torch
    from zeroclone_amd import learner
    g = torch.Generator().manual_seed(B)
    index = torch.randint(0, len(ts), (B,), generator=g).to(ts.rows.device)
    width = comp.width
    v0 = torch.tanh(torch.randn(B, generator=g)).to(index.device)
    x0 = torch.randn((B, width), generator=g).to(index.device)

    def fused():
        v, x = v0.clone().requires_grad_(), x0.clone().requires_grad_()
        mb = learner.minibatch(ts, index)
        Lv, Lp = learner.policy_value_loss(v, x, mb)
        (Lv + Lp).backward()
        return Lv, Lp, v.grad, x.grad

    def composed():
        v, x = v0.clone().requires_grad_(), x0.clone().requires_grad_()
        _, z, mask, target = comp.batch(index)
        Lv, Lp = comp.loss(v, x, z, mask, target)
        (Lv + Lp).backward()
        return Lv, Lp, v.grad, x.grad
    a, b = fused(), composed()   # the two arms compute the same thing
    torch.cuda.synchronize()
    diff = [(p.detach().double() - q.detach().double()).abs().max().item() for p, q in zip(a, b)]
    print(f"(a) {game} B {B}: fused vs composed, max abs difference of Lv, Lp, grad_v, grad_logits: "
          + " ".join(f"{d:.2e}" for d in diff))
    report(f"(a) {game} B {B}", alternate({"fused": fused, "composed": composed}, args.rounds, 10 * args.reps), "us", 1e3)


def part_b(game, ts, comp, args, B: int = 256):
    import torch
    from zeroclone_amd import learner
    from zeroclone_amd.nets import PolicyValueNetwork
    dev = ts.rows.device
    kw = {} if game == "chess" else dict(in_planes=2, board=(6, 7), n_logits=7)
    g = torch.Generator().manual_seed(7)
    index = torch.randint(0, len(ts), (B,), generator=g).to(dev)
    arms = {}
    for name in ("fused", "composed"):
        torch.manual_seed(0)
        model = PolicyValueNetwork(128, 8, **kw).to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)

        def step(name=name, model=model, opt=opt):
            opt.zero_grad()
            if name == "fused":
                mb = learner.minibatch(ts, index)
                v, x = model(mb.planes)
                Lv, Lp = learner.policy_value_loss(v, x, mb)
            else:
                planes, z, mask, target = comp.batch(index)
                v, x = model(planes)
                Lv, Lp = comp.loss(v, x, z, mask, target)
            (Lv + Lp).backward()
            opt.step()
        arms[name] = step
    report(f"(b) {game} 128x8 step, B {B}", alternate(arms, args.rounds, max(args.reps // 2, 5)), "ms", 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--games", default="chess,c4")
    args = ap.parse_args()
    import torch
    from zeroclone_amd import _native
    print(f"# tools/ab_learner.py --rounds {args.rounds} --reps {args.reps}; library: "
          f"{_native.lib().zc_version().decode()}; device: {torch.cuda.get_device_name(0)}", flush=True)
    for game in args.games.split(","):
        ts, pool = build_set(game)
        comp = Composed(ts, pool)
        print(f"== {game}: set of {len(ts)} positions, {ts.pi.numel()} visit-count entries", flush=True)
        for B in (256, 4096):
            part_a(game, ts, comp, B, args)
        part_b(game, ts, comp, args)
        pool.close()


if __name__ == "__main__":
    main()
