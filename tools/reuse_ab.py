#!/usr/bin/env python3
"""A/B in one process: one Connect4 PUCT self-play step (1024 games x 200 sims, batch 32, a
random-init MfmaPolicyValueNetwork) with the tree reuse off and on (C4SelfPlay(reuse_tree=...)),
one captured graph per pool, replayed interleaved.  Prints the median and minimum ms per step
of both and the mean share of kept root visits per search, sum of the kept roots' N / (sims - 1).

  python tools/reuse_ab.py [--games 1024] [--sims 200] [--batch 32] [--reps 30] [--warm 8]
  python tools/reuse_ab.py --off-only [--repo TREE]    # the off pool alone, from another build's tree
"""
import argparse
import os
import statistics
import sys
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=8, help="untimed replays first: the games leave the opening")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--repo", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.repo))
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, PolicyValueNetwork
    from zeroclone_amd.selfplay import C4SelfPlay

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = MfmaPolicyValueNetwork(PolicyValueNetwork(in_planes=2, board=(6, 7), n_logits=7).eval(), dev)
    pools = {}
    for name in ("off",) if a.off_only else ("off", "on"):
        kw = {"reuse_tree": True} if name == "on" else {}
        pool = C4SelfPlay(a.games, a.sims, batch_size=a.batch, seed=7, device=0, puct_net=net, temperature=1.0,
                          **kw)
        pools[name] = (pool, pool.capture_step())
    ms = {name: [] for name in pools}
    share, fresh = [], []
    for rep in range(a.warm + a.reps):
        for name, (pool, g) in pools.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            g.replay()
            torch.cuda.synchronize()
            if rep >= a.warm:
                ms[name].append((time.perf_counter() - t) * 1e3)
                if name == "on":   # a reused search adds sims - 1 visits below its root's kept ones
                    na = pool.ps.na.sum(1).to(torch.float64)
                    share.append(float((na - (a.sims - 1)).mean()) / (a.sims - 1))
                    fresh.append(float((pool.ps.kept == 0).to(torch.float64).mean()))
    for name, v in ms.items():
        print(f"reuse {name}: median {statistics.median(v):.2f} ms  min {min(v):.2f} ms per step "
              f"({a.games} games x {a.sims} sims, batch {a.batch}, {len(v)} interleaved replays)")
    if share:
        print(f"kept root visits per search: {statistics.mean(share):.3f} of sims - 1 "
              f"(searches started afresh: {statistics.mean(fresh):.3f})")
    for pool, _ in pools.values():
        pool.close()


if __name__ == "__main__":
    main()
