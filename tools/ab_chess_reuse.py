#!/usr/bin/env python3
"""A/B of tree reuse on the C5 per-GPU shape (bench.py puct_mode: chess PUCT self-play, 1024
games x 1600 sims, batch 32, the convolutional-head 128 x 8 network on 4 search streams, from
the burned-in crude pool's positions, one graph per step): ChessSelfPlay(reuse_tree=False)
against reuse_tree=True, seeded identically, rounds alternating.  After a burn-in it prints,
per run, ms per step, and for the reuse-on runs the share of searches that reused a tree, the
mean nodes and slots kept, and the mean root visits per search.

    python tools/ab_chess_reuse.py [--games 1024] [--sims 1600] [--burn 3] [--steps 6] [--stat-steps 3] [--rounds 2] [--only off|on]

Timed steps are graph replays with one synchronisation at the end; the statistics come from
further steps that read `kept` and the root visits back after every step.  The slots kept are
not an output of the search: they are counted on the host in the trees of a sample of games
(zc_debug_chess_tree before the step, the subtree of the position the step then keeps)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def subtree(d, r):
    """(nodes, slots) of node r's subtree in a zc_debug_chess_tree dump."""
    nodes = d["nodes"]
    keep = np.zeros(len(nodes), bool)
    keep[r] = True
    par = nodes["parent"].astype(np.int64)
    for i in range(r + 1, len(nodes)):   # ids are in creation order: a parent's id is below its child's
        keep[i] = par[i] < len(nodes) and keep[par[i]]
    return int(keep.sum()), int(nodes["nmoves"][keep].sum())


def run(src, net, games, sims, bs, reuse, burn, steps, stat_steps, sample, dev):
    from zeroclone_amd.selfplay import ChessSelfPlay
    pool = ChessSelfPlay(games, sims, batch_size=bs, seed=6, device=dev.index, puct_net=net, temperature=1.0,
                         puct_streams=4, reuse_tree=reuse)
    pool.adopt(src)
    g = pool.capture_step()
    for _ in range(burn):
        g.replay()
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    for _ in range(steps):
        g.replay()
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t) / steps * 1e3
    out = {"ms": ms}
    reused, knodes, kslots, visits, searches = 0, [], [], [], 0
    for _ in range(stat_steps):
        expect = {}
        if reuse:   # what the coming step keeps, for a sample of games: the subtree of its root
            torch.cuda.synchronize(dev)
            roots = pool.roots.cpu().numpy()
            for s in range(0, games, max(1, games // sample)):
                d = pool.eng.debug_chess_tree(s, max_nodes=pool.eng.max_sims + 1,
                                              max_slots=64 * (pool.eng.max_sims + 1))
                st = d["nodes"]["st"]
                hit = [i for i in range(1, len(st)) if bytes(st[i][:67]) == bytes(roots[s][:67])
                       and int(d["nodes"]["depth"][i]) <= 2]
                expect[s] = [subtree(d, i) for i in hit]   # (a transposition: more than one candidate)
        g.replay()
        torch.cuda.synchronize(dev)
        na = pool.ps.na.sum(dim=1).cpu().numpy()
        visits.append(float(na.mean()))
        searches += games
        if reuse:
            kept = pool.ps.kept.cpu().numpy()
            reused += int((kept > 0).sum())
            knodes.extend(kept[kept > 0].tolist())
            for s, cands in expect.items():
                if kept[s] > 0:
                    sl = [x for n, x in cands if n == kept[s]]
                    assert sl, (s, int(kept[s]), cands)   # the search kept one of the host's subtrees
                    kslots.append(sl[0])
    out["visits"] = statistics.mean(visits) if visits else float("nan")   # (no statistics steps)
    if reuse and searches:
        out.update(share=reused / searches, nodes=statistics.mean(knodes) if knodes else 0.0,
                   slots=statistics.mean(kslots) if kslots else 0.0, sampled=len(kslots))
    pool.check()
    pool.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=1600)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--burn", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--stat-steps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=("off", "on"), help="one variant alone (a profiler run of its kernels)")
    a = ap.parse_args()
    from bench import chess_burned_pool
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, PolicyValueNetwork
    dev = torch.device("cuda", 0)
    src, moves = chess_burned_pool(dev, a.games, 400, 32)
    torch.manual_seed(0)
    net = MfmaPolicyValueNetwork(PolicyValueNetwork(head="conv").eval(), dev)
    print(f"C5 shape: {a.games} games x {a.sims} sims, batch {a.batch}, conv-head 128 x 8 network, 4 streams; crude "
          f"burn-in {moves} moves; per run {a.burn} burn-in steps, {a.steps} timed, {a.stat_steps} for statistics",
          flush=True)
    ms = {False: [], True: []}
    for rnd in range(a.rounds):
        for reuse in ((False, True) if a.only is None else (a.only == "on",)):
            r = run(src, net, a.games, a.sims, a.batch, reuse, a.burn, a.steps, a.stat_steps, a.sample, dev)
            ms[reuse].append(r["ms"])
            line = f"round {rnd} reuse_tree={'on ' if reuse else 'off'} {r['ms']:8.1f} ms/step  root visits/search {r['visits']:.1f}"
            if reuse and "share" in r:
                line += (f"  reused {100 * r['share']:.1f} % of searches, kept {r['nodes']:.1f} nodes / "
                         f"{r['slots']:.1f} slots (slots: {r['sampled']} sampled trees)")
            print(line, flush=True)
    off, on = ms[False], ms[True]
    if a.only is not None:
        return src.close()
    print(f"off: median {statistics.median(off):.1f} ms/step, spread {max(off) - min(off):.1f} ms over {len(off)} runs")
    print(f"on:  median {statistics.median(on):.1f} ms/step, spread {max(on) - min(on):.1f} ms; "
          f"on - off = {statistics.median(on) - statistics.median(off):+.1f} ms")
    src.close()


if __name__ == "__main__":
    main()
