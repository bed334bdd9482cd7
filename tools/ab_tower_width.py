#!/usr/bin/env python3
"""What a 64-channel network costs: the fused 64-channel MFMA tower against the path such a
network took before (the folded torch module on MIOpen), with the 128-channel tower for scale.

At the bench's flush shapes, 8 blocks, values out (the tower and the value head):
  (a) nets.for_inference(ValueNetwork(64, 8), backend="torch"): fp16, channels-last, MIOpen
  (b) the fused 64-channel tower with the value head (MfmaValueNetwork: one launch + the planes'
      NHWC conversion)
  (c) the 128-channel tower of the same depth, the same call
The arms alternate over --rounds rounds, each window --reps calls between device events after a
warm-up call; medians, and each arm's own spread over its rounds.  (b) must beat (a) by more than
(a)'s spread.  TFLOP/s: nets.flops_per_position (the stem on its real planes) over the median.
Then one Connect4 value-network pool step at the bench's 4096 x 800 x 32 shape (a captured
search, replayed) with (a) and with (b).  Prints the library's stamp; --quick: small shapes, to
rehearse."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from zeroclone_amd import _native  # noqa: E402
from zeroclone_amd.nets import ValueNetwork, flops_per_position, for_inference  # noqa: E402
from zeroclone_amd.valued import C4ValuedSearch, NetValue  # noqa: E402

ARMS = (("a", "64 channels, torch (MIOpen)"), ("b", "64 channels, fused MFMA tower"),
        ("c", "128 channels, fused MFMA tower"))


def models(planes, blocks):
    torch.manual_seed(0)
    net64 = ValueNetwork(64, blocks, in_planes=planes).eval()
    net128 = ValueNetwork(128, blocks, in_planes=planes).eval()
    return {"a": for_inference(net64, "cuda", torch.float16, backend="torch"),
            "b": for_inference(net64, "cuda", torch.float16, backend="mfma"),
            "c": for_inference(net128, "cuda", torch.float16, backend="mfma")}


def window(model, x, reps):
    with torch.no_grad():
        model(x)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            model(x)
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(ts):
    med = statistics.median(ts)
    return med, min(ts), max(ts), (max(ts) - min(ts)) / med


def towers(args):
    ok = True
    shapes = [(2, 6, 7, 1024), (17, 8, 8, 512)] if args.quick else [(2, 6, 7, 131072), (17, 8, 8, 32768)]
    for planes, h, w, n in shapes:
        ms = models(planes, args.blocks)
        g = torch.Generator(device="cuda").manual_seed(1)
        x = (torch.rand(n, planes, h, w, device="cuda", generator=g) < 0.3).half()
        with torch.no_grad():   # the two 64-channel paths evaluate one network
            va, vb = ms["a"](x).reshape(-1).double(), ms["b"](x).reshape(-1)
            torch.cuda.synchronize()
        err = (va - vb).abs().max().item()
        ts = {k: [] for k, _ in ARMS}
        for rnd in range(args.rounds):
            order = ARMS[rnd % 3:] + ARMS[:rnd % 3]
            for k, _ in order:
                ts[k].append(window(ms[k], x, args.reps))
            print(f"{h}x{w} round {rnd}: " + "  ".join(f"({k}) {ts[k][-1]:8.3f}" for k, _ in ARMS), flush=True)
        print(f"== {h}x{w} x {n} boards, {planes} planes, {args.blocks} blocks, {args.reps} calls per window, "
              f"{args.rounds} rounds, ms per call; max |value (a) - value (b)| = {err:.2e}")
        med = {}
        for k, name in ARMS:
            med[k], lo, hi, spread = summary(ts[k])
            fl = flops_per_position(128 if k == "c" else 64, args.blocks, planes, h, w) * n
            print(f"({k}) {name:32s} median {med[k]:8.3f} ms  min {lo:8.3f}  max {hi:8.3f}  spread {100 * spread:4.1f} %"
                  f"  {fl / med[k] / 1e9:7.1f} TFLOP/s")
        a_lo, a_hi = min(ts["a"]) / med["a"], max(ts["a"]) / med["a"]
        print(f"(b)/(a) = {med['b'] / med['a']:.4f}   (a)'s own range: {a_lo:.4f} .. {a_hi:.4f}   "
              f"(b)/(c) = {med['b'] / med['c']:.4f}")
        ok = ok and max(ts["b"]) < min(ts["a"])
    return ok


def pool_step(args):
    games, sims, bs = (64, 64, 8) if args.quick else (4096, 800, 32)
    ms = models(2, args.blocks)
    roots = torch.zeros((games, 3), dtype=torch.int64, device="cuda")
    ts = {"a": [], "b": []}
    graphs, engines = {}, []
    for k in ts:   # an engine (the same seeds) and a captured search per arm
        eng = _native.NativeEngine(max_games=games, max_sims=sims, max_batch=bs)
        eng.seed(0, list(range(games)))
        engines.append(eng)
        vs = C4ValuedSearch(eng, games, bs, leaves=False)
        value = NetValue(ms[k]) if k == "a" else (lambda leaves, planes, counts, m=ms[k]: m(planes))
        graphs[k] = (vs, vs.capture(roots, sims, 1.4, value))
        graphs[k][1].replay()
        torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for k in (("a", "b") if rnd % 2 == 0 else ("b", "a")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[k][1].replay()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    print(f"== Connect4 value-network pool step: {games} games x {sims} sims, batch {bs}, {args.blocks} blocks, one "
          f"captured search per window, {args.rounds} rounds, ms per step")
    for k in ts:
        med, lo, hi, spread = summary(ts[k])
        print(f"({k}) {dict(ARMS)[k]:32s} median {med:8.2f} ms  min {lo:8.2f}  max {hi:8.2f}  spread {100 * spread:4.1f} %")
    print(f"(b)/(a) = {statistics.median(ts['b']) / statistics.median(ts['a']):.4f}")
    for eng in engines:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-pool", action="store_true")
    args = ap.parse_args()
    print("# tools/ab_tower_width.py " + " ".join(sys.argv[1:]) + f"; library: {_native.lib().zc_version().decode()}",
          flush=True)
    ok = towers(args)
    if not args.no_pool:
        pool_step(args)
    print("(b) beats (a) at both shapes by more than (a)'s spread" if ok else
          "(b) does NOT beat (a) by more than (a)'s spread")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
