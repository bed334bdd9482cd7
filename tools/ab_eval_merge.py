#!/usr/bin/env python3
"""What merging a flush's equal rows (eval_merge: zeroclone_amd/evalcache.py, EvalCache(merge=True))
returns at the bench's four network pool shapes, on the method of tools/ab_eval_cache.py: every
arm is the pool's whole step captured as one HIP graph and replayed `steps` times between two
device events, from a burned-in pool's mixed game ages, the arms' order rotating over the rounds;
ms per step, medians with ranges.  No clock is pinned.

  (p) eval_cache=N on the PARENT commit's library (--parent-lib), in a process of its own (a
      process loads one library) that runs one timed window each time it is asked to
  (o) eval_cache=N on this library, merging off          -> must lie inside (p)'s own range
  (m) eval_cache=N + eval_merge                          -> (m)/(o): what merging adds to the cache
  (t) eval_merge alone (no table)                        -> (t)/(n): what merging returns alone
  (n) neither

and from the counters: the rows the tower evaluated per step in each arm and the merged share of
the probed rows.  Every arm plays the same games (the options change no move), so the rows are
comparable window by window: (m) must evaluate no more rows than (o).

  c4_value    Connect4, 4096 games x 800 sims, value network (bench.py net_mode), 1 stream
  c4_puct     Connect4, 4096 x 800, PUCT, 7-logit linear head (c4_puct_mode), 4 streams
  chess_value chess, 1024 x 400, value network (chess_modes), 4 streams
  chess_puct  chess, 1024 x 1600, PUCT, convolutional head (puct_mode), 4 streams

    python tools/ab_eval_merge.py --parent-lib zeroclone_amd/libzc_parent.so [--steps 3] [--rounds 5]
"""
import argparse
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from ab_eval_cache import SHAPES, Window, answer, ask, burned, entries_for, spread  # noqa: E402

NEW_SYMBOLS = ("zc_evalcache_merge_scratch_bytes", "zc_evalcache_probe_merged_async",
               "zc_evalcache_commit_merged_async")
ARMS = (("p", "parent library, cache"), ("o", "this library, cache"), ("m", "cache + merge"),
        ("t", "merge alone"), ("n", "neither"))


def make_pool(shape: str, src, eval_cache: int, eval_merge: bool):
    """The pool of bench.py's mode of that name, with the options."""
    import torch
    from zeroclone_amd import _native
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, PolicyValueNetwork, ValueNetwork, for_inference
    from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay
    G, S, B = SHAPES[shape]
    dev = torch.device("cuda", 0)
    kw = dict(eval_cache=eval_cache) if eval_cache else {}
    if eval_merge:
        kw["eval_merge"] = True
    torch.manual_seed(0)
    if shape == "c4_value":
        net = for_inference(ValueNetwork(128, 8, in_planes=2).eval(), dev, torch.float16)
        pool = C4SelfPlay(G, S, c=1.4, batch_size=B, seed=7, net=net, streams=1, **kw)
    elif shape == "c4_puct":
        net = MfmaPolicyValueNetwork(PolicyValueNetwork(in_planes=2, board=(6, 7), n_logits=7).eval(), dev)
        pool = C4SelfPlay(G, S, batch_size=B, seed=7, puct_net=net, temperature=1.0, streams=4, **kw)
    elif shape == "chess_value":
        net = for_inference(ValueNetwork(128, 8).eval(), dev, torch.float16)
        pool = ChessSelfPlay(G, S, batch_size=B, seed=4, net=net, policy=_native.ZC_POLICY_RANDOM, freedom=0.0,
                             streams=4, **kw)
    else:
        net = MfmaPolicyValueNetwork(PolicyValueNetwork(head="conv").eval(), dev)
        pool = ChessSelfPlay(G, S, batch_size=B, seed=6, puct_net=net, temperature=1.0, puct_streams=4, **kw)
    pool.adopt(src)
    return pool


def serve(shape: str, steps: int, entries: int):
    """Arm (p)'s process: the library ZC_LIB names, whose missing entry points stay unbound."""
    from zeroclone_amd import _native
    _native.SIGNATURES = [s for s in _native.SIGNATURES if s[0] not in NEW_SYMBOLS]
    src = burned(shape)
    w = Window(make_pool(shape, src, entries, False))
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print(f"ms {w.run(steps)!r}", flush=True)
    w.pool.close()
    src.close()


def tower_rows(d: dict) -> int:
    return d["probed"] - d["hits"] - d.get("merged", 0)


def run_shape(shape: str, args):
    entries = entries_for(shape, args.entries_factor)
    child = None
    if args.parent_lib:
        env = dict(os.environ, ZC_LIB=os.path.abspath(args.parent_lib))
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", shape, "--steps", str(args.steps),
                                  "--entries", str(entries)],
                                 env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        answer(child, "ready")
    src = burned(shape)
    wins = {"o": Window(make_pool(shape, src, entries, False)), "m": Window(make_pool(shape, src, entries, True)),
            "t": Window(make_pool(shape, src, 0, True)), "n": Window(make_pool(shape, src, 0, False))}
    arms = {k: (lambda k=k: wins[k].run(args.steps)) for k in wins}
    arms["p"] = lambda: ask(child)
    order = [k for k, _ in ARMS if k != "p" or child is not None]
    res = {k: [] for k in order}
    counted = {k: wins[k].pool for k in "omt"}
    seen = {k: p.eval_cache_stats() for k, p in counted.items()}
    deltas = {k: [] for k in counted}
    for rnd in range(args.rounds):
        for k in order[rnd % len(order):] + order[:rnd % len(order)]:   # no arm always follows the same one
            res[k].append(arms[k]())
        for k, p in counted.items():
            now = p.eval_cache_stats()
            deltas[k].append({x: now[x] - seen[k][x] for x in now})
            seen[k] = now
        d = {k: v[-1] for k, v in deltas.items()}
        print(f"{shape} round {rnd}: " + "  ".join(f"({k}) {v[-1]:9.2f}" for k, v in res.items())
              + "   tower rows/step " + "  ".join(f"({k}) {tower_rows(d[k]) / args.steps:.0f}" for k in d)
              + f"  (n) {d['t']['probed'] / args.steps:.0f}   merged of probed (m) "
              f"{d['m']['merged'] / d['m']['probed']:.4f} (t) {d['t']['merged'] / d['t']['probed']:.4f}   "
              f"dropped of (o)'s misses {d['o']['dropped'] / max(d['o']['inserts'] + d['o']['dropped'], 1):.3f}",
              flush=True)
    if child is not None:
        child.stdin.close()
        child.wait(timeout=60)
    G, S, B = SHAPES[shape]
    caches = counted["m"]._caches
    print(f"== {shape}: {G} games x {S} sims, batch {B}, {args.steps} steps per window, {args.rounds} rounds; "
          f"{len(caches)} table(s) of {caches[0].entries} entries, key {caches[0].key_bytes} B, logits "
          f"{caches[0].logit_bytes} B; no clock pinned")
    for k, what in ARMS:
        if k in res:
            print(f"({k}) {what:22s} {spread(res[k])}")
    med = {k: statistics.median(v) for k, v in res.items()}
    if "p" in med:
        print(f"(o)/(p) = {med['o'] / med['p']:.4f}   (p)'s own range: {min(res['p']) / med['p']:.4f} .. "
              f"{max(res['p']) / med['p']:.4f}")
    n_steps = args.steps * args.rounds
    tot = {k: {x: sum(d[x] for d in v) for x in v[0]} for k, v in deltas.items()}
    rows = {k: tower_rows(tot[k]) / n_steps for k in tot}
    rows["n"] = tot["t"]["probed"] / n_steps
    print(f"(m)/(o) = {med['m'] / med['o']:.4f}   (t)/(n) = {med['t'] / med['n']:.4f}   tower rows per step over the "
          f"{n_steps} timed steps: " + "  ".join(f"({k}) {rows[k]:.0f}" for k in "omtn")
          + f"   merged of probed: (m) {tot['m']['merged'] / tot['m']['probed']:.4f}  (t) "
          f"{tot['t']['merged'] / tot['t']['probed']:.4f}")
    worst = max(tower_rows(dm) - tower_rows(do) for dm, do in zip(deltas["m"], deltas["o"]))
    print(f"(m) evaluates no more rows than (o) in every window: {worst <= 0}  (largest (m) - (o): {worst})")
    for w in wins.values():
        w.pool.close()
    src.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's library (arm p; omitted: the other arms only)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--entries-factor", type=float, default=2.0,
                    help="table entries >= this many times the rows one step probes")
    ap.add_argument("--serve", help=argparse.SUPPRESS)
    ap.add_argument("--entries", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args.serve, args.steps, args.entries)
        return
    import torch  # noqa: F401  (before the library loads: it shares torch's HIP runtime)
    from zeroclone_amd import _native
    print(f"# tools/ab_eval_merge.py --steps {args.steps} --rounds {args.rounds} --entries-factor {args.entries_factor}"
          + (" --parent-lib <library of the parent commit>" if args.parent_lib else "")
          + f"; library: {_native.lib().zc_version().decode()}", flush=True)
    for shape in args.shapes.split(","):
        run_shape(shape, args)


if __name__ == "__main__":
    main()
