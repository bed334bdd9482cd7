#!/usr/bin/env python3
"""What the evaluation cache (zeroclone_amd/evalcache.py) returns at the bench's four network
pool shapes, with the arms alternating over several rounds on one device.  Every arm is the
pool's whole step captured as one HIP graph (bench.py's _timed_pool_steps) and replayed `steps`
times between two device events, from a burned-in pool's mixed game ages; ms per step.

  (p) the pool without the cache on the PARENT commit's library (--parent-lib), in a process of
      its own (a process loads one library) that runs one timed window each time it is asked to
  (o) the pool without the cache on this library          -> must lie inside (p)'s spread
  (c) the pool with eval_cache                            -> (c)/(o): what the option returns

and from (c)'s counters: the hit rate and the rows the tower evaluated per step (without the
cache the tower evaluates every probed row).  The tables keep filling from window to window, as
they do in a self-play run: the rounds' hit rates are printed one by one.

  c4_value    Connect4, 4096 games x 800 sims, value network (bench.py net_mode), 1 stream
  c4_puct     Connect4, 4096 x 800, PUCT, 7-logit linear head (c4_puct_mode), 4 streams
  chess_value chess, 1024 x 400, value network (chess_modes), 4 streams
  chess_puct  chess, 1024 x 1600, PUCT, convolutional head (puct_mode), 4 streams

Entries: the power of two at or above twice the rows one step probes (--entries-factor).

    python tools/ab_eval_cache.py --parent-lib zeroclone_amd/libzc_parent.so [--steps 3] [--rounds 5]
"""
import argparse
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("zc_evalcache_bytes", "zc_evalcache_clear_async", "zc_evalcache_probe_async",
               "zc_evalcache_commit_async", "zc_net_tower_counted_async", "zc_net_tower_policy_counted_async")
SHAPES = {"c4_value": (4096, 800, 32), "c4_puct": (4096, 800, 32), "chess_value": (1024, 400, 32),
          "chess_puct": (1024, 1600, 32)}
ARMS = (("p", "parent library, cache off"), ("o", "this library, cache off"), ("c", "this library, cache on"))


def entries_for(shape: str, factor: float) -> int:
    G, S, _ = SHAPES[shape]
    e = 8
    while e < factor * G * S:
        e *= 2
    return e


def burned(shape: str):
    """bench.py's burned-in pools: the rollout pool (Connect4), the crude-score pool (chess)."""
    import torch
    from bench import burn_in, chess_burned_pool
    from zeroclone_amd.selfplay import C4SelfPlay
    if shape.startswith("c4"):
        src = C4SelfPlay(4096, 800, batch_size=32, seed=0)
        burn_in(src)
    else:
        src, _ = chess_burned_pool(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return src


def make_pool(shape: str, src, eval_cache: int):
    """The pool of bench.py's mode of that name, with the option."""
    import torch
    from zeroclone_amd import _native
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, PolicyValueNetwork, ValueNetwork, for_inference
    from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay
    G, S, B = SHAPES[shape]
    dev = torch.device("cuda", 0)
    kw = dict(eval_cache=eval_cache) if eval_cache else {}
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


class Window:
    """A pool's captured step and its timed windows."""

    def __init__(self, pool):
        import torch
        self.pool, self.graph = pool, pool.capture_step()
        self.graph.replay()   # warm-up
        torch.cuda.synchronize()
        pool.take()

    def run(self, steps: int) -> float:
        """ms per step of `steps` replays, between two device events."""
        import torch
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev[0].record()
        for _ in range(steps):
            self.graph.replay()
        ev[1].record()
        torch.cuda.synchronize()
        self.pool.take()
        return ev[0].elapsed_time(ev[1]) / steps


def serve(shape: str, steps: int):
    """Arm (p)'s process: the library ZC_LIB names, whose missing entry points stay unbound."""
    from zeroclone_amd import _native
    _native.SIGNATURES = [s for s in _native.SIGNATURES if s[0] not in NEW_SYMBOLS]
    src = burned(shape)
    w = Window(make_pool(shape, src, 0))
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print(f"ms {w.run(steps)!r}", flush=True)
    w.pool.close()
    src.close()


def answer(child, word: str) -> str:
    for line in child.stdout:
        if line.startswith(word):
            return line[len(word):].strip()
    sys.exit("the parent library's process ended early")


def ask(child) -> float:
    child.stdin.write("go\n")
    child.stdin.flush()
    return float(answer(child, "ms"))


def spread(xs) -> str:
    med = statistics.median(xs)
    return (f"median {med:9.2f} ms/step  min {min(xs):9.2f}  max {max(xs):9.2f}  "
            f"spread {(max(xs) - min(xs)) / med * 100:4.1f} %")


def run_shape(shape: str, args):
    child = None
    if args.parent_lib:
        env = dict(os.environ, ZC_LIB=os.path.abspath(args.parent_lib))
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", shape, "--steps", str(args.steps)],
                                 env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        answer(child, "ready")
    src = burned(shape)
    entries = entries_for(shape, args.entries_factor)
    wins = {"o": Window(make_pool(shape, src, 0)), "c": Window(make_pool(shape, src, entries))}
    arms = {k: (lambda k=k: wins[k].run(args.steps)) for k in wins}
    arms["p"] = lambda: ask(child)
    order = [k for k, _ in ARMS if k != "p" or child is not None]
    res = {k: [] for k in order}
    pool_c = wins["c"].pool
    seen, rates = pool_c.eval_cache_stats(), []
    for rnd in range(args.rounds):
        for k in order[rnd % len(order):] + order[:rnd % len(order)]:   # no arm always follows the same one
            res[k].append(arms[k]())
        now = pool_c.eval_cache_stats()
        d = {k: now[k] - seen[k] for k in now}
        seen = now
        rates.append(d)
        print(f"{shape} round {rnd}: " + "  ".join(f"({k}) {v[-1]:9.2f}" for k, v in res.items())
              + f"   hit rate {d['hits'] / d['probed']:.4f}  tower rows/step {(d['probed'] - d['hits']) / args.steps:.0f}"
              f" of {d['probed'] / args.steps:.0f}  dropped inserts {d['dropped'] / max(d['inserts'] + d['dropped'], 1):.3f}",
              flush=True)
    if child is not None:
        child.stdin.close()
        child.wait(timeout=60)
    G, S, B = SHAPES[shape]
    caches = pool_c._caches
    print(f"== {shape}: {G} games x {S} sims, batch {B}, {args.steps} steps per window, {args.rounds} rounds; "
          f"{len(caches)} table(s) of {caches[0].entries} entries, key {caches[0].key_bytes} B, logits "
          f"{caches[0].logit_bytes} B, {sum(c.table.numel() for c in caches) / 2 ** 20:.0f} MiB in all")
    for k, what in ARMS:
        if k in res:
            print(f"({k}) {what:26s} {spread(res[k])}")
    med = {k: statistics.median(v) for k, v in res.items()}
    if "p" in med:
        print(f"(o)/(p) = {med['o'] / med['p']:.4f}   (p)'s own range: {min(res['p']) / med['p']:.4f} .. "
              f"{max(res['p']) / med['p']:.4f}")
    tot = {k: sum(d[k] for d in rates) for k in rates[0]}
    n_steps = args.steps * args.rounds
    print(f"(c)/(o) = {med['c'] / med['o']:.4f}   hit rate {tot['hits'] / tot['probed']:.4f} over the {n_steps} timed "
          f"steps; tower rows per step: {(tot['probed'] - tot['hits']) / n_steps:.0f} with the cache, "
          f"{tot['probed'] / n_steps:.0f} without")
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
    args = ap.parse_args()
    if args.serve:
        serve(args.serve, args.steps)
        return
    import torch  # noqa: F401  (before the library loads: it shares torch's HIP runtime)
    from zeroclone_amd import _native
    print(f"# tools/ab_eval_cache.py --steps {args.steps} --rounds {args.rounds} --entries-factor {args.entries_factor}"
          + (" --parent-lib <library of the parent commit>" if args.parent_lib else "")
          + f"; library: {_native.lib().zc_version().decode()}", flush=True)
    for shape in args.shapes.split(","):
        run_shape(shape, args)


if __name__ == "__main__":
    main()
