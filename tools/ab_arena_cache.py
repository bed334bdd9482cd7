#!/usr/bin/env python3
"""What an evaluation cache per network (eval_cache / eval_merge on the arena pools) does to the
arena's step, at the arena shapes of profiles/ab_arena.log, with the arms alternating over several
rounds on one device.  Every arm is `steps` step() calls (arm g: graph replays) on one stream with
two different networks, from a burned-in pool's mixed game ages; ms per step, wall clock between
device syncs.

  (p) the plain arena on the PARENT commit's library (--parent-lib), in a process of its own (a
      process loads one library) that runs one timed window each time it is asked to
  (s) the plain arena on this library                  -> (a): must lie inside (p)'s own spread
  (c) the arena with eval_cache alone                  -> (b): (c)/(s), (m)/(s), (b)/(s), with the
  (m) the arena with eval_merge alone                      hit and merged rates per network over
  (b) the arena with both                                  the timed windows
  (g) the arena with both, its step captured once and replayed   -> (c): (g)/(b)

Connect4: 4096 games x 800 sims, batch 32, value-network search (ValueNetwork(128, 8, in_planes=2)
on the MFMA tower); chess: 1024 x 1600 PUCT, policy + value network with the convolutional head,
root noise and temperature as in tools/ab_arena.py.  Entries: the power of two at or above twice
the rows one step probes (--entries-factor), half of them per network.

Each game is measured in a process of its own under `timeout -k 10`, one after the other; the first
that fails, aborts or runs out of time ends the run with its status.

    python tools/ab_arena_cache.py --parent-lib zeroclone_amd/libzc_parent.so [--steps 3] [--rounds 4]
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

from ab_arena import SHAPES, answer, ask, burned, networks, spread, timed_steps  # noqa: E402

NEW_SYMBOLS = ("zc_evalcache_probe_routed_async", "zc_evalcache_commit_routed_async")
ARMS = (("p", "parent library, plain arena"), ("s", "this library, plain arena"), ("c", "eval_cache"),
        ("m", "eval_merge"), ("b", "eval_cache + eval_merge"), ("g", "both, captured step"))
SWITCHES = {"s": {}, "c": dict(cache=True), "m": dict(eval_merge=True), "b": dict(cache=True, eval_merge=True),
            "g": dict(cache=True, eval_merge=True)}
GAME_SECONDS = 900   # a game's process: two burn-ins, six pools, rounds * 6 windows


def entries_for(game: str, factor: float) -> int:
    G, S, _ = SHAPES[game]
    e = 8
    while e < factor * G * S:
        e *= 2
    return e


def make_arena(game: str, src, nets, entries: int = 0, cache: bool = False, eval_merge: bool = False):
    """tools/ab_arena.py's arm (r), with the switches."""
    from zeroclone_amd.arena import C4Arena, ChessArena
    G, S, B = SHAPES[game]
    kw = dict(eval_merge=True) if eval_merge else {}
    if cache:
        kw["eval_cache"] = entries
    if game == "c4":
        pool = C4Arena(G, S, batch_size=B, seed=7, net_a=nets[0], net_b=nets[1], **kw)
    else:
        pool = ChessArena(G, S, batch_size=B, seed=6, puct_net_a=nets[0], puct_net_b=nets[1], temperature=1.0,
                          dirichlet_eps=0.25, **kw)
    pool.adopt(src)
    return pool


class Replayed:
    """Arm (g): the pool's captured step; step() replays it."""

    def __init__(self, pool):
        self.pool, self.graph = pool, pool.capture_step()

    def step(self):
        self.graph.replay()

    def take(self):
        return self.pool.take()


def serve(game: str, steps: int):
    """Arm (p)'s process: the library ZC_LIB names, whose missing entry points stay unbound."""
    from zeroclone_amd import _native
    _native.SIGNATURES = [s for s in _native.SIGNATURES if s[0] not in NEW_SYMBOLS]
    pool = make_arena(game, burned(game), networks(game))
    timed_steps(pool, 1)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print(f"ms {timed_steps(pool, steps)!r}", flush=True)
    pool.close()


def rates(now, seen) -> str:
    """Per network: hits and merged rows of the probed rows since `seen`, and the rows evaluated."""
    out = []
    for name, a, b in zip("AB", now, seen):
        d = {k: a[k] - b[k] for k in a}
        p = max(d["probed"], 1)
        out.append(f"{name}: probed {d['probed']}, hit {d['hits'] / p:.4f}, merged {d.get('merged', 0) / p:.4f}, "
                   f"evaluated {(d['probed'] - d['hits'] - d.get('merged', 0)) / p:.4f}")
    return "   ".join(out)


def run_game(game: str, args):
    import torch  # noqa: F401  (before the library loads: it shares torch's HIP runtime)
    child = None
    if args.parent_lib:
        env = dict(os.environ, ZC_LIB=os.path.abspath(args.parent_lib))
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", game, "--steps", str(args.steps)],
                                 env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        answer(child, "ready")
    src, nets = burned(game), networks(game)
    entries = entries_for(game, args.entries_factor)
    pools = {k: make_arena(game, src, nets, entries, **SWITCHES[k]) for k in "scmbg"}
    runners = dict(pools, g=Replayed(pools["g"]))
    for r in runners.values():
        timed_steps(r, 1)   # warm-up: kernels loaded, buffers allocated
    seen = {k: pools[k].eval_cache_stats(by_network=True) for k in "cmbg"}
    start = dict(seen)
    arms = {k: (lambda k=k: timed_steps(runners[k], args.steps)) for k in runners}
    arms["p"] = lambda: ask(child)
    order = [k for k, _ in ARMS if k != "p" or child is not None]
    res = {k: [] for k in order}
    for rnd in range(args.rounds):
        for k in order[rnd % len(order):] + order[:rnd % len(order)]:   # no arm always follows the same one
            res[k].append(arms[k]())
        print(f"{game} round {rnd}: " + "  ".join(f"({k}) {v[-1]:8.2f}" for k, v in res.items()), flush=True)
        for k in "cmbg":
            now = pools[k].eval_cache_stats(by_network=True)
            print(f"    ({k}) {rates(now, seen[k])}", flush=True)
            seen[k] = now
    if child is not None:
        child.stdin.close()
        child.wait(timeout=60)
    G, S, B = SHAPES[game]
    c = pools["b"]._caches[0]
    print(f"== {game}: {G} games x {S} sims, batch {B}, {args.steps} steps per window, {args.rounds} rounds; per network "
          f"a table of {c.entries} entries, key {c.key_bytes} B, logits {c.logit_bytes} B; ms per step")
    for k, what in ARMS:
        if k in res:
            print(f"({k}) {what:28s} {spread(res[k])}")
    med = {k: statistics.median(v) for k, v in res.items()}
    if "p" in med:
        print(f"(a) (s)/(p) = {med['s'] / med['p']:.4f}   (p)'s own range: {min(res['p']) / med['p']:.4f} .. "
              f"{max(res['p']) / med['p']:.4f}   (s)'s: {min(res['s']) / med['p']:.4f} .. {max(res['s']) / med['p']:.4f}")
    print(f"(b) (c)/(s) = {med['c'] / med['s']:.4f}   (m)/(s) = {med['m'] / med['s']:.4f}   "
          f"(b)/(s) = {med['b'] / med['s']:.4f}")
    print(f"(c) (g)/(b) = {med['g'] / med['b']:.4f}")
    for k in "cmbg":
        print(f"({k}) all windows: {rates(seen[k], start[k])}")
    for k in "sb":
        print(f"({k}) steps {pools[k].steps}, both networks had games in {pools[k].mixed_steps}")
    for pool in pools.values():
        pool.close()
    src.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's library (arm p; omitted: the other arms only)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--entries-factor", type=float, default=2.0,
                    help="table entries (both networks' together) >= this many times the rows one step probes")
    ap.add_argument("--games", default="c4,chess")
    ap.add_argument("--seconds", type=int, default=GAME_SECONDS, help="the time limit of one game's process")
    ap.add_argument("--serve", help=argparse.SUPPRESS)
    ap.add_argument("--run", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args.serve, args.steps)
        return
    if args.run:
        run_game(args.run, args)
        return
    print(f"# tools/ab_arena_cache.py --steps {args.steps} --rounds {args.rounds} --entries-factor {args.entries_factor}"
          + (" --parent-lib <library of the parent commit>" if args.parent_lib else ""), flush=True)
    for game in args.games.split(","):   # one process a game, each under its own time limit
        rc = subprocess.run(["timeout", "-k", "10", str(args.seconds), sys.executable, os.path.abspath(__file__),
                             "--run", game, *sys.argv[1:]]).returncode
        if rc:
            sys.exit(f"{game}: the measurement ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
