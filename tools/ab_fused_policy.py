#!/usr/bin/env python3
"""What recording the policy in the fused launches costs, and what it saves: four arms at the
bench's shapes, alternating over several rounds on one device.

  (a) the pooled launch on the PARENT commit's library (--parent-lib, built from the commit
      before fused_policy): the yardstick, in a process of its own (a process loads one
      library) that is started once and runs one timed launch each time it is asked to
  (b) the same launch on this library, switch off      -> must lie inside (a)'s own spread
  (c) the same launch with fused_policy on             -> its cost, as a ratio to (b)
  (d) the same number of moves with step() and record_policy -> the speed-up of (c) over (d)

Connect4: 4096 games x 800 sims, batch 32, run_pooled(K x G, 2K, carry=True) as bench.py's
run_steps times it (launch + recording, wall clock between device syncs); chess crude score:
1024 x 400, run_pooled(K x G, 2K).  Every pool is burned in to mixed game ages first; (d)
adopts (c)'s games.  Rates are expansions per second of the timed window.

    python tools/ab_fused_policy.py --parent-lib zeroclone_amd/libzc_parent.so [--steps 20] [--rounds 7]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("zc_c4_selfplay_visits", "zc_chess_selfplay_visits", "zc_traj_policy_steps_scratch_bytes",
               "zc_traj_policy_record_steps_async")
SHAPES = {"c4": (4096, 800, 32), "chess": (1024, 400, 32)}


def make_pool(game: str, steps: int, burn: bool = True, **kw):
    import torch
    from bench import burn_in
    from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay
    G, S, B = SHAPES[game]
    cap = max(8 * G, 1024, 4 * steps * G // 7 + 2 * G)   # bench.py's rule, with room for two windows
    if game == "c4":
        pool = C4SelfPlay(G, S, batch_size=B, seed=0, games_cap=cap, **kw)
        if burn:
            burn_in(pool)
    else:
        pool = ChessSelfPlay(G, S, batch_size=B, seed=3, games_cap=cap, **kw)
        moves = 0
        while burn and moves < 600 and int(pool.traj.slot[:, 1].min().item()) < G:   # bench.py's chess_burned_pool
            pool.run(25)
            moves += 25
        pool.take()
    torch.cuda.synchronize()
    return pool


def timed_launch(game: str, pool, steps: int) -> float:
    """One pooled launch of steps x G moves and its recording; expansions per second."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if game == "c4":
        pool.run_pooled(steps * pool.G, 2 * steps, carry=True)
    else:
        pool.run_pooled(steps * pool.G, 2 * steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    exp = int(pool.stats[:, 0].sum().item())
    pool.take()
    return exp / dt


def timed_steps(pool, steps: int) -> float:
    """The same number of moves in lockstep: steps x step(); expansions per second."""
    import torch
    torch.cuda.synchronize()
    e0 = int(pool.totals[0].item())
    t0 = time.perf_counter()
    for _ in range(steps):
        pool.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    exp = int(pool.totals[0].item()) - e0
    pool.take()
    return exp / dt


def serve(game: str, steps: int):
    """Arm (a)'s process: the library ZC_LIB names, whose missing entry points stay unbound."""
    from zeroclone_amd import _native
    _native.SIGNATURES = [s for s in _native.SIGNATURES if s[0] not in NEW_SYMBOLS]
    pool = make_pool(game, steps)
    timed_launch(game, pool, steps)   # warm-up: the carry launch's steady state
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print(f"rate {timed_launch(game, pool, steps)!r}", flush=True)
    pool.close()


def answer(child, word: str) -> str:
    """The child's next line that starts with `word` (a library may print lines of its own)."""
    for line in child.stdout:
        if line.startswith(word):
            return line[len(word):].strip()
    sys.exit("the parent library's process ended early")


def ask(child) -> float:
    child.stdin.write("go\n")
    child.stdin.flush()
    return float(answer(child, "rate"))


def spread(xs) -> str:
    med = statistics.median(xs)
    return f"median {med / 1e6:9.1f} M/s  min {min(xs) / 1e6:9.1f}  max {max(xs) / 1e6:9.1f}  " \
           f"spread {(max(xs) - min(xs)) / med * 100:4.1f} %"


def run_game(game: str, args):
    child = None
    if args.parent_lib:
        env = dict(os.environ, ZC_LIB=os.path.abspath(args.parent_lib))
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", game, "--steps", str(args.steps)],
                                 env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        answer(child, "ready")
    b = make_pool(game, args.steps)
    c = make_pool(game, args.steps, record_policy=True, fused_policy=True)
    d = make_pool(game, args.steps, burn=False, record_policy=True)
    d.adopt(c)                                    # the burned-in games of (c), with their visit counts
    for pool in (b, c):
        timed_launch(game, pool, args.steps)      # warm-up, as in the child
    timed_steps(d, 2)
    res = {k: [] for k in "abcd"}
    arms = {"a": lambda: ask(child), "b": lambda: timed_launch(game, b, args.steps),
            "c": lambda: timed_launch(game, c, args.steps), "d": lambda: timed_steps(d, args.steps)}
    order = [k for k in "abcd" if k != "a" or child is not None]
    for rnd in range(args.rounds):
        for k in order[rnd % len(order):] + order[:rnd % len(order)]:   # no arm always follows the same one
            res[k].append(arms[k]())
        print(f"{game} round {rnd}: " + "  ".join(f"({k}) {v[-1] / 1e6:8.1f}" for k, v in res.items() if v), flush=True)
    if child is not None:
        child.stdin.close()
        child.wait(timeout=60)
    G, S, B = SHAPES[game]
    print(f"== {game}: {G} games x {S} sims, batch {B}, {args.steps} steps per window, {args.rounds} rounds, "
          "M expansions/s")
    for k, what in (("a", "parent library, pooled"), ("b", "this library, switch off"),
                    ("c", "fused_policy on"), ("d", "step() + record_policy")):
        if res[k]:
            print(f"({k}) {what:26s} {spread(res[k])}")
    med = {k: statistics.median(v) for k, v in res.items() if v}
    if "a" in med:
        print(f"(b)/(a) = {med['b'] / med['a']:.4f}   (a)'s own range: {min(res['a']) / med['a']:.4f} .. "
              f"{max(res['a']) / med['a']:.4f}")
    print(f"(c)/(b) = {med['c'] / med['b']:.4f}   (c)/(d) = {med['c'] / med['d']:.2f}")
    for pool in (b, c, d):
        pool.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's library (arm a; omitted: arms b, c, d only)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--games", default="c4,chess")
    ap.add_argument("--serve", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args.serve, args.steps)
        return
    for game in args.games.split(","):
        run_game(game, args)


if __name__ == "__main__":
    main()
