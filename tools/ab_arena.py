#!/usr/bin/env python3
"""What the arena's routing costs and what it saves, at the bench's network shapes, with the
arms alternating over several rounds on one device.  Every arm is `steps` eager step() calls
(the arena cannot be captured: its group sizes are host values) on one stream, from a burned-in
pool's mixed game ages; ms per step, wall clock between device syncs.

  (p) self-play with one network on the PARENT commit's library (--parent-lib), in a process of
      its own (a process loads one library) that runs one timed window each time it is asked to
  (s) the same self-play pool on this library                   -> must lie inside (p)'s spread
  (a) the arena with net_a is net_b                             -> (a)/(s): routing + the per-step read
  (r) the arena with two different networks
  (e) the self-play pool with an evaluate-both callable (both networks on every leaf, selected
      with torch.where; defined here, not in the package)       -> (r)/(e): what routing saves
  (c) the route, gather and scatter kernels alone at those shapes, us per call and GB/s

Connect4: 4096 games x 800 sims, batch 32, value-network search (ValueNetwork(128, 8, in_planes=2)
on the MFMA tower); chess: 1024 x 1600 PUCT (the per-GPU C5 shard), policy + value network with
the convolutional head, root noise and temperature as bench.py's puct_mode in every arm.

    python tools/ab_arena.py --parent-lib zeroclone_amd/libzc_parent.so [--steps 3] [--rounds 4]
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

NEW_SYMBOLS = ("zc_arena_route_async", "zc_arena_gather_async", "zc_arena_scatter_async")
SHAPES = {"c4": (4096, 800, 32), "chess": (1024, 1600, 32)}
ARMS = (("p", "parent library, self-play"), ("s", "this library, self-play"), ("a", "arena, net_a is net_b"),
        ("r", "arena, two networks"), ("e", "self-play, evaluate both"))


def networks(game: str):
    import torch
    from zeroclone_amd.nets import (MfmaPolicyValueNetwork, PolicyValueNetwork, ValueNetwork, for_inference)
    dev, out = torch.device("cuda", 0), []
    for seed in (0, 1):
        torch.manual_seed(seed)
        if game == "c4":
            out.append(for_inference(ValueNetwork(128, 8, in_planes=2).eval(), dev, torch.float16))
        else:
            out.append(MfmaPolicyValueNetwork(PolicyValueNetwork(head="conv").eval(), dev))
    return out


def burned(game: str):
    """bench.py's burned-in pools: the rollout pool (Connect4), the crude-score pool (chess)."""
    import torch
    from bench import burn_in, chess_burned_pool
    from zeroclone_amd.selfplay import C4SelfPlay
    if game == "c4":
        src = C4SelfPlay(4096, 800, batch_size=32, seed=0)
        burn_in(src)
    else:
        src, _ = chess_burned_pool(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return src


class Both:
    """Both networks on every row, selected per game with torch.where: the arena without routing."""
    roots_only = True

    def __init__(self, pool, net_a, net_b, chess: bool):
        self.pool, self.nets, self.chess = pool, (net_a, net_b), chess

    def __call__(self, leaves, planes, counts):
        import torch
        p = self.pool
        turn = (p.roots[:, 64].long() if self.chess else p.roots[:, 2]) & 1
        gno = p.traj.slot[:, 1].long()
        b = ((turn ^ ((gno & 1) ^ 1)) == 1) & (gno >= 0)
        sel = b.repeat_interleave(planes.shape[0] // counts.shape[0])
        oa, ob = self.nets[0](planes), self.nets[1](planes)
        if not self.chess:
            return torch.where(sel, ob.reshape(-1).to(torch.float64), oa.reshape(-1).to(torch.float64))
        return torch.where(sel, ob[0], oa[0]), torch.where(sel[:, None], ob[1], oa[1])


def make_pool(game: str, arm: str, src, nets):
    from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay
    G, S, B = SHAPES[game]
    a, b = nets[0], nets[0] if arm == "a" else nets[1]
    if arm in "ar":
        from zeroclone_amd.arena import C4Arena, ChessArena
        if game == "c4":
            pool = C4Arena(G, S, batch_size=B, seed=7, net_a=a, net_b=b)
        else:
            pool = ChessArena(G, S, batch_size=B, seed=6, puct_net_a=a, puct_net_b=b, temperature=1.0,
                              dirichlet_eps=0.25)
    elif game == "c4":
        pool = C4SelfPlay(G, S, batch_size=B, seed=7, net=a)
        if arm == "e":
            pool.value_fn = Both(pool, a, b, False)
    else:
        pool = ChessSelfPlay(G, S, batch_size=B, seed=6, puct_net=a, temperature=1.0)
        if arm == "e":
            pool.net_fn = Both(pool, a, b, True)
    pool.adopt(src)
    return pool


def timed_steps(pool, steps: int) -> float:
    """ms per step of `steps` eager steps."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        pool.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    pool.take()
    return dt / steps * 1e3


def serve(game: str, steps: int):
    """Arm (p)'s process: the library ZC_LIB names, whose missing entry points stay unbound."""
    from zeroclone_amd import _native
    _native.SIGNATURES = [s for s in _native.SIGNATURES if s[0] not in NEW_SYMBOLS]
    pool = make_pool(game, "s", burned(game), networks(game))
    timed_steps(pool, 1)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print(f"ms {timed_steps(pool, steps)!r}", flush=True)
    pool.close()


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


def run_game(game: str, args):
    child = None
    if args.parent_lib:
        env = dict(os.environ, ZC_LIB=os.path.abspath(args.parent_lib))
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", game, "--steps", str(args.steps)],
                                 env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        answer(child, "ready")
    src, nets = burned(game), networks(game)
    pools = {k: make_pool(game, k, src, nets) for k in "sare"}
    for pool in pools.values():
        timed_steps(pool, 1)   # warm-up: kernels loaded, buffers allocated
    arms = {k: (lambda k=k: timed_steps(pools[k], args.steps)) for k in pools}
    arms["p"] = lambda: ask(child)
    order = [k for k, _ in ARMS if k != "p" or child is not None]
    res = {k: [] for k in order}
    for rnd in range(args.rounds):
        for k in order[rnd % len(order):] + order[:rnd % len(order)]:   # no arm always follows the same one
            res[k].append(arms[k]())
        print(f"{game} round {rnd}: " + "  ".join(f"({k}) {v[-1]:8.2f}" for k, v in res.items()), flush=True)
    if child is not None:
        child.stdin.close()
        child.wait(timeout=60)
    G, S, B = SHAPES[game]
    print(f"== {game}: {G} games x {S} sims, batch {B}, {args.steps} steps per window, {args.rounds} rounds, ms per step")
    for k, what in ARMS:
        if k in res:
            print(f"({k}) {what:26s} {spread(res[k])}")
    med = {k: statistics.median(v) for k, v in res.items()}
    if "p" in med:
        print(f"(s)/(p) = {med['s'] / med['p']:.4f}   (p)'s own range: {min(res['p']) / med['p']:.4f} .. "
              f"{max(res['p']) / med['p']:.4f}")
    for k in "ar":
        print(f"({k}) steps {pools[k].steps}, both groups non-empty in {pools[k].mixed_steps}, last group sizes "
              f"{pools[k].count.tolist()}")
    print(f"(a)/(s) = {med['a'] / med['s']:.4f}   (r)/(e) = {med['r'] / med['e']:.4f}   (r)/(s) = {med['r'] / med['s']:.4f}")
    for pool in pools.values():
        pool.close()
    src.close()


def kernels_alone(reps: int = 20):
    """(c): the three kernels at the two pools' shapes, a random key."""
    import torch
    from zeroclone_amd import _native
    s = torch.cuda.current_stream().cuda_stream

    def timed(fn) -> float:
        for _ in range(3):
            fn()
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us

    print("== (c) the kernels alone: us per call; GB/s = bytes read + bytes written")
    for game, rows_of in (("c4", (("fp64 values", 8), ("planes fp16 [2,6,7]", 168))),
                          ("chess", (("fp64 values", 8), ("NHWC planes fp16 [64,32]", 4096), ("logits fp16 [4096]", 8192)))):
        G, _, B = SHAPES[game]
        key = torch.randint(0, 2, (G,), dtype=torch.int32, device="cuda")
        perm = torch.zeros(G, dtype=torch.int32, device="cuda")
        count = torch.zeros(2, dtype=torch.int32, device="cuda")
        us = timed(lambda: _native.arena_route(G, key.data_ptr(), perm.data_ptr(), count.data_ptr(), s))
        print(f"{game}: route, {G} games: {us:8.1f} us   (group sizes {count.tolist()})")
        for what, rb in rows_of:
            src = torch.randint(0, 255, (G * B * rb,), dtype=torch.uint8, device="cuda")
            dst = torch.zeros_like(src)
            for name, fn in (("gather", _native.arena_gather), ("scatter", _native.arena_scatter)):
                us = timed(lambda: fn(G, B, B, rb, perm.data_ptr(), src.data_ptr(), dst.data_ptr(), s))
                print(f"{game}: {name:7s} {what:26s} {G * B} rows x {rb:5d} B: {us:8.1f} us  "
                      f"{2 * G * B * rb / us / 1e3:8.1f} GB/s")
            us = timed(lambda: torch.index_select(src.view(G, -1), 0, perm.long()))
            print(f"{game}: torch index_select of the same rows (with its int64 index, a new tensor): {us:8.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's library (arm p; omitted: the other arms only)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--games", default="c4,chess")
    ap.add_argument("--serve", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args.serve, args.steps)
        return
    import torch  # noqa: F401  (before the library loads: it shares torch's HIP runtime)
    from zeroclone_amd import _native
    print(f"# tools/ab_arena.py --steps {args.steps} --rounds {args.rounds}"
          + (" --parent-lib <library of the parent commit>" if args.parent_lib else "")
          + f"; library: {_native.lib().zc_version().decode()}", flush=True)
    kernels_alone()
    for game in args.games.split(","):
        run_game(game, args)


if __name__ == "__main__":
    main()
