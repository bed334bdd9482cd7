#!/usr/bin/env python3
"""What a book of openings costs per step and what it buys, on one device.

Step cost, at the bench's pool shapes, the arms alternating over several rounds; every arm is
`steps` eager step() calls from a burned-in pool's mixed game ages, timed with device events, ms
per step, medians, the parent library's own window spread beside them:

  (p) self-play without a book on the PARENT commit's library (--parent-lib), in a process of its
      own (a process loads one library) that runs one timed window each time it is asked to
  (s) the same self-play pool on this library            -> must lie inside (p)'s spread
  (b) the self-play pool with a book                     -> (b)/(s): zc_traj_openings_async per step
  (a) the arena (two networks) without a book
  (k) the arena with the book                            -> (k)/(a)

Connect4: 4096 games x 800 sims, batch 32, value-network search (ValueNetwork(128, 8, in_planes=2)
on the MFMA tower); chess: 1024 x 1600 PUCT, policy + value network with the convolutional head,
root noise and temperature as bench.py's puct_mode.  The books are `openings_from_games` of the
burned-in pools' own finished games, 64 rows (Connect4: ply 4; chess: plies 8, 16, 24, ... until
there are 64 — the crude-score search opens every game alike).

What the book buys: 256 Connect4 arena games (64 slots, the arena's defaults, an evaluation cache
per network) without a book and with 64 rows from `openings_from_games(batch, ply=4)`: the distinct
games (distinct move sequences) among them and the caches' hit rate.

    python tools/ab_openings.py --parent-lib zeroclone_amd/libzc_parent.so [--steps 3] [--rounds 4]
"""
import argparse
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("zc_traj_openings_async", "zc_c4_puct_forget_fresh", "zc_chess_puct_forget_fresh")
SHAPES = {"c4": (4096, 800, 32), "chess": (1024, 1600, 32)}
BOOK_PLY = {"c4": 4, "chess": 8}
ARMS = (("p", "parent library, self-play"), ("s", "self-play, no book"), ("b", "self-play, book"),
        ("a", "arena, no book"), ("k", "arena, book"))


def networks(game: str):
    import torch
    from zeroclone_amd.nets import MfmaPolicyValueNetwork, PolicyValueNetwork, ValueNetwork, for_inference
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


def book_of(game: str, src, rows: int = 64):
    """The burned-in pool plays on; the games it finishes give the book."""
    from zeroclone_amd.selfplay import openings_from_games
    import torch
    src.run(8 if game == "c4" else 25)
    batch = src.take()
    plies = [BOOK_PLY[game]]
    book = openings_from_games(batch, plies[0], rows)
    for ply in range(2 * BOOK_PLY[game], 25 * BOOK_PLY[game], BOOK_PLY[game]):
        if game == "c4" or book.shape[0] >= rows:
            break
        plies.append(ply)
        book = torch.unique(torch.cat([book, openings_from_games(batch, ply)]), dim=0)[:rows]
    if book.shape[0] < rows:
        sys.exit(f"{game}: the burned-in pool's games gave {book.shape[0]} openings, {rows} wanted")
    return book, plies


def make_pool(game: str, arm: str, src, nets, book):
    from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay
    G, S, B = SHAPES[game]
    kw = dict(openings=book) if arm in "bk" else {}
    if arm in "ak":
        from zeroclone_amd.arena import C4Arena, ChessArena
        if game == "c4":
            pool = C4Arena(G, S, batch_size=B, seed=7, net_a=nets[0], net_b=nets[1], **kw)
        else:
            pool = ChessArena(G, S, batch_size=B, seed=6, puct_net_a=nets[0], puct_net_b=nets[1], temperature=1.0,
                              dirichlet_eps=0.25, **kw)
    elif game == "c4":
        pool = C4SelfPlay(G, S, batch_size=B, seed=7, net=nets[0], **kw)
    else:
        pool = ChessSelfPlay(G, S, batch_size=B, seed=6, puct_net=nets[0], temperature=1.0, **kw)
    pool.adopt(src)
    return pool


def timed_steps(pool, steps: int) -> float:
    """ms per step of `steps` eager steps, between two device events."""
    import torch
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(steps):
        pool.step()
    ev[1].record()
    torch.cuda.synchronize()
    pool.take()
    return ev[0].elapsed_time(ev[1]) / steps


def serve(game: str, steps: int):
    """Arm (p)'s process: the library ZC_LIB names, whose missing entry point stays unbound."""
    from zeroclone_amd import _native
    _native.SIGNATURES = [s for s in _native.SIGNATURES if s[0] not in NEW_SYMBOLS]
    pool = make_pool(game, "s", burned(game), networks(game), None)
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


def refills(pool) -> int:
    """Games started beyond the first one of each slot."""
    import torch  # noqa: F401
    from zeroclone_amd import _native
    return int(pool.traj.ctl[_native.ZC_TRAJ_NEXT]) - pool.G


def run_game(game: str, args):
    child = None
    if args.parent_lib:
        env = dict(os.environ, ZC_LIB=os.path.abspath(args.parent_lib))
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", game, "--steps", str(args.steps)],
                                 env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        answer(child, "ready")
    src, nets = burned(game), networks(game)
    book, plies = book_of(game, src)
    pools = {k: make_pool(game, k, src, nets, book) for k in "sbak"}
    start = {k: refills(p) for k, p in pools.items()}
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
    print(f"== {game}: {G} games x {S} sims, batch {B}, {args.steps} steps per window, {args.rounds} rounds, a book of "
          f"{book.shape[0]} rows from " + ("ply " if len(plies) == 1 else "plies ") + ", ".join(map(str, plies))
          + ", ms per step")
    for k, what in ARMS:
        if k in res:
            print(f"({k}) {what:26s} {spread(res[k])}")
    med = {k: statistics.median(v) for k, v in res.items()}
    if "p" in med:
        print(f"(s)/(p) = {med['s'] / med['p']:.4f}   (p)'s own range: {min(res['p']) / med['p']:.4f} .. "
              f"{max(res['p']) / med['p']:.4f}")
    print(f"(b)/(s) = {med['b'] / med['s']:.4f}   (k)/(a) = {med['k'] / med['a']:.4f}   games refilled in the windows: "
          + "  ".join(f"({k}) {refills(p) - start[k]}" for k, p in pools.items()))
    for pool in pools.values():
        pool.close()
    src.close()


def kernel_alone(reps: int = 50):
    """zc_traj_openings_async alone at the two pools' shapes, every slot fresh (the most it writes)."""
    import torch
    from zeroclone_amd.selfplay import Trajectories
    print("== the seeding kernel alone, every slot at a game's first position: us per call")
    for game, words, max_len in (("c4", 3, 43), ("chess", 9, 2049)):
        G = SHAPES[game][0]
        dev = torch.device("cuda", 0)
        tj = Trajectories(G, torch.zeros(words, dtype=torch.int64), max_len, 8, 8 * max_len, dev)
        book = torch.arange(64 * words, dtype=torch.int64, device=dev).reshape(64, words)
        roots = torch.zeros((G, words), dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        for _ in range(3):
            tj.seed_openings(book, 1, roots, s)
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev[0].record()
        for _ in range(reps):
            tj.seed_openings(book, 1, roots, s)
        ev[1].record()
        torch.cuda.synchronize()
        print(f"{game}: {G} slots x {8 * words} B: {ev[0].elapsed_time(ev[1]) / reps * 1e3:7.1f} us")


def what_the_book_buys(total: int = 256, slots: int = 64, rows: int = 64):
    """256 Connect4 arena games at the arena's defaults, cached, without and with a book."""
    import torch
    from zeroclone_amd.arena import C4Arena
    from zeroclone_amd.selfplay import C4SelfPlay, openings_from_games, simulate_games
    nets = networks("c4")
    src = C4SelfPlay(1024, 100, batch_size=32, seed=11)       # rollout self-play: the book's source
    simulate_games(src, 1024)
    book = openings_from_games(src.last_batch, 4, rows)
    src.close()
    print(f"== what the book buys: {total} Connect4 arena games on {slots} slots, 800 sims, two value networks, "
          f"eval_cache 2^20 entries + eval_merge; the book: {book.shape[0]} rows of openings_from_games(batch, ply=4) "
          f"from 1024 rollout self-play games")
    for name, kw in (("no book", {}), ("book", dict(openings=book))):
        arena = C4Arena(slots, 800, batch_size=32, seed=7, net_a=nets[0], net_b=nets[1], eval_cache=1 << 20,
                        eval_merge=True, **kw)
        res = arena.play(total)
        b = arena.last_batch
        moves, games = b.moves.cpu().tolist(), b.games.cpu().tolist()
        lines = {tuple(moves[o:o + n]) for _, _, _, o, n in games}
        with_opening = {(tuple(b.rows[o].cpu().tolist()), tuple(moves[o:o + n])) for _, _, _, o, n in games}
        st = arena.eval_cache_stats()
        print(f"{name:8s} distinct move sequences {len(lines):4d}   distinct (opening, moves) {len(with_opening):4d}   "
              f"score {res.score:.4f} {res.first} {res.second}   probed {st['probed']}  hit rate "
              f"{st['hits'] / st['probed']:.4f}  merged {st['merged'] / st['probed']:.4f}  steps {arena.steps}")
        arena.close()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's library (arm p; omitted: the other arms only)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--games", default="c4,chess")
    ap.add_argument("--parts", default="kernel,buys,steps", help="which of the three reports to run")
    ap.add_argument("--serve", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args.serve, args.steps)
        return
    import torch  # noqa: F401  (before the library loads: it shares torch's HIP runtime)
    from zeroclone_amd import _native
    print(f"# tools/ab_openings.py --steps {args.steps} --rounds {args.rounds}"
          + (" --parent-lib <library of the parent commit>" if args.parent_lib else "")
          + f"; library: {_native.lib().zc_version().decode()}", flush=True)
    parts = args.parts.split(",")
    if "kernel" in parts:
        kernel_alone()
    if "buys" in parts:
        what_the_book_buys()
    for game in args.games.split(",") if "steps" in parts else ():
        run_game(game, args)


if __name__ == "__main__":
    main()
