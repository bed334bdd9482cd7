#!/usr/bin/env python3
"""Golden get_move outputs from the reference at the engine's declared limits: batch sizes up
to 512 (256 for the crude chess search) and 65533 simulations, where node ids pass 15 bits.

Runs ONLY in the build container, like gen_golden.py and gen_golden_chess_search.py, whose
loaders, tagging proxies and recording values it uses: the reference's compiled mcts.get_move
(oracle/_ref) drives the reference's own Python backends and value / policy functions, loaded
by path.  Nothing of the reference is copied.

Output: c4_get_move_limits.json and chess_get_move_limits.json (data only), with the fields
of c4_get_move.json and chess_get_move.json.
Usage: make -C oracle ref && python tests/golden/gen_golden_limits.py [workers]
"""
import json
import os
import random
import sys
import time
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import gen_golden_chess as GC  # noqa: E402
import gen_golden_chess_search as GS  # noqa: E402

TOP = 65533   # zc_engine_create's largest max_sims: node ids are uint16 and 0xFFFF means "none"


def consumed_since(seed, after_state):
    """Exact number of 32-bit words random.seed(seed) has produced by `after_state`, a 624-word
    block at a time: gen_golden.consumed_since one word at a time takes minutes over the
    millions of words a 65533-simulation rollout search draws."""
    words, index = after_state[1][:624], after_state[1][624]
    r = random.Random(seed)
    n = 0
    while n < 1 << 32:
        st = r.getstate()[1]
        if st[:624] == words and st[624] <= index:
            return n + index - st[624]
        k = 624 - st[624] + 1        # the rest of this block and the first word of the next
        r.getrandbits(32 * k)
        n += k
    raise RuntimeError("consumption not found")


_ctx = {}


def _c4_case(job):
    board, turn, seed, sims, bs = job
    if "c4" not in _ctx:
        _ctx["c4"] = G.load_reference()
    mcts, c4, vf, pf = _ctx["c4"]
    t0 = time.time()
    st = c4.create_init_state()._replace(board=G.dec(board), turn=turn)
    rec = G.RecordingValue(vf.Value("random_rollout"))
    random.seed(seed)
    mv = mcts.get_move(G.TState(st.board, st.turn, None), rec, pf.Policy("random"), G.TagBackend(c4), sims, 1.4, bs)
    after = random.getstate()
    order = [m[0] for m in list(c4.get_legal_moves(st))]
    return {"board": board, "turn": turn, "seed": seed, "sims": sims, "bs": bs, "c": 1.4, "move": mv[0],
            "order": order, "root_na": [rec.counts[col] for col in order], "leaves": rec.leaves,
            "consumed": consumed_since(seed, after), "next_word": random.getrandbits(32)}, time.time() - t0


def _chess_case(job):
    fen, seed, sims, bs = job
    if "chess" not in _ctx:
        _ctx["chess"] = (G.load_reference(), GC.load_ref())
    (mcts, _, vf, pf), cb = _ctx["chess"]
    t0 = time.time()
    st = cb.state_from_fen(fen)
    rec = GS.Recording(vf.Value("crude_chess_score"))
    random.seed(seed)
    mv = mcts.get_move(GS.Tagged(st, None), rec, pf.Policy("immediate_value", policy_freedom=3), GS.TagChess(cb),
                       sims, 1.4, bs)
    after = random.getstate()
    root_moves = cb.get_legal_moves(st)
    return {"fen": fen, "seed": seed, "sims": sims, "bs": bs, "c": 1.4, "policy": "immediate_value", "freedom": 3,
            "move": list(mv[0]) + [mv[1]], "root_moves": [list(m[0]) + [m[1]] for m in root_moves],
            "root_na": [rec.counts.get(tuple(m[0]), 0) for m in root_moves], "leaves": rec.leaves,
            "consumed": consumed_since(seed, after), "next_word": random.getrandbits(32)}, time.time() - t0


def main():
    workers = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    _, c4, _, _ = G.load_reference()
    for seed in (3, 4):   # the block counter against the word-by-word one
        r = random.Random(seed)
        r.getrandbits(32 * (700 * seed + 5))
        assert consumed_since(seed, r.getstate()) == G.consumed_since(seed, r.getstate()) == 700 * seed + 5

    init = c4.create_init_state()
    mids = G.random_positions(c4, 2, random.Random(2718), 6, 14)
    deep = G.random_positions(c4, 1, random.Random(31), 30, 36)[0]
    c4_jobs, seed = [], 4000
    for sims, bs in ((1100, 128), (1100, 314), (1100, 315), (1100, 512), (TOP, 32), (TOP, 512)):
        for st in [init] + mids:
            c4_jobs.append((G.enc(st.board), st.turn, seed, sims, bs))
            seed += 1
    c4_jobs.append((G.enc(deep.board), deep.turn, seed, 1100, 512))

    fens = [GC.FENS["kiwipete"], "r1bq1rk1/pp2bppp/2n1pn2/3p4/2PP4/2N1PN2/PP2BPPP/R1BQ1RK1 w - - 0 9"]
    chess_jobs, seed = [], 5000
    for sims, bs in ((400, 129), (400, 256), (TOP, 64), (TOP, 256)):
        for fen in fens:
            chess_jobs.append((fen, seed, sims, bs))
            seed += 1

    meta = {"generator": "tests/golden/gen_golden_limits.py", "python": sys.version.split()[0]}
    # the longest cases first, so that the pool's tail is short
    with ProcessPoolExecutor(workers) as ex:
        for name, fn, jobs in (("c4_get_move_limits.json", _c4_case, c4_jobs),
                               ("chess_get_move_limits.json", _chess_case, chess_jobs)):
            idx = sorted(range(len(jobs)), key=lambda i: -jobs[i][-2])
            out = [None] * len(jobs)
            for i, (case, dt) in zip(idx, ex.map(fn, [jobs[i] for i in idx])):
                out[i] = case
                print(f"{name}: sims {case['sims']} bs {case['bs']} seed {case['seed']}: {dt:.1f}s, "
                      f"{case['consumed']} words", flush=True)
            json.dump({"meta": meta, "cases": out}, open(os.path.join(HERE, name), "w"))


if __name__ == "__main__":
    main()
