"""How often the walk's fp32 UCT decision needs its fp64 fallback, on the bench pool's search
(4096 mixed-depth roots x 800 sims, batch 32).  Needs a counter build of the library:

    ZC_LIB=$PWD/zeroclone_amd/lib_diag_uct.so ZC_CFLAGS=-DZC_DIAG_UCT python -m zeroclone_amd.build --force
    ZC_LIB=$PWD/zeroclone_amd/lib_diag_uct.so python tools/uct_fallback_rate.py

(-DZC_DIAG_UCT puts the contested levels, those with more than one fp32 candidate, into the
stats' rollout_plies word and the levels decided in fp64 into rollout_blocks.)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401
from zeroclone_amd import _native  # noqa: E402
from rollout_stats import mixed_roots  # noqa: E402

if __name__ == "__main__":
    G, sims, bs = 4096, 800, 32
    eng = _native.NativeEngine(max_games=G, max_sims=sims, max_batch=bs)
    eng.seed(0, list(range(G)))
    for c in (1.4, 50.0):
        mv, na, st = eng.c4_search(mixed_roots(G), sims, c, bs)
        flushes = G * ((sims + bs - 1) // bs)
        contested, fell = int(st["rollout_plies"].sum()), int(st["rollout_blocks"].sum())
        print(f"c = {c}: {contested / flushes:.2f} contested levels per flush, {fell} of {contested} decided in fp64 "
              f"({100.0 * fell / max(contested, 1):.3f} %)")
