"""The Connect4 walk's fp32 UCT decision as an executable specification, and the float64
reference it has to agree with (c4_search.hip uct_select8).

A node is 8 slots of (valid, Na, Wa) and its N; every valid slot is visited (Na >= 1: the
unvisited-slot rule is taken before any score is formed).  The reference is the first maximum in
slot order of U_k = fma(c, sqrt(log N / Na_k), Wa_k / Na_k) in float64, the fma with ONE rounding
(mcts.cpp:41-58 as compiled); numpy has no fma, so scores that the two-rounding form puts within
a few ulps of the maximum are formed again exactly, with rationals.
"""
import math
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24  # half an ulp of fp32


def first_order_error(c, n_max):
    """The first-order bound of |fp32 score - fp64 score| for N <= n_max (1-ulp rcp and sqrt)."""
    return U32 * (6.0 * abs(c) * math.sqrt(math.log(max(n_max, 2))) + 4.0)


def delta(c, n_max):
    """zc_internal.h uct_fast_delta: 2 E, E = twice the first-order bound, rounded up to fp32."""
    if not math.isfinite(c) or not np.isfinite(np.float32(c)):
        return np.float32(np.inf)
    with np.errstate(over="ignore"):
        return np.float32(2.0 * (2.0 * first_order_error(c, n_max)) * (1.0 + 2.0 ** -22))


def _fma_exact(c, s, q):
    return float(Fraction(c) * Fraction(s) + Fraction(q))  # float(Fraction) rounds to nearest even


def reference_argmax(valid, na, wa, big_n, c):
    """float64 first-argmax per node ([n, 8] arrays, big_n [n]); -1 where no slot is valid."""
    valid = np.asarray(valid, bool)
    na = np.asarray(na, np.int64)
    wa = np.asarray(wa, np.int64)
    lg = np.log(np.asarray(big_n, np.float64))[:, None]  # glibc log, as the engine's table
    nad = np.where(valid, na, 1).astype(np.float64)
    s = np.sqrt(lg / nad)
    q = np.where(valid, wa, 0).astype(np.float64) / nad
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.where(valid, c * s + q, -np.inf)
    best = np.where(valid.any(1), np.argmax(u, 1), -1)
    if not math.isfinite(c):
        return best.astype(np.int32)  # every score is +inf: the first valid slot
    # nodes where another DISTINCT pair comes within a few ulps of the maximum: exact fma
    m = u.max(1, keepdims=True)
    near = valid & (u >= m - 8.0 * np.spacing(np.abs(m)))
    bna = np.take_along_axis(na, np.maximum(best, 0)[:, None], 1)
    bwa = np.take_along_axis(wa, np.maximum(best, 0)[:, None], 1)
    redo = np.nonzero((near & ((na != bna) | (wa != bwa))).any(1))[0]
    for i in redo:
        top, arg = -math.inf, -1
        for k in np.nonzero(near[i])[0]:
            v = _fma_exact(float(c), float(s[i, k]), float(q[i, k]))
            if v > top:
                top, arg = v, int(k)
        best[i] = arg
    return best.astype(np.int32)


def fp32_scores(valid, na, wa, big_n, c):
    """S_k as the kernel forms it, with numpy's correctly rounded reciprocal and square root."""
    f = np.float32
    lgf = np.log(np.asarray(big_n, np.float64)).astype(f)[:, None]
    r = f(1.0) / np.where(valid, na, 1).astype(f)
    s = np.sqrt(lgf * r)
    q = np.where(valid, wa, 0).astype(f) * r
    with np.errstate(invalid="ignore", over="ignore"):
        # fmaf: the product of two fp32 values is exact in float64
        return (np.float64(f(c)) * s.astype(np.float64) + q.astype(np.float64)).astype(f)


def select(valid, na, wa, big_n, c, dlt, scores=None):
    """The decision procedure.  Returns (slot [n], how [n]); how = 0 one candidate, 1 a tie of
    equal (Na, Wa) pairs, 2 fallback (the slot is then the float64 reference's); -1 / 0 where no
    slot is valid.  scores: fp32 scores to decide from instead of fp32_scores()."""
    valid = np.asarray(valid, bool)
    na = np.asarray(na, np.int64)
    wa = np.asarray(wa, np.int64)
    S = fp32_scores(valid, na, wa, big_n, c) if scores is None else np.asarray(scores, np.float32)
    Sv = np.where(valid, S, np.float32(-np.inf))
    with np.errstate(invalid="ignore"):
        m = np.fmax.reduce(Sv, 1)[:, None]  # fmax: a NaN gives way, as v_max_f32
        thr = (m - np.float32(dlt)).astype(np.float32)
        C = valid & ~(Sv < thr)
    first = np.argmax(C, 1)
    cnt = C.sum(1)
    fna = np.take_along_axis(na, first[:, None], 1)
    fwa = np.take_along_axis(wa, first[:, None], 1)
    equal = ~(C & ((na != fna) | (wa != fwa))).any(1)
    how = np.where(cnt <= 1, 0, np.where(equal, 1, 2)).astype(np.int32)
    slot = first.astype(np.int32)
    fb = np.nonzero(how == 2)[0]
    if len(fb):
        slot[fb] = reference_argmax(valid[fb], na[fb], wa[fb], np.asarray(big_n)[fb], c)
    none = ~valid.any(1)
    slot[none], how[none] = -1, 0
    return slot, how


# ------------------------------------------------------------------ node sets
def tie_patterns(big_n, na0, wa0):
    """Every non-empty set of valid slots, all holding the same pair; then, with all 8 slots
    valid, every non-empty set of slots tied at the top over clearly worse ones."""
    masks = np.arange(1, 256)
    bits = ((masks[:, None] >> np.arange(8)) & 1).astype(bool)
    n = len(masks)
    valid = np.concatenate([bits, np.ones((n, 8), bool)])
    na = np.full((2 * n, 8), na0, np.int64)
    wa = np.full((2 * n, 8), wa0, np.int64)
    wa[n:][~bits] = -na0  # the worst value an edge can have
    return valid, na, wa, np.full(2 * n, big_n, np.int64)


def unit_neighbours(big_n, rng, count):
    """Two to eight children whose pairs differ by one unit of Wa or of Na from the first one."""
    na0 = rng.integers(1, max(2, big_n // 2), count)
    wa0 = rng.integers(-na0, na0 + 1)
    kids = rng.integers(2, 9, count)
    valid = np.arange(8)[None, :] < kids[:, None]
    valid = np.take_along_axis(valid, rng.permuted(np.tile(np.arange(8), (count, 1)), axis=1), 1)
    dna = rng.integers(-1, 2, (count, 8))
    dwa = rng.integers(-1, 2, (count, 8))
    na = np.clip(na0[:, None] + dna, 1, max(1, big_n - 1))
    wa = np.clip(wa0[:, None] + dwa, -na, na)
    return valid, na, wa, np.full(count, big_n, np.int64)


def random_nodes(big_n, rng, count, kids=None):
    """Random children: visit counts that share N - 1 unevenly, values anywhere in [-Na, Na];
    half of the nodes get near-equal children (the search's steady state: UCT keeps them close)."""
    k = rng.integers(1, 9, count) if kids is None else np.full(count, kids)
    valid = np.arange(8)[None, :] < k[:, None]
    valid = np.take_along_axis(valid, rng.permuted(np.tile(np.arange(8), (count, 1)), axis=1), 1)
    share = rng.dirichlet(np.ones(8), count)
    even = rng.random(count) < 0.5
    share[even] = 1.0 / 8 + (share[even] - 1.0 / 8) * 0.02
    na = np.clip((share * (big_n - 1)).astype(np.int64), 1, max(1, big_n - 1))
    mean = rng.uniform(-1, 1, (count, 1))
    spread = np.where(even, 0.02, 1.0)[:, None]
    wa = np.rint(np.clip(mean + spread * rng.uniform(-1, 1, (count, 8)), -1, 1) * na).astype(np.int64)
    return valid, na, wa, np.full(count, big_n, np.int64)


def child_words(valid):
    """The records' child words: a node id where the slot is valid, 0xFFFF where it is not."""
    return np.where(valid, np.arange(8, dtype=np.uint16)[None, :] + 1, 0xFFFF).astype(np.uint16)
