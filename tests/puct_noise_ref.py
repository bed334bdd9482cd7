"""Plain-numpy specification of the two random steps of the PUCT searches (chess_puct.hip,
c4_puct.hip, puct_common.h): the Dirichlet noise mixed into the root priors and the move
sampled in proportion to N^(1/T).  Everything else in those searches is specified by
oracle/puct_ref.py.  Test infrastructure only.

Counters (Philox4x32-10, key = (seed & 2^32-1, seed >> 32)):

    noise   (j, attempt | sno << 6, game, 0x6A09E667)   j = the move's index in list order,
                                                        attempt = 0..63 of the rejection loop
    sample  (game, 0x5BE0CD19, sno, 0)                  word x alone is used

`game` is the engine's game index (first_game + the row of the call), `sno` the game's search
number (ChessPuctSearch.search_no / C4PuctSearch.search_no before the search).

Uniforms: u01(x) = fl32(fl32(x >> 8) + 0.5) * 2^-24.  The fp32 sum is the definition: below
2^23 it is the exact (x >> 8) + 0.5, from 2^23 on fp32 has no halves and the sum rounds to
even, so u01 lies in (0, 1] and both precisions of this file start from the same uniforms.

gamma_draw restates puct_common.h's gamma_draw word for word (Marsaglia-Tsang; alpha < 1 by
Gamma(alpha + 1) * U^(1/alpha)) in float64 — the specification — and in float32 — the
rounding floor a float32 implementation is expected to reach.  softmax / root_prior restate
the backup kernels' prior arithmetic, their wave reductions included (wave_sum).

sample_index: weights w_j = (N_j * 2^-k)^(1/T) in float64, k = the bit length of the largest
count, 1/T = 1 / float64(float32(T)); target = u01(x) * sum(w), the sum taken in list order;
the move is the first j whose running sum exceeds the target, the last move if none does.
The power of two keeps integer 1/T exact and the base below 1, so no T overflows.
"""
import numpy as np

from c4_philox_ref import M32, philox4x32_10

NOISE_TAG = 0x6A09E667
SAMPLE_TAG = 0x5BE0CD19
LANES, CHUNKS = 64, 4   # a wave; the chess kernels hold move q * 64 + lane in register q


def _key(seed):
    return int(seed) & M32, (int(seed) >> 32) & M32


def philox(c0, c1, c2, c3, seed):
    """philox4x32_10 of c4_philox_ref on broadcast uint64 arrays of 32-bit words."""
    ctr = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & np.uint64(M32) for c in (c0, c1, c2, c3)))
    return philox4x32_10(tuple(ctr), _key(seed))


def u01(x, dtype=np.float64):
    x = np.asarray(x, dtype=np.uint64) >> np.uint64(8)
    u = (x.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    return u.astype(dtype)


def cospi(x):
    """cos(pi x) for x in [0, 2]: evaluated in float64 about the nearest multiple of 1/2, then
    rounded to x's type (float32: a correctly rounded cospif but for float64's own error)."""
    x64 = x.astype(np.float64)
    n = np.rint(2.0 * x64)
    r = (x64 - 0.5 * n) * np.pi
    q = n.astype(np.int64) & 3
    c, s = np.cos(r), np.sin(r)
    return np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s))).astype(x.dtype)


def gamma_draw(alpha, seed, game, j, sno, dtype=np.float64, boost=True):
    """Gamma(alpha, 1) draws of (game, j) in search sno, broadcast over the three; returns
    (draws, margins).  A draw's margin is the smallest |log u - (z^2/2 + d - d v + d log v)|
    over the attempts it made, |1 + c z| for an attempt where that is not positive: how far
    the draw was from taking another branch.  boost=False leaves out the U^(1/alpha) factor
    (a deliberately wrong generator for the mutation checks)."""
    f = np.dtype(dtype).type
    game, j, sno = np.broadcast_arrays(*(np.asarray(x, dtype=np.uint64) for x in (game, j, sno)))
    shape = game.shape
    game, j, sno = game.ravel(), j.ravel(), sno.ravel()
    alpha = f(np.float32(alpha))   # the kernels take alpha as a float
    boosted = bool(alpha < f(1))
    a = alpha + f(1) if boosted else alpha
    d = a - f(1) / f(3)
    cc = f(1) / np.sqrt(f(9) * d)
    inv_alpha = f(1) / alpha
    g = np.zeros(game.size, dtype)
    margin = np.full(game.size, np.inf)
    todo = np.arange(game.size)
    for att in range(64):
        if todo.size == 0:
            break
        r = philox(j[todo], np.uint64(att) | (sno[todo] << np.uint64(6)), game[todo], NOISE_TAG, seed)
        u1, u2, u, u4 = (u01(w, dtype) for w in r)
        z = np.sqrt(f(-2) * np.log(u1)) * cospi(f(2) * u2)   # Box-Muller
        v1 = f(1) + cc * z
        pos = v1 > 0
        v = v1 * v1 * v1
        with np.errstate(invalid="ignore", divide="ignore"):
            rhs = f(0.5) * z * z + d - d * v + d * np.log(v)
            lhs = np.log(u)
            acc = pos & (lhs < rhs)
            m = np.where(pos, np.abs(lhs.astype(np.float64) - rhs.astype(np.float64)), np.abs(v1.astype(np.float64)))
        margin[todo] = np.minimum(margin[todo], m)
        gg = d * v
        if boosted and boost:
            gg = gg * np.power(u4, inv_alpha)
        g[todo[acc]] = gg[acc]
        todo = todo[~acc]
    return g.reshape(shape), margin.reshape(shape)


def wave_sum(x):
    """The kernels' sum over a move list: x [..., 256], move q * 64 + lane; each lane adds its
    four registers in order, then the wave adds across lanes by xor-shuffles 32, 16, .. 1."""
    s = x[..., 0:LANES]
    for q in range(1, CHUNKS):
        s = s + x[..., q * LANES:(q + 1) * LANES]
    lane = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    return s[..., 0]


def _pad(x, nm, fill):
    """[G, K] -> [G, 256] with `fill` from each game's nm on."""
    out = np.full((x.shape[0], LANES * CHUNKS), fill, dtype=x.dtype)
    out[:, :x.shape[1]] = x
    out[np.arange(LANES * CHUNKS)[None, :] >= np.asarray(nm)[:, None]] = fill
    return out


def softmax(logits, nm, dtype=np.float64):
    """Priors of each game's first nm[g] moves from their logits [G, K]: exp(l - max) / sum."""
    lg = _pad(np.asarray(logits).astype(dtype), nm, -np.inf)
    mx = lg.max(axis=1, keepdims=True)
    e = np.exp(lg - mx)   # exp(-inf) = 0 past the list
    return (e / wave_sum(e)[:, None])[:, :np.asarray(logits).shape[1]]


def root_prior(sm, alpha, eps, seed, game, nm, sno, dtype=np.float64, boost=True):
    """(1 - eps) * sm + eps * g / sum(g) for sm [G, K] (softmax above, or a kept root's priors),
    game / nm / sno [G]; returns (prior [G, K], margin [G] = the smallest margin among the
    game's draws)."""
    f = np.dtype(dtype).type
    game, nm, sno = (np.asarray(x) for x in (game, nm, sno))
    G, K = sm.shape
    j = np.arange(K)
    g, margin = gamma_draw(alpha, seed, game[:, None], j[None, :], sno[:, None], dtype, boost)
    valid = j[None, :] < nm[:, None]
    g = np.where(valid, g, f(0))
    gs = wave_sum(_pad(g, nm, f(0)))[:, None]
    eps = f(np.float32(eps))
    with np.errstate(invalid="ignore", divide="ignore"):
        noise = np.where(gs > 0, g / gs, f(0))
    prior = (f(1) - eps) * sm.astype(dtype) + eps * noise
    return np.where(valid, prior, f(0)), np.where(valid, margin, np.inf).min(axis=1)


def sample_u(seed, game, sno):
    """The temperature sample's uniform of (game, sno)."""
    return u01(philox(game, SAMPLE_TAG, sno, 0, seed)[0])


def sample_weights(na, T):
    na = np.asarray(na)
    top = na.max(axis=-1, keepdims=True)
    k = np.frexp(top.astype(np.float64))[1]   # bit length (0 for 0)
    inv_t = 1.0 / np.float64(np.float32(T))
    return np.power(np.ldexp(na.astype(np.float64), -k), inv_t)


def sample_index(na, T, seed, game, sno):
    """The sampled move of each (game, sno) for visit counts na [..., nm] in list order;
    returns (index, distance from the target to the nearest running sum over the total)."""
    w = np.broadcast_to(sample_weights(na, T), np.broadcast_shapes(np.shape(na)[:-1], np.shape(game),
                                                                   np.shape(sno)) + np.shape(na)[-1:])
    run = np.cumsum(w, axis=-1)
    tot = run[..., -1]
    target = sample_u(seed, game, sno) * tot
    over = run > target[..., None]
    idx = np.where(over.any(axis=-1), over.argmax(axis=-1), w.shape[-1] - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.abs(run - target[..., None]).min(axis=-1) / tot
    return idx, dist
