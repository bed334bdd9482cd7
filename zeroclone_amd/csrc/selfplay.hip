// selfplay.hip — device-resident self-play trajectories.
//
// Replaces the host side of the reference's self-play data path:
//   Engine.play_move's history append (engine/engine.py:98-108),
//   Engine.get_dataset (engine.py:60-89): each finished game's positions with side-to-move
//     labels — factor 0 (draw) or -1, alternating in sign, the game's list REVERSED, so
//     position i of an n-position game gets f * (-1)^(n-1-i),
//   scripts/train.py:simulate_games (:151-170): a finished game's slot starts a new game only
//     while fewer than the quota have started; every started game is played to its end.
//
// One thread per game slot.  Each slot keeps its current game's positions (opening first) in
// HBM; when the game ends the slot takes its place in the pool (prefix sums over the slots,
// so the layout is deterministic) and copies the game out — positions, labels, the move
// played from each position, and one game record — then restarts from the opening (or goes
// idle when the quota is spent).  Rows are
// opaque byte records (zc_c4_state: 24 B, zc_chess_state: 72 B), copied 8 bytes at a time.
#include "zc_internal.h"

#include <hip/hip_fp16.h>

namespace zc {
namespace {

constexpr int kRecThreads = 1024;

// Exclusive prefix sums over the workgroup of two counters at once (x: games, y: positions);
// returns the workgroup totals in tx / ty.
__device__ __forceinline__ void block_scan2(int &x, long long &y, int &tx, long long &ty) {
    __shared__ int s_x[kRecThreads / 64];
    __shared__ long long s_y[kRecThreads / 64];
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    int ix = x;
    long long iy = y;
    for (int o = 1; o < 64; o <<= 1) {
        const int ux = __shfl_up(ix, o);
        const long long uy = __shfl_up(iy, o);
        if (lane >= o) {
            ix += ux;
            iy += uy;
        }
    }
    if (lane == 63) {
        s_x[wv] = ix;
        s_y[wv] = iy;
    }
    __syncthreads();
    int bx = 0;
    long long by = 0;
    tx = 0;
    ty = 0;
    for (int w = 0; w < kRecThreads / 64; ++w) {
        if (w < wv) {
            bx += s_x[w];
            by += s_y[w];
        }
        tx += s_x[w];
        ty += s_y[w];
    }
    x = bx + ix - x;
    y = by + iy - y;
    __syncthreads();
}

// Pass 1 — one workgroup walks the slots 1024 at a time, so games that end in the same step
// get their game numbers and pool places in slot order (deterministic; the reference refills
// in the order its finished games are listed, train.py:160-167).  Per slot: the result, the
// append, and for a finished game its game record, its pool place (slot[2]) and length
// (slot[3], 0 = nothing to copy), the refill of the slot.  The copy is pass 2.
__global__ __launch_bounds__(kRecThreads) void traj_record_kernel(int n, zc_traj_buffers b, uint8_t *states,
                                                                  const int16_t *moves, int32_t *results,
                                                                  const int32_t *flags, const int32_t *rep) {
    const int W = b.row_bytes / 8;
    const uint64_t *init = (const uint64_t *)b.d_init;
    long long pos_base = b.d_ctl[kTrajPositions], game_base = b.d_ctl[kTrajGames], next = b.d_ctl[kTrajNext];
    long long finished = b.d_ctl[kTrajFinished];
    const long long quota = b.d_ctl[kTrajQuota];
    int overflow = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += kRecThreads) {
        const int g = c0 + (int)threadIdx.x;
        int fin = 0, len = 0, r = ZC_C4_ONGOING, game = -1;
        int32_t *slot = b.d_slot + 4 * (size_t)(g < n ? g : 0);
        uint64_t *row = (uint64_t *)(states + (size_t)(g < n ? g : 0) * b.row_bytes);
        if (g < n) {
            game = slot[1];
            if (game >= 0 && !flags && results[g] == ZC_SLOT_SKIP) {
                game = -2;  // pooled self-play: no move on this slot at this step, left as it is
                slot[3] = 0;
            } else if (game < 0) {  // idle slot (quota spent): held at the opening, nothing recorded
                for (int k = 0; k < W; ++k) row[k] = init[k];
                results[g] = ZC_SLOT_IDLE;
                slot[3] = 0;
            } else {
                if (flags) {
                    // chess: Engine._evaluate (engine.py:148-153) of the position after the
                    // move — check_win -> turn*2-1 (turn = side to move now), check_draw -> 0
                    // (stalemate, the fifty-move rule, or both sides' histories repeating)
                    const int turn = ((const uint8_t *)row)[64];
                    const int f = flags[g];
                    if (f & ZC_CHESS_WIN) r = turn * 2 - 1;
                    else if ((f & (ZC_CHESS_STALEMATE | ZC_CHESS_FIFTY)) || (rep && rep[g] == 3)) r = 0;
                    results[g] = r;
                } else {
                    r = results[g];
                }
                len = slot[0];
                if (len >= b.max_len) {  // longer than the slot holds: flagged
                    overflow |= 2;
                    len = b.max_len - 1;
                }
                uint64_t *hist = (uint64_t *)b.d_hist + ((size_t)g * b.max_len + len) * W;
                for (int k = 0; k < W; ++k) hist[k] = row[k];
                b.d_hmoves[(size_t)g * b.max_len + len - 1] = moves[g];
                ++len;
                fin = r != ZC_C4_ONGOING;
            }
        }
        int gi = fin;
        long long off = fin ? len : 0;
        int tg;
        long long tp;
        block_scan2(gi, off, tg, tp);
        if (g < n && game >= 0) {
            int copy = 0;
            if (fin) {
                const long long G = game_base + gi, P = pos_base + off;
                if (P + len > b.pool_cap || G >= b.games_cap) {  // dropped: no pass-2 copy
                    overflow |= 1;
                    uint64_t *h0 = (uint64_t *)b.d_hist + (size_t)g * b.max_len * W;
                    for (int k = 0; k < W; ++k) h0[k] = init[k];
                } else {
                    int64_t *rec = b.d_games + 4 * (size_t)G;
                    rec[0] = game;
                    rec[1] = ((int64_t)g << 32) | (uint32_t)(r + 1);  // slot | result + 1
                    rec[2] = P;
                    rec[3] = len;
                    slot[2] = (int32_t)P;
                    copy = len;
                }
                // the refill (train.py:165-167): a new game while fewer than `quota` started
                const long long nx = next + gi;
                slot[1] = nx < quota ? (int)nx : -1;
                for (int k = 0; k < W; ++k) row[k] = init[k];
                len = 1;
            }
            slot[0] = len;
            slot[3] = copy | (r == 0 ? 0 : (int)0x80000000);  // length to copy; bit 31: decisive
        }
        pos_base += tp;
        game_base += tg;
        next += tg;
        finished += tg;
    }
    const int ov = (__syncthreads_or(overflow & 1) ? 1 : 0) | (__syncthreads_or(overflow & 2) ? 2 : 0);
    if (threadIdx.x == 0) {
        b.d_ctl[kTrajPositions] = pos_base;
        b.d_ctl[kTrajGames] = game_base;
        b.d_ctl[kTrajNext] = next;
        b.d_ctl[kTrajFinished] = finished;
        b.d_ctl[kTrajOverflow] |= ov;
    }
}

// Pass 2 — one thread per (slot, position): a finished game's positions, labels and moves
// to its pool place (get_dataset: position i of n gets f * (-1)^(n-1-i), f = 0 for a draw,
// -1 otherwise); position 0's thread then restarts the slot's history at the opening.
__global__ void traj_copy_kernel(int n, zc_traj_buffers b) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int g = (int)(t / b.max_len), i = (int)(t % b.max_len);
    if (g >= n) return;
    const int32_t *slot = b.d_slot + 4 * (size_t)g;
    const int s3 = slot[3];
    const int len = s3 & 0x7FFFFFFF;
    if (i >= len) return;
    const int W = b.row_bytes / 8;
    const long long P = slot[2] + (long long)i;
    uint64_t *hist = (uint64_t *)b.d_hist + ((size_t)g * b.max_len + i) * W;
    uint64_t *pool = (uint64_t *)b.d_pool + (size_t)P * W;
    for (int k = 0; k < W; ++k) pool[k] = hist[k];
    const int f0 = s3 < 0 ? -1 : 0;
    b.d_labels[P] = ((len - 1 - i) & 1) ? -f0 : f0;
    b.d_pool_moves[P] = i + 1 < len ? b.d_hmoves[(size_t)g * b.max_len + i] : (int16_t)-1;
    if (i == 0) {
        const uint64_t *init = (const uint64_t *)b.d_init;
        for (int k = 0; k < W; ++k) hist[k] = init[k];
    }
}

// ---------------------------------------------------------------- multi-step record
// The K steps of one self-play launch recorded at once.  Single steps number the games that
// finish in step k after every game of steps < k, in slot order inside a step, and give each
// its pool place in the same order; so a game's number and place are exclusive prefix sums
// over the [K][n] grid in step-major order — of 1 per finished game and of its length.
// Kernels: (A) one wave per slot, lane = step: the finished games' lengths fl[k][n] (and the
// slot's moves played); (B) one workgroup per step: the scan of its row; (C) one workgroup:
// the scan of the row totals, the counters' bases and their update; (D) one wave per slot:
// each finished game's record and positions, labels and moves to its pool place, then the
// unfinished game's new positions appended to the slot's history.
struct StepScratch {
    int32_t *fl, *exg, *exp, *played;   // [K][n], [K][n], [K][n], [n]
    int64_t *rowtot, *rowpre, *base;    // [K][2], [K][2], [4]
};

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

__host__ __device__ inline size_t steps_scratch_layout(int n, int K, uint8_t *p, StepScratch *sc) {
    size_t o = 0;
    const size_t kn = (size_t)K * n * sizeof(int32_t);
    if (sc) sc->fl = (int32_t *)(p + o);
    o = align16(o + kn);
    if (sc) sc->exg = (int32_t *)(p + o);
    o = align16(o + kn);
    if (sc) sc->exp = (int32_t *)(p + o);
    o = align16(o + kn);
    if (sc) sc->played = (int32_t *)(p + o);
    o = align16(o + (size_t)n * sizeof(int32_t));
    if (sc) sc->rowtot = (int64_t *)(p + o);
    o = align16(o + (size_t)K * 2 * sizeof(int64_t));
    if (sc) sc->rowpre = (int64_t *)(p + o);
    o = align16(o + (size_t)K * 2 * sizeof(int64_t));
    if (sc) sc->base = (int64_t *)(p + o);
    return o + 4 * sizeof(int64_t);
}

__device__ __forceinline__ int steps_reached(int K, const int32_t *reached) {
    return reached ? min(K, max(*reached, 0)) : K;
}

constexpr int kSlotWaves = 4;

// (A) lane = step.  A slot's moves are the steps before its first ZC_SLOT_SKIP; a game that
// ends at step k has the positions since the previous finish (opening included) or, for the
// slot's game in progress at the launch's start, its history plus steps 0..k.  Returns the
// slot's moves played (also left in sc.played[g]).
__device__ __forceinline__ int steps_lens(int n, int K, const int32_t *reached, const int32_t *slot,
                                          const int32_t *results, const StepScratch &sc, int g, int lane) {
    const int Kr = steps_reached(K, reached);
    int lenc = slot[4 * (size_t)g];
    bool stopped = slot[4 * (size_t)g + 1] < 0;  // idle slot: nothing recorded
    int m = 0;
    for (int c0 = 0; c0 < Kr; c0 += 64) {
        const int k = c0 + lane;
        const bool valid = k < Kr;
        const int r = (valid && !stopped) ? results[(size_t)k * n + g] : ZC_SLOT_SKIP;
        const unsigned long long skip = __ballot(r == ZC_SLOT_SKIP);
        const int first_skip = skip ? __ffsll((long long)skip) - 1 : 64;
        const unsigned long long played = first_skip == 64 ? ~0ull : ((1ull << first_skip) - 1);
        const unsigned long long fin = __ballot(r != ZC_C4_ONGOING && r != ZC_SLOT_SKIP) & played;
        const unsigned long long prev = fin & ((1ull << lane) - 1);
        int L = 0;
        if ((fin >> lane) & 1) L = prev ? lane - (63 - __clzll((long long)prev)) + 1 : lenc + lane + 1;
        if (valid) sc.fl[(size_t)k * n + g] = L;
        const int np = __popcll(played);
        lenc = fin ? np - (63 - __clzll((long long)fin)) : lenc + np;
        m += np;
        stopped = stopped || first_skip < 64;
    }
    if (lane == 0) sc.played[g] = m;
    return m;
}

__global__ __launch_bounds__(kSlotWaves * 64) void traj_steps_lens_kernel(int n, int K, const int32_t *reached,
                                                                          const int32_t *slot,
                                                                          const int32_t *results, StepScratch sc) {
    const int lane = (int)(threadIdx.x & 63);
    const int g = (int)(blockIdx.x * kSlotWaves + (threadIdx.x >> 6));
    if (g >= n) return;
    steps_lens(n, K, reached, slot, results, sc, g, lane);
}

// (B) one workgroup per step: exclusive prefixes of (finished, length) along the row.
__global__ __launch_bounds__(kRecThreads) void traj_steps_rows_kernel(int n, int K, const int32_t *reached,
                                                                      StepScratch sc) {
    const int k = (int)blockIdx.x;
    if (k >= steps_reached(K, reached)) return;
    const size_t row = (size_t)k * n;
    int gbase = 0;
    long long pbase = 0;
    for (int c0 = 0; c0 < n; c0 += kRecThreads) {
        const int g = c0 + (int)threadIdx.x;
        const int L = g < n ? sc.fl[row + g] : 0;
        int x = L > 0;
        long long y = L;
        int tx;
        long long ty;
        block_scan2(x, y, tx, ty);
        if (g < n) {
            sc.exg[row + g] = gbase + x;
            sc.exp[row + g] = (int32_t)(pbase + y);
        }
        gbase += tx;
        pbase += ty;
    }
    if (threadIdx.x == 0) {
        sc.rowtot[2 * k] = gbase;
        sc.rowtot[2 * k + 1] = pbase;
    }
}

// (C) one workgroup: the rows' exclusive prefixes, the counters' bases (for D) and their update.
__global__ __launch_bounds__(kRecThreads) void traj_steps_totals_kernel(int K, const int32_t *reached,
                                                                        zc_traj_buffers b, StepScratch sc) {
    const int Kr = steps_reached(K, reached);
    long long gb = 0, pb = 0;
    for (int c0 = 0; c0 < Kr; c0 += kRecThreads) {
        const int k = c0 + (int)threadIdx.x;
        int x = k < Kr ? (int)sc.rowtot[2 * k] : 0;
        long long y = k < Kr ? sc.rowtot[2 * k + 1] : 0;
        int tx;
        long long ty;
        block_scan2(x, y, tx, ty);
        if (k < Kr) {
            sc.rowpre[2 * k] = gb + x;
            sc.rowpre[2 * k + 1] = pb + y;
        }
        gb += tx;
        pb += ty;
    }
    if (threadIdx.x == 0) {
        sc.base[0] = b.d_ctl[kTrajPositions];
        sc.base[1] = b.d_ctl[kTrajGames];
        sc.base[2] = b.d_ctl[kTrajNext];
        sc.base[3] = b.d_ctl[kTrajQuota];
        b.d_ctl[kTrajPositions] += pb;
        b.d_ctl[kTrajGames] += gb;
        b.d_ctl[kTrajNext] += gb;
        b.d_ctl[kTrajFinished] += gb;
    }
}

// (D) one wave per slot.  Game `first` (in progress at the launch's start) has its first h =
// slot[0] positions in the slot's history; a later game starts at the opening (h = 1).
// Position i >= h of a game whose first step is bs came from step bs + i - h; the move from
// position i is the one that made position i + 1.
__global__ __launch_bounds__(kSlotWaves * 64) void traj_steps_copy_kernel(int n, int K, const int32_t *reached,
                                                                          zc_traj_buffers b, const uint8_t *states,
                                                                          const int16_t *moves,
                                                                          const int32_t *results, StepScratch sc) {
    const int lane = (int)(threadIdx.x & 63);
    const int g = (int)(blockIdx.x * kSlotWaves + (threadIdx.x >> 6));
    if (g >= n) return;
    int32_t *slot = b.d_slot + 4 * (size_t)g;
    int game = slot[1];
    if (game < 0) return;
    const int W = b.row_bytes / 8;
    const long long pos0 = sc.base[0], games0 = sc.base[1], next0 = sc.base[2], quota = sc.base[3];
    const uint64_t *init = (const uint64_t *)b.d_init;
    uint64_t *hist = (uint64_t *)b.d_hist + (size_t)g * b.max_len * W;
    int16_t *hmv = b.d_hmoves + (size_t)g * b.max_len;
    const int m = sc.played[g];
    int h = slot[0], bs = 0, ov = 0;
    bool first = true;
    for (int c0 = 0; c0 < m && game >= 0; c0 += 64) {
        const int k = c0 + lane;
        const int Lv = k < m ? sc.fl[(size_t)k * n + g] : 0;
        unsigned long long fin = __ballot(Lv > 0);
        while (fin && game >= 0) {
            const int j = __ffsll((long long)fin) - 1;
            fin &= fin - 1;
            const int kk = c0 + j;
            const size_t e = (size_t)kk * n + g;
            const int L = __shfl(Lv, j);
            const long long gi = sc.rowpre[2 * kk] + sc.exg[e];
            const long long G = games0 + gi, P = pos0 + sc.rowpre[2 * kk + 1] + sc.exp[e];
            const int r = results[e];
            if (L > b.max_len) ov |= 2;
            if (P + L > b.pool_cap || G >= b.games_cap) {
                ov |= 1;  // dropped
            } else {
                if (lane == 0) {
                    int64_t *rec = b.d_games + 4 * (size_t)G;
                    rec[0] = game;
                    rec[1] = ((int64_t)g << 32) | (uint32_t)(r + 1);
                    rec[2] = P;
                    rec[3] = L;
                }
                const int f0 = r == 0 ? 0 : -1;
                for (int i = lane; i < L; i += 64) {
                    const uint64_t *src = i < h ? (first ? hist + (size_t)i * W : init)
                                                : (const uint64_t *)(states + ((size_t)(bs + i - h) * n + g) * b.row_bytes);
                    uint64_t *dst = (uint64_t *)b.d_pool + (size_t)(P + i) * W;
                    for (int w = 0; w < W; ++w) dst[w] = src[w];
                    b.d_labels[P + i] = ((L - 1 - i) & 1) ? -f0 : f0;
                    b.d_pool_moves[P + i] = i + 1 >= L ? (int16_t)-1
                                            : (i + 1 < h ? hmv[i] : moves[(size_t)(bs + i + 1 - h) * n + g]);
                }
            }
            // the refill (train.py:165-167), numbered as single steps number it
            const long long nx = next0 + gi;
            if (nx < quota) {
                game = (int)nx;
            } else {
                game = -1;
                ov |= 4;
            }
            first = false;
            h = 1;
            bs = kk + 1;
        }
    }
    // the game in progress: its positions since bs appended to the history
    if (!first)
        for (int w = lane; w < W; w += 64) hist[w] = init[w];
    const int cnt = game >= 0 ? m - bs : 0;
    for (int t = lane; t < cnt; t += 64) {
        const int idx = h + t;
        if (idx >= b.max_len) {
            ov |= 2;
            continue;
        }
        const uint64_t *src = (const uint64_t *)(states + ((size_t)(bs + t) * n + g) * b.row_bytes);
        for (int w = 0; w < W; ++w) hist[(size_t)idx * W + w] = src[w];
        hmv[idx - 1] = moves[(size_t)(bs + t) * n + g];
    }
    ov = (__ballot(ov & 1) ? 1 : 0) | (__ballot(ov & 2) ? 2 : 0) | (__ballot(ov & 4) ? 4 : 0);
    if (lane == 0) {
        slot[0] = min(h + cnt, b.max_len);
        slot[1] = game;
        if (ov) atomicOr((unsigned long long *)(b.d_ctl + kTrajOverflow), (unsigned long long)ov);
    }
}

// ---------------------------------------------------------------- root visit counts
// The policy targets of the searched positions (pi(a) = N(a) / sum N), sparse: one uint32
// (move id | count << 16) per root move with Na > 0, in the root's move-list order.  Slot
// history and pool are both CSR (zc_traj_policy_buffers).
constexpr int kPiSlotFull = 1, kPiPoolFull = 2, kPiSaturated = 4;

// Append — one wave per slot, after the search and before the play: the non-zero counts of the
// slot's row, compacted by ballot + prefix popcount, become the entries of history position
// slot[0] - 1; the running offset is off[pos] -> off[pos + 1].
__global__ __launch_bounds__(kSlotWaves * 64) void traj_policy_append_kernel(int n, zc_traj_buffers b,
                                                                             zc_traj_policy_buffers q,
                                                                             const int32_t *na, const uint16_t *mv,
                                                                             int stride) {
    const int lane = (int)(threadIdx.x & 63);
    const int g = (int)(blockIdx.x * kSlotWaves + (threadIdx.x >> 6));
    if (g >= n) return;
    const int32_t *slot = b.d_slot + 4 * (size_t)g;
    if (slot[1] < 0) return;
    const int pos = slot[0] - 1;
    if (pos < 0 || pos >= b.max_len) return;  // never: slot[0] is in [1, max_len]
    int32_t *off = q.d_slot_off + (size_t)g * (b.max_len + 1);
    uint32_t *dst = q.d_slot_pi + (size_t)g * q.slot_cap;
    const int base = pos ? off[pos] : 0;
    int run = 0, ov = 0;
    for (int c0 = 0; c0 < stride; c0 += 64) {
        const int j = c0 + lane;
        const int cnt = j < stride ? na[(size_t)g * stride + j] : 0;
        const unsigned long long have = __ballot(cnt > 0);
        if (cnt > 0) {
            const long long at = (long long)base + run + __popcll(have & ((1ull << lane) - 1));
            if (cnt > 65535) ov |= kPiSaturated;
            const uint32_t id = mv ? (uint32_t)mv[(size_t)g * stride + j] : (uint32_t)j;
            if (at < q.slot_cap) dst[at] = id | ((uint32_t)min(cnt, 65535) << 16);
            else ov |= kPiSlotFull;
        }
        run += __popcll(have);
    }
    ov = (__ballot(ov & kPiSlotFull) ? kPiSlotFull : 0) | (__ballot(ov & kPiSaturated) ? kPiSaturated : 0);
    if (lane == 0) {
        off[pos + 1] = (int32_t)min((long long)base + run, (long long)q.slot_cap);
        if (ov) atomicOr((unsigned long long *)(q.d_pctl + ZC_TRAJ_PI_OVERFLOW), (unsigned long long)ov);
    }
}

// Commit pass 1 — one workgroup walks the slots 1024 at a time (as traj_record_kernel, which
// ran just before and left each pooled game's length in slot[3] and its place in slot[2]):
// the pooled games' entries get their places in the entry pool in slot order.
__global__ __launch_bounds__(kRecThreads) void traj_policy_reserve_kernel(int n, zc_traj_buffers b,
                                                                          zc_traj_policy_buffers q) {
    long long ent_base = q.d_pctl[ZC_TRAJ_PI_ENTRIES];
    int overflow = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += kRecThreads) {
        const int g = c0 + (int)threadIdx.x;
        int len = 0;
        long long cnt = 0;
        if (g < n) {
            const int32_t *slot = b.d_slot + 4 * (size_t)g;
            int32_t *off = q.d_slot_off + (size_t)g * (b.max_len + 1);
            len = min(slot[3] & 0x7FFFFFFF, b.max_len);
            if (len > 0) cnt = off[len - 1];  // positions 0 .. len-2 were searched
            if (slot[0] == 1) off[0] = 0;     // restarted: its history starts over
        }
        int x = 0, tx;
        long long y = cnt, ty;
        block_scan2(x, y, tx, ty);
        if (g < n) {
            long long at = -1;
            if (len > 0) {
                if (ent_base + y + cnt > q.pi_pool_cap) overflow = 1;  // dropped: first = count = 0
                else at = ent_base + y;
            }
            q.d_slot_base[g] = at;
        }
        ent_base += ty;
    }
    const int ov = __syncthreads_or(overflow);
    if (threadIdx.x == 0) {
        q.d_pctl[ZC_TRAJ_PI_ENTRIES] = ent_base;
        if (ov) q.d_pctl[ZC_TRAJ_PI_OVERFLOW] |= kPiPoolFull;
    }
}

// Commit pass 2 — one wave per slot: first / count of each pooled position, then the game's
// entries as one contiguous block.
__global__ __launch_bounds__(kSlotWaves * 64) void traj_policy_copy_kernel(int n, zc_traj_buffers b,
                                                                           zc_traj_policy_buffers q) {
    const int lane = (int)(threadIdx.x & 63);
    const int g = (int)(blockIdx.x * kSlotWaves + (threadIdx.x >> 6));
    if (g >= n) return;
    const int32_t *slot = b.d_slot + 4 * (size_t)g;
    const int len = min(slot[3] & 0x7FFFFFFF, b.max_len);
    if (len <= 0) return;
    const long long P = slot[2], at = q.d_slot_base[g];
    const int32_t *off = q.d_slot_off + (size_t)g * (b.max_len + 1);
    for (int i = lane; i < len; i += 64) {
        if (P + i >= b.pool_cap) break;  // never: pass 1 of the record placed the game inside
        const int o0 = i ? off[i] : 0;
        q.d_pool_first[P + i] = at < 0 ? 0 : at + o0;
        q.d_pool_count[P + i] = (at < 0 || i + 1 >= len) ? 0 : off[i + 1] - o0;
    }
    if (at < 0) return;
    const int total = min(off[len - 1], q.slot_cap);
    const uint32_t *src = q.d_slot_pi + (size_t)g * q.slot_cap;
    for (int e = lane; e < total; e += 64) q.d_pool_pi[at + e] = src[e];
}

// ---------------------------------------------------------------- multi-step policy record
// The visit counts of the K steps of one self-play launch recorded at once: what K rounds of
// (append, record, commit) leave, from the launch's staged rows na[k][g][stride] (and the root
// moves mv[k][g][stride] that name them; null: id = index).  Runs BEFORE the multi-step record of
// the same launch — it reads the slot table and the counters as the launch found them and
// changes neither.  A single commit reserves the entries of the games finished in its step in
// slot order, so a game's place in the entry pool is a third exclusive prefix sum over the
// [K][n] grid in step-major order, of the entries of each finished game the pool took.
// Kernels: (A) as above, one wave per slot, which here also counts every step's entries nnz[k][g]
// and their running sum cum[k][g] over the slot's game (from the history's fill for the game in
// progress, from 0 after a finish); (B) as above; (E) one workgroup per step: the prefix of
// the row totals before its step (no kernel C: the counters are only read), which of its
// finished games the pool drops, the scan of the others' entries along the row; (F) one wave per
// slot: each finished game's first / count per pooled position and its entries — the history's,
// then the staged rows' — to their pool place, then the unfinished game's rows appended to the
// slot's CSR.
struct PolicyStepScratch {
    StepScratch s;
    int32_t *nnz, *cum;          // [K][n]
    int64_t *exe, *rowtot_e;     // [K][n], [K]
    int64_t *ebase;              // [1] ZC_TRAJ_PI_ENTRIES before the call
};

__host__ __device__ inline size_t policy_steps_scratch_layout(int n, int K, uint8_t *p, PolicyStepScratch *sc) {
    size_t o = align16(steps_scratch_layout(n, K, p, sc ? &sc->s : nullptr));
    const size_t kn = (size_t)K * n;
    if (sc) sc->nnz = (int32_t *)(p + o);
    o = align16(o + kn * sizeof(int32_t));
    if (sc) sc->cum = (int32_t *)(p + o);
    o = align16(o + kn * sizeof(int32_t));
    if (sc) sc->exe = (int64_t *)(p + o);
    o = align16(o + kn * sizeof(int64_t));
    if (sc) sc->rowtot_e = (int64_t *)(p + o);
    o = align16(o + (size_t)K * sizeof(int64_t));
    if (sc) sc->ebase = (int64_t *)(p + o);
    return o + 2 * sizeof(int64_t);
}

// The non-zero counts of one staged row: their number (the whole wave gets it).
__device__ __forceinline__ int policy_row_nnz(const int32_t *row, int stride, int lane) {
    int run = 0;
    for (int c0 = 0; c0 < stride; c0 += 64) {
        const int j = c0 + lane;
        run += __popcll(__ballot(j < stride && row[j] > 0));
    }
    return run;
}

// One staged row compacted (as traj_policy_append_kernel compacts it) to dst[at0 ..), written
// below `cap` only; returns kPiSlotFull / kPiSaturated bits (per lane).
__device__ __forceinline__ int policy_row_emit(const int32_t *row, const uint16_t *mv, int stride, int lane,
                                               uint32_t *dst, long long at0, long long cap) {
    int run = 0, ov = 0;
    for (int c0 = 0; c0 < stride; c0 += 64) {
        const int j = c0 + lane;
        const int cnt = j < stride ? row[j] : 0;
        const unsigned long long have = __ballot(cnt > 0);
        if (cnt > 0) {
            const long long at = at0 + run + __popcll(have & ((1ull << lane) - 1));
            if (cnt > 65535) ov |= kPiSaturated;
            const uint32_t id = mv ? (uint32_t)mv[j] : (uint32_t)j;
            if (at < cap) dst[at] = id | ((uint32_t)min(cnt, 65535) << 16);
            else ov |= kPiSlotFull;
        }
        run += __popcll(have);
    }
    return ov;
}

// (A) with the entry counts: the lengths as traj_steps_lens_kernel, then step by step the rows'
// non-zero counts and their running sum over the slot's game.
__global__ __launch_bounds__(kSlotWaves * 64) void traj_policy_steps_lens_kernel(int n, int K, const int32_t *reached,
                                                                                 zc_traj_buffers b,
                                                                                 zc_traj_policy_buffers q,
                                                                                 const int32_t *results,
                                                                                 const int32_t *na, int stride,
                                                                                 PolicyStepScratch sc) {
    const int lane = (int)(threadIdx.x & 63);
    const int g = (int)(blockIdx.x * kSlotWaves + (threadIdx.x >> 6));
    if (g >= n) return;
    const int32_t *slot = b.d_slot + 4 * (size_t)g;
    const int m = steps_lens(n, K, reached, b.d_slot, results, sc.s, g, lane);
    if (g == 0 && lane == 0) sc.ebase[0] = q.d_pctl[ZC_TRAJ_PI_ENTRIES];  // (F) updates the counter
    if (slot[1] < 0) return;  // idle: m = 0
    const int h = min(max(slot[0], 1), b.max_len);
    int run = q.d_slot_off[(size_t)g * (b.max_len + 1) + h - 1];  // the entries of positions 0 .. h-2
    for (int k = 0; k < m; ++k) {
        const size_t e = (size_t)k * n + g;
        const int c = policy_row_nnz(na + e * stride, stride, lane);
        run += c;
        const int r = results[e];
        if (lane == 0) {
            sc.nnz[e] = c;
            sc.cum[e] = run;
        }
        if (r != ZC_C4_ONGOING) run = 0;  // finished: the next game starts empty
    }
}

// (E) one workgroup per step.  Threads first sum the (games, positions) totals of the rows
// before this one; then along the row each finished game the trajectory pool takes (the test of
// traj_steps_copy_kernel) contributes its entries, clamped as a slot's history clamps them.
__global__ __launch_bounds__(kRecThreads) void traj_policy_steps_rows_kernel(int n, int K, const int32_t *reached,
                                                                             zc_traj_buffers b,
                                                                             zc_traj_policy_buffers q,
                                                                             PolicyStepScratch sc) {
    const int k = (int)blockIdx.x;
    if (k >= steps_reached(K, reached)) return;
    long long gpre = 0, ppre = 0;
    for (int c0 = 0; c0 < k; c0 += kRecThreads) {
        const int kk = c0 + (int)threadIdx.x;
        int x = kk < k ? (int)sc.s.rowtot[2 * kk] : 0;
        long long y = kk < k ? sc.s.rowtot[2 * kk + 1] : 0;
        int tx;
        long long ty;
        block_scan2(x, y, tx, ty);
        gpre += tx;
        ppre += ty;
    }
    const long long pos0 = b.d_ctl[kTrajPositions] + ppre, games0 = b.d_ctl[kTrajGames] + gpre;
    const size_t row = (size_t)k * n;
    long long ebase = 0;
    for (int c0 = 0; c0 < n; c0 += kRecThreads) {
        const int g = c0 + (int)threadIdx.x;
        long long E = 0;
        if (g < n) {
            const int L = sc.s.fl[row + g];
            if (L > 0) {
                const long long G = games0 + sc.s.exg[row + g], P = pos0 + sc.s.exp[row + g];
                if (!(P + L > b.pool_cap || G >= b.games_cap)) E = min(sc.cum[row + g], q.slot_cap);
            }
        }
        int x = 0, tx;
        long long y = E, ty;
        block_scan2(x, y, tx, ty);
        if (g < n) sc.exe[row + g] = ebase + y;
        ebase += ty;
    }
    if (threadIdx.x == 0) {
        sc.rowtot_e[k] = ebase;
        sc.s.rowpre[2 * k] = gpre;
        sc.s.rowpre[2 * k + 1] = ppre;
    }
}

// (F) one wave per slot, walking its games as traj_steps_copy_kernel does.  Position i of a
// game whose first step is bs, with hh = h - 1 of its positions searched before the launch, was
// searched at step bs + i - hh (i >= hh); its entries start at cum - nnz of that step.
__global__ __launch_bounds__(kSlotWaves * 64) void traj_policy_steps_copy_kernel(int n, int K, const int32_t *reached,
                                                                                 zc_traj_buffers b,
                                                                                 zc_traj_policy_buffers q,
                                                                                 const int32_t *na, const uint16_t *mv,
                                                                                 int stride, PolicyStepScratch sc) {
    const int lane = (int)(threadIdx.x & 63);
    const int g = (int)(blockIdx.x * kSlotWaves + (threadIdx.x >> 6));
    if (g >= n) return;
    const int Kr = steps_reached(K, reached);
    const long long ebase = sc.ebase[0];
    if (g == 0 && lane == 0) {  // the counter's update: every wave read its old value from the scratch
        long long tot = 0;
        for (int k = 0; k < Kr; ++k) tot += sc.rowtot_e[k];
        q.d_pctl[ZC_TRAJ_PI_ENTRIES] = ebase + tot;
    }
    const int32_t *slot = b.d_slot + 4 * (size_t)g;
    int game = slot[1];
    if (game < 0) return;
    const long long pos0 = b.d_ctl[kTrajPositions], games0 = b.d_ctl[kTrajGames], next0 = b.d_ctl[kTrajNext],
                    quota = b.d_ctl[kTrajQuota];
    int32_t *off = q.d_slot_off + (size_t)g * (b.max_len + 1);
    uint32_t *spi = q.d_slot_pi + (size_t)g * q.slot_cap;
    const long long cap = q.slot_cap;
    const int m = sc.s.played[g];
    int hh = min(max(slot[0], 1), b.max_len) - 1, bs = 0, ov = 0;
    bool first = true;
    long long epre = 0;  // the entries of the rows before step kdone
    int kdone = 0;
    for (int c0 = 0; c0 < m && game >= 0; c0 += 64) {
        const int k = c0 + lane;
        const int Lv = k < m ? sc.s.fl[(size_t)k * n + g] : 0;
        unsigned long long fin = __ballot(Lv > 0);
        while (fin && game >= 0) {
            const int j = __ffsll((long long)fin) - 1;
            fin &= fin - 1;
            const int kk = c0 + j;
            const size_t e = (size_t)kk * n + g;
            const int L = __shfl(Lv, j);
            for (; kdone < kk; kdone += 64) {
                long long v = (kdone + lane < kk) ? sc.rowtot_e[kdone + lane] : 0;
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                epre += v;
            }
            kdone = kk;
            const long long gi = sc.s.rowpre[2 * kk] + sc.s.exg[e];
            const long long G = games0 + gi, P = pos0 + sc.s.rowpre[2 * kk + 1] + sc.s.exp[e];
            const long long total = sc.cum[e];
            const long long E = min(total, cap);
            if (total > cap) ov |= kPiSlotFull;
            if (!(P + L > b.pool_cap || G >= b.games_cap)) {
                long long at = ebase + epre + sc.exe[e];
                if (at + E > q.pi_pool_cap) {  // dropped: first = count = 0
                    ov |= kPiPoolFull;
                    at = -1;
                }
                for (int i = lane; i < L; i += 64) {
                    long long o0, o1;
                    if (i < hh) {
                        o0 = i ? off[i] : 0;
                        o1 = off[i + 1];
                    } else if (i + 1 < L) {
                        const size_t es = (size_t)(bs + i - hh) * n + g;
                        o1 = min((long long)sc.cum[es], cap);
                        o0 = min((long long)sc.cum[es] - sc.nnz[es], cap);
                    } else {
                        o0 = o1 = E;
                    }
                    q.d_pool_first[P + i] = at < 0 ? 0 : at + o0;
                    q.d_pool_count[P + i] = at < 0 ? 0 : (int32_t)(o1 - o0);
                }
                if (at >= 0) {
                    const long long held = hh > 0 ? min((long long)off[hh], cap) : 0;
                    for (long long x = lane; x < held; x += 64) q.d_pool_pi[at + x] = spi[x];
                    for (int s = bs; s <= kk; ++s) {
                        const size_t es = (size_t)s * n + g;
                        ov |= policy_row_emit(na + es * stride, mv ? mv + es * stride : nullptr, stride, lane,
                                              q.d_pool_pi + at, (long long)sc.cum[es] - sc.nnz[es], cap) & kPiSaturated;
                    }
                }
            }
            // the offsets the single appends of this game left in the slot (a later game of the
            // slot overwrites them as far as it gets)
            for (int s = bs + lane; s <= kk; s += 64) {
                const int pos = hh + (s - bs);
                if (pos < b.max_len) off[pos + 1] = (int32_t)min((long long)sc.cum[(size_t)s * n + g], cap);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            const long long nx = next0 + gi;
            game = nx < quota ? (int)nx : -1;
            first = false;
            hh = 0;
            bs = kk + 1;
        }
    }
    // the game in progress: its rows since bs appended to the slot's CSR
    if (!first && lane == 0) off[0] = 0;
    const int cnt = game >= 0 ? m - bs : 0;
    for (int t = 0; t < cnt; ++t) {
        const int pos = hh + t;
        if (pos >= b.max_len) break;  // never: the record flags a game longer than max_len
        const size_t es = (size_t)(bs + t) * n + g;
        const long long c1 = sc.cum[es];
        ov |= policy_row_emit(na + es * stride, mv ? mv + es * stride : nullptr, stride, lane, spi, c1 - sc.nnz[es], cap);
        if (lane == 0) off[pos + 1] = (int32_t)min(c1, cap);
    }
    ov = (__ballot(ov & kPiSlotFull) ? kPiSlotFull : 0) | (__ballot(ov & kPiPoolFull) ? kPiPoolFull : 0) |
         (__ballot(ov & kPiSaturated) ? kPiSaturated : 0);
    if (lane == 0 && ov) atomicOr((unsigned long long *)(q.d_pctl + ZC_TRAJ_PI_OVERFLOW), (unsigned long long)ov);
}

// Dense targets, width 7 — one wave per row, lane = column: count / sum of the row's entries.
template <typename T>
__global__ __launch_bounds__(256) void traj_policy_dense7_kernel(int n_rows, const int64_t *first,
                                                                 const int32_t *count, const uint32_t *ent, T *out) {
    const int lane = (int)(threadIdx.x & 63);
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int c = count[r];
    const uint32_t *e = ent + first[r];
    int sum = 0, mine = 0;
    for (int k = 0; k < c; ++k) {
        const uint32_t v = e[k];
        sum += (int)(v >> 16);
        if ((int)(v & 0xFFFF) == lane) mine = (int)(v >> 16);
    }
    if (lane < 7) {
        const float p = mine ? __fdiv_rn((float)mine, (float)sum) : 0.0f;
        if constexpr (sizeof(T) == 2) out[r * 7 + lane] = __float2half_rn(p);
        else out[r * 7 + lane] = p;
    }
}

// Dense targets, width 4096 — a pure HBM-write kernel: one wave per row zero-fills its 16 KB
// (fp16: 8 KB) with 16-byte stores, 1 KB per wave instruction, waits for them, then scatters
// the (at most 256) non-zero cells at from * 64 + to.
template <typename T>
__global__ __launch_bounds__(256) void traj_policy_dense4096_kernel(int n_rows, const int64_t *first,
                                                                    const int32_t *count, const uint32_t *ent, T *out) {
    const int lane = (int)(threadIdx.x & 63);
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    T *row = out + r * 4096;
    float4 *row16 = (float4 *)row;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    constexpr int kChunks = 4096 * (int)sizeof(T) / 16;
#pragma unroll
    for (int k = 0; k < kChunks / 64; ++k) row16[k * 64 + lane] = z;
    const int c = count[r];
    if (c <= 0) return;
    const uint32_t *e = ent + first[r];
    int sum = 0;
    for (int k = lane; k < c; k += 64) sum += (int)(e[k] >> 16);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    // the zeros have landed before a cell is written again (same wave, other lanes)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
    const float fs = (float)sum;
    for (int k = lane; k < c; k += 64) {
        const uint32_t v = e[k];
        const int idx = (int)(v & 63) * 64 + (int)((v >> 6) & 63);
        const float p = (v >> 16) ? __fdiv_rn((float)(v >> 16), fs) : 0.0f;
        if constexpr (sizeof(T) == 2) row[idx] = __float2half_rn(p);
        else row[idx] = p;
    }
}

// ---------------------------------------------------------------- openings
// A book of openings in place of the one d_init row: one thread per (slot, word).  A slot whose
// game has only its first position (slot[0] == 1, game >= 0: started by Trajectories.start or
// refilled by the record just before) takes row (game / share) % book_rows of the book as its
// root and as position 0 of its history.  Idle slots and games in progress are not touched, so
// the call can be repeated.
__global__ __launch_bounds__(256) void traj_openings_kernel(int n, zc_traj_buffers b, const uint64_t *book,
                                                            int book_rows, int share, uint64_t *roots) {
    const int W = b.row_bytes / 8;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long g = t / W;
    const int w = (int)(t % W);
    if (g >= n) return;
    const int32_t *slot = b.d_slot + 4 * (size_t)g;
    const int game = slot[1];
    if (game < 0 || slot[0] != 1) return;
    const uint64_t v = book[(size_t)((game / share) % book_rows) * W + w];
    roots[(size_t)g * W + w] = v;
    ((uint64_t *)b.d_hist)[(size_t)g * b.max_len * W + w] = v;
}

}  // namespace

void launch_traj_openings(int n, const zc_traj_buffers &b, const void *book, int book_rows, int share, void *roots,
                          hipStream_t s) {
    const long long threads = (long long)n * (b.row_bytes / 8);
    hipLaunchKernelGGL(traj_openings_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, n, b,
                       (const uint64_t *)book, book_rows, share, (uint64_t *)roots);
}

void launch_traj_policy_append(int n, const zc_traj_buffers &b, const zc_traj_policy_buffers &q, const int32_t *na,
                               const uint16_t *mv, int stride, hipStream_t s) {
    const dim3 slots((unsigned)((n + kSlotWaves - 1) / kSlotWaves)), wb(kSlotWaves * 64);
    hipLaunchKernelGGL(traj_policy_append_kernel, slots, wb, 0, s, n, b, q, na, mv, stride);
}

void launch_traj_policy_commit(int n, const zc_traj_buffers &b, const zc_traj_policy_buffers &q, hipStream_t s) {
    const dim3 slots((unsigned)((n + kSlotWaves - 1) / kSlotWaves)), wb(kSlotWaves * 64);
    hipLaunchKernelGGL(traj_policy_reserve_kernel, dim3(1), dim3(kRecThreads), 0, s, n, b, q);
    hipLaunchKernelGGL(traj_policy_copy_kernel, slots, wb, 0, s, n, b, q);
}

void launch_traj_policy_dense(int n_rows, const int64_t *first, const int32_t *count, const uint32_t *ent, int width,
                              bool half, void *out, hipStream_t s) {
    const dim3 grid((unsigned)((n_rows + 3) / 4)), wb(256);
    if (width == 7) {
        if (half) hipLaunchKernelGGL(traj_policy_dense7_kernel<__half>, grid, wb, 0, s, n_rows, first, count, ent, (__half *)out);
        else hipLaunchKernelGGL(traj_policy_dense7_kernel<float>, grid, wb, 0, s, n_rows, first, count, ent, (float *)out);
    } else {
        if (half) hipLaunchKernelGGL(traj_policy_dense4096_kernel<__half>, grid, wb, 0, s, n_rows, first, count, ent, (__half *)out);
        else hipLaunchKernelGGL(traj_policy_dense4096_kernel<float>, grid, wb, 0, s, n_rows, first, count, ent, (float *)out);
    }
}

size_t traj_steps_scratch_bytes(int n, int K) { return steps_scratch_layout(n, K, nullptr, nullptr); }

void launch_traj_record_steps(int n, int K, const zc_traj_buffers &b, const void *states, const int16_t *moves,
                              const int32_t *results, const int32_t *reached, void *scratch, hipStream_t s) {
    StepScratch sc;
    steps_scratch_layout(n, K, (uint8_t *)scratch, &sc);
    const dim3 slots((unsigned)((n + kSlotWaves - 1) / kSlotWaves)), wb(kSlotWaves * 64);
    hipLaunchKernelGGL(traj_steps_lens_kernel, slots, wb, 0, s, n, K, reached, (const int32_t *)b.d_slot, results, sc);
    hipLaunchKernelGGL(traj_steps_rows_kernel, dim3((unsigned)K), dim3(kRecThreads), 0, s, n, K, reached, sc);
    hipLaunchKernelGGL(traj_steps_totals_kernel, dim3(1), dim3(kRecThreads), 0, s, K, reached, b, sc);
    hipLaunchKernelGGL(traj_steps_copy_kernel, slots, wb, 0, s, n, K, reached, b, (const uint8_t *)states, moves,
                       results, sc);
}

size_t traj_policy_steps_scratch_bytes(int n, int K) { return policy_steps_scratch_layout(n, K, nullptr, nullptr); }

void launch_traj_policy_record_steps(int n, int K, const zc_traj_buffers &b, const zc_traj_policy_buffers &q,
                                     const int32_t *results, const int32_t *na, const uint16_t *mv, int stride,
                                     const int32_t *reached, void *scratch, hipStream_t s) {
    PolicyStepScratch sc;
    policy_steps_scratch_layout(n, K, (uint8_t *)scratch, &sc);
    const dim3 slots((unsigned)((n + kSlotWaves - 1) / kSlotWaves)), wb(kSlotWaves * 64);
    hipLaunchKernelGGL(traj_policy_steps_lens_kernel, slots, wb, 0, s, n, K, reached, b, q, results, na, stride, sc);
    hipLaunchKernelGGL(traj_steps_rows_kernel, dim3((unsigned)K), dim3(kRecThreads), 0, s, n, K, reached, sc.s);
    hipLaunchKernelGGL(traj_policy_steps_rows_kernel, dim3((unsigned)K), dim3(kRecThreads), 0, s, n, K, reached, b, q, sc);
    hipLaunchKernelGGL(traj_policy_steps_copy_kernel, slots, wb, 0, s, n, K, reached, b, q, na, mv, stride, sc);
}

void launch_traj_record(int n, const zc_traj_buffers &b, void *states, const int16_t *moves, int32_t *results,
                        const int32_t *flags, const int32_t *rep, hipStream_t s) {
    hipLaunchKernelGGL(traj_record_kernel, dim3(1), dim3(kRecThreads), 0, s, n, b, (uint8_t *)states, moves, results,
                       flags, rep);
    const long long threads = (long long)n * b.max_len;
    hipLaunchKernelGGL(traj_copy_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, n, b);
}

}  // namespace zc
