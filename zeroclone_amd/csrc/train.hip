// train.hip — the learner's two device steps (include/zeroclone.h, "training"):
//
//   zc_train_batch_async  one minibatch gathered and decoded from a compact training set: the
//                         planes, the labels as floats, every position's legal moves and the
//                         root visit counts as targets aligned with them.  One wave per batch
//                         row: Connect4 four rows a workgroup, chess one (its move generator,
//                         chess_device.h, keeps 5 KB of LDS scratch per position).
//   zc_train_loss_async   mean-squared-error value loss and cross-entropy policy loss over the
//                         LEGAL moves' softmax (puct_common.h softmax_priors is what the searches
//                         evaluate), with both gradients.  Three launches: per-row terms (one wave
//                         per row), one workgroup that adds them up in a fixed order and counts
//                         the policy rows, and the logits' gradient (one wave per row; a
//                         4096-wide row is zero-filled with 16-byte stores, then its at most 256
//                         legal cells are written).
//
// Everything is plain stores and loads: no floating-point atomics, so a call's bits depend on
// its inputs alone.
#include <hip/hip_fp16.h>

#include "chess_device.h"

namespace {

using namespace zc::chessdev;

constexpr int ROW_WAVES = 4;            // batch rows (waves) per workgroup
constexpr int ROW_THREADS = ROW_WAVES * 64;
constexpr int REDUCE_THREADS = 256;
constexpr int MAX_PER_LANE = ZC_CHESS_MAX_MOVES / 64;   // a row's legal moves per lane

__device__ __forceinline__ int rank_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

template <typename T>
__device__ __forceinline__ T to_plane(float v) {
    if constexpr (sizeof(T) == 2) return __float2half(v);
    else return v;
}

__device__ __forceinline__ float wave_sum(float x) {
    for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}
__device__ __forceinline__ float wave_max(float x) {
    for (int d = 32; d; d >>= 1) x = fmaxf(x, __shfl_xor(x, d, 64));
    return x;
}
__device__ __forceinline__ int wave_sum_int(int x) {
    for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// ---------------------------------------------------------------- minibatch, Connect4
// Lane l < 42 owns cell (row l / 7, column l % 7) of both planes; lanes 0..6 own a column of the
// legal list and the targets.  A mirrored row reads column 6 - c wherever it writes column c.
template <typename T>
__global__ __launch_bounds__(ROW_THREADS) void train_batch_c4_kernel(zc_train_set set, int B, const int64_t *index,
                                                                     const uint8_t *flags, T *planes, float *z,
                                                                     uint16_t *legal, int32_t *n_legal, float *target,
                                                                     int32_t *status) {
    const int lane = (int)(threadIdx.x & 63);
    const int b = (int)blockIdx.x * ROW_WAVES + (int)(threadIdx.x >> 6);
    if (b >= B) return;
    const int64_t i = index[b];
    const bool ok = i >= 0 && i < set.n_rows;
    const bool mirror = flags && (flags[b] & 1);
    uint64_t s0 = 0, s1 = 0;
    int turn = 0;
    if (ok) {
        const uint64_t *row = (const uint64_t *)set.d_rows + (size_t)i * 3;
        s0 = row[0];
        s1 = row[1];
        turn = (int)(row[2] & 1);
    }
    if (lane < 42) {
        const int r = lane / 7, c = lane % 7, sc = mirror ? 6 - c : c;
        const int bit = 7 * sc + (5 - r);
        const float x = (float)((s0 >> bit) & 1), o = (float)((s1 >> bit) & 1);
        T *p = planes + (size_t)b * 84;
        p[lane] = to_plane<T>(turn == 0 ? x : o);
        p[42 + lane] = to_plane<T>(turn == 0 ? o : x);
    }
    // the row's entries: every lane reads them all (at most 7)
    const int sc = mirror ? 6 - lane : lane;   // the set's column behind output column `lane`
    const bool playable = ok && lane < 7 && !(((s0 | s1) >> (7 * sc + 5)) & 1);
    int sum = 0, mine = 0, bad = !ok ? 2 : 0;
    if (ok && set.d_pi_off) {
        const int64_t e0 = set.d_pi_off[i], e1 = set.d_pi_off[i + 1];
        for (int64_t k = e0; k < e1; ++k) {
            const uint32_t v = set.d_pi[k];
            const int id = (int)(v & 0xFFFF), cnt = (int)(v >> 16);
            sum += cnt;
            if (id == sc && lane < 7) mine = cnt;
            // an entry for a column that cannot be played (or no column at all) is dropped
            if (id >= 7 || (((s0 | s1) >> (7 * id + 5)) & 1)) bad |= 1;
        }
    }
    const unsigned long long mask = __ballot(playable);
    const int n = __popcll(mask), at = rank_below(mask);
    if (lane < 7) {   // slots past n stay zero: lane j >= n clears slot j
        if (lane >= n) {
            legal[(size_t)b * 7 + lane] = 0;
            target[(size_t)b * 7 + lane] = 0.0f;
        }
        if (playable) {
            legal[(size_t)b * 7 + at] = (uint16_t)lane;
            target[(size_t)b * 7 + at] = mine ? __fdiv_rn((float)mine, (float)sum) : 0.0f;
        }
    }
    if (lane == 0) {
        z[b] = ok ? (float)set.d_labels[i] : 0.0f;
        n_legal[b] = n;
        if (bad) atomicOr(status, bad);
    }
}

// ---------------------------------------------------------------- minibatch, chess
// One wave per workgroup and position: lane = square for the planes (chess.hip's
// chess_planes_kernel, cell for cell), then get_legal_moves into LDS, then the entries matched
// to the list by from/to.
template <typename T>
__global__ __launch_bounds__(64) void train_batch_chess_kernel(zc_train_set set, int B, const int64_t *index, T *planes,
                                                              float *z, uint16_t *legal, int32_t *n_legal,
                                                              float *target, int32_t *status) {
    __shared__ ChessScratch S;
    __shared__ int32_t cnt[kMaxLegal];
    const int b = (int)blockIdx.x, ln = (int)lane();
    if (b >= B) return;
    const int64_t i = index[b];
    const bool ok = i >= 0 && i < set.n_rows;   // block-uniform
    const zc_chess_state *st = (const zc_chess_state *)set.d_rows + (ok ? i : 0);
    const uint8_t pc = ok ? st->board[ln] : (uint8_t)' ';
    const int t = ok ? (int)st->turn : 0, castle = ok ? (int)st->castle : 0;
    {
        const char pieces[12] = {'P', 'N', 'B', 'R', 'Q', 'K', 'p', 'n', 'b', 'r', 'q', 'k'};
        int which = -1;
        for (int k = 0; k < 12; ++k)
            if (pc == (uint8_t)pieces[k]) {
                which = k;
                break;
            }
        T *p = planes + (size_t)b * 17 * 64 + ln;
        for (int k = 0; k < 17; ++k) {
            float v;
            if (k < 12) v = k == which ? 1.0f : 0.0f;
            else if (k == 12) v = t == 0 ? 1.0f : 0.0f;
            else v = (castle >> (k - 13)) & 1 ? 1.0f : 0.0f;
            p[(size_t)k * 64] = to_plane<T>(ok ? v : 0.0f);
        }
    }
    S.board[ln] = pc;
    for (int j = ln; j < kMaxLegal; j += 64) cnt[j] = 0;
    __syncthreads();
    int n = 0, bad = ok ? 0 : 2;
    if (ok) {
        n = legal_moves(S.board, __builtin_amdgcn_readfirstlane(t), S.legal, S.pseudo, S.region);
        if (n < 0) {   // more than 256 legal moves: never in chess
            n = 0;
            bad |= 4;
        }
    }
    __syncthreads();
    int sum = 0;
    if (ok && set.d_pi_off) {
        const int64_t e0 = set.d_pi_off[i], e1 = set.d_pi_off[i + 1];
        for (int64_t k = e0 + ln; k < e1; k += 64) {
            const uint32_t v = set.d_pi[k];
            const uint32_t id = v & 0xFFF;   // from | to << 6
            sum += (int)(v >> 16);
            int at = -1;
            for (int j = 0; j < n; ++j)
                if ((S.legal[j] & 0xFFFu) == id) {
                    at = j;
                    break;
                }
            if (at >= 0) cnt[at] = (int)(v >> 16);
            else bad |= 1;   // not a move of this position: dropped
        }
        sum = wave_sum_int(sum);
    }
    __syncthreads();
    const float fs = (float)sum;
    for (int j = ln; j < kMaxLegal; j += 64) {
        const int c = cnt[j];
        legal[(size_t)b * kMaxLegal + j] = j < n ? S.legal[j] : (uint16_t)0;
        target[(size_t)b * kMaxLegal + j] = c ? __fdiv_rn((float)c, fs) : 0.0f;
    }
    bad = (__ballot(bad & 1) ? 1 : 0) | (bad & 6);
    if (ln == 0) {
        z[b] = ok ? (float)set.d_labels[i] : 0.0f;
        n_legal[b] = n;
        if (bad) atomicOr(status, bad);
    }
}

// ---------------------------------------------------------------- loss
// The policy loss adds terms of very different sizes (a target times a log-probability that can
// be hundreds), so its sums are carried as an unevaluated pair of floats hi + lo (Dekker / Knuth
// error-free transformations: fp32 operations only, the pair good to about 2^-45 relative) and
// rounded once at the end.
struct ff {
    float hi, lo;
};
__device__ __forceinline__ ff two_sum(float a, float b) {
    const float s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ ff ff_add(ff a, ff b) {
    const ff s = two_sum(a.hi, b.hi);
    const float e = s.lo + (a.lo + b.lo), hi = s.hi + e;
    return {hi, e - (hi - s.hi)};
}
__device__ __forceinline__ ff ff_mul(float t, ff a) {   // t * (a.hi + a.lo)
    const float p = t * a.hi;
    return {p, fmaf(t, a.hi, -p) + t * a.lo};
}
__device__ __forceinline__ ff wave_sum_ff(ff x) {
    for (int d = 32; d; d >>= 1) x = ff_add(x, ff{__shfl_xor(x.hi, d, 64), __shfl_xor(x.lo, d, 64)});
    return x;
}

// The scratch: six per-row arrays and the policy rows' count.
struct LossScratch {
    float *sq;       // (v - z)^2
    float *lp;       // -sum_j target_j log p_j (0 on a non-policy row), hi
    float *lp_lo;    //   and lo
    float *mx;       // the legal logits' maximum
    float *den;      // sum_j exp(x_j - max)
    int32_t *pol;    // 1 on a policy row
    int32_t *count;  // [0] = P
};

__host__ __device__ inline LossScratch loss_scratch(void *base, int B) {
    LossScratch s;
    s.sq = (float *)base;
    s.lp = s.sq + B;
    s.lp_lo = s.lp + B;
    s.mx = s.lp_lo + B;
    s.den = s.mx + B;
    s.pol = (int32_t *)(s.den + B);
    s.count = s.pol + B;
    return s;
}
inline int64_t loss_scratch_bytes(int B) { return ((int64_t)6 * B + 4) * 4; }

template <typename T>
__device__ __forceinline__ float logit_at(const T *row, int idx) {
    if constexpr (sizeof(T) == 2) return __half2float(row[idx]);
    else return row[idx];
}

// A legal move's logit index; -1 when the id names none (width 7: a column above 6).
template <int WIDTH>
__device__ __forceinline__ int logit_index(uint32_t id) {
    if constexpr (WIDTH == 7) return id < 7 ? (int)id : -1;
    else return (int)(id & 63) * 64 + (int)((id >> 6) & 63);
}

// Lane l holds the row's legal moves l, l + 64, ...: their logit index, logit and target.
template <int WIDTH, typename T>
struct RowMoves {
    int idx[MAX_PER_LANE];
    float x[MAX_PER_LANE], t[MAX_PER_LANE];
    __device__ __forceinline__ void load(int lane, int n, int stride, const T *logits, const uint16_t *legal,
                                         const float *target, size_t b) {
#pragma unroll
        for (int k = 0; k < MAX_PER_LANE; ++k) {
            const int j = lane + 64 * k;
            idx[k] = -1;
            x[k] = -INFINITY;
            t[k] = 0.0f;
            if (j < n) {
                idx[k] = logit_index<WIDTH>(legal[b * stride + j]);
                if (idx[k] >= 0) {
                    x[k] = logit_at(logits + b * WIDTH, idx[k]);
                    t[k] = target[b * stride + j];
                }
            }
        }
    }
};

// Per-row terms.  logits == nullptr: the value part alone.
template <int WIDTH, typename T>
__global__ __launch_bounds__(ROW_THREADS) void train_loss_rows_kernel(int B, int stride, const T *logits, const float *v,
                                                                      const float *z, const uint16_t *legal,
                                                                      const int32_t *n_legal, const float *target,
                                                                      LossScratch sc, float *grad_v) {
    const int lane = (int)(threadIdx.x & 63);
    const int b = (int)blockIdx.x * ROW_WAVES + (int)(threadIdx.x >> 6);
    if (b >= B) return;
    if (lane == 0) {
        const float d = v[b] - z[b];
        sc.sq[b] = d * d;
        grad_v[b] = 2.0f * d / (float)B;
    }
    if (!logits) return;
    const int n = min(max(n_legal[b], 0), stride);
    RowMoves<WIDTH, T> r;
    r.load(lane, n, stride, logits, legal, target, (size_t)b);
    float tsum = 0.0f, m = -INFINITY;
#pragma unroll
    for (int k = 0; k < MAX_PER_LANE; ++k) {
        tsum += r.t[k];
        if (r.idx[k] >= 0) m = fmaxf(m, r.x[k]);
    }
    tsum = wave_sum(tsum);
    m = wave_max(m);
    float den = 0.0f;
#pragma unroll
    for (int k = 0; k < MAX_PER_LANE; ++k)
        if (r.idx[k] >= 0) den += expf(r.x[k] - m);
    den = wave_sum(den);
    const bool policy = tsum > 0.0f;
    ff lp = {0.0f, 0.0f};
    if (policy) {
        const float lz = logf(den);
#pragma unroll
        for (int k = 0; k < MAX_PER_LANE; ++k)   // -log p_j = log(den) + (max - x_j), the difference exact
            if (r.idx[k] >= 0) lp = ff_add(lp, ff_mul(r.t[k], ff_add(two_sum(m, -r.x[k]), ff{lz, 0.0f})));
        lp = wave_sum_ff(lp);
    }
    if (lane == 0) {
        sc.lp[b] = lp.hi;
        sc.lp_lo[b] = lp.lo;
        sc.mx[b] = m;
        sc.den[b] = den;
        sc.pol[b] = policy ? 1 : 0;
    }
}

// One workgroup: thread t adds rows t, t + 256, ... in that order, a wave adds its lanes'
// sums by a butterfly, wave 0 adds the waves' in wave order.
__global__ __launch_bounds__(REDUCE_THREADS) void train_loss_reduce_kernel(int B, int has_policy, LossScratch sc,
                                                                           float *loss) {
    __shared__ float part[REDUCE_THREADS / 64][3];
    __shared__ int pcount[REDUCE_THREADS / 64];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    float sq = 0.0f;
    ff lp = {0.0f, 0.0f};
    int p = 0;
    for (int b = t; b < B; b += REDUCE_THREADS) {
        sq += sc.sq[b];
        if (has_policy) {
            lp = ff_add(lp, ff{sc.lp[b], sc.lp_lo[b]});
            p += sc.pol[b];
        }
    }
    sq = wave_sum(sq);
    lp = wave_sum_ff(lp);
    p = wave_sum_int(p);
    if (lane == 0) {
        part[wave][0] = sq;
        part[wave][1] = lp.hi;
        part[wave][2] = lp.lo;
        pcount[wave] = p;
    }
    __syncthreads();
    if (t == 0) {
        float a = 0.0f;
        ff c = {0.0f, 0.0f};
        int P = 0;
        for (int w = 0; w < REDUCE_THREADS / 64; ++w) {
            a += part[w][0];
            c = ff_add(c, ff{part[w][1], part[w][2]});
            P += pcount[w];
        }
        loss[0] = a / (float)B;
        float lpm = 0.0f;
        if (P > 0) {   // (hi + lo) / P, the quotient's remainder put back
            const float fp = (float)P, q = c.hi / fp;
            lpm = q + (fmaf(-q, fp, c.hi) + c.lo) / fp;
        }
        loss[1] = lpm;
        sc.count[0] = P;
    }
}

template <typename T>
__device__ __forceinline__ T to_grad(float g) {
    if constexpr (sizeof(T) == 2) return __float2half_rn(g);
    else return g;
}

// The logits' gradient, width 7: lane c < 7 looks its column up in the row's legal list.
template <typename T>
__global__ __launch_bounds__(ROW_THREADS) void train_loss_grad7_kernel(int B, int stride, const T *logits,
                                                                       const uint16_t *legal, const int32_t *n_legal,
                                                                       const float *target, LossScratch sc, T *grad) {
    const int lane = (int)(threadIdx.x & 63);
    const int b = (int)blockIdx.x * ROW_WAVES + (int)(threadIdx.x >> 6);
    if (b >= B || lane >= 7) return;
    float g = 0.0f;
    const int P = sc.count[0];
    if (P > 0 && sc.pol[b]) {
        const int n = min(max(n_legal[b], 0), stride);
        for (int j = 0; j < n; ++j)
            if ((int)legal[(size_t)b * stride + j] == lane) {
                const float p = __fdiv_rn(expf(logit_at(logits + (size_t)b * 7, lane) - sc.mx[b]), sc.den[b]);
                g = __fdiv_rn(p - target[(size_t)b * stride + j], (float)P);
                break;
            }
    }
    grad[(size_t)b * 7 + lane] = to_grad<T>(g);
}

// The logits' gradient, width 4096: the row zero-filled with 16-byte stores (1 KB per wave
// instruction), those waited for, then the legal cells written.
template <typename T>
__global__ __launch_bounds__(ROW_THREADS) void train_loss_grad4096_kernel(int B, int stride, const T *logits,
                                                                          const uint16_t *legal, const int32_t *n_legal,
                                                                          const float *target, LossScratch sc, T *grad) {
    const int lane = (int)(threadIdx.x & 63);
    const int b = (int)blockIdx.x * ROW_WAVES + (int)(threadIdx.x >> 6);
    if (b >= B) return;
    T *row = grad + (size_t)b * 4096;
    float4 *row16 = (float4 *)row;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    constexpr int kChunks = 4096 * (int)sizeof(T) / 16;
#pragma unroll
    for (int k = 0; k < kChunks / 64; ++k) row16[k * 64 + lane] = zero;
    const int P = sc.count[0];
    if (P <= 0 || !sc.pol[b]) return;
    const int n = min(max(n_legal[b], 0), stride);
    RowMoves<4096, T> r;
    r.load(lane, n, stride, logits, legal, target, (size_t)b);
    const float m = sc.mx[b], den = sc.den[b], fp = (float)P;
    // the zeros have landed before a cell is written again (same wave, other lanes)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
    for (int k = 0; k < MAX_PER_LANE; ++k)
        if (r.idx[k] >= 0) {
            const float p = __fdiv_rn(expf(r.x[k] - m), den);
            row[r.idx[k]] = to_grad<T>(__fdiv_rn(p - r.t[k], fp));
        }
}

template <typename T>
void launch_batch(const zc_train_set &set, int B, const int64_t *index, const uint8_t *flags, void *planes, float *z,
                  uint16_t *legal, int32_t *n_legal, float *target, int32_t *status, hipStream_t s) {
    if (set.game == ZC_TRAIN_C4)
        hipLaunchKernelGGL(train_batch_c4_kernel<T>, dim3((unsigned)((B + ROW_WAVES - 1) / ROW_WAVES)), dim3(ROW_THREADS),
                           0, s, set, B, index, flags, (T *)planes, z, legal, n_legal, target, status);
    else
        hipLaunchKernelGGL(train_batch_chess_kernel<T>, dim3((unsigned)B), dim3(64), 0, s, set, B, index, (T *)planes, z,
                           legal, n_legal, target, status);
}

template <int WIDTH, typename T>
void launch_loss(int B, int stride, const void *logits, const float *v, const float *z, const uint16_t *legal,
                 const int32_t *n_legal, const float *target, const LossScratch &sc, float *loss, float *grad_v,
                 void *grad_logits, hipStream_t s) {
    const dim3 rows((unsigned)((B + ROW_WAVES - 1) / ROW_WAVES)), wb(ROW_THREADS);
    hipLaunchKernelGGL((train_loss_rows_kernel<WIDTH, T>), rows, wb, 0, s, B, stride, (const T *)logits, v, z, legal,
                       n_legal, target, sc, grad_v);
    hipLaunchKernelGGL(train_loss_reduce_kernel, dim3(1), dim3(REDUCE_THREADS), 0, s, B, logits ? 1 : 0, sc, loss);
    if (!logits) return;
    if constexpr (WIDTH == 7)
        hipLaunchKernelGGL(train_loss_grad7_kernel<T>, rows, wb, 0, s, B, stride, (const T *)logits, legal, n_legal,
                           target, sc, (T *)grad_logits);
    else
        hipLaunchKernelGGL(train_loss_grad4096_kernel<T>, rows, wb, 0, s, B, stride, (const T *)logits, legal, n_legal,
                           target, sc, (T *)grad_logits);
}

}  // namespace

extern "C" {

int zc_train_batch_async(const zc_train_set *set, int32_t B, const int64_t *d_index, const uint8_t *d_flags,
                         int32_t planes_dtype, void *d_planes, float *d_z, uint16_t *d_legal, int32_t *d_n_legal,
                         float *d_target, int32_t *d_status, void *hip_stream) {
    if (!set || B < 0) return ZC_EINVAL;
    if (planes_dtype != ZC_F32 && planes_dtype != ZC_F16) return ZC_EINVAL;
    if (set->game == ZC_TRAIN_C4 ? set->row_bytes != 24 : set->game == ZC_TRAIN_CHESS ? set->row_bytes != 72 : true)
        return ZC_EINVAL;
    if (set->game == ZC_TRAIN_CHESS && d_flags) return ZC_EINVAL;   // no mirror image of a chess position
    if (set->n_rows < 0 || !!set->d_pi_off != !!set->d_pi) return ZC_EINVAL;
    if (!B) return ZC_OK;
    if (!set->d_rows || !set->d_labels || !d_index || !d_planes || !d_z || !d_legal || !d_n_legal || !d_target ||
        !d_status)
        return ZC_EINVAL;
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    if (planes_dtype == ZC_F16)
        launch_batch<__half>(*set, B, d_index, d_flags, d_planes, d_z, d_legal, d_n_legal, d_target, d_status,
                             (hipStream_t)hip_stream);
    else
        launch_batch<float>(*set, B, d_index, d_flags, d_planes, d_z, d_legal, d_n_legal, d_target, d_status,
                            (hipStream_t)hip_stream);
    return hipGetLastError() == hipSuccess ? ZC_OK : ZC_EHIP;
}

int zc_train_loss_scratch_bytes(int32_t B, int64_t *bytes) {
    if (B < 0 || !bytes) return ZC_EINVAL;
    *bytes = loss_scratch_bytes(B);
    return ZC_OK;
}

int zc_train_loss_async(int32_t B, int32_t width, int32_t stride, const void *d_logits, int32_t logits_dtype,
                        const float *d_v, const float *d_z, const uint16_t *d_legal, const int32_t *d_n_legal,
                        const float *d_target, void *d_scratch, int64_t scratch_bytes, float *d_loss, float *d_grad_v,
                        void *d_grad_logits, void *hip_stream) {
    if (B < 1 || !d_v || !d_z || !d_loss || !d_grad_v) return ZC_EINVAL;
    if (!d_scratch || ((uintptr_t)d_scratch & 15) || scratch_bytes < loss_scratch_bytes(B)) return ZC_EINVAL;
    if (d_logits) {
        if (width != 7 && width != 4096) return ZC_EINVAL;
        if (stride < 1 || stride > ZC_CHESS_MAX_MOVES || (width == 7 && stride > 64)) return ZC_EINVAL;
        if (logits_dtype != ZC_F32 && logits_dtype != ZC_F16) return ZC_EINVAL;
        if (!d_legal || !d_n_legal || !d_target || !d_grad_logits) return ZC_EINVAL;
        if (width == 4096 && ((uintptr_t)d_grad_logits & 15)) return ZC_EINVAL;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    const LossScratch sc = loss_scratch(d_scratch, B);
    const bool half = logits_dtype == ZC_F16;
    (void)hipGetLastError();   // an earlier call's error is not this launch's
#define ZC_LOSS(W, T) \
    launch_loss<W, T>(B, stride, d_logits, d_v, d_z, d_legal, d_n_legal, d_target, sc, d_loss, d_grad_v, d_grad_logits, s)
    if (!d_logits || width == 7) {
        if (d_logits && half) ZC_LOSS(7, __half);
        else ZC_LOSS(7, float);
    } else {
        if (half) ZC_LOSS(4096, __half);
        else ZC_LOSS(4096, float);
    }
#undef ZC_LOSS
    return hipGetLastError() == hipSuccess ? ZC_OK : ZC_EHIP;
}

}  // extern "C"
