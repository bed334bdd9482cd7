// arena.hip — routing for a pool whose games are evaluated by one of two networks
// (include/zeroclone.h, "arena"): the stable partition of the games by their key, and the row
// copies that carry a flush through it (gather -> network A | network B -> scatter).
//
// The route is one workgroup: a pool has at most a few thousand games, and one pass of ballots
// orders them.  The copies move bytes only and sit on no dependency chain, so their one concern
// is coalescing: the lanes of a wave run along a row (and on into the next row of the same
// block when a row is shorter than a wave's access), each at the widest access the row size and
// the two base pointers allow.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zeroclone.h"

namespace {

constexpr int ROUTE_THREADS = ZC_ARENA_ROUTE_THREADS;
constexpr int ROUTE_WAVES = ROUTE_THREADS / 64;
constexpr int COPY_THREADS = 256;
constexpr uint32_t COPY_UNITS = 1024;   // accesses a copy block aims for (4 per thread)

// Lanes below this one whose bit is set in `mask`.
__device__ __forceinline__ int rank_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(ROUTE_THREADS) void arena_route_kernel(int n, const int32_t *__restrict__ key,
                                                                    int32_t *__restrict__ perm,
                                                                    int32_t *__restrict__ count) {
    __shared__ int wave_tot[ROUTE_WAVES][2];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    // the size of group 0: where group 1 starts
    int mine = 0;
    for (int i = t; i < n; i += ROUTE_THREADS) mine += !(key[i] & 1);
    for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (lane == 0) wave_tot[wave][0] = mine;
    __syncthreads();
    int n0 = 0;
    for (int w = 0; w < ROUTE_WAVES; w++) n0 += wave_tot[w][0];
    __syncthreads();
    if (t == 0) {
        count[0] = n0;
        count[1] = n - n0;
    }
    // chunks of ROUTE_THREADS keys in index order, each group's running base carried along
    int base0 = 0, base1 = n0;
    for (int lo = 0; lo < n; lo += ROUTE_THREADS) {
        const int i = lo + t;
        const bool live = i < n;
        const int b = live ? (key[i] & 1) : 0;
        const unsigned long long m0 = __ballot(live && !b), m1 = __ballot(live && b);
        if (lane == 0) {
            wave_tot[wave][0] = __popcll(m0);
            wave_tot[wave][1] = __popcll(m1);
        }
        __syncthreads();
        int before0 = 0, before1 = 0, all0 = 0, all1 = 0;
        for (int w = 0; w < ROUTE_WAVES; w++) {
            const int c0 = wave_tot[w][0], c1 = wave_tot[w][1];
            if (w < wave) {
                before0 += c0;
                before1 += c1;
            }
            all0 += c0;
            all1 += c1;
        }
        if (live) perm[b ? base1 + before1 + rank_below(m1) : base0 + before0 + rank_below(m0)] = i;
        base0 += all0;
        base1 += all1;
        __syncthreads();   // the totals are read before the next chunk overwrites them
    }
}

// Row i * rows + j of the partition-order side <-> row perm[i] * game_rows + j of the game-order
// side, in accesses of sizeof(T): a block owns `block_rows` consecutive partition-order rows and
// its threads run over their accesses in order.
template <typename T, bool SCATTER>
__global__ __launch_bounds__(COPY_THREADS) void arena_copy_kernel(int n, uint32_t rows, uint32_t game_rows,
                                                                  uint32_t units, uint32_t block_rows,
                                                                  const int32_t *__restrict__ perm,
                                                                  const T *__restrict__ src, T *__restrict__ dst) {
    const uint32_t total = (uint32_t)n * rows, r0 = blockIdx.x * block_rows;
    const uint32_t nr = total - r0 < block_rows ? total - r0 : block_rows;
    const uint32_t work = nr * units;
    for (uint32_t a = threadIdx.x; a < work; a += COPY_THREADS) {
        const uint32_t rl = a / units, off = a - rl * units;
        const uint32_t r = r0 + rl, g = r / rows, j = r - g * rows;
        const uint32_t p = (uint32_t)perm[g];
        if (p >= (uint32_t)n) continue;
        const size_t part = (size_t)r * units + off;
        const size_t game = ((size_t)p * game_rows + j) * units + off;
        if (SCATTER)
            dst[game] = src[part];
        else
            dst[part] = src[game];
    }
}

template <typename T, bool SCATTER>
void launch_copy(int n, int rows, int game_rows, int64_t row_bytes, const int32_t *perm, const void *src, void *dst,
                 hipStream_t s) {
    const uint32_t units = (uint32_t)(row_bytes / (int64_t)sizeof(T));
    const uint32_t block_rows = units >= COPY_UNITS ? 1u : (COPY_UNITS + units - 1) / units;
    const uint32_t total = (uint32_t)n * (uint32_t)rows;
    const uint32_t blocks = (total + block_rows - 1) / block_rows;
    hipLaunchKernelGGL((arena_copy_kernel<T, SCATTER>), dim3(blocks), dim3(COPY_THREADS), 0, s, n, (uint32_t)rows,
                       (uint32_t)game_rows, units, block_rows, perm, (const T *)src, (T *)dst);
}

template <bool SCATTER>
int arena_copy(int32_t n, int32_t rows, int32_t game_rows, int64_t row_bytes, const int32_t *d_perm, const void *d_src,
               void *d_dst, void *hip_stream) {
    if (n < 0 || rows < 1 || game_rows < rows || row_bytes < 2 || (row_bytes & 1)) return ZC_EINVAL;
    if ((int64_t)n * game_rows >= ((int64_t)1 << 31)) return ZC_EINVAL;
    if (row_bytes >= ((int64_t)1 << 31)) return ZC_EINVAL;   // a block's accesses are counted in 32 bits
    if (!n) return ZC_OK;
    if (!d_perm || !d_src || !d_dst) return ZC_EINVAL;
    const uintptr_t bits = (uintptr_t)d_src | (uintptr_t)d_dst | (uintptr_t)row_bytes;
    if (bits & 1) return ZC_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    if (!(bits & 15))
        launch_copy<uint4, SCATTER>(n, rows, game_rows, row_bytes, d_perm, d_src, d_dst, s);
    else if (!(bits & 7))
        launch_copy<uint2, SCATTER>(n, rows, game_rows, row_bytes, d_perm, d_src, d_dst, s);
    else if (!(bits & 3))
        launch_copy<uint32_t, SCATTER>(n, rows, game_rows, row_bytes, d_perm, d_src, d_dst, s);
    else
        launch_copy<uint16_t, SCATTER>(n, rows, game_rows, row_bytes, d_perm, d_src, d_dst, s);
    return hipGetLastError() == hipSuccess ? ZC_OK : ZC_EHIP;
}

}  // namespace

extern "C" {

int zc_arena_route_async(int32_t n, const int32_t *d_key, int32_t *d_perm, int32_t *d_count, void *hip_stream) {
    if (n < 0 || !d_count || (n && (!d_key || !d_perm))) return ZC_EINVAL;
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    hipLaunchKernelGGL(arena_route_kernel, dim3(1), dim3(ROUTE_THREADS), 0, (hipStream_t)hip_stream, (int)n, d_key,
                       d_perm, d_count);
    return hipGetLastError() == hipSuccess ? ZC_OK : ZC_EHIP;
}

int zc_arena_gather_async(int32_t n, int32_t rows, int32_t game_rows, int64_t row_bytes, const int32_t *d_perm,
                          const void *d_src, void *d_dst, void *hip_stream) {
    return arena_copy<false>(n, rows, game_rows, row_bytes, d_perm, d_src, d_dst, hip_stream);
}

int zc_arena_scatter_async(int32_t n, int32_t rows, int32_t game_rows, int64_t row_bytes, const int32_t *d_perm,
                           const void *d_src, void *d_dst, void *hip_stream) {
    return arena_copy<true>(n, rows, game_rows, row_bytes, d_perm, d_src, d_dst, hip_stream);
}

}  // extern "C"
