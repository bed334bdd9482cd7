// net_conv64.hip — the residual tower for 64-channel networks on gfx950 matrix cores.
//
// The second width of net_conv.hip's tower (ValueNetwork(64, blocks) / PolicyValueNetwork(64, ...)):
// a quarter of the residual layers' FLOPs of the 128-channel network.  Nothing of the 128 kernels
// is generalised — they are tuned to their own register and LDS budget; this file has its own
// pack kernel, per-layer conv (the yardstick), fused tower (plain and counted, with the value head
// and the policy 1x1 conv as epilogues) and stand-alone value head.  planes_to_nhwc_kernel
// (net_conv.hip) is width-free and feeds both.
//
// Every conv is the implicit GEMM D[cout][pixel] = sum_{tap, cin} Wt[tap][cout][cin] * X[pixel
// shifted by tap][cin] on v_mfma_f32_16x16x32_f16 (M = 16 output channels, N = 16 pixels, K = 32
// input channels per instruction), accumulated tap 0..8 and, inside a tap, k-step 0..cin/32-1:
// the same order in the per-layer kernel and in the fused tower, whose stored bits are equal.
//
// Tile and waves.  One workgroup = 4 waves = 128 pixels (2 chess boards, 3 Connect4 boards).
// Wave w owns output channels [32 (w & 1), +32) x pixels [64 (w >> 1), +64): two M tiles x four
// N tiles, so every activation fragment read from LDS feeds two MFMAs (16 channels x all pixels
// would halve that).  The two waves that share a channel half load the same weight fragments at
// about the same time; the second load is an L1 hit.
//
// LDS layout.  An activation row is a pixel's 64 channels (128 B) padded to kLD = 80 halfs =
// 160 B = ten 16-byte slots.  The B operand is read by ds_read_b128, lane l = (pixel l & 15,
// k-chunk l >> 4); the hardware serves it in four groups of 16 lanes, {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same + 32, each conflict-free when its 16 chunks fall on 16
// different slots of the 256-byte bank row.  A group holds 8 pixels (rows r = 0-3, 12-15 past some
// base) at chunk c and the other 8 (r = 4-11) at chunk c + 1.  With S slots per row the slot is
// (S r + c) mod 16.  For S = 10: 10 r mod 16 takes 8 different EVEN values over any 8 rows that
// differ mod 8 (10 = 2 x 5, 5 odd), which both row sets do; c and c + 1 differ in parity, so the
// 16 slots are distinct — for every tap shift (it moves both sets alike) and every k-step (it adds
// 4 to c).  S = 8 (unpadded) puts rows r and r + 2 on one slot (4-way); S = 9 puts row 4's chunk
// c + 1 on row 13's chunk c (9 x 9 = 1 mod 16): S = 10 is the smallest that works.  (The 128
// tower's 144 halfs are S = 18 = 2 x 9: the same rule.)  A row's slot class is its index mod 8, so 8 zero rows
// stand for every off-board tap: a lane reads the zero row of the class it would have read.
//   tower:  buf0 [128][80], 8 zero rows, buf1 [128][80]  = 42,240 B: three workgroups per CU
//   conv:   one buffer and the zero rows                  = 21,760 B
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "zc_internal.h"

namespace zc {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4x __attribute__((ext_vector_type(4)));

constexpr int kC = 64;              // channels
constexpr int kLD = 80;             // halfs per LDS row (see above)
constexpr int kTP = 128;            // pixels per tile
constexpr int kZR = 8;              // zero rows
constexpr int kZero = kTP;          // first zero row
constexpr int kBuf1 = kTP + kZR;    // buf1's first row
constexpr int kFrag = 512;          // halfs per weight fragment (16 channels x 32 k)
constexpr size_t kTowerLds = (size_t)(2 * kTP + kZR) * kLD * sizeof(_Float16);
constexpr size_t kConvLds = (size_t)(kTP + kZR) * kLD * sizeof(_Float16);

// IEEE 754-2019 maximum: a NaN stays a NaN (net_conv.hip relu_nan, where the reasons are)
__device__ __forceinline__ float relu_nan(float v) { return __builtin_elementwise_maximum(v, 0.0f); }

// One layer's MFMA loop.  J = the layer's k-steps per tap (cin / 32), JN the next layer's.
// a[2 j + m] holds the layer's tap-0 fragments (k-step j, M tile m) on entry and the next
// layer's on exit (from wn, when it is not null: in the ring at the last tap when JN == J, else
// after the loop).  wa / wn already hold the lane's offset into its first fragment; fragment
// (tap, j, m) is ((tap J + j) 4 + m) kFrag halfs further.  Weights come from L2 one tap ahead,
// activation fragments from LDS one k-step ahead.  prow0 = the lane's pixel row of N tile 0.
template <int H, int W, int J, int JN>
__device__ __forceinline__ void mfma_layer64(const _Float16 *lds, int src, const _Float16 *wa, const _Float16 *wn,
                                             h8 (&a)[4], int prow0, const int (&pyx)[4], int q, f4x (&acc)[2][4]) {
    auto rows = [&](int tap, const _Float16 *(&xb)[4]) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int sy = (pyx[n] >> 8) + dy, sx = (pyx[n] & 255) + dx;
            const bool sv = (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W;
            const int row = prow0 + (n * 16 + dy * W + dx);  // the pixel shifted by the tap
            xb[n] = lds + (sv ? src + row : kZero + (row & (kZR - 1))) * kLD + q * 8;
        }
    };
    const _Float16 *xb[4];
    rows(0, xb);
    h8 x[4], xn[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) x[n] = *(const h8 *)(xb[n]);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const _Float16 *xbn[4];
        if (tap + 1 < 9) rows(tap + 1, xbn);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            if (j + 1 < J) {
#pragma unroll
                for (int n = 0; n < 4; ++n) xn[n] = *(const h8 *)(xb[n] + (j + 1) * 32);
            } else if (tap + 1 < 9) {
#pragma unroll
                for (int n = 0; n < 4; ++n) xn[n] = *(const h8 *)(xbn[n]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[2 * j + m], x[n], acc[m][n], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                if (tap + 1 < 9) a[2 * j + m] = *(const h8 *)(wa + (size_t)(((tap + 1) * J + j) * 4 + m) * kFrag);
                else if (JN == J && wn) a[2 * j + m] = *(const h8 *)(wn + (size_t)(j * 4 + m) * kFrag);
            }
            if (j + 1 < J || tap + 1 < 9) {
#pragma unroll
                for (int n = 0; n < 4; ++n) x[n] = xn[n];
            }
        }
        if (tap + 1 < 9) {
#pragma unroll
            for (int n = 0; n < 4; ++n) xb[n] = xbn[n];
        }
    }
    if (JN != J && wn) {
#pragma unroll
        for (int j = 0; j < JN; ++j)
#pragma unroll
            for (int m = 0; m < 2; ++m) a[2 * j + m] = *(const h8 *)(wn + (size_t)(j * 4 + m) * kFrag);
    }
}

// out = rn16(relu?((acc + bias) + residual)), rounded once.  Lane (pixel row prow0 + 16 n, q)
// holds channels co0 + 16 m .. + 3 of its pixel (co0 = the wave's first channel + 4 q).  dst /
// res: the tile's first row, ld halfs per row (LDS: kLD, in place for the tower's residual
// layers; HBM: 64).  The residual reads are issued together, from a valid row; rows at or past
// npix are not written.
__device__ __forceinline__ void epilogue64(_Float16 *dst, const _Float16 *res, int ld, const float4 (&bv)[2], bool relu,
                                           int npix, int prow0, int co0, const f4x (&acc)[2][4]) {
    h4 rv[2][4];
    if (res) {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int P = min(prow0 + n * 16, npix - 1);
#pragma unroll
            for (int m = 0; m < 2; ++m) rv[m][n] = *(const h4 *)(res + (size_t)P * ld + co0 + 16 * m);
        }
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int P = prow0 + n * 16;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            float v[4] = {acc[m][n][0] + bv[m].x, acc[m][n][1] + bv[m].y, acc[m][n][2] + bv[m].z,
                          acc[m][n][3] + bv[m].w};
            if (res) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += (float)rv[m][n][e];
            }
            h4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov[e] = (_Float16)(relu ? relu_nan(v[e]) : v[e]);
            if (P < npix) *(h4 *)(dst + (size_t)P * ld + co0 + 16 * m) = ov;
        }
    }
}

// The lane's pixel of each N tile as y << 8 | x; a pixel at or past npix gets y = 64, so every
// tap of it is off the board and reads a zero row.
template <int H, int W>
__device__ __forceinline__ void pixel_coords(int prow0, int npix, int (&pyx)[4]) {
    constexpr int HW = H * W;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int P = prow0 + n * 16;
        const int pb = P / HW, rem = P - pb * HW, py = rem / W;
        pyx[n] = (P < npix ? py << 8 : 64 << 8) | (rem - py * W);
    }
}

// The per-layer conv (zc_net_conv3x3_packed_w_async at 64 channels): the tile's input rows from
// HBM into LDS, mfma_layer64, the epilogue straight from the accumulators to HBM.  The yardstick
// the fused tower is checked against, not a fast path.
template <int H, int W, int BPH, int CIN>
__global__ __launch_bounds__(256) void conv64_kernel(int nboards, const _Float16 *__restrict__ in,
                                                     const _Float16 *__restrict__ wp, const float *__restrict__ bias,
                                                     const _Float16 *__restrict__ res, _Float16 *__restrict__ out,
                                                     int relu) {
    constexpr int HW = H * W;
    static_assert(BPH * HW <= kTP, "tile too large");
    constexpr int C8 = CIN / 8, J = CIN / 32;
    extern __shared__ __attribute__((aligned(16))) _Float16 lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cw = wave & 1, l16 = lane & 15, q = lane >> 4;
    const int prow0 = 64 * (wave >> 1) + l16;
    const int b0 = blockIdx.x * BPH;
    const int npix = min(BPH, nboards - b0) * HW;
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const _Float16 *const wa = wp + (size_t)(2 * cw * 64 + lane) * 8;
    h8 a[4];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int m = 0; m < 2; ++m) a[2 * j + m] = *(const h8 *)(wa + (size_t)(j * 4 + m) * kFrag);
    {
        const _Float16 *src = in + (size_t)b0 * HW * CIN;
#pragma unroll
        for (int k = 0; k < kTP * C8 / 256; ++k) {
            const int i = tid + k * 256, row = i / C8, c8 = i - row * C8;
            const h8 t = *(const h8 *)(src + (size_t)min(row, npix - 1) * CIN + c8 * 8);
            *(h8 *)(lds + row * kLD + c8 * 8) = row < npix ? t : zero;
        }
        if (tid < kZR * kLD / 8) *(h8 *)(lds + kZero * kLD + tid * 8) = zero;
    }
    int pyx[4];
    pixel_coords<H, W>(prow0, npix, pyx);
    f4x acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f4x{0.0f, 0.0f, 0.0f, 0.0f};
    float4 bv[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) bv[m] = *(const float4 *)(bias + cw * 32 + 16 * m + 4 * q);
    __syncthreads();  // the input tile and the zero rows are in LDS
    mfma_layer64<H, W, J, J>(lds, 0, wa, nullptr, a, prow0, pyx, q, acc);
    const size_t o = (size_t)b0 * HW * kC;
    epilogue64(out + o, res ? res + o : nullptr, kC, bv, relu != 0, npix, prow0, cw * 32 + 4 * q, acc);
}

// The value head's sum of one board on one wave: lane l sums channels 8 (l & 7) .. + 7 over
// pixels l / 8, + 8, ...; the eight pixel groups are added across lanes, each channel's sum is
// weighted, divided by hw, and the eight channel groups are added.  The same arithmetic in the
// same order from HBM (value_head64_kernel) and from LDS (the tower): equal bits.
__device__ __forceinline__ float head64_sum(const _Float16 *act, int ld, int hw, const float *__restrict__ fcw,
                                            int lane) {
    const int c0 = (lane & 7) * 8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p = lane >> 3; p < hw; p += 8) {
        const h8 v = *(const h8 *)(act + (size_t)p * ld + c0);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += (float)v[e];
    }
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float t = s[e] + __shfl_xor(s[e], 8);
        t += __shfl_xor(t, 16);
        t += __shfl_xor(t, 32);
        d += t * fcw[c0 + e];
    }
    d /= (float)hw;
    for (int o = 4; o > 0; o >>= 1) d += __shfl_xor(d, o);
    return d;
}

__global__ __launch_bounds__(256) void value_head64_kernel(int n, int hw, const _Float16 *__restrict__ act,
                                                           const float *__restrict__ fcw, float fcb,
                                                           double *__restrict__ values, int raw) {
    const int i = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;  // a whole wave
    const float d = head64_sum(act + (size_t)i * hw * kC, kC, hw, fcw, lane);
    if (lane == 0) values[i] = raw ? (double)(d + fcb) : (double)tanhf(d + fcb);
}

// The policy head's 1x1 conv on the tower's output while it is in LDS: pw = the folded weights
// as 16x16x32 A fragments [mtiles][2 k-steps][64 lanes][8] (lane l of k-step j of M tile mt holds
// weight[16 mt + l % 16][32 j + 8 (l / 16) + e]; nets.pack_policy_1x1), pb [16 mtiles] fp32,
// out [n * H * W][16 mtiles] fp16.
struct TowerPolicy64 {
    const _Float16 *pw;
    const float *pb;
    _Float16 *out;
    int head_raw;  // test switch: the value head writes its pre-tanh sum
    int mtiles;    // output channels / 16 (2: the 64 -> 32 conv; 4: the 64 -> 64 logit conv)
    int relu;      // ReLU on the outputs (the linear head's conv) or not (logits)
};

// The fused tower (zc_net_tower_w_async and its kin at 64 channels): the stem and every residual
// block of a tile of boards in one workgroup, the activations in LDS from the input planes to the
// last layer,
//   layer 0 (stem)        buf1 (input planes, 32 channels) -> buf0
//   layer 2k+1 (conv1)    buf0 (x)                         -> buf1 (h)
//   layer 2k+2 (conv2)    buf1 (h)                         -> buf0 (x := relu(conv + bias + x), in
//                          place: a lane reads only the residual it overwrites, and no wave reads
//                          buf0 during conv2)
// with one barrier per layer (dst is complete before the next layer reads it; dst was the layer
// before's src, which every wave had finished reading at the previous barrier).
// CNT: the counted form's flag, as net_conv.hip's: `const int32_t *`, a trailing argument points
// at the row count on the device; nboards is then the capacity the grid was sized for, a
// workgroup whose first board is at or past min(*count, nboards) returns before it touches LDS,
// and the others run on the clamped count, so rows at or past it are neither read nor written.
template <int H, int W, int BPH, typename... CNT>
__global__ __launch_bounds__(256) void tower64_kernel(int nboards, int nconv, const _Float16 *__restrict__ in,
                                                      const _Float16 *__restrict__ wall,
                                                      const float *__restrict__ ball, _Float16 *__restrict__ out,
                                                      const float *__restrict__ fcw, float fcb,
                                                      double *__restrict__ values, TowerPolicy64 pol, CNT... cnt) {
    static_assert(sizeof...(CNT) <= 1, "at most one count argument");
    constexpr int HW = H * W;
    static_assert(BPH * HW <= kTP, "tile too large");
    constexpr int CIN0 = 32;
    constexpr size_t kW0 = (size_t)9 * CIN0 * kC, kW = (size_t)9 * kC * kC;  // halfs per layer
    extern __shared__ __attribute__((aligned(16))) _Float16 lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cw = wave & 1, l16 = lane & 15, q = lane >> 4;
    const int prow0 = 64 * (wave >> 1) + l16;
    const int b0 = blockIdx.x * BPH;
    if constexpr (sizeof...(CNT) == 1) {
        const int32_t *const count = (cnt, ...);
        nboards = min(max(*count, 0), nboards);
        if (b0 >= nboards) return;
    }
    const int npix = min(BPH, nboards - b0) * HW;
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const _Float16 *const wl0 = wall + (size_t)(2 * cw * 64 + lane) * 8;
    h8 a[4];
#pragma unroll
    for (int m = 0; m < 2; ++m) a[m] = *(const h8 *)(wl0 + (size_t)m * kFrag);
    {
        constexpr int C8 = CIN0 / 8;
        const _Float16 *src = in + (size_t)b0 * HW * CIN0;
#pragma unroll
        for (int k = 0; k < kTP * C8 / 256; ++k) {
            const int i = tid + k * 256, row = i / C8, c8 = i - row * C8;
            const h8 t = *(const h8 *)(src + (size_t)min(row, npix - 1) * CIN0 + c8 * 8);
            *(h8 *)(lds + (kBuf1 + row) * kLD + c8 * 8) = row < npix ? t : zero;
        }
        if (tid < kZR * kLD / 8) *(h8 *)(lds + kZero * kLD + tid * 8) = zero;
    }
    int pyx[4];
    pixel_coords<H, W>(prow0, npix, pyx);
    __syncthreads();  // the input tile and the zero rows are in LDS
    auto layer = [&](int l, auto j_tag) {
        constexpr int J = decltype(j_tag)::value;
        const int src = (l & 1) ? 0 : kBuf1, dst = (l & 1) ? kBuf1 : 0;
        const _Float16 *const wa = l == 0 ? wl0 : wl0 + kW0 + (size_t)(l - 1) * kW;
        const _Float16 *const wn = l + 1 < nconv ? wl0 + kW0 + (size_t)l * kW : nullptr;  // layer l + 1's
        // the pixel coordinates made opaque per layer, so that the 36 tap addresses are not
        // hoisted out of the layer loop into registers
        int py[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            py[n] = pyx[n];
            __asm__ volatile("" : "+v"(py[n]));
        }
        f4x acc[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = f4x{0.0f, 0.0f, 0.0f, 0.0f};
        float4 bv[2];  // in flight during the MFMA loop
#pragma unroll
        for (int m = 0; m < 2; ++m) bv[m] = *(const float4 *)(ball + (size_t)l * kC + cw * 32 + 16 * m + 4 * q);
        mfma_layer64<H, W, J, 2>(lds, src, wa, wn, a, prow0, py, q, acc);
        _Float16 *const d = lds + dst * kLD;
        epilogue64(d, l >= 2 && !(l & 1) ? d : nullptr, kLD, bv, true, npix, prow0, cw * 32 + 4 * q, acc);
        __syncthreads();
    };
    layer(0, std::integral_constant<int, 1>{});
    for (int l = 1; l < nconv; ++l) layer(l, std::integral_constant<int, 2>{});
    // the tower's output is the last layer's dst: buf0 (nconv is odd)
    if (values) {  // one wave per board
        for (int bi = wave; bi < npix / HW; bi += 4) {
            const float d = head64_sum(lds + bi * HW * kLD, kLD, HW, fcw, lane);
            if (lane == 0) values[b0 + bi] = pol.head_raw ? (double)(d + fcb) : (double)tanhf(d + fcb);
        }
    }
    if (pol.out) {
        // wave w takes N tiles 2 w and 2 w + 1 (16 pixels each); per M tile of 16 output channels
        // two MFMAs over the 64 channels, + bias, ReLU or not, fp16 -> [pixel][16 mtiles]
        const int nout = 16 * pol.mtiles;
        const bool relu = pol.relu != 0;
        for (int mt = 0; mt < pol.mtiles; ++mt) {
            h8 pa[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) pa[j] = *(const h8 *)(pol.pw + ((size_t)(mt * 2 + j) * 64 + lane) * 8);
            const float4 pbv = *(const float4 *)(pol.pb + 16 * mt + 4 * q);
            const float bb[4] = {pbv.x, pbv.y, pbv.z, pbv.w};
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int P = (2 * wave + t) * 16 + l16;
                f4x acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const h8 x = *(const h8 *)(lds + P * kLD + j * 32 + q * 8);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa[j], x, acc, 0, 0, 0);
                }
                if (P < npix) {
                    h4 ov;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {  // a NaN stays a NaN, with the ReLU or without
                        const float y = acc[e] + bb[e];
                        ov[e] = (_Float16)(relu ? relu_nan(y) : y);
                    }
                    *(h4 *)(pol.out + ((size_t)b0 * HW + P) * nout + 16 * mt + 4 * q) = ov;
                }
            }
        }
    }
    if (out) {  // -> HBM, whole 128-byte rows
#pragma unroll
        for (int k = 0; k < kTP * (kC / 8) / 256; ++k) {
            const int i = tid + k * 256, P = i >> 3, c0 = (i & 7) * 8;
            if (P < npix) *(h8 *)(out + ((size_t)b0 * HW + P) * kC + c0) = *(const h8 *)(lds + P * kLD + c0);
        }
    }
}

// [9][64][cin] -> fragments: packed[(((tap * J + j) * 4 + mt) * 64 + lane) * 8 + e] =
// w[tap][16 mt + lane % 16][32 j + 8 (lane / 16) + e], J = cin / 32.
__global__ void pack_conv64_weight_kernel(int cin, const _Float16 *__restrict__ w, _Float16 *__restrict__ packed) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // one 8-half piece
    const int J = cin / 32;
    if (i >= 9 * J * 4 * 64) return;
    const int lane = i & 63, mt = (i >> 6) & 3, j = (i >> 8) % J, tap = (i >> 8) / J;
    const int row = mt * 16 + (lane & 15), k0 = j * 32 + 8 * (lane >> 4);
    *(h8 *)(packed + (size_t)i * 8) = *(const h8 *)(w + ((size_t)tap * kC + row) * cin + k0);
}

template <int H, int W, int BPH>
void launch_tower64(int n, int nconv, const void *in, const void *wall, const float *ball, void *out, const float *fcw,
                    float fcb, double *values, TowerPolicy64 pol, const int32_t *count, hipStream_t s) {
    const dim3 grid((n + BPH - 1) / BPH), block(256);
    if (count)
        hipLaunchKernelGGL((tower64_kernel<H, W, BPH, const int32_t *>), grid, block, kTowerLds, s, n, nconv,
                           (const _Float16 *)in, (const _Float16 *)wall, ball, (_Float16 *)out, fcw, fcb, values, pol,
                           count);
    else
        hipLaunchKernelGGL((tower64_kernel<H, W, BPH>), grid, block, kTowerLds, s, n, nconv, (const _Float16 *)in,
                           (const _Float16 *)wall, ball, (_Float16 *)out, fcw, fcb, values, pol);
}

template <int H, int W, int BPH, int CIN>
void launch_conv64(int n, const void *in, const void *wp, const float *bias, const void *res, void *out, int relu,
                   hipStream_t s) {
    hipLaunchKernelGGL((conv64_kernel<H, W, BPH, CIN>), dim3((n + BPH - 1) / BPH), dim3(256), kConvLds, s, n,
                       (const _Float16 *)in, (const _Float16 *)wp, bias, (const _Float16 *)res, (_Float16 *)out, relu);
}

}  // namespace

bool launch_net64_conv3x3_packed(int n, int h, int w, int cin, const void *in, const void *wp, const float *bias,
                                 const void *res, void *out, int relu, hipStream_t s) {
    if (h == 8 && w == 8 && cin == 64) launch_conv64<8, 8, 2, 64>(n, in, wp, bias, res, out, relu, s);
    else if (h == 8 && w == 8 && cin == 32) launch_conv64<8, 8, 2, 32>(n, in, wp, bias, res, out, relu, s);
    else if (h == 6 && w == 7 && cin == 64) launch_conv64<6, 7, 3, 64>(n, in, wp, bias, res, out, relu, s);
    else if (h == 6 && w == 7 && cin == 32) launch_conv64<6, 7, 3, 32>(n, in, wp, bias, res, out, relu, s);
    else return false;
    return true;
}

bool launch_net64_tower(int n, int h, int w, int cin0, int nconv, const void *in, const void *wall, const float *ball,
                        void *out, const float *fcw, float fcb, double *values, const void *pw, const float *pb,
                        void *pout, hipStream_t s, int pol_channels, int pol_relu, const int32_t *count) {
    if (cin0 != 32 || nconv < 1 || !(nconv & 1)) return false;
    if (pout && pol_channels != 32 && pol_channels != 64) return false;
    const TowerPolicy64 pol{(const _Float16 *)pw, pb, (_Float16 *)pout, net_head_raw(), pol_channels / 16,
                            pol_relu ? 1 : 0};
    if (h == 8 && w == 8) launch_tower64<8, 8, 2>(n, nconv, in, wall, ball, out, fcw, fcb, values, pol, count, s);
    else if (h == 6 && w == 7) launch_tower64<6, 7, 3>(n, nconv, in, wall, ball, out, fcw, fcb, values, pol, count, s);
    else return false;
    return true;
}

bool launch_net64_pack_conv_weight(int cin, const void *w, void *packed, hipStream_t s) {
    if (cin != 32 && cin != 64) return false;
    const int n = 9 * (cin / 32) * 4 * 64;
    hipLaunchKernelGGL(pack_conv64_weight_kernel, dim3((n + 255) / 256), dim3(256), 0, s, cin, (const _Float16 *)w,
                       (_Float16 *)packed);
    return true;
}

void launch_net64_value_head(int n, int hw, const void *act, const float *fcw, float fcb, double *values,
                             hipStream_t s) {
    hipLaunchKernelGGL(value_head64_kernel, dim3((unsigned)(((int64_t)n * 64 + 255) / 256)), dim3(256), 0, s, n, hw,
                       (const _Float16 *)act, fcw, fcb, values, net_head_raw());
}

}  // namespace zc
