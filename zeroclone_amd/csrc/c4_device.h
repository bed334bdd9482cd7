// c4_device.h — device-side building blocks shared by the Connect4 search kernels
// (c4_search.hip: fused rollout search; c4_ext.hip: stepwise search with caller values).
// Included by exactly those translation units; everything is internal to each of them.
#pragma once
#include <math.h>

#include "c4_order_table.h"
#include "zc_internal.h"

namespace zc {
namespace {

__constant__ uint32_t d_order[128] = {ZC_C4_ORDER_LIST};

constexpr uint32_t kRingMask = kRingWords - 1;
constexpr uint64_t kBottom = 0x0000040810204081ull;  // bit 7c: bottom cell of column c
constexpr uint64_t kFull = kBottom * 0x3Full;        // the 42 playable cells
constexpr uint64_t kTop = kBottom << 5;              // top playable cell of each column
// LDS tables: move-list order[128] u32, then sel[128][8] u8 (the r-th set bit of a 7-bit mask),
// then draw_order[128] u32 (the order words indexed by a word's top three tempered bits)
constexpr int kTabBytes = 128 * 4 + 128 * 8 + 128 * 4;

// Untried moves of a node (record +4 / Fresh.u): bit i (i < 7) set while move i of the
// node's move list is untried; bits 28..31 = number of moves.  The reference keeps the
// untried INDICES in list order and lets random.choice pick the r-th (mcts.cpp:67-72); the
// r-th remaining index is the r-th set bit of the mask (one ballot over lanes 0..6).
__device__ __forceinline__ uint32_t untried_init(uint32_t n) { return ((1u << n) - 1u) | (n << 28); }
__device__ __forceinline__ uint32_t untried_count(uint32_t u) { return (uint32_t)__popc(u & 0x7Fu); }

// Fill the LDS tables (whole workgroup): s_order = d_order; sel[m][r] = position of the r-th
// set bit of m (7 when m has fewer), right after s_order; then draw_order.
// draw_order[m]: random.choice over the n moves of legal set m draws getrandbits(k) = t >> (3 - k)
// from a word's top three tempered bits t (k = n.bit_length() <= 3) and accepts it when < n,
// i.e. when t < n << (3 - k).  The word keeps that threshold in bits 24..27 and, in bits
// 3t..3t+2, the column of move t >> (3 - k) for every accepted t: a rollout block tests and
// maps t as it stands, without the shift (and without computing it from n).
__device__ __forceinline__ void load_tables(uint32_t *s_order) {
    for (int i = (int)threadIdx.x; i < 128; i += blockDim.x) {
        const uint32_t o = d_order[i], n = (o >> 24) & 15u;
        s_order[i] = o;
        const uint32_t sh = n ? (uint32_t)__builtin_clz(n) - 29u : 0u;
        uint32_t e = (n << sh) << 24;
        for (uint32_t t = 0; t < (n << sh); ++t) e |= ((o >> (3u * (t >> sh))) & 7u) << (3u * t);
        s_order[128 + 256 + i] = e;
    }
    uint8_t *const s_sel = (uint8_t *)(s_order + 128);
    for (int i = (int)threadIdx.x; i < 1024; i += blockDim.x) {
        const uint32_t m = (uint32_t)i >> 3, r = (uint32_t)i & 7u;
        uint32_t c = 0, pos = 7;
        for (uint32_t b = 0; b < 7; ++b)
            if ((m >> b) & 1u) {
                if (c == r) {
                    pos = b;
                    break;
                }
                ++c;
            }
        s_sel[i] = (uint8_t)pos;
    }
}
__device__ __forceinline__ const uint8_t *sel_table(const uint32_t *s_order) { return (const uint8_t *)(s_order + 128); }
__device__ __forceinline__ const uint32_t *draw_order_table(const uint32_t *s_order) { return s_order + 128 + 256; }
constexpr int kWin = 64;                             // RNG window: one word per lane
// LDS bytes after the leaves' paths: select_flush stores a path with all 64 lanes, so the
// last leaf's lanes >= kMaxDepth land here
constexpr int kPathSpill = 2 * (64 - kMaxDepth) + 24;

// ------------------------------------------------------------------ wave helpers
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t uni64(uint64_t x) {
    return ((uint64_t)uni((uint32_t)(x >> 32)) << 32) | (uint64_t)uni((uint32_t)x);
}
__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }
// lane-wise select by a wave mask in SGPRs: bit `lane` of m set -> b, else a (or 0)
__device__ __forceinline__ uint32_t mask_sel(uint64_t m, uint32_t a, uint32_t b) {
    uint32_t r;
    __asm__("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
    return r;
}
__device__ __forceinline__ uint32_t mask_sel0(uint64_t m, uint32_t b) {
    uint32_t r;
    __asm__("v_cndmask_b32 %0, 0, %1, %2" : "=v"(r) : "v"(b), "s"(m));
    return r;
}
// x + 1 in the lanes of wave mask m (the mask as the add's carry-in)
__device__ __forceinline__ uint32_t add_in_mask(uint32_t x, uint64_t m) {
    uint32_t r;
    uint64_t co;
    __asm__("v_addc_co_u32_e64 %0, %1, 0, %2, %3" : "=v"(r), "=s"(co) : "v"(x), "s"(m));
    return r;
}
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m) {  // set bits of m in lanes below this one
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Wait for x's load here.  Stores and loads share gfx950's in-order vector-memory counter, so
// a load still in flight where two paths join makes the compiler's wait at the join (vmcnt(0))
// also drain every store issued since — on the path that never loaded anything.  Waiting on
// the loading path itself keeps the other path free of it.
template <class T>
__device__ __forceinline__ void vmem_ready(T &x) {
    asm volatile("" : "+v"(x));
}

__device__ __forceinline__ void wave_mem_order() {
    // Same-wave hand-offs through memory (one lane stores, another loads) are ordered by
    // program order on gfx950 (wavefront scope needs no cache action); this only stops the
    // compiler from moving memory operations across the point.
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

template <int CTRL>
__device__ __forceinline__ int dpp(int x) {
    return __builtin_amdgcn_mov_dpp(x, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double dpp(double x) {
    const int lo = dpp<CTRL>(__double2loint(x));
    const int hi = dpp<CTRL>(__double2hiint(x));
    return __hiloint2double(hi, lo);
}

// First maximum over lanes 0..7 (ties -> lower slot), as mcts.cpp:55-58 (`v > best_val`,
// scanning slots in order).  Three DPP steps inside each 8-lane half row: xor 1, xor 2,
// mirror; afterwards every lane of the half row holds the winner.
template <class T>
__device__ __forceinline__ void argmax_step(T &v, int &i, T ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}
template <class T>
__device__ __forceinline__ void argmax8(T &v, int &i) {
    argmax_step(v, i, dpp<0xB1>(v), dpp<0xB1>(i));    // quad_perm [1,0,3,2]
    argmax_step(v, i, dpp<0x4E>(v), dpp<0x4E>(i));    // quad_perm [2,3,0,1]
    argmax_step(v, i, dpp<0x141>(v), dpp<0x141>(i));  // row_half_mirror
}

// The same first maximum for the walk's UCT scores: the maximum over lanes 0..7 by three DPP
// v_max_f64 steps (no index carried, no per-step branch: the compare-and-swap form compiled to
// exec-mask juggling, ~8 SALU per step), then the first slot holding it from one ballot.  The
// scores are finite or -inf (never NaN), and a slot holding the maximum compares equal to it,
// so this is the strict `>` scan of mcts.cpp:55-58 (+0 and -0 compare equal there too).
// Returns the maximum; *first = the lowest slot k < 8 with v == max.
__device__ __forceinline__ double max8_first(double v, int *first) {
    double m = v;
    m = fmax(m, dpp<0xB1>(m));   // quad_perm [1,0,3,2]
    m = fmax(m, dpp<0x4E>(m));   // quad_perm [2,3,0,1]
    m = fmax(m, dpp<0x141>(m));  // row_half_mirror
    *first = __builtin_ctzll((__ballot(v == m) & 0xFFull) | 0x100ull);
    return m;
}

// ------------------------------------------------------------------ Connect4 bitboards
__device__ __forceinline__ uint64_t drop_bit(uint64_t occ, int col) {
    // c4_backend.play_move (:14-23): lowest empty row of `col`; a full column drops nothing.
    const int s = 7 * col;
    return (occ + (1ull << s)) & (0x3Full << s);
}

__device__ __forceinline__ int legal_mask(uint64_t occ) {
    // c4_backend.get_legal_moves (:49-50): column c is legal while its top cell is empty.
    // Gather bit 7c -> bit c with one multiply: the 49 partial products t_c * 2^(56-6i) land
    // on distinct bit positions (7c - 6i is injective on 0..6 x 0..6), so nothing carries
    // and bits 56..62 of the product are exactly t_0..t_6.
    const uint64_t t = (~occ & kTop) >> 5;  // bit 7c
    return (int)((t * 0x0104104104100000ull) >> 56) & 0x7F;
}

__device__ __forceinline__ bool has_four(uint64_t b) {
    // c4_backend.check_win (:25-44) for one token: any horizontal, vertical or diagonal run.
    uint64_t m = b & (b >> 7);
    uint64_t r = m & (m >> 14);
    m = b & (b >> 1);
    r |= m & (m >> 2);
    m = b & (b >> 6);
    r |= m & (m >> 12);
    m = b & (b >> 8);
    r |= m & (m >> 16);
    return r != 0;
}

// ------------------------------------------------------------------ CPython MT19937
__device__ __forceinline__ uint32_t temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// The game's stream lives in a ring of RAW MT words x[p] (absolute position p, slot
// p % kRingWords).  The recurrence x[p] = x[p-227] ^ twist(x[p-624], x[p-623]) regenerates
// it kChunk words at a time, all lanes in parallel (every input is >= 227 words older).
// Three 64-word windows sit in registers: wt (tempered, the window holding the next word),
// wn (tempered, the one after) and wx (raw, in flight from the ring), so a 64-word view
// starting at ANY position of wt is two lane permutes away (rng_view).
struct Rng {
    uint32_t *ring;
    uint32_t base;   // low 32 bits of the absolute position at the search's start (use0)
    int32_t wrel;    // window start - use0 (a multiple of 64 in absolute terms; may be < 0)
    uint32_t off;    // next word to consume = window start + off, off in [0, 128)
    int32_t grel;    // words generated so far - use0
    uint32_t wt;     // tempered x[window start + lane]
    uint32_t wn;     // tempered x[window start + 64 + lane]
    uint32_t wx;     // raw x[window start + 128 + lane], in flight until the window advances
    __device__ __forceinline__ int32_t use() const { return wrel + (int32_t)off; }  // relative to use0
    __device__ __forceinline__ uint32_t slot(int32_t rel) const { return (base + (uint32_t)rel) & kRingMask; }
    __device__ __forceinline__ uint32_t cur() const { return wt; }
};

__device__ __forceinline__ int32_t rng_generate(uint32_t *ring, uint32_t base, int32_t grel, int32_t target) {
    const uint32_t lane = lane_id();
    constexpr int K = kChunk / 64;
    while (grel < target) {
        // every input of the chunk is >= 227 words older than any output: load all, then store
        uint32_t a[K], b[K], m[K];
        const uint32_t p0 = base + (uint32_t)grel + lane;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t p = p0 + 64u * k;
            a[k] = ring[(p - 624) & kRingMask];
            b[k] = ring[(p - 623) & kRingMask];
            m[k] = ring[(p - 227) & kRingMask];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t p = p0 + 64u * k;
            const uint32_t y = (a[k] & 0x80000000u) | (b[k] & 0x7fffffffu);
            ring[p & kRingMask] = m[k] ^ (y >> 1) ^ ((b[k] & 1u) ? 0x9908b0dfu : 0u);
        }
        grel += kChunk;
        wave_mem_order();
    }
    return grel;
}

__device__ __forceinline__ void rng_fill(Rng &r, int32_t target) {
    if (r.grel < target) r.grel = rng_generate(r.ring, r.base, r.grel, target);
}

// use0 / gen0: absolute positions (words consumed / generated) from the game's rngpos.
__device__ __forceinline__ void rng_open(Rng &r, uint32_t *ring, uint64_t use0, uint64_t gen0) {
    r.ring = ring;
    r.base = (uint32_t)use0;
    r.grel = (int32_t)(gen0 - use0);
    r.off = (uint32_t)use0 & (uint32_t)(kWin - 1);
    r.wrel = -(int32_t)r.off;
    rng_fill(r, r.wrel + 3 * kWin);
    r.wt = temper(r.ring[r.slot(r.wrel + (int32_t)lane_id())]);
    r.wn = temper(r.ring[r.slot(r.wrel + kWin + (int32_t)lane_id())]);
    r.wx = r.ring[r.slot(r.wrel + 2 * kWin + (int32_t)lane_id())];
    vmem_ready(r.wx);
}

// Move the windows on by 64 words (precondition: off >= 64).
__device__ __forceinline__ void rng_advance(Rng &r) {
    r.wrel += kWin;
    r.off -= (uint32_t)kWin;
    r.wt = r.wn;
    r.wn = temper(r.wx);
    if (r.grel < r.wrel + 3 * kWin) rng_fill(r, r.wrel + 3 * kWin);
    r.wx = r.ring[r.slot(r.wrel + 2 * kWin + (int32_t)lane_id())];
    vmem_ready(r.wx);  // once per 64 words, instead of at every later join
}

// The 64 tempered words from the next unconsumed one on: lane l = word off + l of the
// window (precondition: off < 64).  Word off + l sits in lane (off + l) % 64 of wt or of wn,
// and every one of those 64 source lanes is read by exactly one lane: lane s by the word
// s (of wt) when s >= off, by the word 64 + s (of wn) otherwise.  So the SOURCE lane picks
// the window, and one lane permute gathers the view.
__device__ __forceinline__ uint32_t rng_view(const Rng &r) {
    const uint32_t lane = lane_id();
    const uint32_t src = lane < r.off ? r.wn : r.wt;
    // ds_bpermute reads the lane from address bits 7:2 only
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane + r.off) << 2), (int)src);
}

// rngpos after the search: {use0 + use(), use0 + grel}
__device__ __forceinline__ void rng_close(const Rng &r, uint64_t use0, uint64_t *rngpos) {
    rngpos[0] = use0 + (uint64_t)(int64_t)r.use();
    rngpos[1] = use0 + (uint64_t)(int64_t)r.grel;
}

// ------------------------------------------------------------------ the stream in LDS
// The fused search (c4_search_kernel) keeps its game's stream in LDS instead of the HBM ring,
// in two rings per wave: the RAW ring (1024 words), which the recurrence and the hand-over
// need, and beside it the DRAW ring, one byte per word holding temper(x) >> 29.  Every
// consumer of the stream in this search reads only the top k <= 3 bits of a tempered word
// (_randbelow(n) with n <= 7), so a 64-word view from ANY position is one byte read per lane
// (rng_view): no windows in registers, no lane permute, no window select.
// Positions are kept relative to org = use0 & ~3 (use0 = the stream's position at the launch's
// start): word org + q sits at slot q % 1024 of both rings, and the draw ring's first 64 bytes
// are repeated after its end, so a view reads the bytes (q % 1024) + lane without a wrap.
// The recurrence runs in bulk (lrng_refill): 224 words a step, lane l < 56 producing the four
// words G + 4l .. G + 4l + 3 and their four draws, whenever fewer than 64 generated words lie
// ahead of the next unconsumed one.
//   * 224 <= 227: every input of a step (x[p-624], x[p-623], x[p-227]) is older than every
//     output, so a step loads, computes, stores.  (256 would read x[p-227] inside itself; two
//     dependent half-steps would pay the step's fixed costs twice.)
//   * G - org is a multiple of 4 (lrng_open makes it one), and so are 624 and 228: each lane's
//     four inputs x[p-624 ..] are one aligned quad, x[p-227 ..] the last three words of one,
//     and a quad never straddles the ring's wrap.
//   * the stream runs at most 63 + 224 = 287 words ahead of the next word U, so the ring
//     [G - 1024, G) always holds the 624-word block of word U-1 (it starts at >= U - 624 >=
//     G - 911), which lrng_close hands over, and the draws of [U, U + 64).
//   * words < 624 are never produced by the recurrence (they are seeded): a stream's
//     generated mark is >= 624 from the start (zc_rng_seed / zc_rng_set_state), the refill
//     starts there, and the words already in the ring are kept — only their draws are made.
// The HBM ring is the hand-over format to every other kernel and to zc_rng_get_state: the
// kernel loads its game's last 1024 words at the start and, at the end, writes back the
// words [min(U & ~63, block start, G' - 624), G') (U = next word, block = the 624-word block
// holding word U-1, G' = words generated, at least that block's end) — what rng_open,
// zc_rng_get_state and the recurrence read.
constexpr int kLRingWords = 1024;
constexpr uint32_t kLRingMask = kLRingWords - 1;
constexpr int kLRingBytes = kLRingWords * 4;
constexpr int kLDrawBytes = kLRingWords + kWin;  // the draw ring: one byte per word, the first 64 again
constexpr int kLStepLanes = 56;                  // lanes of a refill step, four words each
constexpr int kLStep = 4 * kLStepLanes;          // words per refill step
static_assert(kLStep <= 227 && kLStep % 4 == 0, "a refill step's inputs must all be older than its outputs");
static_assert(kLRingWords - 624 - (kWin - 1 + kLStep) >= 0, "the block of word U-1 must stay in the ring");

// The top three bits of the tempered word, temper(x) >> 29, from the raw word: temper's last
// step (y ^= y >> 18) cannot reach them, its third reaches them through bits 16..14 (the mask
// 0xefc60000 has all of 31..29 set), and of its second step only bits 31 and 14 matter (the
// mask 0x9d2c5680 at 31, 30, 29, 16, 15, 14 is 1, 0, 0, 0, 0, 1).
__host__ __device__ constexpr uint32_t mt_draw3(uint32_t x) {
    const uint32_t y = x ^ (x >> 11);
    const uint32_t z = y ^ ((y << 7) & 0x80004000u);
    return (z ^ (z << 15)) >> 29;
}
__host__ __device__ constexpr uint32_t mt_temper_ref(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}
// both are GF(2)-linear in x: equal on zero and on the 32 one-bit words, equal on every word
__host__ __device__ constexpr bool mt_draw3_matches_temper() {
    if (mt_draw3(0u) != mt_temper_ref(0u) >> 29) return false;
    for (int b = 0; b < 32; ++b)
        if (mt_draw3(1u << b) != mt_temper_ref(1u << b) >> 29) return false;
    return true;
}
static_assert(mt_draw3_matches_temper(), "mt_draw3 is not temper(x) >> 29");

struct LRng {
    uint32_t *lds;      // this wave's rings: kLRingWords raw words, then kLDrawBytes of draws
    const uint8_t *dl;  // the draw ring + this lane: a view reads dl[(next word - org) % 1024]
    int32_t urel;       // next word to consume - org
    int32_t lim;        // words generated - org - 64: a view needs urel <= lim
    int32_t uoff;       // use0 - org (0..3)
    __device__ __forceinline__ int32_t use() const { return urel - uoff; }  // words consumed since use0
    __device__ __forceinline__ int32_t grel() const { return lim + kWin; }
    __device__ __forceinline__ uint8_t *draw() const { return (uint8_t *)(lds + kLRingWords); }
};

// (the bit select as one v_bfi_b32, which the compiler otherwise splits into two ANDs and an OR
// once it has merged the shift into them, and the conditional constant as a sign-extended bit
// ANDed with it instead of a compare and a select)
__device__ __forceinline__ uint32_t mt_twist(uint32_t a, uint32_t b, uint32_t m) {
    uint32_t y;
    __asm__("v_bfi_b32 %0, %1, %2, %3" : "=v"(y) : "s"(0x7fffffffu), "v"(b), "v"(a));
    const uint32_t mag = (uint32_t)((int32_t)(b << 31) >> 31) & 0x9908b0dfu;
    return m ^ (y >> 1) ^ mag;
}

// the draws of the four words at slot q (a multiple of 4), a byte each; the first 64 repeated
__device__ __forceinline__ void lrng_put_draws(const LRng &r, uint32_t q, uint32_t x0, uint32_t x1, uint32_t x2,
                                               uint32_t x3) {
    const uint32_t d = mt_draw3(x0) | (mt_draw3(x1) << 8) | (mt_draw3(x2) << 16) | (mt_draw3(x3) << 24);
    *(uint32_t *)(r.draw() + q) = d;
    if (q < (uint32_t)kWin) *(uint32_t *)(r.draw() + kLRingWords + q) = d;
}

// One refill step: the words [G, G + 224) and their draws, G = org + grel().  Lane l's words
// are p .. p+3 with p = grel() + 4l: x[p+j-624] and x[p+j-623] come from the quad at p - 624
// and the word after it, x[p+j-227] from the last three words of the quad at p - 228 and the
// word after it.  (Word by word, which the compiler pairs up: this toolchain's register
// allocator crashes on the 16-byte form of these accesses under the ILP scheduler.)
__device__ __forceinline__ void lrng_refill(LRng &r) {
    const uint32_t lane = lane_id();
    const uint32_t p = (uint32_t)r.grel() + 4u * lane;
    const uint32_t *pa = r.lds + ((p - 624u) & kLRingMask), *pm = r.lds + ((p - 228u) & kLRingMask);
    const uint32_t a0 = pa[0], a1 = pa[1], a2 = pa[2], a3 = pa[3], a4 = r.lds[(p - 620u) & kLRingMask];
    const uint32_t m1 = pm[1], m2 = pm[2], m3 = pm[3], m4 = r.lds[(p - 224u) & kLRingMask];
    const uint32_t x0 = mt_twist(a0, a1, m1), x1 = mt_twist(a1, a2, m2), x2 = mt_twist(a2, a3, m3),
                   x3 = mt_twist(a3, a4, m4);
    if (lane < (uint32_t)kLStepLanes) {  // the lanes past the step read words not yet generated
        uint32_t *px = r.lds + (p & kLRingMask);
        px[0] = x0;
        px[1] = x1;
        px[2] = x2;
        px[3] = x3;
        lrng_put_draws(r, p & kLRingMask, x0, x1, x2, x3);
    }
    r.lim += kLStep;
    wave_mem_order();
}

// Generate the words [g, end) in the ring (positions relative to org), 64 at a time (every
// input is >= 227 older); raw words only.
__device__ __forceinline__ void lrng_generate(uint32_t *lds, int64_t g, int64_t end) {
    const uint32_t lane = lane_id();
    for (; g < end; g += 64) {
        const uint32_t p = (uint32_t)g + lane;
        const uint32_t a = lds[(p - 624) & kLRingMask], b = lds[(p - 623) & kLRingMask],
                       m = lds[(p - 227) & kLRingMask];
        if (g + lane < end) lds[p & kLRingMask] = mt_twist(a, b, m);
        wave_mem_order();
    }
}

// use0 / gen0: absolute positions (words consumed / generated) from the game's rngpos.
// Words already generated (and the seeded block 0..623, which no recurrence produces) are
// kept: the refill starts at the generated mark, and the draws of the loaded words are made here.
// lds: kLRingBytes + kLDrawBytes of this wave's LDS, 16-byte aligned.
__device__ __forceinline__ void lrng_open(LRng &r, uint32_t *lds, const uint32_t *ring, uint64_t use0, uint64_t gen0) {
    const uint32_t lane = lane_id();
    const uint64_t org = use0 & ~(uint64_t)3;
    r.lds = lds;
    r.dl = r.draw() + lane;
    r.uoff = (int32_t)(use0 - org);
    r.urel = r.uoff;
    const uint64_t w0 = use0 & ~(uint64_t)(kWin - 1), target = w0 + 192;
    // the ring can take every word up to gen0 when gen0 - w0 <= 960 (always after this
    // kernel's own close: <= 686); an HBM kernel's lookahead may go further, and then its
    // ring is valid throughout, so the words past the first window are generated again
    uint64_t g = gen0 <= w0 + 960 ? gen0 : (target < 624 ? 624 : target);
    for (uint32_t i = lane; i < (uint32_t)kLRingWords; i += 64) {
        const uint32_t p = (uint32_t)g - (uint32_t)kLRingWords + i;
        lds[(p - (uint32_t)org) & kLRingMask] = ring[p & kRingMask];
    }
    wave_mem_order();
    // the first view's words, and a generated mark that is a multiple of 4 for the refill (every
    // writer of rngpos leaves one: 624, an HBM chunk of 192, a window of 64 or a refill step;
    // not assumed)
    if (g < use0 + kWin || (g & 3u)) {
        const uint64_t ge = ((g < use0 + kWin ? use0 + kWin : g) + 3u) & ~(uint64_t)3u;
        lrng_generate(lds, (int64_t)(g - org), (int64_t)(ge - org));
        g = ge;
    }
    // the draws of all 1024 words in the ring, four per lane and pass ([use0, g) is what the views read)
    for (uint32_t q = 4u * lane; q < (uint32_t)kLRingWords; q += 256u)
        lrng_put_draws(r, q, lds[q], lds[q + 1], lds[q + 2], lds[q + 3]);
    wave_mem_order();
    r.lim = (int32_t)(int64_t)(g - org) - kWin;
}

// The next 64 words' draws, lane l = temper(word next + l) >> 29: one byte read per lane at a
// uniform offset (precondition: urel <= lim, what rng_need establishes).
__device__ __forceinline__ uint32_t rng_view(const LRng &r) { return r.dl[(uint32_t)r.urel & kLRingMask]; }

// Consume w words without reading them (the walk-replay diagnostic: a flush's recorded
// rollout words), then refill until a view can be taken again.
__device__ __forceinline__ void lrng_skip(LRng &r, uint32_t w) {
    r.urel += (int32_t)w;
    while (r.urel > r.lim) lrng_refill(r);
}

// What the code shared by the two streams (select_flush, c4_rollouts) asks of either:
//   rng_need(r)       make a view available (at most 64 words were consumed since the last call)
//   rng_view(r)       lane l: word `next + l`, as its top ViewBits<R>::kBits tempered bits
//   rng_eat(r, w)     consume w <= 64 words of the view
//   draw_shift<R>(n)  a view value >> this = getrandbits(n.bit_length()); n >= 1 (n <= 7 for the LDS stream)
__device__ __forceinline__ void rng_need(Rng &r) {
    if (r.off >= (uint32_t)kWin) rng_advance(r);
}
__device__ __forceinline__ void rng_need(LRng &r) {
    if (r.urel > r.lim) lrng_refill(r);
}
__device__ __forceinline__ void rng_eat(Rng &r, uint32_t w) { r.off += w; }
__device__ __forceinline__ void rng_eat(LRng &r, uint32_t w) { r.urel += (int32_t)w; }
template <class R>
struct ViewBits {
    static constexpr uint32_t kBits = 32;  // whole tempered words
};
template <>
struct ViewBits<LRng> {
    static constexpr uint32_t kBits = 3;  // the draw ring's bytes
};
template <class R>
__device__ __forceinline__ uint32_t draw_shift(uint32_t n) {
    return (uint32_t)__builtin_clz(n) - (32u - ViewBits<R>::kBits);
}

// Write the stream back to the game's HBM ring and rngpos (see above).
__device__ __forceinline__ void lrng_close(const LRng &r, uint32_t *ring, uint64_t use0, uint64_t *rngpos) {
    const uint32_t lane = lane_id();
    const uint64_t org = use0 & ~(uint64_t)3;
    const uint64_t U = org + (uint64_t)(int64_t)r.urel;
    uint64_t G = org + (uint64_t)(int64_t)r.grel();
    const uint64_t blk = U ? (U - 1) / 624 : 0;
    const uint64_t bend = (blk + 1) * 624;
    wave_mem_order();
    if (G < bend) {
        lrng_generate(r.lds, (int64_t)(G - org), (int64_t)(bend - org));
        G = bend;
    }
    // what rng_open reads (the window of U), what zc_rng_get_state reads (U-1's block) and
    // what the recurrence reads next (the last 624 words).  All of it is in the ring [G - 1024,
    // G): G = the block's end gives at most 623 + 63 words; a G past it was left by a refill
    // (G <= U + 287) or loaded at the start from an HBM kernel (rng_fill: G < U + 384), and the
    // start is >= U - 624: at most 911 (1007) words
    const uint64_t wu = U & ~(uint64_t)(kWin - 1);
    uint64_t start = wu < blk * 624 ? wu : blk * 624;
    start = start < G - 624 ? start : G - 624;
    for (uint64_t q = start + lane; q < G; q += 64)
        ring[(uint32_t)q & kRingMask] = r.lds[((uint32_t)q - (uint32_t)org) & kLRingMask];
    if (lane == 0) {
        rngpos[0] = U;
        rngpos[1] = G;
    }
}

// random._randbelow_with_getrandbits(n), 1 <= n < 2**31: k = n.bit_length(); draw
// getrandbits(k) = word >> (32-k) until < n.  All window words are tested at once; the
// first accepted one (in stream order) is the draw, and everything before it is consumed.
template <class R>
__device__ __forceinline__ uint32_t rng_below(R &r, uint32_t n) {
    const uint32_t sh = (uint32_t)__clz(n);
    const uint32_t lane = lane_id();
    for (;;) {
        if (r.off >= (uint32_t)kWin) rng_advance(r);
        const uint32_t v = r.cur() >> sh;
        // one compare: words before `off` get bit 31 set (never < n)
        const uint64_t bal = __ballot((v | ((lane - r.off) & 0x80000000u)) < n);
        if (bal) {
            const int f = __builtin_ctzll(bal);
            r.off = (uint32_t)f + 1;
            return (uint32_t)__builtin_amdgcn_readlane((int)v, f);
        }
        r.off = kWin;
    }
}

// random.choice(untried) of an expansion (policy_functions.py:12 with the untried list in
// list order, mcts.cpp:67-72): rng_below(n) as above, but every lane also looks up row[v]
// (row = sel[untried mask]: the v-th untried move) for its own candidate word, so the move
// index of the accepted draw is a readlane of that lookup (n <= 7, so v < 8).
template <class R>
__device__ __forceinline__ uint32_t rng_below_pick(R &r, uint32_t n, const uint8_t *row) {
    const uint32_t sh = (uint32_t)__clz(n);
    const uint32_t lane = lane_id();
    for (;;) {
        if (r.off >= (uint32_t)kWin) rng_advance(r);
        const uint32_t v = r.cur() >> sh;
        const uint32_t pick = row[v & 7u];
        const uint64_t bal = __ballot((v | ((lane - r.off) & 0x80000000u)) < n);
        if (bal) {
            const int f = __builtin_ctzll(bal);
            r.off = (uint32_t)f + 1;
            return (uint32_t)__builtin_amdgcn_readlane((int)pick, f);
        }
        r.off = kWin;
    }
}

// Per-search counters, accumulated in VGPRs (off the scalar unit, no SGPRs): add() counts a
// uniform value in lane 0.  plies and blocks also take lane-parallel terms (a rollout's plies
// in its leaf's lane), so their totals are the sums over the wave: total().
struct Counters {
    int32_t expansions = 0, depth_sum = 0, plies = 0, blocks = 0;
    __device__ __forceinline__ void add(int32_t &c, int32_t v) { c += (lane_id() == 0) ? v : 0; }
    __device__ __forceinline__ static int32_t total(int32_t c) {  // the same in every lane
        for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
        return c;
    }
};

// A pending leaf, kept in LDS between the phases of a flush (16-byte aligned: the rollout
// reads both boards in one LDS access).
struct alignas(16) Leaf {
    uint64_t p0, p1;  // stones of 'X' / 'O'
    uint32_t meta;    // node | depth << 16 | turn << 24 | legal mask << 25
    int32_t val;      // rollout value from the leaf's side to move
    uint32_t ow;      // d_order[legal mask]: the move-list order word (saves the rollout a lookup)
    uint32_t pad;
};

// LDS copy of a node created in the current flush.  During selection the node lives only
// here; its HBM record is written in one coalesced batch when the flush's leaves are chosen.
struct Fresh {
    uint32_t u;       // untried word (record +4)
    uint32_t ow;      // packed move-list columns (record +12)
    uint32_t link;    // parent | pact << 16 | depth << 24 (record +8)
    uint32_t lmask;   // legal-column mask of the node's position
    int32_t na;       // the edge INTO this node: Na (backup accumulates here, LDS atomics)
    int32_t w;        //                          Wa
    uint32_t pad1, pad2;
    uint16_t ch[8];   // children (record +16)
};
static_assert(sizeof(Fresh) == 48, "Fresh is three 16-byte LDS slots");

// ------------------------------------------------------------------ node records
struct Tree {
    uint8_t *nodes;  // this game's records
    __device__ __forceinline__ uint8_t *rec(int nd) const { return nodes + (size_t)nd * kRecBytes; }
    __device__ __forceinline__ uint32_t *hdr(int nd) const { return (uint32_t *)rec(nd); }
    __device__ __forceinline__ uint16_t *child(int nd) const { return (uint16_t *)(rec(nd) + 16); }
    __device__ __forceinline__ int32_t *na(int nd) const { return (int32_t *)(rec(nd) + 32); }
    // +64: stepwise search: Wa in fp64 (q); rollout search: Wa as int32 (w).  Either way Qa
    // is formed as Wa / Na when read — the IEEE quotient mcts.cpp:95 stores
    __device__ __forceinline__ double *q(int nd) const { return (double *)(rec(nd) + 64); }
    __device__ __forceinline__ int32_t *w(int nd) const { return (int32_t *)(rec(nd) + 64); }
};

// Node(state, legal_moves, parent, idx) (mcts.cpp:23-34): all moves untried, in list order.
// Lanes 0..7 write slot `lane`; lane 0 writes the header.
__device__ __forceinline__ void node_init(const Tree &t, int nd, int parent, int pact, int depth, uint32_t ow) {
    const uint32_t lane = lane_id();
    const uint32_t n = (ow >> 24) & 15u;
    if (lane == 0) {
        uint4 h;
        h.x = 0;                                                                 // N
        h.y = untried_init(n);                                                   // untried, #moves
        h.z = (uint32_t)(parent & 0xFFFF) | ((uint32_t)(pact & 0xFF) << 16) | ((uint32_t)depth << 24);
        h.w = ow;
        *(uint4 *)t.rec(nd) = h;
    }
    if (lane < kSlots) {
        t.child(nd)[lane] = 0xFFFF;
        t.na(nd)[lane] = 0;
        t.q(nd)[lane] = 0.0;  // Wa (either form) = 0
    }
}

__device__ __forceinline__ bool valid_state(uint64_t p0, uint64_t p1, int turn) {
    if ((p0 & p1) || ((p0 | p1) & ~kFull) || (turn & ~1)) return false;
    const uint64_t occ = p0 | p1;
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        const uint64_t col = (occ >> (7 * c)) & 0x3Full;
        if (col & (col + 1)) return false;  // stones must stack from the bottom
    }
    return true;
}

// ------------------------------------------------------------------ phase stamps (diagnostic)
template <bool ON>
struct Stamp {
    uint64_t ph[kPhases];
    uint64_t t;
    __device__ __forceinline__ Stamp() : t(ON ? __builtin_amdgcn_s_memtime() : 0) {
        for (int i = 0; i < kPhases; ++i) ph[i] = 0;
    }
    __device__ __forceinline__ void mark(int k) {
        if (ON) {
            const uint64_t now = __builtin_amdgcn_s_memtime();
            ph[k] += now - t;
            t = now;
        }
    }
};

using ConstDouble = const __attribute__((address_space(4))) double;

// ------------------------------------------------------------------ selection of one flush
// What a flush's selection leaves behind for its backup and publish steps.
struct FlushSel {
    int f0;          // first node created in this flush
    int x0node, d0;  // X0: where the first walk stopped, and its depth
    uint32_t ppath;  // lane l (l <= d0): level l of root..X0 = node | slot << 16
    bool x0_dirty;   // X0 expanded during the flush (its record must be rewritten)
    uint32_t x_u, x_ch;  // X0's untried word / child slot `lane & 7` as last seen
    // select_flush_plan only (planned = true): the fresh nodes are the draws 0..D-1; bit j of
    // Sm: draw j is a chain node's first draw; bit j of Z: draw j created the next chain node
    bool planned = false;
    int D = 0;
    uint64_t Sm = 0, Z = 0;
};

// The walk from the root over HBM records (select, mcts.cpp:47-63): the UCT child (first
// maximum, +inf for an unvisited edge) until a node with untried moves or without children.
// QW = false: the record's +64 slots hold Wa as int32 (rollout search: values are +-1/0);
// QW = true:  they hold Wa in fp64 (stepwise search).  Q = Wa / Na is formed here — the same
//             IEEE quotient mcts.cpp:95 stores, so the UCT inputs are bit-identical.
struct WalkEnd {
    int node, depth, turn;
    uint64_t b0, b1;     // the node's position
    uint32_t pathv;      // lane l (l <= depth): level l of the path = node | slot << 16
    uint32_t u, ow, ch;  // the node's record (ch: slot lane & 7)
};
template <bool QW>
__device__ __forceinline__ WalkEnd walk_hbm(const Tree &t, ConstDouble *logtab, uint64_t rp0, uint64_t rp1,
                                            int rturn, int done, double c, int &status) {
    const uint32_t lane = lane_id();
    const uint32_t k = lane & 7u;
    int node = 0, depth = 0, turn = rturn, nN = done;  // nN = N(node) = Na of its in-edge
    uint64_t b0 = rp0, b1 = rp1;
    uint32_t pathv = (lane == 0) ? 0x00FF0000u : 0u;
    uint32_t u, ow, ch;  // the current node's record (ch: slot k)
    for (;;) {  // the first walk: select (mcts.cpp:47-63) over HBM records
        const uint8_t *R = t.rec(node);
        const uint4 h = *(const uint4 *)R;
        ch = ((const uint16_t *)(R + 16))[k];
        const int32_t na = ((const int32_t *)(R + 32))[k];
        // Wa: fp64 (QW) or int32 (rollout search)
        const double qw = QW ? ((const double *)(R + 64))[k] : (double)((const int32_t *)(R + 64))[k];
        const double lg = logtab[nN];  // log(N), glibc values tabulated on the host
        u = uni(h.y);
        ow = uni(h.w);
        if (untried_count(u)) break;  // untried moves left: expand here
        if (depth >= kMaxDepth - 2) {  // unreachable (a C4 tree is <= 42 deep); never spin
            status = ZC_STATUS_INTERNAL;
            u = 0;
            break;
        }
        const uint32_t nm = u >> 28;
        const bool valid = k < nm && ch != 0xFFFF;
        int best;
        // slots k < nm (a scalar mask) with a child and no visit: masks ANDed, no per-lane bool
        const uint64_t unvisited = ((1ull << nm) - 1ull) & __ballot(ch != 0xFFFF) & __ballot(na == 0) & 0xFFull;
        if (unvisited) {  // +inf beats everything; first such slot
            best = __builtin_ctzll(unvisited);
        } else {
            // UCT (mcts.cpp:41-45) = fma(c, sqrt(log(N)/Na), Qa), first max in slot order
            const double q = valid ? qw / (double)na : 0.0;
            const double v = valid ? fma(c, sqrt(lg / (double)na), q) : -INFINITY;
            int bi;
            const double mx = max8_first(v, &bi);
            if ((__ballot(mx == -INFINITY) & 1ull) != 0) break;  // no child: terminal leaf
            best = bi;
        }
        const int nxt = __builtin_amdgcn_readlane((int)ch, best);
        nN = __builtin_amdgcn_readlane(na, best);
        const uint64_t bit = drop_bit(b0 | b1, (int)((ow >> (3 * best)) & 7u));
        if (turn) b1 |= bit; else b0 |= bit;
        turn ^= 1;
        node = nxt;
        ++depth;
        if (lane == (uint32_t)depth) pathv = (uint32_t)node | ((uint32_t)best << 16);
    }
    return WalkEnd{node, depth, turn, b0, b1, pathv, u, ow, ch};
}

// select + expand of the nb leaves of one flush (mcts.cpp:129-147), shared by the fused
// rollout search and the stepwise search.
//
// No backup happens inside a flush, so (1) the UCT path from the root to the node X0 where
// the flush's first walk stops is shared by every leaf of the flush (each walk resumes where
// the previous one expanded, always at or below X0), and (2) every node below X0 is created
// in this flush ("fresh": id >= f0, Na = W = 0 on every edge).  The reference's walk from a
// node without untried moves takes the first child with the largest UCT; an unvisited child
// scores +inf, so below X0 that is simply the lowest slot holding a fresh child — no
// arithmetic, no HBM.  Fresh nodes live in LDS (`fresh`) until the caller publishes them.
// Leaf j goes to leaves[j] (board, node, depth, turn, legal mask) and its path (node ids of
// levels 0..depth) to paths[j][*] (paths = nullptr: not recorded; the fresh part of a path is
// also the chain of parent links in `fresh`).  QW: as walk_hbm.
template <bool QW, bool STAMP, class RNG>
__device__ __forceinline__ void select_flush(const Tree &t, Fresh *fresh, Leaf *leaves, uint16_t *paths,
                                             const uint32_t *s_order, ConstDouble *logtab,
                                             RNG &rng, Counters &cn, Stamp<STAMP> &stamp, int &nnodes, int &status,
                                             uint64_t rp0, uint64_t rp1, int rturn, int done, int nb, double c,
                                             FlushSel &fs) {
    const uint32_t lane = lane_id();
    const uint32_t k = lane & 7u;  // child slot handled by this lane (lanes 8.. mirror 0..7)
    const int f0 = nnodes;
    for (int i = (int)lane; i < nb; i += 64) {  // fresh slots: no children, zero in-edge counters
        fresh[i].na = 0;
        fresh[i].w = 0;
        *(uint4 *)fresh[i].ch = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    }
    WalkEnd we = walk_hbm<QW>(t, logtab, rp0, rp1, rturn, done, c, status);
    int node = we.node, depth = we.depth, turn = we.turn;
    uint64_t b0 = we.b0, b1 = we.b1;
    uint32_t pathv = we.pathv, u = we.u, ow = we.ow, ch = we.ch;
    int cmask = legal_mask(b0 | b1);  // legal columns of the current node
    const int x0node = node;
    bool x0_dirty = false;
    uint32_t x_u = u, x_ch = ch;
    fs.f0 = f0;
    fs.x0node = x0node;
    fs.d0 = depth;
    fs.ppath = pathv;
    stamp.mark(1);

    // The rest of the flush, a node at a time.  Below X0 the walks take the lowest slot
    // holding a fresh child and a node is left only once it has no untried move, so the
    // flush visits a chain of nodes X0 = N0, N1, ... and at each one expands m = min(#untried,
    // leaves left) moves in a row: m random.choice draws over m, m-1, ... remaining moves
    // (count-sequence known in advance), then the next node is N's child in its lowest slot.
    // The draws are a scalar chain over ONE 64-word view (the accepted word of each draw is
    // the first word after the previous one with (w >> (32-k)) < n); the children and their
    // leaves are then built lane-parallel (lane i = the i-th draw), and the walk into the next
    // node reads the child from those lanes — no LDS round trip, no per-leaf scalar work.
    // ul: the node's untried list (move indices in list order, 3 bits each; random.choice's
    // r-th element, erased in place as mcts.cpp:67-72 does).
    constexpr uint32_t kIdentList = 0x1AC688u;  // 0, 1, ..., 6
    uint32_t ul = 0;
    {
        uint32_t c = 0;
        for (uint32_t bb = 0; bb < 7; ++bb)
            if ((u >> bb) & 1u) ul |= bb << (3 * c++);
    }
    int bulk0 = 0;          // first node id of the last bulk (the children of `node`)
    uint32_t invl = 0;      // lane k: 8 | i when slot k of `node` was expanded by draw i of that bulk
    uint32_t c_low = 0, c_lmask = 0;  // lane i: child i's order word / legal mask
    int j = 0;
    while (j < nb) {
        const uint32_t cnt = untried_count(u);
        if (cnt == 0) {
            const uint64_t fm = ((1ull << (u >> 28)) - 1ull) & __ballot(ch != 0xFFFF) & __ballot((int)ch >= f0) & 0xFFull;
            if (!fm) {  // no child at all: terminal, every remaining leaf of the flush is this node
                const uint32_t meta = (uint32_t)node | ((uint32_t)depth << 16) | ((uint32_t)turn << 24) |
                                      ((uint32_t)cmask << 25);
                for (int i = (int)lane; j + i < nb; i += 64) leaves[j + i] = Leaf{b0, b1, meta, 0, ow, 0};
                if (paths)
                    for (int jj = j; jj < nb; ++jj) paths[jj * kMaxDepth + lane] = (uint16_t)pathv;
                j = nb;
                wave_mem_order();
                break;
            }
            const int s = __builtin_ctzll(fm);
            const int i = __builtin_amdgcn_readlane((int)invl, s) & 7;
            const int child = bulk0 + i;
            if (node == x0node) {  // leaving X0 for good (walks never go back up)
                x_u = u;
                x_ch = ch;
            }
            const uint64_t bit = drop_bit(b0 | b1, (int)((ow >> (3 * s)) & 7u));
            if (turn) b1 |= bit; else b0 |= bit;
            turn ^= 1;
            ++depth;
            if (lane == (uint32_t)depth) pathv = (uint32_t)child | ((uint32_t)s << 16);
            node = child;
            ow = (uint32_t)__builtin_amdgcn_readlane((int)c_low, i);
            cmask = __builtin_amdgcn_readlane((int)c_lmask, i);
            u = untried_init((ow >> 24) & 15u);
            ul = kIdentList;
            ch = 0xFFFF;
            stamp.mark(2);
            continue;
        }
        // ---- m draws (random.choice over cnt, cnt-1, ... untried moves)
        const int m = min((int)cnt, nb - j);
        uint32_t rr = 0;  // lane i < m: draw i's value r (the index into the untried list then)
        {
            int done = 0;
            for (;;) {  // one 64-word view per pass
                rng_need(rng);
                const uint32_t w = rng_view(rng);  // lane l: the next unconsumed word + l
                const int rem = m - done;
                // acceptance masks of the next (up to 7) draws, n = cnt - done - i: independent
                // of each other, issued back to back
                uint64_t A[7];
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                    const uint32_t n = (uint32_t)max((int)cnt - done - i, 1);
                    A[i] = __ballot((w >> draw_shift<RNG>(n)) < n);
                }
                // the draws, a branch-free scalar chain: each takes the lowest accepted word
                // after the last one (lb = acc & -acc); a draw without one zeroes `gt`, and with
                // it every later draw of the view
                uint64_t gt = ~0ull, F = 0;  // lanes after the last accepted word; accepted words
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                    const uint64_t acc = (i < rem ? A[i] : 0ull) & gt;
                    const uint64_t lb = acc & (0ull - acc);
                    F |= lb;
                    gt = 0ull - (lb << 1);
                }
                const int nd = __popcll(F);
                const int f = 63 - __clzll(F | 1ull);  // the last accepted word (F != 0 when nd > 0)
                // lane-parallel: accepted word l is draw di = done + (accepted words below it);
                // its value goes to lane di (a forward permute; lanes outside [done, done + nd)
                // keep theirs)
                const uint32_t di = (uint32_t)done + mbcnt64(F);
                const uint32_t rl = w >> draw_shift<RNG>((uint32_t)max((int)cnt - (int)di, 1));
                const uint32_t got = (uint32_t)__builtin_amdgcn_ds_permute((int)(mask_sel(F, 63u, di) << 2), (int)rl);
                rr = mask_sel(((1ull << nd) - 1ull) << done, rr, got);  // lanes done .. done + nd - 1
                done += nd;
                if (done < m) {  // the view ran out: all of it is consumed
                    rng_eat(rng, (uint32_t)kWin);
                    continue;
                }
                rng_eat(rng, (uint32_t)f + 1u);
                break;
            }
        }
        // draw i's position in the untried list as it was before the bulk (the erase of
        // mcts.cpp:72 undone all at once, a Lehmer code: later draws skip the earlier picks)
        // (step i compares with draw i's own r: lane i is only adjusted by the later steps i' < i)
        uint32_t pl = rr;
        uint32_t rpick[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) rpick[i] = (uint32_t)__builtin_amdgcn_readlane((int)rr, i);
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            const uint64_t later = ((1ull << m) - 1ull) & ~((2ull << i) - 1ull);  // lanes i+1 .. m-1
            pl = add_in_mask(pl, __ballot(pl >= rpick[i]) & later);
        }
        const uint32_t mi_l = (ul >> (3 * (pl & 7u))) & 7u;  // lane i < m: draw i's move index
        // the expanded slots (OR over lanes 0..7, DPP) and, in lane k, the draw that took slot k
        uint32_t slotbit = (int)lane < m ? 1u << mi_l : 0u;
        slotbit |= (uint32_t)dpp<0xB1>((int)slotbit);
        slotbit |= (uint32_t)dpp<0x4E>((int)slotbit);
        slotbit |= (uint32_t)dpp<0x141>((int)slotbit);
        const uint32_t ucl = uni(slotbit);
        const uint32_t sent = (uint32_t)__builtin_amdgcn_ds_permute((int)(((int)lane < m ? mi_l : 63u) << 2),
                                                                     (int)(8u | lane));
        invl = (ucl >> (lane & 7u)) & 1u ? sent : 0u;
        u &= ~ucl;
        // ---- the m children and their leaves, lane i = draw i
        {
            const uint32_t mi = mi_l;
            const int col = (int)((ow >> (3 * mi)) & 7u);
            const uint64_t bit = drop_bit(b0 | b1, col);
            const bool filled = (bit & kTop) != 0;
            c_lmask = (uint32_t)cmask & ~(filled ? (1u << col) : 0u);
            c_low = ow;
            if ((int)lane < m && filled) c_low = s_order[c_lmask];
            const int ldepth = depth + 1;
            const uint32_t leaf = (uint32_t)nnodes + lane;
            if ((int)lane < m) {
                *(uint4 *)&fresh[leaf - (uint32_t)f0] =
                    make_uint4(untried_init((c_low >> 24) & 15u), c_low,
                               (uint32_t)node | (mi << 16) | ((uint32_t)ldepth << 24), c_lmask);
                const uint64_t l0 = turn ? b0 : (b0 | bit), l1 = turn ? (b1 | bit) : b1;
                leaves[j + (int)lane] = Leaf{l0, l1,
                                             leaf | ((uint32_t)ldepth << 16) | ((uint32_t)(turn ^ 1) << 24) | (c_lmask << 25),
                                             0, c_low, 0};
            }
            // leaf j+i's path: the walk's path plus the new node (all 64 lanes store: lanes
            // >= kMaxDepth spill into the next leaf's path, written after this, or the spill bytes)
            if (paths)
                for (int i = 0; i < m; ++i)
                    paths[(j + i) * kMaxDepth + lane] = (uint16_t)(lane == (uint32_t)ldepth ? (uint32_t)(nnodes + i) : pathv);
            // the node's new children
            const uint32_t pk = lane < 8 ? invl : 0u;
            if (pk & 8u) ch = (uint32_t)nnodes + (pk & 7u);
            if (node >= f0) {  // the node's copy in LDS
                if (lane == 0) fresh[node - f0].u = u;
                if (lane < 8 && (pk & 8u)) fresh[node - f0].ch[k] = (uint16_t)ch;
            } else {
                x0_dirty = true;  // X0 itself: written back when the flush is published
            }
            wave_mem_order();
        }
        bulk0 = nnodes;
        nnodes += m;
        j += m;
        stamp.mark(3);
    }
    if (node == x0node) {
        x_u = u;
        x_ch = ch;
    }
    // the flush's expansions = its fresh nodes; their depths summed lane-parallel (bit-sliced
    // ballots) instead of per expansion on the chain
    {
        const int nf = nnodes - f0;
        int dsum = 0;
        for (int base = 0; base < nf; base += 64) {
            const int i = base + (int)lane;
            const uint32_t d = i < nf ? fresh[i].link >> 24 : 0u;
#pragma unroll
            for (int bit = 0; bit < 6; ++bit) dsum += __popcll(__ballot((d >> bit) & 1u)) << bit;
        }
        cn.add(cn.expansions, nf);
        cn.add(cn.depth_sum, dsum);
    }
    fs.x0_dirty = x0_dirty;
    fs.x_u = x_u;
    fs.x_ch = x_ch;
}

}  // namespace
}  // namespace zc
