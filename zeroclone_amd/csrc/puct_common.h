// puct_common.h — the core of the PUCT searches (no reference counterpart),
// shared by chess_puct.hip and c4_puct.hip and included by exactly those translation units.
// Every rule the two games have in common is stated here, once, beside its code: the flush
// schedule, the search's control words, the priors and their failure, the root noise, the
// temperature sample and the re-root's game-independent passes.  The games keep what differs:
// the node layout, the walk, the move generation and the planes.
//
// A game is "Q chunks of 64 moves per lane": move k of a node sits in lane k & 63 as register
// q = k >> 6 of a [Q] array.  Connect4 (7 moves) is Q = 1, chess (256 moves) is Q = 4.  Sums
// over a node's moves add a lane's registers q = 0 .. Q - 1 in order and then run the xor
// butterfly 32 .. 1 (wave_sum_f): the order of tests/puct_noise_ref.py's wave_sum.  Q = 1 is
// that order too, because adding +0.0f is exact.
#pragma once
#include <hip/hip_runtime.h>

#include "c4_device.h"
#include "counter_rng.h"

namespace zc {
namespace {

__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

__device__ __forceinline__ double wave_sum_d(double x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ float wave_max_f(float x) {
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ float wave_sum_f(float x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// Every vector-memory operation of the wave so far has completed: what one lane stored, any
// lane now loads, and a load issued before this point cannot see a store issued after it.
__device__ __forceinline__ void vm_drain() {
    wave_mem_order();
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Leaves of flush f of a search of `sims` simulations in batches of bs: flush 0 is the root
// alone, the other sims - 1 follow in batches.
__device__ __forceinline__ int flush_leaves(int sims, int bs, int f) {
    if (f == 0) return 1;
    return max(0, min(bs, sims - 1 - (f - 1) * bs));
}

// The game's search number: the counter word of its noise and temperature sample.
template <class Params>
__device__ __forceinline__ uint32_t search_number(const Params &p, int gl) {
    return p.search_no ? (uint32_t)__builtin_amdgcn_readfirstlane(p.search_no[gl]) : 0u;
}
template <class Params>
__device__ __forceinline__ uint2 rng_key(const Params &p) {
    return make_uint2((uint32_t)p.seed, (uint32_t)(p.seed >> 32));
}

// ---- control words ----
// A game's search keeps seven words in the game's ctl block.  Which word is which is the
// game's business (the chess words are shared with the other chess searches): a game names
// them in a struct W of static constexpr ints
//   nodes   nodes in the tree            status  ZC_STATUS_* of the search
//   nb      leaves of the pending flush  exp, depth  expansions and the sum of their depths
//   done    the game's last search ran to end with status 0: its tree may be re-rooted
//   reused  the search in progress started from a kept subtree: flush 0 has no leaf
// and the rules below go through them.

// begin / re-root: a search of `kept` kept nodes (0: a fresh root) starts with this status.
template <class W, class Params>
__device__ __forceinline__ void search_reset(const Params &p, int32_t *ctl, int gl, int kept, int status) {
    if (lane_id() != 0) return;
    ctl[W::nodes] = kept ? kept : 1;
    ctl[W::status] = status;
    ctl[W::nb] = 0;
    ctl[W::exp] = 0;
    ctl[W::depth] = 0;
    ctl[W::done] = 0;
    ctl[W::reused] = kept ? 1 : 0;
    if (p.out_kept) p.out_kept[gl] = kept;
}

// forget: the games' trees are not re-rooted by their next begin_reuse.
__global__ void puct_forget_kernel(int32_t *ctl, int first_game, int n_games, int done_word) {
    const int gl = blockIdx.x * blockDim.x + threadIdx.x;
    if (gl < n_games) ctl[(size_t)(first_game + gl) * kCtlWords + done_word] = 0;
}
inline void launch_puct_forget(int32_t *ctl, int first_game, int n_games, int done_word, hipStream_t s) {
    hipLaunchKernelGGL(puct_forget_kernel, dim3((n_games + 63) / 64), dim3(64), 0, s, ctl, first_game, n_games,
                       done_word);
}

// forget, for the games alone whose recorder slot (zc_traj_buffers.d_slot, row gl) holds a game at
// its first position: a refilled slot's tree belongs to the game that ended.
__global__ void puct_forget_fresh_kernel(int32_t *ctl, int first_game, int n_games, int done_word,
                                         const int32_t *slot) {
    const int gl = blockIdx.x * blockDim.x + threadIdx.x;
    if (gl < n_games && slot[4 * (size_t)gl] == 1 && slot[4 * (size_t)gl + 1] >= 0)
        ctl[(size_t)(first_game + gl) * kCtlWords + done_word] = 0;
}
inline void launch_puct_forget_fresh(int32_t *ctl, int first_game, int n_games, int done_word, const int32_t *slot,
                                     hipStream_t s) {
    hipLaunchKernelGGL(puct_forget_fresh_kernel, dim3((n_games + 63) / 64), dim3(64), 0, s, ctl, first_game, n_games,
                       done_word, slot);
}

// select: the walks flush p.flush makes; none in a failed search, none in flush 0 of a search
// on a kept subtree (a kept root is evaluated already).
template <class W, class Params>
__device__ __forceinline__ int select_leaves(const Params &p, const int32_t *ctl, int status) {
    int nb = status ? 0 : flush_leaves(p.sims, p.bs, p.flush);
    if (p.flush == 0 && uni(ctl[W::reused])) nb = 0;
    return nb;
}

// select, after the walks of nb leaves: returns the pending leaves, none where a walk failed.
template <class W, class Params>
__device__ __forceinline__ int select_done(const Params &p, int32_t *ctl, int gl, int nnodes, int status, int nb,
                                           Counters cn) {
    if (status) nb = 0;
    wave_mem_order();
    if (lane_id() == 0) {
        ctl[W::nodes] = nnodes;
        ctl[W::status] = status;
        ctl[W::nb] = nb;
        ctl[W::exp] += cn.expansions;
        ctl[W::depth] += cn.depth_sum;
        if (p.counts) p.counts[gl] = nb;
    }
    return nb;
}

// end (lane 0): the search number moves on, the stats, and whether the tree may be kept.  A
// search on a kept subtree has no flush-0 leaf and adds sims - 1 visits.
template <class W, class Params>
__device__ __forceinline__ void search_done(const Params &p, int32_t *ctl, int gl, int status) {
    if (p.search_no) p.search_no[gl] = (int32_t)(search_number(p, gl) + 1);
    zc_game_stats st{};
    st.status = status;
    st.expansions = ctl[W::exp];
    st.depth_sum = ctl[W::depth];
    // a root flagged at begin (the only source of these two codes) evaluated no leaf; a search
    // stopped part-way (INTERNAL, CAPACITY) reports the simulations it was asked for
    const bool never_ran = status == ZC_STATUS_NO_MOVES || status == ZC_STATUS_BAD_STATE;
    st.leaves = never_ran ? 0 : ctl[W::reused] ? p.sims - 1 : p.sims;
    p.out_stats[gl] = st;
    ctl[W::done] = status == 0 ? 1 : 0;
}

// ---- priors ----
// A lane's registers of a node's moves: v[q] belongs to move q * 64 + lane.  The functions
// below take and return them by value.  A reference to a caller's array reaches the inlined
// code as a flat pointer to private memory, which becomes registers only late in the
// compiler: that form cost the chess backup kernel 8 VGPRs and a step of occupancy.
template <int Q>
struct MoveRegs {
    float v[Q];
};
template <int Q>
struct Priors {
    MoveRegs<Q> pr;
    bool ok;
};

// The softmax of the logits lg of a node's nm moves (-inf in the registers past them).  Not
// ok, and no priors: a NaN or +inf logit on a legal move, or -inf on all of them.
template <int Q>
__device__ __forceinline__ Priors<Q> softmax_priors(MoveRegs<Q> lg, int nm) {
    const uint32_t lane = lane_id();
    float mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < Q; ++q) mx = fmaxf(mx, lg.v[q]);
    mx = wave_max_f(mx);
    Priors<Q> r;
    float sum = 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        r.pr.v[q] = q * 64 + (int)lane < nm ? expf(lg.v[q] - mx) : 0.0f;
        sum += r.pr.v[q];
    }
    sum = wave_sum_f(sum);
    r.ok = __ballot(!(sum > 0.0f && sum < INFINITY)) == 0ull;
#pragma unroll
    for (int q = 0; q < Q; ++q) r.pr.v[q] = r.pr.v[q] / sum;
    return r;
}

// Gamma(alpha, 1) by Marsaglia-Tsang (alpha < 1 via Gamma(alpha + 1) * U^(1/alpha)); the
// draws of (game, move j) in the game's search number sno come from Philox counters
// (j, attempt | sno << 6, game, tag).
__device__ float gamma_draw(float alpha, uint2 key, uint32_t game, uint32_t j, uint32_t sno) {
    const bool boost = alpha < 1.0f;
    const float a = boost ? alpha + 1.0f : alpha;
    const float d = a - 1.0f / 3.0f, cc = 1.0f / sqrtf(9.0f * d);
    float g = 0.0f;
    for (uint32_t att = 0; att < 64; ++att) {
        const uint4 r = philox(make_uint4(j, att | (sno << 6), game, 0x6A09E667u), key);
        // Box-Muller normal from two uniforms
        const float z = sqrtf(-2.0f * logf(u01(r.x))) * cospif(2.0f * u01(r.y));
        const float v1 = 1.0f + cc * z;
        if (v1 <= 0.0f) continue;
        const float v = v1 * v1 * v1, u = u01(r.z);
        if (logf(u) < 0.5f * z * z + d - d * v + d * logf(v)) {
            g = d * v;
            if (boost) g *= powf(u01(r.w), 1.0f / alpha);
            break;
        }
    }
    return g;
}

// Root noise on game g's root priors: pr = (1 - eps) * pr + eps * x, x ~ Dirichlet(alpha) over
// the root's nm moves as normalised gamma draws.  The same for a fresh root (backup of flush
// 0) and for a kept one (re-root), which mixes it into the priors the tree holds.
template <int Q, class Params>
__device__ __forceinline__ MoveRegs<Q> mix_root_noise(const Params &p, int g, int gl, int nm, MoveRegs<Q> pr) {
    const uint32_t lane = lane_id();
    const uint2 key = rng_key(p);
    const uint32_t sno = search_number(p, gl);
    float gm[Q], gs = 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const uint32_t k = q * 64 + lane;
        gm[q] = (int)k < nm ? gamma_draw(p.dir_alpha, key, (uint32_t)g, k, sno) : 0.0f;
        gs += gm[q];
    }
    gs = wave_sum_f(gs);
#pragma unroll
    for (int q = 0; q < Q; ++q) pr.v[q] = (1.0f - p.dir_eps) * pr.v[q] + p.dir_eps * (gs > 0.0f ? gm[q] / gs : 0.0f);
    return pr;
}

// ---- temperature sample ----
// Temperature weight of a root move with n visits: (n * 2^-k)^(1/T), k = the bit length of
// the root's largest count.  The common factor 2^(-k/T) leaves the sampled distribution as
// n^(1/T); the scaled base is below 1, so no temperature overflows (unscaled, 1210^100 does,
// and a total of inf selects no move), and a power of two keeps integer 1/T exact.
__device__ __forceinline__ int count_bits(int32_t max_count) { return max_count > 0 ? 32 - __clz(max_count) : 0; }
__device__ __forceinline__ double temperature_weight(int32_t n, int k, double inv_t) {
    return pow(ldexp((double)n, -k), inv_t);
}

// The root move is sampled proportional to Na^(1/T) by the inverse CDF: the first move in move
// order whose running sum of weights exceeds this target, u * tot with u from the game's Philox
// word of this search (the last move if none does).  tot is the caller's sum of the weights, in
// the caller's own order of summation.  The serial scan stays in the two end kernels: as a
// shared inlined function, in any form, it cost c4_puct_end_kernel a 73rd VGPR and with it a
// step of occupancy.
template <class Params>
__device__ __forceinline__ double temperature_target(const Params &p, int g, int gl, double tot) {
    const uint4 r = philox(make_uint4((uint32_t)g, 0x5BE0CD19u, search_number(p, gl), 0), rng_key(p));
    return (double)u01(r.x) * tot;
}

// ---- tree reuse: the passes of a re-root that do not depend on the game ----
// Node ids are in creation order (a parent's id is below its child's), so one ascending pass
// over the ids, 64 a chunk, decides which nodes descend from the new root r and numbers them,
// and a second one moves the records down in place.

// One chunk of the numbering pass: lane's node i = base + lane (valid: i < n) with parent par.
// Returns the ballot of the chunk's nodes in r's subtree.  A parent in an earlier chunk has its
// final entry in remap (0xFFFF: not kept); parents in this chunk take at most one round per
// level of the tree.
__device__ __forceinline__ uint64_t reroot_mark(int i, bool valid, int par, int r, int base, const uint16_t *remap) {
    bool k = valid && (i == r || (par >= r && par < base && remap[par] != 0xFFFF));
    const bool inpar = valid && par >= base && par < i;
    const int pl = inpar ? par - base : 0;  // the parent's lane
    uint64_t b = __ballot(k);
    for (;;) {
        k = k || (inpar && ((b >> pl) & 1ull));
        const uint64_t nb = __ballot(k);
        if (nb == b) return b;
        b = nb;
    }
}

// The kept records of T[r, n) move to their new ids (remap, new id <= old id), 64 ids a chunk
// as sizeof(Node) / 16 x 64 16-byte pieces.  Every load of a chunk has returned before any of
// its stores is issued, so the stores land only on records that this or an earlier chunk has
// already loaded.
template <class Node>
__device__ void reroot_move_records(Node *T, const uint16_t *remap, int n, int r) {
    static_assert(sizeof(Node) % 16 == 0, "a node record is moved as 16-byte pieces");
    constexpr int kPieces = (int)sizeof(Node) / 16;
    const uint32_t lane = lane_id();
    for (int base = r; base < n; base += 64) {
        const int rows = min(64, n - base);
        const uint4 *src = reinterpret_cast<const uint4 *>(T + base);
        uint4 v[kPieces];
        uint32_t dst[kPieces];
#pragma unroll
        for (int it = 0; it < kPieces; ++it) {
            const int q = it * 64 + (int)lane, rec = q / kPieces;
            const bool valid = rec < rows;
            v[it] = valid ? src[q] : make_uint4(0, 0, 0, 0);
            dst[it] = valid ? (uint32_t)remap[base + rec] : 0xFFFFu;
        }
        vm_drain();
#pragma unroll
        for (int it = 0; it < kPieces; ++it)
            if (dst[it] != 0xFFFFu) reinterpret_cast<uint4 *>(T + dst[it])[(it * 64 + (int)lane) % kPieces] = v[it];
        wave_mem_order();
    }
    vm_drain();
}

}  // namespace
}  // namespace zc
