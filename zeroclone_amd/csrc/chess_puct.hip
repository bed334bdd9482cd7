// chess_puct.hip — AlphaZero-style PUCT search for chess on gfx950 (SURVEY.md §8 a21, config
// C5: a policy + value network, Dirichlet root noise).  The reference has no counterpart
// (its search is plain UCT with one-at-a-time expansion, mcts.cpp:41-78); this extension
// reuses its tree, rules and flush protocol and changes the selection rule:
//
//   select  a = first argmax  Q(a) + c_puct * P(a) * sqrt(sum_b N(b)) / (1 + N(a)),
//           Q(a) = W(a) / N(a) (0 when N(a) = 0), P from the policy head of the node's own
//           evaluation; the walk stops at an edge without a child (the child is created and
//           is the leaf), at a terminal node, or at a node still waiting for its evaluation;
//   virtual loss: every edge of a pending leaf's path counts as one visit lost by the
//           parent's mover (N += 1, W -= 1) until the flush is backed up, so the leaves of a
//           flush spread over the tree instead of repeating one path;
//   backup  per leaf in pending order: the node's priors from the policy logits of its legal
//           moves (first evaluation only), then each edge undoes its virtual loss and takes
//           the value (W += 1 - r, N already counted), r alternating in sign; a terminal
//           leaf's value is -1 (side to move mated) or 0 (no moves otherwise);
//   reuse   (opt-in, zc_chess_puct_begin_reuse) the subtree of the position now at the root, one
//           or two plies below the last search's root, is compacted in place into the next
//           tree, node records and child slots.
//
// What the search shares with the Connect4 one is in puct_common.h, each rule beside its code:
// the flush schedule (flush 0 evaluates the root alone), the control words, the softmax of the
// priors, the root noise, the temperature sample and the re-root's numbering and record move.
// This file holds the game: the walk over a node's 4 x 64 slots, the deferred expansion, the
// slots' part of the re-root and the planes.
//
// Launches (one wave per game): begin or re-root (root node), select (flush f's leaves, planes),
// backup (priors + values), end (move by visits or temperature sampling, visit counts).
#include <hip/hip_fp16.h>

#include "chess_tree.h"
#include "puct_common.h"

namespace zc {
namespace {

// meta[j] bit 31: leaf j's walk created its node (its moves are generated after the walks)
constexpr uint32_t kMetaCreated = 0x80000000u;

// the search's control words (puct_common.h) among the chess searches' (chess_tree.h)
struct PCtl {
    static constexpr int nodes = cNodes, status = cStatus, nb = cNb, exp = cExp, depth = cDepth, done = cDone,
                         reused = cReused;
};

// One PUCT walk + expansion; returns the leaf, its depth, and the edge slots of its path
// in lanes 1..depth of pathv.  Applies the virtual loss on every edge it takes.
//
// The expansion is DEFERRED: the new node gets its id, position, parent, depth and
// `evaluated = 0` here — everything a later walk of the same flush looks at (it stops at a node
// not yet evaluated) — and *created is set; its legal moves are generated after the flush's
// walks, every created node of every game in parallel (puct_expand_kernel, one wave each), and
// committed in creation order (puct_commit_kernel: slot ranges by a prefix sum over the
// creation order, i.e. exactly the ranges the serial create_node would have taken).  Nothing
// reads a node's moves before its first backup, so the tree is the serial one.
__device__ int puct_walk(const ChessParams &p, const CTree &t, CLds &L, int &nnodes, int &slots, int &status,
                         int &ldepth, uint32_t &pathv, Counters &cn, bool &created) {
    const uint32_t lane = lane_id();
    int node = 0, depth = 0;
    pathv = 0;
    for (;;) {
        ChessNode *N = &t.nodes[node];
        const int nm = uni((int)N->nmoves);
        if (nm == 0 || !uni((int)N->evaluated)) break;  // terminal, or a leaf still pending
        if (depth >= kChessPath - 2) {
            status = ZC_STATUS_CAPACITY;
            break;
        }
        const uint32_t base = uni(N->base);
        // ONE round of loads per level: every child slot's N, W, P and child id (up to four
        // 64-slot chunks, registers), issued together; the sum of N, the scores and the child
        // pointer then come from registers (round 4 read N twice and the child once more:
        // three dependent global round trips per level).  Same arithmetic in the same order.
        int32_t na_r[4];
        double w_r[4];
        float pr_r[4];
        uint32_t ch_r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = q * 64 + (int)lane;
            na_r[q] = 0;
            w_r[q] = 0.0;
            pr_r[q] = 0.0f;
            ch_r[q] = 0xFFFFu;
            if (q * 64 < nm && j < nm) {
                na_r[q] = t.na[base + j];
                w_r[q] = t.w[base + j];
                pr_r[q] = t.pr[base + j];
                ch_r[q] = t.ch[base + j];
            }
        }
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = q * 64 + (int)lane;
            if (q * 64 < nm) tot += j < nm ? (double)na_r[q] : 0.0;
        }
        const double sq = sqrt(wave_sum_d(tot));
        double bv = -INFINITY;
        int bi = 0x7FFFFFFF;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = q * 64 + (int)lane;
            if (q * 64 < nm && j < nm) {
                const int32_t na = na_r[q];
                const double qv = na > 0 ? w_r[q] / (double)na : 0.0;
                const double u = p.c * (double)pr_r[q] * sq / (double)(1 + na);
                const double v = qv + u;
                if (v > bv) {
                    bv = v;
                    bi = j;
                }
            }
        }
        argmax64(bv, bi);
        const int best = uni(bi);
        if ((uint32_t)best >= (uint32_t)nm) {  // no score compared above -inf (all NaN): no edge to take
            status = ZC_STATUS_INTERNAL;
            break;
        }
        const uint32_t s = base + (uint32_t)best;
        const int bq = best >> 6;
        const uint32_t chv = bq == 0 ? ch_r[0] : bq == 1 ? ch_r[1] : bq == 2 ? ch_r[2] : ch_r[3];
        const int child = (int)(uint32_t)__builtin_amdgcn_readlane((int)chv, best & 63);
        if (lane == 0) {  // virtual loss: one visit lost by this node's mover
            t.na[s] += 1;
            t.w[s] -= 1.0;
        }
        ++depth;
        if (lane == (uint32_t)depth) pathv = s;
        if (child != 0xFFFF) {
            node = child;
            continue;
        }
        // expand the edge: the child position, its legal moves, no priors yet
        const uint32_t m = uni((uint32_t)t.mv[s]);
        if (lane < 18) ((uint32_t *)&L.st)[lane] = ((const uint32_t *)&N->st)[lane];
        wave_sync_mem();
        chessdev::apply_move_wave(L.st, m);
        wave_sync_mem();
        const int id = nnodes++;
        if (id >= p.M) {
            status = ZC_STATUS_CAPACITY;
            break;
        }
        ChessNode *C = &t.nodes[id];  // the record without its moves (puct_commit_kernel adds them)
        if (lane < 18) ((uint32_t *)&C->st)[lane] = ((const uint32_t *)&L.st)[lane];
        if (lane == 0) {
            C->base = 0;
            C->nmoves = 0;
            C->nu = 0;
            C->parent = (uint16_t)node;
            C->pact = (uint16_t)best;
            C->depth = (uint16_t)depth;
            C->evaluated = 0;
            t.ch[s] = (uint16_t)id;
        }
        created = true;
        cn.add(cn.expansions, 1);
        cn.add(cn.depth_sum, depth);
        wave_sync_mem();
        node = id;
        break;
    }
    ldepth = depth;
    return node;
}

__global__ __launch_bounds__(64) void puct_begin_kernel(ChessParams p) {
    __shared__ CLds L;
    const int gl = blockIdx.x;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    const CTree t = ctree(p, g);
    int32_t *ctl = p.ca.ctl + (size_t)g * kCtlWords;
    const uint32_t lane = lane_id();
    if (lane < 18) {
        const uint32_t w = ((const uint32_t *)&p.roots[gl])[lane];
        ((uint32_t *)&L.st)[lane] = w;
        ((uint32_t *)&p.ca.roots[g])[lane] = w;
    }
    wave_sync_mem();
    int slots = 0, status = 0;
    create_node(t, L, 0, 0xFFFF, 0xFFFF, 0, slots, status);
    if (!status && uni((int)t.nodes[0].nmoves) == 0) status = ZC_STATUS_NO_MOVES;
    if (lane == 0) ctl[cSlots] = slots;
    search_reset<PCtl>(p, ctl, gl, 0, status);
}

// ---- tree reuse: the subtree of the position now at the root becomes the next tree ----
// The re-root of puct_common.h on the chess tree's two address spaces.  The slot ranges are in
// creation order as the node ids are (puct_commit_kernel hands them out in creation order), so
// a kept node's new first slot is <= its old one: the numbering pass also sums the kept nodes'
// move counts into the new bases, and after the node records the slots move down in place, 64
// at a time with every load of a step returned before any of its stores is issued; a last pass
// renumbers the parents.  Every index read from the arena is bounded before it is used: a tree
// that fails a bound is not kept.

// Whether node id (0 < id < n) holds the position in tgt[0..16]: board, turn, fifty, castle
// (word 16's low three bytes; the reserved bytes are not compared).
__device__ __forceinline__ bool reroot_holds(const CTree &t, const uint32_t *tgt, int id, int n) {
    if (id <= 0 || id >= n) return false;
    const uint32_t *w = (const uint32_t *)&t.nodes[id].st;
    bool same = ((w[16] ^ tgt[16]) & 0x00FFFFFFu) == 0u;
#pragma unroll
    for (int q = 0; q < 16; ++q) same = same && w[q] == tgt[q];
    return same;
}

// The first node in slot order among node `par`'s children that holds the position, or -1;
// kids[q] takes the child in slot q * 64 + lane (0xFFFF: none).  false: a bound failed.
__device__ bool reroot_scan(const CTree &t, const uint32_t *tgt, int par, int n, int s, uint32_t (&kids)[4], int &hit) {
    const uint32_t lane = lane_id();
    const int nm = uni((int)t.nodes[par].nmoves);
    const uint32_t base = uni(t.nodes[par].base);
    hit = -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) kids[q] = 0xFFFFu;
    if (nm > ZC_CHESS_MAX_MOVES || (int64_t)base + nm > (int64_t)s) return false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = q * 64 + (int)lane;
        if (q * 64 < nm && j < nm) kids[q] = t.ch[base + j];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q * 64 >= nm || hit >= 0) continue;
        const uint64_t m = __ballot(reroot_holds(t, tgt, (int)kids[q], n));
        if (m) hit = __builtin_amdgcn_readlane((int)kids[q], __builtin_ctzll(m));
    }
    return true;
}

// The node holding the position one ply below the root, else two plies below it (the root's
// children in slot order, each one's children in slot order); -1: none, or a bound failed.
__device__ int reroot_find(const CTree &t, const uint32_t *tgt, int n, int s) {
    uint32_t c1[4], c2[4];
    int hit;
    if (!reroot_scan(t, tgt, 0, n, s, c1, hit)) return -1;
    if (hit >= 0) return hit;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint64_t m = __ballot(c1[q] != 0xFFFFu);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            const int c = __builtin_amdgcn_readlane((int)c1[q], l);
            if (c <= 0 || c >= n) return -1;
            if (!reroot_scan(t, tgt, c, n, s, c2, hit)) return -1;
            if (hit >= 0) return hit;
        }
    }
    return -1;
}

// Pass 1: remap[i] = the new id of node i of r's subtree, 0xFFFF for any other node i >= r;
// rbase[new id] = the node's new first slot, the running sum of the kept nodes' move counts.
// Returns the nodes kept and, in `kslots`, their slots; 0 when a kept node's slot range fails a
// bound.
__device__ int reroot_number(const CTree &t, uint16_t *remap, uint32_t *rbase, int n, int s, int r, int &kslots) {
    const uint32_t lane = lane_id();
    int cnt = 0, tot = 0;
    bool bad = false;
    for (int b0 = r; b0 < n; b0 += 64) {
        const int i = b0 + (int)lane;
        const bool valid = i < n;
        const int par = valid ? (int)t.nodes[i].parent : 0xFFFF;
        const int nm = valid ? (int)t.nodes[i].nmoves : 0;
        const uint32_t ob = valid ? t.nodes[i].base : 0u;
        const uint64_t b = reroot_mark(i, valid, par, r, b0, remap);
        const bool k = (b >> lane) & 1ull;
        const int id = cnt + __popcll(b & ((1ull << lane) - 1ull));
        // exclusive prefix sum of the kept nodes' move counts over the chunk, plus the carry
        const int mine = k ? nm : 0;
        int inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o);
            if ((int)lane >= o) inc += up;
        }
        const int nbase = tot + inc - mine;
        // the slots move down, never up, and come from inside the slots in use
        if (k && (nm > ZC_CHESS_MAX_MOVES || (int64_t)ob + nm > (int64_t)s || (uint32_t)nbase > ob)) bad = true;
        if (valid) remap[i] = k ? (uint16_t)id : (uint16_t)0xFFFF;
        if (k) rbase[id] = (uint32_t)nbase;
        cnt += __popcll(b);
        tot += __builtin_amdgcn_readlane(inc, 63);
        vm_drain();  // the next chunk's lanes read these entries
    }
    kslots = tot;
    return __ballot(bad) ? 0 : cnt;
}

// Pass 2 is reroot_move_records.  Pass 3: the kept slots move to [0, kslots) by flat slot index, 64 slots a step: a window of
// 64 kept nodes (new ids; a moved record still holds its old base) gives, per slot, its node by
// a search over the window's new bases in registers, and so its old slot.  New slot d comes from
// an old slot >= d, so a step's stores land only on slots that this or an earlier step has
// loaded.  The child ids go through the table on the way.
__device__ void reroot_move_slots(const CTree &t, const uint16_t *remap, const uint32_t *rbase, int kept, int n, int r) {
    const uint32_t lane = lane_id();
    for (int k0 = 0; k0 < kept; k0 += 64) {
        const int k = k0 + (int)lane;
        const bool kv = k < kept;
        const uint32_t nb = kv ? rbase[k] : 0xFFFFFFFFu;  // non-decreasing over the window's lanes
        const uint32_t ob = kv ? t.nodes[k].base : 0u;
        const uint32_t nm = kv ? (uint32_t)t.nodes[k].nmoves : 0u;
        const uint32_t lo = uni(nb);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(nb + nm), min(63, kept - 1 - k0));
        for (uint32_t d0 = lo; d0 < hi; d0 += 64) {
            const uint32_t d = d0 + lane;
            int j = 0;  // the last lane of the window whose new base is <= d: the slot's node
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                const uint32_t x = (uint32_t)__shfl((int)nb, j + step);
                if (x <= d) j += step;
            }
            const uint32_t src = (uint32_t)__shfl((int)ob, j) + (d - (uint32_t)__shfl((int)nb, j));
            const bool dv = d < hi && src >= d && (int64_t)src < t.S;
            uint16_t mv = 0, ch = 0xFFFF;
            uint8_t ut = 0;
            int32_t na = 0;
            double w = 0.0;
            float pr = 0.0f;
            if (dv) {
                mv = t.mv[src];
                ut = t.ut[src];
                ch = t.ch[src];
                na = t.na[src];
                w = t.w[src];
                pr = t.pr[src];
            }
            const bool in = dv && (int)ch >= r && (int)ch < n;
            const uint16_t nch = remap[in ? (int)ch : r];  // always a valid entry: no branch around the load
            vm_drain();  // every load of the step has returned before any of its stores is issued
            if (dv) {
                t.mv[d] = mv;
                t.ut[d] = ut;
                t.ch[d] = in ? nch : (uint16_t)0xFFFF;
                t.na[d] = na;
                t.w[d] = w;
                t.pr[d] = pr;
            }
            wave_sync_mem();
        }
    }
    vm_drain();
}

// Pass 4: the moved records' links, one node a lane: the parent through the table (it still
// holds an old id >= r: a kept node's parent is kept), the depth counted from the new root, the
// new base; the new root as puct_begin_kernel writes a root.
__device__ void reroot_link(ChessNode *T, const uint16_t *remap, const uint32_t *rbase, int kept, int n, int r,
                            int rdepth) {
    for (int id = (int)lane_id(); id < kept; id += 64) {
        ChessNode *N = &T[id];
        const uint32_t par = N->parent;
        const bool in = par >= (uint32_t)r && par < (uint32_t)n;
        const uint16_t np = remap[in ? par : (uint32_t)r];
        N->base = rbase[id];
        N->depth = (uint16_t)((int)N->depth - rdepth);
        N->parent = (id == 0 || !in) ? (uint16_t)0xFFFF : np;
        if (id == 0) N->pact = 0xFFFF;
    }
    vm_drain();
}

__global__ __launch_bounds__(64) void puct_reroot_kernel(ChessParams p) {
    __shared__ CLds L;
    __shared__ uint32_t tgt[18];
    const int gl = blockIdx.x;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    const CTree t = ctree(p, g);
    int32_t *ctl = p.ca.ctl + (size_t)g * kCtlWords;
    uint16_t *remap = p.ca.remap + (size_t)g * p.M;
    uint32_t *rbase = p.ca.rbase + (size_t)g * p.M;
    const uint32_t lane = lane_id();
    if (lane < 18) {
        const uint32_t w = ((const uint32_t *)&p.roots[gl])[lane];
        tgt[lane] = w;
        ((uint32_t *)&L.st)[lane] = w;
        ((uint32_t *)&p.ca.roots[g])[lane] = w;
    }
    wave_sync_mem();
    const int n = uni(ctl[cNodes]), s = uni(ctl[cSlots]);
    int r = -1, kept = 0, kslots = 0;
    if (uni(ctl[cDone]) == 1 && n >= 2 && n <= p.M && s >= 0 && (int64_t)s <= t.S) r = uni(reroot_find(t, tgt, n, s));
    if (r > 0) {  // evaluated, with legal moves
        const int nm = uni((int)t.nodes[r].nmoves);
        if (!uni((int)t.nodes[r].evaluated) || nm == 0 || nm > ZC_CHESS_MAX_MOVES) r = -1;
    }
    if (r > 0) {
        kept = reroot_number(t, remap, rbase, n, s, r, kslots);
        // room for this search's nodes and for kChessSlotsPerNode slots each, as a fresh search has
        if ((int64_t)kept + p.sims - 1 > (int64_t)p.M ||
            (int64_t)kslots + (int64_t)kChessSlotsPerNode * (p.sims - 1) > t.S)
            kept = 0;
    }
    int slots = 0, status = 0;
    if (kept) {
        const int rdepth = uni((int)t.nodes[r].depth);
        reroot_move_records(t.nodes, remap, n, r);
        reroot_move_slots(t, remap, rbase, kept, n, r);
        reroot_link(t.nodes, remap, rbase, kept, n, r, rdepth);
        slots = kslots;
        if (p.dir_eps > 0.0f) {  // on the kept priors
            const int nm = uni((int)t.nodes[0].nmoves);
            MoveRegs<4> pr;
#pragma unroll
            for (int q = 0; q < 4; ++q) pr.v[q] = q * 64 + (int)lane < nm ? t.pr[q * 64 + (int)lane] : 0.0f;
            pr = mix_root_noise(p, g, gl, nm, pr);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q * 64 + (int)lane < nm) t.pr[q * 64 + (int)lane] = pr.v[q];
        }
    } else {  // as puct_begin_kernel
        create_node(t, L, 0, 0xFFFF, 0xFFFF, 0, slots, status);
        if (!status && uni((int)t.nodes[0].nmoves) == 0) status = ZC_STATUS_NO_MOVES;
    }
    if (lane == 0) ctl[cSlots] = slots;
    search_reset<PCtl>(p, ctl, gl, kept, status);
}

__global__ __launch_bounds__(64) void puct_select_kernel(ChessParams p) {
    __shared__ CLds L;
    const int gl = blockIdx.x;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    const CTree t = ctree(p, g);
    int32_t *ctl = p.ca.ctl + (size_t)g * kCtlWords;
    const uint32_t lane = lane_id();
    int status = uni(ctl[cStatus]);
    int nb = select_leaves<PCtl>(p, ctl, status);
    int nnodes = uni(ctl[cNodes]), slots = uni(ctl[cSlots]);
    uint32_t *paths = p.ca.paths + (size_t)g * p.max_batch * kChessPath;
    uint32_t *meta = p.ca.meta + (size_t)g * p.max_batch;
    Counters cn;
    int j = 0;
    for (; j < nb && !status; ++j) {
        int d = 0;
        uint32_t pathv = 0;
        bool created = false;
        const int leaf = p.flush == 0 ? 0 : puct_walk(p, t, L, nnodes, slots, status, d, pathv, cn, created);
        if (lane < (uint32_t)kChessPath) paths[(size_t)j * kChessPath + lane] = pathv;
        if (lane == 0) meta[j] = (uint32_t)leaf | ((uint32_t)d << 16) | (created ? kMetaCreated : 0u);
    }
    nb = select_done<PCtl>(p, ctl, gl, nnodes, status, nb, cn);
    // the slots in use before this flush, for puct_commit_kernel: its blocks must not read
    // cSlots, which the block of the flush's last created node rewrites in the same grid
    if (lane == 0) ctl[cSlots0] = slots;
    const size_t obase = (size_t)gl * p.bs;
    for (int k = 0; k < nb; ++k) {
        const ChessNode *N = &t.nodes[uni(meta[k]) & 0xFFFFu];  // (the position is in the record already)
        if (p.leaves && lane < 18) ((uint32_t *)&p.leaves[obase + k])[lane] = ((const uint32_t *)&N->st)[lane];
        if (p.planes) {
            const uint32_t pc = N->st.board[lane];
            const char pieces[12] = {'P', 'N', 'B', 'R', 'Q', 'K', 'p', 'n', 'b', 'r', 'q', 'k'};
            int which = -1;
            for (int q = 0; q < 12; ++q)
                if (pc == (uint8_t)pieces[q]) {
                    which = q;
                    break;
                }
            const int turn = N->st.turn, castle = N->st.castle;
            if (p.planes_f16 == 2) {  // ZC_F16_NHWC32: lane = square, its 32 channels (17 planes, zeros)
                typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
                h8_t v8[4];
#pragma unroll
                for (int q = 0; q < 32; ++q) {
                    float v = 0.0f;
                    if (q < 12) v = q == which ? 1.0f : 0.0f;
                    else if (q == 12) v = turn == 0 ? 1.0f : 0.0f;
                    else if (q < 17) v = (castle >> (q - 13)) & 1 ? 1.0f : 0.0f;
                    v8[q >> 3][q & 7] = (_Float16)v;
                }
                h8_t *o = (h8_t *)((_Float16 *)p.planes + ((obase + k) * 64 + lane) * 32);
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = v8[c];
            } else {
                for (int q = 0; q < 17; ++q) {
                    float v;
                    if (q < 12) v = q == which ? 1.0f : 0.0f;
                    else if (q == 12) v = turn == 0 ? 1.0f : 0.0f;
                    else v = (castle >> (q - 13)) & 1 ? 1.0f : 0.0f;
                    const size_t o = ((obase + k) * 17 + q) * 64 + lane;
                    if (p.planes_f16) ((__half *)p.planes)[o] = __float2half(v);
                    else ((float *)p.planes)[o] = v;
                }
            }
        }
    }
}

// The deferred expansions of a flush, one wave per (leaf, game) whose walk created a node: its
// legal moves (order, capture values, the check flag of a position without moves: create_node's
// generation) into the per-leaf scratch.
__global__ __launch_bounds__(64) void puct_expand_kernel(ChessParams p) {
    __shared__ CLds L;
    const int j = blockIdx.x, gl = blockIdx.y;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    const int32_t *ctl = p.ca.ctl + (size_t)g * kCtlWords;
    if (j >= uni(ctl[cNb])) return;
    const uint32_t mt = uni(p.ca.meta[(size_t)g * p.max_batch + j]);
    if (!(mt & kMetaCreated)) return;
    const CTree t = ctree(p, g);
    const uint32_t lane = lane_id();
    const ChessNode *C = &t.nodes[mt & 0xFFFFu];
    if (lane < 18) ((uint32_t *)&L.st)[lane] = ((const uint32_t *)&C->st)[lane];
    wave_sync_mem();
    const NodeGen gen = create_node_gen(L);
    const size_t x = (size_t)g * p.max_batch + j;
    uint16_t *xm = p.ca.xmv + x * ZC_CHESS_MAX_MOVES;
    for (int k = (int)lane; k < gen.n; k += 64) xm[k] = L.s.legal[k];
    if (lane == 0) {
        p.ca.xinfo[2 * x] = gen.n;
        p.ca.xinfo[2 * x + 1] = (int32_t)(((uint32_t)gen.mat & 0xFFFFu) | ((uint32_t)gen.check << 16));
    }
}

// ... and their commit, one wave per (leaf, game) again: the node's slot range is the slots in
// use before the flush plus the move counts of the nodes created before it in this flush
// (create_node_take's arithmetic, capacity included), then create_node_commit's writes.  The
// last created node of the game publishes the new slot count.
__global__ __launch_bounds__(64) void puct_commit_kernel(ChessParams p) {
    const int j = blockIdx.x, gl = blockIdx.y;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    int32_t *ctl = p.ca.ctl + (size_t)g * kCtlWords;
    const int nb = uni(ctl[cNb]);
    if (j >= nb) return;
    const uint32_t *meta = p.ca.meta + (size_t)g * p.max_batch;
    const uint32_t mt = uni(meta[j]);
    if (!(mt & kMetaCreated)) return;
    const CTree t = ctree(p, g);
    const uint32_t lane = lane_id();
    const size_t x0 = (size_t)g * p.max_batch;
    // the move counts of the nodes created before this one (leaves i < j), and whether a node
    // was created after it (leaves j < i < nb)
    int before = 0;
    bool later = false;
    for (int b = 0; b < nb; b += 64) {
        const int i = b + (int)lane;
        const bool cr = i < nb && (meta[min(i, nb - 1)] & kMetaCreated);
        if (cr && i < j) before += max(p.ca.xinfo[2 * (x0 + i)], 0);
        later |= cr && i > j;
    }
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    const bool last = __ballot(later) == 0ull;
    const int slots0 = uni(ctl[cSlots0]);  // as puct_select_kernel saved it (cSlots changes under this grid)
    int n = uni(p.ca.xinfo[2 * (x0 + j)]);
    const uint32_t mc = (uint32_t)uni(p.ca.xinfo[2 * (x0 + j) + 1]);
    const int base = slots0 + before;
    int status = 0;
    if (n < 0) {
        status = ZC_STATUS_CAPACITY;
        n = 0;
    }
    if ((int64_t)base + n > t.S) {
        status = ZC_STATUS_CAPACITY;
        n = 0;
    }
    const uint16_t *xm = p.ca.xmv + (x0 + j) * ZC_CHESS_MAX_MOVES;
    for (int k = (int)lane; k < n; k += 64) {
        t.mv[base + k] = xm[k];
        t.ut[base + k] = (uint8_t)k;
        t.ch[base + k] = 0xFFFF;
        t.na[base + k] = 0;
        t.w[base + k] = 0.0;
    }
    ChessNode *C = &t.nodes[mt & 0xFFFFu];
    if (lane == 0) {
        C->base = (uint32_t)base;
        C->nmoves = (uint16_t)n;
        C->nu = (uint16_t)n;
        C->material = (int16_t)(mc & 0xFFFFu);
        C->check = (mc >> 16) & 1u;
        if (status) ctl[cStatus] = status;
        if (last) ctl[cSlots] = base + n;  // the flush's last created node
    }
}

__global__ __launch_bounds__(64) void puct_backup_kernel(ChessParams p) {
    const int gl = blockIdx.x;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    const CTree t = ctree(p, g);
    int32_t *ctl = p.ca.ctl + (size_t)g * kCtlWords;
    const uint32_t lane = lane_id();
    const int nb = uni(ctl[cNb]);
    if (uni(ctl[cStatus]) || nb == 0) return;
    const uint32_t *paths = p.ca.paths + (size_t)g * p.max_batch * kChessPath;
    const uint32_t *meta = p.ca.meta + (size_t)g * p.max_batch;
    for (int j = 0; j < nb; ++j) {
        const uint32_t mt = uni(meta[j]);
        const int node = (int)(mt & 0xFFFFu), d = (int)((mt >> 16) & 0xFFu);
        ChessNode *N = &t.nodes[node];
        const int nm = uni((int)N->nmoves);
        const size_t li = (size_t)gl * (p.leaf_rows ? p.leaf_rows : p.bs) + j;
        double v;
        if (nm == 0) {
            v = uni((int)N->check) ? -1.0 : 0.0;  // checkmated side to move / no moves
        } else {
            v = __hiloint2double(uni(__double2hiint(p.values[li])), uni(__double2loint(p.values[li])));
            if (!(fabs(v) < INFINITY)) {  // a NaN or infinite value: the game's backup stops here
                if (lane == 0) ctl[cStatus] = ZC_STATUS_INTERNAL;
                return;
            }
            if (!uni((int)N->evaluated)) {
                // the logits of this node's legal moves (from*64 + to)
                const uint32_t base = uni(N->base);
                MoveRegs<4> lg;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = q * 64 + (int)lane;
                    lg.v[q] = -INFINITY;
                    if (k < nm) {
                        const uint32_t m = t.mv[base + k];
                        const size_t o = li * 4096 + (m & 63u) * 64 + ((m >> 6) & 63u);
                        lg.v[q] = p.logits_f16 ? __half2float(((const __half *)p.logits)[o]) : ((const float *)p.logits)[o];
                    }
                }
                const Priors<4> sm = softmax_priors(lg, nm);
                if (!sm.ok) {
                    if (lane == 0) ctl[cStatus] = ZC_STATUS_INTERNAL;
                    return;
                }
                MoveRegs<4> pr = sm.pr;
                if (node == 0 && p.dir_eps > 0.0f) pr = mix_root_noise(p, g, gl, nm, pr);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = q * 64 + (int)lane;
                    if (k < nm) t.pr[base + k] = pr.v[q];
                }
                if (lane == 0) N->evaluated = 1;
            }
        }
        wave_sync_mem();
        // backup with the virtual loss undone: W += 1 - r on the edge into level l
        if (lane >= 1 && lane <= (uint32_t)d) {
            const uint32_t s = paths[(size_t)j * kChessPath + lane];
            const double r = ((d - (int)lane) & 1) ? -v : v;
            t.w[s] = t.w[s] + 1.0 - r;
        }
        wave_sync_mem();
    }
}

__global__ __launch_bounds__(64) void puct_end_kernel(ChessParams p) {
    const int gl = blockIdx.x;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    const CTree t = ctree(p, g);
    int32_t *ctl = p.ca.ctl + (size_t)g * kCtlWords;
    const uint32_t lane = lane_id();
    const int status = uni(ctl[cStatus]);
    const ChessNode *R = &t.nodes[0];
    const int nm = status == ZC_STATUS_NO_MOVES ? 0 : uni((int)R->nmoves);
    const uint32_t base = uni(R->base);
    for (int j = (int)lane; j < ZC_CHESS_MAX_MOVES; j += 64) {
        p.out_na[(size_t)gl * ZC_CHESS_MAX_MOVES + j] = j < nm ? t.na[base + j] : 0;
        if (p.out_prior) p.out_prior[(size_t)gl * ZC_CHESS_MAX_MOVES + j] = j < nm ? t.pr[base + j] : 0.0f;
    }
    int best = -1;
    if (nm > 0) {
        if (p.temperature <= 0.0f) {  // most visits, first maximum
            int bv = -1, bi = 0x7FFFFFFF;
            for (int b = 0; b < nm; b += 64) {
                const int j = b + (int)lane;
                if (j < nm && t.na[base + j] > bv) {
                    bv = t.na[base + j];
                    bi = j;
                }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const int ov = __shfl_xor(bv, o), oi = __shfl_xor(bi, o);
                if (ov > bv || (ov == bv && oi < bi)) {
                    bv = ov;
                    bi = oi;
                }
            }
            best = uni(bi);
        } else {  // sample proportional to Na^(1/T): inverse CDF over the moves in order
            const double inv_t = 1.0 / (double)p.temperature;
            int32_t top = 0;
            for (int b = 0; b < nm; b += 64) {
                const int j = b + (int)lane;
                if (j < nm) top = max(top, t.na[base + j]);
            }
            for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o));
            const int kb = count_bits(uni(top));
            double tot = 0.0;
            for (int b = 0; b < nm; b += 64) {
                const int j = b + (int)lane;
                tot += j < nm ? temperature_weight(t.na[base + j], kb, inv_t) : 0.0;
            }
            tot = wave_sum_d(tot);
            const double target = temperature_target(p, g, gl, tot);
            double run = 0.0;
            best = nm - 1;
            for (int j = 0; j < nm; ++j) {  // serial scan in move order (<= 256 steps, once per move)
                run += temperature_weight(uni(t.na[base + j]), kb, inv_t);
                if (run > target) {
                    best = j;
                    break;
                }
            }
        }
    }
    if (lane == 0) {
        p.out_move[gl] = (best >= 0 && !status) ? t.mv[base + best] : (uint16_t)0xFFFF;
        search_done<PCtl>(p, ctl, gl, status);
    }
}

}  // namespace

void launch_chess_puct_begin(const ChessParams &p, hipStream_t s) {
    hipLaunchKernelGGL(puct_begin_kernel, dim3(p.n_games), dim3(64), 0, s, p);
}
void launch_chess_puct_reroot(const ChessParams &p, hipStream_t s) {
    hipLaunchKernelGGL(puct_reroot_kernel, dim3(p.n_games), dim3(64), 0, s, p);
}
void launch_chess_puct_forget(const ChessParams &p, hipStream_t s) {
    launch_puct_forget(p.ca.ctl, p.first_game, p.n_games, PCtl::done, s);
}
void launch_chess_puct_forget_fresh(const ChessParams &p, const int32_t *slot, hipStream_t s) {
    launch_puct_forget_fresh(p.ca.ctl, p.first_game, p.n_games, PCtl::done, slot, s);
}
void launch_chess_puct_select(const ChessParams &p, hipStream_t s) {
    hipLaunchKernelGGL(puct_select_kernel, dim3(p.n_games), dim3(64), 0, s, p);
    if (p.flush > 0) {  // flush 0 evaluates the root alone: nothing is created
        hipLaunchKernelGGL(puct_expand_kernel, dim3(p.bs, p.n_games), dim3(64), 0, s, p);
        hipLaunchKernelGGL(puct_commit_kernel, dim3(p.bs, p.n_games), dim3(64), 0, s, p);
    }
}
void launch_chess_puct_backup(const ChessParams &p, hipStream_t s) {
    hipLaunchKernelGGL(puct_backup_kernel, dim3(p.n_games), dim3(64), 0, s, p);
}
void launch_chess_puct_end(const ChessParams &p, hipStream_t s) {
    hipLaunchKernelGGL(puct_end_kernel, dim3(p.n_games), dim3(64), 0, s, p);
}

}  // namespace zc
