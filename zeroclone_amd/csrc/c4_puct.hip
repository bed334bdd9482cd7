// c4_puct.hip — AlphaZero-style PUCT search for Connect4 on gfx950 (SURVEY.md §8 a21 on the
// target game).  The reference has no counterpart: its search is plain UCT with one-at-a-
// time expansion and random rollouts (engine/mcts/src/mcts.cpp:41-78), its network plugin a
// value net only (engine/value_functions.py:61-99).  This extension keeps the reference's
// game rules (engine/games/connect4/c4_backend.py: legal moves in CPython set order,
// check_win on the last mover, check_draw on a full board), its flush protocol and the
// leaf value convention, and changes the search to the chess PUCT form (chess_puct.hip):
//
//   select  a = first argmax  Q(a) + c_puct * P(a) * sqrt(sum_b N(b)) / (1 + N(a)),
//           Q(a) = W(a) / N(a) (0 when N(a) = 0); the walk stops at an edge without a child
//           (the child is created and is the leaf), at a terminal position (four in a row
//           for the last mover, or a full board) or at a node still waiting for its
//           evaluation; virtual loss on every edge walked (N += 1, W -= 1) until backup;
//   backup  per leaf in pending order: a first evaluation sets the node's priors from the
//           policy head's 7 column logits over the legal columns; every edge then takes
//           W += 1 - r with r = the leaf value, alternating in sign (N already counted); a
//           terminal leaf's value is -1 (the side to move has lost) or 0;
//   reuse   (opt-in, zc_c4_puct_begin_reuse) the subtree of the position now at the root, one
//           or two plies below the last search's root, is compacted in place into the next
//           tree.
//
// What the search shares with the chess one is in puct_common.h, each rule beside its code:
// the flush schedule (flush 0 evaluates the root alone), the control words, the softmax of
// the priors, the root noise, the temperature sample and the re-root's numbering and record
// move.  This file holds the game: the node, the walk, the planes and the columns.
//
// Node = one 192-byte record, slot k (a move, in the node's move-list order) in lane k:
// everything a selection step reads is one coalesced load per field.  One wave per game.
// Specification in executable form: oracle/puct_ref.py (C4Rules).
#include <hip/hip_fp16.h>

#include "c4_device.h"
#include "puct_common.h"

namespace zc {
namespace {

static_assert(sizeof(C4PNode) == 192, "C4PNode is 192 bytes");

// the search's control words (puct_common.h) in this game's ctl block
struct PCtl {
    static constexpr int nodes = 0, status = 1, nb = 2, exp = 3, depth = 4, done = 5, reused = 6;
};

__device__ __forceinline__ C4PNode *pnodes(const C4PuctParams &p, int g) { return p.nodes + (size_t)g * p.M; }

// Node(state): move list in CPython set order (c4_backend.get_legal_moves), none at a
// terminal position (the last mover has four, or the board is full).
__device__ __forceinline__ void pnode_init(C4PNode *N, uint64_t s0, uint64_t s1, int turn, int parent, int pact,
                                           int depth) {
    const uint32_t lane = lane_id();
    const uint64_t occ = s0 | s1;
    const bool won = has_four(turn ? s0 : s1);  // check_win: the last mover's stones
    const int lm = legal_mask(occ);
    const uint32_t ow = d_order[lm];
    const int nm = (won || occ == kFull) ? 0 : (int)((ow >> 24) & 15u);
    if (lane == 0) {
        N->s0 = s0;
        N->s1 = s1;
        N->order = ow;
        N->turn = (uint8_t)turn;
        N->nmoves = (uint8_t)nm;
        N->evaluated = 0;
        N->won = won ? 1 : 0;
        N->parent = (uint16_t)parent;
        N->pact = (uint8_t)pact;
        N->depth = (uint8_t)depth;
    }
    if (lane < kSlots) {
        N->child[lane] = 0xFFFF;
        N->na[lane] = 0;
        N->pr[lane] = 0.0f;
        N->w[lane] = 0.0;
    }
}

__global__ __launch_bounds__(64) void c4_puct_begin_kernel(C4PuctParams p) {
    const int gl = blockIdx.x;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    const zc_c4_state root = p.roots[gl];
    const uint64_t s0 = uni64(root.stones[0]), s1 = uni64(root.stones[1]);
    const int turn = uni(root.turn);
    int32_t *ctl = p.ctl + (size_t)g * kCtlWords;
    int status = 0;
    if (!valid_state(s0, s1, turn)) {
        status = ZC_STATUS_BAD_STATE;
    } else {
        C4PNode *N = pnodes(p, g);
        pnode_init(N, s0, s1, turn, 0xFFFF, 0xFF, 0);
        wave_mem_order();
        if (uni((int)N->nmoves) == 0) status = ZC_STATUS_NO_MOVES;
    }
    search_reset<PCtl>(p, ctl, gl, 0, status);
}

// ---- tree reuse: the subtree of the position now at the root becomes the next tree ----
// reroot_find names the new root, reroot_number and puct_common.h's reroot_move_records
// compact its subtree, and reroot_link renumbers the moved records' parent and child links.

// The node holding (s0, s1, turn) one ply below the old root, else two plies below it; the
// first in slot order (slot of the child, then slot of the grandchild), or -1.
__device__ int reroot_find(const C4PNode *T, int n, uint64_t s0, uint64_t s1, int turn) {
    const uint32_t lane = lane_id();
    const int nm0 = uni((int)T[0].nmoves);
    auto holds = [&](int id) {
        return id > 0 && id < n && T[id].s0 == s0 && T[id].s1 == s1 && (int)T[id].turn == turn;
    };
    const int c1 = (int)lane < min(nm0, kSlots) ? (int)T[0].child[lane] : 0xFFFF;
    uint64_t hit = __ballot(holds(c1));
    if (hit) return __builtin_amdgcn_readlane(c1, __builtin_ctzll(hit));
    const int c = __shfl(c1, (int)(lane >> 3));  // lane = child slot * 8 + grandchild slot
    int c2 = 0xFFFF;
    if (c > 0 && c < n && (int)(lane & 7u) < (int)T[c].nmoves) c2 = (int)T[c].child[lane & 7u];
    hit = __ballot(holds(c2));
    if (hit) return __shfl(c2, __builtin_ctzll(hit));
    return -1;
}

// Pass 1: remap[i] = the new id of node i of r's subtree, 0xFFFF for any other node i >= r
// (ids below r are never kept and never looked up).  Returns the number of nodes kept.
__device__ int reroot_number(const C4PNode *T, uint16_t *remap, int n, int r) {
    const uint32_t lane = lane_id();
    int cnt = 0;
    for (int base = r; base < n; base += 64) {
        const int i = base + (int)lane;
        const bool valid = i < n;
        const int par = valid ? (int)T[i].parent : 0xFFFF;
        const uint64_t b = reroot_mark(i, valid, par, r, base, remap);
        const bool k = (b >> lane) & 1ull;
        const int id = cnt + __popcll(b & ((1ull << lane) - 1ull));
        if (valid) remap[i] = k ? (uint16_t)id : (uint16_t)0xFFFF;
        cnt += __popcll(b);
        vm_drain();  // the next chunk's lanes read these entries
    }
    return cnt;
}

// Pass 2 is reroot_move_records.  Pass 3: the moved records' links, one node a lane: parent
// and children through the table (they still hold old ids, all >= r: a kept node's parent and
// children are kept), depth counted from the new root.  Piece 1 of a record holds parent /
// pact / depth, piece 2 its eight children; the nine table reads of a node are independent
// loads.
__device__ void reroot_link(C4PNode *T, const uint16_t *remap, int kept, int n, int r, int rdepth) {
    for (int id = (int)lane_id(); id < kept; id += 64) {
        uint4 *rec = reinterpret_cast<uint4 *>(T + id);
        const uint32_t link = rec[1].z;
        const uint4 ch = rec[2];
        const uint32_t old[9] = {ch.x & 0xFFFFu, ch.x >> 16, ch.y & 0xFFFFu, ch.y >> 16, ch.z & 0xFFFFu,
                                 ch.z >> 16,     ch.w & 0xFFFFu, ch.w >> 16, link & 0xFFFFu};
        uint32_t now[9];
#pragma unroll
        for (int h = 0; h < 9; ++h) {
            const bool in = old[h] >= (uint32_t)r && old[h] < (uint32_t)n;
            const uint32_t m = remap[in ? old[h] : (uint32_t)r];  // always a valid entry: no branch around the load
            now[h] = in ? m : 0xFFFFu;
        }
        rec[2] = make_uint4(now[0] | (now[1] << 16), now[2] | (now[3] << 16), now[4] | (now[5] << 16),
                            now[6] | (now[7] << 16));
        const uint32_t pact = (link >> 16) & 0xFFu, dep = link >> 24;
        reinterpret_cast<uint32_t *>(rec + 1)[2] =
            id == 0 ? 0x00FFFFFFu : now[8] | (pact << 16) | ((dep - (uint32_t)rdepth) << 24);
    }
    vm_drain();
}

__global__ __launch_bounds__(64) void c4_puct_reroot_kernel(C4PuctParams p) {
    const int gl = blockIdx.x;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    const zc_c4_state root = p.roots[gl];
    const uint64_t s0 = uni64(root.stones[0]), s1 = uni64(root.stones[1]);
    const int turn = uni(root.turn);
    int32_t *ctl = p.ctl + (size_t)g * kCtlWords;
    C4PNode *T = pnodes(p, g);
    uint16_t *remap = p.remap + (size_t)g * p.M;
    const uint32_t lane = lane_id();
    int status = 0, kept = 0;
    if (!valid_state(s0, s1, turn)) {
        status = ZC_STATUS_BAD_STATE;
    } else {
        const int n = uni(ctl[PCtl::nodes]);
        int r = -1;
        if (uni(ctl[PCtl::done]) == 1 && n >= 2 && n <= p.M) r = uni(reroot_find(T, n, s0, s1, turn));
        if (r > 0 && (!uni((int)T[r].evaluated) || uni((int)T[r].nmoves) == 0)) r = -1;
        if (r > 0) {
            kept = reroot_number(T, remap, n, r);
            if (kept + p.sims - 1 > p.M) kept = 0;  // no room for this search's nodes: start afresh
        }
        if (kept) {
            const int rdepth = uni((int)T[r].depth);
            reroot_move_records(T, remap, n, r);
            reroot_link(T, remap, kept, n, r, rdepth);
            if (p.dir_eps > 0.0f) {  // on the kept priors
                const int nm = uni((int)T[0].nmoves);
                const MoveRegs<1> pr = mix_root_noise(p, g, gl, nm, MoveRegs<1>{{(int)lane < nm ? T[0].pr[lane] : 0.0f}});
                if ((int)lane < nm) T[0].pr[lane] = pr.v[0];
            }
        } else {
            pnode_init(T, s0, s1, turn, 0xFFFF, 0xFF, 0);
            wave_mem_order();
            if (uni((int)T->nmoves) == 0) status = ZC_STATUS_NO_MOVES;
        }
    }
    search_reset<PCtl>(p, ctl, gl, kept, status);
}

// One PUCT walk + expansion; returns the leaf and its depth, the edges of its path in lanes
// 1..depth of pathv (node | slot << 16).  Applies the virtual loss on every edge it takes.
__device__ int c4_puct_walk(const C4PuctParams &p, C4PNode *T, int &nnodes, int &status, int &ldepth,
                            uint32_t &pathv, Counters &cn) {
    const uint32_t lane = lane_id();
    const uint32_t k = lane & 7u;
    int node = 0, depth = 0;
    pathv = 0;
    for (;;) {
        C4PNode *N = &T[node];
        const int nm = uni((int)N->nmoves);
        if (nm == 0 || !uni((int)N->evaluated)) break;  // terminal, or a leaf still pending
        if (depth >= kMaxDepth - 2) {  // unreachable (a Connect4 game is <= 42 plies)
            status = ZC_STATUS_INTERNAL;
            break;
        }
        const bool valid = (int)k < nm;
        const int32_t na = valid ? N->na[k] : 0;
        const double wk = valid ? N->w[k] : 0.0;
        const float pk = valid ? N->pr[k] : 0.0f;
        const uint32_t chk = valid ? (uint32_t)N->child[k] : 0xFFFFu;  // with the others: no dependent load after the argmax
        // sum_b N(b): lanes 0..7 (integers: exact in any order)
        int tot = (lane < 8u) ? na : 0;
        tot += dpp<0xB1>(tot);
        tot += dpp<0x4E>(tot);
        tot += dpp<0x141>(tot);
        const double sq = sqrt((double)uni(tot));
        const double q = na > 0 ? wk / (double)na : 0.0;
        double v = valid ? q + p.c * (double)pk * sq / (double)(1 + na) : -INFINITY;
        int bi = (int)k;
        argmax8(v, bi);
        const int best = uni(bi);
        if (lane == 0) {  // virtual loss: one visit lost by this node's mover
            N->na[best] = N->na[best] + 1;
            N->w[best] = N->w[best] - 1.0;
        }
        ++depth;
        if (lane == (uint32_t)depth) pathv = (uint32_t)node | ((uint32_t)best << 16);
        const int child = (int)(uint32_t)__builtin_amdgcn_readlane((int)chk, best);
        if (child != 0xFFFF) {
            node = child;
            continue;
        }
        // expand the edge: the child position (c4_backend.play_move), its move list
        const int id = nnodes;
        if (id >= p.M) {
            status = ZC_STATUS_CAPACITY;
            break;
        }
        ++nnodes;
        const uint64_t s0 = uni64(N->s0), s1 = uni64(N->s1);
        const int turn = uni((int)N->turn);
        const int col = (int)((uni(N->order) >> (3 * best)) & 7u);
        const uint64_t bit = drop_bit(s0 | s1, col);
        pnode_init(&T[id], turn ? s0 : s0 | bit, turn ? s1 | bit : s1, turn ^ 1, node, best, depth);
        if (lane == 0) N->child[best] = (uint16_t)id;
        cn.add(cn.expansions, 1);
        cn.add(cn.depth_sum, depth);
        wave_mem_order();
        node = id;
        break;
    }
    ldepth = depth;
    return node;
}

__global__ __launch_bounds__(64) void c4_puct_select_kernel(C4PuctParams p) {
    const int gl = blockIdx.x;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    C4PNode *T = pnodes(p, g);
    int32_t *ctl = p.ctl + (size_t)g * kCtlWords;
    const uint32_t lane = lane_id();
    int status = uni(ctl[PCtl::status]);
    int nb = select_leaves<PCtl>(p, ctl, status);
    int nnodes = uni(ctl[PCtl::nodes]);
    uint32_t *paths = p.paths + (size_t)g * p.max_batch * kMaxDepth;
    uint32_t *meta = p.meta + (size_t)g * p.max_batch;
    Counters cn;
    for (int j = 0; j < nb && !status; ++j) {
        int d = 0;
        uint32_t pathv = 0;
        const int leaf = p.flush == 0 ? 0 : c4_puct_walk(p, T, nnodes, status, d, pathv, cn);
        if (lane < (uint32_t)kMaxDepth) paths[(size_t)j * kMaxDepth + lane] = pathv;
        if (lane == 0) meta[j] = (uint32_t)leaf | ((uint32_t)d << 16);
    }
    nb = select_done<PCtl>(p, ctl, gl, nnodes, status, nb, cn);
    // the pending flush's leaves: states, and state_to_tensor planes (c4_backend.py:52-61:
    // [2][6][7], plane 0 = the side to move's stones, row 0 = top = bit row 5 - r)
    const size_t obase = (size_t)gl * p.bs;
    for (int j = (int)lane; j < nb; j += 64) {
        const C4PNode *N = &T[meta[j] & 0xFFFFu];
        if (p.leaves) {
            zc_c4_state s;
            s.stones[0] = N->s0;
            s.stones[1] = N->s1;
            s.turn = N->turn;
            s.reserved = 0;
            p.leaves[obase + j] = s;
        }
    }
    if (p.planes) {
        for (int idx = (int)lane; idx < nb * 84; idx += 64) {
            const int j = idx / 84, e = idx - j * 84;
            const int pl = e / 42, cell = e - pl * 42;
            const int r = cell / 7, col = cell - r * 7;
            const C4PNode *N = &T[meta[j] & 0xFFFFu];
            const uint64_t stones = (pl == (int)N->turn) ? N->s0 : N->s1;
            const float v = (float)((stones >> (7 * col + 5 - r)) & 1ull);
            const size_t o = (obase + j) * 84 + e;
            if (p.planes_f16) ((__half *)p.planes)[o] = __float2half(v);
            else ((float *)p.planes)[o] = v;
        }
    }
}

__global__ __launch_bounds__(64) void c4_puct_backup_kernel(C4PuctParams p) {
    const int gl = blockIdx.x;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    C4PNode *T = pnodes(p, g);
    int32_t *ctl = p.ctl + (size_t)g * kCtlWords;
    const uint32_t lane = lane_id();
    const int nb = uni(ctl[PCtl::nb]);
    if (uni(ctl[PCtl::status]) || nb == 0) return;
    const uint32_t *paths = p.paths + (size_t)g * p.max_batch * kMaxDepth;
    const uint32_t *meta = p.meta + (size_t)g * p.max_batch;
    for (int j = 0; j < nb; ++j) {
        const uint32_t mt = uni(meta[j]);
        const int node = (int)(mt & 0xFFFFu), d = (int)(mt >> 16);
        C4PNode *N = &T[node];
        const int nm = uni((int)N->nmoves);
        const size_t li = (size_t)gl * (p.leaf_rows ? p.leaf_rows : p.bs) + j;
        double v;
        if (nm == 0) {
            v = uni((int)N->won) ? -1.0 : 0.0;  // the side to move has lost / a full board
        } else {
            v = __hiloint2double(uni(__double2hiint(p.values[li])), uni(__double2loint(p.values[li])));
            if (!(fabs(v) < INFINITY)) {  // a NaN or infinite value: the game's backup stops here
                if (lane == 0) ctl[PCtl::status] = ZC_STATUS_INTERNAL;
                return;
            }
            if (!uni((int)N->evaluated)) {
                // the logits of the node's legal columns, in move-list order (slot k = lane k)
                const bool valid = lane < (uint32_t)nm;
                const uint32_t col = (uni(N->order) >> (3 * (lane & 7u))) & 7u;
                MoveRegs<1> lg{{-INFINITY}};
                if (valid)
                    lg.v[0] = p.logits_f16 ? __half2float(((const __half *)p.logits)[li * 7 + col])
                                           : ((const float *)p.logits)[li * 7 + col];
                const Priors<1> sm = softmax_priors(lg, nm);
                if (!sm.ok) {
                    if (lane == 0) ctl[PCtl::status] = ZC_STATUS_INTERNAL;
                    return;
                }
                MoveRegs<1> pr = sm.pr;
                if (node == 0 && p.dir_eps > 0.0f) pr = mix_root_noise(p, g, gl, nm, pr);
                if (valid) N->pr[lane] = pr.v[0];
                if (lane == 0) N->evaluated = 1;
            }
        }
        wave_mem_order();
        // backup with the virtual loss undone: W += 1 - r on the edge into level l
        if (lane >= 1 && lane <= (uint32_t)d) {
            const uint32_t e = paths[(size_t)j * kMaxDepth + lane];
            C4PNode *P = &T[e & 0xFFFFu];
            const int s = (int)(e >> 16);
            const double r = ((d - (int)lane) & 1) ? -v : v;
            P->w[s] = P->w[s] + 1.0 - r;
        }
        wave_mem_order();
    }
}

__global__ __launch_bounds__(64) void c4_puct_end_kernel(C4PuctParams p) {
    const int gl = blockIdx.x;
    if (gl >= p.n_games) return;
    const int g = p.first_game + gl;
    const C4PNode *R = pnodes(p, g);
    int32_t *ctl = p.ctl + (size_t)g * kCtlWords;
    const uint32_t lane = lane_id();
    const uint32_t k = lane & 7u;
    const int status = uni(ctl[PCtl::status]);
    const int nm = status ? 0 : uni((int)R->nmoves);
    const uint32_t ow = status ? 0u : uni(R->order);
    const int32_t na = (int)k < nm ? R->na[k] : -1;
    if (lane < 7) {  // visits and priors per column
        int pos = -1;
        for (int s = 0; s < nm; ++s)
            if ((int)((ow >> (3 * s)) & 7u) == (int)lane) pos = s;
        p.out_na[(size_t)gl * 7 + lane] = pos >= 0 ? R->na[pos] : 0;
        if (p.out_prior) p.out_prior[(size_t)gl * 7 + lane] = pos >= 0 ? R->pr[pos] : 0.0f;
    }
    int best = -1;
    if (nm > 0) {
        if (p.temperature <= 0.0f) {  // most visits, first maximum in move-list order
            int bv = na, bi = (int)k;
            argmax8(bv, bi);
            best = uni(bi);
        } else {  // sample proportional to Na^(1/T): inverse CDF over the moves in order
            const double inv_t = 1.0 / (double)p.temperature;
            int32_t top = 0;
            for (int j = 0; j < nm; ++j) top = max(top, uni(R->na[j]));
            const int kb = count_bits(top);
            double tot = 0.0;
            for (int j = 0; j < nm; ++j) tot += temperature_weight(uni(R->na[j]), kb, inv_t);
            const double target = temperature_target(p, g, gl, tot);
            double run = 0.0;
            best = nm - 1;
            for (int j = 0; j < nm; ++j) {
                run += temperature_weight(uni(R->na[j]), kb, inv_t);
                if (run > target) {
                    best = j;
                    break;
                }
            }
        }
    }
    if (lane == 0) {
        p.out_move[gl] = best >= 0 ? (int)((ow >> (3 * best)) & 7u) : -1;
        search_done<PCtl>(p, ctl, gl, status);
    }
}

}  // namespace

void launch_c4_puct_begin(const C4PuctParams &p, hipStream_t s) {
    hipLaunchKernelGGL(c4_puct_begin_kernel, dim3(p.n_games), dim3(64), 0, s, p);
}
void launch_c4_puct_reroot(const C4PuctParams &p, hipStream_t s) {
    hipLaunchKernelGGL(c4_puct_reroot_kernel, dim3(p.n_games), dim3(64), 0, s, p);
}
void launch_c4_puct_forget(const C4PuctParams &p, hipStream_t s) {
    launch_puct_forget(p.ctl, p.first_game, p.n_games, PCtl::done, s);
}
void launch_c4_puct_forget_fresh(const C4PuctParams &p, const int32_t *slot, hipStream_t s) {
    launch_puct_forget_fresh(p.ctl, p.first_game, p.n_games, PCtl::done, slot, s);
}
void launch_c4_puct_select(const C4PuctParams &p, hipStream_t s) {
    hipLaunchKernelGGL(c4_puct_select_kernel, dim3(p.n_games), dim3(64), 0, s, p);
}
void launch_c4_puct_backup(const C4PuctParams &p, hipStream_t s) {
    hipLaunchKernelGGL(c4_puct_backup_kernel, dim3(p.n_games), dim3(64), 0, s, p);
}
void launch_c4_puct_end(const C4PuctParams &p, hipStream_t s) {
    hipLaunchKernelGGL(c4_puct_end_kernel, dim3(p.n_games), dim3(64), 0, s, p);
}

}  // namespace zc
