// evalcache.hip — a device-resident cache of network evaluations (include/zeroclone.h,
// "evaluation cache"): a set-associative table keyed by the compact leaf row, and the three
// kernels that carry a flush through it (probe -> counted network on the misses -> commit and
// finish).
//
// The table, ZC_EVALCACHE_WAYS ways per set and a power-of-two number of sets, in one block:
//
//   [header 64 B: epoch u32][meta u32 x E][keys key_bytes x E][values f64 x E][logits lstride x E]
//
// E = ways * sets entries, lstride = logit_bytes rounded up to 16, every array 16-byte aligned.
// An entry's meta word is 0 while it is empty, else (tag << 16) | epoch: a 16-bit tag of the
// key's hash (never 0) that only pre-filters a lookup — a hit is full-key equality — and the
// low 16 bits of the commit launch that wrote it.  The epoch is what keeps two waves of one
// commit launch off one entry: an entry is claimed with one atomicCAS on its meta word, and a
// word that carries the running launch's epoch is not claimable again until the next launch.
//
// One table belongs to one stream: probe and commit are ordered by the stream, so a probe never
// runs beside a commit and there is no reader / writer protocol.  Within a commit launch no
// wave reads a key or a payload; the meta words are read and claimed with device-scope atomics.
//
// There is one flush path with two switches, both compile-time parameters of the kernels.
// CLAIMS (the merged and the routed calls): a key that several of a flush's rows hold is
// evaluated once, with or without a table.  ROUTED (the routed calls): an arena's flush, rows of
// two networks, goes through one probe and one commit over a table, a dense list and a set of
// counters per network.  The host side is one description of a flush (Flush) and one check of it;
// the six entry points fill it in.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zeroclone.h"

namespace {

constexpr int WAYS = ZC_EVALCACHE_WAYS;
static_assert(WAYS == 8, "a set's ways are looked up by lanes 0..7 and picked by three hash bits");
constexpr int HEADER_BYTES = 64;
constexpr int BLOCK = 512, WAVES = BLOCK / 64;   // one wave per row
constexpr int MAX_KEY_WORDS = 64;                // a lane per key word
constexpr int STATS = ZC_EVALCACHE_STAT_MERGED + 1;   // a network's counters in the routed calls

struct Table {
    uint32_t *epoch;
    uint32_t *meta;
    uint64_t *keys;
    double *values;
    uint8_t *logits;
    uint32_t set_mask;
    int kw;               // key words (8 bytes each)
    int64_t logit_bytes, lstride;
};

// false: the sizes are outside what the table covers
bool layout(int64_t entries, int32_t key_bytes, int32_t logit_bytes, int64_t *sets_out, int64_t *bytes_out) {
    if (entries < 1 || entries > ((int64_t)1 << 30)) return false;
    if (key_bytes < 8 || (key_bytes & 7) || key_bytes > 8 * MAX_KEY_WORDS) return false;
    if (logit_bytes < 0 || (logit_bytes & 1) || logit_bytes > (1 << 20)) return false;
    int64_t sets = 1;
    while (sets * 2 * WAYS <= entries) sets *= 2;
    const int64_t E = sets * WAYS, lstride = ((int64_t)logit_bytes + 15) & ~(int64_t)15;
    if (sets_out) *sets_out = sets;
    if (bytes_out) *bytes_out = HEADER_BYTES + E * (4 + (int64_t)key_bytes + 8 + lstride);
    return true;
}

// has_table false ("no table": d_table NULL with entries 0): t's sizes alone are set.
bool make_table(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes, Table *t,
                bool has_table = true) {
    int64_t sets;
    if (has_table && (!d_table || ((uintptr_t)d_table & 15))) return false;
    if (!layout(has_table ? entries : WAYS, key_bytes, logit_bytes, &sets, nullptr)) return false;
    *t = Table{};
    t->kw = key_bytes / 8;
    t->logit_bytes = logit_bytes;
    t->lstride = ((int64_t)logit_bytes + 15) & ~(int64_t)15;
    if (!has_table) return true;
    const int64_t E = sets * WAYS;
    uint8_t *p = (uint8_t *)d_table;
    t->epoch = (uint32_t *)p;
    t->meta = (uint32_t *)(p + HEADER_BYTES);
    t->keys = (uint64_t *)(p + HEADER_BYTES + E * 4);
    t->values = (double *)((uint8_t *)t->keys + E * key_bytes);
    t->logits = (uint8_t *)(t->values + E);
    t->set_mask = (uint32_t)(sets - 1);
    return true;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

// The hash of a key whose word `lane` this lane holds (lanes at or past kw hold nothing): every
// word mixed with its position, xor-ed across the wave, mixed again.  The same in every lane.
__device__ __forceinline__ uint64_t key_hash(uint64_t word, int lane, int kw) {
    uint64_t h = lane < kw ? mix64(word + 0x9E3779B97F4A7C15ULL * (uint64_t)(lane + 1)) : 0;
    uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
    for (int d = 32; d; d >>= 1) {
        lo ^= (uint32_t)__shfl_xor((int)lo, d, 64);
        hi ^= (uint32_t)__shfl_xor((int)hi, d, 64);
    }
    return mix64(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ uint32_t hash_tag(uint64_t h) {
    const uint32_t t = (uint32_t)(h >> 48);
    return t ? t : 1u;
}

// `bytes` from src to dst by the lanes of one wave, at the widest access (16, 8, 4 or 2 bytes)
// that the size and both pointers allow; the choice is the same in every lane.
__device__ __forceinline__ void wave_copy(void *dst, const void *src, int64_t bytes, int lane) {
    const uintptr_t bits = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)bytes;
    if (!(bits & 15)) {
        for (int64_t i = lane; i < bytes / 16; i += 64) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
    } else if (!(bits & 7)) {
        for (int64_t i = lane; i < bytes / 8; i += 64) ((uint2 *)dst)[i] = ((const uint2 *)src)[i];
    } else if (!(bits & 3)) {
        for (int64_t i = lane; i < bytes / 4; i += 64) ((uint32_t *)dst)[i] = ((const uint32_t *)src)[i];
    } else {
        for (int64_t i = lane; i < bytes / 2; i += 64) ((uint16_t *)dst)[i] = ((const uint16_t *)src)[i];
    }
}

__device__ __forceinline__ void count_add(int64_t *p, int v) {
    if (v) atomicAdd((unsigned long long *)p, (unsigned long long)v);
}

// The buffer row of taking-part row r: the first rows_per_game of each game's game_rows rows.
__device__ __forceinline__ int64_t buffer_row(int r, int rows_per_game, int game_rows) {
    const int g = r / rows_per_game;
    return (int64_t)g * game_rows + (r - g * rows_per_game);
}

// The lookup of one wave: lanes 0..7 read the set's meta words and the tag filters the ways;
// for a way that passes, lane i compares key word i (`word`: this lane's).  The entry whose key
// is equal in every word, or -1.
__device__ __forceinline__ int64_t table_find(const Table &t, uint64_t word, uint64_t h, int lane) {
    const int64_t e0 = (int64_t)((uint32_t)h & t.set_mask) * WAYS;
    const uint32_t tag = hash_tag(h);
    const uint32_t meta = lane < WAYS ? t.meta[e0 + lane] : 0u;
    unsigned long long cand = __ballot(lane < WAYS && (meta >> 16) == tag);   // an empty way's tag is 0
    while (cand) {
        const int w = __builtin_ctzll(cand);
        cand &= cand - 1;
        const bool eq = lane < t.kw ? t.keys[(e0 + w) * t.kw + lane] == word : true;
        if (__all(eq)) return e0 + w;
    }
    return -1;
}

// The insert of one wave in a commit launch: the set's first empty way, else the way three hash
// bits pick, unless a way already carries the key's tag (the same key being inserted by another
// wave of this launch, or a tag collision: the insert is dropped either way).  The way is claimed
// with one atomicCAS on its meta word; a wave that loses the claim of an empty way looks at the
// set again, one that loses a victim (or finds it claimed in this launch) drops its insert.
// true: inserted.
__device__ __forceinline__ bool table_insert(const Table &t, uint64_t word, uint64_t h, double v, const uint8_t *lg,
                                             int lane) {
    const int64_t e0 = (int64_t)((uint32_t)h & t.set_mask) * WAYS;
    const uint32_t tag = hash_tag(h), epoch = *t.epoch & 0xFFFFu, mine = (tag << 16) | epoch;
    int64_t entry = -1;
    for (int attempt = 0; attempt < WAYS; ++attempt) {
        const uint32_t meta = lane < WAYS ? __hip_atomic_load(t.meta + e0 + lane, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT)
                                          : 0u;
        if (__ballot(lane < WAYS && (meta >> 16) == tag)) break;
        const unsigned long long empty = __ballot(lane < WAYS && meta == 0u);
        const int w = empty ? __builtin_ctzll(empty) : (int)((h >> 32) & (WAYS - 1));
        const uint32_t old = (uint32_t)__shfl((int)meta, w, 64);
        if (old && (old & 0xFFFFu) == epoch) break;   // claimed in this launch
        int won = 0;
        if (lane == 0) won = atomicCAS(t.meta + e0 + w, old, mine) == old;
        if (__shfl(won, 0, 64)) {
            entry = e0 + w;
            break;
        }
        if (!empty) break;
    }
    if (entry < 0) return false;
    if (lane < t.kw) t.keys[entry * t.kw + lane] = word;
    if (lane == 0) t.values[entry] = v;
    if (t.logit_bytes) wave_copy(t.logits + entry * t.lstride, lg, t.logit_bytes, lane);
    return true;
}

// ---- merging (CLAIMS): a key pending several times in one flush is evaluated once ------------
//
// The flush-local scratch: [claim int32 x S][leader int32 x n_rows], S the power of two with
// 2 * n_rows <= S < 4 * n_rows.  A claim word is 0 while its slot is empty, else 1 + the
// taking-part row that claimed it; leader[r] is the buffer row whose outputs row r takes, or -1
// for a row that takes its own (a hit or a leader).  The probe writes every taking-part row's
// leader word, and the flush's last launch zeroes the claim words again: the scratch is all
// zeros between flushes, and only before the first one does the caller have to make it so.

struct Merge {
    int32_t *claim;
    int32_t *leader;
    uint32_t claim_mask;
};

int64_t claim_slots(int32_t n_rows) {
    int64_t s = 2;
    while (s < 2 * (int64_t)n_rows) s *= 2;
    return s;
}

// The claim walk of taking-part row r, whose wave holds its key (`word`: this lane's) and hash:
// from the slot the hash picks, an empty slot is claimed with one atomicCAS (the row is its
// key's leader: -1); a taken slot's claimant comes back from the CAS, and its key is read from
// `keys`, which no kernel writes during the flush — equal in every word: this row is a follower
// (the claimant's buffer row); else the next slot.  route (NULL: one network): bit 0 of a game's
// word is its network, `bit` this row's; a claimant of the other network counts as an unequal
// key.  At most n_rows claims in 2 * n_rows slots or more end the walk; it is bounded by the
// table's size all the same (a scratch that was not zero), and a row whose walk runs out leads
// without a claim.  The result is the same in every lane.
__device__ __forceinline__ int64_t claim_walk(const Merge &m, const uint64_t *__restrict__ keys, int kw,
                                              uint64_t word, uint64_t h, int r, int n_rows, int rows_per_game,
                                              int game_rows, const int32_t *__restrict__ route, int bit, int lane) {
    uint32_t i = (uint32_t)(h >> 24) & m.claim_mask;   // not the bits that pick the table's set
    for (uint64_t step = 0; step <= m.claim_mask; ++step, i = (i + 1) & m.claim_mask) {
        int old = 0;
        if (lane == 0) old = atomicCAS(m.claim + i, 0, r + 1);
        old = __shfl(old, 0, 64);
        if (old == 0) return -1;   // claimed: this row leads
        const int cr = old - 1;
        if (cr < 0 || cr >= n_rows) continue;   // no row of this flush: the scratch was not zero
        if (route && (route[cr / rows_per_game] & 1) != bit) continue;   // the other network's row
        const int64_t crow = buffer_row(cr, rows_per_game, game_rows);
        const bool eq = lane < kw ? keys[crow * kw + lane] == word : true;
        if (__all(eq)) return crow;
    }
    return -1;
}

// ---- routing (ROUTED): two networks, a table and a dense list each (the arena pools) ---------
//
// Bit 0 of route[game] picks the network of a game's rows: its table (of one layout), its dense
// planes, its half of miss_rows [2][n_rows], its word of d_count [2] and its row of stats [2][5].
// The rows of one network go through the lookup, the claim walk and the insert as an unrouted
// flush's do; the two networks meet in the claim table alone, where a claimant of the other
// network is passed like an unequal key.

// What a flush holds once per network (K = 2: routed): the table, the probe's dense planes, the
// commit's dense values and logits.
template <int K>
struct PerNet {
    Table t[K];
    uint8_t *planes[K];
    const double *values[K];
    const uint8_t *logits[K];
};

template <class T, int K>
__device__ __forceinline__ T pick(const T (&a)[K], int net) {
    if constexpr (K == 2)
        return net ? a[1] : a[0];
    else
        return a[0];
}

// Network `net`'s table of two of one layout, member by member: a select per pointer, where a
// reference picked at run time would put both views into scratch memory.
template <int K>
__device__ __forceinline__ Table pick_table(const Table (&a)[K], int net) {
    Table t = a[0];
    if constexpr (K == 2) {
        t.epoch = net ? a[1].epoch : a[0].epoch;
        t.meta = net ? a[1].meta : a[0].meta;
        t.keys = net ? a[1].keys : a[0].keys;
        t.values = net ? a[1].values : a[0].values;
        t.logits = net ? a[1].logits : a[0].logits;
    }
    return t;
}

// The probe.  One wave per taking-part row r < n_rows (row (r / rows_per_game) * game_rows + r %
// rows_per_game of the buffers).  A hit (table_find) copies the entry's payload to the row's
// output slots; a miss takes the next dense slot of its network (one atomic on its word of
// d_count per workgroup, for all of its missing rows: thread k's, for network k), copies the
// row's planes there and records the row.
// CLAIMS: a claim step (claim_walk) between the lookup and the dense slot; a leader goes on as a
// miss does, a follower records its leader's buffer row.  has_table false: the tables hold the key
// and logit sizes alone and every row goes to the claim table.  Without CLAIMS there is a table
// and has_table, m and route are not read.
// ROUTED: the row's network is picked first; m.claim NULL: no merging (no claim walk, no leader
// word).
template <bool CLAIMS, bool ROUTED>
__global__ __launch_bounds__(BLOCK) void evalcache_probe_kernel(
    PerNet<ROUTED ? 2 : 1> nets, bool has_table, Merge m, const int32_t *__restrict__ route, int n_rows,
    int rows_per_game, int game_rows, const uint64_t *__restrict__ keys, const uint8_t *__restrict__ planes,
    int64_t plane_bytes, double *__restrict__ out_values, uint8_t *__restrict__ out_logits,
    int32_t *__restrict__ miss_rows, int32_t *d_count, int64_t *stats) {
    constexpr int K = ROUTED ? 2 : 1;
    __shared__ int s_miss[WAVES], s_merged[WAVES], s_net[WAVES];   // the last two: CLAIMS and ROUTED alone
    __shared__ int s_base[K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * WAVES + wave;
    const bool live = r < n_rows;
    int net = 0;
    if constexpr (ROUTED) net = live ? __builtin_amdgcn_readfirstlane(route[r / rows_per_game] & 1) : 0;
    const Table t = pick_table(nets.t, net);
    int64_t row = 0, entry = -1, lead = -1;
    if (live) {
        row = buffer_row(r, rows_per_game, game_rows);
        const int kw = t.kw;
        const uint64_t word = lane < kw ? keys[row * kw + lane] : 0;
        const uint64_t h = key_hash(word, lane, kw);
        if (!CLAIMS || has_table) entry = table_find(t, word, h, lane);
        if constexpr (CLAIMS) {
            if (!ROUTED || m.claim) {
                if (entry < 0)
                    lead = claim_walk(m, keys, kw, word, h, r, n_rows, rows_per_game, game_rows,
                                      ROUTED ? route : nullptr, net, lane);
                if (lane == 0) m.leader[r] = (int32_t)lead;
            }
        }
    }
    if (lane == 0) {
        s_miss[wave] = live && entry < 0 && lead < 0;
        if constexpr (CLAIMS) s_merged[wave] = live && lead >= 0;
        if constexpr (ROUTED) s_net[wave] = live ? net : -1;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        int np = ROUTED ? 0 : min(WAVES, n_rows - (int)blockIdx.x * WAVES), nm = 0, nf = 0;   // probed, missing, merged
        for (int w = 0; w < WAVES; ++w) {
            if constexpr (ROUTED) {
                if (s_net[w] != k) continue;
                np += 1;
            }
            nm += s_miss[w];
            if constexpr (CLAIMS) nf += s_merged[w];
        }
        s_base[k] = nm ? atomicAdd(d_count + k, nm) : 0;
        if (stats) {
            int64_t *st = stats + k * STATS;
            count_add(st + ZC_EVALCACHE_STAT_PROBED, np);
            count_add(st + ZC_EVALCACHE_STAT_HITS, np - nm - nf);
            if constexpr (CLAIMS) count_add(st + ZC_EVALCACHE_STAT_MERGED, nf);
        }
    }
    __syncthreads();
    if (!live || lead >= 0) return;   // a follower takes no dense slot and copies no planes
    if (entry >= 0) {
        if (lane == 0) out_values[row] = t.values[entry];
        if (t.logit_bytes)
            wave_copy(out_logits + row * t.logit_bytes, t.logits + entry * t.lstride, t.logit_bytes, lane);
    } else {
        int slot = s_base[net];
        for (int w = 0; w < wave; ++w)
            if (!ROUTED || s_net[w] == net) slot += s_miss[w];
        if (slot < 0 || slot >= n_rows) return;   // d_count was not 0 before the flush: no slot is this row's
        wave_copy(pick(nets.planes, net) + (int64_t)slot * plane_bytes, planes + row * plane_bytes, plane_bytes,
                  lane);
        if (lane == 0) miss_rows[(int64_t)net * n_rows + slot] = (int32_t)row;
    }
}

// The commit.  One wave per dense slot below min(*d_count, cap): the slot's payload goes to its
// row's output slots and, with TABLE, into the table (table_insert).  TABLE false: the scatter
// alone, for a merged flush without a table.
// ROUTED: one grid of cap (= n_rows) waves over both dense lists — wave w serves network 0's
// slot w below its count, else network 1's slot w - count[0] — and has_table says at run time
// whether there are tables (it is not read otherwise).
template <bool TABLE, bool ROUTED>
__global__ __launch_bounds__(BLOCK) void evalcache_commit_kernel(
    PerNet<ROUTED ? 2 : 1> nets, bool has_table, int cap, int64_t total_rows, const uint64_t *__restrict__ keys,
    const int32_t *__restrict__ miss_rows, const int32_t *__restrict__ d_count, double *__restrict__ out_values,
    uint8_t *__restrict__ out_logits, int64_t *stats) {
    constexpr int K = ROUTED ? 2 : 1;
    __shared__ int s_ins[WAVES], s_drop[WAVES], s_net[WAVES];   // the last: ROUTED alone
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w = blockIdx.x * WAVES + wave;
    if constexpr (!ROUTED) has_table = TABLE;
    int count = min(max(d_count[0], 0), cap), net = 0, slot = w;
    if constexpr (ROUTED) {
        net = w >= count;
        if (net) slot = w - count;
        count += min(max(d_count[1], 0), cap - count);
    }
    int ins = 0, drop = 0;
    const int64_t row = w < count ? miss_rows[(int64_t)net * cap + slot] : -1;
    if (row >= 0 && row < total_rows) {
        const Table t = pick_table(nets.t, net);
        const double v = pick(nets.values, net)[slot];
        const uint8_t *lg = pick(nets.logits, net) + (int64_t)slot * t.logit_bytes;
        if (lane == 0) out_values[row] = v;
        if (t.logit_bytes) wave_copy(out_logits + row * t.logit_bytes, lg, t.logit_bytes, lane);
        if (has_table) {
            const uint64_t word = lane < t.kw ? keys[row * t.kw + lane] : 0;
            if (table_insert(t, word, key_hash(word, lane, t.kw), v, lg, lane))
                ins = 1;
            else
                drop = 1;
        }
    }
    if (!stats || !has_table) return;
    if (lane == 0) {
        s_ins[wave] = ins;
        s_drop[wave] = drop;
        if constexpr (ROUTED) s_net[wave] = net;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        int ni = 0, nd = 0;
        for (int i = 0; i < WAVES; ++i) {
            if (ROUTED && s_net[i] != k) continue;
            ni += s_ins[i];
            nd += s_drop[i];
        }
        count_add(stats + k * STATS + ZC_EVALCACHE_STAT_INSERTS, ni);
        count_add(stats + k * STATS + ZC_EVALCACHE_STAT_DROPPED, nd);
    }
}

// A flush's last launch, after the commit: one thread leaves the next flush its counts at 0 and
// the next commit launch another epoch to claim under (epoch_a NULL: no table).
// CLAIMS: before that, one wave per taking-part row; a follower's value and logits come from its
// leader's output slots (a leader is no follower, and a follower's leader is a row of its own
// network, so no wave reads a slot that this launch writes), and every thread zeroes its share of
// the claim words (the grid has 64 threads a row, the table fewer than 4 words a row).  m.claim
// NULL (a flush of no rows, or a routed one without merging): one workgroup, n_rows 0.
template <bool CLAIMS, bool ROUTED>
__global__ __launch_bounds__(BLOCK) void evalcache_finish_kernel(
    Merge m, int n_rows, int rows_per_game, int game_rows, int64_t total_rows, int64_t logit_bytes,
    double *out_values, uint8_t *out_logits, uint32_t *epoch_a, uint32_t *epoch_b, int32_t *d_count) {
    if constexpr (CLAIMS) {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int r = blockIdx.x * WAVES + wave;
        if (r < n_rows) {
            const int64_t lead = m.leader[r];
            if (lead >= 0 && lead < total_rows) {
                const int64_t row = buffer_row(r, rows_per_game, game_rows);
                if (lane == 0) out_values[row] = out_values[lead];
                if (logit_bytes)
                    wave_copy(out_logits + row * logit_bytes, out_logits + lead * logit_bytes, logit_bytes, lane);
            }
        }
        if (m.claim) {
            const int64_t slots = (int64_t)m.claim_mask + 1;
            for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < slots; i += (int64_t)gridDim.x * BLOCK)
                m.claim[i] = 0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        d_count[0] = 0;
        if constexpr (ROUTED) d_count[1] = 0;
        if (!CLAIMS || epoch_a) {
            *epoch_a += 1;
            if constexpr (ROUTED) *epoch_b += 1;
        }
    }
}

// ---- the host side: one description of a flush, one check of it ------------------------------

enum Scratch { SCRATCH_NONE, SCRATCH_REQUIRED, SCRATCH_OPTIONAL };   // the plain, the merged and the routed calls

// A flush as its entry point got it.  A probe leaves the commit's pointers NULL and a commit the
// probe's; an unrouted call leaves every second of two NULL.
struct Flush {
    int nets;          // 1, or 2: the routed calls, which then need two different tables
    bool none_ok;      // "no table" (NULL with entries 0) is a form of the call
    Scratch claims;     // the scratch: none, required, or merging where there is one
    void *table[2];
    int64_t entries;
    int32_t key_bytes, logit_bytes, n_rows, rows_per_game, game_rows;
    const void *keys;
    int32_t *miss_rows, *count;
    double *out_values;
    void *out_logits;
    int64_t *stats;
    void *scratch;
    hipStream_t stream;
    // a probe's
    const int32_t *route;
    const void *planes;
    int64_t plane_bytes;
    void *dense_planes[2];
    // a commit's
    const double *dense_values[2];
    const void *dense_logits[2];
    // check()'s: the tables' views (has_table false: their sizes alone), the scratch's (m.claim
    // NULL: no merging in this flush) and the buffers' rows
    Table t[2];
    bool has_table;
    Merge m;
    int64_t total_rows;
};

Flush flush_of(int nets, bool none_ok, Scratch claims, void *table_a, void *table_b, int64_t entries, int32_t key_bytes,
               int32_t logit_bytes, int32_t n_rows, int32_t rows_per_game, int32_t game_rows, const void *keys,
               const int32_t *miss_rows, int32_t *count, double *out_values, void *out_logits, int64_t *stats,
               void *scratch, void *hip_stream) {
    Flush f{};
    f.nets = nets, f.none_ok = none_ok, f.claims = claims;
    f.table[0] = table_a, f.table[1] = table_b, f.entries = entries;
    f.key_bytes = key_bytes, f.logit_bytes = logit_bytes;
    f.n_rows = n_rows, f.rows_per_game = rows_per_game, f.game_rows = game_rows;
    f.keys = keys, f.miss_rows = (int32_t *)miss_rows, f.count = count;
    f.out_values = out_values, f.out_logits = out_logits, f.stats = stats, f.scratch = scratch;
    f.stream = (hipStream_t)hip_stream;
    return f;
}

// ZC_OK or ZC_EINVAL.  The pointers that only a flush of rows reads or writes are checked with
// n_rows > 0 alone.
int check(Flush &f, bool probe) {
    f.has_table = !f.none_ok || f.table[0] || f.table[1] || f.entries;
    for (int k = 0; k < f.nets; ++k)
        if (!make_table(f.table[k], f.entries, f.key_bytes, f.logit_bytes, &f.t[k], f.has_table)) return ZC_EINVAL;
    if (f.nets == 2 && f.table[0] == f.table[1] && f.has_table) return ZC_EINVAL;
    if (f.n_rows < 0 || f.rows_per_game < 1 || f.game_rows < f.rows_per_game || f.n_rows % f.rows_per_game)
        return ZC_EINVAL;
    f.total_rows = (int64_t)(f.n_rows / f.rows_per_game) * f.game_rows;
    if (f.total_rows >= ((int64_t)1 << 31)) return ZC_EINVAL;
    if (!f.count || ((uintptr_t)f.count & 3) || ((uintptr_t)f.stats & 7)) return ZC_EINVAL;
    if (probe && (f.plane_bytes < 2 || (f.plane_bytes & 1))) return ZC_EINVAL;
    if (f.claims == SCRATCH_OPTIONAL && ((uintptr_t)f.scratch & 3)) return ZC_EINVAL;
    if (!f.n_rows) return ZC_OK;
    const bool two = f.nets == 2, lg = f.logit_bytes != 0;
    const struct {
        const void *p;
        unsigned mask;
        bool required;
    } ptrs[] = {{f.keys, 7, true},
                {f.miss_rows, 3, true},
                {f.out_values, 7, true},
                {f.out_logits, 1, lg},
                {f.route, 3, probe && two},
                {f.planes, 1, probe},
                {f.dense_planes[0], 1, probe},
                {f.dense_planes[1], 1, probe && two},
                {f.dense_values[0], 7, !probe},
                {f.dense_values[1], 7, !probe && two},
                {f.dense_logits[0], 1, !probe && lg},
                {f.dense_logits[1], 1, !probe && lg && two}};
    for (const auto &x : ptrs)
        if ((x.required && !x.p) || ((uintptr_t)x.p & x.mask)) return ZC_EINVAL;
    if (probe && two && f.dense_planes[0] == f.dense_planes[1]) return ZC_EINVAL;
    if (f.claims == SCRATCH_REQUIRED || (f.claims == SCRATCH_OPTIONAL && f.scratch)) {
        if (!f.scratch || ((uintptr_t)f.scratch & 3)) return ZC_EINVAL;
        const int64_t slots = claim_slots(f.n_rows);
        f.m.claim = (int32_t *)f.scratch;
        f.m.leader = f.m.claim + slots;
        f.m.claim_mask = (uint32_t)(slots - 1);
    }
    return ZC_OK;
}

template <int K>
PerNet<K> per_net(const Flush &f) {
    PerNet<K> n;
    for (int k = 0; k < K; ++k) {
        n.t[k] = f.t[k];
        n.planes[k] = (uint8_t *)f.dense_planes[k];
        n.values[k] = f.dense_values[k];
        n.logits[k] = (const uint8_t *)f.dense_logits[k];
    }
    return n;
}

dim3 row_grid(int rows) { return dim3(rows ? (rows + WAVES - 1) / WAVES : 1); }

int done() { return hipGetLastError() == hipSuccess ? ZC_OK : ZC_EHIP; }

// A probe of no rows launches nothing.
template <bool CLAIMS, bool ROUTED>
int probe(Flush f) {
    if (check(f, true) != ZC_OK) return ZC_EINVAL;
    if (!f.n_rows) return ZC_OK;
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    hipLaunchKernelGGL((evalcache_probe_kernel<CLAIMS, ROUTED>), row_grid(f.n_rows), dim3(BLOCK), 0, f.stream,
                       per_net<ROUTED ? 2 : 1>(f), f.has_table, f.m, f.route, (int)f.n_rows, (int)f.rows_per_game,
                       (int)f.game_rows, (const uint64_t *)f.keys, (const uint8_t *)f.planes, f.plane_bytes,
                       f.out_values, (uint8_t *)f.out_logits, f.miss_rows, f.count, f.stats);
    return done();
}

// A commit of no rows still runs its finish launch.
template <bool CLAIMS, bool ROUTED>
int commit(Flush f) {
    if (check(f, false) != ZC_OK) return ZC_EINVAL;
    const auto nets = per_net<ROUTED ? 2 : 1>(f);
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    if (f.n_rows) {
        auto kernel = evalcache_commit_kernel<true, ROUTED>;
        if constexpr (!ROUTED)
            if (!f.has_table) kernel = evalcache_commit_kernel<false, false>;
        hipLaunchKernelGGL(kernel, row_grid(f.n_rows), dim3(BLOCK), 0, f.stream, nets, f.has_table, (int)f.n_rows,
                           f.total_rows, (const uint64_t *)f.keys, (const int32_t *)f.miss_rows,
                           (const int32_t *)f.count, f.out_values, (uint8_t *)f.out_logits, f.stats);
    }
    const int rows = f.m.claim ? f.n_rows : 0;   // the followers' rows
    hipLaunchKernelGGL((evalcache_finish_kernel<CLAIMS, ROUTED>), row_grid(rows), dim3(CLAIMS ? BLOCK : 1), 0, f.stream,
                       f.m, rows, (int)f.rows_per_game, (int)f.game_rows, f.total_rows, (int64_t)f.logit_bytes,
                       f.out_values, (uint8_t *)f.out_logits, f.has_table ? f.t[0].epoch : (uint32_t *)nullptr,
                       f.has_table ? f.t[ROUTED].epoch : (uint32_t *)nullptr, f.count);
    return done();
}

}  // namespace

extern "C" {

int zc_evalcache_bytes(int64_t entries, int32_t key_bytes, int32_t logit_bytes, int64_t *bytes, int64_t *sets) {
    return layout(entries, key_bytes, logit_bytes, sets, bytes) ? ZC_OK : ZC_EINVAL;
}

int zc_evalcache_clear_async(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes,
                             void *hip_stream) {
    Table t;
    if (!make_table(d_table, entries, key_bytes, logit_bytes, &t)) return ZC_EINVAL;
    const size_t n = HEADER_BYTES + ((size_t)t.set_mask + 1) * WAYS * sizeof(uint32_t);
    return hipMemsetAsync(d_table, 0, n, (hipStream_t)hip_stream) == hipSuccess ? ZC_OK : ZC_EHIP;
}

int zc_evalcache_merge_scratch_bytes(int32_t n_rows, int64_t *bytes) {
    if (n_rows < 0 || !bytes) return ZC_EINVAL;
    *bytes = (claim_slots(n_rows) + n_rows) * (int64_t)sizeof(int32_t);
    return ZC_OK;
}

int zc_evalcache_probe_async(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes, int32_t n_rows,
                             int32_t rows_per_game, int32_t game_rows, const void *d_keys, const void *d_planes,
                             int64_t plane_bytes, double *d_out_values, void *d_out_logits, void *d_dense_planes,
                             int32_t *d_miss_rows, int32_t *d_count, int64_t *d_stats, void *hip_stream) {
    Flush f = flush_of(1, false, SCRATCH_NONE, d_table, nullptr, entries, key_bytes, logit_bytes, n_rows, rows_per_game,
                       game_rows, d_keys, d_miss_rows, d_count, d_out_values, d_out_logits, d_stats, nullptr, hip_stream);
    f.planes = d_planes, f.plane_bytes = plane_bytes, f.dense_planes[0] = d_dense_planes;
    return probe<false, false>(f);
}

int zc_evalcache_commit_async(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes, int32_t n_rows,
                              int32_t rows_per_game, int32_t game_rows, const void *d_keys, const int32_t *d_miss_rows,
                              int32_t *d_count, const double *d_dense_values, const void *d_dense_logits,
                              double *d_out_values, void *d_out_logits, int64_t *d_stats, void *hip_stream) {
    Flush f = flush_of(1, false, SCRATCH_NONE, d_table, nullptr, entries, key_bytes, logit_bytes, n_rows, rows_per_game,
                       game_rows, d_keys, d_miss_rows, d_count, d_out_values, d_out_logits, d_stats, nullptr, hip_stream);
    f.dense_values[0] = d_dense_values, f.dense_logits[0] = d_dense_logits;
    return commit<false, false>(f);
}

int zc_evalcache_probe_merged_async(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes,
                                    int32_t n_rows, int32_t rows_per_game, int32_t game_rows, const void *d_keys,
                                    const void *d_planes, int64_t plane_bytes, double *d_out_values,
                                    void *d_out_logits, void *d_dense_planes, int32_t *d_miss_rows, int32_t *d_count,
                                    int64_t *d_stats, void *d_scratch, void *hip_stream) {
    Flush f = flush_of(1, true, SCRATCH_REQUIRED, d_table, nullptr, entries, key_bytes, logit_bytes, n_rows, rows_per_game,
                       game_rows, d_keys, d_miss_rows, d_count, d_out_values, d_out_logits, d_stats, d_scratch, hip_stream);
    f.planes = d_planes, f.plane_bytes = plane_bytes, f.dense_planes[0] = d_dense_planes;
    return probe<true, false>(f);
}

int zc_evalcache_commit_merged_async(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes,
                                     int32_t n_rows, int32_t rows_per_game, int32_t game_rows, const void *d_keys,
                                     const int32_t *d_miss_rows, int32_t *d_count, const double *d_dense_values,
                                     const void *d_dense_logits, double *d_out_values, void *d_out_logits,
                                     int64_t *d_stats, void *d_scratch, void *hip_stream) {
    Flush f = flush_of(1, true, SCRATCH_REQUIRED, d_table, nullptr, entries, key_bytes, logit_bytes, n_rows, rows_per_game,
                       game_rows, d_keys, d_miss_rows, d_count, d_out_values, d_out_logits, d_stats, d_scratch, hip_stream);
    f.dense_values[0] = d_dense_values, f.dense_logits[0] = d_dense_logits;
    return commit<true, false>(f);
}

int zc_evalcache_probe_routed_async(void *d_table_a, void *d_table_b, int64_t entries, int32_t key_bytes,
                                    int32_t logit_bytes, int32_t n_rows, int32_t rows_per_game, int32_t game_rows,
                                    const int32_t *d_route, const void *d_keys, const void *d_planes,
                                    int64_t plane_bytes, double *d_out_values, void *d_out_logits,
                                    void *d_dense_planes_a, void *d_dense_planes_b, int32_t *d_miss_rows,
                                    int32_t *d_count, int64_t *d_stats, void *d_scratch, void *hip_stream) {
    Flush f = flush_of(2, true, SCRATCH_OPTIONAL, d_table_a, d_table_b, entries, key_bytes, logit_bytes, n_rows,
                       rows_per_game, game_rows, d_keys, d_miss_rows, d_count, d_out_values, d_out_logits, d_stats,
                       d_scratch, hip_stream);
    f.route = d_route, f.planes = d_planes, f.plane_bytes = plane_bytes;
    f.dense_planes[0] = d_dense_planes_a, f.dense_planes[1] = d_dense_planes_b;
    return probe<true, true>(f);
}

int zc_evalcache_commit_routed_async(void *d_table_a, void *d_table_b, int64_t entries, int32_t key_bytes,
                                     int32_t logit_bytes, int32_t n_rows, int32_t rows_per_game, int32_t game_rows,
                                     const void *d_keys, const int32_t *d_miss_rows, int32_t *d_count,
                                     const double *d_dense_values_a, const void *d_dense_logits_a,
                                     const double *d_dense_values_b, const void *d_dense_logits_b,
                                     double *d_out_values, void *d_out_logits, int64_t *d_stats, void *d_scratch,
                                     void *hip_stream) {
    Flush f = flush_of(2, true, SCRATCH_OPTIONAL, d_table_a, d_table_b, entries, key_bytes, logit_bytes, n_rows,
                       rows_per_game, game_rows, d_keys, d_miss_rows, d_count, d_out_values, d_out_logits, d_stats,
                       d_scratch, hip_stream);
    f.dense_values[0] = d_dense_values_a, f.dense_logits[0] = d_dense_logits_a;
    f.dense_values[1] = d_dense_values_b, f.dense_logits[1] = d_dense_logits_b;
    return commit<true, true>(f);
}

}  // extern "C"
