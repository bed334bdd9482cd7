// evalcache.hip — a device-resident cache of network evaluations (include/zeroclone.h,
// "evaluation cache"): a set-associative table keyed by the compact leaf row, and the two
// kernels that carry a flush through it (probe -> counted network on the misses -> commit).
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
// The merged entry points (further down) carry a flush through the same three launches and
// evaluate a key that several of its rows hold once, with or without a table.  The routed entry
// points (after them) carry an arena's flush, rows of two networks, through one probe and one
// commit over a table, a dense list and a set of counters per network.  The lookup, the insert,
// the claim walk and the followers' copy are device functions that all three families share.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zeroclone.h"

namespace {

constexpr int WAYS = ZC_EVALCACHE_WAYS;
static_assert(WAYS == 8, "a set's ways are looked up by lanes 0..7 and picked by three hash bits");
constexpr int HEADER_BYTES = 64;
constexpr int BLOCK = 512, WAVES = BLOCK / 64;   // one wave per row
constexpr int MAX_KEY_WORDS = 64;                // a lane per key word

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

bool make_table(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes, Table *t) {
    int64_t sets;
    if (!d_table || ((uintptr_t)d_table & 15) || !layout(entries, key_bytes, logit_bytes, &sets, nullptr)) return false;
    const int64_t E = sets * WAYS;
    uint8_t *p = (uint8_t *)d_table;
    t->epoch = (uint32_t *)p;
    t->meta = (uint32_t *)(p + HEADER_BYTES);
    t->keys = (uint64_t *)(p + HEADER_BYTES + E * 4);
    t->values = (double *)((uint8_t *)t->keys + E * key_bytes);
    t->logits = (uint8_t *)(t->values + E);
    t->set_mask = (uint32_t)(sets - 1);
    t->kw = key_bytes / 8;
    t->logit_bytes = logit_bytes;
    t->lstride = ((int64_t)logit_bytes + 15) & ~(int64_t)15;
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
// bits pick, unless a way already carries the key's tag.  The way is claimed with one atomicCAS
// on its meta word; a wave that loses the claim of an empty way looks at the set again, one
// that loses a victim (or finds it claimed in this launch) drops its insert.  true: inserted.
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

// One wave per taking-part row r < n_rows (row (r / rows_per_game) * game_rows + r %
// rows_per_game of the buffers).  Lanes 0..7 read the set's meta words and the tag filters the
// ways; for a way that passes, lane i compares key word i.  A hit copies the entry's payload to
// the row's output slots; a miss takes the next dense slot (one atomic on *d_count per
// workgroup, for all of its missing rows), copies the row's planes there and records the row.
__global__ __launch_bounds__(BLOCK) void evalcache_probe_kernel(
    Table t, int n_rows, int rows_per_game, int game_rows, const uint64_t *__restrict__ keys,
    const uint8_t *__restrict__ planes, int64_t plane_bytes, double *__restrict__ out_values,
    uint8_t *__restrict__ out_logits, uint8_t *__restrict__ dense_planes, int32_t *__restrict__ miss_rows,
    int32_t *d_count, int64_t *stats) {
    __shared__ int s_miss[WAVES];
    __shared__ int s_base;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * WAVES + wave;
    const bool live = r < n_rows;
    int64_t row = 0, entry = -1;
    if (live) {
        row = buffer_row(r, rows_per_game, game_rows);
        const uint64_t word = lane < t.kw ? keys[row * t.kw + lane] : 0;
        entry = table_find(t, word, key_hash(word, lane, t.kw), lane);
    }
    if (lane == 0) s_miss[wave] = live && entry < 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        int nm = 0;
        for (int w = 0; w < WAVES; ++w) nm += s_miss[w];
        const int nlive = min(WAVES, n_rows - (int)blockIdx.x * WAVES);
        s_base = nm ? atomicAdd(d_count, nm) : 0;
        if (stats) {
            count_add(stats + ZC_EVALCACHE_STAT_PROBED, nlive);
            count_add(stats + ZC_EVALCACHE_STAT_HITS, nlive - nm);
        }
    }
    __syncthreads();
    if (!live) return;
    if (entry >= 0) {
        if (lane == 0) out_values[row] = t.values[entry];
        if (t.logit_bytes)
            wave_copy(out_logits + row * t.logit_bytes, t.logits + entry * t.lstride, t.logit_bytes, lane);
    } else {
        int slot = s_base;
        for (int w = 0; w < wave; ++w) slot += s_miss[w];
        if (slot < 0 || slot >= n_rows) return;   // *d_count was not 0 before the flush: no slot is this row's
        wave_copy(dense_planes + (int64_t)slot * plane_bytes, planes + row * plane_bytes, plane_bytes, lane);
        if (lane == 0) miss_rows[slot] = (int32_t)row;
    }
}

// One wave per dense slot below min(*d_count, cap): the slot's payload goes to its row's output
// slots and into the table — the set's first empty way, else the way three hash bits pick —
// unless a way already carries the key's tag (the same key being inserted by another wave of
// this launch, or a tag collision: the insert is dropped either way).  The way is claimed with
// one atomicCAS on its meta word; a wave that loses the claim of an empty way looks at the set
// again, one that loses a victim (or finds it claimed in this launch) drops its insert.
__global__ __launch_bounds__(BLOCK) void evalcache_commit_kernel(
    Table t, int cap, int64_t total_rows, const uint64_t *__restrict__ keys, const int32_t *__restrict__ miss_rows,
    const int32_t *__restrict__ d_count, const double *__restrict__ dense_values,
    const uint8_t *__restrict__ dense_logits, double *__restrict__ out_values, uint8_t *__restrict__ out_logits,
    int64_t *stats) {
    __shared__ int s_ins[WAVES], s_drop[WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = blockIdx.x * WAVES + wave;
    const int count = min(max(*d_count, 0), cap);
    int ins = 0, drop = 0;
    const int64_t row = slot < count ? miss_rows[slot] : -1;
    if (row >= 0 && row < total_rows) {
        const double v = dense_values[slot];
        const uint8_t *lg = dense_logits + (int64_t)slot * t.logit_bytes;
        if (lane == 0) out_values[row] = v;
        if (t.logit_bytes) wave_copy(out_logits + row * t.logit_bytes, lg, t.logit_bytes, lane);
        const uint64_t word = lane < t.kw ? keys[row * t.kw + lane] : 0;
        if (table_insert(t, word, key_hash(word, lane, t.kw), v, lg, lane))
            ins = 1;
        else
            drop = 1;
    }
    if (!stats) return;
    if (lane == 0) {
        s_ins[wave] = ins;
        s_drop[wave] = drop;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int ni = 0, nd = 0;
        for (int w = 0; w < WAVES; ++w) {
            ni += s_ins[w];
            nd += s_drop[w];
        }
        count_add(stats + ZC_EVALCACHE_STAT_INSERTS, ni);
        count_add(stats + ZC_EVALCACHE_STAT_DROPPED, nd);
    }
}

// After a commit launch: the next flush counts its misses from 0, and the next commit launch
// claims under another epoch.
__global__ void evalcache_finish_kernel(uint32_t *epoch, int32_t *d_count) {
    *d_count = 0;
    *epoch += 1;
}

// ---- merging: a key pending several times in one flush is evaluated once -------------------
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

// The probe kernel with a claim step (claim_walk) between the lookup and the dense slot.
// has_table false: t holds the key and logit sizes alone and every row goes to the claim table.
// A leader goes on as a miss does in the plain probe; a follower records its leader's buffer
// row.
__global__ __launch_bounds__(BLOCK) void evalcache_probe_merged_kernel(
    Table t, bool has_table, Merge m, int n_rows, int rows_per_game, int game_rows, const uint64_t *__restrict__ keys,
    const uint8_t *__restrict__ planes, int64_t plane_bytes, double *__restrict__ out_values,
    uint8_t *__restrict__ out_logits, uint8_t *__restrict__ dense_planes, int32_t *__restrict__ miss_rows,
    int32_t *d_count, int64_t *stats) {
    __shared__ int s_miss[WAVES], s_merged[WAVES];
    __shared__ int s_base;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * WAVES + wave;
    const bool live = r < n_rows;
    int64_t row = 0, entry = -1, lead = -1;
    if (live) {
        row = buffer_row(r, rows_per_game, game_rows);
        const uint64_t word = lane < t.kw ? keys[row * t.kw + lane] : 0;
        const uint64_t h = key_hash(word, lane, t.kw);
        if (has_table) entry = table_find(t, word, h, lane);
        if (entry < 0) lead = claim_walk(m, keys, t.kw, word, h, r, n_rows, rows_per_game, game_rows, nullptr, 0, lane);
        if (lane == 0) m.leader[r] = (int32_t)lead;
    }
    if (lane == 0) {
        s_miss[wave] = live && entry < 0 && lead < 0;
        s_merged[wave] = live && lead >= 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int nm = 0, nf = 0;
        for (int w = 0; w < WAVES; ++w) {
            nm += s_miss[w];
            nf += s_merged[w];
        }
        const int nlive = min(WAVES, n_rows - (int)blockIdx.x * WAVES);
        s_base = nm ? atomicAdd(d_count, nm) : 0;
        if (stats) {
            count_add(stats + ZC_EVALCACHE_STAT_PROBED, nlive);
            count_add(stats + ZC_EVALCACHE_STAT_HITS, nlive - nm - nf);
            count_add(stats + ZC_EVALCACHE_STAT_MERGED, nf);
        }
    }
    __syncthreads();
    if (!live || lead >= 0) return;   // a follower takes no dense slot and copies no planes
    if (entry >= 0) {
        if (lane == 0) out_values[row] = t.values[entry];
        if (t.logit_bytes)
            wave_copy(out_logits + row * t.logit_bytes, t.logits + entry * t.lstride, t.logit_bytes, lane);
    } else {
        int slot = s_base;
        for (int w = 0; w < wave; ++w) slot += s_miss[w];
        if (slot < 0 || slot >= n_rows) return;   // *d_count was not 0 before the flush: no slot is this row's
        wave_copy(dense_planes + (int64_t)slot * plane_bytes, planes + row * plane_bytes, plane_bytes, lane);
        if (lane == 0) miss_rows[slot] = (int32_t)row;
    }
}

// Without a table the commit kernel's scatter alone: one wave per dense slot below
// min(*d_count, cap), the slot's payload to its row's output slots.
__global__ __launch_bounds__(BLOCK) void evalcache_scatter_kernel(
    int cap, int64_t total_rows, int64_t logit_bytes, const int32_t *__restrict__ miss_rows,
    const int32_t *__restrict__ d_count, const double *__restrict__ dense_values,
    const uint8_t *__restrict__ dense_logits, double *__restrict__ out_values, uint8_t *__restrict__ out_logits) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = blockIdx.x * WAVES + wave;
    const int count = min(max(*d_count, 0), cap);
    const int64_t row = slot < count ? miss_rows[slot] : -1;
    if (row < 0 || row >= total_rows) return;
    if (lane == 0) out_values[row] = dense_values[slot];
    if (logit_bytes)
        wave_copy(out_logits + row * logit_bytes, dense_logits + (int64_t)slot * logit_bytes, logit_bytes, lane);
}

// The merged flush's last launch, after the commit's scatter: one wave per taking-part row; a
// follower's value and logits come from its leader's output slots (a leader is no follower, so
// no wave reads a slot that this launch writes).  Every thread zeroes its share of the claim
// words (the grid has 64 threads a row, the table fewer than 4 words a row), and one thread
// does evalcache_finish_kernel's work (epoch NULL: no table).
__device__ __forceinline__ void finish_followers(const Merge &m, int n_rows, int rows_per_game, int game_rows,
                                                 int64_t total_rows, int64_t logit_bytes, double *out_values,
                                                 uint8_t *out_logits) {
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
    if (m.claim) {   // NULL: a flush of no rows
        const int64_t slots = (int64_t)m.claim_mask + 1;
        for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < slots; i += (int64_t)gridDim.x * BLOCK)
            m.claim[i] = 0;
    }
}

__global__ __launch_bounds__(BLOCK) void evalcache_finish_merged_kernel(
    Merge m, int n_rows, int rows_per_game, int game_rows, int64_t total_rows, int64_t logit_bytes,
    double *out_values, uint8_t *out_logits, uint32_t *epoch, int32_t *d_count) {
    finish_followers(m, n_rows, rows_per_game, game_rows, total_rows, logit_bytes, out_values, out_logits);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *d_count = 0;
        if (epoch) *epoch += 1;
    }
}

// ---- routed flush: two networks, a table and a dense list each (the arena pools) ------------
//
// Bit 0 of route[game] picks the network of a game's rows: its table (ta / tb, of one layout),
// its dense planes, its half of miss_rows [2][n_rows], its word of d_count [2] and its row of
// stats [2][5].  The rows of one network go through the lookup, the claim walk and the insert
// of the kernels above; the two networks meet in the claim table alone, where a claimant of the
// other network is passed like an unequal key.

// Network `net`'s table of two of one layout, member by member: a select per pointer, where a
// reference picked at run time would put both views into scratch memory.
__device__ __forceinline__ Table pick_table(const Table &a, const Table &b, int net) {
    Table t = a;
    t.epoch = net ? b.epoch : a.epoch;
    t.meta = net ? b.meta : a.meta;
    t.keys = net ? b.keys : a.keys;
    t.values = net ? b.values : a.values;
    t.logits = net ? b.logits : a.logits;
    return t;
}

// The routed probe: evalcache_probe_merged_kernel with the row's network picked first.
// m.claim NULL: no merging (no claim walk, no leader word).  Threads 0 and 1 of a workgroup
// take the dense slots of network 0's and network 1's missing rows: one atomic each.
__global__ __launch_bounds__(BLOCK) void evalcache_probe_routed_kernel(
    Table ta, Table tb, bool has_table, Merge m, const int32_t *__restrict__ route, int n_rows, int rows_per_game,
    int game_rows, const uint64_t *__restrict__ keys, const uint8_t *__restrict__ planes, int64_t plane_bytes,
    double *__restrict__ out_values, uint8_t *__restrict__ out_logits, uint8_t *__restrict__ dense_a,
    uint8_t *__restrict__ dense_b, int32_t *__restrict__ miss_rows, int32_t *d_count, int64_t *stats) {
    __shared__ int s_miss[WAVES], s_merged[WAVES], s_net[WAVES];
    __shared__ int s_base[2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * WAVES + wave;
    const bool live = r < n_rows;
    const int net = live ? __builtin_amdgcn_readfirstlane(route[r / rows_per_game] & 1) : 0;
    const Table t = pick_table(ta, tb, net);
    int64_t row = 0, entry = -1, lead = -1;
    if (live) {
        row = buffer_row(r, rows_per_game, game_rows);
        const int kw = t.kw;
        const uint64_t word = lane < kw ? keys[row * kw + lane] : 0;
        const uint64_t h = key_hash(word, lane, kw);
        if (has_table) entry = table_find(t, word, h, lane);
        if (m.claim) {
            if (entry < 0)
                lead = claim_walk(m, keys, kw, word, h, r, n_rows, rows_per_game, game_rows, route, net, lane);
            if (lane == 0) m.leader[r] = (int32_t)lead;
        }
    }
    if (lane == 0) {
        s_miss[wave] = live && entry < 0 && lead < 0;
        s_merged[wave] = live && lead >= 0;
        s_net[wave] = net;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        const int nlive = min(WAVES, n_rows - (int)blockIdx.x * WAVES);
        int np = 0, nm = 0, nf = 0;
        for (int w = 0; w < nlive; ++w)
            if (s_net[w] == k) {
                np += 1;
                nm += s_miss[w];
                nf += s_merged[w];
            }
        s_base[k] = nm ? atomicAdd(d_count + k, nm) : 0;
        if (stats) {
            int64_t *st = stats + k * (ZC_EVALCACHE_STAT_MERGED + 1);
            count_add(st + ZC_EVALCACHE_STAT_PROBED, np);
            count_add(st + ZC_EVALCACHE_STAT_HITS, np - nm - nf);
            count_add(st + ZC_EVALCACHE_STAT_MERGED, nf);
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
        for (int w = 0; w < wave; ++w) slot += s_miss[w] && s_net[w] == net;
        if (slot < 0 || slot >= n_rows) return;   // d_count was not 0 before the flush: no slot is this row's
        wave_copy((net ? dense_b : dense_a) + (int64_t)slot * plane_bytes, planes + row * plane_bytes, plane_bytes,
                  lane);
        if (lane == 0) miss_rows[(int64_t)net * n_rows + slot] = (int32_t)row;
    }
}

// The routed commit: one grid of cap (= n_rows) waves over both dense lists — wave w serves
// network 0's slot w below its count, else network 1's slot w - count[0] — each as
// evalcache_commit_kernel serves a slot: the payload to the row's output slots and, with
// tables, into its network's.
__global__ __launch_bounds__(BLOCK) void evalcache_commit_routed_kernel(
    Table ta, Table tb, bool has_table, int cap, int64_t total_rows, const uint64_t *__restrict__ keys,
    const int32_t *__restrict__ miss_rows, const int32_t *__restrict__ d_count,
    const double *__restrict__ dense_values_a, const uint8_t *__restrict__ dense_logits_a,
    const double *__restrict__ dense_values_b, const uint8_t *__restrict__ dense_logits_b,
    double *__restrict__ out_values, uint8_t *__restrict__ out_logits, int64_t *stats) {
    __shared__ int s_ins[WAVES], s_drop[WAVES], s_net[WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w = blockIdx.x * WAVES + wave;
    const int ca = min(max(d_count[0], 0), cap), cb = min(max(d_count[1], 0), cap - ca);
    const int net = w >= ca, slot = net ? w - ca : w;
    int ins = 0, drop = 0;
    const int64_t row = w < ca + cb ? miss_rows[(int64_t)net * cap + slot] : -1;
    if (row >= 0 && row < total_rows) {
        const Table t = pick_table(ta, tb, net);
        const double v = (net ? dense_values_b : dense_values_a)[slot];
        const uint8_t *lg = (net ? dense_logits_b : dense_logits_a) + (int64_t)slot * t.logit_bytes;
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
        s_net[wave] = net;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        int ni = 0, nd = 0;
        for (int i = 0; i < WAVES; ++i)
            if (s_net[i] == k) {
                ni += s_ins[i];
                nd += s_drop[i];
            }
        int64_t *st = stats + k * (ZC_EVALCACHE_STAT_MERGED + 1);
        count_add(st + ZC_EVALCACHE_STAT_INSERTS, ni);
        count_add(st + ZC_EVALCACHE_STAT_DROPPED, nd);
    }
}

// The routed flush's last launch: with merging evalcache_finish_merged_kernel's work over the
// taking-part rows (a follower's leader is a row of its own network), without it one workgroup
// of no rows (m all zero, n_rows 0); both counts to 0, both tables to their next epoch
// (epoch_a NULL: no tables).
__global__ __launch_bounds__(BLOCK) void evalcache_finish_routed_kernel(
    Merge m, int n_rows, int rows_per_game, int game_rows, int64_t total_rows, int64_t logit_bytes,
    double *out_values, uint8_t *out_logits, uint32_t *epoch_a, uint32_t *epoch_b, int32_t *d_count) {
    finish_followers(m, n_rows, rows_per_game, game_rows, total_rows, logit_bytes, out_values, out_logits);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        d_count[0] = 0;
        d_count[1] = 0;
        if (epoch_a) {
            *epoch_a += 1;
            *epoch_b += 1;
        }
    }
}

// The merged calls' table: d_table NULL with entries 0 is "no table" (*has_table false, t's
// sizes alone set).
bool make_table_or_none(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes, Table *t,
                        bool *has_table) {
    *has_table = d_table || entries;
    if (*has_table) return make_table(d_table, entries, key_bytes, logit_bytes, t);
    if (!layout(WAYS, key_bytes, logit_bytes, nullptr, nullptr)) return false;
    *t = Table{};
    t->kw = key_bytes / 8;
    t->logit_bytes = logit_bytes;
    t->lstride = ((int64_t)logit_bytes + 15) & ~(int64_t)15;
    return true;
}

bool make_merge(void *d_scratch, int32_t n_rows, Merge *m) {
    if (!d_scratch || ((uintptr_t)d_scratch & 3)) return false;
    const int64_t slots = claim_slots(n_rows);
    m->claim = (int32_t *)d_scratch;
    m->leader = m->claim + slots;
    m->claim_mask = (uint32_t)(slots - 1);
    return true;
}

// The routed calls' tables: both NULL with entries 0 is "no tables", else two different tables
// of one layout.
bool make_routed_tables(void *d_table_a, void *d_table_b, int64_t entries, int32_t key_bytes, int32_t logit_bytes,
                        Table *ta, Table *tb, bool *has_table) {
    if (!d_table_a != !d_table_b || (d_table_a && d_table_a == d_table_b)) return false;
    return make_table_or_none(d_table_a, entries, key_bytes, logit_bytes, ta, has_table) &&
           make_table_or_none(d_table_b, entries, key_bytes, logit_bytes, tb, has_table);
}

int done() { return hipGetLastError() == hipSuccess ? ZC_OK : ZC_EHIP; }

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

int zc_evalcache_probe_async(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes, int32_t n_rows,
                             int32_t rows_per_game, int32_t game_rows, const void *d_keys, const void *d_planes,
                             int64_t plane_bytes, double *d_out_values, void *d_out_logits, void *d_dense_planes,
                             int32_t *d_miss_rows, int32_t *d_count, int64_t *d_stats, void *hip_stream) {
    Table t;
    if (!make_table(d_table, entries, key_bytes, logit_bytes, &t)) return ZC_EINVAL;
    if (n_rows < 0 || rows_per_game < 1 || game_rows < rows_per_game || n_rows % rows_per_game) return ZC_EINVAL;
    if ((int64_t)(n_rows / rows_per_game) * game_rows >= ((int64_t)1 << 31)) return ZC_EINVAL;
    if (plane_bytes < 2 || (plane_bytes & 1) || !d_count || ((uintptr_t)d_count & 3) || ((uintptr_t)d_stats & 7))
        return ZC_EINVAL;
    if (!n_rows) return ZC_OK;
    if (!d_keys || !d_planes || !d_out_values || !d_dense_planes || !d_miss_rows || (logit_bytes && !d_out_logits))
        return ZC_EINVAL;
    if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_out_values & 7) || ((uintptr_t)d_miss_rows & 3) ||
        (((uintptr_t)d_planes | (uintptr_t)d_dense_planes | (uintptr_t)d_out_logits) & 1))
        return ZC_EINVAL;
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    hipLaunchKernelGGL(evalcache_probe_kernel, dim3((n_rows + WAVES - 1) / WAVES), dim3(BLOCK), 0,
                       (hipStream_t)hip_stream, t, (int)n_rows, (int)rows_per_game, (int)game_rows,
                       (const uint64_t *)d_keys, (const uint8_t *)d_planes, plane_bytes, d_out_values,
                       (uint8_t *)d_out_logits, (uint8_t *)d_dense_planes, d_miss_rows, d_count, d_stats);
    return done();
}

int zc_evalcache_commit_async(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes, int32_t n_rows,
                              int32_t rows_per_game, int32_t game_rows, const void *d_keys, const int32_t *d_miss_rows, int32_t *d_count,
                              const double *d_dense_values, const void *d_dense_logits, double *d_out_values,
                              void *d_out_logits, int64_t *d_stats, void *hip_stream) {
    Table t;
    if (!make_table(d_table, entries, key_bytes, logit_bytes, &t)) return ZC_EINVAL;
    if (n_rows < 0 || !d_count || ((uintptr_t)d_count & 3) || ((uintptr_t)d_stats & 7)) return ZC_EINVAL;
    if (rows_per_game < 1 || game_rows < rows_per_game || n_rows % rows_per_game) return ZC_EINVAL;
    const int64_t total_rows = (int64_t)(n_rows / rows_per_game) * game_rows;
    if (total_rows >= ((int64_t)1 << 31)) return ZC_EINVAL;
    if (n_rows) {
        if (!d_keys || !d_miss_rows || !d_dense_values || !d_out_values ||
            (logit_bytes && (!d_dense_logits || !d_out_logits)))
            return ZC_EINVAL;
        if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_out_values & 7) || ((uintptr_t)d_dense_values & 7) ||
            ((uintptr_t)d_miss_rows & 3) || (((uintptr_t)d_dense_logits | (uintptr_t)d_out_logits) & 1))
            return ZC_EINVAL;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    if (n_rows)
        hipLaunchKernelGGL(evalcache_commit_kernel, dim3((n_rows + WAVES - 1) / WAVES), dim3(BLOCK), 0, s, t,
                           (int)n_rows, total_rows, (const uint64_t *)d_keys, d_miss_rows, (const int32_t *)d_count, d_dense_values,
                           (const uint8_t *)d_dense_logits, d_out_values, (uint8_t *)d_out_logits, d_stats);
    hipLaunchKernelGGL(evalcache_finish_kernel, dim3(1), dim3(1), 0, s, t.epoch, d_count);
    return done();
}

int zc_evalcache_merge_scratch_bytes(int32_t n_rows, int64_t *bytes) {
    if (n_rows < 0 || !bytes) return ZC_EINVAL;
    *bytes = (claim_slots(n_rows) + n_rows) * (int64_t)sizeof(int32_t);
    return ZC_OK;
}

int zc_evalcache_probe_merged_async(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes,
                                    int32_t n_rows, int32_t rows_per_game, int32_t game_rows, const void *d_keys,
                                    const void *d_planes, int64_t plane_bytes, double *d_out_values,
                                    void *d_out_logits, void *d_dense_planes, int32_t *d_miss_rows, int32_t *d_count,
                                    int64_t *d_stats, void *d_scratch, void *hip_stream) {
    Table t;
    Merge m;
    bool has_table;
    if (!make_table_or_none(d_table, entries, key_bytes, logit_bytes, &t, &has_table)) return ZC_EINVAL;
    if (n_rows < 0 || rows_per_game < 1 || game_rows < rows_per_game || n_rows % rows_per_game) return ZC_EINVAL;
    if ((int64_t)(n_rows / rows_per_game) * game_rows >= ((int64_t)1 << 31)) return ZC_EINVAL;
    if (plane_bytes < 2 || (plane_bytes & 1) || !d_count || ((uintptr_t)d_count & 3) || ((uintptr_t)d_stats & 7))
        return ZC_EINVAL;
    if (!n_rows) return ZC_OK;
    if (!d_keys || !d_planes || !d_out_values || !d_dense_planes || !d_miss_rows || (logit_bytes && !d_out_logits))
        return ZC_EINVAL;
    if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_out_values & 7) || ((uintptr_t)d_miss_rows & 3) ||
        (((uintptr_t)d_planes | (uintptr_t)d_dense_planes | (uintptr_t)d_out_logits) & 1))
        return ZC_EINVAL;
    if (!make_merge(d_scratch, n_rows, &m)) return ZC_EINVAL;
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    hipLaunchKernelGGL(evalcache_probe_merged_kernel, dim3((n_rows + WAVES - 1) / WAVES), dim3(BLOCK), 0,
                       (hipStream_t)hip_stream, t, has_table, m, (int)n_rows, (int)rows_per_game, (int)game_rows,
                       (const uint64_t *)d_keys, (const uint8_t *)d_planes, plane_bytes, d_out_values,
                       (uint8_t *)d_out_logits, (uint8_t *)d_dense_planes, d_miss_rows, d_count, d_stats);
    return done();
}

int zc_evalcache_commit_merged_async(void *d_table, int64_t entries, int32_t key_bytes, int32_t logit_bytes,
                                     int32_t n_rows, int32_t rows_per_game, int32_t game_rows, const void *d_keys,
                                     const int32_t *d_miss_rows, int32_t *d_count, const double *d_dense_values,
                                     const void *d_dense_logits, double *d_out_values, void *d_out_logits,
                                     int64_t *d_stats, void *d_scratch, void *hip_stream) {
    Table t;
    Merge m{};
    bool has_table;
    if (!make_table_or_none(d_table, entries, key_bytes, logit_bytes, &t, &has_table)) return ZC_EINVAL;
    if (n_rows < 0 || !d_count || ((uintptr_t)d_count & 3) || ((uintptr_t)d_stats & 7)) return ZC_EINVAL;
    if (rows_per_game < 1 || game_rows < rows_per_game || n_rows % rows_per_game) return ZC_EINVAL;
    const int64_t total_rows = (int64_t)(n_rows / rows_per_game) * game_rows;
    if (total_rows >= ((int64_t)1 << 31)) return ZC_EINVAL;
    if (n_rows) {
        if (!d_keys || !d_miss_rows || !d_dense_values || !d_out_values ||
            (logit_bytes && (!d_dense_logits || !d_out_logits)))
            return ZC_EINVAL;
        if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_out_values & 7) || ((uintptr_t)d_dense_values & 7) ||
            ((uintptr_t)d_miss_rows & 3) || (((uintptr_t)d_dense_logits | (uintptr_t)d_out_logits) & 1))
            return ZC_EINVAL;
        if (!make_merge(d_scratch, n_rows, &m)) return ZC_EINVAL;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    const dim3 grid(n_rows ? (n_rows + WAVES - 1) / WAVES : 1);
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    if (n_rows && has_table)
        hipLaunchKernelGGL(evalcache_commit_kernel, grid, dim3(BLOCK), 0, s, t, (int)n_rows, total_rows,
                           (const uint64_t *)d_keys, d_miss_rows, (const int32_t *)d_count, d_dense_values,
                           (const uint8_t *)d_dense_logits, d_out_values, (uint8_t *)d_out_logits, d_stats);
    else if (n_rows)
        hipLaunchKernelGGL(evalcache_scatter_kernel, grid, dim3(BLOCK), 0, s, (int)n_rows, total_rows,
                           (int64_t)logit_bytes, d_miss_rows, (const int32_t *)d_count, d_dense_values,
                           (const uint8_t *)d_dense_logits, d_out_values, (uint8_t *)d_out_logits);
    hipLaunchKernelGGL(evalcache_finish_merged_kernel, grid, dim3(BLOCK), 0, s, m, (int)n_rows, (int)rows_per_game,
                       (int)game_rows, total_rows, (int64_t)logit_bytes, d_out_values, (uint8_t *)d_out_logits,
                       has_table ? t.epoch : (uint32_t *)nullptr, d_count);
    return done();
}

int zc_evalcache_probe_routed_async(void *d_table_a, void *d_table_b, int64_t entries, int32_t key_bytes,
                                    int32_t logit_bytes, int32_t n_rows, int32_t rows_per_game, int32_t game_rows,
                                    const int32_t *d_route, const void *d_keys, const void *d_planes,
                                    int64_t plane_bytes, double *d_out_values, void *d_out_logits,
                                    void *d_dense_planes_a, void *d_dense_planes_b, int32_t *d_miss_rows,
                                    int32_t *d_count, int64_t *d_stats, void *d_scratch, void *hip_stream) {
    Table ta, tb;
    Merge m{};
    bool has_table;
    if (!make_routed_tables(d_table_a, d_table_b, entries, key_bytes, logit_bytes, &ta, &tb, &has_table))
        return ZC_EINVAL;
    if (n_rows < 0 || rows_per_game < 1 || game_rows < rows_per_game || n_rows % rows_per_game) return ZC_EINVAL;
    if ((int64_t)(n_rows / rows_per_game) * game_rows >= ((int64_t)1 << 31)) return ZC_EINVAL;
    if (plane_bytes < 2 || (plane_bytes & 1) || !d_count || ((uintptr_t)d_count & 3) || ((uintptr_t)d_stats & 7) ||
        ((uintptr_t)d_scratch & 3))
        return ZC_EINVAL;
    if (!n_rows) return ZC_OK;
    if (!d_route || !d_keys || !d_planes || !d_out_values || !d_dense_planes_a || !d_dense_planes_b ||
        d_dense_planes_a == d_dense_planes_b || !d_miss_rows || (logit_bytes && !d_out_logits))
        return ZC_EINVAL;
    if (((uintptr_t)d_route & 3) || ((uintptr_t)d_keys & 7) || ((uintptr_t)d_out_values & 7) ||
        ((uintptr_t)d_miss_rows & 3) ||
        (((uintptr_t)d_planes | (uintptr_t)d_dense_planes_a | (uintptr_t)d_dense_planes_b | (uintptr_t)d_out_logits) &
         1))
        return ZC_EINVAL;
    if (d_scratch && !make_merge(d_scratch, n_rows, &m)) return ZC_EINVAL;
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    hipLaunchKernelGGL(evalcache_probe_routed_kernel, dim3((n_rows + WAVES - 1) / WAVES), dim3(BLOCK), 0,
                       (hipStream_t)hip_stream, ta, tb, has_table, m, d_route, (int)n_rows, (int)rows_per_game,
                       (int)game_rows, (const uint64_t *)d_keys, (const uint8_t *)d_planes, plane_bytes, d_out_values,
                       (uint8_t *)d_out_logits, (uint8_t *)d_dense_planes_a, (uint8_t *)d_dense_planes_b, d_miss_rows,
                       d_count, d_stats);
    return done();
}

int zc_evalcache_commit_routed_async(void *d_table_a, void *d_table_b, int64_t entries, int32_t key_bytes,
                                     int32_t logit_bytes, int32_t n_rows, int32_t rows_per_game, int32_t game_rows,
                                     const void *d_keys, const int32_t *d_miss_rows, int32_t *d_count,
                                     const double *d_dense_values_a, const void *d_dense_logits_a,
                                     const double *d_dense_values_b, const void *d_dense_logits_b,
                                     double *d_out_values, void *d_out_logits, int64_t *d_stats, void *d_scratch,
                                     void *hip_stream) {
    Table ta, tb;
    Merge m{};
    bool has_table;
    if (!make_routed_tables(d_table_a, d_table_b, entries, key_bytes, logit_bytes, &ta, &tb, &has_table))
        return ZC_EINVAL;
    if (n_rows < 0 || !d_count || ((uintptr_t)d_count & 3) || ((uintptr_t)d_stats & 7) || ((uintptr_t)d_scratch & 3))
        return ZC_EINVAL;
    if (rows_per_game < 1 || game_rows < rows_per_game || n_rows % rows_per_game) return ZC_EINVAL;
    const int64_t total_rows = (int64_t)(n_rows / rows_per_game) * game_rows;
    if (total_rows >= ((int64_t)1 << 31)) return ZC_EINVAL;
    if (n_rows) {
        if (!d_keys || !d_miss_rows || !d_dense_values_a || !d_dense_values_b || !d_out_values ||
            (logit_bytes && (!d_dense_logits_a || !d_dense_logits_b || !d_out_logits)))
            return ZC_EINVAL;
        if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_out_values & 7) ||
            (((uintptr_t)d_dense_values_a | (uintptr_t)d_dense_values_b) & 7) || ((uintptr_t)d_miss_rows & 3) ||
            (((uintptr_t)d_dense_logits_a | (uintptr_t)d_dense_logits_b | (uintptr_t)d_out_logits) & 1))
            return ZC_EINVAL;
        if (d_scratch && !make_merge(d_scratch, n_rows, &m)) return ZC_EINVAL;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    const bool merging = n_rows && d_scratch;
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    if (n_rows)
        hipLaunchKernelGGL(evalcache_commit_routed_kernel, dim3((n_rows + WAVES - 1) / WAVES), dim3(BLOCK), 0, s, ta,
                           tb, has_table, (int)n_rows, total_rows, (const uint64_t *)d_keys, d_miss_rows,
                           (const int32_t *)d_count, d_dense_values_a, (const uint8_t *)d_dense_logits_a,
                           d_dense_values_b, (const uint8_t *)d_dense_logits_b, d_out_values, (uint8_t *)d_out_logits,
                           d_stats);
    hipLaunchKernelGGL(evalcache_finish_routed_kernel, dim3(merging ? (n_rows + WAVES - 1) / WAVES : 1), dim3(BLOCK), 0,
                       s, m, merging ? (int)n_rows : 0, (int)rows_per_game, (int)game_rows, total_rows,
                       (int64_t)logit_bytes, d_out_values, (uint8_t *)d_out_logits,
                       has_table ? ta.epoch : (uint32_t *)nullptr, has_table ? tb.epoch : (uint32_t *)nullptr, d_count);
    return done();
}

}  // extern "C"
