// engine.hip — host side of the C-ABI (include/zeroclone.h): engine arena in HBM, per-game
// CPython-compatible random streams, argument checking, and the synchronous / stream-
// ordered search entry points.
#include <algorithm>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "c4_order_table.h"
#include "zc_internal.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define ZC_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return fail(ZC_EHIP, "%s failed: %s", #call, hipGetErrorString(e_));     \
    } while (0)

// CPython 3.10 Modules/_randommodule.c: random.seed(int) -> init_by_array(abs(n) as LE words).
void mt_init_by_array(uint32_t *mt, const uint32_t *key, int len) {
    mt[0] = 19650218u;
    for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    int i = 1, j = 0;
    for (int k = (624 > len ? 624 : len); k; k--) {
        mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
        i++;
        j++;
        if (i >= 624) { mt[0] = mt[623]; i = 1; }
        if (j >= len) j = 0;
    }
    for (int k = 623; k; k--) {
        mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
        i++;
        if (i >= 624) { mt[0] = mt[623]; i = 1; }
    }
    mt[0] = 0x80000000u;
}

template <class T>
int dalloc(zc_engine *e, T **p, size_t count) {
    const size_t bytes = count * sizeof(T);
    if (hipMalloc((void **)p, bytes ? bytes : 16) != hipSuccess)
        return fail(ZC_ENOMEM, "hipMalloc(%zu bytes) failed", bytes);
    e->bytes += (int64_t)bytes;
    return ZC_OK;
}

void free_chess(zc::ChessArena &c) {
    void *ptrs[] = {c.nodes, c.mv, c.ut, c.ch, c.na, c.w, c.prior, c.ctl, c.paths, c.meta, c.roots, c.xmv, c.xinfo,
                    c.remap, c.rbase};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    c = zc::ChessArena{};
}

void free_c4p(zc::C4PuctArena &c) {
    void *ptrs[] = {c.nodes, c.ctl, c.paths, c.meta, c.remap};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    c = zc::C4PuctArena{};
}

void free_gen(zc_engine *e) {
    zc::GenArena &g = e->ga;
    void *ptrs[] = {g.nodes, g.na, g.wa, g.qa, g.child, g.untried, g.ctl, g.pending};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    g = zc::GenArena{};
}

// The Connect4 arena and the synchronous calls' IO block are carved from ONE device
// allocation (base == nullptr: the offsets only, for the size), at 256-byte offsets: an
// engine's creation and destruction cost one hipMalloc / hipFree, not sixteen (a hipFree of a
// megabyte-sized block takes ~0.1 ms on this stack).
// search_sync's packed call block per game: inputs (root, game id), outputs (move, the root's
// visits per column, stats)
constexpr size_t kIoIn = sizeof(zc_c4_state) + sizeof(int32_t);
constexpr size_t kIoOut = sizeof(int32_t) * 8 + sizeof(zc_game_stats);
constexpr size_t kIoBytes = kIoIn + kIoOut;

template <class T>
void carve(uint8_t *base, size_t &off, T **p, size_t count) {
    off = (off + 255) & ~(size_t)255;
    *p = base ? (T *)(base + off) : nullptr;
    off += (count ? count : 1) * sizeof(T);
}

size_t carve_arena(zc_engine *e, uint8_t *base) {
    zc::Arena &a = e->a;
    const size_t G = (size_t)e->cfg.max_games, M = (size_t)e->M, B = (size_t)e->cfg.max_batch;
    size_t off = 0;
    carve(base, off, &a.nodes, G * M * zc::kRecBytes);
    carve(base, off, &a.ring, G * zc::kRingWords);
    carve(base, off, &a.rngpos, G * 2);
    carve(base, off, &a.logtab, M + 2);
    carve(base, off, &a.carry, G);
    carve(base, off, &a.progress, 64);
    carve(base, off, &a.phase, G * zc::kPhases);
    carve(base, off, &a.roots, G);
    carve(base, off, &a.move, G);
    carve(base, off, &a.na, G * 7);
    carve(base, off, &a.ids, G);
    carve(base, off, &a.stats, G);
    carve(base, off, &a.ext_ctl, G * zc::kCtlWords);
    carve(base, off, &a.ext_paths, G * B * zc::kMaxDepth);
    carve(base, off, &a.ext_meta, G * B);
    carve(base, off, &a.ext_roots, G);
    carve(base, off, &e->io_d, G * kIoBytes + 16);
    return off;
}

// Streams and pinned host blocks outlive their engines in per-process pools: creating a HIP
// stream costs milliseconds on this stack (a hardware queue), and an engine per game (the
// reference's Engine per game) would pay it every game.
std::mutex g_pool_mu;
std::vector<std::pair<int, hipStream_t>> g_streams;      // (device, idle stream)
std::vector<std::pair<size_t, uint8_t *>> g_pinned;      // (bytes, idle pinned block)

hipStream_t take_stream(int dev) {
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t i = 0; i < g_streams.size(); ++i)
            if (g_streams[i].first == dev) {
                hipStream_t s = g_streams[i].second;
                g_streams.erase(g_streams.begin() + (long)i);
                return s;
            }
    }
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    return s;
}

void give_stream(int dev, hipStream_t s) {  // s is idle (synchronised)
    if (!s) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_streams.emplace_back(dev, s);
}

// *bytes: the size wanted in, the block's real capacity out (the capacity is what the block
// returns to the pool under).  Best fit: the smallest idle block that is large enough.
uint8_t *take_pinned(size_t *bytes) {
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        long best = -1;
        for (size_t i = 0; i < g_pinned.size(); ++i)
            if (g_pinned[i].first >= *bytes && (best < 0 || g_pinned[i].first < g_pinned[(size_t)best].first))
                best = (long)i;
        if (best >= 0) {
            uint8_t *p = g_pinned[(size_t)best].second;
            *bytes = g_pinned[(size_t)best].first;
            g_pinned.erase(g_pinned.begin() + best);
            return p;
        }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, *bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return (uint8_t *)p;
}

void give_pinned(size_t bytes, uint8_t *p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pinned.emplace_back(bytes, p);
}

void free_arena(zc_engine *e) {
    if (e->a_block) (void)hipFree(e->a_block);
    e->a_block = nullptr;
    e->a = zc::Arena{};
    e->io_d = nullptr;
    give_pinned(e->io_h_bytes, e->io_h);
    e->io_h = nullptr;
}

int check_games(const zc_engine *e, int32_t first, int32_t n) {
    if (first < 0 || n < 0 || (int64_t)first + n > e->cfg.max_games)
        return fail(ZC_ECAPACITY, "games [%d, %d) outside engine capacity %d", first, first + n, e->cfg.max_games);
    return ZC_OK;
}

int check_search(const zc_engine *e, int32_t first, int32_t n, int32_t sims, double c, int32_t bs) {
    if (int r = check_games(e, first, n)) return r;
    if (sims < 1) return fail(ZC_EINVAL, "simulations must be >= 1 (got %d)", sims);
    if (bs < 1) return fail(ZC_EINVAL, "batch_size must be >= 1 (got %d)", bs);
    if (sims > e->cfg.max_sims) return fail(ZC_ECAPACITY, "simulations %d > engine max_sims %d", sims, e->cfg.max_sims);
    if (bs > e->cfg.max_batch) return fail(ZC_ECAPACITY, "batch_size %d > engine max_batch %d", bs, e->cfg.max_batch);
    if (!isfinite(c)) return fail(ZC_EINVAL, "c must be finite");
    return ZC_OK;
}

// Games with a self-play move carried over by zc_c4_selfplay_carry_async ([carry_lo, carry_hi),
// conservatively: every game a carry launch covered until a launch that resumes them all).
// Their trees and MT streams belong to the suspended searches: entry points that would search
// or reseed them refuse, so a game's moves stay the moves an uninterrupted run plays.
int check_carry(const zc_engine *e, int32_t first, int32_t n) {
    if (n > 0 && first < e->carry_hi && first + n > e->carry_lo)
        return fail(ZC_EINVAL, "games [%d, %d) overlap games [%d, %d) whose self-play moves are carried over "
                    "(zc_c4_selfplay_carry_async): finish them with zc_c4_selfplay_async / "
                    "zc_c4_selfplay_pooled_async over those games, or drop them with zc_c4_carry_discard",
                    first, first + n, e->carry_lo, e->carry_hi);
    return ZC_OK;
}

// A self-play launch with the visit-count staging registered (zc_*_selfplay_visits): its steps
// must fit the staging.
int check_visits_cap(const char *setter, const void *staging, int cap, int32_t moves) {
    if (staging && moves > cap)
        return fail(ZC_EINVAL, "%d steps exceed the %d steps of the visit-count staging (%s)", moves, cap, setter);
    return ZC_OK;
}

void carry_covered(zc_engine *e, int32_t first, int32_t n) {  // a launch that leaves none carried
    if (first <= e->carry_lo && first + n >= e->carry_hi) e->carry_lo = e->carry_hi = 0;
}

const zc_c4_state *roots_base(const zc_c4_state *d_roots, int32_t first) {  // game 0's row, never dereferenced
    return (const zc_c4_state *)((uintptr_t)d_roots - (uintptr_t)first * sizeof(zc_c4_state));
}

// A self-play launch while moves are carried over: the kernel resumes {simulations done, nodes,
// Philox tag} under THIS launch's parameters and re-reads the root from THIS launch's d_roots,
// so a launch that overlaps the carried games must bring what the suspending launch had (another
// sims / batch_size / c finishes the move as no uninterrupted search would; other root rows graft
// the kept tree onto another position).  The rollout mode and seed cannot differ: their setter
// refuses while moves are carried (zc_c4_set_rollout_mode).  A carry launch is checked even where it
// does not overlap: the engine keeps one record for the whole range.  Refused before anything is
// enqueued.
int check_resume(const zc_engine *e, int32_t first, int32_t n, const zc_c4_state *d_roots, int32_t sims, double c,
                 int32_t bs, int carry) {
    if (e->carry_hi <= e->carry_lo || n <= 0) return ZC_OK;
    if (!carry && !(first < e->carry_hi && first + n > e->carry_lo)) return ZC_OK;
    const zc_engine::CarrySearch &k = e->carried;
    const char *const tail = "finish the carried moves with the suspending launch's parameters and root buffer, or "
                             "drop them with zc_c4_carry_discard";
    if (sims != k.sims)
        return fail(ZC_EINVAL, "sims %d differs from the %d of the self-play moves carried over games [%d, %d): %s",
                    sims, k.sims, e->carry_lo, e->carry_hi, tail);
    if (bs != k.bs)
        return fail(ZC_EINVAL, "batch_size %d differs from the %d of the self-play moves carried over games "
                    "[%d, %d): %s", bs, k.bs, e->carry_lo, e->carry_hi, tail);
    if (c != k.c)
        return fail(ZC_EINVAL, "c %.17g differs from the %.17g of the self-play moves carried over games [%d, %d): %s",
                    c, k.c, e->carry_lo, e->carry_hi, tail);
    if (roots_base(d_roots, first) != k.roots0)
        return fail(ZC_EINVAL, "d_roots / first_game: game %d's root row is not the row the suspending launch gave "
                    "it (moves carried over games [%d, %d)): %s", first, e->carry_lo, e->carry_hi, tail);
    return ZC_OK;
}

bool valid_c4(const zc_c4_state &s) {
    const uint64_t full = 0x0000040810204081ull * 0x3Full;
    if ((s.stones[0] & s.stones[1]) || ((s.stones[0] | s.stones[1]) & ~full) || (s.turn & ~1)) return false;
    const uint64_t occ = s.stones[0] | s.stones[1];
    for (int c = 0; c < 7; ++c) {
        const uint64_t col = (occ >> (7 * c)) & 0x3Full;
        if (col & (col + 1)) return false;
    }
    return true;
}

zc::SearchParams make_params(zc_engine *e, int32_t first, int32_t n, const zc_c4_state *roots, int32_t sims,
                             double c, int32_t bs, int32_t *mv, int32_t *na, zc_game_stats *st) {
    zc::SearchParams p{};
    p.first_game = first;
    p.n_games = n;
    p.sims = sims;
    p.bs = bs;
    p.M = e->M;
    p.c = c;
    p.uct_delta = zc::uct_fast_delta(c, e->M);
    p.roots = roots;
    p.out_move = mv;
    p.out_na = na;
    p.out_stats = st;
    p.a = e->a;
    p.max_batch = e->cfg.max_batch;
    p.stamp = e->stamp;
    p.tstamps = e->tstamps;
    p.philox = e->rollout_mode == ZC_ROLLOUT_PHILOX;
    p.philox_seed = e->rollout_seed;
    return p;
}

}  // namespace

// ---------------------------------------------------------------- stepwise search
namespace {
using StepSearch = zc_engine::StepSearch;
using PuctSearch = zc_engine::PuctSearch;

// The four stepwise searches (zc_c4_ext_*, zc_chess_ext_*, zc_chess_puct_*, zc_c4_puct_*) share
// one protocol, begin -> [select(f) -> backup(f)] * flushes -> end, every step over games
// inside the begin call's range.
int value_flushes(int sims, int bs) { return (sims + bs - 1) / bs; }
int puct_flushes(int sims, int bs) { return 1 + (sims - 1 + bs - 1) / bs; }  // flush 0: the roots alone

void set_step(StepSearch &s, int32_t first, int32_t n, int32_t sims, double c, int32_t bs, int flushes) {
    s.first = first;
    s.n = n;
    s.sims = sims;
    s.bs = bs;
    s.flushes = flushes;
    s.c = c;
    s.active = true;
}

// A step of search `s` over games [first, first + n), and over flush `flush` where it has one.
int check_step(const StepSearch &s, int32_t first, int32_t n, int32_t flush, bool need_flush) {
    if (!s.active) return fail(ZC_EINVAL, "no %s search in progress (call %s_begin first)", s.what, s.what);
    if (first < s.first || n < 0 || (int64_t)first + n > (int64_t)s.first + s.n)
        return fail(ZC_EINVAL, "games [%d, %d) outside the %s search's range [%d, %d)", first, first + n, s.what,
                    s.first, s.first + s.n);
    if (need_flush && (flush < 0 || flush >= s.flushes))
        return fail(ZC_EINVAL, "flush %d outside [0, %d)", flush, s.flushes);
    return ZC_OK;
}

// A host-policy step (zc_*_hp_walk / zc_*_hp_expand) on one game's leaf `leaf` of flush `flush`.
int check_hp(const StepSearch &s, int32_t game, int32_t flush, int32_t leaf) {
    if (int r = check_step(s, game, 1, flush, true)) return r;
    const int nb = std::min(s.bs, s.sims - flush * s.bs);
    if (leaf < 0 || leaf >= nb) return fail(ZC_EINVAL, "leaf %d outside flush %d's [0, %d)", leaf, flush, nb);
    return ZC_OK;
}

// The frame of a step over games [first, first + n) of `search` (eng's record of it, evaluated
// once eng is known not to be null): the arguments (`cond`: the buffers n > 0 needs), the
// lock, the range and the flush, the device.
#define ZC_STEP_ENTRY(search, flush, need_flush, cond)                                          \
    if (!eng || (n && !(cond))) return fail(ZC_EINVAL, "null argument");                        \
    std::lock_guard<std::mutex> lk(eng->mu);                                                    \
    if (int r = check_step(search, first, n, flush, need_flush)) return r;                      \
    if (!n) return ZC_OK;                                                                       \
    ZC_HIP(hipSetDevice(eng->cfg.device));

int check_planes_dtype(int32_t planes_dtype) {
    if (planes_dtype != ZC_F32 && planes_dtype != ZC_F16) return fail(ZC_EINVAL, "planes_dtype must be ZC_F32 or ZC_F16");
    return ZC_OK;
}

zc::ExtParams ext_params(zc_engine *e, int32_t first, int32_t n) {
    zc::ExtParams p{};
    p.first_game = first;
    p.n_games = n;
    p.sims = e->c4_value.sims;
    p.bs = e->c4_value.bs;
    p.M = e->M;
    p.max_batch = e->cfg.max_batch;
    p.c = e->c4_value.c;
    p.a = e->a;
    return p;
}
}  // namespace

extern "C" {

const char *zc_version(void) { return "zeroclone_amd 0.1.0 (gfx950)"; }

const char *zc_last_error(void) { return g_err.c_str(); }

int zc_device_count(int32_t *count) {
    int n = 0;
    ZC_HIP(hipGetDeviceCount(&n));
    *count = n;
    return ZC_OK;
}

int zc_engine_create(const zc_engine_config *cfg, zc_engine **out) {
    if (!cfg || !out) return fail(ZC_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->max_games < 1) return fail(ZC_EINVAL, "max_games must be >= 1");
    if (cfg->max_sims < 1 || cfg->max_sims > 65533) return fail(ZC_EINVAL, "max_sims must be in [1, 65533]");
    if (cfg->max_batch < 1 || cfg->max_batch > 512) return fail(ZC_EINVAL, "max_batch must be in [1, 512]");
    int ndev = 0;
    ZC_HIP(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(ZC_EINVAL, "device %d not present (%d devices)", cfg->device, ndev);
    ZC_HIP(hipSetDevice(cfg->device));

    zc_engine *e = new zc_engine();
    e->cfg = *cfg;
    e->M = cfg->max_sims + 1;
    const size_t G = (size_t)cfg->max_games, M = (size_t)e->M;
    zc::Arena &a = e->a;
    int rc = ZC_OK;
    const size_t block = carve_arena(e, nullptr);
    if (hipMalloc(&e->a_block, block) != hipSuccess) {
        e->a_block = nullptr;
        rc = fail(ZC_ENOMEM, "hipMalloc(%zu bytes) failed", block);
    } else {
        e->bytes += (int64_t)block;
        carve_arena(e, (uint8_t *)e->a_block);
    }
    if (!rc) {
        e->io_h_bytes = G * kIoBytes + 16;
        e->io_h = take_pinned(&e->io_h_bytes);
        if (!e->io_h) rc = fail(ZC_ENOMEM, "hipHostMalloc(%zu bytes) failed", e->io_h_bytes);
    }
    if (!rc && !(e->stream = take_stream(cfg->device))) rc = fail(ZC_EHIP, "hipStreamCreate failed");
    if (!rc && (hipMemsetAsync(a.phase, 0, G * zc::kPhases * sizeof(int64_t), e->stream) != hipSuccess ||
                hipMemsetAsync(a.ext_ctl, 0, G * zc::kCtlWords * sizeof(int32_t), e->stream) != hipSuccess ||
                hipMemsetAsync(a.carry, 0, G * sizeof(uint4), e->stream) != hipSuccess))
        rc = fail(ZC_EHIP, "memset failed");
    if (!rc) {
        // log(N) exactly as the reference gets it: glibc log on the host (mcts.cpp:44).
        std::vector<double> lg(M + 2);
        for (size_t n = 0; n < M + 2; ++n) lg[n] = log((double)n);
        if (hipMemcpyAsync(a.logtab, lg.data(), lg.size() * sizeof(double), hipMemcpyHostToDevice, e->stream) !=
                hipSuccess ||
            hipStreamSynchronize(e->stream) != hipSuccess)
            rc = fail(ZC_EHIP, "logtab upload failed");
    }
    if (rc) {
        (void)hipDeviceSynchronize();
        free_arena(e);
        give_stream(cfg->device, e->stream);
        delete e;
        return rc;
    }
    *out = e;
    // every game starts as random.seed(game index)
    std::vector<uint64_t> seeds(G);
    for (size_t g = 0; g < G; ++g) seeds[g] = g;
    return zc_rng_seed(e, 0, (int32_t)G, seeds.data());
}

int zc_engine_destroy(zc_engine *eng) {
    if (!eng) return ZC_OK;
    {
        std::lock_guard<std::mutex> lk(eng->mu);
        (void)hipSetDevice(eng->cfg.device);
        (void)hipStreamSynchronize(eng->stream);
        free_arena(eng);
        free_chess(eng->ca);
        free_gen(eng);
        free_c4p(eng->c4p);
        give_stream(eng->cfg.device, eng->stream);
    }
    delete eng;
    return ZC_OK;
}

int zc_engine_footprint(const zc_engine *eng, int64_t *bytes) {
    if (!eng || !bytes) return fail(ZC_EINVAL, "null argument");
    *bytes = eng->bytes;
    return ZC_OK;
}

int zc_rng_seed(zc_engine *eng, int32_t first, int32_t n, const uint64_t *seeds) {
    if (!eng || (!seeds && n)) return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, first, n)) return r;
    if (int r = check_carry(eng, first, n)) return r;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    std::vector<uint32_t> words((size_t)n * 624);
    std::vector<uint64_t> pos((size_t)n * 2);
    for (int32_t i = 0; i < n; ++i) {
        const uint32_t key[2] = {(uint32_t)seeds[i], (uint32_t)(seeds[i] >> 32)};
        mt_init_by_array(&words[(size_t)i * 624], key, key[1] ? 2 : 1);
        pos[2 * (size_t)i] = 624;   // index 624: the next draw twists (random.seed leaves this)
        pos[2 * (size_t)i + 1] = 624;
    }
    if (n) {
        ZC_HIP(hipMemcpy2DAsync(eng->a.ring + (size_t)first * zc::kRingWords, zc::kRingWords * sizeof(uint32_t),
                                words.data(), 624 * sizeof(uint32_t), 624 * sizeof(uint32_t), (size_t)n,
                                hipMemcpyHostToDevice, eng->stream));
        ZC_HIP(hipMemcpyAsync(eng->a.rngpos + 2 * (size_t)first, pos.data(), pos.size() * sizeof(uint64_t),
                              hipMemcpyHostToDevice, eng->stream));
        ZC_HIP(hipStreamSynchronize(eng->stream));
    }
    return ZC_OK;
}

int zc_rng_set_state(zc_engine *eng, int32_t game, const uint32_t *mt624, int32_t index) {
    if (!eng || !mt624) return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, game, 1)) return r;
    if (int r = check_carry(eng, game, 1)) return r;
    if (index < 0 || index > 624) return fail(ZC_EINVAL, "MT index must be in [0, 624] (got %d)", index);
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    const uint64_t pos[2] = {(uint64_t)index, 624};
    ZC_HIP(hipMemcpyAsync(eng->a.ring + (size_t)game * zc::kRingWords, mt624, 624 * sizeof(uint32_t),
                          hipMemcpyHostToDevice, eng->stream));
    ZC_HIP(hipMemcpyAsync(eng->a.rngpos + 2 * (size_t)game, pos, sizeof pos, hipMemcpyHostToDevice, eng->stream));
    ZC_HIP(hipStreamSynchronize(eng->stream));
    return ZC_OK;
}

int zc_rng_get_state(zc_engine *eng, int32_t game, uint32_t *mt624, int32_t *index) {
    if (!eng || !mt624 || !index) return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, game, 1)) return r;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    uint64_t pos[2];
    std::vector<uint32_t> ring(zc::kRingWords);
    ZC_HIP(hipMemcpyAsync(pos, eng->a.rngpos + 2 * (size_t)game, sizeof pos, hipMemcpyDeviceToHost, eng->stream));
    ZC_HIP(hipMemcpyAsync(ring.data(), eng->a.ring + (size_t)game * zc::kRingWords, zc::kRingWords * sizeof(uint32_t),
                          hipMemcpyDeviceToHost, eng->stream));
    ZC_HIP(hipStreamSynchronize(eng->stream));
    // Python's state after consuming word `use-1`: the 624-word block holding it, and the
    // offset of the next word inside that block (624 = block exhausted).  CPython twists a
    // whole block at once; the kernels generate words only as far as they read, so the
    // block's words beyond pos[1] (words generated) are completed here by the recurrence.
    const uint64_t use = pos[0];
    const uint64_t blk = use == 0 ? 0 : (use - 1) / 624;
    for (uint64_t p = std::max<uint64_t>(pos[1], 624); p < (blk + 1) * 624; ++p) {
        const uint32_t m = zc::kRingWords - 1;
        const uint32_t a = ring[(p - 624) & m], b = ring[(p - 623) & m], x = ring[(p - 227) & m];
        const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
        ring[p & m] = x ^ (y >> 1) ^ ((b & 1u) ? 0x9908b0dfu : 0u);
    }
    for (int i = 0; i < 624; ++i) mt624[i] = ring[(blk * 624 + (uint64_t)i) & (zc::kRingWords - 1)];
    *index = (int32_t)(use - blk * 624);
    return ZC_OK;
}

int zc_c4_selfplay_async(zc_engine *eng, int32_t first, int32_t n, zc_c4_state *d_roots, int32_t sims, double c,
                         int32_t bs, int32_t moves, zc_c4_state *d_out_states, int16_t *d_out_moves,
                         int32_t *d_out_results, zc_game_stats *d_stats, void *hip_stream) {
    if (!eng || (n && (!d_roots || !d_out_states || !d_out_moves || !d_out_results || !d_stats)))
        return fail(ZC_EINVAL, "null argument");
    if (int r = check_search(eng, first, n, sims, c, bs)) return r;
    if (moves < 1) return fail(ZC_EINVAL, "moves must be >= 1 (got %d)", moves);
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_resume(eng, first, n, d_roots, sims, c, bs, 0)) return r;
    if (int r = check_visits_cap("zc_c4_selfplay_visits", eng->c4_visits, eng->c4_visits_cap, moves)) return r;
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::SearchParams p = make_params(eng, first, n, d_roots, sims, c, bs, nullptr, eng->c4_visits, d_stats);
    p.moves = moves;
    p.io_roots = d_roots;
    p.out_states = d_out_states;
    p.out_moves16 = d_out_moves;
    p.out_results = d_out_results;
    // the pace-balancing counter (priorities only: two free runs of one engine in flight on
    // different streams would share it and balance less well, with the same outputs)
    ZC_HIP(hipMemsetAsync(eng->a.progress, 0, sizeof(int32_t), (hipStream_t)hip_stream));
    p.progress = eng->a.progress;
    zc::launch_c4_selfplay(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    carry_covered(eng, first, n);   // carried moves resume first and this launch suspends none
    return ZC_OK;
}

namespace {
int c4_pooled(zc_engine *eng, int32_t first, int32_t n, zc_c4_state *d_roots, int32_t sims, double c, int32_t bs,
              int32_t moves_cap, int64_t budget, int32_t *d_ticket, zc_c4_state *d_out_states, int16_t *d_out_moves,
              int32_t *d_out_results, zc_game_stats *d_stats, void *hip_stream, int carry) {
    if (!eng || (n && (!d_roots || !d_out_states || !d_out_moves || !d_out_results || !d_stats || !d_ticket)))
        return fail(ZC_EINVAL, "null argument");
    if (int r = check_search(eng, first, n, sims, c, bs)) return r;
    if (moves_cap < 1) return fail(ZC_EINVAL, "moves_cap must be >= 1 (got %d)", moves_cap);
    if (budget < 0 || budget > (int64_t)moves_cap * n || budget >= ((int64_t)1 << 31))
        return fail(ZC_EINVAL, "budget %lld outside [0, moves_cap x n_games] or >= 2^31", (long long)budget);
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_resume(eng, first, n, d_roots, sims, c, bs, carry)) return r;
    if (int r = check_visits_cap("zc_c4_selfplay_visits", eng->c4_visits, eng->c4_visits_cap, moves_cap)) return r;
    ZC_HIP(hipSetDevice(eng->cfg.device));
    // A wave takes its tickets only once resident: with more games than the chip holds at
    // once, the first waves could spend the whole budget and the rest never move.  Refused.
    // The check assumes the device runs nothing else: ranks sharing one GPU (bench.py
    // --share-device, a rehearsal mode) or concurrent kernels can still delay some
    // workgroups past the budget, and those games then make no move in that launch (their
    // rows report ZC_SLOT_IDLE; nothing is lost, only the moves' spread over games shifts).
    int resident = 0;
    if (zc::c4_selfplay_resident_games(bs, eng->rollout_mode == ZC_ROLLOUT_PHILOX, &resident))
        return fail(ZC_EHIP, "occupancy query failed");
    if (n > resident)
        return fail(ZC_EINVAL, "pooled self-play of %d games: at most %d (batch %d) are resident at once, and "
                    "the rest would never move; use zc_c4_selfplay_async or fewer games per launch", n, resident, bs);
    hipStream_t s = (hipStream_t)hip_stream;
    ZC_HIP(hipMemsetAsync(d_ticket, 0, 2 * sizeof(int32_t), s));
    zc::SearchParams p = make_params(eng, first, n, d_roots, sims, c, bs, nullptr, eng->c4_visits, d_stats);
    p.moves = moves_cap;
    p.io_roots = d_roots;
    p.out_states = d_out_states;
    p.out_moves16 = d_out_moves;
    p.out_results = d_out_results;
    p.ticket = d_ticket;
    p.budget = (int32_t)budget;
    p.carry = carry;
    zc::launch_c4_selfplay(p, s);
    ZC_HIP(hipGetLastError());
    if (!carry) {
        carry_covered(eng, first, n);
    } else if (eng->carry_hi <= eng->carry_lo) {
        eng->carry_lo = first;
        eng->carry_hi = first + n;
        eng->carried = {sims, bs, c, roots_base(d_roots, first)};
    } else {  // same parameters and root rows (check_resume): the one record holds
        eng->carry_lo = std::min(eng->carry_lo, first);
        eng->carry_hi = std::max(eng->carry_hi, first + n);
    }
    return ZC_OK;
}
}  // namespace

int zc_c4_selfplay_pooled_async(zc_engine *eng, int32_t first, int32_t n, zc_c4_state *d_roots, int32_t sims,
                                double c, int32_t bs, int32_t moves_cap, int64_t budget, int32_t *d_ticket,
                                zc_c4_state *d_out_states, int16_t *d_out_moves, int32_t *d_out_results,
                                zc_game_stats *d_stats, void *hip_stream) {
    return c4_pooled(eng, first, n, d_roots, sims, c, bs, moves_cap, budget, d_ticket, d_out_states, d_out_moves,
                     d_out_results, d_stats, hip_stream, 0);
}

int zc_c4_selfplay_carry_async(zc_engine *eng, int32_t first, int32_t n, zc_c4_state *d_roots, int32_t sims,
                               double c, int32_t bs, int32_t moves_cap, int64_t budget, int32_t *d_ticket,
                               zc_c4_state *d_out_states, int16_t *d_out_moves, int32_t *d_out_results,
                               zc_game_stats *d_stats, void *hip_stream) {
    return c4_pooled(eng, first, n, d_roots, sims, c, bs, moves_cap, budget, d_ticket, d_out_states, d_out_moves,
                     d_out_results, d_stats, hip_stream, 1);
}

int zc_c4_selfplay_visits(zc_engine *eng, int32_t *d_na, int32_t steps_cap) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    if (d_na && steps_cap < 1) return fail(ZC_EINVAL, "steps_cap must be >= 1 (got %d)", steps_cap);
    std::lock_guard<std::mutex> lk(eng->mu);
    eng->c4_visits = d_na;
    eng->c4_visits_cap = d_na ? steps_cap : 0;
    return ZC_OK;
}

int zc_c4_carry_discard(zc_engine *eng, int32_t first, int32_t n, void *hip_stream) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, first, n)) return r;
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    ZC_HIP(hipMemsetAsync(eng->a.carry + first, 0, (size_t)n * sizeof(uint4), (hipStream_t)hip_stream));
    carry_covered(eng, first, n);
    return ZC_OK;
}

int zc_c4_pooled_max_games(zc_engine *eng, int32_t batch_size, int32_t *out) {
    if (!eng || !out) return fail(ZC_EINVAL, "null argument");
    if (batch_size < 1 || batch_size > eng->cfg.max_batch) return fail(ZC_EINVAL, "bad batch_size %d", batch_size);
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    int r = 0;
    if (zc::c4_selfplay_resident_games(batch_size, eng->rollout_mode == ZC_ROLLOUT_PHILOX, &r))
        return fail(ZC_EHIP, "occupancy query failed");
    *out = r;
    return ZC_OK;
}

int zc_c4_search_async(zc_engine *eng, int32_t first, int32_t n, const zc_c4_state *d_roots, int32_t sims, double c,
                       int32_t bs, int32_t *d_move, int32_t *d_na, zc_game_stats *d_stats, void *hip_stream) {
    if (!eng || (n && (!d_roots || !d_move || !d_na || !d_stats))) return fail(ZC_EINVAL, "null argument");
    if (int r = check_search(eng, first, n, sims, c, bs)) return r;
    if (int r = check_carry(eng, first, n)) return r;
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    hipStream_t s = (hipStream_t)hip_stream;
    zc::launch_c4_search(make_params(eng, first, n, d_roots, sims, c, bs, d_move, d_na, d_stats), s);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

namespace {
int search_sync(zc_engine *eng, int32_t first, int32_t n, const int32_t *ids, const zc_c4_state *roots, int32_t sims,
                double c, int32_t bs, int32_t *out_move, int32_t *out_na, zc_game_stats *out_stats) {
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    hipStream_t s = eng->stream;
    // inputs [roots | ids] and outputs [moves | visits (n x 7) | stats] at 16-byte offsets in
    // one block: one host-to-device and one device-to-host copy, both through pinned memory
    const size_t rb = (size_t)n * sizeof(zc_c4_state), ib = ids ? (size_t)n * sizeof(int32_t) : 0;
    const size_t ob = (rb + ib + 15) & ~(size_t)15;
    const size_t outb = (size_t)n * kIoOut;
    uint8_t *const hb = eng->io_h, *const db = eng->io_d;
    memcpy(hb, roots, rb);
    if (ids) memcpy(hb + rb, ids, ib);
    ZC_HIP(hipMemcpyAsync(db, hb, rb + ib, hipMemcpyHostToDevice, s));
    // from here on the pinned block may be in flight: every return drains the stream first, so
    // the next call's memcpy into the block cannot race this call's copies
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{s};
    int32_t *const d_move = (int32_t *)(db + ob);
    zc::SearchParams p = make_params(eng, first, n, (const zc_c4_state *)db, sims, c, bs, d_move, d_move + n,
                                     (zc_game_stats *)(db + ob + (size_t)n * 32));
    p.game_ids = ids ? (const int32_t *)(db + rb) : nullptr;
    zc::launch_c4_search(p, s);
    ZC_HIP(hipGetLastError());
    ZC_HIP(hipMemcpyAsync(hb + ob, db + ob, outb, hipMemcpyDeviceToHost, s));
    ZC_HIP(hipStreamSynchronize(s));
    memcpy(out_move, hb + ob, (size_t)n * sizeof(int32_t));
    memcpy(out_na, hb + ob + (size_t)n * 4, (size_t)n * 7 * sizeof(int32_t));
    const zc_game_stats *const st = (const zc_game_stats *)(hb + ob + (size_t)n * 32);
    if (out_stats) memcpy(out_stats, st, (size_t)n * sizeof(zc_game_stats));
    for (int32_t i = 0; i < n; ++i) {
        const int g = ids ? ids[i] : first + i;
        if (st[i].status == ZC_STATUS_NO_MOVES)
            return fail(ZC_EINVAL, "game %d: root has no legal move (reference: undefined behaviour)", g);
        if (st[i].status == ZC_STATUS_INTERNAL)
            return fail(ZC_EDEVICE, "game %d: search invariant violated on the device", g);
        if (st[i].status)
            return fail(ZC_EINVAL, "game %d: invalid Connect4 state (status %lld)", g, (long long)st[i].status);
    }
    return ZC_OK;
}
}  // namespace

int zc_c4_set_rollout_mode(zc_engine *eng, int32_t mode, uint64_t seed) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    if (mode != ZC_ROLLOUT_EXACT && mode != ZC_ROLLOUT_PHILOX) return fail(ZC_EINVAL, "unknown rollout mode %d", mode);
    std::lock_guard<std::mutex> lk(eng->mu);
    if (eng->carry_hi > eng->carry_lo)
        return fail(ZC_EINVAL, "the rollout mode cannot change while self-play moves are carried over games [%d, %d) "
                    "(zc_c4_selfplay_carry_async): their searches would change generator mid-move; finish or "
                    "discard them first", eng->carry_lo, eng->carry_hi);
    eng->rollout_mode = mode;
    eng->rollout_seed = seed;
    return ZC_OK;
}

int zc_c4_search(zc_engine *eng, int32_t first, int32_t n, const zc_c4_state *roots, int32_t sims, double c,
                 int32_t bs, int32_t *out_move, int32_t *out_na, zc_game_stats *out_stats) {
    if (!eng || (n && (!roots || !out_move || !out_na))) return fail(ZC_EINVAL, "null argument");
    if (int r = check_search(eng, first, n, sims, c, bs)) return r;
    if (int r = check_carry(eng, first, n)) return r;
    if (!n) return ZC_OK;
    return search_sync(eng, first, n, nullptr, roots, sims, c, bs, out_move, out_na, out_stats);
}

int zc_c4_search_games(zc_engine *eng, int32_t n, const int32_t *games, const zc_c4_state *roots, int32_t sims,
                       double c, int32_t bs, int32_t *out_move, int32_t *out_na, zc_game_stats *out_stats) {
    if (!eng || (n && (!games || !roots || !out_move || !out_na))) return fail(ZC_EINVAL, "null argument");
    if (int r = check_search(eng, 0, 0, sims, c, bs)) return r;
    if (n > eng->cfg.max_games) return fail(ZC_ECAPACITY, "%d games > engine capacity %d", n, eng->cfg.max_games);
    std::vector<char> seen((size_t)eng->cfg.max_games, 0);
    for (int32_t i = 0; i < n; ++i) {
        if (games[i] < 0 || games[i] >= eng->cfg.max_games)
            return fail(ZC_ECAPACITY, "game %d outside engine capacity %d", games[i], eng->cfg.max_games);
        if (seen[(size_t)games[i]]++) return fail(ZC_EINVAL, "game %d listed twice", games[i]);
        if (int r = check_carry(eng, games[i], 1)) return r;
    }
    if (!n) return ZC_OK;
    return search_sync(eng, 0, n, games, roots, sims, c, bs, out_move, out_na, out_stats);
}

int zc_c4_play_async(zc_engine *eng, int32_t n, zc_c4_state *d_states, const int32_t *d_moves, int32_t *d_results,
                     int32_t reset, void *hip_stream) {
    if (!eng || n < 0 || (n && (!d_states || !d_moves || !d_results))) return fail(ZC_EINVAL, "bad argument");
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    hipStream_t s = (hipStream_t)hip_stream;
    zc::launch_c4_play(n, d_states, d_moves, d_results, reset, s);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_c4_rollouts(zc_engine *eng, int32_t game, int32_t n, const zc_c4_state *states, int32_t *out_values,
                   int64_t *out_words) {
    if (!eng || n < 0 || (n && (!states || !out_values))) return fail(ZC_EINVAL, "bad argument");
    if (int r = check_games(eng, game, 1)) return r;
    if (int r = check_carry(eng, game, 1)) return r;
    for (int32_t i = 0; i < n; ++i)
        if (!valid_c4(states[i])) return fail(ZC_EINVAL, "state %d is not a valid Connect4 position", i);
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    hipStream_t s = eng->stream;
    zc_c4_state *ds = nullptr;
    int32_t *dv = nullptr;
    int64_t *dw = nullptr;
    ZC_HIP(hipMalloc(&ds, (n ? n : 1) * sizeof(zc_c4_state)));
    ZC_HIP(hipMalloc(&dv, (n ? n : 1) * sizeof(int32_t)));
    ZC_HIP(hipMalloc(&dw, sizeof(int64_t)));
    if (n) ZC_HIP(hipMemcpyAsync(ds, states, (size_t)n * sizeof(zc_c4_state), hipMemcpyHostToDevice, s));
    zc::launch_c4_rollout_seq(eng->a, game, n, ds, dv, dw, s);
    ZC_HIP(hipGetLastError());
    int64_t words = 0;
    if (n) ZC_HIP(hipMemcpyAsync(out_values, dv, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ZC_HIP(hipMemcpyAsync(&words, dw, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ZC_HIP(hipStreamSynchronize(s));
    (void)hipFree(ds);
    (void)hipFree(dv);
    (void)hipFree(dw);
    if (out_words) *out_words = words;
    return ZC_OK;
}


int zc_c4_ext_begin(zc_engine *eng, int32_t first, int32_t n, const zc_c4_state *d_roots, int32_t sims, double c,
                    int32_t bs, void *hip_stream) {
    if (!eng || (n && !d_roots)) return fail(ZC_EINVAL, "null argument");
    if (int r = check_search(eng, first, n, sims, c, bs)) return r;
    if (int r = check_carry(eng, first, n)) return r;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    set_step(eng->c4_value, first, n, sims, c, bs, value_flushes(sims, bs));
    if (!n) return ZC_OK;
    zc::ExtParams p = ext_params(eng, first, n);
    p.roots = d_roots;
    zc::launch_c4_ext_begin(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_c4_ext_select(zc_engine *eng, int32_t first, int32_t n, int32_t flush, zc_c4_state *d_leaves, void *d_planes,
                     int32_t planes_dtype, int32_t *d_counts, void *hip_stream) {
    if (int r = check_planes_dtype(planes_dtype)) return r;
    ZC_STEP_ENTRY(eng->c4_value, flush, true, true)
    zc::ExtParams p = ext_params(eng, first, n);
    p.flush = flush;
    p.leaves = d_leaves;
    p.planes = d_planes;
    p.planes_f16 = planes_dtype == ZC_F16;
    p.counts = d_counts;
    zc::launch_c4_ext_select(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_c4_ext_backup(zc_engine *eng, int32_t first, int32_t n, int32_t flush, const double *d_values,
                     void *hip_stream) {
    ZC_STEP_ENTRY(eng->c4_value, flush, true, d_values)
    zc::ExtParams p = ext_params(eng, first, n);
    p.flush = flush;
    p.values = d_values;
    zc::launch_c4_ext_backup(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_c4_ext_end(zc_engine *eng, int32_t first, int32_t n, int32_t *d_move, int32_t *d_na, zc_game_stats *d_stats,
                  void *hip_stream) {
    ZC_STEP_ENTRY(eng->c4_value, 0, false, d_move && d_na && d_stats)
    zc::ExtParams p = ext_params(eng, first, n);
    p.out_move = d_move;
    p.out_na = d_na;
    p.out_stats = d_stats;
    zc::launch_c4_ext_end(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_c4_hp_walk(zc_engine *eng, int32_t game, int32_t flush, int32_t leaf, zc_c4_hp_node *d_node,
                  void *hip_stream) {
    if (!eng || !d_node) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_hp(eng->c4_value, game, flush, leaf)) return r;
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::ExtParams p = ext_params(eng, game, 1);
    p.flush = flush;
    p.hp_leaf = leaf;
    p.hp_node = d_node;
    zc::launch_c4_hp_walk(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_c4_hp_expand(zc_engine *eng, int32_t game, int32_t flush, int32_t leaf, int32_t untried_index,
                    zc_c4_state *d_leaf, void *hip_stream) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_hp(eng->c4_value, game, flush, leaf)) return r;
    if (untried_index < -1 || untried_index > 6) return fail(ZC_EINVAL, "untried index %d outside [-1, 7)", untried_index);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::ExtParams p = ext_params(eng, game, 1);
    p.flush = flush;
    p.hp_leaf = leaf;
    p.hp_index = untried_index;
    p.leaves = d_leaf;
    zc::launch_c4_hp_expand(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

// ---------------------------------------------------------------- chess rules
#define ZC_CHESS_ENTRY(cond)                                                   \
    if (!eng || n < 0 || (n && !(cond))) return fail(ZC_EINVAL, "bad argument"); \
    if (!n) return ZC_OK;                                                      \
    std::lock_guard<std::mutex> lk(eng->mu);                                   \
    ZC_HIP(hipSetDevice(eng->cfg.device));

int zc_chess_legal_moves_async(zc_engine *eng, int32_t n, const zc_chess_state *d_states, uint16_t *d_moves,
                               int32_t *d_counts, void *hip_stream) {
    ZC_CHESS_ENTRY(d_states && d_moves && d_counts)
    zc::launch_chess_legal(n, d_states, d_moves, d_counts, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_debug_chess_probe_async(zc_engine *eng, int32_t n, const zc_chess_state *d_states, int32_t *d_out,
                               void *hip_stream) {
    ZC_CHESS_ENTRY(d_states && d_out)
    zc::launch_chess_probe(n, d_states, d_out, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_children_async(zc_engine *eng, int32_t n, const zc_chess_state *d_states, zc_chess_state *d_children,
                            uint16_t *d_moves, int32_t *d_counts, void *hip_stream) {
    ZC_CHESS_ENTRY(d_states && d_children && d_counts)
    zc::launch_chess_children(n, d_states, d_children, d_moves, d_counts, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_play_async(zc_engine *eng, int32_t n, const zc_chess_state *d_in, const uint16_t *d_moves,
                        zc_chess_state *d_out, void *hip_stream) {
    ZC_CHESS_ENTRY(d_in && d_moves && d_out)
    zc::launch_chess_play(n, d_in, d_moves, d_out, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_terminal_async(zc_engine *eng, int32_t n, const zc_chess_state *d_states, int32_t *d_flags,
                            void *hip_stream) {
    ZC_CHESS_ENTRY(d_states && d_flags)
    zc::launch_chess_terminal(n, d_states, d_flags, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_repetition_async(int32_t n, int32_t cap, const uint16_t *d_hist, const int32_t *d_len, int32_t *d_out,
                              void *hip_stream) {
    if (n < 0 || (n && (!d_hist || !d_len || !d_out))) return fail(ZC_EINVAL, "bad argument");
    if (!n) return ZC_OK;
    if (!zc::launch_chess_repetition(n, cap, d_hist, d_len, d_out, (hipStream_t)hip_stream))
        return fail(ZC_EINVAL, "history capacity %d outside [1, 4096]", cap);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

namespace {
int check_traj(int32_t n, const zc_traj_buffers *buf, const void *d_states) {
    if (n < 0 || !buf) return fail(ZC_EINVAL, "bad argument");
    const zc_traj_buffers &b = *buf;
    if (b.row_bytes < 8 || (b.row_bytes & 7) || b.max_len < 2 || b.pool_cap < 0 || b.pool_cap > INT32_MAX ||
        b.games_cap < 0)
        return fail(ZC_EINVAL, "bad trajectory buffer shape (row_bytes %d, max_len %d)", b.row_bytes, b.max_len);
    if (!b.d_hist || !b.d_hmoves || !b.d_slot || !b.d_pool || !b.d_labels || !b.d_pool_moves || !b.d_games ||
        !b.d_ctl || !b.d_init)
        return fail(ZC_EINVAL, "null trajectory buffer");
    if (((uintptr_t)b.d_hist | (uintptr_t)b.d_pool | (uintptr_t)b.d_init | (uintptr_t)d_states) & 7)
        return fail(ZC_EINVAL, "rows must be 8-byte aligned");
    return ZC_OK;
}
}  // namespace

int zc_traj_steps_scratch_bytes(int32_t n, int32_t steps, int64_t *bytes) {
    if (n < 0 || steps < 0 || !bytes) return fail(ZC_EINVAL, "bad argument");
    *bytes = (int64_t)zc::traj_steps_scratch_bytes(n, steps);
    return ZC_OK;
}

int zc_traj_record_steps_async(int32_t n, const zc_traj_buffers *buf, void *d_states, const int16_t *d_moves,
                               int32_t *d_results, int32_t steps, const int32_t *d_reached, void *d_scratch,
                               int64_t scratch_bytes, void *hip_stream) {
    if (int r = check_traj(n, buf, d_states)) return r;
    if (steps < 0) return fail(ZC_EINVAL, "steps must be >= 0 (got %d)", steps);
    if ((int64_t)n * steps >= ((int64_t)1 << 31)) return fail(ZC_EINVAL, "n x steps must be < 2^31");
    if (n && steps && (!d_states || !d_moves || !d_results)) return fail(ZC_EINVAL, "bad argument");
    if (!n || !steps) return ZC_OK;
    if (!d_scratch || ((uintptr_t)d_scratch & 15) || scratch_bytes < (int64_t)zc::traj_steps_scratch_bytes(n, steps))
        return fail(ZC_EINVAL, "scratch: %lld bytes at %p, need %zu bytes 16-byte aligned", (long long)scratch_bytes,
                    d_scratch, zc::traj_steps_scratch_bytes(n, steps));
    zc::launch_traj_record_steps(n, steps, *buf, d_states, d_moves, d_results, d_reached, d_scratch,
                                 (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_traj_record_async(int32_t n, const zc_traj_buffers *buf, void *d_states, const int16_t *d_moves,
                         int32_t *d_results, const int32_t *d_flags, const int32_t *d_rep, void *hip_stream) {
    if (n < 0 || !buf) return fail(ZC_EINVAL, "bad argument");
    const zc_traj_buffers &b = *buf;
    if (b.row_bytes < 8 || (b.row_bytes & 7) || b.max_len < 2 || b.pool_cap < 0 || b.pool_cap > INT32_MAX ||
        b.games_cap < 0)
        return fail(ZC_EINVAL, "bad trajectory buffer shape (row_bytes %d, max_len %d)", b.row_bytes, b.max_len);
    if (!b.d_hist || !b.d_hmoves || !b.d_slot || !b.d_pool || !b.d_labels || !b.d_pool_moves || !b.d_games ||
        !b.d_ctl || !b.d_init)
        return fail(ZC_EINVAL, "null trajectory buffer");
    if (((uintptr_t)b.d_hist | (uintptr_t)b.d_pool | (uintptr_t)b.d_init | (uintptr_t)d_states) & 7)
        return fail(ZC_EINVAL, "rows must be 8-byte aligned");
    if (n && (!d_states || !d_moves || !d_results)) return fail(ZC_EINVAL, "bad argument");
    if (!n) return ZC_OK;
    zc::launch_traj_record(n, b, d_states, d_moves, d_results, d_flags, d_rep, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_traj_openings_async(int32_t n, const zc_traj_buffers *buf, const void *d_book, int32_t book_rows,
                           int32_t share, void *d_roots, void *hip_stream) {
    if (int r = check_traj(n, buf, d_roots)) return r;
    if (book_rows < 1 || share < 1)
        return fail(ZC_EINVAL, "book_rows and share must be >= 1 (got %d, %d)", book_rows, share);
    if (!d_book || !d_roots) return fail(ZC_EINVAL, "bad argument");
    if ((uintptr_t)d_book & 7) return fail(ZC_EINVAL, "rows must be 8-byte aligned");
    if (!n) return ZC_OK;
    zc::launch_traj_openings(n, *buf, d_book, book_rows, share, d_roots, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

namespace {
int check_traj_policy(const zc_traj_policy_buffers *pol) {
    if (!pol) return fail(ZC_EINVAL, "bad argument");
    const zc_traj_policy_buffers &q = *pol;
    if (q.slot_cap < 0 || q.pi_pool_cap < 0)
        return fail(ZC_EINVAL, "bad policy buffer shape (slot_cap %d, pi_pool_cap %lld)", q.slot_cap,
                    (long long)q.pi_pool_cap);
    if (!q.d_slot_pi || !q.d_slot_off || !q.d_slot_base || !q.d_pool_pi || !q.d_pool_first || !q.d_pool_count ||
        !q.d_pctl)
        return fail(ZC_EINVAL, "null policy buffer");
    return ZC_OK;
}
}  // namespace

int zc_traj_policy_append_async(int32_t n, const zc_traj_buffers *buf, const zc_traj_policy_buffers *pol,
                                const int32_t *d_root_na, const uint16_t *d_root_moves, int32_t stride,
                                void *hip_stream) {
    if (int r = check_traj(n, buf, nullptr)) return r;
    if (int r = check_traj_policy(pol)) return r;
    if (stride < 1 || stride > 65536) return fail(ZC_EINVAL, "stride must be in [1, 65536] (got %d)", stride);
    if (n && !d_root_na) return fail(ZC_EINVAL, "bad argument");
    if (!n) return ZC_OK;
    zc::launch_traj_policy_append(n, *buf, *pol, d_root_na, d_root_moves, stride, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_traj_policy_commit_async(int32_t n, const zc_traj_buffers *buf, const zc_traj_policy_buffers *pol,
                                void *hip_stream) {
    if (int r = check_traj(n, buf, nullptr)) return r;
    if (int r = check_traj_policy(pol)) return r;
    if (!n) return ZC_OK;
    zc::launch_traj_policy_commit(n, *buf, *pol, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_traj_policy_steps_scratch_bytes(int32_t n, int32_t steps, int64_t *bytes) {
    if (n < 0 || steps < 0 || !bytes) return fail(ZC_EINVAL, "bad argument");
    *bytes = (int64_t)zc::traj_policy_steps_scratch_bytes(n, steps);
    return ZC_OK;
}

int zc_traj_policy_record_steps_async(int32_t n, const zc_traj_buffers *buf, const zc_traj_policy_buffers *pol,
                                      const int32_t *d_results, const int32_t *d_na, const uint16_t *d_root_moves,
                                      int32_t stride, int32_t steps, const int32_t *d_reached, void *d_scratch,
                                      int64_t scratch_bytes, void *hip_stream) {
    if (int r = check_traj(n, buf, nullptr)) return r;
    if (int r = check_traj_policy(pol)) return r;
    if (stride < 1 || stride > 65536) return fail(ZC_EINVAL, "stride must be in [1, 65536] (got %d)", stride);
    if (steps < 0) return fail(ZC_EINVAL, "steps must be >= 0 (got %d)", steps);
    if ((int64_t)n * steps >= ((int64_t)1 << 31)) return fail(ZC_EINVAL, "n x steps must be < 2^31");
    if (n && steps && (!d_results || !d_na)) return fail(ZC_EINVAL, "bad argument");
    if (!n || !steps) return ZC_OK;
    const size_t need = zc::traj_policy_steps_scratch_bytes(n, steps);
    if (!d_scratch || ((uintptr_t)d_scratch & 15) || scratch_bytes < (int64_t)need)
        return fail(ZC_EINVAL, "scratch: %lld bytes at %p, need %zu bytes 16-byte aligned", (long long)scratch_bytes,
                    d_scratch, need);
    zc::launch_traj_policy_record_steps(n, steps, *buf, *pol, d_results, d_na, d_root_moves, stride, d_reached,
                                        d_scratch, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_traj_policy_dense_async(int32_t n_rows, const int64_t *d_first, const int32_t *d_count,
                               const uint32_t *d_entries, int32_t width, int32_t dtype, void *d_out,
                               void *hip_stream) {
    if (width != 7 && width != 4096) return fail(ZC_EINVAL, "width must be 7 or 4096 (got %d)", width);
    if (dtype != ZC_F32 && dtype != ZC_F16) return fail(ZC_EINVAL, "dtype must be ZC_F32 or ZC_F16");
    if (n_rows < 0 || (n_rows && (!d_first || !d_count || !d_out))) return fail(ZC_EINVAL, "bad argument");
    if (width == 4096 && ((uintptr_t)d_out & 15)) return fail(ZC_EINVAL, "d_out must be 16-byte aligned");
    if (!n_rows) return ZC_OK;
    zc::launch_traj_policy_dense(n_rows, d_first, d_count, d_entries, width, dtype == ZC_F16, d_out,
                                 (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_planes_async(zc_engine *eng, int32_t n, const zc_chess_state *d_states, void *d_planes,
                          int32_t planes_dtype, void *hip_stream) {
    if (planes_dtype != ZC_F32 && planes_dtype != ZC_F16) return fail(ZC_EINVAL, "planes_dtype must be ZC_F32 or ZC_F16");
    ZC_CHESS_ENTRY(d_states && d_planes)
    zc::launch_chess_planes(n, d_states, d_planes, planes_dtype == ZC_F16, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}
#undef ZC_CHESS_ENTRY

// ---------------------------------------------------------------- chess tree search
}  // extern "C"

namespace {
int ensure_chess(zc_engine *e) {
    zc::ChessArena &c = e->ca;
    if (c.nodes) return ZC_OK;
    const size_t G = (size_t)e->cfg.max_games, M = (size_t)e->M;
    const size_t S = M * zc::kChessSlotsPerNode;
    zc::ChessArena n{};
    n.S = (int64_t)S;
    int rc = ZC_OK;
    if (!rc) rc = dalloc(e, &n.nodes, G * M);
    if (!rc) rc = dalloc(e, &n.mv, G * S);
    if (!rc) rc = dalloc(e, &n.ut, G * S);
    if (!rc) rc = dalloc(e, &n.ch, G * S);
    if (!rc) rc = dalloc(e, &n.na, G * S);
    if (!rc) rc = dalloc(e, &n.w, G * S);
    if (!rc) rc = dalloc(e, &n.prior, G * S);
    if (!rc) rc = dalloc(e, &n.ctl, G * zc::kCtlWords);
    if (!rc) rc = dalloc(e, &n.paths, G * (size_t)e->cfg.max_batch * zc::kChessPath);
    if (!rc) rc = dalloc(e, &n.meta, G * (size_t)e->cfg.max_batch);
    if (!rc) rc = dalloc(e, &n.roots, G);
    if (!rc) rc = dalloc(e, &n.xmv, G * (size_t)e->cfg.max_batch * ZC_CHESS_MAX_MOVES);
    if (!rc) rc = dalloc(e, &n.xinfo, G * (size_t)e->cfg.max_batch * 2);
    if (!rc && hipMemset(n.ctl, 0, G * zc::kCtlWords * sizeof(int32_t)) != hipSuccess) rc = fail(ZC_EHIP, "memset failed");
    if (rc) {
        free_chess(n);
        return rc;
    }
    c = n;
    return ZC_OK;
}

zc::ChessParams chess_params(zc_engine *e, int32_t first, int32_t n, int32_t sims, double c, int32_t bs, int32_t policy,
                             double freedom) {
    zc::ChessParams p{};
    p.first_game = first;
    p.n_games = n;
    p.sims = sims;
    p.bs = bs;
    p.M = e->M;
    p.max_batch = e->cfg.max_batch;
    p.c = c;
    p.policy = policy;
    p.freedom = freedom;
    static const double kCapVal[5] = {0.0, 1.0, 3.0, 5.0, 9.0};
    for (int i = 0; i < 5; ++i)
        for (int k = 0; k < 5; ++k)
            if (kCapVal[k] >= kCapVal[i] - freedom) p.cls_ok |= 1u << (5 * i + k);
    p.a = e->a;
    p.ca = e->ca;
    return p;
}

int check_chess(zc_engine *e, int32_t first, int32_t n, int32_t sims, double c, int32_t bs, int32_t policy,
                double freedom) {
    if (int r = check_search(e, first, n, sims, c, bs)) return r;
    if (policy != ZC_POLICY_RANDOM && policy != ZC_POLICY_IMMEDIATE_VALUE)
        return fail(ZC_EINVAL, "policy must be ZC_POLICY_RANDOM or ZC_POLICY_IMMEDIATE_VALUE");
    if (!isfinite(freedom)) return fail(ZC_EINVAL, "policy_freedom must be finite");
    return ZC_OK;
}

zc::ChessParams chess_value_params(zc_engine *e, int32_t first, int32_t n) {  // of the zc_chess_ext_* search
    const zc_engine::ChessValueSearch &s = e->chess_value;
    return chess_params(e, first, n, s.sims, s.c, s.bs, s.policy, s.freedom);
}
}  // namespace

extern "C" {

int zc_chess_reserve(zc_engine *eng) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    return ensure_chess(eng);
}

int zc_chess_search_async(zc_engine *eng, int32_t first, int32_t n, const zc_chess_state *d_roots, int32_t sims,
                          double c, int32_t bs, int32_t policy, double freedom, uint16_t *d_move, int32_t *d_na,
                          zc_game_stats *d_stats, void *hip_stream) {
    if (!eng || (n && (!d_roots || !d_move || !d_na || !d_stats))) return fail(ZC_EINVAL, "null argument");
    if (int r = check_chess(eng, first, n, sims, c, bs, policy, freedom)) return r;
    if (bs > 256) return fail(ZC_EINVAL, "batch_size %d > 256 (crude-score chess search)", bs);
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    if (int r = ensure_chess(eng)) return r;
    zc::ChessParams p = chess_params(eng, first, n, sims, c, bs, policy, freedom);
    p.roots = d_roots;
    p.out_move = d_move;
    p.out_na = d_na;
    p.out_stats = d_stats;
    zc::launch_chess_search(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

}  // extern "C"

namespace {
int check_play_buffers(int32_t n, const zc_chess_play_buffers *b) {
    if (!b) return fail(ZC_EINVAL, "null play buffers");
    if (n && (!b->d_roots || !b->d_init || !b->d_hist || !b->d_hist_len || !b->d_err))
        return fail(ZC_EINVAL, "null play buffer");
    if (b->hist_cap < 1 || b->hist_cap > 4096) return fail(ZC_EINVAL, "hist_cap %d outside [1, 4096]", b->hist_cap);
    return ZC_OK;
}
zc::ChessPlayParams play_params(const zc_chess_play_buffers *b) {
    zc::ChessPlayParams q{};
    q.roots = b->d_roots;
    q.init = b->d_init;
    q.hist = b->d_hist;
    q.hlen = b->d_hist_len;
    q.cap = b->hist_cap;
    q.err = b->d_err;
    return q;
}
int chess_selfplay_common(zc_engine *eng, int32_t first, int32_t n, const zc_chess_play_buffers *b, int32_t sims,
                          double c, int32_t bs, int32_t policy, double freedom, int32_t moves, int64_t budget,
                          int32_t *d_ticket, zc_chess_state *d_out_states, uint16_t *d_out_moves,
                          int32_t *d_out_results, zc_game_stats *d_stats, void *hip_stream) {
    if (!eng || (n && (!d_out_states || !d_out_moves || !d_out_results || !d_stats))) return fail(ZC_EINVAL, "null argument");
    if (int r = check_play_buffers(n, b)) return r;
    if (int r = check_chess(eng, first, n, sims, c, bs, policy, freedom)) return r;
    if (bs > 256) return fail(ZC_EINVAL, "batch_size %d > 256 (crude-score chess search)", bs);
    if (moves < 1) return fail(ZC_EINVAL, "moves must be >= 1 (got %d)", moves);
    if (d_ticket && (budget < 0 || budget > (int64_t)moves * n || budget >= ((int64_t)1 << 31)))
        return fail(ZC_EINVAL, "budget %lld outside [0, moves_cap x n_games] or >= 2^31", (long long)budget);
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_visits_cap("zc_chess_selfplay_visits", eng->chess_visits, eng->chess_visits_cap, moves)) return r;
    ZC_HIP(hipSetDevice(eng->cfg.device));
    if (int r = ensure_chess(eng)) return r;
    hipStream_t s = (hipStream_t)hip_stream;
    if (d_ticket) {
        int resident = 0;
        if (zc::chess_selfplay_resident_games(b->hist_cap, &resident)) return fail(ZC_EHIP, "occupancy query failed");
        if (n > resident)
            return fail(ZC_EINVAL, "pooled chess self-play of %d games: at most %d are resident at once", n, resident);
        ZC_HIP(hipMemsetAsync(d_ticket, 0, 2 * sizeof(int32_t), s));
    }
    zc::ChessParams p = chess_params(eng, first, n, sims, c, bs, policy, freedom);
    p.roots = b->d_roots;
    zc::ChessPlayParams q = play_params(b);
    q.out_states = d_out_states;
    q.out_moves = d_out_moves;
    q.out_results = d_out_results;
    q.moves = moves;
    q.ticket = d_ticket;
    q.budget = (int32_t)budget;
    q.stats = d_stats;
    q.out_step_na = eng->chess_visits;
    q.out_step_moves = eng->chess_visit_moves;
    zc::launch_chess_selfplay(p, q, s);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}
}  // namespace

extern "C" {

int zc_chess_play_step_async(int32_t n, const zc_chess_play_buffers *b, const uint16_t *d_moves,
                             const zc_game_stats *d_search_stats, zc_chess_state *d_out_states,
                             int32_t *d_out_results, void *hip_stream) {
    if (n < 0 || (n && (!d_moves || !d_out_states || !d_out_results))) return fail(ZC_EINVAL, "bad argument");
    if (int r = check_play_buffers(n, b)) return r;
    if (!n) return ZC_OK;
    zc::ChessPlayParams q = play_params(b);
    q.in_moves = d_moves;
    q.search_stats = d_search_stats;
    q.out_states = d_out_states;
    q.out_results = d_out_results;
    zc::launch_chess_play_step(q, n, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_selfplay_async(zc_engine *eng, int32_t first, int32_t n, const zc_chess_play_buffers *b, int32_t sims,
                            double c, int32_t bs, int32_t policy, double freedom, int32_t moves,
                            zc_chess_state *d_out_states, uint16_t *d_out_moves, int32_t *d_out_results,
                            zc_game_stats *d_stats, void *hip_stream) {
    return chess_selfplay_common(eng, first, n, b, sims, c, bs, policy, freedom, moves, 0, nullptr, d_out_states,
                                 d_out_moves, d_out_results, d_stats, hip_stream);
}

int zc_chess_selfplay_pooled_async(zc_engine *eng, int32_t first, int32_t n, const zc_chess_play_buffers *b,
                                   int32_t sims, double c, int32_t bs, int32_t policy, double freedom,
                                   int32_t moves_cap, int64_t budget, int32_t *d_ticket, zc_chess_state *d_out_states,
                                   uint16_t *d_out_moves, int32_t *d_out_results, zc_game_stats *d_stats,
                                   void *hip_stream) {
    if (n && !d_ticket) return fail(ZC_EINVAL, "null argument");
    return chess_selfplay_common(eng, first, n, b, sims, c, bs, policy, freedom, moves_cap, budget, d_ticket,
                                 d_out_states, d_out_moves, d_out_results, d_stats, hip_stream);
}

int zc_chess_selfplay_visits(zc_engine *eng, int32_t *d_na, uint16_t *d_root_moves, int32_t steps_cap) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    if (d_na && (!d_root_moves || steps_cap < 1))
        return fail(ZC_EINVAL, "the staging needs d_root_moves and steps_cap >= 1 (got %d)", steps_cap);
    std::lock_guard<std::mutex> lk(eng->mu);
    eng->chess_visits = d_na;
    eng->chess_visit_moves = d_na ? d_root_moves : nullptr;
    eng->chess_visits_cap = d_na ? steps_cap : 0;
    return ZC_OK;
}

int zc_chess_pooled_max_games(int32_t hist_cap, int32_t *out) {
    if (!out || hist_cap < 1 || hist_cap > 4096) return fail(ZC_EINVAL, "bad argument");
    int r = 0;
    if (zc::chess_selfplay_resident_games(hist_cap, &r)) return fail(ZC_EHIP, "occupancy query failed");
    *out = r;
    return ZC_OK;
}

int zc_chess_ext_begin(zc_engine *eng, int32_t first, int32_t n, const zc_chess_state *d_roots, int32_t sims, double c,
                       int32_t bs, int32_t policy, double freedom, void *hip_stream) {
    if (!eng || (n && !d_roots)) return fail(ZC_EINVAL, "null argument");
    if (int r = check_chess(eng, first, n, sims, c, bs, policy, freedom)) return r;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    if (int r = ensure_chess(eng)) return r;
    set_step(eng->chess_value, first, n, sims, c, bs, value_flushes(sims, bs));
    eng->chess_value.policy = policy;
    eng->chess_value.freedom = freedom;
    if (!n) return ZC_OK;
    zc::ChessParams p = chess_value_params(eng, first, n);
    p.roots = d_roots;
    zc::launch_chess_ext_begin(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_ext_select(zc_engine *eng, int32_t first, int32_t n, int32_t flush, zc_chess_state *d_leaves,
                        void *d_planes, int32_t planes_dtype, int32_t *d_counts, void *hip_stream) {
    if (int r = check_planes_dtype(planes_dtype)) return r;
    ZC_STEP_ENTRY(eng->chess_value, flush, true, true)
    zc::ChessParams p = chess_value_params(eng, first, n);
    p.flush = flush;
    p.leaves = d_leaves;
    p.planes = d_planes;
    p.planes_f16 = planes_dtype == ZC_F16;
    p.counts = d_counts;
    zc::launch_chess_ext_select(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_ext_backup(zc_engine *eng, int32_t first, int32_t n, int32_t flush, const double *d_values,
                        void *hip_stream) {
    ZC_STEP_ENTRY(eng->chess_value, flush, true, d_values)
    zc::ChessParams p = chess_value_params(eng, first, n);
    p.flush = flush;
    p.values = d_values;
    zc::launch_chess_ext_backup(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_ext_end(zc_engine *eng, int32_t first, int32_t n, uint16_t *d_move, int32_t *d_na, zc_game_stats *d_stats,
                     void *hip_stream) {
    ZC_STEP_ENTRY(eng->chess_value, 0, false, d_move && d_na && d_stats)
    zc::ChessParams p = chess_value_params(eng, first, n);
    p.out_move = d_move;
    p.out_na = d_na;
    p.out_stats = d_stats;
    zc::launch_chess_ext_end(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_hp_walk(zc_engine *eng, int32_t game, int32_t flush, int32_t leaf, zc_chess_hp_node *d_node,
                     void *hip_stream) {
    if (!eng || !d_node) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_hp(eng->chess_value, game, flush, leaf)) return r;
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::ChessParams p = chess_value_params(eng, game, 1);
    p.flush = flush;
    p.hp_leaf = leaf;
    p.hp_node = d_node;
    zc::launch_chess_hp_walk(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_hp_expand(zc_engine *eng, int32_t game, int32_t flush, int32_t leaf, int32_t untried_index,
                       zc_chess_state *d_leaf, void *hip_stream) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_hp(eng->chess_value, game, flush, leaf)) return r;
    if (untried_index < -1 || untried_index >= ZC_CHESS_MAX_MOVES)
        return fail(ZC_EINVAL, "untried index %d outside [-1, %d)", untried_index, ZC_CHESS_MAX_MOVES);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::ChessParams p = chess_value_params(eng, game, 1);
    p.flush = flush;
    p.hp_leaf = leaf;
    p.hp_index = untried_index;
    p.leaves = d_leaf;
    zc::launch_chess_hp_expand(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_rollouts_async(zc_engine *eng, int32_t game, int32_t n_states, const zc_chess_state *d_states,
                            const uint16_t *d_hist, const int32_t *d_hist_len, int32_t hist_cap, double *d_values,
                            int32_t *d_status, void *hip_stream) {
    if (!eng || (n_states && (!d_states || !d_hist || !d_hist_len || !d_values))) return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, game, 1)) return r;
    if (n_states < 0 || hist_cap < 1) return fail(ZC_EINVAL, "n_states must be >= 0 and hist_cap >= 1");
    if (!n_states) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    if (int r = ensure_chess(eng)) return r;
    zc::ChessParams p = chess_params(eng, game, 1, 1, 1.0, 1, 0, 0.0);
    p.rstates = d_states;
    p.n_states = n_states;
    p.rhist = d_hist;
    p.rhlen = d_hist_len;
    p.rhcap = hist_cap;
    p.rvalues = d_values;
    p.rstatus = d_status;
    zc::launch_chess_rollouts(p, false, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_ext_rollouts(zc_engine *eng, int32_t first, int32_t n, int32_t flush, const uint16_t *d_hist,
                          const int32_t *d_hist_len, int32_t hist_cap, double *d_values, int32_t *d_status,
                          void *hip_stream) {
    if (hist_cap < 1) return fail(ZC_EINVAL, "hist_cap must be >= 1");
    ZC_STEP_ENTRY(eng->chess_value, flush, true, d_hist && d_hist_len && d_values)
    zc::ChessParams p = chess_value_params(eng, first, n);
    p.flush = flush;
    p.rhist = d_hist;
    p.rhlen = d_hist_len;
    p.rhcap = hist_cap;
    p.rvalues = d_values;
    p.rstatus = d_status;
    zc::launch_chess_rollouts(p, true, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_ext_leaf_moves(zc_engine *eng, int32_t first, int32_t n, int32_t flush, uint16_t *d_moves,
                            int32_t *d_depth, void *hip_stream) {
    ZC_STEP_ENTRY(eng->chess_value, flush, true, d_moves && d_depth)
    zc::ChessParams p = chess_value_params(eng, first, n);
    p.flush = flush;
    p.path_moves = d_moves;
    p.path_depth = d_depth;
    zc::launch_chess_leaf_moves(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

// ---------------------------------------------------------------- PUCT searches (chess, Connect4)
int zc_chess_puct_flushes(int32_t sims, int32_t bs) {
    if (sims < 2 || bs < 1) return fail(ZC_EINVAL, "PUCT search needs sims >= 2 and batch_size >= 1");
    return puct_flushes(sims, bs);
}

}  // extern "C"

namespace {
int ensure_c4p(zc_engine *e) {
    if (e->c4p.nodes) return ZC_OK;
    const size_t G = (size_t)e->cfg.max_games, M = (size_t)e->M;
    zc::C4PuctArena n{};
    int rc = dalloc(e, &n.nodes, G * M);
    if (!rc) rc = dalloc(e, &n.ctl, G * zc::kCtlWords);
    if (!rc) rc = dalloc(e, &n.paths, G * (size_t)e->cfg.max_batch * zc::kMaxDepth);
    if (!rc) rc = dalloc(e, &n.meta, G * (size_t)e->cfg.max_batch);
    if (!rc && hipMemset(n.ctl, 0, G * zc::kCtlWords * sizeof(int32_t)) != hipSuccess) rc = fail(ZC_EHIP, "memset failed");
    if (rc) {
        free_c4p(n);
        return rc;
    }
    e->c4p = n;
    return ZC_OK;
}

// d_search_no is indexed by game - first_game of the begin call; a launch over a sub-range
// [first, first + n) indexes it from its own first game
int32_t *search_no_at(const PuctSearch &s, int32_t first) {
    return s.search_no ? s.search_no + (first - s.first) : nullptr;
}

// The two games of the PUCT search, as the steps below need them: the engine's record of the
// search, the arena (`ensure`: with the re-root's scratch for a begin_reuse), the kernel
// parameters of a step over games [first, first + n), the planes formats of select
// (ZC_EINVAL, or the kernel's code in *fmt) and the launchers.
struct ChessPuct {
    using State = zc_chess_state;
    using Move = uint16_t;
    static PuctSearch &search(zc_engine *e) { return e->chess_puct; }
    static bool has_tree(const zc_engine *e) { return e->ca.nodes != nullptr; }
    static int ensure(zc_engine *e, bool reuse) {
        if (int r = ensure_chess(e)) return r;
        const size_t GM = (size_t)e->cfg.max_games * (size_t)e->M;
        if (reuse && !e->ca.remap)
            if (int r = dalloc(e, &e->ca.remap, GM)) return r;
        if (reuse && !e->ca.rbase)
            if (int r = dalloc(e, &e->ca.rbase, GM)) return r;
        return ZC_OK;
    }
    static zc::ChessParams params(zc_engine *e, int32_t first, int32_t n) {
        const PuctSearch &s = e->chess_puct;
        zc::ChessParams p = chess_params(e, first, n, s.sims, s.c, s.bs, 0, 0.0);
        p.dir_alpha = s.alpha;
        p.dir_eps = s.eps;
        p.seed = s.seed;
        p.search_no = search_no_at(s, first);
        return p;
    }
    static int planes_format(int32_t dtype, int *fmt) {
        if (dtype != ZC_F32 && dtype != ZC_F16 && dtype != ZC_F16_NHWC32)
            return fail(ZC_EINVAL, "planes_dtype must be ZC_F32, ZC_F16 or ZC_F16_NHWC32");
        *fmt = dtype == ZC_F16 ? 1 : dtype == ZC_F16_NHWC32 ? 2 : 0;
        return ZC_OK;
    }
    static constexpr auto begin = zc::launch_chess_puct_begin, reroot = zc::launch_chess_puct_reroot,
                          forget = zc::launch_chess_puct_forget, select = zc::launch_chess_puct_select,
                          backup = zc::launch_chess_puct_backup, end = zc::launch_chess_puct_end;
    static constexpr auto forget_fresh = zc::launch_chess_puct_forget_fresh;
};

struct C4Puct {
    using State = zc_c4_state;
    using Move = int32_t;
    static PuctSearch &search(zc_engine *e) { return e->c4_puct; }
    static bool has_tree(const zc_engine *e) { return e->c4p.nodes != nullptr; }
    static int ensure(zc_engine *e, bool reuse) {
        if (int r = ensure_c4p(e)) return r;
        if (reuse && !e->c4p.remap) return dalloc(e, &e->c4p.remap, (size_t)e->cfg.max_games * (size_t)e->M);
        return ZC_OK;
    }
    static zc::C4PuctParams params(zc_engine *e, int32_t first, int32_t n) {
        const PuctSearch &s = e->c4_puct;
        zc::C4PuctParams p{};
        p.first_game = first;
        p.n_games = n;
        p.sims = s.sims;
        p.bs = s.bs;
        p.M = e->M;
        p.max_batch = e->cfg.max_batch;
        p.c = s.c;
        p.nodes = e->c4p.nodes;
        p.ctl = e->c4p.ctl;
        p.paths = e->c4p.paths;
        p.meta = e->c4p.meta;
        p.remap = e->c4p.remap;
        p.dir_alpha = s.alpha;
        p.dir_eps = s.eps;
        p.seed = s.seed;
        p.search_no = search_no_at(s, first);
        return p;
    }
    static int planes_format(int32_t dtype, int *fmt) {
        *fmt = dtype == ZC_F16;
        return check_planes_dtype(dtype);
    }
    static constexpr auto begin = zc::launch_c4_puct_begin, reroot = zc::launch_c4_puct_reroot,
                          forget = zc::launch_c4_puct_forget, select = zc::launch_c4_puct_select,
                          backup = zc::launch_c4_puct_backup, end = zc::launch_c4_puct_end;
    static constexpr auto forget_fresh = zc::launch_c4_puct_forget_fresh;
};

// begin / begin_reuse: the same validation and search parameters; the reuse form launches the
// re-root kernel in place of the begin kernel.  The search is recorded once its arena exists.
template <class G>
int puct_begin(zc_engine *eng, int32_t first, int32_t n, const typename G::State *d_roots, int32_t sims, double c_puct,
               int32_t bs, float alpha, float eps, uint64_t seed, int32_t *d_search_no, bool reuse, int32_t *d_kept,
               void *hip_stream) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    if (n && !d_roots) return fail(ZC_EINVAL, "null argument");
    if (int r = check_search(eng, first, n, sims, c_puct, bs)) return r;
    if (sims < 2) return fail(ZC_EINVAL, "PUCT search needs sims >= 2 (flush 0 evaluates the root)");
    if (!(alpha > 0.0f) || !(eps >= 0.0f && eps <= 1.0f)) return fail(ZC_EINVAL, "need alpha > 0 and 0 <= eps <= 1");
    ZC_HIP(hipSetDevice(eng->cfg.device));
    if (int r = G::ensure(eng, reuse)) return r;
    PuctSearch &s = G::search(eng);
    set_step(s, first, n, sims, c_puct, bs, puct_flushes(sims, bs));
    s.alpha = alpha;
    s.eps = eps;
    s.seed = seed;
    s.search_no = d_search_no;
    if (!n) return ZC_OK;
    auto p = G::params(eng, first, n);
    p.roots = d_roots;
    p.out_kept = reuse ? d_kept : nullptr;
    (reuse ? G::reroot : G::begin)(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

template <class G>
int puct_forget(zc_engine *eng, int32_t first, int32_t n, void *hip_stream) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, first, n)) return r;
    std::lock_guard<std::mutex> lk(eng->mu);
    if (!n || !G::has_tree(eng)) return ZC_OK;  // no tree yet: nothing is kept
    ZC_HIP(hipSetDevice(eng->cfg.device));
    G::forget(G::params(eng, first, n), (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

template <class G>
int puct_forget_fresh(zc_engine *eng, int32_t first, int32_t n, const int32_t *d_slot, void *hip_stream) {
    if (!eng || (n > 0 && !d_slot)) return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, first, n)) return r;
    std::lock_guard<std::mutex> lk(eng->mu);
    if (!n || !G::has_tree(eng)) return ZC_OK;  // no tree yet: nothing is kept
    ZC_HIP(hipSetDevice(eng->cfg.device));
    G::forget_fresh(G::params(eng, first, n), d_slot, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

template <class G>
int puct_select(zc_engine *eng, int32_t first, int32_t n, int32_t flush, typename G::State *d_leaves, void *d_planes,
                int32_t planes_dtype, int32_t *d_counts, void *hip_stream) {
    int fmt = 0;
    if (int r = G::planes_format(planes_dtype, &fmt)) return r;
    ZC_STEP_ENTRY(G::search(eng), flush, true, true)
    auto p = G::params(eng, first, n);
    p.flush = flush;
    p.leaves = d_leaves;
    p.planes = d_planes;
    p.planes_f16 = fmt;
    p.counts = d_counts;
    G::select(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

template <class G>
int puct_backup(zc_engine *eng, int32_t first, int32_t n, int32_t flush, const double *d_values, const void *d_logits,
                int32_t logits_dtype, int32_t rows_per_game, void *hip_stream) {
    if (logits_dtype != ZC_F32 && logits_dtype != ZC_F16) return fail(ZC_EINVAL, "logits_dtype must be ZC_F32 or ZC_F16");
    if (rows_per_game < 0 || (rows_per_game > 0 && flush != 0))
        return fail(ZC_EINVAL, "rows_per_game must be 0 (batch_size rows), or >= 1 for flush 0 (the roots)");
    ZC_STEP_ENTRY(G::search(eng), flush, true, d_values && d_logits)
    auto p = G::params(eng, first, n);
    p.flush = flush;
    p.values = d_values;
    p.logits = d_logits;
    p.logits_f16 = logits_dtype == ZC_F16;
    p.leaf_rows = rows_per_game;
    G::backup(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

template <class G>
int puct_end(zc_engine *eng, int32_t first, int32_t n, float temperature, typename G::Move *d_move, int32_t *d_na,
             float *d_prior, zc_game_stats *d_stats, void *hip_stream) {
    if (!(temperature >= 0.0f)) return fail(ZC_EINVAL, "temperature must be >= 0");
    ZC_STEP_ENTRY(G::search(eng), 0, false, d_move && d_na && d_stats)
    auto p = G::params(eng, first, n);
    p.temperature = temperature;
    p.out_move = d_move;
    p.out_na = d_na;
    p.out_prior = d_prior;
    p.out_stats = d_stats;
    G::end(p, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}
}  // namespace

extern "C" {

int zc_chess_puct_begin(zc_engine *eng, int32_t first, int32_t n, const zc_chess_state *d_roots, int32_t sims,
                        double c_puct, int32_t bs, float alpha, float eps, uint64_t seed, int32_t *d_search_no,
                        void *hip_stream) {
    return puct_begin<ChessPuct>(eng, first, n, d_roots, sims, c_puct, bs, alpha, eps, seed, d_search_no, false,
                                 nullptr, hip_stream);
}
int zc_chess_puct_begin_reuse(zc_engine *eng, int32_t first, int32_t n, const zc_chess_state *d_roots, int32_t sims,
                              double c_puct, int32_t bs, float alpha, float eps, uint64_t seed, int32_t *d_search_no,
                              int32_t *d_kept, void *hip_stream) {
    return puct_begin<ChessPuct>(eng, first, n, d_roots, sims, c_puct, bs, alpha, eps, seed, d_search_no, true, d_kept,
                                 hip_stream);
}
int zc_chess_puct_forget(zc_engine *eng, int32_t first, int32_t n, void *hip_stream) {
    return puct_forget<ChessPuct>(eng, first, n, hip_stream);
}
int zc_chess_puct_forget_fresh(zc_engine *eng, int32_t first, int32_t n, const int32_t *d_slot, void *hip_stream) {
    return puct_forget_fresh<ChessPuct>(eng, first, n, d_slot, hip_stream);
}
int zc_chess_puct_select(zc_engine *eng, int32_t first, int32_t n, int32_t flush, zc_chess_state *d_leaves,
                         void *d_planes, int32_t planes_dtype, int32_t *d_counts, void *hip_stream) {
    return puct_select<ChessPuct>(eng, first, n, flush, d_leaves, d_planes, planes_dtype, d_counts, hip_stream);
}
int zc_chess_puct_backup_ex(zc_engine *eng, int32_t first, int32_t n, int32_t flush, const double *d_values,
                            const void *d_logits, int32_t logits_dtype, int32_t rows_per_game, void *hip_stream) {
    return puct_backup<ChessPuct>(eng, first, n, flush, d_values, d_logits, logits_dtype, rows_per_game, hip_stream);
}
int zc_chess_puct_backup(zc_engine *eng, int32_t first, int32_t n, int32_t flush, const double *d_values,
                         const void *d_logits, int32_t logits_dtype, void *hip_stream) {
    return puct_backup<ChessPuct>(eng, first, n, flush, d_values, d_logits, logits_dtype, 0, hip_stream);
}
int zc_chess_puct_end(zc_engine *eng, int32_t first, int32_t n, float temperature, uint16_t *d_move, int32_t *d_na,
                      float *d_prior, zc_game_stats *d_stats, void *hip_stream) {
    return puct_end<ChessPuct>(eng, first, n, temperature, d_move, d_na, d_prior, d_stats, hip_stream);
}

int zc_c4_puct_begin(zc_engine *eng, int32_t first, int32_t n, const zc_c4_state *d_roots, int32_t sims,
                     double c_puct, int32_t bs, float alpha, float eps, uint64_t seed, int32_t *d_search_no,
                     void *hip_stream) {
    return puct_begin<C4Puct>(eng, first, n, d_roots, sims, c_puct, bs, alpha, eps, seed, d_search_no, false, nullptr,
                              hip_stream);
}
int zc_c4_puct_begin_reuse(zc_engine *eng, int32_t first, int32_t n, const zc_c4_state *d_roots, int32_t sims,
                           double c_puct, int32_t bs, float alpha, float eps, uint64_t seed, int32_t *d_search_no,
                           int32_t *d_kept, void *hip_stream) {
    return puct_begin<C4Puct>(eng, first, n, d_roots, sims, c_puct, bs, alpha, eps, seed, d_search_no, true, d_kept,
                              hip_stream);
}
int zc_c4_puct_forget(zc_engine *eng, int32_t first, int32_t n, void *hip_stream) {
    return puct_forget<C4Puct>(eng, first, n, hip_stream);
}
int zc_c4_puct_forget_fresh(zc_engine *eng, int32_t first, int32_t n, const int32_t *d_slot, void *hip_stream) {
    return puct_forget_fresh<C4Puct>(eng, first, n, d_slot, hip_stream);
}
int zc_c4_puct_select(zc_engine *eng, int32_t first, int32_t n, int32_t flush, zc_c4_state *d_leaves, void *d_planes,
                      int32_t planes_dtype, int32_t *d_counts, void *hip_stream) {
    return puct_select<C4Puct>(eng, first, n, flush, d_leaves, d_planes, planes_dtype, d_counts, hip_stream);
}
int zc_c4_puct_backup_ex(zc_engine *eng, int32_t first, int32_t n, int32_t flush, const double *d_values,
                         const void *d_logits, int32_t logits_dtype, int32_t rows_per_game, void *hip_stream) {
    return puct_backup<C4Puct>(eng, first, n, flush, d_values, d_logits, logits_dtype, rows_per_game, hip_stream);
}
int zc_c4_puct_backup(zc_engine *eng, int32_t first, int32_t n, int32_t flush, const double *d_values,
                      const void *d_logits, int32_t logits_dtype, void *hip_stream) {
    return puct_backup<C4Puct>(eng, first, n, flush, d_values, d_logits, logits_dtype, 0, hip_stream);
}
int zc_c4_puct_end(zc_engine *eng, int32_t first, int32_t n, float temperature, int32_t *d_move, int32_t *d_na,
                   float *d_prior, zc_game_stats *d_stats, void *hip_stream) {
    return puct_end<C4Puct>(eng, first, n, temperature, d_move, d_na, d_prior, d_stats, hip_stream);
}
#undef ZC_STEP_ENTRY

int zc_debug_c4_puct_tree(zc_engine *eng, int32_t game, int32_t max_nodes, void *out_nodes, int32_t *out_count) {
    if (!eng || !out_nodes || !out_count) return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, game, 1)) return r;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    const zc::C4PuctArena &c = eng->c4p;
    if (!c.nodes) return fail(ZC_EINVAL, "no Connect4 PUCT tree (no PUCT search has run)");
    ZC_HIP(hipDeviceSynchronize());
    int32_t nn = 0;
    ZC_HIP(hipMemcpy(&nn, c.ctl + (size_t)game * zc::kCtlWords, sizeof nn, hipMemcpyDeviceToHost));
    if (nn > max_nodes) return fail(ZC_ECAPACITY, "tree has %d nodes (buffer: %d)", nn, max_nodes);
    ZC_HIP(hipMemcpy(out_nodes, c.nodes + (size_t)game * eng->M, (size_t)nn * sizeof(zc::C4PNode),
                     hipMemcpyDeviceToHost));
    *out_count = nn;
    return ZC_OK;
}

int zc_debug_chess_tree(zc_engine *eng, int32_t game, int32_t max_nodes, int32_t max_slots, void *out_nodes,
                        uint16_t *out_mv, float *out_prior, int32_t *out_na, double *out_w, uint16_t *out_child,
                        int32_t *out_counts) {
    if (!eng || !out_nodes || !out_mv || !out_prior || !out_na || !out_w || !out_child || !out_counts)
        return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, game, 1)) return r;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    const zc::ChessArena &c = eng->ca;
    if (!c.nodes) return fail(ZC_EINVAL, "no chess tree (no chess search has run)");
    ZC_HIP(hipStreamSynchronize(nullptr));
    ZC_HIP(hipDeviceSynchronize());
    int32_t ctl[2];  // per-game control words 0, 1: nodes, slots used
    ZC_HIP(hipMemcpy(ctl, c.ctl + (size_t)game * zc::kCtlWords, sizeof ctl, hipMemcpyDeviceToHost));
    if (ctl[0] > max_nodes || ctl[1] > max_slots)
        return fail(ZC_ECAPACITY, "tree has %d nodes / %d slots (buffers: %d / %d)", ctl[0], ctl[1], max_nodes, max_slots);
    const size_t no = (size_t)game * eng->M, so = (size_t)game * (size_t)c.S;
    ZC_HIP(hipMemcpy(out_nodes, c.nodes + no, (size_t)ctl[0] * sizeof(zc::ChessNode), hipMemcpyDeviceToHost));
    ZC_HIP(hipMemcpy(out_mv, c.mv + so, (size_t)ctl[1] * sizeof(uint16_t), hipMemcpyDeviceToHost));
    ZC_HIP(hipMemcpy(out_prior, c.prior + so, (size_t)ctl[1] * sizeof(float), hipMemcpyDeviceToHost));
    ZC_HIP(hipMemcpy(out_na, c.na + so, (size_t)ctl[1] * sizeof(int32_t), hipMemcpyDeviceToHost));
    ZC_HIP(hipMemcpy(out_w, c.w + so, (size_t)ctl[1] * sizeof(double), hipMemcpyDeviceToHost));
    ZC_HIP(hipMemcpy(out_child, c.ch + so, (size_t)ctl[1] * sizeof(uint16_t), hipMemcpyDeviceToHost));
    out_counts[0] = ctl[0];
    out_counts[1] = ctl[1];
    return ZC_OK;
}

// ---------------------------------------------------------------- value-network layers
int zc_net_conv3x3_async(int32_t n, int32_t h, int32_t w, int32_t cin, const void *d_in, const void *d_weight,
                         const float *d_bias, const void *d_residual, void *d_out, int32_t relu, void *hip_stream) {
    if (n < 0 || (n && (!d_in || !d_weight || !d_bias || !d_out))) return fail(ZC_EINVAL, "bad argument");
    if (!n) return ZC_OK;
    if (!zc::launch_net_conv3x3(n, h, w, cin, d_in, d_weight, d_bias, d_residual, d_out, relu ? 1 : 0,
                                (hipStream_t)hip_stream))
        return fail(ZC_EINVAL, "conv3x3 shape (h %d, w %d, cin %d) not supported", h, w, cin);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_net_conv3x3_pack_async(int32_t cin, const void *d_weight, void *d_packed, void *hip_stream) {
    if (!d_weight || !d_packed || ((uintptr_t)d_weight & 15) || ((uintptr_t)d_packed & 15))
        return fail(ZC_EINVAL, "bad argument");
    if (!zc::launch_net_pack_conv_weight(cin, d_weight, d_packed, (hipStream_t)hip_stream))
        return fail(ZC_EINVAL, "conv3x3 pack: cin %d not supported", cin);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_net_conv3x3_packed_async(int32_t n, int32_t h, int32_t w, int32_t cin, const void *d_in, const void *d_packed,
                                const float *d_bias, const void *d_residual, void *d_out, int32_t relu,
                                void *hip_stream) {
    if (n < 0 || (n && (!d_in || !d_packed || !d_bias || !d_out)) || ((uintptr_t)d_packed & 15))
        return fail(ZC_EINVAL, "bad argument");
    if (!n) return ZC_OK;
    if (!zc::launch_net_conv3x3_packed(n, h, w, cin, d_in, d_packed, d_bias, d_residual, d_out, relu ? 1 : 0,
                                       (hipStream_t)hip_stream))
        return fail(ZC_EINVAL, "conv3x3 shape (h %d, w %d, cin %d) not supported", h, w, cin);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

// The five tower entry points: the checks, then launch_net_tower.  policy: the forms with a policy
// head, which need it and the value head whole (d_out: none); the others need d_out or d_values,
// and d_fc_w with d_values.  ex: the forms that take policy_channels (32 or 64) and relu, and read
// d_pb 16 bytes at a time.  counted: the forms that take their row count from d_count.  channels:
// 128 (the entry points above the _w_ family) or 64 (net_conv64.hip), checked by the caller.
static int net_tower(int32_t channels, bool policy, bool ex, bool counted, int32_t n, int32_t h, int32_t w,
                     int32_t cin0, int32_t nconv, const void *d_in, const void *d_packed, const float *d_bias, void *d_out, const float *d_fc_w,
                     float fc_b, double *d_values, const void *d_pw, const float *d_pb, int32_t policy_channels,
                     int32_t relu, void *d_pout, const int32_t *d_count, void *hip_stream) {
    bool ok = n >= 0 && !(((uintptr_t)d_packed | (uintptr_t)d_in | (uintptr_t)d_bias) & 15) &&
              (!n || (d_in && d_packed && d_bias));
    if (policy)
        ok = ok && !((uintptr_t)d_pw & 15) && !((uintptr_t)d_pout & 7) &&
             (!n || (d_fc_w && d_values && d_pw && d_pb && d_pout));
    else
        ok = ok && !((uintptr_t)d_out & 15) && (!n || ((d_out || d_values) && (d_fc_w || !d_values)));
    if (ex) ok = ok && !((uintptr_t)d_pb & 15) && (policy_channels == 32 || policy_channels == 64);
    if (counted) ok = ok && d_count && !((uintptr_t)d_count & 3);
    if (!ok) return fail(ZC_EINVAL, "bad argument");
    if (!n) return ZC_OK;
    if (channels == 64) {
        if (!zc::launch_net64_tower(n, h, w, cin0, nconv, d_in, d_packed, d_bias, d_out, d_values ? d_fc_w : nullptr,
                                    fc_b, d_values, d_pw, d_pb, d_pout, (hipStream_t)hip_stream, policy_channels, relu,
                                    d_count))
            return fail(ZC_EINVAL, "64-channel tower shape (h %d, w %d, cin0 %d, %d convs) not supported", h, w, cin0,
                        nconv);
        ZC_HIP(hipGetLastError());
        return ZC_OK;
    }
    if (!zc::launch_net_tower(n, h, w, cin0, nconv, d_in, d_packed, d_bias, d_out, d_values ? d_fc_w : nullptr, fc_b,
                              d_values, d_pw, d_pb, d_pout, (hipStream_t)hip_stream, policy_channels, relu, d_count))
        return fail(ZC_EINVAL, "tower shape (h %d, w %d, cin0 %d, %d convs) not supported", h, w, cin0, nconv);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_net_tower_async(int32_t n, int32_t h, int32_t w, int32_t cin0, int32_t nconv, const void *d_in,
                       const void *d_packed, const float *d_bias, void *d_out, const float *d_fc_w, float fc_b,
                       double *d_values, void *hip_stream) {
    return net_tower(128, false, false, false, n, h, w, cin0, nconv, d_in, d_packed, d_bias, d_out, d_fc_w, fc_b, d_values,
                     nullptr, nullptr, 32, 1, nullptr, nullptr, hip_stream);
}

int zc_net_tower_policy_async(int32_t n, int32_t h, int32_t w, int32_t cin0, int32_t nconv, const void *d_in,
                              const void *d_packed, const float *d_bias, const float *d_fc_w, float fc_b,
                              double *d_values, const void *d_pw, const float *d_pb, void *d_pout, void *hip_stream) {
    return net_tower(128, true, false, false, n, h, w, cin0, nconv, d_in, d_packed, d_bias, nullptr, d_fc_w, fc_b, d_values,
                     d_pw, d_pb, 32, 1, d_pout, nullptr, hip_stream);
}

int zc_net_tower_policy_ex_async(int32_t n, int32_t h, int32_t w, int32_t cin0, int32_t nconv, const void *d_in,
                                 const void *d_packed, const float *d_bias, const float *d_fc_w, float fc_b,
                                 double *d_values, const void *d_pw, const float *d_pb, int32_t policy_channels,
                                 int32_t relu, void *d_pout, void *hip_stream) {
    return net_tower(128, true, true, false, n, h, w, cin0, nconv, d_in, d_packed, d_bias, nullptr, d_fc_w, fc_b, d_values,
                     d_pw, d_pb, policy_channels, relu, d_pout, nullptr, hip_stream);
}

int zc_net_tower_counted_async(int32_t n, int32_t h, int32_t w, int32_t cin0, int32_t nconv, const void *d_in,
                               const void *d_packed, const float *d_bias, void *d_out, const float *d_fc_w, float fc_b,
                               double *d_values, const int32_t *d_count, void *hip_stream) {
    return net_tower(128, false, false, true, n, h, w, cin0, nconv, d_in, d_packed, d_bias, d_out, d_fc_w, fc_b, d_values,
                     nullptr, nullptr, 32, 1, nullptr, d_count, hip_stream);
}

int zc_net_tower_policy_counted_async(int32_t n, int32_t h, int32_t w, int32_t cin0, int32_t nconv, const void *d_in,
                                      const void *d_packed, const float *d_bias, const float *d_fc_w, float fc_b,
                                      double *d_values, const void *d_pw, const float *d_pb, int32_t policy_channels,
                                      int32_t relu, void *d_pout, const int32_t *d_count, void *hip_stream) {
    return net_tower(128, true, true, true, n, h, w, cin0, nconv, d_in, d_packed, d_bias, nullptr, d_fc_w, fc_b, d_values,
                     d_pw, d_pb, policy_channels, relu, d_pout, d_count, hip_stream);
}

int zc_net_planes_to_nhwc_async(int32_t n, int32_t cin, int32_t hw, int32_t cpad, const void *d_planes, void *d_out,
                                void *hip_stream) {
    if (n < 0 || cin < 1 || hw < 1 || cpad < cin || (cpad & 7) || ((uintptr_t)d_out & 15) ||
        (n && (!d_planes || !d_out)))
        return fail(ZC_EINVAL, "bad argument");
    if (!n) return ZC_OK;
    zc::launch_net_planes_to_nhwc(n, cin, hw, cpad, d_planes, d_out, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_net_value_head_async(int32_t n, int32_t hw, const void *d_act, const float *d_fc_w, float fc_b,
                            double *d_values, void *hip_stream) {
    if (n < 0 || hw < 1 || (n && (!d_act || !d_fc_w || !d_values))) return fail(ZC_EINVAL, "bad argument");
    // the head reads whole 256-byte pixel rows (128 fp16 channels) in 16-byte pieces
    if ((uintptr_t)d_act & 15) return fail(ZC_EINVAL, "d_act must be 16-byte aligned (128-channel fp16 NHWC rows)");
    if (!n) return ZC_OK;
    zc::launch_net_value_head(n, hw, d_act, d_fc_w, fc_b, d_values, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

// The _w_ family: the entry points above with the network's width as their first argument.  128
// is the call above, argument for argument; 64 runs net_conv64.hip; every other width is refused.
static int net_width(int32_t channels) {
    if (channels == 64 || channels == 128) return ZC_OK;
    return fail(ZC_EINVAL, "%d channels not supported: the MFMA network kernels cover 64 and 128 channels", channels);
}

int zc_net_conv3x3_pack_w_async(int32_t channels, int32_t cin, const void *d_weight, void *d_packed,
                                void *hip_stream) {
    if (int rc = net_width(channels)) return rc;
    if (channels == 128) return zc_net_conv3x3_pack_async(cin, d_weight, d_packed, hip_stream);
    if (!d_weight || !d_packed || ((uintptr_t)d_weight & 15) || ((uintptr_t)d_packed & 15))
        return fail(ZC_EINVAL, "bad argument");
    if (!zc::launch_net64_pack_conv_weight(cin, d_weight, d_packed, (hipStream_t)hip_stream))
        return fail(ZC_EINVAL, "conv3x3 pack: cin %d not supported at 64 channels (32 or 64)", cin);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_net_conv3x3_packed_w_async(int32_t channels, int32_t n, int32_t h, int32_t w, int32_t cin, const void *d_in,
                                  const void *d_packed, const float *d_bias, const void *d_residual, void *d_out,
                                  int32_t relu, void *hip_stream) {
    if (int rc = net_width(channels)) return rc;
    if (channels == 128)
        return zc_net_conv3x3_packed_async(n, h, w, cin, d_in, d_packed, d_bias, d_residual, d_out, relu, hip_stream);
    // the kernel moves activations 16 and 8 bytes at a time and reads the bias 16 at a time
    if (n < 0 || (n && (!d_in || !d_packed || !d_bias || !d_out)) ||
        (((uintptr_t)d_packed | (uintptr_t)d_in | (uintptr_t)d_bias) & 15) ||
        (((uintptr_t)d_residual | (uintptr_t)d_out) & 7))
        return fail(ZC_EINVAL, "bad argument");
    if (!n) return ZC_OK;
    if (!zc::launch_net64_conv3x3_packed(n, h, w, cin, d_in, d_packed, d_bias, d_residual, d_out, relu ? 1 : 0,
                                         (hipStream_t)hip_stream))
        return fail(ZC_EINVAL, "64-channel conv3x3 shape (h %d, w %d, cin %d) not supported", h, w, cin);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_net_tower_w_async(int32_t channels, int32_t n, int32_t h, int32_t w, int32_t cin0, int32_t nconv,
                         const void *d_in, const void *d_packed, const float *d_bias, void *d_out,
                         const float *d_fc_w, float fc_b, double *d_values, void *hip_stream) {
    if (int rc = net_width(channels)) return rc;
    return net_tower(channels, false, false, false, n, h, w, cin0, nconv, d_in, d_packed, d_bias, d_out, d_fc_w, fc_b,
                     d_values, nullptr, nullptr, 32, 1, nullptr, nullptr, hip_stream);
}

int zc_net_tower_policy_w_async(int32_t channels, int32_t n, int32_t h, int32_t w, int32_t cin0, int32_t nconv,
                                const void *d_in, const void *d_packed, const float *d_bias, const float *d_fc_w,
                                float fc_b, double *d_values, const void *d_pw, const float *d_pb,
                                int32_t policy_channels, int32_t relu, void *d_pout, void *hip_stream) {
    if (int rc = net_width(channels)) return rc;
    return net_tower(channels, true, true, false, n, h, w, cin0, nconv, d_in, d_packed, d_bias, nullptr, d_fc_w, fc_b,
                     d_values, d_pw, d_pb, policy_channels, relu, d_pout, nullptr, hip_stream);
}

int zc_net_tower_counted_w_async(int32_t channels, int32_t n, int32_t h, int32_t w, int32_t cin0, int32_t nconv,
                                 const void *d_in, const void *d_packed, const float *d_bias, void *d_out,
                                 const float *d_fc_w, float fc_b, double *d_values, const int32_t *d_count,
                                 void *hip_stream) {
    if (int rc = net_width(channels)) return rc;
    return net_tower(channels, false, false, true, n, h, w, cin0, nconv, d_in, d_packed, d_bias, d_out, d_fc_w, fc_b,
                     d_values, nullptr, nullptr, 32, 1, nullptr, d_count, hip_stream);
}

int zc_net_tower_policy_counted_w_async(int32_t channels, int32_t n, int32_t h, int32_t w, int32_t cin0,
                                        int32_t nconv, const void *d_in, const void *d_packed, const float *d_bias,
                                        const float *d_fc_w, float fc_b, double *d_values, const void *d_pw,
                                        const float *d_pb, int32_t policy_channels, int32_t relu, void *d_pout,
                                        const int32_t *d_count, void *hip_stream) {
    if (int rc = net_width(channels)) return rc;
    return net_tower(channels, true, true, true, n, h, w, cin0, nconv, d_in, d_packed, d_bias, nullptr, d_fc_w, fc_b,
                     d_values, d_pw, d_pb, policy_channels, relu, d_pout, d_count, hip_stream);
}

int zc_net_value_head_w_async(int32_t channels, int32_t n, int32_t hw, const void *d_act, const float *d_fc_w,
                              float fc_b, double *d_values, void *hip_stream) {
    if (int rc = net_width(channels)) return rc;
    if (channels == 128) return zc_net_value_head_async(n, hw, d_act, d_fc_w, fc_b, d_values, hip_stream);
    if (n < 0 || hw < 1 || (n && (!d_act || !d_fc_w || !d_values))) return fail(ZC_EINVAL, "bad argument");
    // the head reads whole 128-byte pixel rows (64 fp16 channels) in 16-byte pieces
    if ((uintptr_t)d_act & 15) return fail(ZC_EINVAL, "d_act must be 16-byte aligned (64-channel fp16 NHWC rows)");
    if (!n) return ZC_OK;
    zc::launch_net64_value_head(n, hw, d_act, d_fc_w, fc_b, d_values, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_chess_from_fen(const char *fen, zc_chess_state *out) {
    // state_from_fen (chess_backend.cpp:525-556): placement, side, castling; en passant and
    // the full-move number are ignored; the half-move clock becomes the fifty counter.
    if (!fen || !out) return fail(ZC_EINVAL, "null argument");
    zc_chess_state s{};
    const char *p = fen;
    int idx = 0;
    for (; *p && *p != ' '; ++p) {
        if (*p == '/') continue;
        if (*p >= '0' && *p <= '9') {
            for (int i = 0; i < *p - '0'; ++i) {
                if (idx >= 64) return fail(ZC_EINVAL, "FEN placement longer than 64 squares");
                s.board[idx++] = ' ';
            }
        } else {
            if (idx >= 64) return fail(ZC_EINVAL, "FEN placement longer than 64 squares");
            s.board[idx++] = (uint8_t)*p;
        }
    }
    if (idx != 64) return fail(ZC_EINVAL, "FEN placement covers %d squares, not 64", idx);
    while (*p == ' ') ++p;
    s.turn = (p[0] == 'w' && (p[1] == ' ' || p[1] == 0)) ? 0 : 1;
    while (*p && *p != ' ') ++p;
    while (*p == ' ') ++p;
    for (; *p && *p != ' '; ++p) {
        if (*p == 'K') s.castle |= 1;
        if (*p == 'Q') s.castle |= 2;
        if (*p == 'k') s.castle |= 4;
        if (*p == 'q') s.castle |= 8;
    }
    while (*p == ' ') ++p;
    while (*p && *p != ' ') ++p;
    while (*p == ' ') ++p;
    s.fifty = (uint8_t)atoi(p);
    *out = s;
    return ZC_OK;
}

int zc_chess_init(zc_chess_state *out) {
    return zc_chess_from_fen("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", out);
}

int zc_c4_from_rows(const char *rows, int32_t turn, zc_c4_state *out) {
    if (!rows || !out) return fail(ZC_EINVAL, "null argument");
    if (turn != 0 && turn != 1) return fail(ZC_EINVAL, "turn must be 0 or 1");
    zc_c4_state s{};
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 7; ++c) {
            const char ch = rows[r * 7 + c];
            const uint64_t bit = 1ull << (7 * c + (5 - r));
            if (ch == 'X') s.stones[0] |= bit;
            else if (ch == 'O') s.stones[1] |= bit;
        }
    s.turn = turn;
    *out = s;
    return ZC_OK;
}

int zc_c4_to_rows(const zc_c4_state *s, char *rows) {
    if (!s || !rows) return fail(ZC_EINVAL, "null argument");
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 7; ++c) {
            const uint64_t bit = 1ull << (7 * c + (5 - r));
            rows[r * 7 + c] = (s->stones[0] & bit) ? 'X' : (s->stones[1] & bit) ? 'O' : ' ';
        }
    return ZC_OK;
}

int zc_c4_legal_order(int32_t mask, int32_t *cols) {
    if (mask < 0 || mask > 127 || !cols) return fail(ZC_EINVAL, "mask must be in [0, 127]");
    const uint32_t w = ZC_C4_ORDER_INIT[mask];
    const int n = (int)((w >> 24) & 15u);
    for (int k = 0; k < n; ++k) cols[k] = (int32_t)((w >> (3 * k)) & 7u);
    return n;
}

int zc_debug_uct(zc_engine *eng, int32_t n, const double *logn, const int32_t *na, const double *q, double c,
                 double *out) {
    if (!eng || n < 0) return fail(ZC_EINVAL, "bad argument");
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    double *dl, *dq, *dout;
    int32_t *dn;
    ZC_HIP(hipMalloc(&dl, n * sizeof(double)));
    ZC_HIP(hipMalloc(&dq, n * sizeof(double)));
    ZC_HIP(hipMalloc(&dout, n * sizeof(double)));
    ZC_HIP(hipMalloc(&dn, n * sizeof(int32_t)));
    hipStream_t s = eng->stream;
    ZC_HIP(hipMemcpyAsync(dl, logn, n * sizeof(double), hipMemcpyHostToDevice, s));
    ZC_HIP(hipMemcpyAsync(dq, q, n * sizeof(double), hipMemcpyHostToDevice, s));
    ZC_HIP(hipMemcpyAsync(dn, na, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    zc::launch_uct_debug(n, dl, dn, dq, c, dout, s);
    ZC_HIP(hipGetLastError());
    ZC_HIP(hipMemcpyAsync(out, dout, n * sizeof(double), hipMemcpyDeviceToHost, s));
    ZC_HIP(hipStreamSynchronize(s));
    (void)hipFree(dl);
    (void)hipFree(dq);
    (void)hipFree(dout);
    (void)hipFree(dn);
    return ZC_OK;
}

int zc_debug_c4_uct_select(zc_engine *eng, int32_t n, const uint16_t *child, const int32_t *na, const int32_t *wa,
                           const int32_t *big_n, double c, int32_t *out_slot, int32_t *out_how) {
    if (!eng || n < 0 || (n && (!child || !na || !wa || !big_n || !out_slot || !out_how)))
        return fail(ZC_EINVAL, "bad argument");
    for (int32_t i = 0; i < n; ++i) {
        if (big_n[i] < 1 || big_n[i] > eng->M) return fail(ZC_EINVAL, "node %d: N outside [1, max_sims + 1]", i);
        for (int k = 0; k < 8; ++k) {
            const int32_t a = na[8 * (size_t)i + k], w = wa[8 * (size_t)i + k];
            if (a < 0 || a > big_n[i] || w < -a || w > a)
                return fail(ZC_EINVAL, "node %d slot %d: need 0 <= Na <= N and |Wa| <= Na", i, k);
        }
    }
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    const size_t slots = 8 * (size_t)n;
    uint8_t *blk;  // na, wa [8n] | N, slot, how [n] | child [8n]
    ZC_HIP(hipMalloc(&blk, slots * 10 + (size_t)n * 12));
    int32_t *dna = (int32_t *)blk, *dwa = dna + slots, *dn = dwa + slots, *dslot = dn + n, *dhow = dslot + n;
    uint16_t *dch = (uint16_t *)(dhow + n);
    hipStream_t s = eng->stream;
    int r = ZC_OK;
    auto hip = [&](hipError_t e) {
        if (e != hipSuccess && r == ZC_OK) r = fail(ZC_EHIP, "%s", hipGetErrorString(e));
    };
    hip(hipMemcpyAsync(dna, na, slots * 4, hipMemcpyHostToDevice, s));
    hip(hipMemcpyAsync(dwa, wa, slots * 4, hipMemcpyHostToDevice, s));
    hip(hipMemcpyAsync(dn, big_n, (size_t)n * 4, hipMemcpyHostToDevice, s));
    hip(hipMemcpyAsync(dch, child, slots * 2, hipMemcpyHostToDevice, s));
    if (r == ZC_OK) {
        zc::launch_c4_uct_select_debug(n, dch, dna, dwa, dn, eng->a.logtab, c, zc::uct_fast_delta(c, eng->M), dslot,
                                       dhow, s);
        hip(hipGetLastError());
    }
    hip(hipMemcpyAsync(out_slot, dslot, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    hip(hipMemcpyAsync(out_how, dhow, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    hip(hipStreamSynchronize(s));
    (void)hipFree(blk);
    return r;
}

int zc_debug_c4_rollout(zc_engine *eng, int32_t first, int32_t n, const zc_c4_state *states, int32_t *out_value,
                        int64_t *out_words) {
    if (!eng || (n && (!states || !out_value || !out_words))) return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, first, n)) return r;
    if (int r = check_carry(eng, first, n)) return r;
    for (int32_t i = 0; i < n; ++i)
        if (!valid_c4(states[i])) return fail(ZC_EINVAL, "state %d is not a valid Connect4 position", i);
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::Arena &a = eng->a;
    hipStream_t s = eng->stream;
    int64_t *dw;
    ZC_HIP(hipMalloc(&dw, n * sizeof(int64_t)));
    ZC_HIP(hipMemcpyAsync(a.roots, states, (size_t)n * sizeof(zc_c4_state), hipMemcpyHostToDevice, s));
    zc::launch_c4_rollout_debug(a, eng->M, first, n, a.roots, a.move, dw, s);
    ZC_HIP(hipGetLastError());
    ZC_HIP(hipMemcpyAsync(out_value, a.move, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ZC_HIP(hipMemcpyAsync(out_words, dw, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ZC_HIP(hipStreamSynchronize(s));
    (void)hipFree(dw);
    return ZC_OK;
}

int zc_debug_c4_walk_async(zc_engine *eng, int32_t first, int32_t n, const zc_c4_state *d_roots, int32_t sims,
                           double c, int32_t bs, int32_t mode, int8_t *d_vals, uint32_t *d_words, int32_t *d_move,
                           int32_t *d_na, zc_game_stats *d_stats, void *hip_stream) {
    if (!eng || (n && (!d_roots || !d_vals || !d_words || !d_move || !d_na || !d_stats)))
        return fail(ZC_EINVAL, "null argument");
    if (mode != 1 && mode != 2) return fail(ZC_EINVAL, "mode must be 1 (record) or 2 (replay)");
    if (int r = check_search(eng, first, n, sims, c, bs)) return r;
    if (int r = check_carry(eng, first, n)) return r;
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::SearchParams p = make_params(eng, first, n, d_roots, sims, c, bs, d_move, d_na, d_stats);
    if (p.philox || p.stamp) return fail(ZC_EINVAL, "the walk diagnostic runs the exact, unstamped search");
    // the logs are indexed by engine game (g * sims, g * flushes): shift so game `first` is row 0
    p.walk_vals = d_vals - (size_t)first * sims;
    p.walk_words = d_words - (size_t)first * ((sims + bs - 1) / bs);
    zc::launch_c4_walk(p, mode, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_debug_rng_copy(zc_engine *eng, int32_t first, int32_t n, void *d_buf, int32_t restore, void *hip_stream) {
    if (!eng || (n && !d_buf)) return fail(ZC_EINVAL, "null argument");
    if (int r = check_games(eng, first, n)) return r;
    if (!n) return ZC_OK;
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    hipStream_t s = (hipStream_t)hip_stream;
    uint8_t *ring = (uint8_t *)(eng->a.ring + (size_t)first * zc::kRingWords);
    uint8_t *pos = (uint8_t *)(eng->a.rngpos + 2 * (size_t)first);
    uint8_t *b = (uint8_t *)d_buf;
    const size_t rb = (size_t)n * zc::kRingWords * sizeof(uint32_t), pb = (size_t)n * 2 * sizeof(uint64_t);
    ZC_HIP(hipMemcpyAsync(restore ? ring : b, restore ? b : ring, rb, hipMemcpyDeviceToDevice, s));
    ZC_HIP(hipMemcpyAsync(restore ? pos : b + rb, restore ? b + rb : pos, pb, hipMemcpyDeviceToDevice, s));
    return ZC_OK;
}

int zc_debug_c4_launch_stamps(zc_engine *eng, uint64_t *d_buf) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    eng->tstamps = d_buf;
    return ZC_OK;
}

int zc_debug_net_switch(const char *name, int32_t value, int32_t *old) {
    int prev = 0;
    if (!zc::net_switch(name, value, &prev))
        return fail(ZC_EINVAL, "zc_debug_net_switch: unknown switch or value (%s = %d)", name ? name : "(null)", value);
    if (old) *old = prev;
    return ZC_OK;
}

int zc_debug_phase_cycles_games(zc_engine *eng, int32_t n_games, int64_t *out) {
    if (!eng || !out) return fail(ZC_EINVAL, "null argument");
    if (n_games < 0 || n_games > eng->cfg.max_games) return fail(ZC_EINVAL, "n_games outside the engine");
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    ZC_HIP(hipDeviceSynchronize());
    ZC_HIP(hipMemcpy(out, eng->a.phase, (size_t)n_games * zc::kPhases * sizeof(int64_t), hipMemcpyDeviceToHost));
    return ZC_OK;
}

int zc_debug_phase_cycles(zc_engine *eng, int32_t enable, int64_t *out8) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    ZC_HIP(hipDeviceSynchronize());
    const size_t G = (size_t)eng->cfg.max_games;
    constexpr int K = zc::kPhases;
    if (out8) {
        std::vector<int64_t> ph(G * K);
        ZC_HIP(hipMemcpy(ph.data(), eng->a.phase, ph.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (int k = 0; k < K; ++k) out8[k] = 0;
        for (size_t g = 0; g < G; ++g)
            for (int k = 0; k < K; ++k) out8[k] += ph[K * g + k];
    }
    ZC_HIP(hipMemset(eng->a.phase, 0, G * K * sizeof(int64_t)));
    eng->stamp = enable ? 1 : 0;
    return ZC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- any game backend (gen_search.hip)
namespace {
size_t gen_slot_bytes() { return sizeof(int32_t) * 3 + sizeof(double) * 2; }  // na, child, untried, wa, qa

// Grow the any-backend tree to hold `nodes` nodes and `slots` move slots, keeping its
// content (the device is synchronised first: a search may be in flight).
int gen_reserve_locked(zc_engine *e, int64_t nodes, int64_t slots) {
    zc::GenArena &g = e->ga;
    if (!g.ctl) {
        if (hipMalloc((void **)&g.ctl, zc::kGenCtlWords * sizeof(int32_t)) != hipSuccess ||
            hipMalloc((void **)&g.pending, (size_t)e->cfg.max_batch * sizeof(int32_t)) != hipSuccess)
            return fail(ZC_ENOMEM, "hipMalloc failed (any-backend tree control)");
        if (hipMemset(g.ctl, 0, zc::kGenCtlWords * sizeof(int32_t)) != hipSuccess) return fail(ZC_EHIP, "memset failed");
        e->bytes += zc::kGenCtlWords * sizeof(int32_t) + (size_t)e->cfg.max_batch * sizeof(int32_t);
    }
    if (nodes <= g.node_cap && slots <= g.slot_cap) return ZC_OK;
    if (nodes > INT32_MAX || slots > INT32_MAX) return fail(ZC_ECAPACITY, "any-backend tree beyond 2^31 nodes or slots");
    const int64_t nn = std::max<int64_t>(nodes, g.node_cap), ns = std::max<int64_t>(slots, g.slot_cap);
    zc::GenArena n = g;
    bool ok = hipMalloc((void **)&n.nodes, (size_t)nn * sizeof(zc::GenNode)) == hipSuccess;
    ok = ok && hipMalloc((void **)&n.na, (size_t)ns * sizeof(int32_t)) == hipSuccess;
    ok = ok && hipMalloc((void **)&n.wa, (size_t)ns * sizeof(double)) == hipSuccess;
    ok = ok && hipMalloc((void **)&n.qa, (size_t)ns * sizeof(double)) == hipSuccess;
    ok = ok && hipMalloc((void **)&n.child, (size_t)ns * sizeof(int32_t)) == hipSuccess;
    ok = ok && hipMalloc((void **)&n.untried, (size_t)ns * sizeof(int32_t)) == hipSuccess;
    if (!ok) {
        void *ptrs[] = {n.nodes, n.na, n.wa, n.qa, n.child, n.untried};
        for (void *p : ptrs)
            if (p && p != g.nodes && p != g.na && p != g.wa && p != g.qa && p != g.child && p != g.untried)
                (void)hipFree(p);
        return fail(ZC_ENOMEM, "hipMalloc failed (any-backend tree of %lld nodes, %lld slots)", (long long)nn,
                    (long long)ns);
    }
    ZC_HIP(hipDeviceSynchronize());
    if (g.node_cap) {
        const size_t on = (size_t)g.node_cap, os = (size_t)g.slot_cap;
        ZC_HIP(hipMemcpy(n.nodes, g.nodes, on * sizeof(zc::GenNode), hipMemcpyDeviceToDevice));
        ZC_HIP(hipMemcpy(n.na, g.na, os * sizeof(int32_t), hipMemcpyDeviceToDevice));
        ZC_HIP(hipMemcpy(n.wa, g.wa, os * sizeof(double), hipMemcpyDeviceToDevice));
        ZC_HIP(hipMemcpy(n.qa, g.qa, os * sizeof(double), hipMemcpyDeviceToDevice));
        ZC_HIP(hipMemcpy(n.child, g.child, os * sizeof(int32_t), hipMemcpyDeviceToDevice));
        ZC_HIP(hipMemcpy(n.untried, g.untried, os * sizeof(int32_t), hipMemcpyDeviceToDevice));
        void *old[] = {g.nodes, g.na, g.wa, g.qa, g.child, g.untried};
        for (void *p : old) (void)hipFree(p);
    }
    e->bytes += (nn - g.node_cap) * (int64_t)sizeof(zc::GenNode) + (ns - g.slot_cap) * (int64_t)gen_slot_bytes();
    n.node_cap = (int32_t)nn;
    n.slot_cap = ns;
    g = n;
    return ZC_OK;
}

zc::GenParams gen_params(const zc_engine *e) {
    zc::GenParams p{};
    p.sims = e->gx_sims;
    p.bs = e->gx_bs;
    p.c = e->gx_c;
    p.logtab = e->a.logtab;
    p.a = e->ga;
    return p;
}

int check_gx(const zc_engine *e) {
    if (!e->gx_active) return fail(ZC_EINVAL, "no any-backend search in progress (call zc_gen_begin first)");
    return ZC_OK;
}
}  // namespace

extern "C" {

int zc_gen_reserve(zc_engine *eng, int32_t nodes, int64_t slots) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    if (nodes < 1 || slots < 0) return fail(ZC_EINVAL, "need nodes >= 1 and slots >= 0");
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    return gen_reserve_locked(eng, nodes, slots);
}

int zc_gen_capacity(zc_engine *eng, int32_t *nodes, int64_t *slots) {
    if (!eng || !nodes || !slots) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    *nodes = eng->ga.node_cap;
    *slots = eng->ga.slot_cap;
    return ZC_OK;
}

int zc_gen_begin(zc_engine *eng, int32_t sims, double c, int32_t bs, int32_t root_moves, void *hip_stream) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    if (int r = check_search(eng, 0, 0, sims, c, bs)) return r;
    if (root_moves < 0) return fail(ZC_EINVAL, "root_moves must be >= 0");
    std::lock_guard<std::mutex> lk(eng->mu);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    if (int r = gen_reserve_locked(eng, (int64_t)sims + 1, std::max<int64_t>(root_moves, eng->ga.slot_cap))) return r;
    eng->gx_sims = sims;
    eng->gx_bs = bs;
    eng->gx_c = c;
    eng->gx_active = true;
    zc::launch_gen_begin(gen_params(eng), root_moves, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_gen_walk(zc_engine *eng, int32_t *d_out, int32_t out_cap, void *hip_stream) {
    if (!eng || !d_out) return fail(ZC_EINVAL, "null argument");
    if (out_cap < 5) return fail(ZC_EINVAL, "out_cap must be >= 5");
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_gx(eng)) return r;
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::launch_gen_walk(gen_params(eng), d_out, out_cap, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_gen_expand(zc_engine *eng, int32_t untried_index, int32_t child_moves, void *hip_stream) {
    if (!eng) return fail(ZC_EINVAL, "null argument");
    if (untried_index < -1 || child_moves < 0) return fail(ZC_EINVAL, "bad untried_index / child_moves");
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_gx(eng)) return r;
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::launch_gen_expand(gen_params(eng), untried_index, child_moves, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_gen_backup(zc_engine *eng, int32_t n_leaves, const double *d_values, void *hip_stream) {
    if (!eng || (n_leaves && !d_values)) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_gx(eng)) return r;
    if (n_leaves < 0 || n_leaves > eng->gx_bs) return fail(ZC_EINVAL, "n_leaves %d outside [0, batch_size]", n_leaves);
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::launch_gen_backup(gen_params(eng), n_leaves, d_values, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    return ZC_OK;
}

int zc_gen_end(zc_engine *eng, int32_t *d_out, int32_t *d_root_na, int32_t na_cap, void *hip_stream) {
    if (!eng || !d_out) return fail(ZC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    if (int r = check_gx(eng)) return r;
    ZC_HIP(hipSetDevice(eng->cfg.device));
    zc::launch_gen_end(gen_params(eng), d_out, d_root_na, d_root_na ? na_cap : 0, (hipStream_t)hip_stream);
    ZC_HIP(hipGetLastError());
    eng->gx_active = false;
    return ZC_OK;
}

}  // extern "C"
