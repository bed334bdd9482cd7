"""The merged flush of the evaluation cache (csrc/evalcache.hip: zc_evalcache_probe_merged_async,
zc_evalcache_commit_merged_async; EvalCache(merge=True); the pools' eval_merge): among the rows
of one flush that miss the table — or all of them when there is no table — rows with an equal
key are evaluated once and the others take a copy, and every output is what evaluating the row
itself gives, bit for bit.  The raw-kernel cases run a fake network: a torch function of the
dense planes whose result does not depend on the batch it is computed in.  The argument checks
at the end need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_eval_cache import (BS, N_GAMES, _c4_roots, _chess_roots, _outputs, _policy_model, _pool, _pool_state,
                                 _random_keys, _same, _value_model, eng)  # noqa: F401  (eng: the engine fixture)

gpu = pytest.mark.gpu

STATS = ("probed", "hits", "inserts", "dropped", "merged")
GUARD = 16   # bytes on either side of every buffer of the harness


# ---------------------------------------------------------------------------------------------
# helpers


class _Guarded:
    """A device buffer with GUARD bytes of 0xA5 before it and 0x5A after it."""

    def __init__(self, shape, dtype, fill=0):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.zeros(n + 2 * GUARD, dtype=torch.uint8, device="cuda")
        self.buf[:GUARD] = 0xA5
        self.buf[-GUARD:] = 0x5A
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(shape)
        if fill:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[-GUARD:] == 0x5A).all())


def _values(planes):
    """The fake network's value: the row's sum, exact in fp64 in any order (small integers)."""
    return planes.double().sum(1)


def _logits(planes, logit_bytes):
    """The fake network's logits: byte j of a row is byte j % plane_bytes of its planes, plus j."""
    if not logit_bytes:
        return None
    pb = planes.view(torch.uint8)
    j = torch.arange(logit_bytes, device="cuda")
    return (pb[:, j % pb.shape[1]] + j.to(torch.uint8)[None]).contiguous()


def _rows_of(assign, key_bytes, plane_halfs, seed):
    """Rows whose key and planes are those of the distinct position assign[row]: (keys, planes)."""
    n = int(max(assign)) + 1
    keys = _random_keys(n, key_bytes, seed)
    assert len({tuple(r) for r in keys.cpu().tolist()}) == n
    g = torch.Generator().manual_seed(seed + 1)
    planes = torch.randint(-8, 9, (n, plane_halfs), generator=g).half().cuda()
    a = torch.as_tensor(np.asarray(assign, np.int64)).cuda()
    return keys[a].contiguous(), planes[a].contiguous()


class _Flush:
    """The merged calls on guarded buffers of one flush shape; entries 0: no table."""

    def __init__(self, entries, key_bytes, logit_bytes, total_rows, plane_halfs, rows=1, game_rows=1, stream=0):
        from zeroclone_amd import _native
        self.nat, self.sizes, self.lb = _native, (entries, key_bytes, logit_bytes), logit_bytes
        self.rows, self.game_rows, self.total, self.stream = rows, game_rows, total_rows, stream
        self.n = n = total_rows // game_rows * rows
        self.table = _Guarded((_native.evalcache_bytes(*self.sizes)[0],), torch.uint8) if entries else None
        self.scratch = _Guarded((_native.evalcache_merge_scratch_bytes(n) // 4,), torch.int32)
        self.count = _Guarded((1,), torch.int32)
        self.stats_t = _Guarded((5,), torch.int64)
        self.out_v = _Guarded((total_rows,), torch.float64, -7.0)
        self.out_l = _Guarded((total_rows, logit_bytes), torch.uint8, 0x5A) if logit_bytes else None
        self.dense = _Guarded((n, plane_halfs), torch.float16, -3.0)
        self.miss = _Guarded((n,), torch.int32, -1)
        self.dv = _Guarded((n,), torch.float64)
        self.dl = _Guarded((n, logit_bytes), torch.uint8) if logit_bytes else None

    def fresh(self):
        self.out_v.t.fill_(-7.0)
        self.miss.t.fill_(-1)
        self.dense.t.fill_(-3.0)
        if self.lb:
            self.out_l.t.fill_(0x5A)

    def _ptr(self, g):
        return g.t.data_ptr() if g is not None else 0

    def probe(self, keys, planes):
        self.nat.evalcache_probe_merged(self._ptr(self.table), *self.sizes, self.n, self.rows, self.game_rows,
                                        keys.data_ptr(), planes.data_ptr(), planes.shape[1] * 2, self._ptr(self.out_v),
                                        self._ptr(self.out_l), self._ptr(self.dense), self._ptr(self.miss),
                                        self._ptr(self.count), self._ptr(self.stats_t), self._ptr(self.scratch),
                                        self.stream)

    def network(self):
        """On the whole dense buffer, as a launch that cannot know the count would."""
        self.dv.t.copy_(_values(self.dense.t))
        if self.lb:
            self.dl.t.copy_(_logits(self.dense.t, self.lb))

    def commit(self, keys):
        self.nat.evalcache_commit_merged(self._ptr(self.table), *self.sizes, self.n, self.rows, self.game_rows,
                                         keys.data_ptr(), self._ptr(self.miss), self._ptr(self.count),
                                         self._ptr(self.dv), self._ptr(self.dl), self._ptr(self.out_v),
                                         self._ptr(self.out_l), self._ptr(self.stats_t), self._ptr(self.scratch),
                                         self.stream)

    def stats(self):
        return dict(zip(STATS, (int(x) for x in self.stats_t.t.cpu())))

    def intact(self):
        return all(g.intact() for g in vars(self).values() if isinstance(g, _Guarded))

    def flush(self, keys, planes):
        """probe -> checks of the dense rows -> network -> commit -> checks of every output;
        returns (the dense slots' rows, the counters' deltas)."""
        before = self.stats()
        self.fresh()
        self.probe(keys, planes)
        k = int(self.count.t.item())
        assert 0 <= k <= self.n
        miss = self.miss.t.cpu().numpy()
        assert (miss[k:] == -1).all()
        led = miss[:k].astype(np.int64)
        assert len(set(led.tolist())) == k
        mi = torch.from_numpy(led).cuda()
        assert torch.equal(self.dense.t[:k].view(torch.int16), planes[mi].view(torch.int16))
        assert bool((self.dense.t[k:] == -3.0).all())
        self.network()
        self.commit(keys)
        torch.cuda.synchronize()
        assert int(self.count.t.item()) == 0                        # reset for the next flush
        assert bool((self.scratch.t[:-self.n] == 0).all())          # and so is the claim table
        self.check_outputs(planes)
        d = {key: v - before[key] for key, v in self.stats().items()}
        assert d["probed"] == self.n
        _identity(d, self.table is not None)
        assert self.intact()
        return led, d

    def taking_part(self):
        r = torch.arange(self.total, device="cuda")
        return (r % self.game_rows) < self.rows

    def check_outputs(self, planes):
        part = self.taking_part()
        assert torch.equal(self.out_v.t[part], _values(planes)[part])
        assert bool((self.out_v.t[~part] == -7.0).all())
        if self.lb:
            assert torch.equal(self.out_l.t[part], _logits(planes, self.lb)[part])
            assert bool((self.out_l.t[~part] == 0x5A).all())


def _identity(s, table=True):
    """probed = hits + merged + inserts + dropped; without a table hits = inserts = dropped = 0 and
    the probed - merged other rows were evaluated."""
    if table:
        assert s["probed"] == s["hits"] + s["merged"] + s["inserts"] + s["dropped"], s
    else:
        assert s["hits"] == s["inserts"] == s["dropped"] == 0 <= s["merged"] <= s["probed"], s


def _assign(n, distinct, seed):
    """n rows over `distinct` positions, each at least once, shuffled."""
    rng = np.random.default_rng(seed)
    a = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
    rng.shuffle(a)
    return a


SHAPES = [(24, 84, 0), (24, 84, 14), (72, 1088, 0), (72, 64, 8192)]


# ---------------------------------------------------------------------------------------------
# 1. merged probe / commit is exact


@gpu
@pytest.mark.parametrize("key_bytes,plane_halfs,logit_bytes", SHAPES)
def test_merged_flush_evaluates_each_key_once_and_every_row_gets_its_output(key_bytes, plane_halfs, logit_bytes):
    """96 rows (12 workgroups of 8 waves) over 20 keys, an empty table; then the same rows again."""
    a = _assign(96, 20, seed=key_bytes + logit_bytes)
    keys, planes = _rows_of(a, key_bytes, plane_halfs, seed=3)
    f = _Flush(8192, key_bytes, logit_bytes, 96, plane_halfs)
    led, d = f.flush(keys, planes)
    assert len(led) == 20 and sorted(a[led].tolist()) == list(range(20))   # the 20 keys, each once
    assert d["hits"] == 0 and d["merged"] == 76 and d["inserts"] + d["dropped"] == 20, d
    # again: a row whose key was inserted hits, and the rest merge among themselves
    led2, d2 = f.flush(keys, planes)
    assert len(led2) == 20 - d["inserts"] and len(set(a[led2].tolist())) == len(led2)
    rest = int(np.isin(a, a[led2]).sum())                                  # rows of the keys not in the table
    assert d2["hits"] == 96 - rest and d2["merged"] == rest - len(led2), (d, d2)
    print(f"key {key_bytes} planes {plane_halfs} logits {logit_bytes}: {d} then {d2}")


# ---------------------------------------------------------------------------------------------
# 2. extremes


@gpu
def test_one_key_is_evaluated_once_and_distinct_keys_do_not_merge():
    f = _Flush(1024, 24, 14, 64, 84)
    keys, planes = _rows_of(np.zeros(64, np.int64), 24, 84, seed=5)
    led, d = f.flush(keys, planes)
    assert len(led) == 1 and d["merged"] == 63 and d["hits"] == 0
    f = _Flush(1024, 24, 14, 64, 84)
    keys, planes = _rows_of(np.arange(64), 24, 84, seed=6)
    led, d = f.flush(keys, planes)
    assert sorted(led.tolist()) == list(range(64)) and d["merged"] == 0   # a permutation of the rows


def test_no_rows_is_ok():
    """n_rows == 0: ZC_OK from the probe before any pointer is looked at, without a device."""
    from zeroclone_amd import _native
    L, null = _native.lib(), ctypes.c_void_p(None)
    cnt = ctypes.c_int32(0)
    b = ctypes.c_int64(-1)
    assert L.zc_evalcache_merge_scratch_bytes(0, ctypes.byref(b)) == 0 and b.value == 8
    assert L.zc_evalcache_probe_merged_async(null, 0, 24, 0, 0, 1, 1, null, null, 168, null, null, null, null,
                                             ctypes.cast(ctypes.byref(cnt), ctypes.c_void_p), null, null, null) == 0


@gpu
def test_a_flush_of_no_rows_finishes_the_flush():
    """The commit of no rows still leaves *d_count = 0 (no scratch needed)."""
    from zeroclone_amd import _native
    count = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    _native.evalcache_probe_merged(0, 0, 24, 0, 0, 1, 1, 0, 0, 168, 0, 0, 0, 0, count.data_ptr(), 0, 0)
    _native.evalcache_commit_merged(0, 0, 24, 0, 0, 1, 1, 0, 0, count.data_ptr(), 0, 0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert int(count.item()) == 0


# ---------------------------------------------------------------------------------------------
# 3. the claim table's walk past taken slots


@gpu
def test_claim_walk_passes_slots_taken_by_other_keys():
    """512 keys twice in 2048 claim slots: different keys meet in a slot for any hash, so this
    fails if an unequal claimant counts as equal or the walk stops at the first taken slot."""
    a = np.concatenate([np.arange(512), np.arange(512)])
    np.random.default_rng(8).shuffle(a)
    keys, planes = _rows_of(a, 72, 64, seed=9)
    f = _Flush(1 << 14, 72, 16, 1024, 64)
    led, d = f.flush(keys, planes)
    assert len(led) == 512 and sorted(a[led].tolist()) == list(range(512))
    assert d["merged"] == 512 and d["hits"] == 0, d


# ---------------------------------------------------------------------------------------------
# 4. no table


@gpu
@pytest.mark.parametrize("key_bytes,plane_halfs,logit_bytes", SHAPES)
def test_merging_without_a_table(key_bytes, plane_halfs, logit_bytes):
    a = _assign(96, 20, seed=key_bytes + logit_bytes)
    keys, planes = _rows_of(a, key_bytes, plane_halfs, seed=3)
    f = _Flush(0, key_bytes, logit_bytes, 96, plane_halfs)
    for _ in range(2):   # nothing is kept: the second flush evaluates the 20 keys again
        led, d = f.flush(keys, planes)
        assert len(led) == 20 and sorted(a[led].tolist()) == list(range(20))
        assert d == {"probed": 96, "hits": 0, "inserts": 0, "dropped": 0, "merged": 76}


# ---------------------------------------------------------------------------------------------
# 5. the short flush


@gpu
@pytest.mark.parametrize("entries", [1024, 0])
def test_short_flush_merges_each_games_first_rows_only(entries):
    """rows_per_game 3 of game_rows 8, 16 games: the 48 taking-part rows hold 10 keys, and rows
    3..7 of every game hold the same keys without taking part."""
    games, gr, nb = 16, 8, 3
    a = np.random.default_rng(11).integers(0, 10, games * gr)
    part = (np.arange(games * gr) % gr) < nb
    a[np.flatnonzero(part)[:10]] = np.arange(10)   # every key among the taking-part rows
    keys, planes = _rows_of(a, 24, 84, seed=12)
    f = _Flush(entries, 24, 14, games * gr, 84, rows=nb, game_rows=gr)
    led, d = f.flush(keys, planes)   # checks the sentinels of the other rows and the guard bytes
    assert len(led) == 10 and part[led].all() and sorted(a[led].tolist()) == list(range(10))
    assert d["probed"] == 48 and d["merged"] == 38 and d["hits"] == 0, d
    led2, d2 = f.flush(keys, planes)
    if entries:   # the rows of the inserted keys hit, the rest merge among themselves
        rest = int((np.isin(a, a[led2]) & part).sum())
        assert len(led2) == 10 - d["inserts"] and d2["hits"] == 48 - rest and d2["merged"] == rest - len(led2)
    else:
        assert len(led2) == 10 and d2["merged"] == 38


# ---------------------------------------------------------------------------------------------
# 6. graph replay: the scratch resets itself


@gpu
@pytest.mark.parametrize("entries", [4096, 0])
def test_merged_flush_replays_from_a_graph(entries):
    n, kb, ph, lb = 96, 24, 84, 14
    side = torch.cuda.Stream()
    f = _Flush(entries, kb, lb, n, ph, stream=side.cuda_stream)
    keys = torch.zeros((n, kb // 8), dtype=torch.int64, device="cuda")
    planes = torch.zeros((n, ph), dtype=torch.float16, device="cuda")

    def step():
        f.probe(keys, planes)
        f.network()
        f.commit(keys)

    k0, p0 = _rows_of(_assign(n, 7, seed=20), kb, ph, seed=21)
    keys.copy_(k0)
    planes.copy_(p0)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()   # the fake network's kernels loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    seen = f.stats()
    for i, distinct in enumerate((20, 96, 1)):   # the duplicate structure changes between replays
        k, p = _rows_of(_assign(n, distinct, seed=30 + i), kb, ph, seed=40 + i)
        keys.copy_(k)
        planes.copy_(p)
        f.fresh()
        g.replay()
        torch.cuda.synchronize()
        f.check_outputs(planes)
        now = f.stats()
        d = {key: now[key] - seen[key] for key in now}
        seen = now
        assert d["probed"] == n
        _identity(d, bool(entries))
        assert d["merged"] == n - distinct and d["hits"] == 0, (i, d)   # fresh keys every time
        assert int(f.count.t.item()) == 0 and bool((f.scratch.t[:-n] == 0).all()) and f.intact()


# ---------------------------------------------------------------------------------------------
# 7. the searches: the merging callable against the plain one


@gpu
@pytest.mark.parametrize("entries", [1 << 14, 0])
@pytest.mark.parametrize("game", ["c4", "chess"])
@pytest.mark.parametrize("sims", [64, 60])   # 60: the last flush holds 4 of the 8 leaves (rows())
def test_value_search_with_merging_returns_the_plain_search(eng, game, sims, entries):
    from zeroclone_amd.evalcache import CachedValue, EvalCache
    from zeroclone_amd.nets import MfmaValueNetwork
    from zeroclone_amd.valued import C4ValuedSearch, ChessValuedSearch, NetValue
    roots = _c4_roots() if game == "c4" else _chess_roots()
    if game == "c4":
        roots[1] = roots[0]   # two games from the opening: their first flushes hold the same rows
    net = MfmaValueNetwork(_value_model(2 if game == "c4" else 17, seed=21), "cuda")
    seeds = list(range(50, 50 + N_GAMES))
    cache = EvalCache(entries, 24 if game == "c4" else 72, 0, merge=True)
    out = []
    for fn in (NetValue(net), CachedValue(net, cache)):
        vs = (C4ValuedSearch if game == "c4" else ChessValuedSearch)(eng, N_GAMES, BS, leaves=True)
        eng.seed(0, seeds)
        vs.run(roots, sims, 1.4, fn)
        out.append(_outputs(vs))
    _same(out[0], out[1], (game, sims, entries))
    s = cache.stats()
    print(f"{game} value search, {sims} sims, {entries} entries: {s}")
    assert tuple(s) == STATS and s["probed"] == N_GAMES * (8 * (sims // BS) + sims % BS)
    _identity(s, bool(entries))
    assert (cache.table is None) == (not entries)
    if game == "c4":
        assert s["merged"] > 0


@gpu
@pytest.mark.parametrize("entries", [1 << 14, 0])
@pytest.mark.parametrize("game", ["c4", "chess"])
def test_puct_search_with_merging_returns_the_plain_search(eng, game, entries):
    """Connect4 with the linear head, chess with the convolutional head."""
    from zeroclone_amd.evalcache import CachedPolicy, EvalCache
    from zeroclone_amd.nets import MfmaPolicyValueNetwork
    from zeroclone_amd.valued import C4PuctSearch, ChessPuctSearch, PolicyNet
    c4 = game == "c4"
    roots = _c4_roots() if c4 else _chess_roots()
    if c4:
        roots[1] = roots[0]
    net = MfmaPolicyValueNetwork(_policy_model("c4" if c4 else "chess", seed=22), "cuda")
    cache = EvalCache(entries, 24 if c4 else 72, 14 if c4 else 8192, merge=True)
    kw = {} if c4 else dict(planes_nhwc=True)
    out = []
    for fn in (PolicyNet(net), CachedPolicy(net, cache)):
        ps = (C4PuctSearch if c4 else ChessPuctSearch)(eng, N_GAMES, BS, seed=3, leaves=True, **kw)
        ps.run(roots, 64, fn, temperature=1.0)
        o = _outputs(ps)
        o["prior"] = ps.prior.clone()
        out.append(o)
    _same(out[0], out[1], (game, entries))
    s = cache.stats()
    print(f"{game} PUCT search, {entries} entries: {s}")
    _identity(s, bool(entries))
    if c4:
        assert s["merged"] > 0   # the two equal roots, at the least


# ---------------------------------------------------------------------------------------------
# 8. the pools


def _tower_rows(s):
    return s["probed"] - s["hits"] - s.get("merged", 0)


@gpu
@pytest.mark.parametrize("kind,steps", [("c4_value", 6), ("c4_puct", 6), ("chess_puct", 3)])
def test_pool_with_merging_plays_the_pool_without_it(kind, steps):
    """Neither option / the cache alone / the cache and merging / merging alone: one game
    record, and merging never evaluates more rows than the cache alone does."""
    states, rows = [], []
    for entries, merge in ((0, False), (1 << 16, False), (1 << 16, True), (0, True)):
        pool = _pool(kind, entries, eval_merge=merge)
        for _ in range(steps):
            pool.step()
        pool.check()
        states.append(_pool_state(pool))
        if entries or merge:
            s = pool.eval_cache_stats()
            print(f"{kind} eval_cache {entries} eval_merge {merge}: {s}")
            assert ("merged" in s) == merge
            if merge:
                _identity(s, bool(entries))
                assert all((c.table is None) == (not entries) for c in pool._caches)
            rows.append(_tower_rows(s))
        pool.close()
    for st in states[1:]:
        for k in states[0]:
            assert torch.equal(states[0][k], st[k]), (kind, k)
    cache_only, both, merge_only = rows
    assert both <= cache_only
    if kind == "c4_value":   # every game's first flush from the opening holds the same rows
        assert both < cache_only and merge_only < N_GAMES * 64 * steps


@gpu
@pytest.mark.parametrize("kind", ["c4_value", "chess_puct"])
@pytest.mark.parametrize("entries", [1 << 16, 0])
def test_merging_pool_replays_its_step_from_a_graph(kind, entries):
    a, b = _pool(kind, entries, eval_merge=True), _pool(kind, entries, eval_merge=True)
    g = b.capture_step()
    for i in range(3):
        a.step()
        g.replay()
        torch.cuda.synchronize()
        for k in ("roots", "moves", "results"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (kind, entries, i, k)
    _identity(b.eval_cache_stats(), bool(entries))
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------
# 9. the refusals (no GPU)


def test_no_table_needs_merge():
    from zeroclone_amd.evalcache import EvalCache
    with pytest.raises(ValueError):
        EvalCache(0, 24)
    with pytest.raises(ValueError):
        EvalCache(-8, 24, merge=True)
    c = EvalCache(0, 24, merge=True)
    assert c.table is None and c.merge and c.entries == 0


def test_pools_refuse_eval_merge_they_cannot_serve():
    from zeroclone_amd.arena import C4Arena, ChessArena
    from zeroclone_amd.nets import PolicyValueNetwork, ValueNetwork
    from zeroclone_amd.selfplay import C4SelfPlay, ChessSelfPlay
    for cls in (C4SelfPlay, ChessSelfPlay):
        with pytest.raises(ValueError, match="eval_merge"):
            cls(8, 64, eval_merge=True)                                   # no network
        with pytest.raises(ValueError, match="MFMA"):
            cls(8, 64, eval_merge=True, net=ValueNetwork(128, 1, in_planes=2))   # a torch module
        with pytest.raises(ValueError, match="MFMA"):
            cls(8, 64, eval_merge=True, eval_cache=64, puct_net=PolicyValueNetwork(blocks=1))
    with pytest.raises(ValueError, match="eval_merge"):
        C4Arena(8, 64, net_a=object(), net_b=object(), eval_merge=True)
    with pytest.raises(ValueError, match="eval_merge"):
        ChessArena(8, 64, puct_net_a=object(), puct_net_b=object(), eval_merge=True)


def test_merged_entry_points_refuse_bad_arguments():
    """ZC_EINVAL before any launch: the pointers are never followed."""
    from zeroclone_amd import _native
    L, EINVAL = _native.lib(), _native.ZC_EINVAL
    P = ctypes.c_void_p
    b = ctypes.c_int64(0)
    assert L.zc_evalcache_merge_scratch_bytes(-1, ctypes.byref(b)) == EINVAL
    assert L.zc_evalcache_merge_scratch_bytes(8, None) == EINVAL
    for n, slots in ((1, 2), (2, 4), (3, 8), (96, 256), (1024, 2048)):
        assert L.zc_evalcache_merge_scratch_bytes(n, ctypes.byref(b)) == 0 and b.value == 4 * (slots + n)

    good = dict(table=0, entries=0, key_bytes=24, logit_bytes=0, n_rows=8, rpg=1, gr=1, keys=0x1000, planes=0x2000,
                plane_bytes=168, out_v=0x3000, out_l=0, dense=0x4000, miss=0x5000, count=0x6000, stats=0x7000,
                scratch=0x8000)

    def probe(**kw):
        a = dict(good, **kw)
        return L.zc_evalcache_probe_merged_async(
            P(a["table"] or None), a["entries"], a["key_bytes"], a["logit_bytes"], a["n_rows"], a["rpg"], a["gr"],
            P(a["keys"] or None), P(a["planes"] or None), a["plane_bytes"], P(a["out_v"] or None),
            P(a["out_l"] or None), P(a["dense"] or None), P(a["miss"] or None), P(a["count"] or None),
            P(a["stats"] or None), P(a["scratch"] or None), None)

    def commit(**kw):
        a = dict(good, dv=0x9000, dl=0)
        a.update(kw)
        return L.zc_evalcache_commit_merged_async(
            P(a["table"] or None), a["entries"], a["key_bytes"], a["logit_bytes"], a["n_rows"], a["rpg"], a["gr"],
            P(a["keys"] or None), P(a["miss"] or None), P(a["count"] or None), P(a["dv"] or None),
            P(a["dl"] or None), P(a["out_v"] or None), P(a["out_l"] or None), P(a["stats"] or None),
            P(a["scratch"] or None), None)

    bad = [dict(entries=64),                       # entries without a table
           dict(table=0x100),                      # a table of no entries
           dict(table=0x108, entries=64),          # a table off its 16-byte alignment
           dict(key_bytes=20), dict(key_bytes=0), dict(key_bytes=520), dict(logit_bytes=7),
           dict(n_rows=-1), dict(rpg=0), dict(rpg=3, gr=2), dict(n_rows=8, rpg=3, gr=8),
           dict(n_rows=1 << 30, rpg=1, gr=2),      # 2^31 buffer rows
           dict(count=0), dict(count=0x6002), dict(stats=0x7004),
           dict(keys=0), dict(keys=0x1004), dict(out_v=0x3004), dict(miss=0x5002), dict(miss=0),
           dict(scratch=0), dict(scratch=0x8002),
           dict(logit_bytes=14)]                   # logits without their output pointer
    for kw in bad:
        assert probe(**kw) == EINVAL, ("probe", kw)
        assert commit(**kw) == EINVAL, ("commit", kw)
    for kw in (dict(plane_bytes=0), dict(plane_bytes=7), dict(planes=0), dict(planes=0x2001), dict(dense=0),
               dict(dense=0x4001)):
        assert probe(**kw) == EINVAL, ("probe", kw)
    for kw in (dict(dv=0), dict(dv=0x9004), dict(logit_bytes=14, out_l=0xA000), dict(logit_bytes=14, out_l=0xA000, dl=0xB001)):
        assert commit(**kw) == EINVAL, ("commit", kw)
    # the Python wrappers refuse the same before the library is asked
    with pytest.raises(ValueError):
        _native.evalcache_probe_merged(0, 0, 24, 0, 8, 3, 8, 0x1000, 0x2000, 168, 0x3000, 0, 0x4000, 0x5000, 0x6000,
                                       0, 0x8000)
    with pytest.raises(ValueError):
        _native.evalcache_commit_merged(0, 0, 24, 0, 8, 1, 1, 0x1000, 0x5000, 0x6000, 0x9000, 0, 0x3000, 0, 0, 0)
    with pytest.raises(ValueError):
        _native.evalcache_merge_scratch_bytes(-1)
