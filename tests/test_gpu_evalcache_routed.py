"""The routed flush of the evaluation cache (csrc/evalcache.hip: zc_evalcache_probe_routed_async,
zc_evalcache_commit_routed_async) against its numpy spec (tests/evalcache_routed_ref.py): a table,
a dense list and a set of counters per network, picked by bit 0 of the game's route word.

The "networks" are scripted: the planes of a row are its key's bytes, and network k's value and
logits are exact integer functions of those bytes and of k, different for A and B — so an output
that came from the other network's table, dense list or launch is a wrong number, not a near one.
The dense order and the leaders may vary from run to run, so every flush compares each network's
set of miss rows (with merging: one row of every group of equal keys), the outputs after the
commit, and the counters; the tables the device leaves are read back and must be an outcome the
commit's rules allow (RoutedSpec.commit_observed).  The argument checks at the end need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import evalcache_ref as ref
from evalcache_routed_ref import STATS, RoutedSpec
from test_gpu_eval_merge import _Guarded

gpu = pytest.mark.gpu

ROUTES = {"a": lambda n: np.zeros(n, np.int32), "b": lambda n: np.ones(n, np.int32),
          "alt": lambda n: (np.arange(n) % 2).astype(np.int32),
          "high": lambda n: ((np.arange(n) * 5 // 3 % 2) | (0x7FFFFFF0 - 16 * np.arange(n))).astype(np.int32)}


# ---------------------------------------------------------------------------------------------
# the scripted networks, on the host (from the keys) and on the device (from the dense planes)


def _host_bytes(keys):
    return np.ascontiguousarray(keys).view(np.uint8).reshape(keys.shape[0], -1).astype(np.int64)


def host_values(keys, k):
    b = _host_bytes(keys)
    return (b.sum(1) * (k + 2) + 1000 * k + b[:, 0]).astype(np.float64)


def host_logits(keys, k, logit_bytes):
    b = _host_bytes(keys)
    j = np.arange(logit_bytes)
    return ((b[:, j % b.shape[1]] * (3 + 2 * k) + j[None] + 17 * k) & 0xFF).astype(np.uint8)


def dev_values(planes, k):
    b = planes.to(torch.int64)
    return (b.sum(1) * (k + 2) + 1000 * k + b[:, 0]).to(torch.float64)


def dev_logits(planes, k, logit_bytes):
    b = planes.to(torch.int64)
    j = torch.arange(logit_bytes, device=planes.device)
    return ((b[:, j % b.shape[1]] * (3 + 2 * k) + j[None] + 17 * k) & 0xFF).to(torch.uint8)


def _pool_keys(n, kw, seed):
    keys = np.random.default_rng(seed).integers(0, 1 << 64, (n, kw), dtype=np.uint64)
    assert len({tuple(k) for k in keys.tolist()}) == n
    return keys


# ---------------------------------------------------------------------------------------------
# the harness: the routed calls on guarded buffers of one flush shape, held to the spec


class Routed:
    def __init__(self, entries, key_bytes, logit_bytes, n_games, rows=1, game_rows=1, merge=False):
        from zeroclone_amd import _native
        self.nat, self.sizes, self.kb, self.lb = _native, (entries, key_bytes, logit_bytes), key_bytes, logit_bytes
        self.rows, self.game_rows, self.games, self.merge = rows, game_rows, n_games, merge
        self.total, self.n = n_games * game_rows, n_games * rows
        n, total = self.n, self.total
        self.lay = ref.layout(entries, key_bytes, logit_bytes) if entries else None
        self.tables = [_Guarded((_native.evalcache_bytes(*self.sizes)[0],), torch.uint8) for _ in range(2)] \
            if entries else None
        self.scratch = _Guarded((_native.evalcache_merge_scratch_bytes(n) // 4,), torch.int32) if merge else None
        self.count = _Guarded((2,), torch.int32)
        self.stats_t = _Guarded((2, 5), torch.int64)
        self.out_v = _Guarded((total,), torch.float64, -7.0)
        self.out_l = _Guarded((total, logit_bytes), torch.uint8, 0x5A) if logit_bytes else None
        self.dense = [_Guarded((n, key_bytes), torch.uint8, 0xEE) for _ in range(2)]
        self.miss = _Guarded((2, n), torch.int32, -1)
        self.dv = [_Guarded((n,), torch.float64) for _ in range(2)]
        self.dl = [_Guarded((n, logit_bytes), torch.uint8) for _ in range(2)] if logit_bytes else None
        self.spec = RoutedSpec(entries, key_bytes, logit_bytes, merge)

    def _ptr(self, g):
        return g.t.data_ptr() if g is not None else 0

    def _tptr(self):
        return [self._ptr(t) for t in self.tables] if self.tables else [0, 0]

    def fresh(self):
        self.out_v.t.fill_(-7.0)
        self.miss.t.fill_(-1)
        for d in self.dense:
            d.t.fill_(0xEE)
        if self.lb:
            self.out_l.t.fill_(0x5A)

    def probe(self, keys_t, planes, route_t):
        self.nat.evalcache_probe_routed(*self._tptr(), *self.sizes, self.n, self.rows, self.game_rows,
                                        route_t.data_ptr(), keys_t.data_ptr(), planes.data_ptr(), self.kb,
                                        self._ptr(self.out_v), self._ptr(self.out_l), self._ptr(self.dense[0]),
                                        self._ptr(self.dense[1]), self._ptr(self.miss), self._ptr(self.count),
                                        self._ptr(self.stats_t), self._ptr(self.scratch))

    def networks(self):
        """Each on its whole dense buffer, as a launch that cannot know the count would."""
        for k in range(2):
            self.dv[k].t.copy_(dev_values(self.dense[k].t, k))
            if self.lb:
                self.dl[k].t.copy_(dev_logits(self.dense[k].t, k, self.lb))

    def commit(self, keys_t):
        dl = [self._ptr(d) for d in self.dl] if self.lb else [0, 0]
        self.nat.evalcache_commit_routed(*self._tptr(), *self.sizes, self.n, self.rows, self.game_rows,
                                         keys_t.data_ptr(), self._ptr(self.miss), self._ptr(self.count),
                                         self._ptr(self.dv[0]), dl[0], self._ptr(self.dv[1]), dl[1],
                                         self._ptr(self.out_v), self._ptr(self.out_l), self._ptr(self.stats_t),
                                         self._ptr(self.scratch))

    def stats(self):
        return [dict(zip(STATS, (int(x) for x in row))) for row in self.stats_t.t.cpu()]

    def observed(self):
        out = []
        for t in self.tables:
            raw = t.t.cpu().numpy()
            E, lay = self.lay.entries, self.lay
            out.append((int(raw[:4].view(np.uint32)[0]), raw[lay.meta:lay.meta + 4 * E].view(np.uint32).copy(),
                        raw[lay.keys:lay.keys + self.kb * E].view(np.uint64).reshape(E, -1).copy()))
        return out

    def empty(self, k):
        """Table k holds no entry: all zeros past the header's epoch word (every commit moves both
        tables' epochs on, with or without a row of theirs)."""
        return not bool(self.tables[k].t[4:].any())

    def intact(self):
        def walk(x):
            if isinstance(x, _Guarded):
                yield x
            elif isinstance(x, list):
                for y in x:
                    yield from walk(y)
        return all(g.intact() for v in vars(self).values() for g in walk(v))

    def flush(self, keys, route):
        """keys [total, kw] uint64, route [games] int32 -> the spec's Flush.  Checks the dense
        lists after the probe and every output, count, counter and guard after the commit."""
        keys_t = torch.from_numpy(keys.view(np.int64)).cuda()
        planes = keys_t.view(torch.uint8).view(self.total, self.kb).clone()
        route_t = torch.from_numpy(np.ascontiguousarray(route, dtype=np.int32)).cuda()
        f = self.spec.probe(keys, route, self.rows, self.game_rows)
        self.fresh()
        self.probe(keys_t, planes, route_t)
        count = self.count.t.cpu().tolist()
        miss = self.miss.t.cpu().numpy()
        assert min(count) >= 0 and sum(count) <= self.n, count
        for k in range(2):
            c = count[k]
            led = miss[k, :c].tolist()
            assert (miss[k, c:] == -1).all()
            assert c == len(f.groups[k]) == len(set(led)), (k, c, len(f.groups[k]))
            assert all(len(set(g) & set(led)) == 1 for g in f.groups[k]), (k, "a dense row per group of the spec")
            assert torch.equal(self.dense[k].t[:c], planes[torch.as_tensor(led, dtype=torch.int64).cuda()])
            assert bool((self.dense[k].t[c:] == 0xEE).all())
        self.networks()
        self.commit(keys_t)
        torch.cuda.synchronize()
        assert self.count.t.cpu().tolist() == [0, 0]
        if self.merge:
            assert bool((self.scratch.t[:-self.n] == 0).all())   # the claim words
        self.check_outputs(keys, f)
        self.spec.commit_observed(keys, f, self.observed() if self.tables else None)
        assert self.stats() == self.spec.stats, (self.stats(), self.spec.stats)
        self.spec.identity()
        assert self.intact()
        return f

    def check_outputs(self, keys, f):
        part = np.zeros(self.total, bool)
        part[f.rows] = True
        net = np.zeros(self.total, np.int64)
        net[f.rows] = f.net
        want = np.where(net == 1, host_values(keys, 1), host_values(keys, 0))
        got = self.out_v.t.cpu().numpy()
        assert np.array_equal(got[part], want[part])
        assert (got[~part] == -7.0).all()                        # rows past rows_per_game: untouched
        if self.lb:
            wl = np.where((net == 1)[:, None], host_logits(keys, 1, self.lb), host_logits(keys, 0, self.lb))
            gl = self.out_l.t.cpu().numpy()
            assert np.array_equal(gl[part], wl[part])
            assert (gl[~part] == 0x5A).all()


def _assigned(pool, total, rng):
    return pool[rng.integers(0, pool.shape[0], total)]


# ---------------------------------------------------------------------------------------------
# 1. every shape against the spec


@gpu
@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merge"])
@pytest.mark.parametrize("entries", [8, 1024])
@pytest.mark.parametrize("rows,game_rows", [(1, 1), (3, 4), (4, 8)])
@pytest.mark.parametrize("key_bytes,logit_bytes", [(24, 0), (24, 14), (72, 8192)])
def test_routed_flush_equals_the_spec(key_bytes, logit_bytes, rows, game_rows, entries, merge):
    """Game counts 1, 5 and 11 (11 games of one row: a workgroup's eight rows hold misses of both
    networks) under every route; three flushes each: fresh keys with duplicates within and across
    the networks, the same rows again (what was inserted hits), and a mix of old and new keys.
    8 entries are one set: evictions, drops and lost claims."""
    kw = key_bytes // 8
    for games in (1, 5, 11):
        for name, route_of in ROUTES.items():
            h = Routed(entries, key_bytes, logit_bytes, games, rows, game_rows, merge)
            rng = np.random.default_rng(games * 7 + len(name))
            pool = _pool_keys(max(3, games * rows // 2) + 4, kw, seed=games + key_bytes)
            route = route_of(games)
            keys = _assigned(pool[:-4], h.total, rng)
            f1 = h.flush(keys, route)
            assert not f1.hit.any()
            f2 = h.flush(keys, route)
            if entries == 1024:
                assert f2.hit.all(), (games, name)
            h.flush(_assigned(pool, h.total, rng), route)
            if name in ("a", "b"):   # the other network's side saw nothing
                k = 0 if name == "b" else 1
                assert h.spec.stats[k] == dict.fromkeys(STATS, 0)
                assert h.empty(k)


# ---------------------------------------------------------------------------------------------
# 2. isolation: the test the feature stands on


@gpu
@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merge"])
@pytest.mark.parametrize("key_bytes,logit_bytes", [(24, 14), (72, 8192)])
def test_a_key_cached_for_one_network_misses_for_the_other(key_bytes, logit_bytes, merge):
    games = 20
    keys = _pool_keys(games, key_bytes // 8, seed=41)
    h = Routed(1024, key_bytes, logit_bytes, games, merge=merge)
    a, b = np.zeros(games, np.int32), np.ones(games, np.int32)
    h.flush(keys, a)
    assert h.stats()[0]["inserts"] == games and h.stats()[1] == dict.fromkeys(STATS, 0)
    assert h.empty(1)
    fb = h.flush(keys, b)                                  # the same keys under route B: every row misses
    assert not fb.hit.any() and fb.miss_rows(1) == set(range(games))
    s = h.stats()
    assert s[0] == dict(probed=games, hits=0, inserts=games, dropped=0, merged=0)
    assert s[1] == dict(probed=games, hits=0, inserts=games, dropped=0, merged=0)
    # each table now returns its own network's payload for the same key (flush checks the outputs)
    alt = (np.arange(games) % 2).astype(np.int32)
    assert h.flush(keys, alt).hit.all() and h.flush(keys, 1 - alt).hit.all()
    s = h.stats()
    assert s[0]["hits"] == s[1]["hits"] == games and s[0]["inserts"] == s[1]["inserts"] == games


# ---------------------------------------------------------------------------------------------
# 3. all-A: the unrouted calls


@gpu
@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merge"])
@pytest.mark.parametrize("rows,game_rows", [(1, 1), (3, 4)])
def test_all_a_routes_equal_the_unrouted_calls(rows, game_rows, merge):
    """Every route bit 0 (the high bits set): outputs and network A's counters are those of
    zc_evalcache_probe_async / _commit_async (with a scratch: the merged calls) on the same rows;
    table B stays all zeros past its epoch word, which every commit moves on, and count[1] is 0
    throughout."""
    from zeroclone_amd import _native
    kb, lb, games = 24, 14, 11
    h = Routed(1024, kb, lb, games, rows, game_rows, merge)
    n, total = h.n, h.total
    table = torch.zeros(_native.evalcache_bytes(1024, kb, lb)[0], dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(_native.evalcache_merge_scratch_bytes(n) // 4, dtype=torch.int32, device="cuda")
    miss = torch.zeros(n, dtype=torch.int32, device="cuda")
    dense = torch.zeros((n, kb), dtype=torch.uint8, device="cuda")
    tail = (scratch.data_ptr(),) if merge else ()
    probe, commit = (_native.evalcache_probe_merged, _native.evalcache_commit_merged) if merge else \
        (_native.evalcache_probe, _native.evalcache_commit)
    rng = np.random.default_rng(4)
    pool = _pool_keys(12, kb // 8, seed=6)
    route = np.full(games, 0x7FFFFFFE, np.int32)
    for i in range(3):
        keys = _assigned(pool[:8] if i < 2 else pool, total, rng) if i != 1 else keys
        h.flush(keys, route)
        keys_t = torch.from_numpy(keys.view(np.int64)).cuda()
        planes = keys_t.view(torch.uint8).view(total, kb).clone()
        out_v = torch.full((total,), -7.0, dtype=torch.float64, device="cuda")
        out_l = torch.full((total, lb), 0x5A, dtype=torch.uint8, device="cuda")
        probe(table.data_ptr(), 1024, kb, lb, n, rows, game_rows, keys_t.data_ptr(), planes.data_ptr(), kb,
              out_v.data_ptr(), out_l.data_ptr(), dense.data_ptr(), miss.data_ptr(), count.data_ptr(),
              stats.data_ptr(), *tail)
        dv, dl = dev_values(dense, 0), dev_logits(dense, 0, lb)
        commit(table.data_ptr(), 1024, kb, lb, n, rows, game_rows, keys_t.data_ptr(), miss.data_ptr(),
               count.data_ptr(), dv.data_ptr(), dl.data_ptr(), out_v.data_ptr(), out_l.data_ptr(), stats.data_ptr(),
               *tail)
        torch.cuda.synchronize()
        assert torch.equal(out_v, h.out_v.t) and torch.equal(out_l, h.out_l.t)
        got = h.stats()
        assert list(got[0].values()) == stats.cpu().tolist(), (i, got[0], stats)
        assert got[1] == dict.fromkeys(STATS, 0) and h.empty(1)


@gpu
def test_count_of_the_other_network_stays_zero_after_the_probe():
    h = Routed(1024, 24, 0, 11)
    keys = _pool_keys(11, 3, seed=2)
    keys_t = torch.from_numpy(keys.view(np.int64)).cuda()
    planes = keys_t.view(torch.uint8).view(11, 24).clone()
    for bit in (0, 1):
        route_t = torch.full((11,), bit | 0x40, dtype=torch.int32, device="cuda")
        h.probe(keys_t, planes, route_t)
        want = [11, 0] if bit == 0 else [0, 11]
        assert h.count.t.cpu().tolist() == want
        h.networks()
        h.commit(keys_t)
        assert h.count.t.cpu().tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------
# 4. merging


@gpu
@pytest.mark.parametrize("entries", [1024, 0])
@pytest.mark.parametrize("key_bytes,logit_bytes", [(24, 14), (72, 0)])
def test_duplicates_merge_within_a_network_and_never_across(key_bytes, logit_bytes, entries):
    """24 games over 4 keys, alternating networks: every key is pending six times, three times
    per network.  It is evaluated twice — once per network — and MERGED counts the other two rows
    of each network; then the same flush again on the same scratch (without tables it evaluates
    everything again; with them everything hits)."""
    games = 24
    pool = _pool_keys(4, key_bytes // 8, seed=8)
    keys = pool[np.arange(games) // 2 % 4]
    route = (np.arange(games) % 2).astype(np.int32)
    h = Routed(entries, key_bytes, logit_bytes, games, merge=True)
    for again in range(2):
        f = h.flush(keys, route)       # the outputs: every follower got its own network's payload
        if again and entries:
            assert f.hit.all()
            continue
        for k in range(2):
            assert len(f.groups[k]) == 4 and all(len(g) == 3 for g in f.groups[k])
    s = h.stats()
    for k in range(2):
        assert s[k]["merged"] == (8 if entries else 16) and s[k]["probed"] == 24
        assert s[k]["inserts"] == (4 if entries else 0)


# ---------------------------------------------------------------------------------------------
# 5. the refusals (no GPU)


def test_routed_entry_points_refuse_bad_arguments():
    """ZC_EINVAL before any launch: the pointers are never followed."""
    from zeroclone_amd import _native
    L, EINVAL = _native.lib(), _native.ZC_EINVAL
    P = ctypes.c_void_p
    good = dict(ta=0, tb=0, entries=0, key_bytes=24, logit_bytes=0, n_rows=8, rpg=1, gr=1, route=0x900, keys=0x1000,
                planes=0x2000, plane_bytes=168, out_v=0x3000, out_l=0, da=0x4000, db=0x4800, miss=0x5000,
                count=0x6000, stats=0x7000, scratch=0x8000, dva=0x9000, dvb=0x9800, dla=0, dlb=0)

    def probe(**kw):
        a = dict(good, **kw)
        return L.zc_evalcache_probe_routed_async(
            P(a["ta"] or None), P(a["tb"] or None), a["entries"], a["key_bytes"], a["logit_bytes"], a["n_rows"],
            a["rpg"], a["gr"], P(a["route"] or None), P(a["keys"] or None), P(a["planes"] or None), a["plane_bytes"],
            P(a["out_v"] or None), P(a["out_l"] or None), P(a["da"] or None), P(a["db"] or None),
            P(a["miss"] or None), P(a["count"] or None), P(a["stats"] or None), P(a["scratch"] or None), None)

    def commit(**kw):
        a = dict(good, **kw)
        return L.zc_evalcache_commit_routed_async(
            P(a["ta"] or None), P(a["tb"] or None), a["entries"], a["key_bytes"], a["logit_bytes"], a["n_rows"],
            a["rpg"], a["gr"], P(a["keys"] or None), P(a["miss"] or None), P(a["count"] or None),
            P(a["dva"] or None), P(a["dla"] or None), P(a["dvb"] or None), P(a["dlb"] or None),
            P(a["out_v"] or None), P(a["out_l"] or None), P(a["stats"] or None), P(a["scratch"] or None), None)

    bad = [dict(entries=64),                                  # entries without tables
           dict(ta=0x100, tb=0x10000),                        # tables of no entries
           dict(ta=0x100, entries=64),                        # one table alone
           dict(ta=0x100, tb=0x100, entries=64),              # one table twice
           dict(ta=0x108, tb=0x10000, entries=64),            # a table off its 16-byte alignment
           dict(key_bytes=20), dict(key_bytes=0), dict(key_bytes=520), dict(logit_bytes=7),
           dict(n_rows=-1), dict(rpg=0), dict(rpg=3, gr=2), dict(n_rows=8, rpg=3, gr=8),
           dict(n_rows=1 << 30, rpg=1, gr=2),                 # 2^31 buffer rows
           dict(count=0), dict(count=0x6002), dict(stats=0x7004), dict(scratch=0x8002),
           dict(keys=0), dict(keys=0x1004), dict(out_v=0x3004), dict(miss=0x5002), dict(miss=0),
           dict(logit_bytes=14)]                              # logits without their output pointer
    for kw in bad:
        assert probe(**kw) == EINVAL, ("probe", kw)
        assert commit(**kw) == EINVAL, ("commit", kw)
    for kw in (dict(plane_bytes=0), dict(plane_bytes=7), dict(planes=0), dict(planes=0x2001), dict(da=0), dict(db=0),
               dict(db=0x4000), dict(da=0x4001), dict(route=0), dict(route=0x902)):
        assert probe(**kw) == EINVAL, ("probe", kw)
    for kw in (dict(dva=0), dict(dvb=0), dict(dvb=0x9804), dict(logit_bytes=14, out_l=0xA000),
               dict(logit_bytes=14, out_l=0xA000, dla=0xB000), dict(logit_bytes=14, out_l=0xA000, dla=0xB000, dlb=0xC001)):
        assert commit(**kw) == EINVAL, ("commit", kw)
    # no rows: ZC_OK from the probe before any pointer is looked at; a NULL scratch is "no merging"
    cnt = (ctypes.c_int32 * 2)(0, 0)
    assert probe(n_rows=0, count=ctypes.addressof(cnt), route=0, keys=0, planes=0, out_v=0, da=0, db=0, miss=0,
                 stats=0, scratch=0) == 0
    # the Python wrappers refuse the same before the library is asked
    args = (0, 0, 0, 24, 0, 8, 1, 1, 0x900, 0x1000, 0x2000, 168, 0x3000, 0, 0x4000, 0x4800, 0x5000, 0x6000)
    with pytest.raises(ValueError):
        _native.evalcache_probe_routed(*args[:5], 8, 3, 8, *args[8:])          # n_rows no multiple of rows_per_game
    with pytest.raises(ValueError):
        _native.evalcache_probe_routed(*args[:8], 0, *args[9:])                # a null route
    with pytest.raises(ValueError):
        _native.evalcache_probe_routed(*args[:2], 64, *args[3:])               # entries without tables
    with pytest.raises(ValueError):
        _native.evalcache_probe_routed(*args[:11], 7, *args[12:])              # odd plane_bytes
    with pytest.raises(ValueError):
        _native.evalcache_probe_routed(*args[:15], 0x4000, *args[16:])         # one dense buffer twice
    with pytest.raises(ValueError):
        _native.evalcache_commit_routed(0, 0, 0, 24, 0, 8, 1, 1, 0x1000, 0x5000, 0x6000, 0x9000, 0, 0, 0, 0x3000, 0)
    with pytest.raises(ValueError):
        _native.evalcache_commit_routed(0, 0, 0, 20, 0, 8, 1, 1, 0x1000, 0x5000, 0x6000, 0x9000, 0, 0x9800, 0,
                                        0x3000, 0)


def test_routed_cache_refusals():
    from zeroclone_amd.evalcache import RoutedCachedPolicy, RoutedCachedValue, RoutedEvalCache
    from zeroclone_amd.nets import PolicyValueNetwork, ValueNetwork
    with pytest.raises(ValueError):
        RoutedEvalCache(0, 24)                      # no tables needs merge
    with pytest.raises(ValueError):
        RoutedEvalCache(64, 20)
    c = RoutedEvalCache(0, 24, merge=True)
    assert c.tables is None and c.merge and c.entries == 0
    with pytest.raises(ValueError, match="MfmaValueNetwork"):
        RoutedCachedValue(ValueNetwork(128, 1, in_planes=2), ValueNetwork(128, 1, in_planes=2), c)
    with pytest.raises(ValueError, match="MfmaPolicyValueNetwork"):
        RoutedCachedPolicy(PolicyValueNetwork(blocks=1), PolicyValueNetwork(blocks=1), RoutedEvalCache(64, 72, 8192))
