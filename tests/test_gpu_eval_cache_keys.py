"""The evaluation cache's one sentence (include/zeroclone.h): A HIT IS FULL-KEY EQUALITY, the
16-bit tag only pre-filters — and the merged flush's "every key word equal".  Random keys almost
never reach the key comparison (same set AND same tag), so these tests build the keys that do,
with tests/evalcache_ref.py: the table's hash, layout and one-row behaviour in plain integers.

  a. the spec's hash is the device's (what keeps the rest honest)
  b. same set, same tag, another key: no hit — every word index, the tag remap 0 -> 1
  c. the probe goes on to the next way with the same tag (a table written by hand)
  d. placement and eviction against the model, flush by flush
  e. the epoch's 16-bit wrap, and a full set whose victim carries the running epoch's low half
  f. the merge compares every word
  g. the copies' four access widths and misaligned base pointers
  h. real rows that differ outside the board (chess word 8, Connect4's turn) through CachedValue

Everything is bit-exact.  Every device buffer a kernel writes has guard bytes on either side;
the fake network is a torch function of the dense planes that does not depend on the batch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import evalcache_ref as ref
from test_gpu_eval_cache import _c4_roots, _value_model
from test_gpu_eval_merge import GUARD, STATS, _Guarded

gpu = pytest.mark.gpu
pytestmark = gpu


# ---------------------------------------------------------------------------------------------
# helpers


def _dev_keys(keys):
    """uint64 [n, kw] -> the device key buffer (int64, 8-byte aligned)."""
    return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64).copy()).cuda()


def _planes(ids, plane_bytes, seed=0):
    """uint8 [n, plane_bytes]: position ids[i]'s planes — its id in bytes 0..1, then bytes that
    depend on the id alone."""
    tbl = np.random.default_rng(1234 + seed).integers(0, 256, (1024, plane_bytes), dtype=np.uint8)
    tbl[:, 0] = np.arange(1024) & 255
    tbl[:, 1] = np.arange(1024) >> 8
    return torch.from_numpy(tbl[np.asarray(ids, np.int64)]).cuda()


def _net_values(planes):
    """The fake network's value: the id, plus the other bytes' sum / 2^20 — exact in fp64 and
    different for different positions."""
    p = planes.double()
    return p[:, 0] + 256.0 * p[:, 1] + p[:, 2:].sum(1) / 2.0 ** 20


def _net_logits(planes, logit_bytes):
    """Byte j of a row's logits is byte j % plane_bytes of its planes, plus j."""
    j = torch.arange(logit_bytes, device="cuda")
    return (planes[:, j % planes.shape[1]] + j.to(torch.uint8)[None]).contiguous()


class _Bytes:
    """n bytes that start `off` bytes past a 16-byte boundary, with guard bytes on either side."""

    def __init__(self, n, off=0, fill=0):
        self.buf = torch.zeros(GUARD + off + n + GUARD, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.buf[:self.lo] = 0xA5
        self.buf[self.hi:] = 0x5A
        self.t = self.buf[self.lo:self.hi]
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == off

    def intact(self):
        return bool((self.buf[:self.lo] == 0xA5).all()) and bool((self.buf[self.hi:] == 0x5A).all())


class _Tab:
    """A table in a guarded buffer, read and written through the spec's layout, with the miss
    count and the five counters; entries 0: no table (the merged calls)."""

    def __init__(self, entries, key_bytes, logit_bytes):
        from zeroclone_amd import _native
        self.nat, self.sizes = _native, (entries, key_bytes, logit_bytes)
        self.kw, self.lb = key_bytes // 8, logit_bytes
        self.mem = self.lay = None
        if entries:
            self.lay = ref.layout(*self.sizes)
            assert _native.evalcache_bytes(*self.sizes) == (self.lay.bytes, self.lay.sets)
            self.mem = _Guarded((self.lay.bytes,), torch.uint8)
        self.count = _Guarded((1,), torch.int32)
        self.stats_t = _Guarded((5,), torch.int64)

    @property
    def ptr(self):
        return self.mem.t.data_ptr() if self.mem is not None else 0

    def clear(self):
        self.nat.evalcache_clear(self.ptr, *self.sizes)
        torch.cuda.synchronize()

    def stats(self):
        return dict(zip(STATS, (int(x) for x in self.stats_t.t.cpu())))

    def _np(self, lo, n, dtype):
        return self.mem.t[lo:lo + n].cpu().numpy().view(dtype)

    def epoch(self):
        return int(self._np(self.lay.epoch, 4, np.uint32)[0])

    def set_epoch(self, v):
        self.mem.t[self.lay.epoch:self.lay.epoch + 4].view(torch.int32)[0] = int(v)

    def meta(self):
        return self._np(self.lay.meta, 4 * self.lay.entries, np.uint32)

    def keys(self):
        return self._np(self.lay.keys, 8 * self.kw * self.lay.entries, np.uint64).reshape(-1, self.kw)

    def values(self):
        return self._np(self.lay.values, 8 * self.lay.entries, np.float64)

    def logits(self):
        return self._np(self.lay.logits, self.lay.lstride * self.lay.entries, np.uint8).reshape(-1, self.lay.lstride)

    def used_entries(self):
        return int((self.meta() != 0).sum())

    def write(self, entry, meta, key, value, logits):
        """An entry by hand, inside the table's block."""
        L = self.lay
        assert 0 <= entry < L.entries and len(key) == self.kw and len(logits) == self.lb

        def put(lo, a):
            b = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
            assert 0 <= lo and lo + b.numel() <= L.bytes
            self.mem.t[lo:lo + b.numel()] = b
        put(L.meta + 4 * entry, np.array([meta], np.uint32))
        put(L.keys + 8 * self.kw * entry, np.asarray(key, np.uint64))
        put(L.values + 8 * entry, np.array([value], np.float64))
        put(L.logits + L.lstride * entry, np.asarray(logits, np.uint8))

    def intact(self):
        return all(g.intact() for g in (self.mem, self.count, self.stats_t) if g is not None)


class _Rows:
    """The buffers of flushes of n rows (rows_per_game = game_rows = 1) on a _Tab, all guarded;
    merged: the merged calls.  offs: the byte offsets from a 16-byte boundary of d_planes,
    d_dense_planes, d_out_logits and d_dense_logits."""

    def __init__(self, tab, n, plane_bytes, merged=False, offs=(0, 0, 0, 0)):
        self.tab, self.n, self.pb, self.merged, self.lb = tab, n, plane_bytes, merged, tab.lb
        self.planes = _Bytes(n * plane_bytes, offs[0])
        self.dense = _Bytes(n * plane_bytes, offs[1])
        self.out_l = _Bytes(n * self.lb, offs[2]) if self.lb else None
        self.dl = _Bytes(n * self.lb, offs[3]) if self.lb else None
        self.out_v = _Guarded((n,), torch.float64)
        self.dv = _Guarded((n,), torch.float64)
        self.miss = _Guarded((n,), torch.int32)
        self.scratch = _Guarded((tab.nat.evalcache_merge_scratch_bytes(n) // 4,), torch.int32) if merged else None

    def intact(self):
        return self.tab.intact() and all(g.intact() for g in vars(self).values() if isinstance(g, (_Guarded, _Bytes)))

    def _ptr(self, g):
        return g.t.data_ptr() if g is not None else 0

    def _dense(self):
        return self.dense.t.view(self.n, self.pb)

    def _delta(self, before):
        return {k: v - before[k] for k, v in self.tab.stats().items()}

    def probe(self, keys, planes):
        """The probe launch with fresh sentinels, and what every probe must do: the count, the
        packed miss rows and their planes, hits' and non-hits' output slots, the counters.
        -> missed (buffer rows in dense order), hit (rows), out_v / out_l (copies), d (deltas)."""
        t, n = self.tab, self.n
        assert keys.shape == (n, t.kw) and planes.shape == (n, self.pb) and planes.dtype == torch.uint8
        self.planes.t.view(n, self.pb).copy_(planes)
        self.out_v.t.fill_(-7.0)
        self.miss.t.fill_(-1)
        self.dense.t.fill_(0xC3)
        if self.lb:
            self.out_l.t.fill_(0x5A)
        before = t.stats()
        args = (t.ptr, *t.sizes, n, 1, 1, keys.data_ptr(), self._ptr(self.planes), self.pb, self._ptr(self.out_v),
                self._ptr(self.out_l), self._ptr(self.dense), self._ptr(self.miss), self._ptr(t.count),
                self._ptr(t.stats_t))
        if self.merged:
            t.nat.evalcache_probe_merged(*args, self._ptr(self.scratch))
        else:
            t.nat.evalcache_probe(*args)
        torch.cuda.synchronize()
        k = int(t.count.t.item())
        assert 0 <= k <= n
        miss = self.miss.t.cpu().numpy()
        assert (miss[k:] == -1).all()
        led = miss[:k].astype(np.int64)
        assert len(set(led.tolist())) == k and ((led >= 0) & (led < n)).all()
        mi = torch.from_numpy(led).cuda()
        assert torch.equal(self._dense()[:k], planes[mi])              # the misses' planes, packed
        assert bool((self._dense()[k:] == 0xC3).all())
        out_v = self.out_v.t.clone()
        out_l = self.out_l.t.view(n, self.lb).clone() if self.lb else None
        hit = np.flatnonzero((out_v != -7.0).cpu().numpy()).tolist()   # the fake values are >= 0
        assert not set(hit) & set(led.tolist())
        cold = torch.ones(n, dtype=torch.bool, device="cuda")
        cold[hit] = False
        if self.lb:
            assert bool((out_l[cold] == 0x5A).all())                   # a row that did not hit: slots untouched
        d = self._delta(before)
        assert d["probed"] == n and d["hits"] == len(hit) and d["inserts"] == d["dropped"] == 0, d
        assert d["merged"] == (n - len(hit) - k if self.merged else 0), d
        assert self.intact()
        return SimpleNamespace(missed=led.tolist(), hit=hit, out_v=out_v, out_l=out_l, d=d)

    def commit(self, keys):
        """The fake network on the whole dense buffer (a launch cannot know the count), then the
        commit.  -> the counters' deltas."""
        t, n = self.tab, self.n
        before = t.stats()
        self.dv.t.copy_(_net_values(self._dense()))
        if self.lb:
            self.dl.t.view(n, self.lb).copy_(_net_logits(self._dense(), self.lb))
        args = (t.ptr, *t.sizes, n, 1, 1, keys.data_ptr(), self._ptr(self.miss), self._ptr(t.count),
                self._ptr(self.dv), self._ptr(self.dl), self._ptr(self.out_v), self._ptr(self.out_l),
                self._ptr(t.stats_t))
        if self.merged:
            t.nat.evalcache_commit_merged(*args, self._ptr(self.scratch))
        else:
            t.nat.evalcache_commit(*args)
        torch.cuda.synchronize()
        assert int(t.count.t.item()) == 0
        if self.merged:
            assert bool((self.scratch.t[:-n] == 0).all())
        d = self._delta(before)
        assert d["probed"] == d["hits"] == d["merged"] == 0, d
        assert self.intact()
        return d

    def outputs_are_own(self, planes, rows=None):
        """Every row (or `rows`) holds what evaluating the row itself gives."""
        idx = torch.arange(self.n, device="cuda") if rows is None else torch.as_tensor(rows, device="cuda")
        assert torch.equal(self.out_v.t[idx], _net_values(planes)[idx])
        if self.lb:
            assert torch.equal(self.out_l.t.view(self.n, self.lb)[idx], _net_logits(planes, self.lb)[idx])

    def flush(self, keys, planes):
        """probe -> network -> commit; every row ends with its own output.  -> (probe's result,
        the whole flush's deltas)."""
        p = self.probe(keys, planes)
        c = self.commit(keys)
        self.outputs_are_own(planes)
        d = {k: p.d[k] + c[k] for k in c}
        if self.tab.mem is not None:
            assert d["probed"] == d["hits"] + d["merged"] + d["inserts"] + d["dropped"], d
            assert c["inserts"] + c["dropped"] == len(p.missed), (c, p.missed)
        else:
            assert d["hits"] == d["inserts"] == d["dropped"] == 0, d
        return p, d


def _distinct_tag_keys(n, kw, seed, sets=1):
    """n random keys, no two of one set with the same tag."""
    keys = np.random.default_rng(seed).integers(0, 1 << 64, (4 * n, kw), dtype=np.uint64)
    h = ref.key_hash(keys)
    _, first = np.unique(ref.set_index(h, sets) << 16 | ref.tag(h).astype(np.int64), return_index=True)
    assert len(first) >= n
    return keys[np.sort(first)[:n]]


def _same_table(tab, model):
    """The device table's meta and key arrays are the model's, way for way."""
    assert np.array_equal(tab.meta(), model.meta), (tab.meta(), model.meta)
    assert np.array_equal(tab.keys(), model.keys)
    assert tab.epoch() == model.epoch


def _payloads_match(tab, model, plane_bytes):
    """Every used entry's value and logits are those of the position the model keeps there."""
    used = np.flatnonzero(model.meta)
    pl = _planes([model.payload[e] for e in used], plane_bytes)
    assert np.array_equal(tab.values()[used], _net_values(pl).cpu().numpy())
    if tab.lb:
        assert np.array_equal(tab.logits()[used, :tab.lb], _net_logits(pl, tab.lb).cpu().numpy())


PB = 8   # plane bytes of the tests that are not about the copies


# ---------------------------------------------------------------------------------------------
# a. the spec's hash is the device's


def _placement_keys(kw, sets, n=256):
    """All-zero, all-ones, single bits of the first and the last word, then random keys; a key
    that would be a set's ninth or share a tag within its set is left out (by the spec)."""
    one = np.uint64(1)
    cand = [np.zeros(kw, np.uint64), np.full(kw, np.uint64((1 << 64) - 1))]
    for w in sorted({0, kw - 1}):
        for b in (0, 1, 15, 16, 31, 32, 33, 47, 48, 62, 63):
            k = np.zeros(kw, np.uint64)
            k[w] = one << np.uint64(b)
            cand.append(k)
    cand = np.concatenate([np.array(cand), np.random.default_rng(kw).integers(0, 1 << 64, (2 * n, kw), dtype=np.uint64)])
    h = ref.key_hash(cand)
    s, t = ref.set_index(h, sets), ref.tag(h)
    seen, keep = {}, []
    for i in range(len(cand)):
        tags = seen.setdefault(int(s[i]), set())
        if len(tags) < ref.WAYS and int(t[i]) not in tags and len(keep) < n:
            tags.add(int(t[i]))
            keep.append(i)
    assert len(keep) == n and keep[:3] == [0, 1, 2]
    assert len({tuple(r) for r in cand[keep].tolist()}) == n
    return cand[keep]


@pytest.mark.parametrize("key_bytes", [8, 24, 72, 512])
def test_one_flush_places_every_key_where_the_spec_does(key_bytes):
    kw, lb, n = key_bytes // 8, 16, 256
    tab = _Tab(4096, key_bytes, lb)
    assert tab.lay.sets == 512
    tab.clear()
    keys = _placement_keys(kw, 512, n)
    planes = _planes(np.arange(n), PB)
    p, d = _Rows(tab, n, PB).flush(_dev_keys(keys), planes)
    assert sorted(p.missed) == list(range(n))
    assert d == {"probed": n, "hits": 0, "inserts": n, "dropped": 0, "merged": 0}
    h = ref.key_hash(keys)
    sets, tags = ref.set_index(h, 512), ref.tag(h)
    vals, lgs = _net_values(planes).cpu().numpy(), _net_logits(planes, lb).cpu().numpy()
    want = {}
    for i in range(n):
        want.setdefault(int(sets[i]), set()).add((int(tags[i]), tuple(keys[i].tolist()), float(vals[i]), lgs[i].tobytes()))
    meta, tk, tv, tl = tab.meta(), tab.keys(), tab.values(), tab.logits()
    assert ((meta & 0xFFFF) == 0).all() and tab.epoch() == 1           # a cleared table's first launch
    got = {}
    for e in np.flatnonzero(meta):
        got.setdefault(int(e) // ref.WAYS, set()).add((int(meta[e]) >> 16, tuple(tk[e].tolist()), float(tv[e]),
                                                       tl[e, :lb].tobytes()))
    assert len(np.flatnonzero(meta)) == n and got == want
    for s in want:                                                      # a set fills from way 0
        ways = meta[s * ref.WAYS:(s + 1) * ref.WAYS] != 0
        assert ways[:len(want[s])].all() and not ways[len(want[s]):].any()


# ---------------------------------------------------------------------------------------------
# b. same set, same tag, different key: no hit


def _no_hit_for_the_colliding_key(tab, one, two, a, b, ia, ib, stored_tag):
    """A in, then B — equal set, equal tag, another key — through one flush, then both in one."""
    kw, lb = tab.kw, tab.lb
    tab.clear()
    ka, kb = _dev_keys(a[None]), _dev_keys(b[None])
    pa, pb = _planes([ia], PB), _planes([ib], PB)
    p, d = one.flush(ka, pa)
    assert p.missed == [0] and d["inserts"] == 1
    e = int(ref.set_index(ref.key_hash(a), tab.lay.sets)[0]) * ref.WAYS
    meta = tab.meta()
    assert int(meta[e]) == stored_tag << 16 and tab.used_entries() == 1  # the predicted tag, epoch half 0
    assert stored_tag == int(ref.tag(ref.key_hash(b))[0])
    p = one.probe(kb, pb)                                                # B: its planes are in the dense buffer,
    assert p.missed == [0] and p.hit == [] and p.d["hits"] == 0          # its slots untouched (probe's checks)
    c = one.commit(kb)
    assert c["dropped"] == 1 and c["inserts"] == 0                       # the device saw the equal tag
    one.outputs_are_own(pb)
    assert tab.used_entries() == 1 and np.array_equal(tab.keys()[e], a)
    both, pl = _dev_keys(np.stack([a, b])), _planes([ia, ib], PB)
    p = two.probe(both, pl)
    assert p.hit == [0] and p.missed == [1]
    assert torch.equal(p.out_v[:1], _net_values(pl)[:1])                 # A's payload, bit for bit
    assert torch.equal(p.out_l[:1], _net_logits(pl, lb)[:1])
    c = two.commit(both)
    assert c["dropped"] == 1 and c["inserts"] == 0
    two.outputs_are_own(pl)


@pytest.mark.parametrize("sets", [1, 64])
@pytest.mark.parametrize("kw", [3, 9])
def test_a_key_that_differs_in_one_word_with_the_same_set_and_tag_does_not_hit(kw, sets):
    """Every word index, 8 pairs each; kw 9, word 8 is where zc_chess_state keeps turn, fifty and
    castle."""
    tab = _Tab(8 * sets, 8 * kw, 16)
    assert tab.lay.sets == sets
    one, two = _Rows(tab, 1, PB), _Rows(tab, 2, PB)
    for j in range(kw):
        a, b = ref.colliding_pairs(kw, j, sets, 8)
        for i in range(8):
            for x, y in ((a[i], b[i]), (b[i], a[i])) if i == 0 else ((a[i], b[i]),):
                _no_hit_for_the_colliding_key(tab, one, two, x, y, 2 * i, 2 * i + 1, int(ref.tag(ref.key_hash(x))[0]))


@pytest.mark.parametrize("sets", [1, 64])
@pytest.mark.parametrize("kw", [3, 9])
def test_raw_tag_0_is_stored_as_tag_1_and_a_raw_tag_1_key_of_the_set_misses(kw, sets):
    tab = _Tab(8 * sets, 8 * kw, 16)
    one, two = _Rows(tab, 1, PB), _Rows(tab, 2, PB)
    k0, k1 = ref.raw_tag_pair(kw, sets)
    assert int(ref.key_hash(k0)[0]) >> 48 == 0 and int(ref.key_hash(k1)[0]) >> 48 == 1
    _no_hit_for_the_colliding_key(tab, one, two, k0, k1, 10, 11, 1)     # stored with tag 1, hits; the other misses
    _no_hit_for_the_colliding_key(tab, one, two, k1, k0, 11, 10, 1)


# ---------------------------------------------------------------------------------------------
# c. the probe goes on to the next candidate


@pytest.mark.parametrize("merged", [False, True])
@pytest.mark.parametrize("key_bytes", [24, 72])
def test_probe_goes_on_to_the_next_way_with_the_same_tag(key_bytes, merged):
    """The commit never leaves two equal tags in a set, so the table is written by hand: way 2
    holds B, way 5 holds A, same tag; B differs from A in its last word only.  C has the tag and
    the set and is in neither way."""
    kw, lb, sets = key_bytes // 8, 16, 64
    tab = _Tab(8 * sets, key_bytes, lb)
    tab.clear()
    a, b, c = ref.colliding_groups(kw, kw - 1, sets, 1, 3)[0]
    h = ref.key_hash(np.stack([a, b, c]))
    assert len(set(ref.tag(h).tolist())) == 1 and len(set(ref.set_index(h, sets).tolist())) == 1
    assert (a[:-1] == b[:-1]).all() and a[-1] != b[-1]
    t, e0 = int(ref.tag(h)[0]), int(ref.set_index(h, sets)[0]) * ref.WAYS
    lg_b, lg_a = np.arange(16, dtype=np.uint8) + 0x20, np.arange(16, dtype=np.uint8) + 0x80
    tab.write(e0 + 2, t << 16 | 3, b, 2.25, lg_b)
    tab.write(e0 + 5, t << 16 | 6, a, 5.5, lg_a)
    tab.set_epoch(9)
    torch.cuda.synchronize()
    keys, planes = _dev_keys(np.stack([a, b, c, a])), _planes([1, 2, 3, 1], PB)
    r = _Rows(tab, 4, PB, merged=merged)
    p = r.probe(keys, planes)
    assert p.hit == [0, 1, 3] and p.missed == [2], (p.hit, p.missed)
    assert p.out_v.tolist()[:2] == [5.5, 2.25] and p.out_v[3].item() == 5.5
    assert p.out_l[0].cpu().numpy().tobytes() == lg_a.tobytes() == p.out_l[3].cpu().numpy().tobytes()
    assert p.out_l[1].cpu().numpy().tobytes() == lg_b.tobytes()
    d = r.commit(keys)
    assert d["dropped"] == 1 and d["inserts"] == 0                       # C: its tag is in the set
    r.outputs_are_own(planes, rows=[2])
    assert tab.used_entries() == 2 and tab.epoch() == 10


# ---------------------------------------------------------------------------------------------
# d. placement and eviction against the model


@pytest.mark.parametrize("key_bytes", [24, 72])
def test_one_set_places_and_evicts_as_the_model_does(key_bytes):
    kw, lb, n = key_bytes // 8, 16, 24
    tab, model = _Tab(8, key_bytes, lb), ref.TableModel(8, key_bytes, lb)
    tab.clear()
    keys = _distinct_tag_keys(n, kw, seed=key_bytes)
    one = _Rows(tab, 1, PB)
    for i in range(n):
        p, d = one.flush(_dev_keys(keys[i:i + 1]), _planes([i], PB))
        hit, entry = model.flush(keys[i], i)
        assert hit == -1 and entry >= 0 and p.missed == [0] and d["inserts"] == 1
        if i >= 8:
            assert entry == int(ref.victim_way(ref.key_hash(keys[i]))[0])
        _same_table(tab, model)                                          # way index and epoch half included
    _payloads_match(tab, model, PB)
    residents = sorted(model.payload[e] for e in range(8))
    assert len(set(residents)) == 8
    planes = _planes(np.arange(n), PB)
    p = _Rows(tab, n, PB).probe(_dev_keys(keys), planes)                 # evicted keys: missed, slots untouched
    for i in range(n):
        model.probe(keys[i])
    assert p.hit == residents and sorted(p.missed) == sorted(set(range(n)) - set(residents))
    hi = torch.tensor(residents, device="cuda")
    assert torch.equal(p.out_v[hi], _net_values(planes)[hi]) and torch.equal(p.out_l[hi], _net_logits(planes, lb)[hi])
    s = tab.stats()
    assert {k: s[k] for k in model.stats} == model.stats and s["merged"] == 0
    assert model.stats == {"probed": 2 * n, "hits": 8, "inserts": n, "dropped": 0}


# ---------------------------------------------------------------------------------------------
# e. the epoch's wrap


@pytest.mark.parametrize("sets", [1, 64])
@pytest.mark.parametrize("epoch0", [0xFFFE, 0x1FFFE])
def test_the_epoch_half_wraps_and_an_entry_of_epoch_half_0_is_not_empty(epoch0, sets):
    key_bytes, lb = 24, 16
    tab, model = _Tab(8 * sets, key_bytes, lb), ref.TableModel(8 * sets, key_bytes, lb, epoch=epoch0)
    tab.clear()
    tab.set_epoch(epoch0)
    keys = _distinct_tag_keys(5, 3, seed=epoch0 % 1000 + sets, sets=sets)
    one = _Rows(tab, 1, PB)
    order = [0, 1, 2, 3, 2, 4]                                           # key 2 goes in at epoch half 0
    for step, i in enumerate(order):
        p, d = one.flush(_dev_keys(keys[i:i + 1]), _planes([i], PB))     # outputs right, the counters' identity
        hit, entry = model.flush(keys[i], i)
        assert (p.hit == [0]) == (hit >= 0) == (step == 4), (step, p.hit, hit)   # no false hit, and the true one
        assert d["inserts"] == (entry >= 0) and d["dropped"] == 0
        _same_table(tab, model)
        if step == 2:
            e = entry
            assert int(tab.meta()[e]) == int(ref.tag(ref.key_hash(keys[2]))[0]) << 16   # tag << 16 | 0
        assert tab.used_entries() == model.used_entries() == min(step + 1, 4) + (step == 5)
    _payloads_match(tab, model, PB)
    assert int(tab.meta()[e]) & 0xFFFF == 0 and tab.epoch() == epoch0 + 6
    planes = _planes(np.arange(5), PB)
    p = _Rows(tab, 5, PB).probe(_dev_keys(keys), planes)
    assert p.hit == [0, 1, 2, 3, 4]
    assert torch.equal(p.out_v, _net_values(planes)) and torch.equal(p.out_l, _net_logits(planes, lb))
    s = tab.stats()
    assert (s["probed"], s["hits"], s["inserts"], s["dropped"]) == (11, 6, 5, 0)


def test_a_full_sets_victim_that_carries_the_running_epoch_half():
    """The entry victim_way picks was written 65536 commit launches ago, as far as its meta word
    tells.  The contract: the row gets its output, and the table either took the new key (the
    old one misses from now on) or dropped it (the old one still hits) — which of the two is not
    promised, and is printed here."""
    key_bytes, lb = 72, 16
    tab = _Tab(8, key_bytes, lb)
    tab.clear()
    keys = _distinct_tag_keys(9, 9, seed=41)
    one, two = _Rows(tab, 1, PB), _Rows(tab, 2, PB)
    for i in range(8):
        one.flush(_dev_keys(keys[i:i + 1]), _planes([i], PB))
    v = int(ref.victim_way(ref.key_hash(keys[8]))[0])
    meta = tab.meta()
    assert tab.used_entries() == 8 and (meta & 0xFFFF).tolist() == list(range(8))
    tab.set_epoch(0x10000 + (int(meta[v]) & 0xFFFF))
    p, d = one.flush(_dev_keys(keys[8:9]), _planes([8], PB))             # the row gets its output
    assert p.missed == [0] and d["inserts"] + d["dropped"] == 1
    pair, pl = _dev_keys(keys[[v, 8]]), _planes([v, 8], PB)
    p = two.probe(pair, pl)
    print(f"aliased epoch: {'inserted' if d['inserts'] else 'dropped'}")
    if d["inserts"]:
        assert p.hit == [1] and p.missed == [0] and np.array_equal(tab.keys()[v], keys[8])
    else:
        assert p.hit == [0] and p.missed == [1] and np.array_equal(tab.keys()[v], keys[v])
    assert torch.equal(p.out_v[p.hit], _net_values(pl)[p.hit]) and tab.used_entries() == 8
    assert tab.stats() == {"probed": 11, "hits": 1, "inserts": 8 + d["inserts"], "dropped": d["dropped"], "merged": 0}


# ---------------------------------------------------------------------------------------------
# f. the merge compares every word


def _one_word_keys(kw, j, n=256):
    """n keys that differ in word j only: there it holds the single bits and small counters."""
    words = [1 << b for b in range(64)]
    c = 0
    while len(words) < n:
        if c & (c - 1) or c == 0:          # not a single bit
            words.append(c)
        c += 1
    keys = np.tile(np.random.default_rng(100 * kw + j).integers(0, 1 << 64, kw, dtype=np.uint64), (n, 1))
    keys[:, j] = np.array(words, np.uint64)
    assert len({tuple(r) for r in keys.tolist()}) == n
    return keys


MERGE_WORDS = [(1, 0)] + [(3, j) for j in range(3)] + [(9, j) for j in range(9)] + [(64, j) for j in (0, 31, 62, 63)]


@pytest.mark.parametrize("entries", [1 << 14, 0])
@pytest.mark.parametrize("kw,j", MERGE_WORDS)
def test_rows_that_differ_in_one_word_do_not_merge(kw, j, entries):
    """256 keys twice, shuffled: 256 leaders, one per key, and 256 followers of their own key.
    kw 1: the shortest key; kw 64: a key word in every lane."""
    n, lb = 256, 16
    keys = _one_word_keys(kw, j, n)
    a = np.concatenate([np.arange(n), np.arange(n)])
    np.random.default_rng(kw + j).shuffle(a)
    tab = _Tab(entries, 8 * kw, lb)
    if entries:
        tab.clear()
    planes = _planes(a, PB)
    p, d = _Rows(tab, 2 * n, PB, merged=True).flush(_dev_keys(keys[a]), planes)   # every row: its own output
    assert len(p.missed) == n and sorted(a[p.missed].tolist()) == list(range(n))
    assert d["merged"] == n and d["hits"] == 0, d
    if entries:
        assert d["inserts"] + d["dropped"] == n


# ---------------------------------------------------------------------------------------------
# g. copy widths and alignment

# (logit_bytes, plane_bytes, offsets of d_planes / d_dense_planes / d_out_logits / d_dense_logits).
# wave_copy takes the widest access that divides the size and both addresses; a table entry's
# logits are 16-byte aligned, rows lie size bytes apart.
COPIES = [
    (2, 2, (0, 0, 0, 0)),      # both: the 2-byte path, by the size
    (4, 12, (0, 4, 8, 4)),     # both: the 4-byte path, by the size (bases 4-byte aligned)
    (12, 6, (4, 2, 2, 0)),     # logits: size 12 but d_out_logits at 2 -> the 2-byte path through a misaligned base;
                               # planes: the 2-byte path by the size
    (28, 168, (8, 0, 4, 8)),   # logits: the 4-byte path; planes: 168 = 8 * 21 at offsets 8 and 0 -> the 8-byte path
    (24, 168, (4, 8, 0, 8)),   # logits: the 8-byte path (24, bases at 0 and 8); planes: 168 with d_planes at 4 ->
                               # the 4-byte path through a misaligned base
    (24, 12, (2, 0, 8, 2)),    # logits: table -> d_out_logits by 8 bytes, d_dense_logits at 2 -> the scatter and the
                               # table's copy by 2; planes: size 12 with d_planes at 2 -> the 2-byte path
    # none of the sizes above is a multiple of 16, so two more select the 16-byte path and,
    # with the same sizes, the 8-byte path through bases at 8:
    (32, 32, (0, 0, 0, 0)),
    (32, 32, (8, 0, 0, 8)),
]


@pytest.mark.parametrize("logit_bytes,plane_bytes,offs", COPIES)
def test_copies_are_byte_exact_at_every_width_and_alignment(logit_bytes, plane_bytes, offs):
    """24 rows over 6 keys.  Merged: leaders' planes and scatter, followers' copies, then the
    table's logits read back by the hits of a second flush.  Plain: 24 scattered misses, then
    hits.  probe() and flush() compare every byte and every guard."""
    n, nk = 24, 6
    keys = _distinct_tag_keys(nk, 3, seed=logit_bytes + plane_bytes, sets=16)
    a = np.concatenate([np.arange(nk), np.random.default_rng(offs[0]).integers(0, nk, n - nk)])
    np.random.default_rng(7).shuffle(a)
    dk, planes = _dev_keys(keys[a]), _planes(a, plane_bytes, seed=plane_bytes)
    for merged in (True, False):
        tab = _Tab(128, 24, logit_bytes)
        tab.clear()
        r = _Rows(tab, n, plane_bytes, merged=merged, offs=offs)
        p, d = r.flush(dk, planes)
        if merged:
            assert len(p.missed) == nk and d["merged"] == n - nk and d["inserts"] == nk, d
        else:
            assert len(p.missed) == n and d["inserts"] == nk and d["dropped"] == n - nk, d
        pl6 = _planes(np.arange(nk), plane_bytes, seed=plane_bytes)   # the table's own bytes
        ent = [int(np.flatnonzero((tab.keys() == keys[i]).all(1) & (tab.meta() != 0))[0]) for i in range(nk)]
        assert np.array_equal(tab.logits()[ent, :logit_bytes], _net_logits(pl6, logit_bytes).cpu().numpy())
        assert np.array_equal(tab.values()[ent], _net_values(pl6).cpu().numpy())
        p, d = r.flush(dk, planes)                                     # every row hits: the stored logits
        assert p.hit == list(range(n)) and d["hits"] == n
        assert torch.equal(p.out_l, _net_logits(planes, logit_bytes)) and torch.equal(p.out_v, _net_values(planes))


# ---------------------------------------------------------------------------------------------
# h. real rows that differ outside the board


def _chess_rows():
    """16 zc_chess_state rows of one board: the base, the other side to move, five other castling
    rights, four other fifty-move counters (equal planes: the network does not see the counter),
    and five exact repeats.  -> (rows uint8 [16, 72], the number of distinct rows)."""
    from zeroclone_amd._native import CHESS_STATE_DTYPE, chess_from_fen
    base = chess_from_fen("r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1")
    rows = []

    def add(**kw):
        r = np.array(base, CHESS_STATE_DTYPE)
        for k, v in kw.items():
            r[k] = v
        rows.append(r)
    add()
    add(turn=1)
    for castle in (14, 13, 11, 7, 0):
        add(castle=castle)
    for fifty in (1, 2, 49, 255):
        add(fifty=fifty)
    add()
    add()
    add(turn=1)
    add(fifty=1)
    add(castle=0)
    a = np.array(rows, CHESS_STATE_DTYPE).view(np.uint8).reshape(16, 72)
    assert (a[:, :64] == a[0, :64]).all() and (a[:, 67:] == 0).all()    # they differ in key word 8 alone
    assert len({r.tobytes() for r in a}) == 11
    return a.copy(), 11


def _c4_rows():
    """20 zc_c4_state rows: 8 boards with either side to move (equal stones, another turn: the
    planes swap), and 4 repeats."""
    roots = _c4_roots().cpu().numpy()
    other = roots.copy()
    other[:, 2] ^= 1
    a = np.concatenate([roots, other, roots[:2], other[5:7]])
    assert (a[:8, :2] == a[8:16, :2]).all() and len({r.tobytes() for r in a}) == 16
    return a, 16


@pytest.mark.parametrize("mode", ["table", "table+merge", "merge"])
@pytest.mark.parametrize("game", ["chess", "c4"])
def test_rows_that_differ_outside_the_board_get_their_own_values(game, mode):
    """CachedValue as the searches call it, two flushes, against the plain MfmaValueNetwork on
    the same planes.  The counters: only the exact repeats are served from another row — a
    fifty-only variant is another key, although its output is equal."""
    from zeroclone_amd import learner
    from zeroclone_amd.evalcache import CachedValue, EvalCache
    from zeroclone_amd.nets import MfmaValueNetwork
    if game == "chess":
        rows, distinct = _chess_rows()
        leaves = torch.from_numpy(rows).cuda()
        planes = learner._chess_planes_torch(torch.from_numpy(rows)).half().cuda().contiguous()
        keys = rows.view(np.uint64)
        fifty = [0, 7, 8, 9, 10]                                        # the base and its fifty-only variants
        assert all(torch.equal(planes[0], planes[i]) for i in fifty)
    else:
        rows, distinct = _c4_rows()
        leaves = torch.from_numpy(rows).cuda()
        planes = learner._c4_planes_torch(torch.from_numpy(rows), None)[0].half().cuda().contiguous()
        keys = rows.view(np.uint64)
        assert not torch.equal(planes[3], planes[11])                   # (the empty board's are equal: rows 0 and 8)
    n, key_bytes = rows.shape[0], rows.shape[1] * rows.itemsize
    h = ref.key_hash(keys)
    uniq = {r.tobytes(): (int(s), int(t)) for r, s, t in zip(rows, ref.set_index(h, 512), ref.tag(h))}
    assert len(set(uniq.values())) == distinct                           # no two of them share set and tag
    net = MfmaValueNetwork(_value_model(17 if game == "chess" else 2, seed=61), "cuda")
    want = net(planes).clone()
    torch.cuda.synchronize()
    if game == "chess":
        assert len({want[i].item() for i in fifty}) == 1 and want[0].item() != want[1].item()
    cache = EvalCache(0 if mode == "merge" else 4096, key_bytes, 0, merge=mode != "table")
    fn = CachedValue(net, cache)
    got1 = fn(leaves, planes, None).clone()
    s1 = cache.stats()
    got2 = fn(leaves, planes, None).clone()
    s2 = cache.stats()
    assert torch.equal(got1, want) and torch.equal(got2, want)
    d2 = {k: s2[k] - s1[k] for k in s2}
    print(f"{game} {mode}: {s1} then {d2}")
    rep = n - distinct
    if mode == "table":
        assert s1 == {"probed": n, "hits": 0, "inserts": distinct, "dropped": rep}
        assert d2 == {"probed": n, "hits": n, "inserts": 0, "dropped": 0}
    elif mode == "table+merge":
        assert s1 == {"probed": n, "hits": 0, "inserts": distinct, "dropped": 0, "merged": rep}
        assert d2 == {"probed": n, "hits": n, "inserts": 0, "dropped": 0, "merged": 0}
    else:
        assert s1 == d2 == {"probed": n, "hits": 0, "inserts": 0, "dropped": 0, "merged": rep}
