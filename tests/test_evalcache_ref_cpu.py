"""tests/evalcache_ref.py itself: its finders meet the conditions that
tests/test_gpu_eval_cache_keys.py relies on (so no GPU case can come up empty), the table model
places and evicts as the header says, and the layout is the size formula's.  No GPU."""
import numpy as np
import pytest

import evalcache_ref as ref


def test_mix64_is_the_murmur3_finaliser():
    """Against Python's unbounded integers."""
    def one(x):
        m = (1 << 64) - 1
        x ^= x >> 33
        x = x * 0xff51afd7ed558ccd & m
        x ^= x >> 33
        x = x * 0xc4ceb9fe1a85ec53 & m
        return x ^ x >> 33
    xs = [0, 1, (1 << 64) - 1, 0x9E3779B97F4A7C15, 1 << 63, 0x0123456789ABCDEF]
    assert [int(v) for v in ref.mix64(np.array(xs, np.uint64))] == [one(x) for x in xs]
    assert int(ref.mix64(np.array([0], np.uint64))[0]) == 0

    def key_hash(words):
        m, acc = (1 << 64) - 1, 0
        for i, w in enumerate(words):
            acc ^= one((w + 0x9E3779B97F4A7C15 * (i + 1)) & m)
        return one(acc)
    keys = np.random.default_rng(1).integers(0, 1 << 64, (16, 9), dtype=np.uint64)
    keys[0], keys[1] = 0, np.uint64((1 << 64) - 1)
    h = ref.key_hash(keys)
    assert [int(v) for v in h] == [key_hash([int(w) for w in row]) for row in keys]
    for v in h:
        v = int(v)
        assert int(ref.tag(np.uint64(v))) == ((v >> 48) or 1)
        assert int(ref.set_index(np.uint64(v), 64)) == (v & 0xFFFFFFFF) & 63
        assert int(ref.victim_way(np.uint64(v))) == (v >> 32) & 7
        assert int(ref.claim_start(np.uint64(v), 2047)) == (v >> 24) & 2047


@pytest.mark.parametrize("sets", [1, 64])
@pytest.mark.parametrize("kw", [1, 3, 9, 64])
def test_colliding_pairs_differ_in_one_word_and_share_set_and_tag(kw, sets):
    for j in range(kw):
        a, b = ref.colliding_pairs(kw, j, sets, 8)
        assert a.shape == b.shape == (8, kw) and a.dtype == b.dtype == np.uint64
        diff = a != b
        assert diff[:, j].all() and diff.sum() == 8                     # word j and no other
        assert len({tuple(r) for r in np.concatenate([a, b]).tolist()}) == 16
        ha, hb = ref.key_hash(a), ref.key_hash(b)
        assert (ha != hb).all()
        assert np.array_equal(ref.tag(ha), ref.tag(hb))
        assert np.array_equal(ref.set_index(ha, sets), ref.set_index(hb, sets))
        a2, _ = ref.colliding_pairs(kw, j, sets, 8)
        assert np.array_equal(a, a2)                                    # deterministic


@pytest.mark.parametrize("sets", [1, 64])
@pytest.mark.parametrize("kw", [3, 9])
def test_raw_tags_0_and_1_in_one_set(kw, sets):
    k0, k1 = ref.raw_tag_pair(kw, sets)
    h0, h1 = ref.key_hash(k0), ref.key_hash(k1)
    assert int(h0[0]) >> 48 == 0 and int(h1[0]) >> 48 == 1
    assert int(ref.tag(h0)[0]) == int(ref.tag(h1)[0]) == 1              # the remap 0 -> 1
    assert int(ref.set_index(h0, sets)[0]) == int(ref.set_index(h1, sets)[0])
    assert not np.array_equal(k0, k1)


def test_key_with_raw_tag_for_the_shortest_key():
    for t in (0, 1):
        k = ref.key_with_raw_tag(1, t)
        assert k.shape == (1,) and int(ref.key_hash(k)[0]) >> 48 == t


def _distinct_tag_keys(n, kw, seed):
    keys = np.random.default_rng(seed).integers(0, 1 << 64, (4 * n, kw), dtype=np.uint64)
    _, first = np.unique(ref.tag(ref.key_hash(keys)), return_index=True)
    keys = keys[np.sort(first)[:n]]
    assert len(keys) == n
    return keys


@pytest.mark.parametrize("kw", [3, 9])
def test_table_model_fills_the_ways_in_order_then_evicts_the_victim_way(kw):
    m = ref.TableModel(8, 8 * kw, 16)
    keys = _distinct_tag_keys(9, kw, seed=kw)
    tags = ref.tag(ref.key_hash(keys))
    for i in range(8):
        assert m.flush(keys[i], i) == (-1, i)                           # ways 0..7 in order
        assert int(m.meta[i]) == int(tags[i]) << 16 | i                 # tag << 16 | epoch
    assert m.used_entries() == 8 and m.epoch == 8
    assert m.flush(keys[3], "again") == (3, -1) and m.payload[3] == 3   # a hit writes nothing
    v = int(ref.victim_way(ref.key_hash(keys[8:9]))[0])
    assert m.flush(keys[8], 8) == (-1, v)                               # the 9th key: the victim way
    assert int(m.meta[v]) == int(tags[8]) << 16 | 9 and np.array_equal(m.keys[v], keys[8])
    assert m.probe(keys[v]) == -1 and m.probe(keys[8]) == v             # the evicted key stops hitting
    assert m.stats == {"probed": 12, "hits": 2, "inserts": 9, "dropped": 0}


def test_table_model_drops_a_key_whose_tag_a_way_carries():
    a, b = ref.colliding_pairs(3, 2, 1, 8)
    m = ref.TableModel(8, 24)
    assert m.flush(a[0], "a") == (-1, 0)
    assert m.flush(b[0], "b") == (-1, -1)                               # same tag, other key: no hit, dropped
    assert m.used_entries() == 1 and m.probe(a[0]) == 0 and m.probe(b[0]) == -1
    assert m.stats == {"probed": 4, "hits": 1, "inserts": 1, "dropped": 1}
    assert m.epoch == 2                                                 # a commit launch moves it, dropped or not


def test_table_model_epoch_half_wraps_and_zero_is_not_empty():
    m = ref.TableModel(8, 24, epoch=0xFFFE)
    keys = _distinct_tag_keys(4, 3, seed=5)
    tags = ref.tag(ref.key_hash(keys))
    for i in range(4):
        m.flush(keys[i], i)
    assert [int(x) & 0xFFFF for x in m.meta[:4]] == [0xFFFE, 0xFFFF, 0, 1]
    assert int(m.meta[2]) == int(tags[2]) << 16 != 0 and m.used_entries() == 4
    assert m.probe(keys[2]) == 2 and m.epoch == 0x10002


@pytest.mark.parametrize("entries,sets", [(8, 1), (15, 1), (16, 2), (8192, 1024), (1 << 14, 2048), (1000, 64)])
@pytest.mark.parametrize("key_bytes", [8, 24, 72, 512])
@pytest.mark.parametrize("logit_bytes", [0, 2, 14, 16, 28, 8192])
def test_layout_is_the_size_formula(entries, sets, key_bytes, logit_bytes):
    lay = ref.layout(entries, key_bytes, logit_bytes)
    E = 8 * sets
    r16 = (logit_bytes + 15) // 16 * 16
    assert lay.sets == sets and lay.entries == E and lay.lstride == r16
    assert lay.bytes == 64 + E * (4 + key_bytes + 8 + r16)
    assert (lay.epoch, lay.meta) == (0, 64)
    assert lay.keys - lay.meta == 4 * E and lay.values - lay.keys == key_bytes * E
    assert lay.logits - lay.values == 8 * E and lay.bytes - lay.logits == r16 * E
    assert all(off % 16 == 0 for off in (lay.meta, lay.keys, lay.values, lay.logits))


def test_layout_agrees_with_the_library():
    """zc_evalcache_bytes needs no device."""
    from zeroclone_amd import _native
    for entries in (8, 100, 8192, 1 << 14):
        for kb, lb in ((8, 0), (24, 14), (72, 8192), (512, 28)):
            lay = ref.layout(entries, kb, lb)
            assert _native.evalcache_bytes(entries, kb, lb) == (lay.bytes, lay.sets)
