"""tests/evalcache_routed_ref.py, the numpy spec of the routed flush, checked against itself and
against tests/evalcache_ref.py's one-table model: rows of one network behave as the unrouted spec
on that network's table, equal keys under different route bits never merge and never hit each
other's table, and the counters add up per network.  No GPU."""
import numpy as np
import pytest

import evalcache_ref as ref
from evalcache_routed_ref import STATS, RoutedSpec, taking_part


def _keys(n, kw, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, (n, kw), dtype=np.uint64)


def test_taking_part_rows():
    assert taking_part(3, 1, 1).tolist() == [0, 1, 2]
    assert taking_part(2, 3, 4).tolist() == [0, 1, 2, 4, 5, 6]
    assert taking_part(2, 4, 8).tolist() == [0, 1, 2, 3, 8, 9, 10, 11]


@pytest.mark.parametrize("net", [0, 1])
@pytest.mark.parametrize("entries,kw", [(8, 3), (64, 9)])
def test_rows_of_one_network_behave_as_the_unrouted_spec_on_its_table(net, entries, kw):
    """Flushes of one row each, where TableModel is exact: the same hits, the same entries, the
    same counters; the other network's table and counters stay untouched."""
    spec, one = RoutedSpec(entries, 8 * kw), ref.TableModel(entries, 8 * kw)
    pool = _keys(24, kw, seed=entries + kw)   # more keys than an 8-entry table holds: evictions
    order = np.random.default_rng(5).integers(0, 24, 120)
    for i in order:
        key = pool[i][None]
        f = spec.probe(key, [net | 6], 1, 1)            # the high bits are ignored
        hit, _ = one.flush(pool[i], None)
        assert bool(f.hit[0]) == (hit >= 0) and f.net.tolist() == [net]
        assert f.miss_rows(net) == (set() if hit >= 0 else {0}) and not f.miss_rows(1 - net)
        spec.commit_in_order(key, f)
        t = spec.tables[net]
        assert np.array_equal(t.meta, one.meta) and np.array_equal(t.keys, one.keys) and t.epoch == one.epoch
    assert {k: spec.stats[net][k] for k in one.stats} == one.stats and one.stats["hits"] > 0
    assert spec.stats[net]["merged"] == 0
    assert spec.stats[1 - net] == dict.fromkeys(STATS, 0) and not spec.tables[1 - net].meta.any()
    spec.identity()


@pytest.mark.parametrize("merge", [False, True])
def test_equal_keys_under_different_route_bits_never_meet(merge):
    """12 games of one key each, 3 distinct keys, alternating networks."""
    kw = 3
    keys = _keys(3, kw, seed=1)[np.arange(12) % 3]
    route = np.arange(12) % 2
    spec = RoutedSpec(1024, 8 * kw, merge=merge)
    f = spec.probe(keys, route, 1, 1)
    assert not f.hit.any()
    for k in range(2):
        rows = sorted(f.miss_rows(k))
        assert rows == [r for r in range(12) if r % 2 == k]
        # with merging the two rows of a key and a network share a list; never a row of the other network
        assert len(f.groups[k]) == (3 if merge else 6)
        assert all(len({tuple(keys[r]) for r in g}) == 1 and {route[r] for r in g} == {k} for g in f.groups[k])
        assert spec.stats[k]["merged"] == (3 if merge else 0)
    spec.commit_in_order(keys, f)
    assert spec.held(0) == spec.held(1) == {tuple(int(w) for w in k) for k in keys[:3]}
    spec.identity()
    # network A's rows alone again: they hit A's table; then a key only A holds misses under B
    only_a = RoutedSpec(1024, 8 * kw, merge=merge)
    fa = only_a.probe(keys, np.zeros(12, int), 1, 1)
    only_a.commit_in_order(keys, fa)
    assert not only_a.held(1)
    fb = only_a.probe(keys, np.ones(12, int), 1, 1)
    assert not fb.hit.any() and len(fb.miss_rows(1)) == 12 and only_a.stats[1]["hits"] == 0
    only_a.commit_in_order(keys, fb)
    assert only_a.probe(keys, route, 1, 1).hit.all()
    only_a.identity()


@pytest.mark.parametrize("entries,merge", [(8, False), (8, True), (1024, False), (1024, True), (0, True)])
def test_counters_add_up_per_network(entries, merge):
    kw, games, rpg, gr = 3, 11, 3, 4
    spec = RoutedSpec(entries, 8 * kw, merge=merge)
    rng = np.random.default_rng(3)
    for flush in range(6):
        keys = _keys(14, kw, seed=9)[rng.integers(0, 14, games * gr)]
        route = rng.integers(0, 1 << 20, games)
        f = spec.probe(keys, route, rpg, gr)
        assert f.rows.size == games * rpg and all(r % gr < rpg for r in f.rows)
        spec.commit_in_order(keys, f)
        spec.identity()
    assert sum(s["probed"] for s in spec.stats) == 6 * games * rpg
    if entries:
        assert all(s["hits"] > 0 for s in spec.stats)
    if merge:
        assert all(s["merged"] > 0 for s in spec.stats)
    if entries == 8:
        assert any(s["dropped"] > 0 for s in spec.stats)


def test_commit_observed_refuses_what_the_rules_forbid():
    kw = 3
    keys = _keys(4, kw, seed=2)
    spec = RoutedSpec(64, 8 * kw)
    f = spec.probe(keys, [0, 0, 1, 1], 1, 1)
    twin = RoutedSpec(64, 8 * kw)
    twin.commit_in_order(keys, twin.probe(keys, [0, 0, 1, 1], 1, 1))
    good = [(t.epoch, t.meta.copy(), t.keys.copy()) for t in twin.tables]
    swapped = [good[1], good[0]]                       # each table holds the other network's keys
    with pytest.raises(AssertionError):
        spec.commit_observed(keys, f, swapped)
    empty = [(1, np.zeros_like(good[0][1]), np.zeros_like(good[0][2]))] * 2   # dropped with room
    with pytest.raises(AssertionError):
        RoutedSpec(64, 8 * kw).commit_observed(keys, f, empty)
    spec2 = RoutedSpec(64, 8 * kw)
    spec2.commit_observed(keys, spec2.probe(keys, [0, 0, 1, 1], 1, 1), good)
    assert spec2.stats == twin.stats and spec2.probe(keys, [0, 0, 1, 1], 1, 1).hit.all()
