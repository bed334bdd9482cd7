"""The routed flush of the evaluation cache (csrc/evalcache.hip: zc_evalcache_probe_routed_async,
zc_evalcache_commit_routed_async; include/zeroclone.h "routed flush") in numpy: two tables of
tests/evalcache_ref.py's TableModel, one per network, and what a flush of MANY rows determines.

A probe is fully determined by the two tables: which rows hit, which miss, and — with merging —
which rows of one network hold one key (one of them leads, the kernels do not say which).  A
commit is not: which of several rows that want one way wins it is the hardware's choice.  So the
spec has two commits.  `commit_in_order` inserts the leading rows one after another, an outcome
the kernels may produce, and needs no device; `commit_observed` takes the tables the device left,
checks that they are an outcome the rules allow — every changed entry holds a key that missed, in
that key's set, under its tag and the launch's epoch; a key that missed and is not there had no
way to take — and adopts them.  Either way the counters are exact.  No GPU and no library."""
from __future__ import annotations

import numpy as np

import evalcache_ref as ref

STATS = ("probed", "hits", "inserts", "dropped", "merged")


def taking_part(n_games: int, rows_per_game: int, game_rows: int) -> np.ndarray:
    """The buffer rows of the taking-part rows 0 .. n_games * rows_per_game - 1."""
    r = np.arange(n_games * rows_per_game)
    return r // rows_per_game * game_rows + r % rows_per_game


class Flush:
    """A probe's outcome.  rows: the taking-part buffer rows; net[i]: the network of rows[i];
    hit[i]; groups[k]: the missing rows of network k as lists of buffer rows — without merging
    one row a list, with it the rows of one key together: the device's dense list of network k
    holds exactly one row of every list."""

    def __init__(self, rows, net, hit, groups):
        self.rows, self.net, self.hit, self.groups = rows, net, hit, groups

    def miss_rows(self, k: int) -> set:
        return {r for g in self.groups[k] for r in g}


class RoutedSpec:
    def __init__(self, entries: int, key_bytes: int, logit_bytes: int = 0, merge: bool = False):
        assert entries or merge, "no tables needs merging"
        self.merge, self.kw = merge, key_bytes // 8
        self.tables = [ref.TableModel(entries, key_bytes, logit_bytes) for _ in range(2)] if entries else None
        self.stats = [dict.fromkeys(STATS, 0) for _ in range(2)]

    def held(self, k: int) -> set:
        t = self.tables[k]
        return {tuple(int(w) for w in t.keys[e]) for e in np.flatnonzero(t.meta)}

    def probe(self, keys, route, rows_per_game: int, game_rows: int) -> Flush:
        """keys [buffer rows, kw] uint64, route [n_games] (bit 0 counts)."""
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1, self.kw)
        n_games = keys.shape[0] // game_rows
        rows = taking_part(n_games, rows_per_game, game_rows)
        net = (np.asarray(route).astype(np.int64)[rows // game_rows] & 1).astype(np.int64)
        hit = np.zeros(rows.size, bool)
        groups = [{}, {}]
        for i, (r, k) in enumerate(zip(rows.tolist(), net.tolist())):
            hit[i] = self.tables is not None and self.tables[k].probe(keys[r]) >= 0
            if not hit[i]:   # with merging equal keys of ONE network share a list; else every row its own
                groups[k].setdefault(tuple(int(w) for w in keys[r]) if self.merge else r, []).append(r)
        for k in range(2):
            s, mine = self.stats[k], net == k
            led = len(groups[k])
            s["probed"] += int(mine.sum())
            s["hits"] += int((hit & mine).sum())
            s["merged"] += int((~hit & mine).sum()) - led
        return Flush(rows, net, hit, [list(g.values()) for g in groups])

    def _count(self, k: int, led: int, inserts: int):
        if self.tables is not None:
            self.stats[k]["inserts"] += inserts
            self.stats[k]["dropped"] += led - inserts

    def commit_in_order(self, keys, flush: Flush):
        """The leading rows (each list's first) inserted one after another under one epoch."""
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1, self.kw)
        for k in range(2):
            inserts = 0
            if self.tables is not None:
                t = self.tables[k]
                epoch = t.epoch
                for g in flush.groups[k]:
                    inserts += t.commit(keys[g[0]]) >= 0
                    t.epoch = epoch        # one launch: TableModel.commit moved it on
                t.epoch = (epoch + 1) & 0xFFFFFFFF
            self._count(k, len(flush.groups[k]), inserts)

    def commit_observed(self, keys, flush: Flush, observed):
        """observed[k] = (epoch, meta [E] uint32, keys [E, kw] uint64) of table k after the
        commit.  Asserts that it is an outcome the commit's rules allow and adopts it."""
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1, self.kw)
        for k in range(2):
            if self.tables is None:
                self._count(k, len(flush.groups[k]), 0)
                continue
            t = self.tables[k]
            epoch, meta, tkeys = observed[k]
            assert int(epoch) == (t.epoch + 1) & 0xFFFFFFFF, (k, epoch, t.epoch)
            missed = {tuple(int(w) for w in keys[g[0]]) for g in flush.groups[k]}
            changed = np.flatnonzero((meta != t.meta) | (tkeys != t.keys).any(1))
            seen = set()
            for e in changed.tolist():
                key = tuple(int(w) for w in tkeys[e])
                assert key in missed and key not in seen, (k, e, "an entry changed to a key that did not miss, or twice")
                seen.add(key)
                h = ref.key_hash(np.asarray(key, np.uint64))
                assert int(ref.set_index(h, t.lay.sets)[0]) == e // ref.WAYS, (k, e, "outside the key's set")
                assert int(meta[e]) == (int(ref.tag(h)[0]) << 16) | (t.epoch & 0xFFFF), (k, e, "tag or epoch")
                assert not (t.meta[e] and (int(t.meta[e]) & 0xFFFF) == (t.epoch & 0xFFFF)), (k, e, "claimed twice")
            for key in missed - seen:   # a drop has a reason: the key's tag in its set, or no way to take
                h = ref.key_hash(np.asarray(key, np.uint64))
                e0 = int(ref.set_index(h, t.lay.sets)[0]) * ref.WAYS
                ways = meta[e0:e0 + ref.WAYS]
                assert ((ways >> 16) == int(ref.tag(h)[0])).any() or (ways != 0).all(), (k, key, "dropped with room")
            t.meta, t.keys, t.epoch = meta.copy(), tkeys.copy(), int(epoch)
            self._count(k, len(flush.groups[k]), len(seen))

    def identity(self):
        for s in self.stats:
            if self.tables is not None:
                assert s["probed"] == s["hits"] + s["merged"] + s["inserts"] + s["dropped"], s
            else:
                assert s["hits"] == s["inserts"] == s["dropped"] == 0 <= s["merged"] <= s["probed"], s
