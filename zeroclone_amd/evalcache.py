"""An evaluation cache for the network searches (include/zeroclone.h "evaluation cache",
csrc/evalcache.hip): a flush's rows whose position was evaluated before take the stored value
and logits, and the network runs on the others alone.

    probe -> network on the dense rows of the misses (a counted launch) -> commit

The key is the whole compact leaf row (zc_c4_state, zc_chess_state), and the planes are a
function of that row; the MFMA towers compute every board independently of its neighbours, so
a stored output is the computed one bit for bit and a search with the cache returns what the
search without it returns.  The miss count lives on the device and the network call takes it
there (nets.MfmaValueNetwork.tower's `count`), so the path has no host read and a whole move
can be captured in a HIP graph as before.

`CachedValue(net, cache)` stands where `valued.NetValue(net)` stands and `CachedPolicy(net,
cache)` where `valued.PolicyNet(net)` does.  Both need the leaf rows: allocate the search with
leaves=True.  One EvalCache belongs to one stream and to one set of weights: give every
stream's replica of the network a cache of its own, and `clear()` it when the weights change.

`EvalCache(..., merge=True)` runs the merged calls (zc_evalcache_probe_merged_async / ..._commit_
merged_async): among a flush's rows that miss the table, rows with an equal key are evaluated
once and the others take a copy.  With entries = 0 there is no table and merging is all the
cache does, at no memory beyond a few words a row.

`RoutedEvalCache` with `RoutedCachedValue(net_a, net_b, cache)` / `RoutedCachedPolicy(net_a, net_b,
cache)` is the same for an arena's two networks (arena.py): a table per network behind one routed
probe and one routed commit, each network counted on its own misses.  They stand where
valued.RoutedValue / RoutedPolicy stand, and take the route bits themselves (`set_route(key)`),
not a partition.
"""
from __future__ import annotations

import torch

from . import _native
from .nets import MfmaPolicyValueNetwork, MfmaValueNetwork


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


class _Cache:
    """An evaluation cache over K tables, K = 1 (EvalCache) or 2 (RoutedEvalCache, a table per
    network): the tables (zc_evalcache_*), a miss count and a row of counters per table, and per
    flush shape the dense buffers of the misses and, with merge, the scratch, all allocated at
    first use."""
    K: int
    COUNTERS: tuple   # the counters' shape; (): the cache's own stat names

    def __init__(self, entries: int, key_bytes: int, logit_bytes: int = 0, device="cuda", merge: bool = False):
        if merge:
            _native.evalcache_check_merged_sizes(entries, key_bytes, logit_bytes)
        else:
            _native.evalcache_check_sizes(entries, key_bytes, logit_bytes)
        self.entries, self.key_bytes, self.logit_bytes = int(entries), int(key_bytes), int(logit_bytes)
        self.merge = bool(merge)
        self._stat_names = _native.EVALCACHE_MERGED_STATS if merge else _native.EVALCACHE_STATS
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise ValueError("the evaluation cache lives on a GPU")
        self.tables = self.count = None    # allocated at first use
        self._bufs = {}

    def _sizes(self):
        return self.entries, self.key_bytes, self.logit_bytes

    def _ensure(self):
        if self.count is None:
            if torch.cuda.is_current_stream_capturing():   # the zero fill would be replayed with the graph
                raise RuntimeError("the evaluation cache must exist before a graph capture: call clear() first")
            if self.entries:
                nbytes, self.sets = _native.evalcache_bytes(*self._sizes())
                self.tables = tuple(torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)   # all zeros: empty
                                    for _ in range(self.K))
            self.count = torch.zeros(self.K, dtype=torch.int32, device=self.dev)
            self.counters = torch.zeros(self.COUNTERS or len(self._stat_names), dtype=torch.int64, device=self.dev)

    def _table_ptrs(self) -> tuple:
        return tuple(t.data_ptr() for t in self.tables) if self.tables is not None else (0,) * self.K

    def clear(self):
        """Empty the tables (stream-ordered; the counters keep counting).  Without tables (entries
        = 0) there is nothing to empty."""
        self._ensure()
        for t in self.tables or ():
            _native.evalcache_clear(t.data_ptr(), *self._sizes(), _stream(self.dev))

    def _stats(self) -> tuple:
        """A dict of the counters per table.  Synchronises."""
        self._ensure()
        return tuple(dict(zip(self._stat_names, (int(x) for x in row))) for row in self.counters.view(self.K, -1).cpu())

    def _scratch(self, n_rows: int) -> torch.Tensor:
        """The merged calls' scratch for flushes of n_rows rows: zeros at first, and every flush
        leaves it so."""
        return self._buf("merge", (_native.evalcache_merge_scratch_bytes(n_rows) // 4,), torch.int32)

    def _buf(self, name: str, shape: tuple, dtype) -> torch.Tensor:
        key = (name, tuple(shape), dtype)
        b = self._bufs.get(key)
        if b is None:
            b = self._bufs[key] = torch.zeros(key[1], dtype=dtype, device=self.dev)
        return b

    def _keys(self, leaves, planes, game_rows: int):
        if leaves is None:
            raise ValueError("the evaluation cache keys on the leaf rows: allocate the search with leaves=True")
        if not leaves.is_contiguous() or not planes.is_contiguous():
            raise ValueError("leaves and planes must be contiguous")
        if leaves[0].numel() * leaves.element_size() != self.key_bytes:
            raise ValueError(f"a leaf row has {leaves[0].numel() * leaves.element_size()} bytes, the cache's keys "
                             f"{self.key_bytes}")
        if leaves.shape[0] != planes.shape[0] or leaves.shape[0] % game_rows:
            raise ValueError("leaves and planes must hold the same whole number of games' rows")

    def _flush_args(self, n_rows: int) -> tuple:
        """(the entry points' family, the arguments after the counters) of this cache's flushes."""
        scratch = self._scratch(n_rows).data_ptr() if self.merge else 0
        if self.K == 2:
            return "_routed", (scratch, _stream(self.dev))
        return ("_merged", (scratch, _stream(self.dev))) if self.merge else ("", (_stream(self.dev),))

    def _probe(self, leaves, planes, rows: int, game_rows: int, route, out_values, out_logits=None):
        """The first `rows` of each game's game_rows rows through the tables (route: K = 2 alone):
        the hits' payloads land in out_values / out_logits; returns (per table the misses' planes,
        packed from row 0 of a buffer of n_games * rows rows; self.count = their numbers on the
        device)."""
        self._keys(leaves, planes, game_rows)
        self._ensure()
        n_games = leaves.shape[0] // game_rows
        n_rows = n_games * rows
        if self.K == 2:
            self._route(route, n_games)
        dense = tuple(self._buf(f"planes{k}", (n_rows, *planes.shape[1:]), planes.dtype) for k in range(self.K))
        family, last = self._flush_args(n_rows)
        getattr(_native, "evalcache_probe" + family)(
            *self._table_ptrs(), *self._sizes(), n_rows, rows, game_rows, *((route.data_ptr(),) if self.K == 2 else ()),
            leaves.data_ptr(), planes.data_ptr(), planes[0].numel() * planes.element_size(), out_values.data_ptr(),
            out_logits.data_ptr() if out_logits is not None else 0, *(d.data_ptr() for d in dense),
            self._buf("miss", (self.K, n_rows), torch.int32).data_ptr(), self.count.data_ptr(), self.counters.data_ptr(), *last)
        return dense, self.count

    def _commit(self, leaves, rows: int, game_rows: int, dense_values, dense_logits, out_values, out_logits=None):
        """After the networks ran on _probe's dense planes: per table the misses' values and
        logits (None for value networks) go to their rows' slots of out_values / out_logits and
        into the table (with merge, their followers' slots too); self.count is 0 again."""
        n_rows = leaves.shape[0] // game_rows * rows
        for v in dense_values:
            if v.dtype != torch.float64 or v.numel() < n_rows:
                raise ValueError(f"the network must return fp64 values for {n_rows} rows")
        if self.K == 2 and dense_values[0].data_ptr() == dense_values[1].data_ptr():
            raise ValueError("the two networks must return their values in two buffers (one network on both sides: "
                             "give one side a replica())")
        if self.logit_bytes:
            for lg in dense_logits or (None,) * self.K:
                if lg is None or not lg.is_contiguous() or lg.shape[0] < n_rows or \
                        lg[0].numel() * lg.element_size() != self.logit_bytes:
                    raise ValueError(f"the network must return contiguous logits of {self.logit_bytes} bytes a row")
        logits = [lg.data_ptr() for lg in dense_logits] if self.logit_bytes else [0] * self.K
        family, last = self._flush_args(n_rows)
        getattr(_native, "evalcache_commit" + family)(
            *self._table_ptrs(), *self._sizes(), n_rows, rows, game_rows, leaves.data_ptr(),
            self._buf("miss", (self.K, n_rows), torch.int32).data_ptr(), self.count.data_ptr(),
            *(p for v, lg in zip(dense_values, logits) for p in (v.data_ptr(), lg)), out_values.data_ptr(),
            out_logits.data_ptr() if out_logits is not None else 0, self.counters.data_ptr(), *last)


class EvalCache(_Cache):
    """The table (zc_evalcache_*), its miss counter, its four counters and the dense buffers of
    the misses (allocated per flush shape at first use).  entries: the table holds the largest
    power-of-two number of 8-way sets within it.  key_bytes: the leaf row's size (24: zc_c4_state,
    72: zc_chess_state).  logit_bytes: the logits of one row (0: a value network).  merge: equal
    rows of one flush are evaluated once (a fifth counter, "merged", and a scratch per flush
    shape); entries = 0, with merge alone: no table."""
    K, COUNTERS = 1, ()

    @property
    def table(self):
        return self.tables[0] if self.tables is not None else None

    def stats(self) -> dict:
        """{"probed", "hits", "inserts", "dropped"} so far, and "merged" with merge=True.
        Synchronises."""
        return self._stats()[0]

    def probe(self, leaves, planes, rows: int, game_rows: int, out_values, out_logits=None):
        """The first `rows` of each game's game_rows rows through the table: the hits' payloads
        land in out_values / out_logits; returns (the misses' planes packed from row 0 of a
        buffer of n_games * rows rows, self.count = their number on the device)."""
        dense, count = self._probe(leaves, planes, rows, game_rows, None, out_values, out_logits)
        return dense[0], count

    def commit(self, leaves, rows: int, game_rows: int, dense_values, dense_logits, out_values, out_logits=None):
        """After the network ran on probe's dense planes: the misses' outputs go to their rows'
        slots of out_values / out_logits and into the table (with merge, their followers' slots
        too); self.count is 0 again."""
        self._commit(leaves, rows, game_rows, (dense_values,), (dense_logits,), out_values, out_logits)


class RoutedEvalCache(_Cache):
    """Two tables for an arena's two networks behind one routed flush (zc_evalcache_probe_routed_
    async / ..._commit_routed_async): bit 0 of a game's route word picks the table, the dense list
    and the counters of its rows, so that each network runs counted on its own misses with no
    gather, no scatter and no host read.  entries: per table.  It holds the two tables, the two
    counts, the [2][5] counters, two dense buffers per flush shape and, with merge, the scratch;
    entries = 0 with merge: no tables.  Rows of different networks never merge and never hit each
    other's table."""
    K, COUNTERS = 2, (2, len(_native.EVALCACHE_MERGED_STATS))

    def stats(self) -> tuple[dict, dict]:
        """(network A's, network B's) counters, each with EvalCache.stats()'s keys.  Synchronises."""
        return self._stats()

    def _route(self, route, n_games: int):
        if route is None or route.dtype != torch.int32 or route.dim() != 1 or not route.is_contiguous() or \
                route.shape[0] != n_games or route.device != self.count.device:
            raise ValueError(f"the route must be a contiguous int32 [{n_games}] tensor on the cache's device: one "
                             "word per game of the flush")

    def probe(self, leaves, planes, rows: int, game_rows: int, route, out_values, out_logits=None):
        """EvalCache.probe with route [n_games] int32 (bit 0: the game's network): returns ((the
        misses' planes of network A, of network B), each packed from row 0 of a buffer of
        n_games * rows rows; self.count [2] = their numbers on the device)."""
        return self._probe(leaves, planes, rows, game_rows, route, out_values, out_logits)

    def commit(self, leaves, rows: int, game_rows: int, dense_values, dense_logits, out_values, out_logits=None):
        """EvalCache.commit with dense_values = (network A's, network B's) and dense_logits the
        same (None for value networks); both counts are 0 again."""
        self._commit(leaves, rows, game_rows, dense_values, dense_logits, out_values, out_logits)


class _Cached:
    """What the four cached callables share: a network per table of the cache, and the rows per
    game of a whole flush."""
    wants_leaves = True
    route = None   # the routed callables': set_route()

    def __init__(self, nets: tuple, cache: _Cache):
        name, number = type(self).__name__, "two" if len(nets) == 2 else "an"
        for net in nets:
            if not isinstance(net, self.KIND):
                raise ValueError(f"{name} needs {number} {self.KIND.__name__}{self.HOW}: a torch module cannot take "
                                 "its row count from the device")
        self._check(nets, cache)
        self.nets, self.cache = nets, cache

    def _rows(self, leaves, planes) -> int:
        """The rows per game of a flush of all of planes' rows, after the refusals: with one
        network every row stands for itself."""
        if leaves is None:
            raise ValueError(f"{type(self).__name__} needs the leaf rows: allocate the search with leaves=True")
        if len(self.nets) == 1:
            return 1
        if self.route is None or planes.shape[0] % self.route.shape[0]:
            raise ValueError("set_route() first, with one word per game of the flush")
        return planes.shape[0] // self.route.shape[0]

    def _run(self, dense, count) -> list:
        """Each network on its dense planes, counted on its own misses."""
        return [net(d, count=count[k:k + 1]) for k, (net, d) in enumerate(zip(self.nets, dense))]


class _CachedValue(_Cached):
    KIND, HOW = MfmaValueNetwork, " (nets.for_inference(..., backend='mfma'))"

    def _check(self, nets, cache):
        if cache.logit_bytes:
            raise ValueError("a value network's cache holds no logits (logit_bytes = 0)")

    def _flush(self, leaves, planes, rows: int, game_rows: int, out):
        dense, count = self.cache._probe(leaves, planes, rows, game_rows, self.route, out)
        self.cache._commit(leaves, rows, game_rows, self._run(dense, count), None, out)
        return out

    @torch.no_grad()
    def __call__(self, leaves, planes, counts):
        rows = self._rows(leaves, planes)
        return self._flush(leaves, planes, rows, rows, self.cache._buf("out", (planes.shape[0],), torch.float64))

    @torch.no_grad()
    def rows(self, planes, n: int, bs: int, nb: int, out, leaves=None):
        """NetValue.rows: the short last flush, each game's first nb rows alone."""
        self._rows(leaves, planes)
        return self._flush(leaves, planes, nb, bs, out)


class _CachedPolicy(_Cached):
    KIND, HOW = MfmaPolicyValueNetwork, ""
    roots_only = True

    def _check(self, nets, cache):
        for net in nets:
            if not (net.conv_head or net.fused):
                raise ValueError(f"{type(self).__name__} needs the fused policy head (32 policy planes on 64 or "
                                 "128 channels)")
        for net in nets:
            if cache.logit_bytes != 2 * net.logits_width:
                raise ValueError(f"the network's logits are {2 * net.logits_width} bytes a row, the cache's "
                                 f"{cache.logit_bytes}")
        self.width = nets[0].logits_width

    @torch.no_grad()
    def __call__(self, leaves, planes, counts):
        c, L = self.cache, planes.shape[0]
        rows = self._rows(leaves, planes)
        vo = c._buf("vout", (L,), torch.float64)
        lo = c._buf("lout", (L, self.width), torch.float16)
        dense, count = c._probe(leaves, planes, rows, rows, self.route, vo, lo)
        outs = self._run(dense, count)
        c._commit(leaves, rows, rows, tuple(v for v, _ in outs), tuple(lg.contiguous() for _, lg in outs), vo, lo)
        return vo, lo


class CachedValue(_CachedValue):
    """valued.NetValue behind an EvalCache: a value search's value_fn over an MfmaValueNetwork.
    The search must be allocated with leaves=True (the shared driver then passes the leaf rows to
    rows() too)."""

    def __init__(self, net, cache: EvalCache):
        super().__init__((net,), cache)
        self.model = net


class CachedPolicy(_CachedPolicy):
    """valued.PolicyNet behind an EvalCache: a PUCT search's net_fn over an
    MfmaPolicyValueNetwork (linear or convolutional head, fused).  The cache's logit_bytes is
    the network's logits row: 2 * n_logits (fp16).  The search must be allocated with
    leaves=True; the roots flush gets the roots' rows from the shared driver."""

    def __init__(self, net, cache: EvalCache):
        super().__init__((net,), cache)
        self.net = net


class _Routed:
    """What the two routed cached callables share: the two networks (one network on both sides
    plays through a replica — weights shared, output buffers its own — and still gets two tables)
    and the route."""

    def __init__(self, net_a, net_b, cache: RoutedEvalCache):
        super().__init__((net_a, net_b), cache)
        if not isinstance(cache, RoutedEvalCache):
            raise ValueError("a routed cached callable needs a RoutedEvalCache")
        self.nets = (net_a, net_b.replica() if net_b is net_a else net_b)

    def set_route(self, key: torch.Tensor):
        """key [n_games] int32 on the device: bit 0 = the network of the game's rows (0: A, 1: B)."""
        if key.dtype != torch.int32 or key.dim() != 1 or not key.is_contiguous():
            raise ValueError("the route must be a contiguous int32 [n_games] tensor")
        self.route = key


class RoutedCachedValue(_Routed, _CachedValue):
    """valued.RoutedValue behind a RoutedEvalCache: an arena value search's value_fn over two
    MfmaValueNetwork.  The search must be allocated with leaves=True."""


class RoutedCachedPolicy(_Routed, _CachedPolicy):
    """valued.RoutedPolicy behind a RoutedEvalCache: an arena PUCT search's net_fn over two
    MfmaPolicyValueNetwork of one head (linear or convolutional, fused) and one logits width.  The
    search must be allocated with leaves=True; the roots flush gets the roots' rows from the
    shared driver."""
