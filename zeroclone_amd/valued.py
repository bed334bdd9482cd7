"""Stepwise Connect4 search with caller-supplied leaf values (include/zeroclone.h zc_c4_ext_*).

mcts.get_move (engine/mcts/src/mcts.cpp:102-160) pauses at every flush (:112-127) and hands
the pending leaves to `value.batch` (engine/value_functions.py:16-32).  `C4ValuedSearch`
drives the same loop for many games at once with the tree on the GPU:

    begin -> [select(f) -> value_fn(leaves, planes, counts) -> backup(f)] * n_flush -> end

`value_fn` returns one fp64 value per leaf slot (n_games * batch_size, leaf j of game i at
i*batch_size + j) for the leaf's side to move.  Two value functions are provided:

* `NetValue(model)` — the reference's network modes (value_functions.py:61-99, network.py):
  the planes are built on the device in state_to_tensor layout and fed straight into the
  fp16 model; no host round trip, so a whole move can be captured in one HIP graph
  (`C4ValuedSearch.capture`).
* `HostValue(value, backend)` — any reference-style Value object: the leaves go to the host
  as c4_backend states and `value.batch(states, backend=backend)` is called once per game
  per flush, as the reference does.  Slow, but it runs any plugin on the GPU tree search.

The chess value search and the two PUCT searches follow the same protocol; `_StepSearch`
holds what the four share and each class what differs: its begin, select, backup and end.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _ptr(t) -> int:
    return t.data_ptr() if t is not None else 0


def _split_flushes(search, nfl: int, fns: list, first_game: int, select, evaluate_backup):
    """The flush loop of every stepwise search: the flushes of k contiguous game parts, part i
    on stream i (stream 0: the current one; the others fork from it and join back), fns[i] the
    part's value / network function; one function is one part, the whole search on the current
    stream.  The parts share no tree, buffer or counter — select and backup of a part touch
    only its games and its slices of the leaf / plane / count / value buffers, and each fns[i]
    owns its network buffers — so the order of the launches across parts does not matter, and
    the GPU runs one part's search kernels beside another part's network.  select(first, n, f,
    leaves, planes, counts, stream); evaluate_backup(first, n, f, fn, leaves, planes, counts,
    values, stream) calls fn and backs its output up."""
    n, bs, k = search.n, search.bs, len(fns)
    main = torch.cuda.current_stream(search.dev)
    if len(search._side) < k - 1:
        search._side = [torch.cuda.Stream(search.dev) for _ in range(k - 1)]
    streams = [main] + search._side[:k - 1]
    for st in streams[1:]:
        st.wait_stream(main)
    parts = []
    for i in range(k):
        lo, hi = i * n // k, (i + 1) * n // k
        if hi > lo:
            sl = slice(lo * bs, hi * bs)
            parts.append((lo, hi, streams[i], fns[i], search.leaves[sl] if search.leaves is not None else None,
                          search.planes[sl] if search.planes is not None else None, search.counts[lo:hi],
                          search.values[sl]))
    for f in range(nfl):
        for lo, hi, st, fn, lv, pv, cv, vv in parts:
            with torch.cuda.stream(st):
                select(first_game + lo, hi - lo, f, lv, pv, cv, st.cuda_stream)
                evaluate_backup(first_game + lo, hi - lo, f, fn, lv, pv, cv, vv, st.cuda_stream)
    for st in streams[1:]:
        main.wait_stream(st)


def _value_backup(sims: int, bs: int, backup):
    """evaluate_backup of a value search's part (_split_flushes): fn.flush_values(first, n,
    flush, stream) where fn has it (values computed on the device from the tree itself), else
    the part's network on its leaves (a short last flush on its nb leaves only, NetValue.rows;
    a function with wants_leaves gets the leaf rows there too), then backup(first, n, flush,
    values, stream)."""
    def evaluate_backup(first, m, f, fn, lv, pv, cv, vv, st):
        nb = min(bs, sims - f * bs)   # every game's pending leaves (0 after an error)
        if hasattr(fn, "flush_values"):
            v = fn.flush_values(first, m, f, st)
        elif nb < bs and hasattr(fn, "rows") and pv is not None:
            if getattr(fn, "wants_leaves", False):
                v = fn.rows(pv, m, bs, nb, vv, leaves=lv)
            else:
                v = fn.rows(pv, m, bs, nb, vv)
        else:
            v = fn(lv, pv, cv)
        if v.data_ptr() != vv.data_ptr():
            vv.copy_(v.reshape(-1))
        backup(first, m, f, vv.data_ptr(), st)
    return evaluate_backup


class PolicyNet:
    """A policy + value network as a PUCT search's net_fn: net(planes) -> (values fp64 [rows],
    logits [rows, n_logits]).  It depends on the planes alone, so the search may call it on
    the n root positions of flush 0 (one leaf a game) instead of all n * batch_size slots."""
    roots_only = True

    def __init__(self, net):
        self.net = net

    def __call__(self, leaves, planes, counts):
        return self.net(planes)


def _puct_backup(bs: int, backup):
    """evaluate_backup of a PUCT search (part): fn on the flush's planes, then backup(first, n,
    flush, values, logits, logits_f16, stream, rows).  Flush 0 holds the roots only: a
    roots_only fn evaluates the n root positions alone (rows = 1), and gets their leaf rows
    when it has wants_leaves (and the search keeps leaf rows)."""
    def evaluate_backup(first, m, f, fn, lv, pv, cv, vv, st):
        if f == 0 and getattr(fn, "roots_only", False):
            roots = pv.view(m, bs, *pv.shape[1:])[:, 0].contiguous()
            rl = None
            if getattr(fn, "wants_leaves", False) and lv is not None:
                rl = lv.view(m, bs, *lv.shape[1:])[:, 0].contiguous()
            v, logits = fn(rl, roots, cv)
            v = v.reshape(-1).to(torch.float64).contiguous()
            logits = logits.contiguous()
            backup(first, m, f, v.data_ptr(), logits.data_ptr(), logits.dtype == torch.float16, st, rows=1)
            return
        v, logits = fn(lv, pv, cv)
        if v.data_ptr() != vv.data_ptr():
            vv.copy_(v.reshape(-1))
        logits = logits.contiguous()
        backup(first, m, f, vv.data_ptr(), logits.data_ptr(), logits.dtype == torch.float16, st)
    return evaluate_backup


def _warm_parts(search, fns):
    """Each part's function once on its own slice, and a PolicyNet also at the roots flush's
    shape (graph capture warms kernels and buffers)."""
    k, n, bs = len(fns), search.n, search.bs
    for i, fn in enumerate(fns):
        lo, hi = i * n // k, (i + 1) * n // k
        fn(search.leaves[lo * bs:hi * bs] if search.leaves is not None else None,
           search.planes[lo * bs:hi * bs] if search.planes is not None else None, search.counts[lo:hi])
        if getattr(fn, "roots_only", False):
            rl = None
            if getattr(fn, "wants_leaves", False) and search.leaves is not None:
                rl = search.leaves[lo * bs:hi * bs:bs].contiguous()
            fn(rl, search.planes[lo * bs:hi * bs:bs].contiguous(), search.counts[lo:hi])


class _StepSearch:
    """What the four stepwise searches share: the buffers, the checks and the move

        begin -> [select(f) -> evaluate -> backup(f)] * flushes -> end    (_split_flushes)

    A search kind (_ValueSearch, _PuctSearch) gives _begin(first, roots, sims, par, stream),
    _select (as _split_flushes calls it), _evaluate_backup(sims) (the rule for _split_flushes),
    _end(first, par, stream) and _flushes(sims), written against the engine's wrappers of its
    STEPS; par is the move's own parameter, a value search's c or a PUCT search's temperature.
    A game's class gives GAME, which selects those wrappers, and the row shapes below."""
    GAME = ""                        # "c4" / "chess": the engine's <GAME>_<step> wrappers
    STEPS = ()                       # the kind's steps: self._<step> = eng.<GAME>_<step>, looked up once
    STATE = ""                       # the C struct of a root / leaf row
    LEAF = ((0,), torch.uint8)       # a leaf row's shape and dtype (the roots' too)
    PLANES = (0, 0, 0)               # one leaf's planes
    MOVE = torch.int32
    NA = 0                           # root visit counts (and priors) per game
    PRIOR = False

    def _alloc(self, eng, n_games: int, batch_size: int, planes_dtype, leaves: bool = True, planes: bool = True):
        if batch_size > eng.max_batch:
            raise ValueError(f"batch_size {batch_size} > engine max_batch {eng.max_batch}")
        if n_games > eng.max_games:
            raise ValueError(f"{n_games} games > engine capacity {eng.max_games}")
        if planes_dtype not in (torch.float16, torch.float32):
            raise ValueError("planes_dtype must be float16 or float32")
        self.eng, self.n, self.bs = eng, n_games, batch_size
        for step in self.STEPS:
            setattr(self, "_" + step, getattr(eng, f"{self.GAME}_{step}"))
        self.dev = dev = torch.device("cuda", eng.device)
        L, (row, row_dtype) = n_games * batch_size, self.LEAF
        self.leaves = torch.zeros((L, *row), dtype=row_dtype, device=dev) if leaves else None
        self.planes = torch.zeros((L, *self.PLANES), dtype=planes_dtype, device=dev) if planes else None
        self.counts = torch.zeros(n_games, dtype=torch.int32, device=dev)
        self.values = torch.zeros(L, dtype=torch.float64, device=dev)
        self.move = torch.zeros(n_games, dtype=self.MOVE, device=dev)
        self.na = torch.zeros((n_games, self.NA), dtype=torch.int32, device=dev)
        if self.PRIOR:
            self.prior = torch.zeros((n_games, self.NA), dtype=torch.float32, device=dev)
        self.stats = torch.zeros((n_games, _native.STATS_FIELDS), dtype=torch.int64, device=dev)
        self._side = []   # the streams of parts 1.. (_split_flushes)

    def _enqueue(self, roots: torch.Tensor, sims: int, fn, first_game: int, par: float):
        row, row_dtype = self.LEAF
        if roots.shape != (self.n, *row) or roots.dtype != row_dtype or not roots.is_contiguous():
            raise ValueError(f"roots must be a contiguous {str(row_dtype)[6:]} [n_games, {row[0]}] tensor of "
                             f"{self.STATE} rows")
        if roots.device != self.dev:
            raise ValueError("roots must live on the engine's device")
        s = _stream(self.dev)
        self._begin(first_game, roots, sims, par, s)
        fns = list(fn) if isinstance(fn, (list, tuple)) else [fn]
        _split_flushes(self, self._flushes(sims), fns, first_game, self._select, self._evaluate_backup(sims))
        self._end(first_game, par, s)
        return self.move, self.na, self.stats

    def _run(self, *move):
        self._enqueue(*move)
        torch.cuda.current_stream(self.dev).synchronize()
        return self.move, self.na, self.stats

    def _capture(self, roots, sims, fn, first_game, par):
        side = torch.cuda.Stream(self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):  # warm the function's kernels outside capture
            _warm_parts(self, fn if isinstance(fn, (list, tuple)) else [fn])
        torch.cuda.current_stream(self.dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._enqueue(roots, sims, fn, first_game, par)
        return g


class _ValueSearch(_StepSearch):
    """value_fn: one callable, or a list of k callables — then the games are split into k
    contiguous parts searched on k streams (_split_flushes).  The results are the same."""
    STEPS = ("ext_begin", "ext_select", "ext_backup", "ext_end")
    _begin_extra = ()   # what the game's ext_begin takes after batch_size

    def _flushes(self, sims: int) -> int:
        return (sims + self.bs - 1) // self.bs

    def _begin(self, first, roots, sims, c, s):
        self._ext_begin(first, self.n, roots.data_ptr(), sims, c, self.bs, *self._begin_extra, s)

    def _select(self, first, m, f, lv, pv, cv, s):
        self._ext_select(first, m, f, _ptr(lv), _ptr(pv), pv is None or pv.dtype == torch.float16, cv.data_ptr(), s)

    def _evaluate_backup(self, sims):
        return _value_backup(sims, self.bs, self._ext_backup)

    def _end(self, first, c, s):
        self._ext_end(first, self.n, self.move.data_ptr(), self.na.data_ptr(), self.stats.data_ptr(), s)

    def enqueue(self, roots: torch.Tensor, sims: int, c: float, value_fn, first_game: int = 0):
        """Enqueue one whole move on torch's current stream (no host synchronisation unless
        value_fn makes one)."""
        return self._enqueue(roots, sims, value_fn, first_game, c)

    def run(self, roots: torch.Tensor, sims: int, c: float, value_fn, first_game: int = 0):
        return self._run(roots, sims, value_fn, first_game, c)

    def capture(self, roots: torch.Tensor, sims: int, c: float, value_fn, first_game: int = 0):
        """Capture one move into a HIP graph (value_fn must be capturable, e.g. NetValue).
        Returns the graph; graph.replay() re-runs the move on the current contents of
        `roots` and of the games' RNG streams."""
        return self._capture(roots, sims, value_fn, first_game, c)


class _PuctSearch(_StepSearch):
    """net_fn: one callable, or a list of k callables — then the games are split into k
    contiguous parts searched on k streams (_split_flushes): one part's select, backup and
    policy GEMM overlap another part's tower.  The results are the same."""
    PRIOR = True
    STEPS = ("puct_begin", "puct_begin_reuse", "puct_forget", "puct_forget_fresh", "puct_select", "puct_backup",
             "puct_end")
    _select_extra = {}   # what the game's puct_select takes besides

    def _alloc_puct(self, eng, n_games, batch_size, c_puct, alpha, eps, seed, planes_dtype, leaves):
        self._alloc(eng, n_games, batch_size, planes_dtype, leaves)
        self.c, self.alpha, self.eps, self.seed = c_puct, alpha, eps, seed
        # per-game search number: the Philox counter word of the root noise and the
        # temperature sample; each search adds 1 on the device (graph replays included)
        self.search_no = torch.zeros(n_games, dtype=torch.int32, device=self.dev)

    def _alloc_reuse(self, reuse: bool):
        """reuse and kept; with reuse, the re-root's scratch too exists before any graph capture."""
        self.reuse, self.kept = bool(reuse), None
        if self.reuse:
            self.kept = torch.zeros(self.n, dtype=torch.int32, device=self.dev)
            z = torch.zeros((1, *self.LEAF[0]), dtype=self.LEAF[1], device=self.dev)
            self._puct_begin_reuse(0, 0, z.data_ptr(), 2, self.c, self.bs, self.alpha, self.eps, self.seed)
            self.forget()   # trees of an earlier search object on this engine are not this one's

    def forget(self, first_game: int = 0, n: int | None = None):
        """Drop the kept trees of games [first_game, first_game + n) (default: this search's n
        games), stream-ordered: their next search starts afresh."""
        self._puct_forget(first_game, self.n if n is None else n, _stream(self.dev))

    def forget_fresh(self, slot: torch.Tensor, stream: int | None = None):
        """Drop the kept trees of the games whose recorder slot (Trajectories.slot, [n, 4] int32)
        holds a game at its first position, on the device (stream: default torch's current one):
        a refilled slot's tree belongs to the game that ended."""
        self._puct_forget_fresh(0, self.n, slot.data_ptr(), stream if stream is not None else _stream(self.dev))

    def _flushes(self, sims: int) -> int:
        return _native.check(_native.lib().zc_chess_puct_flushes(int(sims), int(self.bs)))

    def _begin(self, first, roots, sims, temperature, s):
        args = (first, self.n, roots.data_ptr(), sims, self.c, self.bs, self.alpha, self.eps, self.seed,
                self.search_no.data_ptr())
        if self.reuse:
            self._puct_begin_reuse(*args, self.kept.data_ptr(), stream=s)
        else:
            self._puct_begin(*args, stream=s)

    def _select(self, first, m, f, lv, pv, cv, s):
        self._puct_select(first, m, f, _ptr(lv), pv.data_ptr(), pv.dtype == torch.float16, cv.data_ptr(), s,
                          **self._select_extra)

    def _evaluate_backup(self, sims):
        return _puct_backup(self.bs, self._puct_backup)

    def _end(self, first, temperature, s):
        self._puct_end(first, self.n, temperature, self.move.data_ptr(), self.na.data_ptr(), self.prior.data_ptr(),
                       self.stats.data_ptr(), s)

    def enqueue(self, roots: torch.Tensor, sims: int, net_fn, temperature: float = 0.0, first_game: int = 0):
        return self._enqueue(roots, sims, net_fn, first_game, temperature)

    def run(self, roots, sims, net_fn, temperature: float = 0.0, first_game: int = 0):
        return self._run(roots, sims, net_fn, first_game, temperature)

    def capture(self, roots, sims, net_fn, temperature: float = 0.0, first_game: int = 0):
        return self._capture(roots, sims, net_fn, first_game, temperature)


class C4ValuedSearch(_ValueSearch):
    GAME = "c4"
    STATE, LEAF, PLANES, MOVE, NA = "zc_c4_state", ((3,), torch.int64), (2, 6, 7), torch.int32, 7

    def __init__(self, eng: "_native.NativeEngine", n_games: int, batch_size: int = 32,
                 planes_dtype: torch.dtype = torch.float16, leaves: bool = True, planes: bool = True):
        self._alloc(eng, n_games, batch_size, planes_dtype, leaves, planes)


class NetValue:
    """Value('network_*') (value_functions.py:61-99): model(planes) in the planes' dtype;
    the [B, 1] output is the value for each leaf's side to move."""

    def __init__(self, model: torch.nn.Module):
        self.model = model

    @torch.no_grad()
    def __call__(self, leaves, planes, counts):
        return self.model(planes).reshape(-1).to(torch.float64)

    @torch.no_grad()
    def rows(self, planes, n: int, bs: int, nb: int, out):
        """A flush whose games all hold nb < bs pending leaves (the last flush of a search
        whose simulations are not a multiple of the batch): the network runs on those n*nb
        boards only, and their values land in out's first nb slots of each game (the others
        are never backed up).  Each board's value does not depend on its batch: the values
        are those of the full call."""
        sub = planes.view(n, bs, *planes.shape[1:])[:, :nb].reshape(n * nb, *planes.shape[1:])
        out.view(n, bs)[:, :nb].copy_(self.model(sub).reshape(n, nb).to(torch.float64))
        return out


class _Routed:
    """Two callables behind one: game perm[i] (i < n_a) is fn_a's, the others fn_b's
    (`set_route`, the partition of zc_arena_route_async).  A flush's rows are gathered into
    partition order (zc_arena_gather_async), fn_a runs on the first n_a games' rows and fn_b on
    the rest, each in one call and an empty group in none, and the outputs are scattered back
    to game order (zc_arena_scatter_async).  Only the planes are routed: the inner callables
    get leaves=None.  The gather buffers are kept between calls; n_a is a host value, so a
    routed flush cannot be replayed from a graph captured under another partition."""

    def __init__(self, fn_a, fn_b):
        self.fns = (fn_a, fn_b)
        self.perm, self.n_a = None, 0
        self._bufs = {}

    def set_route(self, perm: torch.Tensor, n_a: int):
        """perm [n] int32 on the device: the games in partition order; the first n_a are fn_a's."""
        if perm.dtype != torch.int32 or perm.dim() != 1 or not perm.is_contiguous():
            raise ValueError("perm must be a contiguous int32 [n_games] tensor")
        if not 0 <= int(n_a) <= perm.shape[0]:
            raise ValueError(f"n_a {n_a} outside [0, {perm.shape[0]}]")
        self.perm, self.n_a = perm, int(n_a)

    def _buf(self, name: str, shape: tuple, like: torch.Tensor, dtype=None) -> torch.Tensor:
        """One buffer per use and shape (a search has two or three: the full flush, the short
        last one, the roots), allocated at its first call."""
        key = (name, tuple(shape), dtype or like.dtype, like.device)
        b = self._bufs.get(key)
        if b is None:
            b = self._bufs[key] = torch.zeros(key[1], dtype=key[2], device=key[3])
        return b

    def _games(self, n: int):
        if self.perm is None or self.perm.shape[0] != n:
            raise ValueError(f"set_route() first, with a partition of the flush's {n} games")

    def _gather(self, name: str, src: torch.Tensor, n: int, rows: int, game_rows: int) -> torch.Tensor:
        """The first `rows` of each game's game_rows rows of src, in partition order."""
        if not src.is_contiguous() or src.shape[0] != n * game_rows:
            raise ValueError(f"a routed tensor must be contiguous with {n * game_rows} rows")
        dst = self._buf(name, (n * rows, *src.shape[1:]), src)
        _native.arena_gather(n, rows, game_rows, src[0].numel() * src.element_size(), self.perm.data_ptr(),
                             src.data_ptr(), dst.data_ptr(), _stream(src.device))
        return dst

    def _scatter(self, src: torch.Tensor, dst: torch.Tensor, n: int, rows: int, game_rows: int):
        _native.arena_scatter(n, rows, game_rows, src[0].numel() * src.element_size(), self.perm.data_ptr(),
                              src.data_ptr(), dst.data_ptr(), _stream(src.device))

    def _groups(self, n: int, rows: int):
        """(fn, first row, end row, first game, end game) of each non-empty group."""
        k = self.n_a
        return [(fn, lo * rows, hi * rows, lo, hi) for fn, lo, hi in ((self.fns[0], 0, k), (self.fns[1], k, n))
                if hi > lo]


class RoutedValue(_Routed):
    """A value search's value_fn over two value functions (e.g. two NetValue)."""

    def _values(self, planes, n: int, rows: int, game_rows: int, counts, out):
        self._games(n)
        g = self._gather("planes", planes, n, rows, game_rows)
        v = self._buf("values", (n * rows,), planes, torch.float64)
        for fn, lo, hi, g0, g1 in self._groups(n, rows):
            v[lo:hi].copy_(fn(None, g[lo:hi], counts[g0:g1] if counts is not None else None).reshape(-1))
        self._scatter(v, out, n, rows, game_rows)
        return out

    @torch.no_grad()
    def __call__(self, leaves, planes, counts):
        n = counts.shape[0]
        rows = planes.shape[0] // n
        self._games(n)
        c = self._gather("counts", counts, n, 1, 1)
        return self._values(planes, n, rows, rows, c, self._buf("out", (n * rows,), planes, torch.float64))

    @torch.no_grad()
    def rows(self, planes, n: int, bs: int, nb: int, out):
        """The short last flush (NetValue.rows): the first nb rows of each game are gathered and
        evaluated (counts=None for the inner callables), and the values land in out's first nb
        slots of each game."""
        return self._values(planes, n, nb, bs, None, out)


class RoutedPolicy(_Routed):
    """A PUCT search's net_fn over two policy + value networks (e.g. two PolicyNet): returns
    (values fp64, logits) in game order.  Like PolicyNet it depends on the planes alone, so the
    roots flush evaluates one row a game.  Both networks must return logits of one dtype and
    width."""
    roots_only = True

    def __init__(self, fn_a, fn_b):
        super().__init__(fn_a, fn_b)
        self._logits = None   # (dtype, width) of the first network that ran

    @torch.no_grad()
    def __call__(self, leaves, planes, counts):
        n = counts.shape[0]
        rows = planes.shape[0] // n
        self._games(n)
        g = self._gather("planes", planes, n, rows, rows)
        c = self._gather("counts", counts, n, 1, 1)
        v = self._buf("values", (n * rows,), planes, torch.float64)
        lg = None
        for fn, lo, hi, g0, g1 in self._groups(n, rows):
            fv, fl = fn(None, g[lo:hi], c[g0:g1])
            fl = fl.reshape(hi - lo, -1)
            if self._logits is None:
                self._logits = (fl.dtype, fl.shape[1])
            if (fl.dtype, fl.shape[1]) != self._logits:
                raise ValueError(f"the two networks' logits differ: {fl.dtype} x {fl.shape[1]} against "
                                 f"{self._logits[0]} x {self._logits[1]}")
            if lg is None:
                lg = self._buf("logits", (n * rows, fl.shape[1]), fl)
            v[lo:hi].copy_(fv.reshape(-1))
            lg[lo:hi].copy_(fl)
        vo = self._buf("vout", (n * rows,), planes, torch.float64)
        lo_ = self._buf("lout", tuple(lg.shape), lg)
        self._scatter(v, vo, n, rows, rows)
        self._scatter(lg, lo_, n, rows, rows)
        return vo, lo_


class HostValue:
    """Any reference-style Value object: value.batch(states, backend=backend) per game per
    flush, on c4_backend states built from the device leaves.  With `eng`, Python's global
    `random` is game first_game + i's device stream during the call (the flush's expansion
    draws already taken, as in mcts.cpp:112-127), so a value object that draws from `random`
    gets the reference's numbers and the search continues after them."""

    def __init__(self, value, backend, eng=None, first_game: int = 0):
        self.value, self.backend, self.eng, self.first = value, backend, eng, first_game

    def __call__(self, leaves, planes, counts):
        from .engine._device import game_stream
        from .engine.games.connect4 import c4_backend as zb
        rows = leaves.cpu().numpy().view(np.uint64)
        cnt = counts.cpu().numpy()
        bs = rows.shape[0] // cnt.shape[0]
        out = np.zeros(rows.shape[0], np.float64)
        for i, k in enumerate(cnt):
            if k == 0:
                continue
            states = [zb.from_zc(int(r[0]), int(r[1]), int(r[2]) & 1) for r in rows[i * bs: i * bs + k]]
            if self.eng is None:
                v = self.value.batch(states, backend=self.backend)
            else:
                with game_stream(self.eng, self.first + i):
                    v = self.value.batch(states, backend=self.backend)
            out[i * bs: i * bs + k] = [float(x) for x in v]
        return torch.from_numpy(out).to(leaves.device)


class ChessValuedSearch(_ValueSearch):
    """Stepwise chess search (zc_chess_ext_*): the configs/chess_value.yaml path — a value
    network evaluates every flush's leaves (planes [n*bs, 17, 8, 8]) between the select and
    backup kernels.  Same protocol and value_fn contract as C4ValuedSearch."""
    GAME = "chess"
    _begin_extra = property(lambda self: (self.policy, self.freedom))
    STATE, LEAF, PLANES, MOVE, NA = ("zc_chess_state", ((72,), torch.uint8), (17, 8, 8), torch.int16,
                                     _native.CHESS_MAX_MOVES)

    def __init__(self, eng: "_native.NativeEngine", n_games: int, batch_size: int = 32,
                 planes_dtype: torch.dtype = torch.float16, leaves: bool = True, planes: bool = True,
                 policy: int = _native.ZC_POLICY_RANDOM, freedom: float = 0.0):
        self._alloc(eng, n_games, batch_size, planes_dtype, leaves, planes)
        self.policy, self.freedom = policy, freedom
        eng.chess_reserve()   # the tree arena exists before any graph capture


class ChessPuctSearch(_PuctSearch):
    """AlphaZero-style PUCT search for chess (zc_chess_puct_*).

    net_fn(leaves, planes, counts) -> (values fp64 [n*bs], logits [n*bs, 4096] fp32/fp16,
    index from*64 + to).  Flush 0 evaluates the roots; Dirichlet(alpha) noise of weight eps
    goes on the root priors; end() picks by visits (temperature 0) or samples.

    reuse=True: every search keeps, per game, the subtree of its root position when the game's
    previous search holds it one or two plies below its root (zc_chess_puct_begin_reuse), and
    then adds sims - 1 visits below the kept ones; `kept` [n] int32 = nodes kept (0: a fresh
    tree).  The engine needs max_sims above sims for anything to be kept; forget() drops the
    trees, and so does any other chess search of the game."""
    GAME = "chess"
    STATE, LEAF, PLANES, MOVE, NA = ChessValuedSearch.STATE, ChessValuedSearch.LEAF, (17, 8, 8), torch.int16, \
        _native.CHESS_MAX_MOVES

    def __init__(self, eng: "_native.NativeEngine", n_games: int, batch_size: int = 32, c_puct: float = 1.5,
                 dirichlet_alpha: float = 0.3, dirichlet_eps: float = 0.25, seed: int = 0,
                 planes_dtype: torch.dtype = torch.float16, leaves: bool = True, planes_nhwc: bool = False,
                 reuse: bool = False):
        """planes_nhwc: the select kernel writes the planes in the MFMA tower's input layout, fp16
        [n * batch_size, 64, 32] (17 planes then zeros, square-major), so the network takes them
        without a conversion launch (MfmaPolicyValueNetwork with the convolutional head)."""
        if planes_nhwc and planes_dtype != torch.float16:
            raise ValueError("planes_nhwc needs fp16 planes")
        self.planes_nhwc = planes_nhwc
        self._select_extra = {"planes_nhwc": planes_nhwc}
        if planes_nhwc:
            self.PLANES = (64, 32)
        self._alloc_puct(eng, n_games, batch_size, c_puct, dirichlet_alpha, dirichlet_eps, seed, planes_dtype, leaves)
        eng.chess_reserve()   # the tree arena exists before any graph capture
        self._alloc_reuse(reuse)


class C4PuctSearch(_PuctSearch):
    """AlphaZero-style PUCT search for Connect4 (zc_c4_puct_*, SURVEY §8 a21 on the target
    game): the chess PUCT search's selection, virtual loss, Dirichlet root noise and
    temperature on the Connect4 rules.

    net_fn(leaves, planes, counts) -> (values fp64 [n*bs], logits [n*bs, 7] fp32/fp16, one per
    column) — e.g. `lambda l, p, c: net(p)` with nets.MfmaPolicyValueNetwork over
    PolicyValueNetwork(in_planes=2, board=(6, 7), n_logits=7).

    reuse=True: every search keeps, per game, the subtree of its root position when the game's
    previous search holds it one or two plies below its root (zc_c4_puct_begin_reuse), and then
    adds sims - 1 visits below the kept ones; `kept` [n] int32 = nodes kept (0: a fresh tree).
    The engine needs max_sims above sims for anything to be kept; forget() drops the trees."""
    GAME = "c4"
    STATE, LEAF, PLANES, MOVE, NA = C4ValuedSearch.STATE, C4ValuedSearch.LEAF, (2, 6, 7), torch.int32, 7

    def __init__(self, eng: "_native.NativeEngine", n_games: int, batch_size: int = 32, c_puct: float = 1.5,
                 dirichlet_alpha: float = 0.3, dirichlet_eps: float = 0.25, seed: int = 0,
                 planes_dtype: torch.dtype = torch.float16, leaves: bool = True, reuse: bool = False):
        self._alloc_puct(eng, n_games, batch_size, c_puct, dirichlet_alpha, dirichlet_eps, seed, planes_dtype, leaves)
        # the tree arena exists before any graph capture
        z = torch.zeros((1, 3), dtype=torch.int64, device=self.dev)
        self._puct_begin(0, 0, z.data_ptr(), 2, c_puct, batch_size, dirichlet_alpha, dirichlet_eps, seed)
        self._alloc_reuse(reuse)
