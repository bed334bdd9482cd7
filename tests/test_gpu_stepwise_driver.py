"""The launch sequence of the four stepwise search drivers (zeroclone_amd/valued.py) as a
closed-form specification: a recording proxy around NativeEngine logs every call, and the log
of one move must be

    begin; for flush f: for part [lo, hi): select(f), backup(f); end

with first = first_game + lo, n = hi - lo, each buffer pointer the search's buffer offset by
the part's slice, part 0 on the current stream and part 1 on another.  One callable is one
part; a list of k callables is k parts with boundaries i * n // k (valued._split_flushes).

5 games at batch 4 and 10 simulations: a value search has 3 flushes, the last one short (2
leaves a game); a PUCT search has 1 + ceil(9 / 4) = 4, flush 0 holding the roots alone."""
import inspect

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, BS, SIMS, C = 5, 4, 10, 1.4
PARTS2 = [(0, 2), (2, 5)]   # i * 5 // 2


class Recorder:
    """Forwards to a NativeEngine and logs (method, arguments by name) of every call."""

    def __init__(self, eng):
        self._eng, self.log = eng, []

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if not callable(attr):
            return attr
        sig = inspect.signature(attr)

        def call(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            self.log.append((name, dict(b.arguments)))
            return attr(*a, **k)
        return call


class Zeros(torch.nn.Module):
    """A network that returns zeros and records how many boards it was given."""

    def __init__(self, seen, n_logits=0):
        super().__init__()
        self.seen, self.n_logits = seen, n_logits

    def forward(self, x):
        self.seen.append(x.shape[0])
        if not self.n_logits:
            return torch.zeros((x.shape[0], 1), dtype=x.dtype, device=x.device)
        return (torch.zeros(x.shape[0], dtype=torch.float64, device=x.device),
                torch.zeros((x.shape[0], self.n_logits), dtype=torch.float32, device=x.device))


def c4_roots():
    return torch.zeros((N, 3), dtype=torch.int64, device="cuda")   # empty boards, X to move


def chess_roots():
    from zeroclone_amd import _native
    rows = np.array([_native.chess_init()] * N, _native.CHESS_STATE_DTYPE).view(np.uint8).reshape(N, 72)
    return torch.from_numpy(rows.copy()).cuda()


# family: search class, its calls' prefix, PUCT or value search, logits per row, roots
FAMILIES = {
    "c4_ext": ("C4ValuedSearch", "c4_ext", False, 0, c4_roots),
    "chess_ext": ("ChessValuedSearch", "chess_ext", False, 0, chess_roots),
    "chess_puct": ("ChessPuctSearch", "chess_puct", True, 4096, chess_roots),
    "c4_puct": ("C4PuctSearch", "c4_puct", True, 7, c4_roots),
}


def run_form(family, form, first_game, main):
    """One move of `family`'s search on a fresh engine, `form` = "one" (a callable), "list1" or
    "list2" (a list of 1 or 2 callables), on stream `main`.  Returns (search, roots, log, boards
    seen by the network, outputs)."""
    from zeroclone_amd import _native, valued
    cls, prefix, puct, n_logits, roots_fn = FAMILIES[family]
    eng = _native.NativeEngine(max_games=8, max_sims=16, max_batch=BS)
    try:
        eng.seed(0, list(range(100, 108)))
        rec = Recorder(eng)
        search = getattr(valued, cls)(rec, N, BS, seed=3) if puct else getattr(valued, cls)(rec, N, BS)
        roots, seen = roots_fn(), []
        make = (lambda: valued.PolicyNet(Zeros(seen, n_logits))) if puct else (lambda: valued.NetValue(Zeros(seen)))
        fn = {"one": make, "list1": lambda: [make()], "list2": lambda: [make(), make()]}[form]()
        torch.cuda.synchronize()
        del rec.log[:]   # the constructor's reservations
        with torch.cuda.stream(main):
            if puct:
                search.run(roots, SIMS, fn, 0.0, first_game)
            else:
                search.run(roots, SIMS, C, fn, first_game)
        torch.cuda.synchronize()
        out = {k: getattr(search, k).cpu().numpy() for k in ("move", "na", "stats") + (("prior",) if puct else ())}
        return search, roots, rec.log, seen, out
    finally:
        eng.close()


def expected(family, search, roots, parts, first_game, main):
    """[(method, {argument: value})]: the arguments the specification fixes; `other` in place of
    a stream: any stream but `main`."""
    _, prefix, puct, _, _ = FAMILIES[family]
    s, ptr = search, lambda t, rows: t.data_ptr() + rows * t.stride(0) * t.element_size()
    flushes = 1 + -(-(SIMS - 1) // BS) if puct else -(-SIMS // BS)
    log = [(prefix + "_begin", dict(first_game=first_game, n=N, d_roots=roots.data_ptr(), sims=SIMS, batch_size=BS,
                                    stream=main, **(dict(d_search_no=s.search_no.data_ptr()) if puct else {})))]
    for f in range(flushes):
        for i, (lo, hi) in enumerate(parts):
            st = main if i == 0 else "other"
            where = dict(first_game=first_game + lo, n=hi - lo, flush=f, stream=st)
            log.append((prefix + "_select", dict(where, d_leaves=ptr(s.leaves, lo * BS), d_planes=ptr(s.planes, lo * BS),
                                                 planes_f16=True, d_counts=ptr(s.counts, lo),
                                                 **(dict(planes_nhwc=False) if prefix == "chess_puct" else {}))))
            if puct and f == 0:
                log.append((prefix + "_backup", dict(where, rows=1, logits_f16=False)))
            elif puct:
                log.append((prefix + "_backup", dict(where, rows=0, logits_f16=False, d_values=ptr(s.values, lo * BS))))
            else:
                log.append((prefix + "_backup", dict(where, d_values=ptr(s.values, lo * BS))))
    log.append((prefix + "_end", dict(first_game=first_game, n=N, d_move=s.move.data_ptr(), d_na=s.na.data_ptr(),
                                      d_stats=s.stats.data_ptr(), stream=main,
                                      **(dict(d_prior=s.prior.data_ptr(), temperature=0.0) if puct else {}))))
    return log


def expected_boards(family, parts):
    puct = FAMILIES[family][2]
    if puct:   # the roots, then every slot of every flush
        return [(hi - lo) * (1 if f == 0 else BS) for f in range(4) for lo, hi in parts]
    return [(hi - lo) * min(BS, SIMS - f * BS) for f in range(3) for lo, hi in parts]


def relative(search, log):
    """The log with every pointer as (buffer, byte offset), or "temporary" outside the search's
    buffers: comparable between two search objects."""
    bufs = {k: getattr(search, k) for k in ("leaves", "planes", "counts", "values", "move", "na", "stats")}
    for k in ("prior", "search_no"):
        if hasattr(search, k):
            bufs[k] = getattr(search, k)

    def rel(key, v):
        if not key.startswith("d_") or not v:
            return v
        for name, t in bufs.items():
            if t.data_ptr() <= v < t.data_ptr() + t.numel() * t.element_size():
                return (name, v - t.data_ptr())
        return "temporary"
    return [(m, {k: rel(k, v) for k, v in a.items()}) for m, a in log]


def check_log(log, want, main):
    assert [m for m, _ in log] == [m for m, _ in want]
    for (m, got), (_, exp) in zip(log, want):
        for k, v in exp.items():
            if k == "stream" and v == "other":
                assert got[k] not in (main, 0), (m, got)
            else:
                assert got[k] == v, (m, k, got, v)


@pytest.mark.parametrize("first_game", [0, 1])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_launch_sequence(family, first_game):
    main = torch.cuda.Stream()
    runs = {form: run_form(family, form, first_game, main) for form in ("one", "list1", "list2")}
    for form, (search, roots, log, seen, out) in runs.items():
        parts = PARTS2 if form == "list2" else [(0, N)]
        check_log(log, expected(family, search, roots, parts, first_game, main.cuda_stream), main.cuda_stream)
        assert seen == expected_boards(family, parts), form
        assert (out["stats"][:, 5] == 0).all()
    # one callable is a list of one
    one, list1 = runs["one"], runs["list1"]
    assert relative(one[0], one[2]) == relative(list1[0], list1[2])
    # and the parts search what the whole searches
    for form in ("list1", "list2"):
        for k, v in runs["one"][4].items():
            assert np.array_equal(v, runs[form][4][k]), (form, k)
