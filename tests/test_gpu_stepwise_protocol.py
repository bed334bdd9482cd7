"""The C library's argument checks on the four stepwise searches (include/zeroclone.h:
zc_c4_ext_*, zc_chess_ext_*, zc_chess_puct_*, zc_c4_puct_*), called through ctypes so that
every argument can be wrong on its own: a step before any begin, games outside the begin
call's range, a flush outside the search's flushes, null buffers, bad dtype codes.

Engines of 4 games, 16 simulations, batch 4; a search of 10 simulations at batch 4 on games
[1, 3): the value searches have ceil(10 / 4) = 3 flushes, the PUCT searches 1 + ceil(9 / 4) =
4.  Apart from the begins every probe is either refused or covers no game, so none of them
launches a kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIMS, BS = 10, 4
FIRST, N = 1, 2          # the search's games: [1, 3)
F16, F16_NHWC32 = 1, 2   # ZC_F16, ZC_F16_NHWC32


class Step:
    """One entry point after begin.  kind: "range" (first, n, flush), "end" (first, n) or "hp"
    (game, flush, leaf); tail(p, **kw): the arguments between those and the stream, p[name]
    the pointer for buffer `name`; required: the buffers that must not be null when n > 0."""

    def __init__(self, sym, kind, tail, required=()):
        self.sym, self.kind, self.tail, self.required = sym, kind, tail, required

    def __repr__(self):
        return self.sym


def _select(p, code=F16):
    return [p["leaves"], p["planes"], code, p["counts"]]


def _value_steps(g):
    return [Step(f"zc_{g}_ext_select", "range", _select),
            Step(f"zc_{g}_ext_backup", "range", lambda p: [p["values"]], ("values",)),
            Step(f"zc_{g}_ext_end", "end", lambda p: [p["move"], p["na"], p["stats"]], ("move", "na", "stats")),
            Step(f"zc_{g}_hp_walk", "hp", lambda p: [p["node"]], ("node",)),
            Step(f"zc_{g}_hp_expand", "hp", lambda p: [0, p["leaf"]])]


def _puct_steps(g):
    return [Step(f"zc_{g}_puct_select", "range", _select),
            Step(f"zc_{g}_puct_backup_ex", "range",
                 lambda p, dtype=0, rows=0: [p["values"], p["logits"], dtype, rows], ("values", "logits")),
            Step(f"zc_{g}_puct_end", "end", lambda p: [0.0, p["move"], p["na"], p["prior"], p["stats"]],
                 ("move", "na", "stats"))]


def _begin(sym, extra):
    def begin(L, h, first, n, roots, sims=SIMS, **kw):
        return getattr(L, sym)(h, first, n, roots, sims, 1.4, BS, *extra(**kw), None)
    return begin


def _puct_extra(alpha=0.3, eps=0.25):
    return [alpha, eps, 7, None]


FAMILIES = {
    "c4_ext": dict(chess=False, puct=False, flushes=3, begin=_begin("zc_c4_ext_begin", lambda: []),
                   steps=_value_steps("c4")),
    "chess_ext": dict(chess=True, puct=False, flushes=3, begin=_begin("zc_chess_ext_begin", lambda: [0, 0.0]),
                      steps=_value_steps("chess") + [
                          Step("zc_chess_ext_rollouts", "range",
                               lambda p: [p["hist"], p["hist_len"], 8, p["values"], p["status"]],
                               ("hist", "hist_len", "values")),
                          Step("zc_chess_ext_leaf_moves", "range", lambda p: [p["moves"], p["depth"]],
                               ("moves", "depth"))]),
    "chess_puct": dict(chess=True, puct=True, flushes=4, begin=_begin("zc_chess_puct_begin", _puct_extra),
                       steps=_puct_steps("chess")),
    "c4_puct": dict(chess=False, puct=True, flushes=4, begin=_begin("zc_c4_puct_begin", _puct_extra),
                    steps=_puct_steps("c4")),
}


class Probe:
    """An engine, a family's table and device memory for the pointer arguments (one scratch
    block serves them all: no probe lets a kernel touch it)."""

    def __init__(self, family):
        from zeroclone_amd import _native
        self.native, self.L = _native, _native.lib()
        self.fam = FAMILIES[family]
        self.eng = _native.NativeEngine(max_games=4, max_sims=16, max_batch=4)
        self.scratch = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        if self.fam["chess"]:
            rows = np.array([_native.chess_init()] * 4, _native.CHESS_STATE_DTYPE).view(np.uint8).reshape(4, 72)
            self.roots = torch.from_numpy(rows.copy()).cuda()
        else:
            self.roots = torch.zeros((4, 3), dtype=torch.int64, device="cuda")   # empty boards, X to move

    def begin(self, first=FIRST, n=N, **kw):
        return self.fam["begin"](self.L, self.eng.handle, first, n, self.roots.data_ptr(), **kw)

    def call(self, step, first=FIRST, n=0, flush=0, leaf=0, null=None, **kw):
        ptr = self.scratch.data_ptr()
        p = {name: ptr for name in ("leaves", "planes", "counts", "values", "logits", "move", "na", "prior", "stats",
                                    "node", "leaf", "hist", "hist_len", "status", "moves", "depth")}
        if null:
            p[null] = None
        head = {"range": (first, n, flush), "end": (first, n), "hp": (first, flush, leaf)}[step.kind]
        return getattr(self.L, step.sym)(self.eng.handle, *head, *step.tail(p, **kw), None)

    def ok(self, step, **kw):
        assert self.native.check(self.call(step, **kw)) == 0, (step, kw)

    def refused(self, step, **kw):
        rc = self.call(step, **kw)
        assert rc == self.native.ZC_EINVAL, (step, kw, rc)
        with pytest.raises(ValueError):
            self.native.check(rc)

    def steps(self, *kinds):
        return [s for s in self.fam["steps"] if s.kind in kinds]

    def close(self):
        torch.cuda.synchronize()
        self.eng.close()


@pytest.fixture(params=list(FAMILIES))
def fresh(request):
    p = Probe(request.param)
    yield p
    p.close()


@pytest.fixture(scope="module", params=list(FAMILIES))
def begun(request):
    """A search of SIMS simulations at batch BS in progress on games [1, 3)."""
    p = Probe(request.param)
    assert p.native.check(p.begin()) == 0
    torch.cuda.synchronize()
    yield p
    p.close()


def test_steps_before_any_begin_are_refused(fresh):
    for s in fresh.steps("range", "end", "hp"):
        fresh.refused(s, n=0)
        fresh.refused(s, n=1)


def test_games_outside_the_begin_range_are_refused(begun):
    for s in begun.steps("range", "end"):
        begun.refused(s, first=0, n=1)
        begun.refused(s, first=2, n=2)
        begun.refused(s, first=2, n=-1)
    for s in begun.steps("hp"):
        begun.refused(s, first=0)
        begun.refused(s, first=3)


def test_flush_outside_the_search_is_refused(begun):
    F = begun.fam["flushes"]
    for s in begun.steps("range", "hp"):
        begun.refused(s, flush=-1)
        begun.refused(s, flush=F)
    for s in begun.steps("range"):
        begun.ok(s, first=2, n=0, flush=F - 1)
        begun.ok(s, first=1, n=0, flush=0)
    for s in begun.steps("end"):   # end takes no flush
        begun.ok(s, first=2, n=0)


def test_null_buffers_are_refused(begun):
    for s in begun.steps("range", "end", "hp"):
        for name in s.required:
            begun.refused(s, n=1, null=name)
            if s.kind != "hp":
                begun.ok(s, n=0, null=name)   # no game: no buffer needed


def test_host_policy_leaf_range(begun):
    """The last flush of 10 simulations at batch 4 holds 2 leaves."""
    last = begun.fam["flushes"] - 1
    for s in begun.steps("hp"):
        begun.refused(s, flush=last, leaf=2)
        begun.refused(s, flush=0, leaf=BS)
        begun.refused(s, flush=0, leaf=-1)


def test_plane_codes(begun):
    """ZC_F16_NHWC32 is the chess PUCT search's alone; no search takes an unknown code."""
    for s in begun.steps("range"):
        if s.tail is not _select:
            continue
        begun.refused(s, code=3)
        begun.refused(s, code=-1)
        if s.sym == "zc_chess_puct_select":
            begun.ok(s, code=F16_NHWC32)
        else:
            begun.refused(s, code=F16_NHWC32)


def test_puct_backup_arguments(begun):
    if not begun.fam["puct"]:
        return
    backup = next(s for s in begun.fam["steps"] if s.sym.endswith("backup_ex"))
    begun.refused(backup, rows=-1)
    begun.refused(backup, rows=1, flush=1)
    begun.refused(backup, dtype=2)
    begun.refused(backup, dtype=-1)
    begun.ok(backup, rows=1, flush=0)
    begun.ok(backup, rows=0, flush=1, dtype=1)


def test_puct_begin_arguments(fresh):
    if not fresh.fam["puct"]:
        return
    for bad in (dict(sims=1), dict(alpha=0.0), dict(eps=1.5)):
        with pytest.raises(ValueError):
            fresh.native.check(fresh.begin(**bad))
    select = fresh.fam["steps"][0]
    fresh.refused(select, n=0)   # a refused begin starts no search
    assert fresh.native.check(fresh.begin()) == 0
    fresh.ok(select, n=0)


def test_begin_over_no_game(fresh):
    """C4PuctSearch reserves its arena with such a begin."""
    assert fresh.native.check(fresh.begin(first=0, n=0)) == 0
    for s in fresh.steps("range"):
        fresh.ok(s, first=0, n=0, flush=0)
        fresh.refused(s, first=0, n=1, flush=0)
