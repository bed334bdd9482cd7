"""The trajectory recorder's kernels (csrc/selfplay.hip) against tests/traj_ref.py on scripted
self-play tables: no engine, no search, no network.  Every case runs through the single-step
calls, step by step, and, where the quota is unlimited, again through the multi-step calls; both
must leave, bit for bit, what the model specifies.  Every buffer is a slice of a larger tensor
whose rows before and after it are guards, checked at the end of every case; what a case never
writes keeps a second fill value, so a stray write inside a buffer shows too."""
import ctypes

import numpy as np
import pytest
import torch

import traj_ref as tr
from traj_ref import TrajModel
from zeroclone_amd import _native
from zeroclone_amd.selfplay import Trajectories

pytestmark = pytest.mark.gpu

GUARD, FILL, PAD = -21555, -21777, 64
POISON_RESULT, POISON_MOVE, POISON_COUNT = 12345, 0x5A5A, 70000   # would show if read
VP = ctypes.c_void_p


def guarded(rows, width, dtype):
    """[rows][width] of FILL between PAD guard rows of GUARD on either side."""
    big = torch.full((rows + 2 * PAD, width), GUARD, dtype=dtype, device="cuda")
    big[PAD:PAD + rows] = FILL
    return big, big[PAD:PAD + rows]


class Cfg:
    def __init__(self, n, words, max_len, pool_cap, games_cap, quota=None, slot_cap=None, pi_pool_cap=0):
        self.__dict__.update(locals())

    def model(self, **over):
        c = {**self.__dict__, **over}
        return TrajModel(c["n"], tr.init_row(c["words"]), c["max_len"], c["pool_cap"], c["games_cap"], c["quota"],
                         c["slot_cap"], c["pi_pool_cap"])

    def but(self, **over):
        c = {k: v for k, v in {**self.__dict__, **over}.items() if k != "self"}
        return Cfg(**c)


class Dev:
    """The recorder's buffers, hand-built: zc_traj_buffers / zc_traj_policy_buffers over guarded
    slices, started as Trajectories.start starts them."""

    def __init__(self, c: Cfg):
        self.c, n, W, ml = c, c.n, c.words, c.max_len
        self.big = {}
        shapes = {"hist": (n * ml, W, torch.int64), "hmoves": (n * ml, 1, torch.int16), "slot": (n, 4, torch.int32),
                  "pool": (c.pool_cap, W, torch.int64), "labels": (c.pool_cap, 1, torch.int32),
                  "pool_moves": (c.pool_cap, 1, torch.int16), "games": (c.games_cap, 4, torch.int64),
                  "ctl": (1, 8, torch.int64), "init": (1, W, torch.int64)}
        if c.slot_cap is not None:
            shapes.update({"slot_pi": (n * c.slot_cap, 1, torch.int32), "slot_off": (n, ml + 1, torch.int32),
                           "slot_base": (n, 1, torch.int64), "pool_pi": (c.pi_pool_cap, 1, torch.int32),
                           "pool_first": (c.pool_cap, 1, torch.int64), "pool_count": (c.pool_cap, 1, torch.int32),
                           "pctl": (1, 4, torch.int64)})
        for name, (rows, width, dtype) in shapes.items():
            self.big[name], t = guarded(rows, width, dtype)
            setattr(self, name, t)
        q = tr.UNLIMITED if c.quota is None else c.quota
        ids = torch.arange(n, dtype=torch.int32, device="cuda")
        self.init[0] = torch.tensor(tr.init_row(W), dtype=torch.int64)
        self.slot.zero_()
        self.slot[:, 0] = 1
        self.slot[:, 1] = torch.where(ids < min(q, n), ids, torch.full_like(ids, -1))
        self.hist.view(n, ml, W)[:, 0] = self.init[0]
        self.ctl.zero_()
        self.ctl[0, _native.ZC_TRAJ_NEXT] = min(q, n)
        self.ctl[0, _native.ZC_TRAJ_QUOTA] = q
        b = _native.TrajBuffers()
        b.row_bytes, b.max_len, b.pool_cap, b.games_cap = 8 * W, ml, c.pool_cap, c.games_cap
        for f in ("hist", "hmoves", "slot", "pool", "labels", "pool_moves", "games", "ctl", "init"):
            setattr(b, "d_" + f, getattr(self, f).data_ptr())
        self.buf = b
        if c.slot_cap is not None:
            self.slot_off[:, 0] = 0
            self.pctl.zero_()
            p = _native.TrajPolicyBuffers()
            p.slot_cap, p.pi_pool_cap = c.slot_cap, c.pi_pool_cap
            for f in ("slot_pi", "slot_off", "slot_base", "pool_pi", "pool_first", "pool_count", "pctl"):
                setattr(p, "d_" + f, getattr(self, f).data_ptr())
            self.pol = p
        self.lib = _native.lib()
        self.stream = VP(torch.cuda.current_stream().cuda_stream or None)

    # ---------------------------------------------------------------- the calls
    def upload(self, t, lo, hi):
        d = {k: torch.from_numpy(np.ascontiguousarray(v[lo:hi].view(np.int16) if v.dtype == np.uint16 else v[lo:hi]))
             .cuda() for k, v in t.items() if v is not None}
        return d

    def single(self, t, lo, hi, policy=False, chess=False, rep=True):
        """Steps [lo, hi) through append / record / commit; returns the tables as the calls left them."""
        d = self.upload(t, lo, hi)
        n = self.c.n
        if policy:                                   # a slot without a move was not searched
            d["na"][d["results"] == tr.SKIP] = 0
        for k in range(hi - lo):
            if policy:
                rm = d.get("root_moves")
                _native.check(self.lib.zc_traj_policy_append_async(
                    n, ctypes.byref(self.buf), ctypes.byref(self.pol), VP(d["na"][k].data_ptr()),
                    VP(rm[k].data_ptr() if rm is not None else None), d["na"].shape[2], self.stream))
            _native.check(self.lib.zc_traj_record_async(
                n, ctypes.byref(self.buf), VP(d["states"][k].data_ptr()), VP(d["moves"][k].data_ptr()),
                VP(d["results"][k].data_ptr()), VP(d["flags"][k].data_ptr() if chess else None),
                VP(d["rep"][k].data_ptr() if chess and rep else None), self.stream))
            if policy:
                _native.check(self.lib.zc_traj_policy_commit_async(n, ctypes.byref(self.buf), ctypes.byref(self.pol),
                                                                   self.stream))
        torch.cuda.synchronize()
        return d

    def multi(self, t, lo, hi, policy=False, reached=None):
        """Steps [lo, hi) through the multi-step calls, the policy's first; the rows at and above
        `reached` and the visit counts of slots without a move hold values that would show."""
        d = self.upload(t, lo, hi)
        n, steps = self.c.n, hi - lo
        kr = TrajModel.reached_steps(steps, reached)
        d["results"][kr:] = POISON_RESULT
        d["moves"][kr:] = POISON_MOVE
        d["states"][kr:] = 0x5A5A5A5A5A5A5A5A
        if policy:
            d["na"][kr:] = POISON_COUNT
            d["na"][d["results"] == tr.SKIP] = POISON_COUNT
        sent = {k: v.clone() for k, v in d.items()}
        d_reached = None if reached is None else torch.tensor([reached], dtype=torch.int32, device="cuda")
        r_ptr = VP(d_reached.data_ptr() if d_reached is not None else None)
        need = ctypes.c_int64(0)
        if policy:
            _native.check(self.lib.zc_traj_policy_steps_scratch_bytes(n, steps, ctypes.byref(need)))
            self.big["pscratch"] = ps = torch.full((need.value + 16 * PAD,), 0x5C, dtype=torch.uint8, device="cuda")
            rm = d.get("root_moves")
            _native.check(self.lib.zc_traj_policy_record_steps_async(
                n, ctypes.byref(self.buf), ctypes.byref(self.pol), VP(d["results"].data_ptr()), VP(d["na"].data_ptr()),
                VP(rm.data_ptr() if rm is not None else None), d["na"].shape[2], steps, r_ptr, VP(ps.data_ptr()),
                need.value, self.stream))
            self.scratch_tail = [(ps, need.value)]
        else:
            self.scratch_tail = []
        _native.check(self.lib.zc_traj_steps_scratch_bytes(n, steps, ctypes.byref(need)))
        sc = torch.full((need.value + 16 * PAD,), 0x5C, dtype=torch.uint8, device="cuda")
        _native.check(self.lib.zc_traj_record_steps_async(
            n, ctypes.byref(self.buf), VP(d["states"].data_ptr()), VP(d["moves"].data_ptr()),
            VP(d["results"].data_ptr()), steps, r_ptr, VP(sc.data_ptr()), need.value, self.stream))
        self.scratch_tail.append((sc, need.value))
        torch.cuda.synchronize()
        for k, v in d.items():                       # the launch's tables are not modified
            assert torch.equal(v, sent[k]), k
        for s, used in self.scratch_tail:
            assert bool((s[used:] == 0x5C).all()), "scratch written past its declared size"

    # ---------------------------------------------------------------- the comparison
    def check(self, m: TrajModel):
        c, n, W, ml = self.c, self.c.n, self.c.words, self.c.max_len
        for name, big in self.big.items():
            if name == "pscratch":
                continue
            assert bool((big[:PAD] == GUARD).all()) and bool((big[-PAD:] == GUARD).all()), f"guard of {name}"
        ctl = self.ctl[0].tolist()
        assert ctl[:6] == [m.positions, m.n_games, m.next, m.quota, m.finished, m.overflow], "d_ctl"
        assert ctl[6:] == [0, 0]
        slot = self.slot[:, :2].tolist()
        assert slot == m.slot, "slot table"
        hist, hmoves = self.hist.view(n, ml, W).tolist(), self.hmoves.view(n, ml).tolist()
        for g in range(n):
            ln = m.slot[g][0]
            rows, mv = (ml - 1, ml - 2) if g in m.unspecified else (ln, ln - 1)
            assert [tuple(r) for r in hist[g][:rows]] == m.hist[g][:rows], f"history of slot {g}"
            assert hmoves[g][:mv] == m.hmoves[g][:mv], f"moves of slot {g}"
        fill_row = (FILL,) * W
        assert [tuple(r) for r in self.pool.tolist()] == [fill_row if r is None else r for r in m.pool], "d_pool"
        assert self.labels[:, 0].tolist() == [FILL if v is None else v for v in m.labels], "d_labels"
        assert self.pool_moves[:, 0].tolist() == [FILL if v is None else v for v in m.pool_moves], "d_pool_moves"
        want = [[FILL] * 4 if r is None else [r[0], r[1] << 32 | (r[2] + 1), r[3], r[4]] for r in m.games]
        assert self.games.tolist() == want, "d_games"
        if c.slot_cap is None:
            return
        assert self.pctl[0].tolist() == [m.entries, m.pi_overflow, 0, 0], "d_pctl"
        off, spi = self.slot_off.tolist(), self.slot_pi.view(n, c.slot_cap).tolist()
        for g in range(n):
            if g in m.unspecified:
                continue
            ln = m.slot[g][0]
            assert off[g][:ln] == m.slot_off[g][:ln], f"offsets of slot {g}"
            have = m.slot_off[g][ln - 1]
            assert [v & 0xFFFFFFFF for v in spi[g][:have]] == m.slot_pi[g][:have], f"entries of slot {g}"
        u32 = lambda v: v & 0xFFFFFFFF   # noqa: E731
        assert [u32(v) for v in self.pool_pi[:, 0].tolist()] == [u32(FILL) if v is None else v for v in m.pool_pi], \
            "d_pool_pi"
        assert self.pool_first[:, 0].tolist() == [FILL if v is None else v for v in m.pool_first], "d_pool_first"
        assert self.pool_count[:, 0].tolist() == [FILL if v is None else v for v in m.pool_count], "d_pool_count"


def model_single(m, t, lo, hi, policy=False, chess=False, rep=True):
    """Steps [lo, hi) through the model's single steps; returns the states and results the calls
    leave in the tables."""
    st_out, res_out = t["states"][lo:hi].copy(), t["results"][lo:hi].copy()
    for k in range(lo, hi):
        res = [int(x) for x in t["results"][k]]
        states = [tuple(int(x) for x in r) for r in t["states"][k]]
        nak = None
        if policy:
            nak = [t["na"][k][g] if res[g] != tr.SKIP else () for g in range(m.n)]
        m.step(states, t["moves"][k], res, nak, t.get("root_moves")[k] if policy and t.get("root_moves") is not None
               else None, t["flags"][k] if chess else None, t["rep"][k] if chess and rep else None)
        st_out[k - lo], res_out[k - lo] = np.array(states, dtype=np.int64), res
    return st_out, res_out


def run_case(c: Cfg, t, steps, policy=False, pre=0, reached=None, multi=True, chess=False):
    """The case through single steps and (multi) with its first `pre` steps through single steps and
    the rest in one multi-step call; each against a model of its own.  Returns the two models."""
    kr = pre + TrajModel.reached_steps(steps - pre, reached)
    m1, d1 = c.model(), Dev(c)
    want_states, want_results = model_single(m1, t, 0, kr, policy, chess)
    left = d1.single(t, 0, kr, policy, chess)
    d1.check(m1)
    assert np.array_equal(left["results"].cpu().numpy(), want_results), "d_results after single steps"
    assert np.array_equal(left["states"].cpu().numpy(), want_states), "d_states after single steps"
    if not multi:
        return m1, None
    m2, d2 = c.model(), Dev(c)
    model_single(m2, t, 0, pre, policy, chess)
    d2.single(t, 0, pre, policy, chess)
    sl = slice(pre, steps)
    if policy:
        rm = t.get("root_moves")
        m2.policy_record_steps(t["results"][sl], t["na"][sl], None if rm is None else rm[sl], steps - pre, reached)
        m2.record_steps_after_policy(t["states"][sl], t["moves"][sl], t["results"][sl], steps - pre, reached)
    else:
        m2.record_steps(t["states"][sl], t["moves"][sl], t["results"][sl], steps - pre, reached)
    d2.multi(t, pre, steps, policy, reached)
    d2.check(m2)
    return m1, m2


def sized(c: Cfg, t, steps):
    """The positions and game records the table's finished games need."""
    m = c.but(pool_cap=1 << 14, games_cap=1 << 10, slot_cap=None).model()
    model_single(m, t, 0, steps)
    return m.positions, m.n_games


def _len_pattern(kind, n):
    if kind == "twos":                      # every live slot finishes at every step
        return [[2] * 8 for _ in range(n)]
    return [[2 + (g * 7 // 3 + i) % 2 for i in range(8)] for g in range(n)]   # 2 and 3 mixed along the slots


# ------------------------------------------------------------------ slot chunks
@pytest.mark.parametrize("kind", ["twos", "mixed"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_slot_chunks(n, kind):
    steps = 5 if n < 1000 else 3
    t = tr.scripted(n, steps, 8, _len_pattern(kind, n), stride=7)
    c = Cfg(n, 1, 4, 3 * n * steps, n * steps, slot_cap=3 * 7, pi_pool_cap=7 * 2 * n * steps)
    m1, m2 = run_case(c, t, steps, policy=True)
    assert m1.finished >= n * (steps // 2) and m1.overflow == 0 and m1.pi_overflow == 0
    if kind == "mixed" and n > 1024:        # finishes on both sides of a 1024 boundary in one step
        fins = [np.nonzero(t["results"][k] != tr.ONGOING)[0] for k in range(steps)]
        assert any(f.min() < 1024 <= f.max() for f in fins)


# ------------------------------------------------------------------ step chunks
def _step_lengths(steps):
    """Slot 0 finishes at step 63, slot 1 at step 64, slot 2 at 59, 70 (a game spanning 60 to 70),
    80 and 100 (two finishes in one 64-step chunk) and then not before step 200; afterwards short
    and long games mixed, the last one cut so that slot 0 finishes at the last step, slot 1 at the
    one before and slot 2 at step 1024 (where the table has one)."""
    tail = (2, 3, 5, 17, 64, 65, 66, 100, 2, 2, 31)
    out = [[65], [66], [61, 12, 11, 21, 101]]
    for g, ls in enumerate(out):
        total = (steps - g if g < 2 or steps <= 1024 else 1025)   # moves up to the slot's last finish
        cur, i = sum(x - 1 for x in ls), 0
        if cur >= total:
            continue
        while cur + tail[(i * 3 + g) % len(tail)] - 1 < total:
            ls.append(tail[(i * 3 + g) % len(tail)])
            cur, i = cur + ls[-1] - 1, i + 1
        ls.append(total - cur + 1)
    return out


@pytest.mark.parametrize("steps", [63, 64, 65, 128, 129, 1024, 1025, 1030])
def test_step_chunks(steps):
    lengths = _step_lengths(steps)
    t = tr.scripted(3, steps, 8, lengths, stride=7)
    fin = [np.nonzero(t["results"][:, g] != tr.ONGOING)[0].tolist() for g in range(3)]
    if steps > 100:
        assert fin[0][0] == 63 and fin[1][0] == 64 and fin[2][:4] == [59, 70, 80, 100]
        assert fin[2][4:5] == [200][:steps > 200]
    if steps > 200:                          # the last finishes: the last two steps, and step 1024
        assert [f[-1] for f in fin] == [steps - 1, steps - 2, 1024 if steps > 1024 else steps - 3]
    c = Cfg(3, 1, 128, 3 * steps + 400, steps + 8, slot_cap=127 * 7, pi_pool_cap=7 * (3 * steps + 400))
    m1, m2 = run_case(c, t, steps, policy=True)
    assert m1.overflow == 0 and m1.pi_overflow == 0 and m1.finished == sum(len(f) for f in fin)


@pytest.mark.parametrize("row_bytes", [8, 24, 72])
def test_game_in_progress_before_the_call(row_bytes):
    """Games 5 positions long when the multi-step call begins: one finishes at the call's step 0,
    one at its step 64, one not at all."""
    pre, steps = 4, 4 + 70
    t = tr.scripted(3, steps, row_bytes, [[6, 3], [70, 2], [200]], stride=7)
    assert t["results"][pre, 0] != tr.ONGOING and t["results"][pre + 64, 1] != tr.ONGOING
    c = Cfg(3, row_bytes // 8, 80, 400, 40, slot_cap=79 * 7, pi_pool_cap=3000)
    m1, m2 = run_case(c, t, steps, policy=True, pre=pre)
    assert m2.slot[2] == [steps + 1, 2] and m2.finished == m1.finished > 2


@pytest.mark.parametrize("row_bytes", [8, 24, 72])
def test_row_sizes(row_bytes):
    n, steps = 70, 9
    t = tr.scripted(n, steps, row_bytes, [[2 + (g + i) % 4 for i in range(9)] for g in range(n)])
    c = Cfg(n, row_bytes // 8, 6, 2 * n * steps, n * steps)
    m1, _ = run_case(c, t, steps)
    assert m1.finished > 2 * n


# ------------------------------------------------------------------ SKIP and reached
@pytest.mark.parametrize("reached", [None, 0, -7, "steps-1", "steps", "steps+5"])
def test_skip_and_reached(reached):
    n, steps = 67, 12
    reached = {"steps-1": steps - 1, "steps": steps, "steps+5": steps + 5}.get(reached, reached)
    lengths = [[2 + (g + i) % 3 for i in range(12)] for g in range(n)]
    skip = [None if g % 4 == 0 else (g * 5) % (steps + 1) for g in range(n)]      # 0 .. steps: stops at once, never
    t = tr.scripted(n, steps, 24, lengths, stride=7, skip_after=skip, skip_move=-1)   # -1 = 0xFFFF in 16 bits
    # after a slot's first step without a move the table may hold anything but a move
    for g in range(n):
        if skip[g] is not None and skip[g] + 1 < steps and g % 3 == 0:
            t["moves"][skip[g] + 1:, g] = POISON_MOVE
    c = Cfg(n, 3, 5, 3 * n * steps, n * steps, slot_cap=4 * 7, pi_pool_cap=7 * 3 * n * steps)
    m1, m2 = run_case(c, t, steps, policy=True, reached=reached)
    if reached is None or reached >= steps - 1:
        assert m1.finished > n


# ------------------------------------------------------------------ chess results
@pytest.mark.parametrize("rep", [False, True], ids=["rep-absent", "rep"])
def test_chess_results_single_step(rep):
    """Every combination of the WIN / STALEMATE / FIFTY bits with rep in {0, 2, 3} and both turns;
    two idle slots; then a second step on the restarted slots."""
    combos = [(f, r, turn) for f in range(8) for r in (0, 2, 3) for turn in (0, 1)]
    n = len(combos) + 2
    t = tr.scripted(n, 2, 72, [[9]] * n, chess=True)
    for g, (f, r, turn) in enumerate(combos):
        for k in range(2):
            t["flags"][k, g], t["rep"][k, g] = f, (r if k == 0 else (0, 2, 3)[(g + 1) % 3])
            t["states"][k, g, 8] = (int(t["states"][k, g, 8]) & ~0xFF) | (turn ^ k)
    t["results"][:] = 77
    c = Cfg(n, 9, 6, 3 * 2 * n, 2 * n)
    m, d = c.model(), Dev(c)                 # the last two slots idled by hand: the refills go on
    for g in (n - 2, n - 1):
        m.slot[g] = [1, -1]
    d.slot[n - 2:, 1] = -1
    want_states, want_results = model_single(m, t, 0, 2, chess=True, rep=rep)
    left = d.single(t, 0, 2, chess=True, rep=rep)
    d.check(m)
    assert np.array_equal(left["results"].cpu().numpy(), want_results)
    assert np.array_equal(left["states"].cpu().numpy(), want_states)
    assert want_results[0, -2:].tolist() == [tr.IDLE] * 2
    for g, (f, r, turn) in enumerate(combos):
        want = turn * 2 - 1 if f & 1 else (0 if f & 6 or (rep and r == 3) else tr.ONGOING)
        assert want_results[0, g] == want


# ------------------------------------------------------------------ quota
@pytest.mark.parametrize("quota", [0, 3, 5, 6])
def test_quota_single_steps(quota):
    n, steps = 5, 9
    t = tr.scripted(n, steps, 24, [[2, 3, 2, 2], [3, 2, 4], [4, 2], [2, 2, 2, 2, 2], [5, 3]], stride=7)
    c = Cfg(n, 3, 6, 120, 40, quota=quota, slot_cap=35, pi_pool_cap=400)
    m, _ = run_case(c, t, steps, policy=True, multi=False)
    assert m.overflow == 0 and m.finished == quota and all(s == [1, -1] for s in m.slot)


def test_quota_runs_out_inside_a_multi_step_record():
    """Quota n + 1: at the call's last step slots 1 and 3 finish; slot 1 takes the last game, slot 3's
    refill passes the quota (bit 2) and the slot goes idle."""
    n, steps = 5, 4
    t = tr.scripted(n, steps, 8, [[9], [5], [9], [5], [9]], stride=7)
    c = Cfg(n, 1, 8, 40, 8, quota=n + 1, slot_cap=49, pi_pool_cap=100)
    m1, m2 = run_case(c, t, steps, policy=True)
    assert m1.overflow == 0 and m2.overflow == tr.OV_QUOTA
    assert m2.slot[1] == [1, n] and m2.slot[3] == [1, -1] and m2.games[:2] == m1.games[:2]


# ------------------------------------------------------------------ capacity
CAP_TABLE = dict(n=6, steps=7, lengths=[[3, 2, 4], [2, 5], [4, 4], [8], [2, 2, 2, 3], [9]])


def _cap_case(policy=True):
    t = tr.scripted(CAP_TABLE["n"], CAP_TABLE["steps"], 24, CAP_TABLE["lengths"], stride=7)
    c = Cfg(6, 3, 8, 0, 0, slot_cap=49 if policy else None, pi_pool_cap=2000)
    return t, c, sized(c, t, 7)


@pytest.mark.parametrize("short", [0, 1, 9])
def test_pool_cap_exact_fit_and_short(short):
    t, c, (positions, games) = _cap_case()
    m1, m2 = run_case(c.but(pool_cap=positions - short, games_cap=games), t, 7, policy=True)
    for m in (m1, m2):
        assert m.overflow == (tr.OV_POOL if short else 0) and (m.positions, m.n_games) == (positions, games)
        dropped = [r is None for r in m.games]
        assert (sum(dropped) == short if short < 2 else sum(dropped) > 1) and dropped == sorted(dropped)
        assert m.pi_overflow == 0 and (short == 0) == (None not in m.pool)


@pytest.mark.parametrize("short", [0, 1, 4])
def test_games_cap_exact_fit_and_short(short):
    t, c, (positions, games) = _cap_case()
    m1, m2 = run_case(c.but(pool_cap=positions, games_cap=games - short), t, 7, policy=True)
    for m in (m1, m2):
        assert m.overflow == (tr.OV_POOL if short else 0) and (m.positions, m.n_games) == (positions, games)
        assert (None in m.pool) == bool(short)


@pytest.mark.parametrize("over", [0, 1])
def test_max_len_exact_fit_and_one_more(over):
    """max_len 8: slot 3's game of 8 positions fits; slot 5's game reaches 8 positions at the last
    step (over = 0) or 9 one step later (bit 1: the flag, the other slots, the guards)."""
    steps = 7 + over
    t = tr.scripted(6, steps, 24, CAP_TABLE["lengths"][:5] + [[12]])
    c = Cfg(6, 3, 8, 100, 20)
    m1, m2 = run_case(c, t, steps)
    for m in (m1, m2):
        assert m.overflow == (tr.OV_MAXLEN if over else 0) and m.unspecified == ({5} if over else set())
        assert m.slot[5] == [8, 5] and any(r[4] == 8 for r in m.games if r)


# ------------------------------------------------------------------ policy rows
NNZ_256 = (0, 1, 63, 64, 65, 128, 129, 256)


def _nnz_cases(g, j, p, stride):
    if p == 1 and g % 2 == 0:
        return 0                            # an all-zero row in the middle of a game
    return NNZ_256[(g + 3 * j + p) % 8] * stride // 256 if stride == 256 else (0, 1, 7, 3)[(g + j + p) % 4]


POLICY_LENGTHS = [[3, 2, 4, 3, 3] if g % 3 else [4, 4, 2, 5] for g in range(9)]


@pytest.mark.parametrize("stride,ids", [(7, False), (_native.CHESS_MAX_MOVES, True)])
def test_policy_rows(stride, ids):
    """Rows with 0 .. all cells non-zero, an all-zero row in the middle of a game, games that start
    and end inside the call, slots that finish twice and go on."""
    n, steps = 9, 8
    t = tr.scripted(n, steps, 8, POLICY_LENGTHS, stride=stride, with_ids=ids, nnz=_nnz_cases)
    seen = {int(x) for x in (t["na"] > 0).sum(2).reshape(-1)}
    assert seen >= (set(NNZ_256) if stride == 256 else {0, 1, 3, 7})
    c = Cfg(n, 1, 6, 200, 40, slot_cap=5 * stride, pi_pool_cap=200 * stride)
    m1, m2 = run_case(c, t, steps, policy=True)
    assert m1.pi_overflow == 0 and m1.finished >= 2 * n
    zero_mid = [p for p in range(m1.positions - 1) if m1.pool_count[p] == 0 and m1.pool_moves[p] != -1
                and m1.pool_first[p + 1] == m1.pool_first[p]]
    assert zero_mid, "no all-zero row inside a game"
    assert all(m1.pool_count[p] == 0 for p in range(m1.positions) if m1.pool_moves[p] == -1)


@pytest.mark.parametrize("count,bit", [(65535, 0), (65536, tr.PI_SAT), (1 << 30, tr.PI_SAT)])
def test_policy_count_saturates(count, bit):
    n, steps = 3, 6
    t = tr.scripted(n, steps, 8, [[3, 3, 3]] * n, stride=7, nnz=lambda g, j, p, s: 5)
    cells = [(k, g) for k in range(steps) for g in range(n) if (k + g) % 3 == 0]
    for k, g in cells:
        c0 = int(np.nonzero(t["na"][k, g])[0][1])
        t["na"][k, g, c0] = count
    c = Cfg(n, 1, 4, 100, 20, slot_cap=21, pi_pool_cap=300)
    m1, m2 = run_case(c, t, steps, policy=True)
    assert m1.pi_overflow == bit == m2.pi_overflow
    assert sum(1 for e in m1.pool_pi if e is not None and e >> 16 == 65535) >= len(cells) // 2


@pytest.mark.parametrize("short", [0, 1])
def test_policy_slot_cap_exact_fit_and_short(short):
    n, steps = 9, 8
    t = tr.scripted(n, steps, 8, POLICY_LENGTHS, stride=256, with_ids=True, nnz=_nnz_cases)
    m0 = Cfg(n, 1, 6, 200, 40, slot_cap=1 << 14, pi_pool_cap=1 << 16).model()
    model_single(m0, t, 0, steps, True)
    per_game = max([m0.pool_first[r[3] + r[4] - 1] - m0.pool_first[r[3]] for r in m0.games if r]
                   + [len(e) for e in m0.slot_pi])
    c = Cfg(n, 1, 6, 200, 40, slot_cap=per_game - short, pi_pool_cap=1 << 16)
    m1, m2 = run_case(c, t, steps, policy=True)
    assert m1.pi_overflow == (tr.PI_SLOT if short else 0) == m2.pi_overflow
    assert m1.entries < m0.entries if short else m1.entries == m0.entries


@pytest.mark.parametrize("short", [0, 1, 300])
def test_policy_pool_cap_exact_fit_and_short(short):
    n, steps = 9, 8
    t = tr.scripted(n, steps, 8, POLICY_LENGTHS, stride=256, with_ids=True, nnz=_nnz_cases)
    m0 = Cfg(n, 1, 6, 200, 40, slot_cap=1 << 14, pi_pool_cap=1 << 16).model()
    model_single(m0, t, 0, steps, True)
    c = Cfg(n, 1, 6, 200, 40, slot_cap=5 * 256, pi_pool_cap=m0.entries - short)
    m1, m2 = run_case(c, t, steps, policy=True)
    for m in (m1, m2):
        assert m.pi_overflow == (tr.PI_POOL if short else 0) and m.entries == m0.entries and m.overflow == 0
        zeroed = [r for r in m.games if r and all(m.pool_first[p] == 0 and m.pool_count[p] == 0
                                                  for p in range(r[3], r[3] + r[4]))]
        assert bool(zeroed) == bool(short)


def test_a_game_the_pool_drops_reserves_no_entries():
    t, c, (positions, games) = _cap_case()
    m0 = c.but(pool_cap=positions, games_cap=games).model()
    model_single(m0, t, 0, 7, True)
    m1, m2 = run_case(c.but(pool_cap=positions - 9, games_cap=games), t, 7, policy=True)
    for m in (m1, m2):
        kept = [r for r in m.games if r]
        want = sum(m0.pool_count[p] for r in kept for p in range(r[3], r[3] + r[4]))
        assert m.entries == want < m0.entries and m.pi_overflow == 0


# ------------------------------------------------------------------ refusals
def test_multi_step_calls_refuse_bad_arguments():
    c = Cfg(3, 1, 4, 20, 8, slot_cap=21, pi_pool_cap=60)
    d, lib = Dev(c), _native.lib()
    t = d.upload(tr.scripted(3, 4, 8, [[3]] * 3, stride=7), 0, 4)
    sc = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    need = ctypes.c_int64(0)
    _native.check(lib.zc_traj_steps_scratch_bytes(3, 4, ctypes.byref(need)))

    def rec(n=3, steps=4, scratch=sc.data_ptr(), nbytes=1 << 16, buf=d.buf):
        return lib.zc_traj_record_steps_async(n, ctypes.byref(buf), VP(t["states"].data_ptr()),
                                              VP(t["moves"].data_ptr()), VP(t["results"].data_ptr()), steps, None,
                                              VP(scratch), nbytes, d.stream)

    def pol(stride=7, steps=4, scratch=sc.data_ptr(), nbytes=1 << 16):
        return lib.zc_traj_policy_record_steps_async(3, ctypes.byref(d.buf), ctypes.byref(d.pol),
                                                     VP(t["results"].data_ptr()), VP(t["na"].data_ptr()), None, stride,
                                                     steps, None, VP(scratch), nbytes, d.stream)
    bad = _native.TrajBuffers.from_buffer_copy(d.buf)
    bad.max_len = 1
    for rc in (rec(steps=-1), rec(scratch=sc.data_ptr() + 8), rec(nbytes=need.value - 1), rec(scratch=None),
               rec(n=1 << 20, steps=1 << 11), rec(buf=bad), pol(stride=0), pol(stride=65537), pol(steps=-1),
               pol(nbytes=need.value), pol(scratch=sc.data_ptr() + 4)):
        assert rc == _native.ZC_EINVAL
    assert rec(steps=0) == 0 and pol(steps=0) == 0 and rec(n=0) == 0
    torch.cuda.synchronize()
    d.check(c.model())                         # the refused and the empty calls wrote nothing


# ------------------------------------------------------------------ through Trajectories
def _dense(batch, width):
    n = len(batch["rows"])
    out = np.zeros((n, width), np.float32)
    for i in range(n):
        ent = batch["pi"][batch["pi_off"][i]:batch["pi_off"][i + 1]]
        total = np.float32(sum(e >> 16 for e in ent))
        for e in ent:
            mid = e & 0xFFFF
            idx = mid if width == 7 else (mid & 63) * 64 + ((mid >> 6) & 63)
            out[i, idx] = np.float32(e >> 16) / total
    return out


@pytest.mark.parametrize("game", ["connect4", "chess"])
def test_through_trajectories(game):
    """Trajectories.record / record_policy / record_steps / take and TrajBatch.policy_targets
    against the model's take(): the wrapper's ordering and re-basing."""
    chess = game == "chess"
    n, steps, words = 7, 10, 9 if chess else 3
    width, stride = (4096, _native.CHESS_MAX_MOVES) if chess else (7, 7)
    lengths = [[2 + (3 * g + i) % 4 for i in range(10)] for g in range(n)]
    t = tr.scripted(n, steps, 8 * words, lengths, stride=stride, with_ids=chess, chess=chess,
                    nnz=lambda g, j, p, s: (g + j + 2 * p) % 8)
    init = torch.tensor(tr.init_row(words), dtype=torch.int64)
    dev = torch.device("cuda")
    for multi in (False, True):
        m = TrajModel(n, tr.init_row(words), 6, 400, 80, slot_cap=5 * stride, pi_pool_cap=400 * 8)
        tj = Trajectories(n, init, 6, 80, 400, dev, policy_width=width, pi_slot_cap=5 * stride, pi_pool_cap=400 * 8)
        d = {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda()
             for k, v in t.items() if v is not None}
        half = steps // 2
        for lo, hi in ((0, half), (half, steps)):          # two takes: the second re-bases again
            if multi:
                tj.record_steps(d["states"][lo:hi].data_ptr(), d["moves"][lo:hi], d["results"][lo:hi].contiguous(),
                                hi - lo, na=d["na"][lo:hi], root_moves=d["root_moves"][lo:hi] if chess else None)
                m.record_steps(t["states"][lo:hi], t["moves"][lo:hi], t["results"][lo:hi], hi - lo,
                               na=t["na"][lo:hi], root_moves=t["root_moves"][lo:hi] if chess else None)
            else:
                for k in range(lo, hi):
                    tj.record_policy(d["na"][k], d["root_moves"][k] if chess else None)
                    tj.record(d["states"][k].data_ptr(), d["moves"][k], d["results"][k],
                              d["flags"][k] if chess else None, d["rep"][k] if chess else None)
                model_single(m, t, lo, hi, True, chess)
            got, want = tj.take(), m.take()
            assert got.rows.tolist() == [list(r) for r in want["rows"]]
            assert got.labels.tolist() == want["labels"] and got.moves.tolist() == want["moves"]
            assert [tuple(g) for g in got.games.tolist()] == want["games"] and len(want["games"]) > n
            assert got.pi_off.tolist() == want["pi_off"]
            assert [v & 0xFFFFFFFF for v in got.pi.tolist()] == want["pi"]
            dense = got.policy_targets(width).cpu().numpy()
            assert np.array_equal(dense, _dense(want, width))
            assert int(tj.ctl[_native.ZC_TRAJ_FINISHED]) == m.finished
