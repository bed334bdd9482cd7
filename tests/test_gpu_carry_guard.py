"""The edges of the carry protocol (zc_c4_selfplay_carry_async), by hand through the C ABI:
16 games x 64 simulations, batch 8, at most 4 moves per game and launch; every carry launch gets
a budget of one move per game, so moves are suspended at a flush boundary and carried over.

While moves are carried over, the engine refuses (ZC_EINVAL -> ValueError), on the host and
before anything is enqueued,
  * a self-play launch (free, pooled or carry) that would resume them under another sims,
    batch_size, c, root buffer or row shift, and a change of the rollout mode: the outputs keep
    their fill pattern, and the matching launch that follows still finishes every game's
    free-run moves (a twin engine's one free run);
  * every entry point that would search or reseed the carried games — accepted on games outside
    the carried range;
and the guarded range [carry_lo, carry_hi) grows by carry launches, is lifted only by a launch or
a discard that covers all of it, and a discard leaves searches that start afresh.  A carried game
whose root row is overwritten with a bad state loses its carried move: flagged, then searchable
and playable afresh, equal to a fresh twin."""
import numpy as np
import pytest
import torch

from c4_raw_pool import BAD_STATE, LEAVES, STATUS, RawPool, c4_rows, raw_state

pytestmark = pytest.mark.gpu

G, SIMS, BS, CAP, C = 16, 64, 8, 4, 1.4
MAX_SIMS, MAX_BATCH = 128, 16           # room for the mismatched sims and batch_size to be legal ones
SEEDS = [1000 + 7 * g for g in range(G)]
TOTAL = 3 * CAP + 1                      # the most moves a game finishes in any test below
P = dict(sims=SIMS, bs=BS, c=C)


def pool():
    return RawPool(G, MAX_SIMS, MAX_BATCH, SEEDS, TOTAL)


@pytest.fixture(scope="module")
def free_run():
    """Each game's first TOTAL moves of an uninterrupted run: (result, move, state) rows."""
    p = pool()
    rows = p.launch("free", TOTAL, **P)
    assert bool((p.stats[:, STATUS] == 0).all()) and all(len(r) == TOTAL for r in rows)
    p.close()
    return rows


def carry_launch(p, first=0, n=G):
    """A carry launch over [first, first + n) with one ticket per game; asserts that moves were
    suspended (tickets drawn below the budget = moves started; fewer finished)."""
    rows = p.launch("carry", CAP, first=first, n=n, budget=n, **P)
    assert bool((p.stats[:n, STATUS] == 0).all())
    in_flight = n - sum(len(r) for r in rows)
    assert in_flight > 0
    assert int(p.stats[:n, LEAVES].sum()) < n * SIMS       # ... their simulations only partly run
    return rows


def guarded(p, g):
    """Does the engine hold game g in its carried range?  set_rng_state(get_rng_state) is the
    probe: refused under the guard, and the same MT19937 stream when accepted."""
    mt, idx = p.eng.get_rng_state(g)
    try:
        p.eng.set_rng_state(g, mt, idx)
    except ValueError as e:
        assert "carried over" in str(e)
        return True
    return False


def extend(seq, rows, first=0):
    for i, r in enumerate(rows):
        seq[first + i] += r


def assert_free_run(seq, free_run, games=range(G)):
    for g in games:
        assert len(seq[g]) <= TOTAL
        assert seq[g] == free_run[g][:len(seq[g])], g


MISMATCH = {
    "sims": (dict(sims=32), r"sims 32 differs from the 64"),
    "batch_size": (dict(bs=16), r"batch_size 16 differs from the 8"),
    "c": (dict(c=1.5), r"c 1\.5 differs from the 1\.3999"),
    "d_roots": (dict(other_buffer=True), r"d_roots"),
    "first_game": (dict(first=1, n=G - 1, same_pointer=True), r"first_game"),
    "rollout mode": (None, r"rollout mode"),
}


@pytest.mark.parametrize("form", ["free", "pooled", "carry"])
@pytest.mark.parametrize("what", list(MISMATCH))
def test_resuming_launch_with_another_parameter_is_refused(free_run, what, form):
    p = pool()
    seq = [[] for _ in range(G)]
    extend(seq, carry_launch(p))
    roots0 = p.roots.clone()
    change, msg = MISMATCH[what]
    if change is None:       # the mode cannot change under carried moves, so no launch can bring another
        p.fill()
        with pytest.raises(ValueError, match=msg):
            p.eng.c4_rollout_mode("philox", 7)
    else:
        kw = dict(P)
        kw.update({k: v for k, v in change.items() if k in ("sims", "bs", "c", "first", "n")})
        if change.get("other_buffer"):
            other = p.roots.clone()
            kw["roots_ptr"] = other.data_ptr()
        if change.get("same_pointer"):   # rows shifted by one game under the same pointer
            kw["roots_ptr"] = p.roots.data_ptr()
        n = kw.get("n", G)
        with pytest.raises(ValueError, match=msg):
            p.launch(form, CAP, budget=n if form == "carry" else None, **kw)
    # refused on the host: nothing was enqueued, so nothing wrote (ticket words included)
    assert p.untouched()
    assert torch.equal(p.roots, roots0)
    assert guarded(p, 0) and guarded(p, G - 1)
    # the matching launch resumes the carried moves as if nothing had been tried
    if form == "carry":
        extend(seq, p.launch("carry", CAP, budget=G, **P))
        extend(seq, p.launch("pooled", 1, budget=0, **P))      # the drain
    else:
        extend(seq, p.launch(form, CAP, **P))
    assert bool((p.stats[:, STATUS] == 0).all())
    assert not guarded(p, 0)
    assert min(len(s) for s in seq) >= 1
    assert_free_run(seq, free_run)
    p.close()


def test_a_second_carry_launch_with_other_parameters_is_refused_on_disjoint_games(free_run):
    p = pool()
    seq = [[] for _ in range(G)]
    extend(seq, carry_launch(p, 0, 8))
    with pytest.raises(ValueError, match="sims 32 differs"):      # the engine keeps one record
        p.launch("carry", CAP, first=8, n=8, budget=8, sims=32, bs=BS, c=C)
    assert p.untouched()
    p.launch("free", CAP, first=8, n=8, sims=32, bs=BS, c=C)      # a plain launch beside the range may differ
    assert bool((p.stats[:8, STATUS] == 0).all())
    assert guarded(p, 0)
    extend(seq, p.launch("pooled", 1, first=0, n=8, budget=0, **P))
    assert_free_run(seq, free_run, range(8))
    p.close()


def test_entry_points_refuse_carried_games_and_accept_the_others(free_run):
    p = pool()
    e = p.eng
    seq = [[] for _ in range(G)]
    extend(seq, carry_launch(p, 0, 8))
    empty = np.zeros(4, _dtype())
    d_roots = c4_rows(empty)
    d_move = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_na = torch.zeros((4, 7), dtype=torch.int32, device="cuda")
    d_stats = torch.zeros((4, 8), dtype=torch.int64, device="cuda")
    d_vals = torch.zeros(4 * SIMS, dtype=torch.int8, device="cuda")
    d_words = torch.zeros(4 * (SIMS // BS), dtype=torch.int32, device="cuda")
    calls = {
        "c4_search": lambda f: e.c4_search(empty, SIMS, C, BS, first_game=f),
        "c4_search_games": lambda f: e.c4_search_games([f + 3, f + 1, f, f + 2], empty, SIMS, C, BS),
        "c4_search_async": lambda f: e.c4_search_async(d_roots.data_ptr(), 4, SIMS, C, BS, d_move.data_ptr(),
                                                       d_na.data_ptr(), d_stats.data_ptr(), first_game=f),
        "c4_ext_begin": lambda f: e.c4_ext_begin(f, 4, d_roots.data_ptr(), SIMS, C, BS),
        "c4_rollouts": lambda f: e.c4_rollouts(empty, game=f),
        "seed": lambda f: e.seed(f, [5, 6, 7, 8]),
        "set_rng_state": lambda f: e.set_rng_state(f, *e.get_rng_state(f)),
        "debug_c4_rollout": lambda f: e.debug_c4_rollout(empty, first_game=f),
        "c4_walk_async": lambda f: e.c4_walk_async(f, 4, d_roots.data_ptr(), SIMS, C, BS, 1, d_vals.data_ptr(),
                                                   d_words.data_ptr(), d_move.data_ptr(), d_na.data_ptr(),
                                                   d_stats.data_ptr()),
    }
    for name, call in calls.items():
        for first in (0, 2, 5):            # inside [0, 8), and [5, 9) across its end
            with pytest.raises(ValueError, match="carried over"):
                call(first)
        call(8)                            # outside: accepted
        call(12)
        torch.cuda.synchronize()
    with pytest.raises(ValueError, match="carried over"):          # one carried id in a list of free ones
        e.c4_search_games([9, 12, 7, 15], empty, SIMS, C, BS)
    # the carried games were left alone by all of it: they finish their free-run moves
    extend(seq, p.launch("pooled", 1, first=0, n=8, budget=0, **P))
    assert min(len(s) for s in seq[:8]) >= 1
    assert_free_run(seq, free_run, range(8))
    p.close()


def _dtype():
    from zeroclone_amd._native import C4_STATE_DTYPE
    return C4_STATE_DTYPE


def test_carried_range_grows_and_is_lifted_only_as_a_whole(free_run):
    p = pool()
    seq = [[] for _ in range(G)]
    assert not guarded(p, 0)
    extend(seq, carry_launch(p, 0, 8))
    assert guarded(p, 0) and guarded(p, 7) and not guarded(p, 8)
    extend(seq, carry_launch(p, 8, 8), 8)
    assert all(guarded(p, g) for g in (0, 7, 8, 15))               # [0, 16)
    extend(seq, p.launch("pooled", CAP, first=0, n=8, **P))        # finishes [0, 8)'s moves, lifts nothing
    assert all(guarded(p, g) for g in (0, 7, 8, 15))
    extend(seq, p.launch("free", 1, **P))                          # [0, 16): lifted
    assert not any(guarded(p, g) for g in (0, 7, 8, 15))
    assert_free_run(seq, free_run)
    # discard: part of the range lifts nothing, the whole range everything
    carry_launch(p)
    p.eng.c4_carry_discard(0, 8)
    assert all(guarded(p, g) for g in (0, 7, 8, 15))
    p.eng.c4_carry_discard(0, G)
    torch.cuda.synchronize()
    assert not any(guarded(p, g) for g in (0, 7, 8, 15))
    # every game's next search starts afresh (a resumed one would run sims - done < sims)
    moves = 2
    rows = p.launch("free", moves, **P)
    assert all(len(r) == moves for r in rows)
    assert p.stats[:, LEAVES].tolist() == [SIMS * moves] * G
    assert bool((p.stats[:, STATUS] == 0).all())
    p.close()


def test_bad_root_under_a_carried_move_drops_it(free_run):
    p = pool()
    seq = [[] for _ in range(G)]
    extend(seq, carry_launch(p))
    leaves = p.stats[:, LEAVES].tolist()
    # a game suspended in its first move: some simulations run, no move finished
    suspended = [g for g in range(1, G) if not seq[g] and 0 < leaves[g] < SIMS]
    assert suspended, f"no game was suspended in its first move: leaves {leaves}"
    v = suspended[0]
    before = p.rng(v)
    p.roots[v] = c4_rows(np.array([raw_state(1, 1, 0)], _dtype()))[0]     # overlapping stones
    bad_row = p.roots[v].clone()
    rows = p.launch("pooled", 1, budget=0, **P)                            # the drain
    assert int(p.stats[v, STATUS]) == BAD_STATE and rows[v] == []
    assert p.stats[v].tolist() == [0, 0, 0, 0, 0, BAD_STATE, 0, 0]
    assert torch.equal(p.roots[v], bad_row) and p.rng(v) == before
    extend(seq, rows)
    others = [g for g in range(G) if g != v]
    assert bool((p.stats[others, STATUS] == 0).all()) and min(len(seq[g]) for g in others) >= 1
    assert_free_run(seq, free_run, others)
    assert not guarded(p, v)
    # a valid root again, and the stream of a fresh twin: the game is searched and played afresh
    t = pool()
    p.roots[v] = 0
    for q in (p, t):
        q.eng.seed(v, [4242])
    empty = np.zeros(1, _dtype())
    a = p.eng.c4_search(empty, SIMS, C, BS, first_game=v)
    b = t.eng.c4_search(empty, SIMS, C, BS, first_game=v)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    moves = 3
    ra = p.launch("free", moves, first=v, n=1, **P)
    rb = t.launch("free", moves, first=v, n=1, **P)
    assert ra == rb and len(ra[0]) == moves
    assert p.stats[0].tolist() == t.stats[0].tolist()
    assert int(p.stats[0, LEAVES]) == SIMS * moves and int(p.stats[0, STATUS]) == 0
    assert p.rng(v) == t.rng(v)
    p.close()
    t.close()
