"""Edge cases of the Connect4 rollout kernel (c4_rollouts), against the oracle on one MT stream.

eng.c4_rollouts rolls a list of leaves out in order on one game's stream, 64 leaves to a group
(each leaf's value and plies are kept in its lane of the group and stored after it), so the
lists here are 1, 63, 64, 65 and 129 leaves long, made of the positions where the block logic
has an edge: a leaf already won, a full board, one / two / three empty cells (the board-full
exit; every such ply is a fill, the first one included, and the last allowed ply is one), a
single legal column, and ordinary mid-game boards that run into fills.  A prefix rollout on the
same stream, with a seed searched on the CPU, puts the list's first view at window offset 0, 1
or 63; the oracle's `drawn` count says which offsets and window crossings a list really hits.
Values and the stream position must equal the oracle's.

The search-level case runs the fused kernel (the stream kept in LDS, whose two windows trade
places at every advance, so both phases occur many times in each search) at batch sizes 1, 31
and 33 against the oracle, and pins the rollout counters.
"""
import ctypes
import random

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SEED0 = 624  # a freshly seeded stream stands at word 624 of the generator: window offset 624 % 64


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=16, max_sims=64, max_batch=64)
    yield e
    e.close()


def states(boards):
    from zeroclone_amd._native import C4_STATE_DTYPE, c4_from_rows
    out = np.zeros(len(boards), C4_STATE_DTYPE)
    for i, (b, t) in enumerate(boards):
        out[i] = c4_from_rows(b, t)
    return out


def full_board():
    """A full board without four in a row: columns alternate, rows are XXOOXXO or its inverse."""
    rows = ["".join("XO"[(int(c in (2, 3, 6))) ^ (r & 1)] for c in range(7)) for r in range(6)]
    b = "".join(rows)
    assert oracle.check_draw(b) and not oracle.check_win(b, 0) and not oracle.check_win(b, 1)
    return b


def without_top(b, cols):
    """b with the top cell of each of `cols` empty (those columns stand at height 5)."""
    b = list(b)
    for c in cols:
        b[c] = "."
    return "".join(b)


def special_positions():
    full = full_board()
    won, t = "." * 42, 0
    for col in (0, 1, 0, 1, 0, 2, 0):  # X: four in column 0
        won, t = oracle.play(won, t, col)
    assert oracle.check_win(won, t)
    one_col = list(full)  # a single legal column with three empty cells: n = 1, its third ply fills it
    for r in range(3):
        one_col[7 * r + 3] = "."
    out = [(won, t), (full, 0), (full, 1),
           (without_top(full, [4]), 0), (without_top(full, [0]), 1),           # one empty cell
           (without_top(full, [1, 5]), 0), (without_top(full, [2, 3]), 1),     # two: both plies fill
           (without_top(full, [0, 3, 6]), 1), (without_top(full, [1, 2, 4]), 0),  # three
           ("".join(one_col), 1), ("".join(one_col), 0)]
    # mid-game boards that lean on a few columns: fills early in the rollout, one to seven moves
    rng = random.Random(99)
    while len(out) < 40:
        b, t = "." * 42, 0
        lean = rng.sample(range(7), rng.randint(1, 3))
        for _ in range(rng.randint(0, 36)):
            legal = [c for c in range(7) if b[c] == "."]
            pref = [c for c in legal if c in lean]
            b, t = oracle.play(b, t, rng.choice(pref if pref and rng.random() < 0.8 else legal))
            if oracle.check_win(b, t):
                break
        out.append((b, t))
    return out


@pytest.fixture(scope="module")
def pool():
    return special_positions()


def prefix(pool):
    return [pool[-1], pool[-2], pool[-3]]


def oracle_rollouts(mt, boards):
    """Values, and the stream position (words since seeding) before each leaf and after the last."""
    vals, pos = [], []
    for b, t in boards:
        pos.append(mt.drawn)
        vals.append(oracle.lib().zco_rollout(b.encode(), t, ctypes.byref(mt.s)))
    pos.append(mt.drawn)
    return vals, pos


def seed_for_offset(pool, off, salt):
    """A seed after whose prefix rollouts the stream stands at window offset `off`."""
    for seed in range(1000 * salt, 1000 * salt + 4000):
        mt = oracle.MT(seed)
        _, pos = oracle_rollouts(mt, prefix(pool))
        if (SEED0 + pos[-1]) % 64 == off:
            return seed
    raise AssertionError(f"no seed found for offset {off}")


@pytest.mark.parametrize("off", [0, 1, 63])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_rollout_lists_match_oracle(eng, pool, count, off):
    seed = seed_for_offset(pool, off, count)
    # the special positions at the list's start, around the 64-leaf group boundary and at its end
    boards = [pool[(i + count + off) % len(pool)] for i in range(count)]
    for k, i in enumerate(j for j in (0, 62, 63, 64, 65, 127, 128, count - 1) if j < count):
        boards[i] = pool[(k + off + count) % 11]
    mt = oracle.MT(seed)
    pvals, ppos = oracle_rollouts(mt, prefix(pool))
    vals, pos = oracle_rollouts(mt, boards)
    assert (SEED0 + pos[0]) % 64 == off  # the first view of the list starts at this window offset
    if count >= 63:
        # rollouts that start in one 64-word window and end in another: in windows of both parities
        crossed = {((SEED0 + pos[i + 1]) // 64) % 2 for i in range(count)
                   if (SEED0 + pos[i]) // 64 != (SEED0 + pos[i + 1]) // 64}
        assert crossed == {0, 1}
        # and, over the list, views that start at every kind of offset the kernel distinguishes
        starts = {(SEED0 + p) % 64 for p in pos[:-1]}
        assert len(starts) > 16
    eng.seed(2, [seed])
    got, words = eng.c4_rollouts(states(prefix(pool)), game=2)
    assert [int(x) for x in got] == pvals and words == ppos[-1]
    got, words = eng.c4_rollouts(states(boards), game=2)
    assert [int(x) for x in got] == vals
    assert words == pos[-1] - pos[0]


def test_special_positions_one_by_one(eng, pool):
    """Each special position alone (a list of one leaf, a fresh stream each): the already-won
    leaf, the full board and the boards with one to three empty cells consume what the oracle
    consumes (nothing, for the first two) and give its value."""
    for k, (b, t) in enumerate(pool[:11]):
        for seed in (5 + k, 1005 + k):
            v, drawn = oracle.rollout(b, t, seed)
            eng.seed(1, [seed])
            got, words = eng.c4_rollouts(states([(b, t)]), game=1)
            assert (int(got[0]), words) == (v, drawn), (k, seed)
    assert oracle.rollout(*pool[0], 1) == (-1, 0) and oracle.rollout(*pool[1], 1) == (0, 0)


# (rollout_plies, rollout_blocks) of the 8 games below, per batch size: the values of the library
# before the rollout's leaf and block loops were reshaped, recorded from a run of that library
# on the same input, next to the new one (the oracle does not count plies or blocks, so they
# are not from a CPU replay)
COUNTERS = {
    1: ([199, 396, 112, 74, 326, 271, 768, 898], [42, 71, 36, 30, 60, 49, 80, 90]),
    31: ([382, 325, 225, 99, 288, 530, 708, 889], [72, 63, 63, 44, 59, 81, 89, 96]),
    33: ([350, 348, 239, 104, 291, 474, 708, 888], [69, 62, 59, 44, 57, 78, 88, 89]),
}


@pytest.mark.parametrize("bs", [1, 31, 33])
def test_search_counters_and_oracle(eng, bs):
    n, sims = 8, 64
    rng = random.Random(4242)
    boards = []
    while len(boards) < n:
        b, t = "." * 42, 0
        lean = rng.sample(range(7), rng.randint(1, 3))
        ok = True
        for _ in range(rng.randint(6, 38)):
            legal = [c for c in range(7) if b[c] == "."]
            pref = [c for c in legal if c in lean]
            b, t = oracle.play(b, t, rng.choice(pref if pref and rng.random() < 0.7 else legal))
            if oracle.check_win(b, t):
                ok = False
                break
        if ok and not oracle.check_draw(b):
            boards.append((b, t))
    seeds = [104729 * g + 7 for g in range(n)]
    eng.seed(0, seeds)
    mv, na, stats = eng.c4_search(states(boards), sims, 1.4, bs)
    omv, ona, ocons = oracle.get_move_batch([b for b, _ in boards], [t for _, t in boards], seeds, sims, 1.4, bs)
    assert np.array_equal(mv, omv)
    assert np.array_equal(na, ona)
    assert np.array_equal(stats["rng_words"], ocons.astype(np.int64))
    print("rollout counters", bs, [int(x) for x in stats["rollout_plies"]], [int(x) for x in stats["rollout_blocks"]])
    assert ([int(x) for x in stats["rollout_plies"]], [int(x) for x in stats["rollout_blocks"]]) == COUNTERS[bs]
