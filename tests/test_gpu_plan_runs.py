"""The planned flush's chain, built by runs (c4_search.hip select_flush_plan, stage 1a), against
the oracle: move, root visits and MT words, from roots whose chains have several runs in one
flush (columns at heights 4 and 5: runs of length 1 and 2, two fills in one chain), reach the
terminal chain node (one or two legal columns) or have one long run (the empty board), at batch
sizes with a short last flush.

That the roots do what they are chosen for is checked on the CPU: the oracle's search with its
rollouts passed in as the value function (same stream, same order: the same search) shows every
flush's leaves, from which the chain is read off — its nodes are the leaves that the next
depth's leaves extend, a run ends where the legal set changes, and leaves repeated at a flush's
end are the terminal node's."""
import ctypes
import random

import numpy as np
import pytest

import oracle
from c4_positions import EMPTY, states

pytestmark = pytest.mark.gpu

C = 1.4


def legal(b):
    return tuple(col for col in range(7) if b[col] == ".")


def heights(b):
    return [sum(b[r * 7 + col] != "." for r in range(6)) for col in range(7)]


def random_root(rng, want):
    """A position without a win, reached by random play, that satisfies want(board)."""
    while True:
        b, t = EMPTY, 0
        lean = rng.sample(range(7), rng.randint(2, 5))
        for _ in range(41):
            cols = legal(b)
            pref = [col for col in cols if col in lean]
            b, t = oracle.play(b, t, rng.choice(pref if pref and rng.random() < 0.8 else cols))
            if oracle.check_win(b, t) or oracle.check_draw(b):
                break
            if want(b):
                return b, t


def tall_columns(b):  # at least two open columns of height 4 or 5, one of each
    h = heights(b)
    return 4 in h and 5 in h and len(legal(b)) >= 4


def roots_tall(n, seed):
    rng = random.Random(seed)
    return [random_root(rng, tall_columns) for _ in range(n)]


def roots_narrow(n, seed):  # the same with two or three open columns: short batches get past a fill
    rng = random.Random(seed)
    return [random_root(rng, lambda b: {4, 5} <= set(heights(b)) and len(legal(b)) in (2, 3)) for _ in range(n)]


def roots_few(n, seed):
    rng = random.Random(seed)
    return [random_root(rng, lambda b, k=1 + i % 2: len(legal(b)) == k) for i in range(n)]


def roots_empty(n, seed):
    return [(EMPTY, 0)] * n


def chain_of_flush(boards):
    """(runs among the chain nodes below X0 that take draws, terminal node reached)."""
    terminal = len(boards) >= 2 and boards[-1] == boards[-2] and any(b != boards[-1] for b in boards)
    while len(boards) >= 2 and boards[-1] == boards[-2]:
        boards = boards[:-1]
    groups = []
    for b in boards:
        if groups and b.count(".") == groups[-1][0].count("."):
            groups[-1].append(b)
        else:
            groups.append([b])
    chain = []
    for k in range(len(groups) - 1):
        nxt = groups[k + 1][0]
        cand = [b for b in groups[k] if all(x == y or x == "." for x, y in zip(b, nxt))]
        assert len(cand) == 1
        chain.append(cand[0])
    sets = [legal(b) for b in chain]
    runs = (1 + sum(a != b for a, b in zip(sets, sets[1:]))) if sets else 0
    return runs, terminal


def oracle_search(boards, seeds, sims, bs):
    """Per game (move, visits by column, words) and the most runs / whether T occurred."""
    mv, na, words = oracle.get_move_batch([b for b, _ in boards], [t for _, t in boards], seeds, sims, C, bs)
    most_runs, terminals = 0, 0
    for g, (b, t) in enumerate(boards):
        mt = oracle.MT(seeds[g])

        def rollouts(leaves, turns, mt=mt):
            nonlocal most_runs, terminals
            runs, term = chain_of_flush(list(leaves))
            most_runs = max(most_runs, runs)
            terminals += term
            return [oracle.lib().zco_rollout(x.encode(), y, ctypes.byref(mt.s)) for x, y in zip(leaves, turns)]

        col, vis, order = oracle.get_move_valued(b, t, mt, sims, C, bs, rollouts)
        by_col = np.zeros(7, np.int32)
        by_col[order] = vis
        # the instrumented search is the search
        assert col == mv[g] and np.array_equal(by_col, na[g]) and mt.drawn == words[g]
    return mv, na, words, most_runs, terminals


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=64, max_sims=200, max_batch=63)
    yield e
    e.close()


# (roots, games, sims, batch, the runs some flush's chain must have): two runs = a fill below X0
# after which the chain goes on, three = two fills in one chain.  A batch of 5 or 8 only gets
# that far where few columns are open; the empty board's one long run only ends in a batch of 63.
CASES = [(roots_tall, 32, 150, 32, 3), (roots_tall, 16, 200, 63, 3), (roots_tall, 32, 150, 8, 2),
         (roots_narrow, 16, 97, 5, 2), (roots_narrow, 32, 150, 8, 3),
         (roots_few, 32, 150, 32, 2), (roots_few, 32, 150, 8, 2), (roots_few, 16, 97, 5, 2),
         (roots_few, 16, 200, 63, 2), (roots_empty, 16, 200, 63, 2)]


@pytest.mark.parametrize("make,n,sims,bs,min_runs", CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_search_matches_oracle_on_chains_with_several_runs(eng, make, n, sims, bs, min_runs):
    assert sims % bs  # a short last flush
    boards = make(n, 100 + bs)
    seeds = [1000 * bs + 13 * g + 1 for g in range(n)]
    mv, na, words, most_runs, terminals = oracle_search(boards, seeds, sims, bs)
    assert most_runs >= min_runs
    if make is roots_few:
        assert terminals > 0  # the terminal chain node T
    eng.seed(0, seeds)
    gmv, gna, st = eng.c4_search(states(boards), sims, C, bs)
    assert (st["status"] == 0).all()
    assert np.array_equal(gmv, mv)
    assert np.array_equal(gna, na)
    assert np.array_equal(st["rng_words"], words.astype(np.int64))
