"""The walk's fp32 UCT decision (tests/uct_fast_ref.py: candidate set, identical-pair rule, fp64
fallback) never disagrees with the float64 first-argmax, neither with numpy's correctly rounded
fp32 scores nor with scores pushed as far from the float64 ones as 1-ulp hardware may go."""
import numpy as np
import pytest

import uct_fast_ref as ur

N_MAX = 65534  # the engine's largest max_sims + 1
CS = [0.0, 1.4, 50.0]


def check(nodes, c, rng=None):
    valid, na, wa, big_n = nodes
    want = ur.reference_argmax(valid, na, wa, big_n, c)
    dlt = ur.delta(c, N_MAX)
    slot, how = ur.select(valid, na, wa, big_n, c, dlt)
    assert np.array_equal(slot, want)
    if rng is not None and np.isfinite(c):
        # any scores within the first-order bound of the float64 ones (then rounded to fp32)
        lg = np.log(np.asarray(big_n, np.float64))[:, None]
        nad = np.where(valid, na, 1).astype(np.float64)
        u = c * np.sqrt(lg / nad) + np.where(valid, wa, 0) / nad
        e = np.array([ur.first_order_error(c, int(n)) for n in np.unique(big_n)])
        e = e[np.searchsorted(np.unique(big_n), big_n)][:, None]
        for sign in (rng.choice([-1.0, 1.0], u.shape), rng.uniform(-1, 1, u.shape)):
            slot2, _ = ur.select(valid, na, wa, big_n, c, dlt, scores=(u + sign * e).astype(np.float32))
            assert np.array_equal(slot2, want)
    return how


@pytest.mark.parametrize("c", CS + [float("inf")])
@pytest.mark.parametrize("big_n", [2, 800, 65533])
def test_exact_ties_take_the_first_slot_without_fallback(big_n, c):
    na0 = max(1, (big_n - 1) // 8)
    for wa0 in sorted({-na0, 0, na0 // 3, na0}):
        how = check(ur.tie_patterns(big_n, na0, wa0), c)
        if np.isfinite(c):
            assert (how <= 1).all()  # one candidate or the identical-pair rule, never fp64
        assert (how[:255][np.array([bin(m).count("1") > 1 for m in range(1, 256)])] == 1).all()


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("big_n", [2, 800, 65533])
def test_pairs_one_unit_apart(big_n, c):
    rng = np.random.default_rng(big_n)
    check(ur.unit_neighbours(big_n, rng, 4000), c, rng)


@pytest.mark.parametrize("c", CS + [float("inf"), -1.4])
def test_mixed_valid_and_invalid_slots(c):
    rng = np.random.default_rng(5)
    for big_n in (2, 9, 800, 65533):
        valid, na, wa, n = ur.random_nodes(big_n, rng, 2000)
        valid[:50] = False  # nodes without a child
        slot = check((valid, na, wa, n), c, rng)
        del slot


def test_random_nodes_and_fallback_rate():
    rng = np.random.default_rng(11)
    parts = [ur.random_nodes(big_n, rng, 25000) for big_n in (50, 800, 2100, 65533)]
    nodes = tuple(np.concatenate([p[i] for p in parts]) for i in range(4))
    assert len(nodes[3]) == 100000
    for c in (1.4, 50.0):
        how = check(nodes, c, rng if c == 1.4 else None)
        contested = int((how >= 1).sum())
        print(f"c = {c}: {contested} of 100000 nodes contested, {int((how == 2).sum())} fell back "
              f"({100.0 * (how == 2).mean():.2f} % of all nodes)")
    inf_how = check(nodes, float("inf"))
    kids = nodes[0].sum(1)
    pairs_equal = np.array([len({(a, w) for a, w, v in zip(*r) if v}) <= 1 for r in
                            zip(nodes[1][:2000], nodes[2][:2000], nodes[0][:2000])])
    assert (inf_how[:2000][(kids[:2000] > 1) & ~pairs_equal] == 2).all()  # c = inf: fp64 wherever contested
