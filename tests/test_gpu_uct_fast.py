"""The walk's fp32 UCT decision on the device (zc_debug_c4_uct_select runs uct_select8, the
code the rollout search's walk runs) against the float64 first-argmax: an exhaustive grid of
two-child nodes, random seven-child nodes at large N and extreme c, ties and c = inf."""
import numpy as np
import pytest

import uct_fast_ref as ur

pytestmark = pytest.mark.gpu

MAX_SIMS = 65533


@pytest.fixture(scope="module")
def eng():
    from zeroclone_amd._native import NativeEngine
    e = NativeEngine(max_games=1, max_sims=MAX_SIMS, max_batch=32)
    yield e
    e.close()


def two_child_grid(total):
    """Every (Na1, Wa1, Na2, Wa2) with Na1 + Na2 = total, as [n, 2] arrays."""
    na, wa = [], []
    for a in range(1, total):
        b = total - a
        w1, w2 = np.meshgrid(np.arange(-a, a + 1), np.arange(-b, b + 1), indexing="ij")
        na.append(np.stack([np.full(w1.size, a), np.full(w1.size, b)], 1))
        wa.append(np.stack([w1.ravel(), w2.ravel()], 1))
    return np.concatenate(na), np.concatenate(wa)


def test_exhaustive_two_child_nodes(eng):
    """N = 2..64, the children's visits summing to N - 1 (an inner node) or N (the root), every
    pair of values; the two children in changing slots among empty ones."""
    c = 1.4
    fell = nodes = 0
    for lo in range(2, 65, 8):
        na2, wa2, big, s1, s2 = [], [], [], [], []
        for N in range(lo, min(lo + 8, 65)):
            for total in (N - 1, N):
                if total < 2:
                    continue
                a, w = two_child_grid(total)
                na2.append(a)
                wa2.append(w)
                big.append(np.full(len(a), N))
                s1.append(np.full(len(a), N % 3))
                s2.append(np.full(len(a), 3 + (N + total) % 5))
        na2, wa2, big = np.concatenate(na2), np.concatenate(wa2), np.concatenate(big)
        slots = np.stack([np.concatenate(s1), np.concatenate(s2)], 1)
        n = len(big)
        want = slots[np.arange(n), ur.reference_argmax(np.ones((n, 2), bool), na2, wa2, big, c)]
        valid = np.zeros((n, 8), bool)
        na = np.zeros((n, 8), np.int32)
        wa = np.zeros((n, 8), np.int32)
        for j in range(2):
            valid[np.arange(n), slots[:, j]] = True
            na[np.arange(n), slots[:, j]] = na2[:, j]
            wa[np.arange(n), slots[:, j]] = wa2[:, j]
        slot, how = eng.debug_c4_uct_select(ur.child_words(valid), na, wa, big, c)
        assert np.array_equal(slot, want)
        same = (na2[:, 0] == na2[:, 1]) & (wa2[:, 0] == wa2[:, 1])
        assert (how[same] == 1).all()  # a tie of equal pairs: the first slot, no fp64
        fell += int((how == 2).sum())
        nodes += n
    print(f"two-child grid: {nodes} nodes, {fell} decided in fp64 ({100.0 * fell / nodes:.3f} %)")


@pytest.mark.parametrize("c", [0.0, 1.4, 50.0, float("inf")])
@pytest.mark.parametrize("big_n", [800, 2100, 65533])
def test_random_seven_child_nodes(eng, big_n, c):
    rng = np.random.default_rng(big_n)
    valid, na, wa, big = ur.random_nodes(big_n, rng, 20000, kids=7)
    # a share of exact ties: the best pair copied over one to six other children
    for i in range(0, 4000):
        ks = np.nonzero(valid[i])[0]
        src = ks[rng.integers(len(ks))]
        dst = rng.choice(ks, rng.integers(1, 7), replace=False)
        na[i, dst], wa[i, dst] = na[i, src], wa[i, src]
    tied_all = np.zeros(len(big), bool)
    tied_all[:500] = True
    na[:500], wa[:500] = na[:500, :1], wa[:500, :1]
    slot, how = eng.debug_c4_uct_select(ur.child_words(valid), na, wa, big, c)
    assert np.array_equal(slot, ur.reference_argmax(valid, na, wa, big, c))
    assert (how[tied_all] == 1).all()  # identical pairs do not fall back, whatever c is
    pairs = np.where(valid, na.astype(np.int64) * (1 << 20) + wa, -1)
    contested = np.array([len(set(r[r >= 0].tolist())) > 1 for r in pairs])
    if np.isinf(c):
        assert (how[contested] == 2).all()  # no margin holds: fp64 wherever the pairs differ
    else:
        print(f"N = {big_n}, c = {c}: {int((how == 2).sum())} of {len(big)} nodes decided in fp64")
        # At the searches' c = 1.4 the margin is 8e-6 while these nodes' best two children lie
        # ~5e-3 apart: a fallback needs a coincidence (well under 1 % of the nodes).  No rate is
        # held elsewhere: with c = 0 the score is Wa / Na alone and different pairs with one
        # quotient (0 / 98 and 0 / 101) are real ties that only fp64 may break, and at c = 50 the
        # margin (2.4e-4) reaches the near-equal children's spacing at N = 65533.
        if c == 1.4:
            assert (how == 2).mean() < 0.05


def test_unvisited_slot_and_childless_node(eng):
    valid = np.zeros((3, 8), bool)
    valid[0, [1, 4, 6]] = True
    valid[1, [2, 3]] = True
    na = np.zeros((3, 8), np.int32)
    wa = np.zeros((3, 8), np.int32)
    na[0, [1, 4, 6]] = [5, 0, 0]  # slot 4: the first unvisited child
    na[1, [2, 3]] = [3, 4]
    wa[1, [2, 3]] = [-3, 4]
    slot, how = eng.debug_c4_uct_select(ur.child_words(valid), na, wa, [9, 8, 8], 1.4)
    assert slot.tolist() == [4, 3, -1] and how.tolist() == [0, 0, 0]
