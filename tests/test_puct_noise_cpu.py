"""CPU checks of the PUCT noise / temperature specification (tests/puct_noise_ref.py): its
draws have the distributions it claims (Kolmogorov-Smirnov against the analytic CDFs, 1 %
critical value 1.63 / sqrt(n)), its counter words do not alias (|correlation| < 4 / sqrt(n)),
its sampler draws in proportion to N^(1/T) (chi-square, 0.1 % critical value), and the same
assertions reject four deliberately wrong specifications.  Fixed seeds: deterministic."""
import numpy as np
import pytest

import puct_noise_ref as ref

try:
    from scipy.special import betainc, gammainc
    from scipy.stats import chi2 as _chi2

    def chi2_critical(df):
        return float(_chi2.ppf(0.999, df))
except ImportError:   # pragma: no cover
    import torch

    def gammainc(a, x):
        return torch.special.gammainc(torch.as_tensor(float(a), dtype=torch.float64), torch.as_tensor(x)).numpy()

    betainc = None

    def chi2_critical(df):
        # Wilson-Hilferty, z(0.999) = 3.0902
        return df * (1 - 2 / (9 * df) + 3.0902 * np.sqrt(2 / (9 * df))) ** 3

N = 40000
SEED = 0x123456789ABCDEF
ALPHAS = [0.03, 0.3, 1.0, 2.5]


def ks(x, cdf):
    x = np.sort(np.asarray(x, dtype=np.float64).ravel())
    n = x.size
    F = cdf(x)
    return max((np.arange(1, n + 1) / n - F).max(), (F - np.arange(n) / n).max())


def ks_ok(x, cdf):
    return ks(x, cdf) < 1.63 / np.sqrt(np.asarray(x).size)


def gamma_sample(alpha, **kw):
    """N draws: 200 games x 200 moves of search 5."""
    return ref.gamma_draw(alpha, SEED, np.arange(200)[:, None], np.arange(200)[None, :], 5, **kw)[0]


def beta_sample(alpha, k, **kw):
    """Move 0's share of the noise in N games of k moves."""
    g = ref.gamma_draw(alpha, SEED + 1, np.arange(N)[:, None], np.arange(k)[None, :], 2, **kw)[0]
    return g[:, 0] / g.sum(axis=1)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_draws_are_gamma(alpha):
    a = float(np.float32(alpha))
    g = gamma_sample(alpha)
    assert g.size == N and (g > 0).all()
    assert ks_ok(g, lambda x: gammainc(a, x)), ks(g, lambda x: gammainc(a, x))
    # the float32 run is the same generator but for rounding (and underflow: at alpha = 0.03
    # U^(1/alpha) leaves float32's range for about one draw in twenty) and the rare draw whose
    # accept flips
    g32 = gamma_sample(alpha, dtype=np.float32)
    assert g32.dtype == np.float32
    big = g > 1e-30
    assert (np.abs(g32[big] / g[big] - 1) > 1e-3).mean() < 1e-3


@pytest.mark.skipif(betainc is None, reason="no regularised incomplete beta function")
@pytest.mark.parametrize("k", [7, 20])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_normalised_draws_have_beta_marginals(alpha, k):
    a = float(np.float32(alpha))
    x = beta_sample(alpha, k)
    assert ks_ok(x, lambda t: betainc(a, (k - 1) * a, t)), ks(x, lambda t: betainc(a, (k - 1) * a, t))


def corr(x, y):
    return abs(float(np.corrcoef(np.ravel(x), np.ravel(y))[0, 1]))


def test_counter_words_do_not_alias():
    n = 201
    gi, ji = np.arange(n)[:, None], np.arange(n)[None, :]
    off = ~np.eye(n, dtype=bool)   # (g, g) is one and the same draw
    lim = 4 / np.sqrt(off.sum())
    a = ref.gamma_draw(0.3, SEED, gi, ji, 3)[0]
    assert corr(a[off], a.T[off]) < lim                                         # (game, j) / (j, game)
    assert corr(a[off], ref.gamma_draw(0.3, SEED, gi, ji, 4)[0][off]) < lim      # sno / sno + 1
    assert corr(a[off], ref.gamma_draw(0.3, SEED + 1, gi, ji, 3)[0][off]) < lim  # seed / seed + 1
    # a noise draw and the temperature word of the same game (over games and search numbers)
    g, s = np.arange(200)[:, None], np.arange(200)[None, :]
    assert corr(ref.gamma_draw(0.3, SEED, g, 0, s)[0], ref.sample_u(SEED, g, s)) < 4 / np.sqrt(N)
    assert corr(ref.sample_u(SEED, g, s), ref.sample_u(SEED, g, s + 1)) < 4 / np.sqrt(N)
    assert corr(ref.sample_u(SEED, g, s), ref.sample_u(SEED + 1, g, s)) < 4 / np.sqrt(N)
    # aliased words would show as correlation 1
    assert corr(a[off], ref.gamma_draw(0.3, SEED, gi, ji, 3)[0][off]) > 0.999


COUNTS = [np.array([10, 0, 3, 25, 0, 7, 1]),
          np.array([5, 1, 12, 3, 9, 2, 7, 4, 11, 6, 8, 10, 1, 3, 2, 12, 6, 5, 9, 4]),
          1 + (np.arange(218) * 7 + np.arange(218) // 12) % 12]
PAIRS = 200000


def chi2_ok(idx, weights):
    """Frequencies of idx against weights / sum(weights); a move of weight 0 never occurs."""
    cnt = np.bincount(idx, minlength=weights.size)
    if (cnt[weights == 0] != 0).any():
        return False
    p = weights[weights > 0] / weights.sum()
    exp = p * idx.size
    stat = ((cnt[weights > 0] - exp) ** 2 / exp).sum()
    return stat < chi2_critical(p.size - 1)


def sample(na, T):
    g, s = np.arange(400)[:, None], np.arange(PAIRS // 400)[None, :]
    return ref.sample_index(na, T, SEED, g, s)[0].ravel()


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("c", range(len(COUNTS)))
def test_sample_index_draws_in_proportion_to_the_tempered_counts(c, T):
    na = COUNTS[c]
    idx = sample(na, T)
    assert idx.size == PAIRS
    assert (na[idx] > 0).all()
    assert chi2_ok(idx, na.astype(np.float64) ** (1 / T))


def test_low_temperature_tends_to_the_argmax():
    """T = 0.01: unscaled, 2000^100 overflows a double; the scaled weights give the argmax."""
    na = np.array([3, 700, 2000, 1300, 0, 12, 1])   # (1300 / 2000)^100 = 2e-19 of the top weight
    idx, _ = ref.sample_index(na, 0.01, SEED, np.arange(4096), 7)
    assert (idx == 2).all()
    assert np.isfinite(ref.sample_weights(na, 0.01)).all() and ref.sample_weights(na, 0.01).sum() > 0
    tie = np.array([5, 1500, 0, 1500])
    idx, _ = ref.sample_index(tie, 0.01, SEED, np.arange(4096), 7)
    assert set(idx.tolist()) == {1, 3}


def test_the_assertions_reject_wrong_specifications():
    """Mutation checks: a generator with alpha scaled by 1.15, one without the alpha < 1 boost,
    a sampler with T in place of 1/T, and one that walks the CDF in reverse order."""
    for alpha in ALPHAS:
        a = float(np.float32(alpha))
        assert not ks_ok(gamma_sample(alpha * 1.15), lambda x: gammainc(a, x)), alpha
        if betainc is not None:
            for k in (7, 20):
                assert not ks_ok(beta_sample(alpha * 1.15, k), lambda t: betainc(a, (k - 1) * a, t)), (alpha, k)
    for alpha in (0.03, 0.3):
        a = float(np.float32(alpha))
        assert not ks_ok(gamma_sample(alpha, boost=False), lambda x: gammainc(a, x)), alpha
        if betainc is not None:
            assert not ks_ok(beta_sample(alpha, 7, boost=False), lambda t: betainc(a, 6 * a, t)), alpha
    for na in COUNTS:
        w = na.astype(np.float64)
        for T in (0.5, 2.0):
            assert not chi2_ok(sample(na, 1 / T), w ** (1 / T))      # T for 1/T
        for T in (0.5, 1.0, 2.0):
            assert not chi2_ok(sample(na[::-1], T), w ** (1 / T))    # reverse walk, forward report
