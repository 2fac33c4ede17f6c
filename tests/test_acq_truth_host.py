"""Host (-m "not gpu"): the 50-digit acquisition truth of tests/acq_truth.py against the REFERENCE's own arithmetic — scipy.stats.norm's
cdf / pdf, NumPy, the formulas of oracle.gp_oracle.base_acq and constraint_prob — over z in [-39, 39] and sd over 1e-6 ... 2.

The reference's worst constant c of the error model `c eps (1 + z^2) T + DBL_MIN` measures ~1 (3000 points, seed 0: EI 1.06, POI 1.71,
factor 1.26, gradients EI 1.28 / POI 1.38); asserted <= 4, so a broken helper fails here, without a GPU.  The GPU tests bar the device at
8 c_ref on their own inputs and rely on the cap asserted here: at most 5 % of a uniform z spread has T below DBL_MIN."""
import numpy as np
import pytest

import acq_truth as T

N = 3000
Y_MAX, XI = 1.2345, 0.01


@pytest.fixture(scope="module")
def sample():
    rng = np.random.RandomState(0)
    z = rng.uniform(-39.0, 39.0, N)
    z[:200] = rng.uniform(-1.5, 1.5, 200)                   # the erf / erfc switch at |z| = 1 well covered
    z[200:208] = [-1.0, 1.0, np.nextafter(-1.0, 0), np.nextafter(1.0, 2), np.nextafter(-1.0, -2), np.nextafter(1.0, 0), 0.0, -0.0]
    sd = 10.0 ** rng.uniform(-6.0, np.log10(2.0), N)
    mu = z * sd + Y_MAX + XI
    dmu, dsd = rng.standard_normal((N, 2)), rng.standard_normal((N, 2))
    return mu, sd, dmu, dsd, T.acq_truth(mu, sd, Y_MAX, XI, dmu, dsd)


def test_the_reference_meets_the_truth_at_about_one_ulp(sample):
    mu, sd, dmu, dsd, tr = sample
    assert tr["ok"].all()
    z = tr["z"]
    assert z.min() < -38.5 and z.max() > 38.5 and np.sum(np.abs(z) < 1) >= 100
    ei, poi = T.reference_values(mu, sd, Y_MAX, XI)
    c_ei = T.worst(T.constants(ei, tr["ei"], tr["w_ei"]))
    c_poi = T.worst(T.constants(poi, tr["poi"], tr["w_poi"]))
    print(f"c_ref: EI {c_ei:.3f} POI {c_poi:.3f}")
    assert 0.1 <= c_ei <= 4.0 and 0.1 <= c_poi <= 4.0       # (a truth that says "anything goes" would measure ~0)
    g_ei, g_poi = T.reference_gradients(mu, sd, dmu, dsd, Y_MAX, XI)
    c_gei = T.worst(T.constants(g_ei, tr["g_ei"], tr["w_g_ei"]))
    c_gpoi = T.worst(T.constants(g_poi, tr["g_poi"], tr["w_g_poi"]))
    print(f"c_ref: gradient EI {c_gei:.3f} POI {c_gpoi:.3f}")
    assert 0.1 <= c_gei <= 4.0 and 0.1 <= c_gpoi <= 4.0
    # the floor covers a small share only: T < DBL_MIN needs z below about -37.5
    for t in (tr["t_ei"], tr["t_poi"]):
        assert np.mean(t < T.DBL_MIN) <= 0.05
    assert np.mean(tr["t_poi"] < T.DBL_MIN) > 0.0           # ... and the sample does reach it


def test_the_truth_is_not_the_reference_rewritten(sample):
    """Spot values no implementation detail enters: Phi(0) = 1/2, Phi(-z) + Phi(z) = 1, EI(z = 0) = sd / sqrt(2 pi), and a wrong
    value is seen: one ulp per (1 + z^2) off in the lower tail measures c ~ 1 / eps-fold of nothing but itself."""
    tr = T.acq_truth(np.array([1.25]), np.array([0.5]), 1.25, 0.0)
    assert tr["z"][0] == 0.0 and float(tr["poi"][0]) == 0.5
    assert abs(float(tr["ei"][0]) - 0.5 / np.sqrt(2 * np.pi)) < 1e-16
    mu, sd, _, _, big = sample
    a = np.linspace(0.0, 20.0, 41)
    up, lo = T.acq_truth(a, np.full(41, 0.5), 0.0, 0.0), T.acq_truth(-a, np.full(41, 0.5), 0.0, 0.0)      # z and -z exactly
    assert np.all(np.abs(T.to_float(up["poi"] + lo["poi"] - 1)) < 1e-45)
    assert np.all(np.abs(T.to_float(up["ei"] - lo["ei"] - a)) < 1e-45)           # EI(z) - EI(-z) = aa
    ei, poi = T.reference_values(mu, sd, Y_MAX, XI)
    tail = big["z"] < -8
    wrong = poi * (1.0 + 64 * T.EPS * (1.0 + big["z"] ** 2))
    assert T.worst(T.constants(wrong[tail], big["poi"][tail], big["w_poi"][tail])) > 32
    zeros = np.zeros(N)                                     # a kernel that returns zeros fails wherever T is a normal number
    c0 = T.constants(zeros, big["poi"], big["w_poi"])
    assert np.all(c0[big["t_poi"] > 1e-300] > 1e9)


def test_aa_is_the_fp64_difference():
    """With a truth built from the EXACT mu - y_max - xi the reference's own constant rises a hundredfold where the subtraction
    rounds (mu and y_max of opposite signs, the sum close to xi: the first operation is an addition, the second cancels): that is
    the subtraction's rounding, not the formula's — and every device site rounds it the same way."""
    import mpmath as mp

    rng = np.random.RandomState(2)
    n, y_max, xi = 400, -0.4, 1.0
    z = rng.uniform(-39.0, 39.0, n)
    sd = 10.0 ** rng.uniform(-6.0, np.log10(2.0), n)
    mu = z * sd + (y_max + xi)
    tr = T.acq_truth(mu, sd, y_max, xi)
    ei, _ = T.reference_values(mu, sd, y_max, xi)
    c_ei = T.worst(T.constants(ei, tr["ei"], tr["w_ei"]))
    ctx = T._ctx
    exact = []
    for m, s in zip(mu, sd):
        a = ctx.mpf(float(m)) - ctx.mpf(y_max) - ctx.mpf(xi)
        zz = a / ctx.mpf(float(s))
        exact.append(a * T._Phi(zz) + ctx.mpf(float(s)) * T._phi(zz))
    c_exact = T.worst(T.constants(ei, T._obj(exact), tr["w_ei"]))
    print(f"c_ref against the exact difference: {c_exact:.1f} (fp64 difference: {c_ei:.3f})")
    assert c_ei <= 4.0 and c_exact > 25 * c_ei
    assert mp.mp.dps < T.DPS                                # the helper works in a context of its own


def test_the_constraint_factor(sample):
    rng = np.random.RandomState(1)
    n = N
    m = rng.uniform(-1.0, 1.0, n)
    s = 10.0 ** rng.uniform(-6.0, np.log10(2.0), n)
    zl = rng.uniform(-39.0, 39.0, n)
    worst_c, floor_share = 0.0, []
    for i in range(0, n, 500):                              # six pairs of bounds: narrow band, one-sided either way, wide band
        sl = slice(i, i + 500)
        kind = (i // 500) % 4
        # bounds are per constraint, z per candidate: place the means so that candidate k sees z_l[k]
        lb, ub = 0.25, 0.25 + 0.01
        mm = lb - zl[sl] * s[sl]
        if kind == 1:
            lb = -np.inf
        elif kind == 2:
            ub = lb + 3.0
        elif kind == 3:
            ub = np.inf
        tr = T.band_truth(mm, s[sl], lb, ub)
        assert tr["ok"].all()
        c = T.constants(T.reference_band(mm, s[sl], lb, ub), tr["p"], tr["w"])
        worst_c = max(worst_c, T.worst(c))
        floor_share.append(np.mean(T.to_float(tr["w"]) < T.DBL_MIN))
    print(f"c_ref: factor {worst_c:.3f}")
    assert 0.1 <= worst_c <= 4.0
    assert np.mean(floor_share) <= 0.05
    # the short-circuits and the scale rule
    one = T.band_truth(m[:5], s[:5], -np.inf, np.inf)
    assert all(p == 1 for p in one["p"]) and all(w == 1 for w in one["w"])
    assert np.all(T.reference_band(m[:5], s[:5], -np.inf, np.inf) == 1.0)
    bad = T.band_truth(np.array([0.0, 0.0]), np.array([0.0, -1.0]), -1.0, 1.0)
    assert not bad["ok"].any() and all(T._ctx.isnan(p) for p in bad["p"])
    assert np.all(np.isnan(T.reference_band(np.array([0.0, 0.0]), np.array([0.0, -1.0]), -1.0, 1.0)))
