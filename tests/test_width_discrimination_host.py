"""CPU: the problems of tests/test_gpu_width.py can fail.  Each plausible wide-kernel bug — a column dropped, the length scales
of columns t and t +- 32 swapped, the upper half of a 64-lane sum skipped (rows 2 and 3 of the wave, columns 32..63) — is applied
to the oracle, and must move K, mu / sigma and the LML gradient by at least 100x the bar the GPU test holds them to.  NumPy only:
no broken kernel is ever run."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from test_gpu_width import KERNELS, NOISE, PROBE_COLS, kernel_with_noise, length_scale, lml_oracle, post_tol, probe, problem

BARS = {"K": 1e-14, "grad": 1e-7}


def _partner(t):
    return t + 32 if t < 32 else t - 32


def _quantities(kernel, X, y, ls, Xc, keep=None):
    """K, (mu, sd) over Xc and the LML gradient, with only the columns in `keep` seen by the kernel (None: all of them)."""
    if keep is not None:
        X, Xc, ls = X[:, keep], Xc[:, keep], ls[keep]
    yn, _, _ = O.normalize_targets(y)
    gp = O.fit_fixed_theta(kernel, X, y, ls, NOISE)
    mu, sd = O.predict(gp, Xc)
    _, grad = lml_oracle(kernel, X, yn, ls)
    if keep is not None:
        full = np.zeros(64)
        full[keep] = grad
        grad = full
    return kernel_with_noise(kernel, X, ls), mu, sd, grad


def _moved(a, b):
    """The relative moves the GPU test measures (rel_err's max-norm): K, mu, sd, gradient (of its largest component)."""
    def rel(x, ref):
        return float(np.max(np.abs(x - ref)) / max(float(np.max(np.abs(ref))), 1e-300))

    return {"K": rel(a[0], b[0]), "mu": rel(a[1], b[1]), "sd": rel(a[2], b[2]), "grad": rel(a[3], b[3])}


def _assert_far(moves, kernel, what):
    bars = dict(BARS, mu=post_tol(kernel), sd=post_tol(kernel))
    for k, m in moves.items():
        assert m >= 100 * bars[k], f"{what}: {k} moves {m:.2e}, under 100x its bar {bars[k]:.0e}"


@pytest.mark.parametrize("kernel", KERNELS, ids=["matern", "rbf"])
@pytest.mark.parametrize("t", PROBE_COLS)
def test_single_live_column_perturbations_are_far_outside_the_bars(kernel, t):
    X, y, ls, Xc = probe(50, t, kernel, M=200)
    ref = _quantities(kernel, X, y, ls, Xc)
    assert np.count_nonzero(ref[3]) == 1 and ref[3][t] != 0.0

    # column t lost (zero in X and in the candidates): every point coincides
    Xz, Xcz = X.copy(), Xc.copy()
    Xz[:, t] = 0.0
    Xcz[:, t] = 0.0
    _assert_far(_moved(_quantities(kernel, Xz, y, ls, Xcz), ref), kernel, f"t={t} zeroed")

    # length scale of column t +- 32 applied to column t (and the other way round)
    sw = ls.copy()
    p = _partner(t)
    sw[t], sw[p] = ls[p], ls[t]
    moved = _moved(_quantities(kernel, X, y, sw, Xc), ref)
    _assert_far(moved, kernel, f"t={t} swapped with {p}")

    # a 64-lane sum that adds only rows 0 and 1 of the wave: columns 32..63 never reach the distance
    if t >= 32:
        _assert_far(_moved(_quantities(kernel, X, y, ls, Xc, keep=np.arange(32)), ref), kernel, f"t={t} upper half dropped")


@pytest.mark.parametrize("kernel", KERNELS, ids=["matern", "rbf"])
def test_the_upper_half_of_a_full_width_problem_matters(kernel):
    """The every-column problem at d = 64: dropping columns 32..63, or swapping the length scales of the two halves, moves every
    compared quantity far outside its bar."""
    X, y, ls, Xc = problem(120, 64, kernel, M=200)
    ref = _quantities(kernel, X, y, ls, Xc)
    assert np.all(ref[3] != 0.0)
    _assert_far(_moved(_quantities(kernel, X, y, ls, Xc, keep=np.arange(32)), ref), kernel, "columns 32..63 dropped")
    sw = np.concatenate([ls[32:], ls[:32]])
    _assert_far(_moved(_quantities(kernel, X, y, sw, Xc), ref), kernel, "halves' length scales swapped")


def test_the_problems_are_conditioned_and_every_column_is_live():
    """kappa(K) between 1e1 and 1e8 wherever the GPU test compares, and the per-column length scales are all distinct."""
    from test_gpu_width import FIT_NS, WIDTHS, kappa

    for d in WIDTHS:
        ls = length_scale(d, O.MATERN25, True)
        assert np.unique(ls).shape == (d,)
    for N in FIT_NS:
        for kernel in KERNELS:
            for d in (4, 17, 64):
                X, _, ls, _ = problem(N, d, kernel)
                assert 1e1 <= kappa(kernel, X, ls) <= 1e8, (N, d, kernel)
    for t in (0, 63):
        X, _, ls, _ = probe(1000, t, O.RBF)
        assert 1e1 <= kappa(O.RBF, X, ls) <= 1e8
