"""CPU: the problems of tests/test_gpu_sizes.py can fail, and its N / M lists reach both sides of every size switch.

Each plausible size bug — a ragged trtri pair whose off-diagonal block of W stays zero, the last diagonal block of L factored without
the previous step's rank-128 update, a posterior that skips the ragged last 64 rows of W, an LML graph replayed on the previous call's
y or X, an appended row scaled into Xs one row late — is applied to the oracle on the GPU test's own problems, and must move a quantity
that test compares by at least 100x the bar it holds it to.  NumPy only: no broken kernel is ever run."""
import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

from oracle import gp_oracle as O
from test_gpu_sizes import (FIT_NS, LANE_NS, NOISE, POST_CASES, POST_NPS, SHAPES, Problem, _post_shape, kernel_with_noise,
                            length_scale, lml_ref, make_data, small_batch_limit)

BARS = {"K": 1e-14, "L": 1e-10, "WL-I": 1e-7, "alpha": 1e-7, "mu": 1e-9, "sd": 1e-9, "lml": 1e-10, "grad": 1e-7}


def rel(x, ref):
    return float(np.max(np.abs(x - ref)) / max(float(np.max(np.abs(ref))), 1e-300))


def assert_far(moves, what):
    for k, m in moves.items():
        assert m >= 100 * BARS[k], f"{what}: {k} moves {m:.2e}, under 100x its bar {BARS[k]:.0e}"


def np_of(N):
    return (N + 63) // 64 * 64


def ragged_pairs(NP, nb=64):
    """(b, r0, b2) of every ragged pair of gpbo_api.hip trtri()'s recursive doubling."""
    out = []
    b = nb
    while b < NP:
        full = NP // (2 * b)
        rag = NP - full * 2 * b
        if rag > b:
            out.append((b, full * 2 * b, rag - b))
        b *= 2
    return out


def sd_with(W, p, Xc):
    """sigma over Xc from a given W = L^-1 (the device's formulation: var = 1 - ||W k*||^2), in units of y_std."""
    Kt = O.kernel_matrix(p.kernel, Xc, p.X, p.ls)
    V = W @ Kt.T
    return np.sqrt(np.maximum(1.0 - np.einsum("ij,ij->j", V, V), 0.0)) * p.ys


# -- the lists reach both sides of every switch ----------------------------------------------------------------------------
def test_the_size_lists_reach_both_sides_of_every_switch():
    nps = {np_of(N) for N in FIT_NS}
    assert 64 in nps and 128 in nps                                                           # fused | strip (64 | 65)
    assert 768 in nps and 832 in nps                                                          # strip | multi-launch (768 | 769)
    assert any(n <= 2048 for n in nps if n > 768) and any(2048 < n <= 4096 for n in nps) and any(n > 4096 for n in nps)  # outer panel
    assert 4032 in nps and 4096 in nps and 4160 in nps                                       # look-ahead from NP = 4096, 4032 below
    assert any((n // 64) % 2 for n in nps if n > 4096) and any((n // 64) % 2 for n in nps if 2048 < n < 4096)  # an odd last block
    b2s = {b2 for n in nps for _, _, b2 in ragged_pairs(n)}
    assert {128, 320, 384, 448, 960, 1984} <= b2s, sorted(b2s)
    assert any(1984 <= n < 2048 for n in nps) and any(2048 <= n < 4096 for n in nps)        # lml_batch grouping at 2048 ...
    assert 4032 in {np_of(N) for N in LANE_NS} and 4096 in {np_of(N) for N in LANE_NS}       # ... and at 4096, in the lane test
    for NP in POST_NPS:
        ms = {M for n, M in POST_CASES if n == NP}
        lim = small_batch_limit(NP)
        assert {lim, lim + 1, 4096, 4097} <= ms, NP
        if 256 < NP <= 512:
            for lo in (8064, 9088, 16384, 32640):             # Mp = round_up(M, 128) on both sides of 8192, 9216, 16384, 32768
                assert {lo, lo + 1} <= ms and (lo + 127) // 128 != (lo + 128) // 128, (NP, lo)
    chunks = {(NP + 255) // 256 for NP in POST_NPS}
    assert {1, 2, 3} <= chunks and max(chunks) >= 9


def test_the_problems_below_the_multi_launch_sizes_are_conditioned():
    """kappa in the window for the fit problems up to N = 1088 and the posterior grid's up to NP = 1088 (the GPU test asserts it for
    every case; the larger ones cost seconds each on a CPU)."""
    from test_gpu_sizes import KAPPA_WINDOW

    for N in (n for n in FIT_NS if n <= 1088):
        for s in SHAPES:
            p = Problem(N, *s, M=0)
            assert KAPPA_WINDOW[0] <= p.kappa <= KAPPA_WINDOW[1], p.what
    for NP in (n for n in POST_NPS if n <= 1088):
        p = Problem(NP - 7, *_post_shape(NP), M=0, seed=2)
        assert KAPPA_WINDOW[0] <= p.kappa <= KAPPA_WINDOW[1], p.what


# -- the bugs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (833, 4032))
def test_a_ragged_trtri_pair_with_its_off_diagonal_block_left_zero(N):
    p = Problem(N, *SHAPES[0])
    W = solve_triangular(p.L, np.eye(N), lower=True)
    sd = sd_with(W, p, p.Xc)
    pairs = ragged_pairs(np_of(N))
    assert pairs
    for b, r0, b2 in pairs:
        rows = slice(r0 + b, min(r0 + b + b2, N))
        cols = slice(r0, r0 + b)
        Wb = W.copy()
        Wb[rows, cols] = 0.0
        dWL = W[rows, cols] @ p.L[cols, :]              # (Wb - W) L, the only rows of Wb L - I that move
        assert_far({"WL-I": float(np.max(np.abs(dWL))), "sd": rel(sd_with(Wb, p, p.Xc), sd)}, f"N={N} pair b={b} b2={b2}")


@pytest.mark.parametrize("N", (2113, 5003))
def test_the_last_diagonal_block_without_the_previous_steps_update(N):
    p = Problem(N, *SHAPES[0], M=0)
    a = (N - 1) // 64 * 64                               # the last 64-row block (rows a .. N-1 of the real matrix)
    S = p.K[a:, a:] - p.L[a:, :a - 128] @ p.L[a:, :a - 128].T
    Lb = p.L.copy()
    Lb[a:, a:] = cholesky(S, lower=True)
    assert_far({"L": rel(Lb, p.L)}, f"N={N}")


def test_a_posterior_that_skips_the_ragged_last_row_chunk():
    """NP = 832 (the posterior grid's problem, N = 825): rows 768 .. 824 of W are the last row chunk's."""
    NP = 832
    p = Problem(NP - 7, *_post_shape(NP), M=300, seed=2)
    W = solve_triangular(p.L, np.eye(p.N), lower=True)
    Wb = W.copy()
    Wb[768:] = 0.0
    assert_far({"sd": rel(sd_with(Wb, p, p.Xc), sd_with(W, p, p.Xc))}, "last 64 rows of W ignored")


@pytest.mark.parametrize("N", (1088, 2113))
def test_an_lml_replayed_on_the_previous_calls_y_or_x(N):
    """The data sequence of test_lml_batch_graph_replay_on_new_data: a replay that read the previous call's y (call 2 on call 1's
    y) or X (call 3 on call 2's X)."""
    kernel, d = O.MATERN25, 5
    ls = length_scale(kernel, d, False, N)
    X1, y1, _ = make_data(N, d, 200 + N)
    X3, y2, _ = make_data(N, d, 300 + N)
    y1, y2 = O.normalize_targets(y1)[0], O.normalize_targets(y2)[0]
    for (Xr, yr), (Xs, ys), what in (((X1, y2), (X1, y1), "stale y"), ((X3, y2), (X1, y2), "stale X")):
        v, g = lml_ref(kernel, Xr, yr, ls)
        vb, gb = lml_ref(kernel, Xs, ys, ls)
        assert_far({"lml": abs(vb - v) / max(1.0, abs(v)), "grad": rel(gb, g)}, f"N={N} {what}")


@pytest.mark.parametrize("n0,k", [(767, 1), (768, 1), (1000, 1), (1005, 17), (2000, 100)])
def test_an_appended_row_scaled_into_xs_one_row_late(n0, k):
    """The rows of one fit_append call land one row down: row n0 keeps the zero padding (the scaled origin) and the last new row
    falls into the padding.  Measured as test_gpu_sizes' fit_append runs measure it (assert_same_model's K, L and posterior)."""
    kernel, d = O.MATERN25, 5
    n = n0 + k
    X, y, Xc = make_data(n, d, 7, M=300)
    ls = length_scale(kernel, d, False, n)
    Xb = X.copy()
    Xb[n0 + 1:n] = X[n0:n - 1]
    Xb[n0] = 0.0
    yn, _, _ = O.normalize_targets(y)
    gp, gpb = (O.fit_fixed_theta(kernel, Z, yn, ls, NOISE, normalize_y=False) for Z in (X, Xb))
    mu, sd = O.predict(gp, Xc)
    mub, sdb = O.predict(gpb, Xc)
    assert_far({"K": rel(kernel_with_noise(kernel, Xb, ls), kernel_with_noise(kernel, X, ls)), "L": rel(gpb.L, gp.L),
                "mu": rel(mub, mu), "sd": rel(sdb, sd)}, f"n0={n0} k={k}")
