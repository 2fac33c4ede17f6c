"""GPU (-m gpu): every (padded width, kernel kind[, accumulator count]) INSTANCE of the kernels that generate k* on the device
behind with_dp_kernel (csrc/gpbo_internal.h) and that tests/test_gpu_width.py predates: path_eval_kernel<DP, K, NS>
(gpbo_sample_paths), path_ascend_kernel<DP, K> (gpbo_ascend_paths), kg_points_kernel<DP, K> and kg_cov_kernel<DP, K, NS>
(gpbo_kg_argbest), posterior_refresh_kernel<DP, K, .> (gpbo_posterior_refresh), and the five row widths of
trust_region_wave_kernel (gpbo_generate_candidates_trust_region).  An instance has its own unrolled loops, LDS image, register
budget and launch-bounds fit; the sibling files run the edges of the CODE (sizes, tiers, conventions), this one the instance axis.

Widths: one per tier with the padding columns live-adjacent, d = 3, 6, 11, 23, 47 (DP = 4, 8, 16, 32, 64, each partly filled), and
the full d = 64.  Kinds: all four.  Per-column length scales and a target built from every column, so a lost, duplicated or
mis-strided column changes the answer; tests/test_instance_cover_host.py asserts that these tables reach the full product of
instances and that the plausible instance bugs move every compared quantity by at least 100x its bar.

Shapes, the smallest at which these kernels can still go wrong: N = 130 (its rows cross the 64-row LDS stage twice, the last stage
is short), M = 257 (several single-wave workgroups and a ragged last one), F = 65 (one full 64-feature LDS stage and one left over).

No bar here is new:
  gpbo_sample_paths        tests/test_gpu_sample_paths.py: err_of, bar max(1e-9, 8 x the spread between paths_cho and paths_winv), and
                           its `check` (the picks compared wherever the truth's best and second are GAP_FLOOR apart: asserted on
                           the truth alone; it holds in every case at the sibling's default data seed, checked on the CPU);
  gpbo_ascend_paths        tests/test_gpu_path_ascent.py: check_evaluation (max_iter = 0: value and gradient, its two bars);
  gpbo_kg_argbest          tests/test_gpu_kg.py: kg_truth.BAR on |error| / scale, the point means, the selection exact against the
                           returned values; the truth of every case must have >= 10 % of its candidates at KG >= 1e-3 scale (KG_F:
                           the length-scale factor per (d, kind) that achieves it, found on the CPU with kg_truth);
  gpbo_posterior_refresh   tests/test_gpu_posterior_refresh.py: route 1, test_gpu_sizes.check_posterior at tol_of(kind) against the
                           oracle's refit and against the device's own full pass;
  trust-region generator   tests/test_gpu_turbo.py: test_generator_equals_the_truth_bit_for_bit itself, at other shapes.

posterior_refresh_kernel, (tier, kind) pairs that tests/test_gpu_posterior_refresh.py reaches: its shapes have d = 1 and 3 (DP 4) and
d = 16 (DP 16) with all four kinds, d = 8 (DP 8) and d = 64 (DP 64) with Matern-2.5 and RBF only; its further tests use d = 3, 5, 8, 16
with Matern-2.5 or RBF.  Never run: DP 8 with nu = 1.5 / 0.5, DP 32 with any kind, DP 64 with nu = 1.5 / 0.5 — REFRESH_CASES, at
that file's smallest shape (N0 = 5, one appended row, M = 257).

Each parametrised test prints its worst error over its bar; the worst per kernel goes as JSON to the file GPBO_INSTANCE_REPORT names
(if set)."""
import functools

import numpy as np
import pytest

import kg_truth as KT
import matern_family_truth as F
import test_gpu_kg as KG
import test_gpu_path_ascent as PA
import test_gpu_posterior_refresh as RF
import test_gpu_sample_paths as SP
import test_gpu_sizes as SZ
import test_gpu_turbo as TT
from conftest import rel_err
from mes_truth import argbest

pytestmark = pytest.mark.gpu

DIMS = (3, 6, 11, 23, 47, 64)
KINDS = (F.RBF, F.MATERN25, F.MATERN15, F.MATERN05)
KNAME = SP.KNAME
N, M, FN = 130, 257, 65

#: worst error / bar per kernel
WORST = {}


def record(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _instance_report():
    yield
    import json
    import os

    print("worst error / bar per kernel: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))
    out = os.environ.get("GPBO_INSTANCE_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(dict(sorted(WORST.items())), f, indent=1)


# ---- gpbo_sample_paths: path_eval_kernel<DP, K, NS> ---------------------------------------------------------------------------------
PATH_S = (1, 3, 5)          # NS = 1, 4 and 16 (path_plan.h: path_eval_ns), the last two partly filled
PATH_CASES = [(d, k, S) for d in DIMS for k in KINDS for S in PATH_S]


@functools.lru_cache(maxsize=None)
def path_case(d, kind, S):
    """(the sibling's default data seed: with it the truth's best and second best are GAP_FLOOR apart in every case, which
    tests/test_instance_cover_host.py asserts on the CPU)"""
    c = SP.Case(N, M, FN, d, S, kind, True, "fp64")
    c.ref, c.bar, c.own = c.references()
    return c


@pytest.mark.parametrize("d,kind,S", PATH_CASES, ids=[f"d{d}-{KNAME[k]}-s{S}" for d, k, S in PATH_CASES])
def test_sample_paths_instance(engine, d, kind, S):
    c = path_case(d, kind, S)
    c.fit(engine)
    e = SP.check(c, *c.sample(engine), c.ref, c.bar, c.own)
    print(f"{c.what}: error / bar {e / c.bar:.2e}")
    record("path_eval_kernel", e / c.bar)


# ---- gpbo_ascend_paths: path_ascend_kernel<DP, K> -----------------------------------------------------------------------------------
ASCENT_S, ASCENT_K = 5, 3
ASCENT_CASES = [(d, k) for d in DIMS for k in KINDS]


@functools.lru_cache(maxsize=None)
def ascent_case(d, kind):
    c = PA.Case(N, FN, d, ASCENT_S, ASCENT_K, kind, True, "fp64")
    c.ref = c.references(c.clipped)
    return c


@pytest.mark.parametrize("d,kind", ASCENT_CASES, ids=[f"d{d}-{KNAME[k]}" for d, k in ASCENT_CASES])
def test_ascend_paths_instance(engine, d, kind):
    c = ascent_case(d, kind)
    c.fit(engine)
    out = c.ascend(engine, max_iter=0, return_gradient=True)
    f_ref, g_ref, bar_f, bar_g = c.ref[:4]
    worst = max(PA.err_f(out["f"], f_ref) / bar_f, PA.err_g(out["g"], g_ref) / bar_g)
    print(f"{c.what}: worst error / bar {worst:.2e}")
    PA.check_evaluation(c, out, c.ref)
    record("path_ascend_kernel", worst)


# ---- gpbo_kg_argbest: kg_points_kernel<DP, K>, kg_cov_kernel<DP, K, NS> -----------------------------------------------------------
KG_N = 40
KG_J = (9, 25, 40)          # NS = 16, 32 and 64 by kg_cov_ns' own rule (kg.hip), each partly filled; GPBO_KG_NS is not set
KG_CASES = [(d, k, J) for d in DIMS for k in KINDS for J in KG_J]
#: the length-scale factor f (length scale = f sqrt(d) x the per-column spread) per (d, kind) at which the truth has at least 10 % of
#: its candidates at KG >= 1e-3 scale for every J above: the largest of 0.5, 0.4, 0.3, 0.25, 0.2, 0.15, 0.12 with a share of at least
#: 30 %, found on the CPU with kg_truth on the oracle's posterior (the share is not monotone in f: a long length scale leaves
#: little to learn, a short one little covariance with the points)
KG_F = {(d, k): 0.5 for d in DIMS for k in KINDS}
KG_F.update({(3, F.MATERN25): 0.12, (3, F.MATERN05): 0.25, (6, F.RBF): 0.3, (23, F.RBF): 0.3, (47, F.RBF): 0.3})


@functools.lru_cache(maxsize=None)
def kg_case(d, kind, J):
    return KG.Case(KG_N, d, M, kind, KG_F[(d, kind)], J)


def kg_points(c, mu):
    """suggest_kg's points (the sibling's `points`) in REVERSE order: the highest means last.  A line changes KG only where it is
    on the upper envelope, and the highest mean's always is: in this order the last live accumulators of the partly filled NS group —
    where an instance goes wrong first — hold the lines that no candidate's value can do without.  (In the sibling's order they
    hold the low-mean points, and the last but one reading the last one's weights moves no value at all.)"""
    return np.ascontiguousarray(c.points(mu)[::-1])


@pytest.mark.parametrize("d,kind,J", KG_CASES, ids=[f"d{d}-{KNAME[k]}-j{J}" for d, k, J in KG_CASES])
def test_kg_instance(engine, d, kind, J):
    c = kg_case(d, kind, J)
    what = f"{c.what} {KNAME[kind]}"
    mu, sd = c.posterior(engine)
    pts = kg_points(c, mu)
    bi, bv, si, sv, ys, mu_pts = engine.kg_argbest(pts, k_seeds=8, y_mean=KG.Y_MEAN, y_std=KG.Y_STD, return_values=True,
                                                   return_point_means=True)
    want_pts = c.mean_at(pts)
    e_pts = np.abs(mu_pts - want_pts).max() / max(1.0, np.abs(want_pts).max())
    print(f"{what}: point means off by {np.abs(mu_pts - want_pts).max():.2e}, error / bar {e_pts / KT.BAR:.2e}")
    assert e_pts <= KT.BAR
    want, scale = c.truth(mu, sd, pts, mu_pts)
    assert np.mean(want >= 1e-3 * scale) >= 0.10, "the truth is (nearly) zero everywhere: this fixture checks nothing"
    worst = KG.check_values(what, ys, want, scale)
    print(f"{what}: values' error / bar {worst / KT.BAR:.2e}")
    record("kg_points_kernel", e_pts / KT.BAR)
    record("kg_cov_kernel", worst / KT.BAR)
    # the selection, exact against the returned values
    wi, wv, wsi, wsv = argbest(ys, 8)
    assert bi == wi and bv == wv and np.array_equal(si, wsi) and np.array_equal(sv, wsv)


# ---- gpbo_posterior_refresh: the (tier, kind) pairs its own file leaves out ---------------------------------------------------------
REFRESH_N0, _, REFRESH_M, REFRESH_ROWS, _ = RF.SHAPES["one-launch"]
REFRESH_CASES = [(6, F.MATERN15), (6, F.MATERN05), (23, F.RBF), (23, F.MATERN25), (23, F.MATERN15), (23, F.MATERN05),
                 (47, F.MATERN15), (47, F.MATERN05)]


@functools.lru_cache(maxsize=None)
def refresh_case(d, kind):
    c = RF.Case(REFRESH_N0, d, REFRESH_M, REFRESH_ROWS, True, kind)
    c.mu_o, c.sd_o = c.truth(c.N)
    return c


@pytest.mark.parametrize("d,kind", REFRESH_CASES, ids=[f"d{d}-{KNAME[k]}" for d, k in REFRESH_CASES])
def test_posterior_refresh_instance(engine, d, kind):
    c = refresh_case(d, kind)
    tol = RF.tol_of(kind)
    RF.arm(engine, c)
    ym, ys = RF.append(engine, c, c.N0, c.N)
    mu, sd, route = engine.posterior_refresh(0, ym, ys, return_route=True)
    assert route == 1
    worst = max(rel_err(mu, c.mu_o), rel_err(sd, c.sd_o)) / tol
    print(f"{c.what}: vs oracle mu {rel_err(mu, c.mu_o):.2e} sd {rel_err(sd, c.sd_o):.2e}, worst error / bar {worst:.2e}")
    SZ.check_posterior(mu, sd, c.mu_o, c.sd_o, ys, c.what + " refresh vs oracle", tol)
    mu_f, sd_f = engine.posterior(0, ym, ys)
    SZ.check_posterior(mu, sd, mu_f, sd_f, ys, c.what + " refresh vs full pass", tol)
    record("posterior_refresh_kernel", worst)


# ---- gpbo_generate_candidates_trust_region: the ballot groups of 1, 2 and 8 lanes ----------------------------------------------------
def _tr_rows(d):
    """rows of one workgroup of trust_region_wave_kernel at d = 4 << lc: 1024 >> lc"""
    return 4096 // d


TR_SHAPES = [(d, m) for d in (4, 8, 32) for m in (1, _tr_rows(d) - 1, _tr_rows(d) + 1, 4099)]


@pytest.mark.parametrize("d,m", TR_SHAPES, ids=[f"d{d}-m{m}" for d, m in TR_SHAPES])
def test_trust_region_wave_width(engine, d, m):
    """the four thresholds, the bit-for-bit comparison against turbo_truth.generate and the at least one / exactly one / all d
    coordinates changed assertions of the sibling's test, run as they stand"""
    TT.test_generator_equals_the_truth_bit_for_bit(engine, d, m)
