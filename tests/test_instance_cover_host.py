"""CPU: what tests/test_gpu_instances.py rests on, asserted here and not hoped for.

Coverage.  pad_dim (csrc/gpbo_internal.h), path_eval_ns (csrc/path_plan.h) and kg_cov_ns (csrc/kg.hip) are restated in Python and
pinned to the sources (path_plan.h compiled for the host as tests/test_path_plan_host.py does; the other two are one expression each,
cut out of their file and compiled the same way).  Through them the GPU file's case tables map onto the FULL product of instances:
path_eval_kernel 5 widths x 4 kinds x NS {1, 4, 16} = 60, path_ascend_kernel 20, kg_points_kernel 20, kg_cov_kernel x NS {16, 32,
64} = 60, posterior_refresh_kernel 20 together with tests/test_gpu_posterior_refresh.py's own cases, and the row widths lc = 0 .. 4 of
trust_region_wave_kernel together with tests/test_gpu_turbo.py's shapes.  The tables are imported, not copied.

Conditions of the GPU cases that depend on the reference alone: every gpbo_sample_paths case has its truth's best and second best
GAP_FLOOR apart; every gpbo_kg_argbest case has at least 10 % of its candidates at KG >= 1e-3 scale on the oracle's posterior.

Discrimination, in the manner of tests/test_width_discrimination_host.py.  The plausible instance bugs are applied to the NumPy truth
of what ONE kernel instance computes (the model it reads — K, W, alpha, the path weights V — stays the correct one: other kernels
made it) and must move the compared quantity by at least 100x the bar the GPU test holds it to, for every (d, kind) of the tables:
  drop    the last live column of the tier never reaches the distance (and, separately, the feature argument);
  pad     the first padding column read as live: the point's side holds the point's (scaled) column 0, the train side 0 — a
          mis-strided read; at d = 64 there is no padding column;
  kind    a neighbouring kind's formula (kind - 1, kind + 1 where they exist);
  acc     one accumulator of a partly filled NS group reading its neighbour's weights: the last but one live column reads the
          last one's, and the last live column the zero column beyond it.
NumPy only: no broken kernel is ever run."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky, solve_triangular

import kg_truth as KT
import matern_family_truth as F
import paths_ascent_truth as AT
import paths_truth as P
import test_gpu_instances as I
import test_gpu_kg as KG
import test_gpu_path_ascent as PA
import test_gpu_posterior_refresh as RF
import test_gpu_sample_paths as SP
import test_gpu_turbo as TT
import test_path_plan_host as PP
from conftest import ROOT, rel_err

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")
TIERS = (4, 8, 16, 32, 64)
FAR = 100.0


# ---- the dispatch rules, restated ---------------------------------------------------------------------------------------------------
def pad_dim(d):
    return 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64


def path_eval_ns(S):
    return 1 if S == 1 else (4 if S <= 4 else 16)


def kg_cov_ns(J):
    return 16 if J <= 16 else (32 if J <= 32 else 64)


def test_path_eval_ns_is_the_headers(tmp_path):
    plan = PP.Plan(str(tmp_path))
    assert [plan.L.ns(S) for S in range(1, 17)] == [path_eval_ns(S) for S in range(1, 17)]


def test_pad_dim_and_kg_cov_ns_are_the_sources(tmp_path):
    """the one-line pad_dim of gpbo_internal.h and the return expression of kg.hip's kg_cov_ns (the debug build's GPBO_KG_NS
    override in front of it is not the product's rule), compiled for the host as they stand"""
    pad = re.search(r"^inline int pad_dim\(int d\) \{[^\n]*\}$", open(os.path.join(CSRC, "gpbo_internal.h")).read(), re.M)
    ns = re.search(r"^static int kg_cov_ns\(int J\) \{\n(?:[^\n}]*\n)*?(  return J [^\n]*;)\n\}$",
                   open(os.path.join(CSRC, "kg.hip")).read(), re.M)
    assert pad and ns, "pad_dim / kg_cov_ns are no longer where this test reads them"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, so = str(tmp_path / "rules.cpp"), str(tmp_path / "librules.so")
    with open(src, "w") as f:
        f.write(pad.group(0) + '\nextern "C" {\nint pad(int d) { return pad_dim(d); }\nint kg_ns(int J) {\n' + ns.group(1) + "\n}\n}\n")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    assert [L.pad(d) for d in range(1, 65)] == [pad_dim(d) for d in range(1, 65)]
    assert [L.kg_ns(J) for J in range(1, 65)] == [kg_cov_ns(J) for J in range(1, 65)]


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
def test_the_case_tables_reach_every_instance():
    assert {pad_dim(d) for d in I.DIMS} == set(TIERS) and set(I.KINDS) == {F.RBF, F.MATERN25, F.MATERN15, F.MATERN05}
    # one width per tier with padding columns live-adjacent, and the full 64
    assert sorted(d for d in I.DIMS if d < pad_dim(d)) == [3, 6, 11, 23, 47] and 64 in I.DIMS
    both = {(t, k) for t in TIERS for k in I.KINDS}
    path_eval = {(pad_dim(d), k, path_eval_ns(S)) for d, k, S in I.PATH_CASES}
    assert path_eval == {(t, k, ns) for t, k in both for ns in (1, 4, 16)} and len(path_eval) == 60
    assert all(S < path_eval_ns(S) for S in I.PATH_S if S > 1), "the NS groups above 1 are partly filled"
    ascent = {(pad_dim(d), k) for d, k in I.ASCENT_CASES}
    assert ascent == both and len(ascent) == 20
    kg_points = {(pad_dim(d), k) for d, k, _ in I.KG_CASES}
    assert kg_points == both and len(kg_points) == 20
    kg_cov = {(pad_dim(d), k, kg_cov_ns(J)) for d, k, J in I.KG_CASES}
    assert kg_cov == {(t, k, ns) for t, k in both for ns in (16, 32, 64)} and len(kg_cov) == 60
    assert all(J < kg_cov_ns(J) for J in I.KG_J), "every NS group is partly filled"
    assert set(I.KG_F) == {(d, k) for d in I.DIMS for k in I.KINDS}
    # the refresh kernel: the sibling's own cases and the ones added, no pair twice
    own = {(pad_dim(RF.SHAPES[s][1]), k) for s, k in RF.CASES}
    added = {(pad_dim(d), k) for d, k in I.REFRESH_CASES}
    assert not (own & added) and (own | added) == both and len(own | added) == 20
    assert (I.REFRESH_N0, I.REFRESH_M, I.REFRESH_ROWS) == (5, 257, 1)
    # the wave kernel serves d = 4 << lc alone
    lc_of = {4 << lc: lc for lc in range(5)}
    assert {lc_of[d] for d, _ in TT.SHAPES if d in lc_of} == {2, 4}
    assert {lc_of[d] for d, _ in I.TR_SHAPES} == {0, 1, 3}
    for d in (4, 8, 32):
        R = 1024 >> lc_of[d]
        assert {m for dd, m in I.TR_SHAPES if dd == d} == {1, R - 1, R + 1, 4099}


# ---- the references' own conditions -------------------------------------------------------------------------------------------------
def test_every_sample_paths_case_has_a_pick_to_compare():
    for d, kind, S in I.PATH_CASES:
        c = I.path_case(d, kind, S)
        _, gaps = P.argmax_with_gap(c.ref)
        assert gaps.min() >= SP.GAP_FLOOR, f"{c.what}: the truth's own best / second gap {gaps.min():.2e}: pick another seed"


def oracle_posterior(c):
    gp = F.fit_fixed_theta(c.kind, c.X, c.yn, c.ls, KG.NOISE, normalize_y=False)
    mu, sd = F.predict(gp, c.Xc)
    return gp, KG.Y_STD * mu + KG.Y_MEAN, KG.Y_STD * sd


def test_every_kg_case_has_something_to_learn():
    for d, kind, J in I.KG_CASES:
        c = I.kg_case(d, kind, J)
        _, mu, sd = oracle_posterior(c)
        pts = I.kg_points(c, mu)
        want, scale = c.truth(mu, sd, pts, c.mean_at(pts))
        share = float(np.mean(want >= 1e-3 * scale))
        assert share >= 0.10, f"{c.what} {I.KNAME[kind]}: {share:.2f} of the candidates at KG >= 1e-3 scale: another f"


# ---- discrimination -------------------------------------------------------------------------------------------------------------------
def mutants(d, kind):
    out = ["drop"] + (["pad"] if d < pad_dim(d) else [])
    return out + [("kind", k) for k in (kind - 1, kind + 1) if k in I.KINDS]


def mutate(mutant, kind, A, B, ls):
    """(kind, points A, train points B, length scales) as the broken instance sees them"""
    if mutant == "drop":
        return kind, A[..., :-1], B[:, :-1], ls[:-1]
    if mutant == "pad":
        return kind, np.concatenate([A, A[..., :1]], axis=-1), np.hstack([B, np.zeros((B.shape[0], 1))]), np.append(ls, ls[0])
    if isinstance(mutant, tuple):
        return mutant[1], A, B, ls
    return kind, A, B, ls


def kstar(mutant, kind, A, B, ls):
    return F.kernel_matrix(*mutate(mutant, kind, A, B, ls))


def far(move, bar, what):
    assert move >= FAR * bar, f"{what}: moves {move:.2e}, under {FAR:.0f}x its bar {bar:.2e}"


def neighbour_weights(V, n_live):
    """the two `acc` bugs on weight columns V (N, n_live): yields (name, V')"""
    a = V.copy()
    a[:, n_live - 2] = V[:, n_live - 1]
    yield "acc: the last but one reads the last", a
    b = V.copy()
    b[:, n_live - 1] = 0.0
    yield "acc: the last reads the zero column", b


@pytest.mark.parametrize("d", I.DIMS)
@pytest.mark.parametrize("kind", I.KINDS, ids=[I.KNAME[k] for k in I.KINDS])
def test_sample_paths_bugs_are_far_outside_the_bar(d, kind):
    for S in (5, 3):
        c = I.path_case(d, kind, S)
        U, Gc, K, Kt = P._parts(kind, c.X, c.ls, c.eta, 1.0, c.omega, c.phase, c.w, c.eps, c.Xc)
        V = cho_solve((cholesky(K, lower=True), True), c.yn[:, None] - U)

        def values(Kt, V, Gc=Gc):
            return (SP.Y_STD * (Gc + Kt @ V) + SP.Y_MEAN).T

        assert SP.err_of(values(Kt, V), c.ref) <= 1e-12                       # the pieces are the reference's
        for name, Vm in neighbour_weights(V, S):
            far(SP.err_of(values(Kt, Vm), c.ref), c.bar, f"{c.what} {name}")
        if S != 5:
            continue
        for m in mutants(d, kind):
            far(SP.err_of(values(kstar(m, kind, c.Xc, c.X, c.ls), V), c.ref), c.bar, f"{c.what} {m}")
        fs = np.sqrt(2.0 / c.F)                                              # the feature phase without its last column
        G_drop = fs * (P.features(c.omega[:, :-1], c.phase, (c.Xc / c.ls)[:, :-1]) @ c.w.T)
        far(SP.err_of(values(Kt, V, G_drop), c.ref), c.bar, f"{c.what} drop (features)")


@pytest.mark.parametrize("d", I.DIMS)
@pytest.mark.parametrize("kind", I.KINDS, ids=[I.KNAME[k] for k in I.KINDS])
def test_ascend_paths_bugs_are_far_outside_the_bars(d, kind):
    c = I.ascent_case(d, kind)
    f_ref, g_ref, bar_f, bar_g = c.ref[:4]
    V = P.path_weights(*c.truth_args())
    omega = np.asarray(c.omega, dtype=np.float64)
    for m in mutants(d, kind):
        k2, Xq, X, ls = mutate(m, kind, c.clipped, c.X, c.ls)
        om = omega[:, :-1] if m == "drop" else (np.hstack([omega, np.zeros((c.F, 1))]) if m == "pad" else omega)
        f, g = AT.path_value_grad(k2, X, c.yn, ls, c.eta, om, c.phase, c.w, c.eps, Xq, PA.Y_MEAN, PA.Y_STD, V=V)
        g = np.concatenate([g, np.zeros(g.shape[:2] + (1,))], axis=2)[:, :, :d]      # the d components the kernel stores
        far(PA.err_f(f, f_ref), bar_f, f"{c.what} {m}: value")
        far(PA.err_g(g, g_ref), bar_g, f"{c.what} {m}: gradient")


KG_SUBSET = 96          # candidates the envelopes are rebuilt for (kg_values is a Python loop per candidate)


@pytest.mark.parametrize("d", I.DIMS)
@pytest.mark.parametrize("kind", I.KINDS, ids=[I.KNAME[k] for k in I.KINDS])
def test_kg_bugs_are_far_outside_the_bar(d, kind):
    for J in I.KG_J:
        c = I.kg_case(d, kind, J)
        gp, mu, sd = oracle_posterior(c)
        pts = I.kg_points(c, mu)
        mu_pts = c.mean_at(pts)
        Xc, mu_s, sd_s = c.Xc[:KG_SUBSET], mu[:KG_SUBSET], sd[:KG_SUBSET]
        B = cho_solve((gp.L, True), F.kernel_matrix(kind, c.X, pts, c.ls))     # K'^-1 k*(a_j): the device's -V

        def kg(m, Bm):
            cov = kstar(m, kind, Xc, pts, c.ls) - kstar(m, kind, Xc, c.X, c.ls) @ Bm
            return KT.kg_values(mu_s, sd_s, cov, mu_pts, KG.Y_STD, KG.NOISE, 0.0, return_scale=True)

        ref, scale = kg(None, B)
        want, _ = c.truth(mu_s, sd_s, pts, mu_pts, Xc=Xc)
        assert np.nanmax(np.abs(ref - want) / scale) <= 1e-12                  # the pieces are the reference's
        what = f"{c.what} {I.KNAME[kind]}"
        for name, Bm in neighbour_weights(B, J):
            far(float(np.nanmax(np.abs(kg(None, Bm)[0] - ref) / scale)), KT.BAR, f"{what} kg_cov {name}")
        if J != I.KG_J[0]:
            continue
        for m in mutants(d, kind):
            far(float(np.nanmax(np.abs(kg(m, B)[0] - ref) / scale)), KT.BAR, f"{what} kg_cov {m}")
            got = KG.Y_STD * (kstar(m, kind, pts, c.X, c.ls) @ gp.alpha) + KG.Y_MEAN
            far(float(np.abs(got - mu_pts).max() / max(1.0, np.abs(mu_pts).max())), KT.BAR, f"{what} kg_points {m}")


@pytest.mark.parametrize("d,kind", I.REFRESH_CASES, ids=[f"d{d}-{I.KNAME[k]}" for d, k in I.REFRESH_CASES])
def test_posterior_refresh_bugs_are_far_outside_the_bar(d, kind):
    """the incremental route restated: mu = y_std k* . alpha + y_mean, var = var_old - (W[N - 1, :] . k*)^2 for the one appended row"""
    c = I.refresh_case(d, kind)
    tol = RF.tol_of(kind)
    yn, ym, ys = c.norm(c.N)
    X = c.X[:c.N]
    gp = F.fit_fixed_theta(kind, X, yn, c.ls, RF.NOISE, normalize_y=False)
    w_row = solve_triangular(gp.L, np.eye(c.N), lower=True)[c.N - 1]
    gp0 = F.fit_fixed_theta(kind, c.X[:c.N0], c.norm(c.N0)[0], c.ls, RF.NOISE, normalize_y=False)
    var_old = F._normal_variance(gp0, F.kernel_matrix(kind, c.Xc, c.X[:c.N0], c.ls))

    def refresh(m, a=gp.alpha, w=w_row):
        Kt = kstar(m, kind, c.Xc, X, c.ls)
        return ys * (Kt @ a) + ym, ys * np.sqrt(np.maximum(var_old - (Kt @ w) ** 2, 0.0))

    mu, sd = refresh(None)
    assert rel_err(mu, c.mu_o) <= 1e-10 and rel_err(sd, c.sd_o) <= 1e-7       # the restatement is the oracle's refit
    for m in mutants(d, kind):
        mu_m, sd_m = refresh(m)
        far(rel_err(mu_m, c.mu_o), tol, f"{c.what} {m}: mu")
        far(rel_err(sd_m, c.sd_o), tol, f"{c.what} {m}: sd")
    mu_m, sd_m = refresh(None, a=w_row, w=gp.alpha)                           # acc: the two weight columns of NC = 2 swapped
    far(rel_err(mu_m, c.mu_o), tol, f"{c.what} acc: mu")
    far(rel_err(sd_m, c.sd_o), tol, f"{c.what} acc: sd")
