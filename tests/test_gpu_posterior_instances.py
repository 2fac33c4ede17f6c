"""GPU (-m gpu): every (padded width, kernel kind) INSTANCE of the five k*-generating templates of the posterior pass, the ones that
tests/test_gpu_width.py already ran and tests/test_gpu_instances.py therefore left alone:

    posterior_kernel_v2<DP, K, 1>            Fused256, 8 waves                  launch_posterior_fused
    posterior_kernel_v2<DP, K, 1, 32, 16>    Fused512, 16 waves, 1024 threads   launch_posterior_fused
    kstar_gen_kernel<DP, K, SlabF64>         launch_gen
    kstar_gen_kernel<DP, K, SlabI8>          launch_gen
    kstar_gen_kernel<DP, K, SlabF32>         launch_gen

5 templates x 5 widths x 4 kinds = 100 instances.  The earlier files met nu = 1.5 / 0.5 at one width only (tests/test_gpu_matern_family.py,
DP 8; its int8 case DP 16); tests/test_posterior_instance_cover_host.py holds the table of the instances that none of them launched and
asserts that the tables below reach all 100, each by SHAPE under the product's own rule (csrc/posterior_plan.h; no GPBO_POST_* switch is
read by the product build).

ROWS: the smallest shapes at which each kernel still runs its full structure.  N is off the 64-row padding, the last row chunk is
ragged, M is ragged against the 64-candidate tile and the 128 granule.  Widths and kinds are test_gpu_instances': d = 3, 6, 11, 23, 47
(one partly filled width per tier) and the full 64, all four kinds: 8 x 6 x 4 = 192 cases.  Data: test_gpu_sizes.make_data (a target
built from every column, candidate 7 ON training point 3), per-column length scales on test_gpu_posterior_refresh.length_scale's
pattern (LS_F3: the shorter factors d = 3 needs to keep kappa(K + 1e-6 I) under 5e6, found on the CPU).  The reference is
tests/matern_family_truth.py, computed once per (N, d, kind) and shared between the rows of equal N.

Each case runs three passes over the same M candidates (same path, same tiling):
  (a) clean, against the oracle.  No bar is new: fp64 rows test_gpu_sizes.check_posterior at test_gpu_posterior_refresh.tol_of(kind)
      (1e-9 Matern / 1e-6 RBF max-norm, 1e-5 per candidate); fp32 rows tests/test_gpu_f32.py's rel_err(mu) < 1e-7 and
      max |sd^2 - sd_ref^2| < 2e-5 y_std^2.
  (b) edited: at most six rows replaced (EDITS: NaN in the last live column, all NaN, +inf, -inf, a copy of training point N - 1 — in
      the ragged last chunk —, every coordinate 1e3), the rest untouched.  isnan(mu), isnan(sd) are the oracle's pattern exactly; every
      row that was not edited has the clean pass's BITS; the far row has mu == y_mean exactly and |sd - y_std| <= 1e-12 y_std; the copy
      is finite, sd >= 0, and within the per-candidate bar (fp64) / the variance bar (fp32) of the oracle; gpbo_acq_argbest (UCB) returns
      the first NaN (row 1) with a NaN value and its values' NaN pattern is mu's (tests/test_gpu_int8_exact.py holds the same on the
      int8 route).
  (c) reversed: the edited set in reverse row order gives the edited pass's outputs reversed, bit for bit.
(b) and (c) are DESIGN.md's locality — a candidate's bits depend neither on its position nor on its neighbours — which
tests/test_gpu_properties.py asserts at C3 on the int8 route only.

Each case prints its worst error over its bar; the worst per template goes as JSON to the file GPBO_POSTERIOR_INSTANCE_REPORT names (if set)."""
import collections
import functools

import numpy as np
import pytest

import matern_family_truth as F
import test_gpu_posterior_refresh as RF
import test_gpu_sizes as SZ
from bayesianoptimization_amd.engine import F32
from conftest import elementwise_err, rel_err
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

DIMS = (3, 6, 11, 23, 47, 64)
KINDS = (F.RBF, F.MATERN25, F.MATERN15, F.MATERN05)
KNAME = RF.KNAME
NOISE = SZ.NOISE
F32_MU_BAR, F32_VAR_BAR = 1e-7, 2e-5          # tests/test_gpu_f32.py
FAR_SD_BAR = 1e-12                            # tests/test_gpu_int8_exact.py::test_non_finite_and_edge_candidates_end_to_end

Row = collections.namedtuple("Row", "N M f32 path fuse_ends part_chunks template")
#: name -> (N, M, fp32 mode, the path / fuse_ends / part_chunks plan_posterior gives the shape, the template that generates k* there)
ROWS = {
    "small": Row(130, 5, False, "Small", False, 0, "kstar_small_kernel<K>"),
    "fused256-1": Row(130, 257, False, "Fused256", True, 1, "posterior_kernel_v2<DP, K, 1>"),
    "fused256-2": Row(300, 257, False, "Fused256", False, 2, "posterior_kernel_v2<DP, K, 1>"),
    "fused512": Row(300, 9217, False, "Fused512", True, 1, "posterior_kernel_v2<DP, K, 1, 32, 16>"),
    "slab_f64": Row(520, 641, False, "SlabF64", False, 3, "kstar_gen_kernel<DP, K, SlabF64>"),
    "slab_i8": Row(2050, 257, False, "SlabI8", False, 17, "kstar_gen_kernel<DP, K, SlabI8>"),
    "slab_f32-16": Row(300, 257, True, "SlabF32", False, 2, "kstar_gen_kernel<DP, K, SlabF32>"),
    "slab_f32-32": Row(520, 641, True, "SlabF32", False, 2, "kstar_gen_kernel<DP, K, SlabF32>"),
}
#: (d, kind) outermost, the rows of one (d, kind) side by side: the references of equal N are then used back to back
CASES = [(r, d, k) for d in DIMS for k in KINDS for r in ROWS]
#: candidates the reference is computed for, per N: the largest M of the rows with that N
M_OF_N = {N: max(r.M for r in ROWS.values() if r.N == N) for N in {r.N for r in ROWS.values()}}

#: d = 3: the length-scale factor f (length scale = f sqrt(d) x the per-column spread) per (kind, N) where
#: test_gpu_posterior_refresh.length_scale's leaves kappa(K + 1e-6 I) above 5e6, the upper edge of test_gpu_sizes.KAPPA_WINDOW: the
#: largest of 0.2, 0.16, 0.12, 0.1, 0.08, 0.06, 0.05 that brings it under, found on the CPU
#: (tests/test_posterior_instance_cover_host.py asserts kappa for every (N, d, kind); the values are in docs/LAB_NOTEBOOK.md §29)
LS_F3 = {(F.RBF, 300): 0.08, (F.RBF, 520): 0.08, (F.RBF, 2050): 0.05, (F.MATERN25, 520): 0.2}

#: the edited rows of pass (b): row -> kind of edit; M = 5 has one of each family in five rows (row 0 stays clean)
EDITS_SMALL = {1: "nan-last", 2: "+inf-first", 3: "far", 4: "copy"}


def edits_of(M):
    if M == 5:
        return dict(EDITS_SMALL)
    return {1: "nan-last", 64: "nan-all", 65: "+inf-first", 130: "-inf-last", M - 2: "copy", M - 1: "far"}


def length_scale(kind, d, N):
    ls = RF.length_scale(kind, d, True, N)
    if d == 3 and (kind, N) in LS_F3:
        ls = LS_F3[(kind, N)] * np.sqrt(d) * np.geomspace(0.75, 1.33, d)
    return ls


def apply_edits(Xc, X, edits):
    """a copy of Xc with the rows of `edits` replaced"""
    Xe = Xc.copy()
    d = Xc.shape[1]
    for i, e in edits.items():
        if e == "nan-last":
            Xe[i, d - 1] = np.nan
        elif e == "nan-all":
            Xe[i] = np.nan
        elif e == "+inf-first":
            Xe[i, 0] = np.inf
        elif e == "-inf-last":
            Xe[i, d - 1] = -np.inf
        elif e == "copy":
            Xe[i] = X[-1]                      # training point N - 1: in the ragged last row chunk
        elif e == "far":
            Xe[i] = 1e3                        # every k* underflows to 0
        else:
            raise ValueError(e)
    return Xe


class Truth:
    """One (N, d, kind): data, length scales, the oracle's fit and its clean posterior over M_OF_N[N] candidates (left unchanged)."""

    def __init__(self, N, d, kind):
        self.N, self.d, self.kind = N, d, kind
        self.X, self.y, self.Xc = SZ.make_data(N, d, 31 * N + d + kind, M_OF_N[N])
        self.yn, self.ym, self.ys = O.normalize_targets(self.y)
        self.ls = length_scale(kind, d, N)
        self.gp = F.fit_fixed_theta(kind, self.X, self.yn, self.ls, NOISE, normalize_y=False)
        self.mu_o, self.sd_o = self.posterior(self.Xc)
        for a in (self.X, self.y, self.yn, self.Xc, self.ls, self.mu_o, self.sd_o):
            a.setflags(write=False)

    def posterior(self, Xc):
        """the oracle's (mu, sd) in the targets' units; non-finite candidates give what NumPy gives"""
        with np.errstate(all="ignore"):
            mu, sd = F.predict(self.gp, Xc)
        return self.ys * mu + self.ym, self.ys * sd

    def edited(self, M):
        """(edits, edited candidates, the oracle's mu / sd over them): the clean reference with the edited rows recomputed — six
        rows in a call of their own, so no BLAS blocking decides what a NaN's neighbours get"""
        edits = edits_of(M)
        Xe = apply_edits(self.Xc[:M], self.X, edits)
        rows = sorted(edits)
        mu, sd = self.mu_o[:M].copy(), self.sd_o[:M].copy()
        for i in rows:                          # one at a time: a candidate's reference must not depend on its neighbours either
            mu[i], sd[i] = (v[0] for v in self.posterior(Xe[i:i + 1]))
        return edits, Xe, mu, sd


@functools.lru_cache(maxsize=8)
def truth(N, d, kind):
    return Truth(N, d, kind)


#: worst error / bar per template
WORST = {}


def record(template, ratio):
    WORST[template] = max(WORST.get(template, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _posterior_instance_report():
    yield
    import json
    import os

    print("worst error / bar per template: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))
    out = os.environ.get("GPBO_POSTERIOR_INSTANCE_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(dict(sorted(WORST.items())), f, indent=1)


def check_clean(row, mu, sd, mu_o, sd_o, ys, what, kind):
    """pass (a) at the sibling files' bars; returns the worst error / bar"""
    if row.f32:
        e_mu, e_var = rel_err(mu, mu_o), float(np.max(np.abs(sd ** 2 - sd_o ** 2))) / ys ** 2
        print(f"{what}: f32 mu {e_mu:.2e} (bar {F32_MU_BAR:.0e}), var {e_var:.2e} (bar {F32_VAR_BAR:.0e})")
        assert e_mu < F32_MU_BAR and e_var < F32_VAR_BAR, f"{what}: mu {e_mu:.2e}, var {e_var:.2e}"
        return max(e_mu / F32_MU_BAR, e_var / F32_VAR_BAR)
    tol = RF.tol_of(kind)
    e_sd1, e_mu1 = elementwise_err(sd, sd_o, mu, mu_o, ys)
    print(f"{what}: mu {rel_err(mu, mu_o):.2e} sd {rel_err(sd, sd_o):.2e} (bar {tol:.0e}), per candidate sd {e_sd1:.2e} mu {e_mu1:.2e} (bar 1e-05)")
    return max(SZ.check_posterior(mu, sd, mu_o, sd_o, ys, what, tol), e_sd1 / 1e-5, e_mu1 / 1e-5)


@pytest.mark.parametrize("row,d,kind", CASES, ids=[f"{r}-d{d}-{KNAME[k]}" for r, d, k in CASES])
def test_posterior_instance(engine, row, d, kind):
    r = ROWS[row]
    t = truth(r.N, d, kind)
    M, ym, ys = r.M, t.ym, t.ys
    what = f"{row} N={r.N} M={M} d={d} {KNAME[kind]}"
    engine.fit(t.X, t.yn, kind, t.ls, NOISE, precision=F32 if r.f32 else 0)

    # (a) the clean pass against the oracle
    engine.set_candidates(t.Xc[:M])
    mu, sd = engine.posterior(0, ym, ys)
    worst = check_clean(r, mu, sd, t.mu_o[:M], t.sd_o[:M], ys, what, kind)

    # (b) the edited pass
    edits, Xe, mu_o, sd_o = t.edited(M)
    assert len(edits) <= 6
    engine.set_candidates(Xe)
    mu_e, sd_e = engine.posterior(0, ym, ys)
    bi, bv, _, _, vals = engine.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    nan_rows = {e: (bool(np.isnan(mu_e[i])), bool(np.isnan(sd_e[i])), bool(np.isnan(mu_o[i]))) for i, e in edits.items()}
    print(f"{what}: NaN (mu, sd, oracle) per edited row {nan_rows}")
    assert np.array_equal(np.isnan(mu_e), np.isnan(mu_o)), f"{what}: mu's NaN pattern is not the oracle's: {nan_rows}"
    assert np.array_equal(np.isnan(sd_e), np.isnan(sd_o)), f"{what}: sd's NaN pattern is not the oracle's: {nan_rows}"
    keep = np.ones(M, dtype=bool)
    keep[sorted(edits)] = False
    moved = np.flatnonzero(keep & ((mu_e != mu) | (sd_e != sd)))
    assert moved.size == 0, f"{what}: untouched rows {moved[:8]} changed bits next to the edited ones"
    far = next(i for i, e in edits.items() if e == "far")
    print(f"{what}: far row mu - y_mean {mu_e[far] - ym:.3e}, sd / y_std - 1 {sd_e[far] / ys - 1.0:.3e}")
    assert mu_e[far] == ym and abs(sd_e[far] - ys) <= FAR_SD_BAR * ys, what
    copy = next(i for i, e in edits.items() if e == "copy")
    assert np.isfinite(mu_e[copy]) and np.isfinite(sd_e[copy]) and sd_e[copy] >= 0.0, what
    if r.f32:
        e_copy = abs(sd_e[copy] ** 2 - sd_o[copy] ** 2) / ys ** 2 / F32_VAR_BAR
        assert e_copy < 1.0, f"{what}: the copy's variance {e_copy:.2e} of its bar"
    else:
        e_copy = max(elementwise_err(sd_e[[copy]], sd_o[[copy]], mu_e[[copy]], mu_o[[copy]], ys)) / 1e-5
        assert e_copy <= 1.0, f"{what}: the copy is {e_copy:.2e} of the per-candidate bar off the oracle"
    worst = max(worst, e_copy)
    assert bi == 1 and np.isnan(bv), f"{what}: arg-best {bi}, {bv}: not the first NaN"
    assert np.array_equal(np.isnan(vals), np.isnan(mu_e)), f"{what}: the acquisition's NaN pattern is not mu's"

    # (c) the edited set in reverse row order
    engine.set_candidates(np.ascontiguousarray(Xe[::-1]))
    mu_r, sd_r = engine.posterior(0, ym, ys)
    diff = np.flatnonzero(~((mu_r[::-1] == mu_e) | (np.isnan(mu_r[::-1]) & np.isnan(mu_e)))
                          | ~((sd_r[::-1] == sd_e) | (np.isnan(sd_r[::-1]) & np.isnan(sd_e))))
    assert np.array_equal(mu_r[::-1], mu_e, equal_nan=True) and np.array_equal(sd_r[::-1], sd_e, equal_nan=True), \
        f"{what}: rows {diff[:8]} of {diff.size} have other bits at the mirrored position"

    print(f"{what}: worst error / bar {worst:.2e}")
    record(r.template, worst)
