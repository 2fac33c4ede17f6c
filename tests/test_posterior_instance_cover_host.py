"""CPU: what tests/test_gpu_posterior_instances.py rests on, asserted here and not hoped for.  Its tables are imported, not copied.

Coverage.  Through pad_dim (tests/test_instance_cover_host.py restates it and pins it to csrc/gpbo_internal.h) the GPU file's table
reaches all 100 instances of the five k*-generating posterior templates — posterior_kernel_v2<DP, K, 1> (Fused256),
posterior_kernel_v2<DP, K, 1, 32, 16> (Fused512), kstar_gen_kernel<DP, K, SlabF64 | SlabI8 | SlabF32> — and through plan_posterior
(csrc/posterior_plan.h compiled for the host, tests/test_posterior_plan_host.build_plan) with the product's GEMV limit
(test_gpu_sizes.small_batch_limit, pinned here to csrc/posterior_small.hip: the rule's lines cut out of the file and compiled) each
(NP, M, precision) takes the named path with the named fuse_ends and part_chunks.

Instances that no earlier test file launched (NEVER_BEFORE, asserted), from those files' own case tables walked through the same
plan: tests/test_gpu_width.py (POST_CASES, its fp32 test), test_gpu_matern_family.py (POST_PATHS x KINDS, its fp32 test),
test_gpu_f32.py, test_gpu_sizes.py (FIT_CASES at M = 300, POST_CASES, F32_CASES), test_gpu_posterior_refresh.py (CASES and its fp32 slot),
test_gpu_instances.py (the full passes of its KG and refresh cases), the golden workloads (bayesianoptimization_amd/workloads.py:
test_gpu_golden.py, test_gpu_f32.py) and, as literal rows, the int8 files that have no table (test_gpu_int8_exact.py:
d = 2, 8, 16 with Matern-2.5 and RBF).  DP x kind, "-" never launched, "x" launched (kinds in the order RBF, nu = 2.5, 1.5, 0.5):

    template    DP 4    DP 8    DP 16   DP 32   DP 64     never
    Fused256    xxxx    xxxx    xxxx    xxxx    xxxx       0
    Fused512    xx--    xxxx    xx--    xx--    xx--       8
    SlabF64     xx--    xxxx    xx--    xx--    xx--       8
    SlabI8      xx--    xx--    xxxx    xx--    xx--       8
    SlabF32     -x--    xxxx    -x--    xx--    xx--      10
                                                          34 of 100

(Fused256 is complete only through NP = 64 ... 192, one row chunk: with two chunks — three launches — it had met nu = 1.5 / 0.5 at no
width.  The fp32 holes among Matern-2.5 / RBF: RBF at DP 4 and DP 16.)  After this file: 0 of 100.

Conditions on the reference alone: kappa(K + 1e-6 I) <= 5e6 (the upper edge of test_gpu_sizes.KAPPA_WINDOW) for every (N, d, kind);
the oracle's non-finite pattern — a NaN coordinate gives NaN for every kind, a +-inf coordinate NaN for nu = 2.5 / 1.5 and exactly
(0, 1) in normalised units for RBF / nu = 0.5, the far row exactly (0, 1); at most 6 rows of a case are edited.

Discrimination, in the manner of tests/test_width_discrimination_host.py and with test_instance_cover_host's mutants: the last live
column dropped from the distance, the first padding column read as live (not at d = 64), a neighbouring kind's formula — applied to the
NumPy truth of what ONE generator instance computes (k*; the model K, L, alpha stays the correct one: the fit kernels made it) for
every (N, d, kind), over the candidates of the smallest row of that N.  Each must move mu AND sd by at least 100x
test_gpu_posterior_refresh.tol_of(kind), and on the fp32 rows' N mu by 100x its 1e-7 (the generator under test writes both the slab and
the means); the fp32 variance's move over its bar 2e-5 is printed, its smallest value per mutant too (docs/LAB_NOTEBOOK.md §29 records
them: 5.5e2 at the least), and held to the same 100x.  NumPy only: no broken kernel is ever run."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.linalg import eigvalsh, solve_triangular

import matern_family_truth as F
import test_gpu_f32 as TF
import test_gpu_instances as GI
import test_gpu_matern_family as MF
import test_gpu_posterior_instances as PI
import test_gpu_posterior_refresh as RF
import test_gpu_sizes as SZ
import test_gpu_width as GW
import test_instance_cover_host as IC
import test_posterior_plan_host as PL
from bayesianoptimization_amd import workloads as W
from conftest import ROOT, rel_err
from oracle import gp_oracle as O

CSRC = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")
TIERS = IC.TIERS
pad_dim = IC.pad_dim
FIVE = {"Fused256": "posterior_kernel_v2<DP, K, 1>", "Fused512": "posterior_kernel_v2<DP, K, 1, 32, 16>",
        "SlabF64": "kstar_gen_kernel<DP, K, SlabF64>", "SlabI8": "kstar_gen_kernel<DP, K, SlabI8>",
        "SlabF32": "kstar_gen_kernel<DP, K, SlabF32>"}
#: the docstring's table: path -> tier -> the kinds (RBF, nu = 2.5, 1.5, 0.5) no earlier file launched
NEVER_BEFORE = {
    "Fused256": {},
    "Fused512": {t: (F.MATERN15, F.MATERN05) for t in (4, 16, 32, 64)},
    "SlabF64": {t: (F.MATERN15, F.MATERN05) for t in (4, 16, 32, 64)},
    "SlabI8": {t: (F.MATERN15, F.MATERN05) for t in (4, 8, 32, 64)},
    "SlabF32": {4: (F.RBF, F.MATERN15, F.MATERN05), 16: (F.RBF, F.MATERN15, F.MATERN05), 32: (F.MATERN15, F.MATERN05),
                64: (F.MATERN15, F.MATERN05)},
}


def np_of(N):
    return (N + 63) // 64 * 64


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return PL.build_plan(str(tmp_path_factory.mktemp("plan")))


def path_of(plan, N, M, f32=False):
    return plan(np_of(N), M, f32, SZ.small_batch_limit(np_of(N)))


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
def test_small_batch_limit_is_the_sources(tmp_path):
    """the product rule of posterior_small.hip's small_batch_limit (the debug build's GPBO_SMALL_MAX override in front of it is not
    the product's rule), compiled for the host as it stands"""
    body = re.search(r"^int small_batch_limit\(int64_t NP\) \{\n(?:[^\n]*\n)*?((?:  if \(NP <= \d+\) return \d+;\n)+  return \d+;)\n\}$",
                     open(os.path.join(CSRC, "posterior_small.hip")).read(), re.M)
    assert body, "small_batch_limit is no longer where this test reads it"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, so = str(tmp_path / "limit.cpp"), str(tmp_path / "liblimit.so")
    with open(src, "w") as f:
        f.write('#include <cstdint>\nextern "C" int limit(int64_t NP) {\n' + body.group(1) + "\n}\n")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.limit.argtypes = [ctypes.c_int64]
    nps = list(range(64, 20480, 64))
    assert [L.limit(n) for n in nps] == [SZ.small_batch_limit(n) for n in nps]


def test_the_kind_constants_are_one_numbering():
    assert (O.RBF, O.MATERN25) == (F.RBF, F.MATERN25) and PI.KINDS == GI.KINDS and PI.DIMS == GI.DIMS


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
def test_every_row_takes_its_path(plan):
    for name, r in PI.ROWS.items():
        got = path_of(plan, r.N, r.M, r.f32)
        assert got[:3] == (r.path, r.fuse_ends, r.part_chunks), (name, got)
        assert r.template == FIVE.get(r.path, "kstar_small_kernel<K>"), name
        NP = np_of(r.N)
        assert r.N % 64 and NP % 256, f"{name}: N is off the 64-row padding and the last 256-row chunk is ragged"
        if r.path != "Small":
            assert r.M % 64 and r.M % 128 and r.M > 130, name
            assert r.M > SZ.small_batch_limit(NP)
    assert np_of(PI.ROWS["fused256-2"].N) - 256 == 64 and PI.ROWS["fused256-2"].N - 256 == 44      # the second chunk's live rows
    assert (PI.ROWS["fused512"].M + 127) // 128 * 128 == 9344
    assert np_of(PI.ROWS["slab_f32-16"].N) < 512 <= np_of(PI.ROWS["slab_f32-32"].N)               # 16x16 | 32x32 MFMAs
    assert PI.ROWS["slab_i8"].M > 128 and np_of(PI.ROWS["slab_i8"].N) // 256 + 1 == 9
    # every N's rows share one reference; the rows of one (d, kind) are neighbours in the case list
    assert set(PI.M_OF_N) == {130, 300, 520, 2050} and PI.M_OF_N[300] == 9217
    assert len(PI.CASES) == 192 and len(set(PI.CASES)) == 192


def test_the_case_table_reaches_all_100_instances():
    assert {pad_dim(d) for d in PI.DIMS} == set(TIERS) and set(PI.KINDS) == {F.RBF, F.MATERN25, F.MATERN15, F.MATERN05}
    assert sorted(d for d in PI.DIMS if d < pad_dim(d)) == [3, 6, 11, 23, 47] and 64 in PI.DIMS
    reached = {(PI.ROWS[r].template, pad_dim(d), k) for r, d, k in PI.CASES if PI.ROWS[r].path in FIVE}
    assert reached == {(t, dp, k) for t in FIVE.values() for dp in TIERS for k in PI.KINDS} and len(reached) == 100
    # Fused256 with one row chunk AND with two, at every instance
    for row in ("fused256-1", "fused256-2"):
        assert {(pad_dim(d), k) for r, d, k in PI.CASES if r == row} == {(dp, k) for dp in TIERS for k in PI.KINDS}


def earlier_files_instances(plan):
    """{(path, DP, kind)} of the full posterior passes of the earlier files' case tables (the docstring names them)"""
    seen = set()

    def add(N, M, d, kind, f32=False):
        seen.add((path_of(plan, N, M, f32)[0], pad_dim(d), int(kind)))

    for p, d, k in GW.POST_CASES:
        add(*GW.POST_PATHS[p], d, k)
    for N in (300, 1000):                                    # test_f32_posterior_at_every_width, its kernel rule restated
        for d in GW.SLOW_WIDTHS:
            add(N, 5003, d, O.MATERN25 if d in (5, 33) else O.RBF, True)
    for k in MF.KINDS:
        for N, d, M in MF.POST_PATHS.values():
            add(N, M, d, k)
        for N in (200, 600):                                 # test_f32_mode_within_1e4_of_the_range_with_the_exact_arg_best
            add(N, 3000, 5, k, True)
    for N, d, M, k, _ in TF.test_f32_posterior_against_oracle.pytestmark[0].args[1]:
        add(N, M, d, k, True)
        add(N, M, d, k)                                      # "and the fp64 mode on the same context is untouched"
    for N, k, d, _ in SZ.FIT_CASES:
        add(N, 300, d, k)
    for NP, M in SZ.POST_CASES:
        k, d, _ = SZ._post_shape(NP)
        add(NP - 7, M, d, k)
    for NP, M in SZ.F32_CASES:
        k, d, _ = SZ._post_shape(NP)
        add(NP - 7, M, d, k, True)
    for s, k in RF.CASES:
        N0, d, M, rows, _ = RF.SHAPES[s]
        add(N0, M, d, k)
        add(N0 + rows, M, d, k)
    add(300, 5000, 5, F.MATERN25, True)                      # test_f32_slot_keeps_the_f32_bars
    for d, k, _ in GI.KG_CASES:
        add(GI.KG_N, GI.M, d, k)
    for d, k in GI.REFRESH_CASES:
        add(GI.REFRESH_N0, GI.REFRESH_M, d, k)
        add(GI.REFRESH_N0 + GI.REFRESH_ROWS, GI.REFRESH_M, d, k)
    for w in W.ALL.values():
        add(w.N, w.M, w.d, w.kernel)
    for name in ("C2", "C5S", "C5"):                         # test_f32_against_reference_goldens
        add(W.ALL[name].N, W.ALL[name].M, W.ALL[name].d, W.ALL[name].kernel, True)
    for d in (2, 8, 16):                                     # test_gpu_int8_exact.py: N = 2100, M = 3000
        for k in (F.MATERN25, F.RBF):
            add(2100, 3000, d, k)
    return seen


def test_the_instances_no_earlier_file_launched(plan):
    seen = earlier_files_instances(plan)
    never = {p: {} for p in FIVE}
    for p in FIVE:
        for t in TIERS:
            missing = tuple(k for k in PI.KINDS if (p, t, k) not in seen)
            if missing:
                never[p][t] = missing
    print({p: {t: [PI.KNAME[k] for k in ks] for t, ks in v.items()} for p, v in never.items()})
    assert never == NEVER_BEFORE
    assert sum(len(ks) for v in never.values() for ks in v.values()) == 34
    # ... and Fused256 with two row chunks had met nu = 1.5 / 0.5 nowhere: every earlier launch of them has NP <= 256
    two_chunk = set()
    for k in MF.KINDS:
        for N, d, M in MF.POST_PATHS.values():
            got = path_of(plan, N, M)
            if got[0] == "Fused256" and got[2] > 1:
                two_chunk.add((pad_dim(d), k))
    assert not two_chunk


# ---- conditions on the reference alone -----------------------------------------------------------------------------------------------
NDK = [(N, d, k) for d in PI.DIMS for k in PI.KINDS for N in sorted(PI.M_OF_N)]
NDK_IDS = [f"N{N}-d{d}-{PI.KNAME[k]}" for N, d, k in NDK]


def kappa_of(t):
    K = t.gp.L @ t.gp.L.T
    n = K.shape[0]
    return float(eigvalsh(K, subset_by_index=[n - 1, n - 1])[0] / eigvalsh(K, subset_by_index=[0, 0])[0])


def test_the_d3_factors_are_the_table():
    """LS_F3 holds exactly the (kind, N) whose sibling factor leaves kappa above the window, each shorter than the sibling's"""
    for (kind, N), f in PI.LS_F3.items():
        assert f < RF.length_scale(kind, 3, True, N)[0] / (0.75 * np.sqrt(3))
        assert np.array_equal(PI.length_scale(kind, 3, N), f * np.sqrt(3) * np.geomspace(0.75, 1.33, 3))
    for d in PI.DIMS[1:]:
        assert np.array_equal(PI.length_scale(F.RBF, d, 300), RF.length_scale(F.RBF, d, True, 300))
    for kind in PI.KINDS:
        for N in PI.M_OF_N:
            ls = PI.length_scale(kind, 3, N)
            assert np.unique(ls).shape == (3,)


@pytest.mark.parametrize("N,d,kind", NDK, ids=NDK_IDS)
def test_reference_conditions_and_discrimination(N, d, kind):
    t = PI.truth(N, d, kind)
    what = f"N={N} d={d} {PI.KNAME[kind]}"
    kap = kappa_of(t)
    print(f"{what}: f = {t.ls[0] / (0.75 * np.sqrt(d)):.3f}, kappa {kap:.2e}")
    assert kap <= SZ.KAPPA_WINDOW[1], f"{what}: kappa {kap:.2e} above {SZ.KAPPA_WINDOW[1]:.0e}: a shorter factor in LS_F3"

    # the oracle's non-finite pattern, per row that shares this reference
    rows = [r for r in PI.ROWS.values() if r.N == N]
    for r in rows:
        edits, Xe, mu, sd = t.edited(r.M)
        assert len(edits) <= 6 and r.M - len(edits) >= (1 if r.M == 5 else r.M - 6)
        assert sorted(edits.values()) == sorted(PI.edits_of(r.M).values()) and min(edits) == 1      # the first NaN is row 1
        untouched = np.ones(r.M, dtype=bool)
        untouched[sorted(edits)] = False
        assert np.array_equal(mu[untouched], t.mu_o[:r.M][untouched]) and np.isfinite(mu[untouched]).all()
        assert np.array_equal(Xe[untouched], t.Xc[:r.M][untouched])
        for i, e in edits.items():
            mu_n, sd_n = (mu[i] - t.ym) / t.ys, sd[i] / t.ys
            if e.startswith("nan") or ("inf" in e and kind in (F.MATERN25, F.MATERN15)):
                assert np.isnan(mu[i]) and np.isnan(sd[i]), (what, e)
            elif "inf" in e or e == "far":
                assert mu_n == 0.0 and sd_n == 1.0 and mu[i] == t.ym and sd[i] == t.ys, (what, e, mu_n, sd_n)
            else:
                assert e == "copy" and np.isfinite(mu[i]) and 0.0 <= sd_n < 0.05, (what, e, sd_n)
                assert np.array_equal(Xe[i], t.X[N - 1]) and N - 1 >= (np_of(N) - 1) // 256 * 256      # in the last row chunk
    assert np.isnan(mu[1])

    # discrimination, over the candidates of the smallest template row of this N
    M = min(r.M for r in rows if r.path in FIVE)
    Xc = t.Xc[:M]

    def posterior(m):
        Kt = IC.kstar(m, kind, Xc, t.X, t.ls)
        V = solve_triangular(t.gp.L, Kt.T, lower=True, check_finite=False)
        var = np.maximum(1.0 - np.einsum("ij,ij->j", V, V), 0.0)
        return t.ys * (Kt @ t.gp.alpha) + t.ym, t.ys * np.sqrt(var)

    mu0, sd0 = posterior(None)
    assert rel_err(mu0, t.mu_o[:M]) <= 1e-12 and rel_err(sd0, t.sd_o[:M]) <= 1e-9            # the restatement is the reference's
    tol = RF.tol_of(kind)
    f32 = any(r.f32 for r in rows)
    for m in IC.mutants(d, kind):
        mu, sd = posterior(m)
        IC.far(rel_err(mu, t.mu_o[:M]), tol, f"{what} {m}: mu")
        IC.far(rel_err(sd, t.sd_o[:M]), tol, f"{what} {m}: sd")
        if f32:
            IC.far(rel_err(mu, t.mu_o[:M]), PI.F32_MU_BAR, f"{what} {m}: fp32 mu")
            ratio = float(np.max(np.abs(sd ** 2 - t.sd_o[:M] ** 2))) / t.ys ** 2 / PI.F32_VAR_BAR
            print(f"{what} {m}: fp32 variance moves {ratio:.2e} x its bar")
            name = m if isinstance(m, str) else "kind"
            VAR_RATIO[name] = min(VAR_RATIO.get(name, np.inf), ratio)
            IC.far(ratio * PI.F32_VAR_BAR, PI.F32_VAR_BAR, f"{what} {m}: fp32 variance")


#: the smallest fp32 variance move / bar per mutant over the fp32 rows' (N, d, kind), printed at the end of the module
VAR_RATIO = {}


@pytest.fixture(scope="module", autouse=True)
def _variance_ratios():
    yield
    print("smallest fp32 variance move / bar per mutant: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(VAR_RATIO.items())))
