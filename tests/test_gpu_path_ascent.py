"""GPU (-m gpu): gpbo_ascend_paths — posterior function draws climbed from their starts to local maximisers in one launch — against
tests/paths_ascent_truth.py, and suggest_thompson(refine=K) on the real engine.

Parity of one evaluation (max_iter = 0, explicit starts).  Value error as tests/test_gpu_sample_paths.py measures it,
max |f - f_ref| / (y_std max(1, max |f_ref,n|)); gradient error max |g - g_ref| / (y_std max(1, max |g_ref,n|)), the references in
normalised-target units.  Tiny cases (N <= 65, F <= 65): the reference is the 50-digit truth, the bar max(1e-9, 8 x the fp64
restatement's own error against it).  Other cases: the reference is the fp64 restatement, the bar max(1e-9, 8 x the spread between
its two summation routes).  1e-9 and the 8 are tests/test_gpu_sample_paths.py's rule.  The shapes are the edges of the kernel: the
per-thread stride of 256 on both sides for points and features, all three fit tiers, padded dimensions up to 64, starts on a box
face, on a box corner, outside the box and (nu = 0.5) exactly on a training point.

Ascent: per run x inside the box, f_out >= the start's value from the max_iter = 0 call (the same arithmetic, a monotone optimiser:
exact), f_out the truth's value at x_out, status 0 only where the truth's projected gradient is below tolerance; on a smooth case
the device's best over the starts is SciPy's (L-BFGS-B, checked against TNC on the truth alone) or better."""
import functools

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import paths_ascent_truth as T
import paths_truth as P
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_thompson
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.engine import F32, GpEngine, GroupEngine
from bayesianoptimization_amd.thompson import spectral_draw
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

KNAME = {F.RBF: "rbf", F.MATERN25: "matern25", F.MATERN15: "matern15", F.MATERN05: "matern05"}
NOISE = 1e-4
Y_MEAN, Y_STD = 3.5, 0.4
BAR, MARGIN, GAP_FLOOR = 1e-9, 8.0, 1e-6
PGTOL = 1e-5
LO, HI = 0.1, 0.9

#: name -> (N, F, d, S, K, kind, one length scale per dimension, reference)
CASES = {
    "n1-f1-d1-s1-k1": (1, 1, 1, 1, 1, F.RBF, False, "mp"),
    "n63-f65-d2-s2-k3": (63, 65, 2, 2, 3, F.MATERN25, True, "mp"),
    "n64-f64-d5-s5-k8": (64, 64, 5, 5, 8, F.MATERN15, True, "mp"),
    "n65-f63-d1-s16-k1": (65, 63, 1, 16, 1, F.MATERN05, False, "mp"),
    "n255-f257-d17-s16-k2": (255, 257, 17, 16, 2, F.RBF, True, "fp64"),
    "n256-f255-d33-s5-k8": (256, 255, 33, 5, 8, F.MATERN25, False, "fp64"),
    "n257-f256-d64-s2-k3": (257, 256, 64, 2, 3, F.MATERN15, True, "fp64"),
    "n800-f1000-d7-s16-k8": (800, 1000, 7, 16, 8, F.MATERN05, True, "fp64"),
}
ASCENT_CASES = [n for n in CASES if CASES[n][0] >= 63]


def length_scale(d, per_dim):
    s = 0.5 * np.sqrt(d)
    return s * np.geomspace(0.75, 1.33, d) if per_dim else np.array([s])


def err_f(f, ref):
    ref_n = (ref - Y_MEAN) / Y_STD
    return float(np.max(np.abs(f - ref)) / (Y_STD * max(1.0, float(np.max(np.abs(ref_n))))))


def err_g(g, ref):
    return float(np.max(np.abs(g - ref)) / (Y_STD * max(1.0, float(np.max(np.abs(ref / Y_STD))))))


class Case:
    """Data, draws, starts and box of one case (computed once, shared, never changed)."""

    def __init__(self, N, Fn, d, S, K, kind, per_dim, reference, amplitude=1.0, white=0.0, seed=0, smooth=False):
        self.N, self.F, self.d, self.S, self.K, self.kind, self.reference = N, Fn, d, S, K, kind, reference
        self.amplitude, self.white = amplitude, white
        self.X, y = F.data(N, d, seed=seed + 17 * N + d)
        self.yn = (y - y.mean()) / y.std() if N > 1 else np.array([0.3])
        self.ls = length_scale(d, per_dim)
        rs = np.random.RandomState(2000 + seed + N + Fn + S * K)
        self.omega, self.phase = spectral_draw(kind, Fn, d, rs)
        self.w = rs.standard_normal((S, Fn))
        self.eps = rs.standard_normal((S, N)) * np.sqrt(NOISE + white)
        self.eta = (NOISE + white) / amplitude
        self.lo, self.hi = np.full(d, LO), np.full(d, HI)
        starts = rs.uniform(LO, HI, size=(S * K, d))
        if not smooth:
            starts[0, 0] = LO                                              # on a face
            if S * K > 1:
                starts[1] = np.where(rs.uniform(size=d) < 0.5, LO, HI)     # on a corner
            if S * K > 2:
                inside = np.flatnonzero(((self.X >= LO) & (self.X <= HI)).all(axis=1))
                if kind == F.MATERN05 and inside.size:
                    starts[2] = self.X[inside[0]]                          # exactly on a training point
                else:
                    starts[2, -1] = HI + 0.5                               # outside: clipped onto the face
        self.starts = starts.reshape(S, K, d)
        self.clipped = np.clip(self.starts, self.lo, self.hi)
        self.what = f"N={N} F={Fn} d={d} S={S} K={K} {KNAME[kind]}"

    def truth_args(self):
        return (self.kind, self.X, self.yn, self.ls, self.eta, self.omega, self.phase, self.w, self.eps)

    def fp64(self, Xq, route="cho", paths=None):
        return T.path_value_grad(*self.truth_args(), Xq, Y_MEAN, Y_STD, amplitude=self.amplitude, route=route, paths=paths)

    def references(self, Xq):
        """(f_ref, g_ref, bar_f, bar_g, own_f, own_g) at the points Xq (S, K, d)"""
        f64, g64 = self.fp64(Xq)
        if self.reference == "mp":
            if not hasattr(self, "_mp"):
                self._mp = T.MpPaths(*self.truth_args(), Y_MEAN, Y_STD, amplitude=self.amplitude)
            f_ref, g_ref = T.path_value_grad_mp(*self.truth_args(), Xq, Y_MEAN, Y_STD, amplitude=self.amplitude, model=self._mp)
            own_f, own_g = err_f(f64, f_ref), err_g(g64, g_ref)
        else:
            f_ref, g_ref = f64, g64
            f2, g2 = self.fp64(Xq, route="winv")
            own_f, own_g = err_f(f2, f_ref), err_g(g2, g_ref)
        return f_ref, g_ref, max(BAR, MARGIN * own_f), max(BAR, MARGIN * own_g), own_f, own_g

    def fit(self, eng, precision=0):
        scaled = {} if (self.amplitude, self.white) == (1.0, 0.0) else {"amplitude": self.amplitude, "white": self.white}
        eng.fit(self.X, self.yn, self.kind, self.ls, NOISE, precision=precision, **scaled)

    def ascend(self, eng, **kw):
        kw.setdefault("starts", self.starts)
        return eng.ascend_paths(self.omega, self.phase, self.w, self.eps, self.lo, self.hi, y_mean=Y_MEAN, y_std=Y_STD, **kw)


@functools.lru_cache(maxsize=None)
def case_of(name):
    c = Case(*CASES[name])
    c.ref = c.references(c.clipped)
    return c


def check_evaluation(c, out, ref):
    f_ref, g_ref, bar_f, bar_g, own_f, own_g = ref
    assert out["x"].shape == (c.S, c.K, c.d) and out["f"].shape == (c.S, c.K) and out["g"].shape == (c.S, c.K, c.d)
    assert np.array_equal(out["x"], c.clipped), "max_iter = 0: x_out is the clipped start"
    ef, eg = err_f(out["f"], f_ref), err_g(out["g"], g_ref)
    print(f"{c.what}: value error {ef:.2e} (bar {bar_f:.2e}, the reference's own {own_f:.2e}); "
          f"gradient error {eg:.2e} (bar {bar_g:.2e}, own {own_g:.2e})")
    assert ef <= bar_f, f"{c.what}: value error {ef:.2e} over its bar {bar_f:.2e}"
    assert eg <= bar_g, f"{c.what}: gradient error {eg:.2e} over its bar {bar_g:.2e}"
    assert (out["n_eval"] == 1).all() and (out["start_idx"] == -1).all() and out["best_idx"] is None
    pg = T.projected_gradient_norm(out["x"], out["g"], c.lo, c.hi)
    assert np.array_equal(out["status"], np.where(pg <= PGTOL, 0, 2))


# ---- 1. one evaluation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_evaluation_parity(engine, name):
    c = case_of(name)
    c.fit(engine)
    check_evaluation(c, c.ascend(engine, max_iter=0, return_gradient=True), c.ref)


@functools.lru_cache(maxsize=None)
def mid_case():
    c = Case(130, 64, 5, 5, 3, F.MATERN25, True, "fp64")
    c.ref = c.references(c.clipped)
    return c


def test_scaled_slot(engine):
    c = Case(130, 64, 5, 5, 3, F.MATERN25, True, "fp64", amplitude=2.5, white=1e-3)
    ref = c.references(c.clipped)
    c.fit(engine)
    check_evaluation(c, c.ascend(engine, max_iter=0, return_gradient=True), ref)
    unit = T.path_value_grad(*c.truth_args(), c.clipped, Y_MEAN, Y_STD, amplitude=1.0)[0]
    assert err_f(unit, ref[0]) > 1e-3          # the amplitude is in the prior draw: the unit model's values differ


def test_f32_slot_gives_the_fp64_bits(engine):
    c = mid_case()
    c.fit(engine)
    a = c.ascend(engine, return_gradient=True)
    c.fit(engine, precision=F32)
    b = c.ascend(engine, return_gradient=True)
    check_evaluation(c, c.ascend(engine, max_iter=0, return_gradient=True), c.ref)
    for key in ("x", "f", "g", "status", "n_eval"):
        assert np.array_equal(a[key], b[key]), key


def test_after_fit_append(engine):
    N0, rows = 130, 3
    c = Case(N0 + rows, 64, 5, 5, 3, F.MATERN15, True, "fp64")
    ref = c.references(c.clipped)
    engine.fit(c.X[:N0], c.yn[:N0] * 1.1 - 0.05, c.kind, c.ls, NOISE)      # other targets before the append
    engine.fit_append(c.X[N0:], c.yn)
    check_evaluation(c, c.ascend(engine, max_iter=0, return_gradient=True), ref)


# ---- 2. the ascent ----------------------------------------------------------------------------------------------------------------
def check_ascent(c, eng):
    start = c.ascend(eng, max_iter=0)
    out = c.ascend(eng, return_gradient=True)
    assert (out["x"] >= c.lo).all() and (out["x"] <= c.hi).all()
    assert (out["f"] >= start["f"]).all(), "a run ended below its start"
    f_ref, g_ref, bar_f, bar_g, own_f, own_g = c.references(out["x"])
    ef, eg = err_f(out["f"], f_ref), err_g(out["g"], g_ref)
    gain = (out["f"] - start["f"]) / Y_STD
    print(f"{c.what}: at x_out value error {ef:.2e} (bar {bar_f:.2e}), gradient error {eg:.2e} (bar {bar_g:.2e}); status counts "
          f"{np.bincount(out['status'].ravel(), minlength=4).tolist()}, evaluations {out['n_eval'].min()}..{out['n_eval'].max()}, "
          f"mean gain {gain.mean():.3f} y_std")
    assert ef <= bar_f and eg <= bar_g
    assert set(np.unique(out["status"])) <= {0, 1, 2, 3}
    pg = T.projected_gradient_norm(out["x"], g_ref, c.lo, c.hi)
    slack = PGTOL + bar_g * Y_STD * max(1.0, float(np.max(np.abs(g_ref / Y_STD))))
    assert (pg[out["status"] == 0] <= slack).all(), "status 0 where the truth's projected gradient is not below tolerance"
    assert np.array_equal(out["winner"], np.argmax(out["f"], axis=1)) and np.array_equal(out["f_best"], out["f"].max(axis=1))
    cut = c.ascend(eng, max_iter=3)
    assert np.isin(cut["status"], (0, 1, 2)).all() and (cut["n_eval"] <= 4 * 3 + 64).all() and (cut["f"] >= start["f"]).all()
    return out


@pytest.mark.parametrize("name", ASCENT_CASES)
def test_ascent(engine, name):
    c = case_of(name)
    c.fit(engine)
    check_ascent(c, engine)


SMOOTH_SEED = 1


@functools.lru_cache(maxsize=None)
def smooth_case():
    """RBF, l = 0.5 sqrt(d), F = 64, d = 5: smooth enough that two SciPy methods agree on every path's best-over-starts."""
    c = Case(64, 64, 5, 4, 4, F.RBF, False, "fp64", seed=SMOOTH_SEED, smooth=True)
    V = P.path_weights(*c.truth_args())
    best = {}
    for method in ("L-BFGS-B", "TNC"):
        vals = []
        for s in range(c.S):
            def vg(p, s=s):
                fv, gv = T.path_value_grad(*c.truth_args(), p[None, None, :], Y_MEAN, Y_STD, V=V, paths=[s])
                return fv[0, 0], gv[0, 0]

            vals.append(T.scipy_ascent(vg, c.starts[s], c.lo, c.hi, method=method)[1].max())
        best[method] = np.array(vals)
    c.scipy_best = best
    return c


def test_smooth_case_finds_scipys_optimum_or_better(engine):
    c = smooth_case()
    a, b = c.scipy_best["L-BFGS-B"], c.scipy_best["TNC"]
    scale = np.maximum(np.abs(a), 1e-12)
    assert (np.abs(a - b) <= 1e-8 * scale).all(), f"the reference's two methods disagree ({a - b}): pick another seed"
    c.fit(engine)
    out = check_ascent(c, engine)
    assert not np.isin(out["status"], (2, 3)).any()
    print(f"{c.what}: device best - SciPy best per path {(out['f_best'] - a).tolist()}")
    assert (out["f_best"] >= a - 1e-8 * scale).all()


# ---- 3. resident starts -----------------------------------------------------------------------------------------------------------
def test_resident_starts(engine):
    c = mid_case()
    M, K = 257, 4
    Xc = np.random.RandomState(77).uniform(LO, HI, size=(M, c.d))
    c.fit(engine)
    engine.set_candidates(Xc)
    idx, val, values = engine.sample_paths(c.omega, c.phase, c.w, c.eps, y_mean=Y_MEAN, y_std=Y_STD, return_values=True)
    out = c.ascend(engine, starts=None, n_starts=K)
    assert np.array_equal(out["best_idx"], idx) and np.array_equal(out["best_val"], val)
    assert np.array_equal(out["start_idx"][:, 0], idx)
    truth = P.paths_cho(*c.truth_args(), Xc, Y_MEAN, Y_STD)
    order = np.argsort(-truth, axis=1, kind="stable")[:, :K + 1]
    top = np.take_along_axis(truth, order, axis=1)
    gaps = (top[:, :-1] - top[:, 1:]) / (truth.max(axis=1) - truth.min(axis=1))[:, None]
    assert gaps.min() >= GAP_FLOOR, f"the truth's neighbouring gaps {gaps.min():.2e}: pick another seed"
    assert np.array_equal(out["start_idx"], order[:, :K])
    # the runs start AT those candidates: the same bits as explicit starts
    again = c.ascend(engine, starts=Xc[out["start_idx"]])
    for key in ("x", "f", "status", "n_eval"):
        assert np.array_equal(out[key], again[key]), key
    start = c.ascend(engine, starts=Xc[out["start_idx"]], max_iter=0)
    assert np.array_equal(start["f"][:, 0], val) or err_f(start["f"][:, 0], val) <= c.ref[2]      # the candidate pass's value
    assert (out["f_best"] >= start["f"][:, 0]).all()
    off = c.ascend(engine, starts=None, n_starts=K, index_offset=10**10)
    assert np.array_equal(off["start_idx"], out["start_idx"] + 10**10) and np.array_equal(off["best_idx"], idx + 10**10)
    assert np.array_equal(off["x"], out["x"])
    engine.set_candidates(Xc[:3])
    with pytest.raises(ValueError, match="n_starts"):
        c.ascend(engine, starts=None, n_starts=4)
    assert c.ascend(engine, starts=None, n_starts=3)["start_idx"].shape == (c.S, 3)


# ---- 4. exact properties ------------------------------------------------------------------------------------------------------------
def test_bitwise_repeatable_and_alone_equals_in_the_full_grid(engine):
    c = Case(130, 65, 5, 16, 8, F.MATERN25, True, "fp64")
    c.fit(engine)
    a = c.ascend(engine, return_gradient=True)
    b = c.ascend(engine, return_gradient=True)
    keys = ("x", "f", "g", "status", "n_eval")
    for key in keys:
        assert np.array_equal(a[key], b[key]), key
    for s, k in ((0, 0), (15, 7), (7, 3), (3, 5)):
        one = engine.ascend_paths(c.omega, c.phase, c.w[s:s + 1], c.eps[s:s + 1], c.lo, c.hi, starts=c.starts[s:s + 1, k:k + 1],
                                  y_mean=Y_MEAN, y_std=Y_STD, return_gradient=True)
        for key in keys:
            assert np.array_equal(one[key][0, 0], a[key][s, k]), f"run ({s}, {k}) alone differs from the same run among 128: {key}"


# ---- 5. a reader ----------------------------------------------------------------------------------------------------------------------
def test_reader_only(engine):
    eng = engine
    c = mid_case()
    M = 257
    Xc = np.random.RandomState(78).uniform(size=(M, c.d))

    def fit():
        c.fit(eng)
        eng.set_candidates(Xc)

    fit()
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    eng.take_negative_variance_flag()
    before = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    c.ascend(eng, starts=None, n_starts=4)
    c.ascend(eng)                                                         # explicit starts
    after = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)      # still answers, from the posterior before the calls
    assert before[0] == after[0] and before[1] == after[1] and np.array_equal(before[2], after[2])
    assert np.array_equal(before[3], after[3]) and np.array_equal(before[4], after[4])
    assert np.array_equal(eng.get_candidate_rows(np.arange(M), c.d), Xc)
    assert eng.take_negative_variance_flag() is False
    x_new = np.random.RandomState(5).uniform(size=(2, c.d))
    yn2 = np.concatenate([c.yn, [0.2, -0.4]])
    eps2 = np.hstack([c.eps, np.zeros((c.S, 2))])

    def arm():
        fit()
        eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
        eng.fit_append(x_new, yn2)

    arm()
    mu_a, sd_a, route_a = eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True)
    arm()
    eng.ascend_paths(c.omega, c.phase, c.w, eps2, c.lo, c.hi, n_starts=2, y_mean=Y_MEAN, y_std=Y_STD)
    eng.ascend_paths(c.omega, c.phase, c.w, eps2, c.lo, c.hi, starts=c.starts, y_mean=Y_MEAN, y_std=Y_STD)
    mu_b, sd_b, route_b = eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True)
    assert route_a == 1 and route_b == 1
    assert np.array_equal(mu_a, mu_b) and np.array_equal(sd_a, sd_b)
    assert np.array_equal(eng.get_candidate_rows(np.arange(M), c.d), Xc)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    eng = engine
    c = case_of("n63-f65-d2-s2-k3")
    c.fit(eng)
    eng.set_candidates(c.clipped.reshape(-1, c.d))
    kw = {"y_mean": Y_MEAN, "y_std": Y_STD}
    for n in (0, 9):
        with pytest.raises(ValueError, match="n_starts"):
            eng.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, c.hi, n_starts=n, **kw)
        with pytest.raises(ValueError, match="n_starts"):
            eng.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, c.hi, starts=np.zeros((c.S, n, c.d)), **kw)
    for n_paths in (0, 17):
        with pytest.raises(ValueError, match="n_paths"):
            eng.ascend_paths(c.omega, c.phase, np.zeros((n_paths, c.F)), np.zeros((n_paths, c.N)), c.lo, c.hi, n_starts=1, **kw)
    hi = c.hi.copy()
    hi[1] = c.lo[1]
    with pytest.raises(ValueError, match="box"):
        eng.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, hi, starts=c.starts, **kw)
    for bad in (np.inf, np.nan):
        hi = c.hi.copy()
        hi[0] = bad
        with pytest.raises(ValueError, match="box"):
            eng.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, hi, starts=c.starts, **kw)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="y_std"):
            eng.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, c.hi, starts=c.starts, y_std=bad)
    with pytest.raises(ValueError):       # shapes that do not fit the slot's model never reach the library
        eng.ascend_paths(c.omega, c.phase, c.w, c.eps[:, :-1], c.lo, c.hi, **kw)
    with pytest.raises(ValueError):
        eng.ascend_paths(c.omega[:, :1], c.phase, c.w, c.eps, c.lo, c.hi, **kw)
    with pytest.raises(ValueError):
        eng.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo[:1], c.hi, **kw)
    with pytest.raises(ValueError):
        eng.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, c.hi, starts=c.starts[:, :, :1], **kw)
    # NULL arguments, at the C boundary
    R = c.S * c.K
    bi, bv = np.empty(c.S, dtype=np.int64), np.empty(c.S)
    x, f, st, si = np.empty((R, c.d)), np.empty(R), np.zeros(R, dtype=np.int32), np.empty(R, dtype=np.int64)
    stp = st.ctypes.data_as(_lib._c_int_p)
    w, eps, starts = np.ascontiguousarray(c.w), np.ascontiguousarray(c.eps), np.ascontiguousarray(c.starts)

    def call(slot=0, omega=dptr(c.omega), phase=dptr(c.phase), weights=dptr(w), noise=dptr(eps), s=dptr(starts), lo=dptr(c.lo),
             hi=dptr(c.hi), best_idx=iptr(bi), best_val=dptr(bv), x_out=dptr(x), f_out=dptr(f), status=stp, start_idx=iptr(si),
             handle=None):
        return eng._lib.gpbo_ascend_paths(handle or eng._h, slot, Y_MEAN, Y_STD, c.S, c.F, omega, phase, weights, noise, c.K, s, lo, hi,
                                          -1, 0, best_idx, best_val, x_out, f_out, None, status, None, start_idx)

    assert call() == _lib.GPBO_OK and call(best_idx=None, best_val=None) == _lib.GPBO_OK      # g_out, n_eval_out and (with starts) best_* may be NULL
    for name in ("omega", "phase", "weights", "noise", "lo", "hi", "x_out", "f_out", "status", "start_idx"):
        assert call(**{name: None}) == _lib.ERR_INVALID, name
    assert call(s=None) == _lib.GPBO_OK
    assert call(s=None, best_idx=None) == _lib.ERR_INVALID and call(s=None, best_val=None) == _lib.ERR_INVALID
    # a slot that gpbo_lml left unfitted
    eng.fit(c.X, c.yn, c.kind, c.ls, NOISE, slot=3)
    eng.lml(c.X, c.yn, c.kind, c.ls, NOISE, slot=3)
    with pytest.raises(GpboError, match="not been fitted"):
        eng.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, c.hi, starts=c.starts, slot=3, **kw)
    assert call(slot=3) == _lib.ERR_STATE
    # a fit pending on the slot
    with eng.overlapped_fits():
        eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        assert call() == _lib.ERR_STATE
    # candidates of another d: only the resident form minds
    eng.set_candidates(np.random.RandomState(1).uniform(size=(10, c.d + 1)))
    with pytest.raises(GpboError, match="dimension"):
        eng.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, c.hi, n_starts=2, **kw)
    assert call() == _lib.GPBO_OK
    fresh = GpEngine(0)
    try:
        with pytest.raises(GpboError, match="not been fitted"):
            fresh.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, c.hi, starts=c.starts, slot=5, **kw)
        assert call(slot=5, handle=fresh._h) == _lib.ERR_STATE
        fresh.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        with pytest.raises(GpboError, match="no candidates"):
            fresh.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, c.hi, n_starts=2, **kw)
        assert fresh.ascend_paths(c.omega, c.phase, c.w, c.eps, c.lo, c.hi, starts=c.starts, **kw)["x"].shape == (c.S, c.K, c.d)
    finally:
        fresh.close()
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.ascend_paths(object.__new__(GroupEngine), c.omega, c.phase, c.w, c.eps, c.lo, c.hi)


def test_a_non_finite_start_is_status_2_at_the_start(engine):
    c = mid_case()
    c.fit(engine)
    starts = c.starts.copy()
    starts[1, 1, 2] = np.nan
    out = c.ascend(engine, starts=starts)
    ref = c.ascend(engine)
    assert out["status"][1, 1] == 2 and np.isnan(out["x"][1, 1, 2]) and np.array_equal(out["x"][1, 1, :2], c.clipped[1, 1, :2])
    mask = np.ones((c.S, c.K), dtype=bool)
    mask[1, 1] = False
    assert np.array_equal(out["f"][mask], ref["f"][mask]) and np.array_equal(out["x"][mask], ref["x"][mask])
    assert out["winner"][1] != 1 and np.isfinite(out["f_best"]).all()


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------
def test_suggest_thompson_refined_on_the_real_engine(engine):
    D, N, M, Q, FEATURES = 3, 30, 2000, 5, 256
    bounds = np.array([[0.0, 1.0]] * D)
    X = np.random.RandomState(130).uniform(size=(N, D))
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2

    def driver():
        return B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=7, n_random=M)

    drv, twin = driver(), driver()
    picks = suggest_thompson(drv, Q, n_random=M, n_features=FEATURES, refine=4)
    plain = suggest_thompson(twin, Q, n_random=M, n_features=FEATURES)
    a, b = drv._random_state.get_state(), twin._random_state.get_state()
    assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    rows = np.array([list(p.values()) for p in picks])
    rows0 = np.array([list(p.values()) for p in plain])
    assert (rows >= bounds[:, 0]).all() and (rows <= bounds[:, 1]).all()
    assert drv._acquisition_function.i == 0 and drv._gp.X_train_.shape[0] == N
    # the documented draws, replayed on a third RandomState
    third = driver()
    third._gp.fit(third._space.params, third._space.target)
    rng = third._random_state
    np.column_stack([rng.uniform(0.0, 1.0, M) for _ in range(D)])
    gp = drv._gp
    omega, phase = spectral_draw(gp._kind, FEATURES, D, rng)
    w = rng.standard_normal((Q, FEATURES))
    eps = rng.standard_normal((Q, N)) * np.sqrt(float(gp.alpha))
    yn = (y - gp._y_train_mean) / gp._y_train_std
    args = (int(gp._kind), X, yn, np.array(gp._ls), float(gp.alpha), omega, phase, w, eps)
    f1 = T.path_value_grad(*args, rows[:, None, :], gp._y_train_mean, gp._y_train_std)[0][:, 0]
    f0 = T.path_value_grad(*args, rows0[:, None, :], gp._y_train_mean, gp._y_train_std)[0][:, 0]
    # >= up to the value bar: the device orders its OWN values exactly, the truth's differ from them by the evaluation's error
    slack = BAR * gp._y_train_std * max(1.0, float(np.max(np.abs((f0 - gp._y_train_mean) / gp._y_train_std))))
    print(f"truth value of the refined picks - of the candidate picks, in y_std: {((f1 - f0) / gp._y_train_std).tolist()}")
    assert (f1 >= f0 - slack).all()
    assert (f1 > f0 + slack).any(), "no pick improved on its candidate"
