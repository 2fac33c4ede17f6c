"""GPU (-m gpu): every stage of the int8 posterior pass (posterior_i8.hip, kstar_gen_kernel's digit branch) alone, through the
debug build's gpbo_debug_i8_* entry points, against exact integer arithmetic on the host (tests/i8_reference.py, validated by
tests/test_i8_reference_host.py):

  * the W packer: row exponents equal frexp, scales are the exact powers of two, every stored byte is the host's digit of
    Q = rint(W_ij 2^(54 - e_i)), everything outside the N x N lower triangle is zero whatever the input holds there;
  * the k* generator's digit branch: the decoded Q of every (candidate, train point) is rint(k* 2^54) of the bits the fp64
    branch writes, the partial means of both branches are the same bits, and the fp64 slab is the oracle's kernel matrix;
  * the GEMM on raw operands: `part` equals the order model bit for bit and lies within the derived bound
    (i8_reference.PART_BOUND_UNITS x 2^-53 x the exact sum) of the exact sum of squares — with per-row exponents 20 binades apart
    inside every 16-row tile, single digit-plane pairs, single entries around every tiling boundary, and all digits at -128 / +127
    at NP = 16384 where the int32 level sums reach 0.875 of 2^31;
  * non-finite and edge candidates end to end at NP = 2112: the oracle's NaN pattern, the fp64 path's values."""
import ctypes
import os

import numpy as np
import pytest

import i8_reference as R
from conftest import rel_err
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

S = R.S


def _report(what, part, L, e, wscale):
    """Both bars of a GEMM result: bitwise against the order model, and the derived bound against the exact sum."""
    model = R.order_model_part(L, wscale)
    units = R.part_error_units(part, R.exact_part(L, e))
    same = np.array_equal(part, model)
    print(f"{what}: max error {units:.3f} of {R.PART_BOUND_UNITS} x 2^-53 x exact ({units / R.PART_BOUND_UNITS:.3f} of the bound), "
          f"bitwise equal to the order model: {same}")
    assert units <= R.PART_BOUND_UNITS, (what, units)
    assert same, (what, int(np.sum(part != model)), "outputs differ from the order model")


# ---- the W packer -------------------------------------------------------------------------------------------------------
def _packer_input(N, NP, seed):
    rng = np.random.RandomState(seed)
    W = rng.standard_normal((NP, NP)) * 10.0 ** rng.uniform(-3, 1, size=(NP, 1))
    for r in range(100, 110):                                  # rows spanning 1e-12 ... 1e4
        W[r] = np.sign(rng.standard_normal(NP)) * 10.0 ** rng.uniform(-12, 4, NP)
    for r in (7, 1500, N - 1):                                 # all-zero rows (their lower-triangle part)
        W[r, :r + 1] = 0.0
    special = {}
    r = 200
    for k in (-40, -3, 0, 1, 17):                              # maxima exactly 2^k, 2^k (1 - 2^-53), and their negatives
        for mx in (2.0 ** k, np.nextafter(2.0 ** k, 0.0), -(2.0 ** k), -np.nextafter(2.0 ** k, 0.0)):
            W[r, :r + 1] = rng.uniform(-0.4, 0.4, r + 1) * 2.0 ** k
            W[r, int(rng.randint(r + 1))] = mx
            special[r] = mx
            r += 37
    # the maximum in the row's LAST lower-triangle column, and in its first
    W[1900, :1901] = rng.uniform(-0.1, 0.1, 1901)
    W[1900, 1900] = 0.75
    W[1901, :1902] = rng.uniform(-0.1, 0.1, 1902)
    W[1901, 0] = -0.75
    # finite, large garbage above the diagonal and in the rows and columns >= N: ignored
    garbage = 1e30 * rng.uniform(0.5, 1.0, size=(NP, NP)) * np.sign(rng.standard_normal((NP, NP)))
    outside = np.triu(np.ones((NP, NP), dtype=bool), 1)
    outside[N:, :] = True
    outside[:, N:] = True
    W[outside] = garbage[outside]
    return np.ascontiguousarray(W), special, outside


@pytest.mark.parametrize("N,NP", [(2048, 2048), (2080, 2112)])
def test_w_packer_against_host_quantisation(debug_engine, N, NP):
    W, special, outside = _packer_input(N, NP, seed=NP)
    Wd, wexp, wscale = debug_engine.debug_i8_pack_w(W, N)
    e = R.row_exponents(W, N)
    for r, mx in special.items():                              # the input is what it is meant to be
        assert np.max(np.abs(W[r, :r + 1])) == abs(mx)
    assert e[200] == -39 and e[200 + 37] == -40                # frexp: 2^k -> k + 1, the value just below -> k
    assert np.array_equal(wexp, e), np.nonzero(wexp != e)[0][:10]
    assert np.array_equal(wscale, R.scale_of_exponent(e))
    m, ex = np.frexp(wscale)
    assert np.all(m == 0.5) and np.array_equal(ex - 1, e - 2 * R.F + 8 * (S - 1))   # exact powers of two
    D = R.unpack_w(Wd, NP)
    Q = R.undigits(D)
    Qh = R.w_quantized(W, N, e)
    bad = int(np.sum(Q != Qh))
    print(f"N = {N}, NP = {NP}: {bad} of {Q.size} quantised entries differ; exponents {e.min()} ... {e.max()}")
    assert bad == 0
    assert np.array_equal(D, R.digits(Qh)), "the bytes are the balanced digits of Q (leading digit within [-65, 65])"
    assert not np.any(D[:, outside]), "a byte outside the N x N lower triangle is not zero"
    assert Wd.size == R.wd_bytes(NP)


# ---- the k* generator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,d,ls", [(O.MATERN25, 2, 0.03), (O.RBF, 2, 0.03), (O.MATERN25, 16, 0.08), (O.RBF, 16, 0.18)])
def test_kstar_digit_branch_against_the_fp64_branch(debug_engine, kernel, d, ls):
    N, NP, M = 2100, 2112, 448
    rng = np.random.RandomState(100 + d + kernel)
    X = rng.uniform(size=(N, d))
    y = np.sin(3.0 * X.sum(1)) + 0.1 * rng.standard_normal(N)
    Xc = rng.uniform(size=(M, d))
    for at in (0, 128):                                        # in both slabs below: copies of training points, far points
        Xc[at:at + 32] = X[at:at + 32]
        Xc[at + 32:at + 48] = 1e3 + rng.uniform(size=(16, d))
    yn, ym, ys = O.normalize_targets(y)
    debug_engine.fit(X, yn, kernel, ls, 1e-4)
    debug_engine.set_candidates(Xc)
    with pytest.raises(ValueError):                            # buffers sized from another NP than the model's: refused, nothing written
        debug_engine.debug_i8_kstar_digits(NP + 64, 0, 64)
    for m0, ldk in ((0, 64), (128, 320)):
        Kd, kst, mu_part = debug_engine.debug_i8_kstar_digits(NP, m0, ldk)
        Q = R.undigits(R.unpack_k(Kd, ldk, NP))                # [ldk][NP]
        assert np.all((kst >= 0.0) & (kst <= 1.0))
        Qf = np.rint(np.ldexp(kst, R.F)).astype(np.int64).T    # of the fp64 branch's own bits
        edge = int(np.sum((kst > 2.0 ** -60) & (kst < 2.0 ** -53)))
        ties = int(np.sum(np.ldexp(kst, R.F) % 1.0 == 0.5))
        ones, zeros = int(np.sum(kst[:N] == 1.0)), int(np.sum(kst[:N, 32:48] == 0.0))
        bad = int(np.sum(Q != Qf))
        Ko = O.kernel_matrix(kernel, X, Xc[m0:m0 + ldk], ls)
        err_k = rel_err(kst[:N], Ko)
        same_mu = np.array_equal(mu_part[0].view(np.int64), mu_part[1].view(np.int64))
        print(f"kernel {kernel}, d = {d}, m0 = {m0}, ldk = {ldk}: {bad} of {Q.size} Q differ; k* = 1: {ones}, k* = 0 (far): {zeros}, "
              f"2^-60 < k* < 2^-53: {edge}, exact ties: {ties}; K rel err {err_k:.2e}; partial means bitwise equal: {same_mu}")
        # the inputs hold what the case is about
        assert ones >= 32 and zeros == 16 * N and edge >= 20, (ones, zeros, edge)
        assert bad == 0
        assert same_mu
        assert err_k < 1e-14, err_k
        assert np.array_equal(R.unpack_k(Kd, ldk, NP), R.digits(Q)), "the bytes are the balanced digits of Q"


# ---- the GEMM on raw operands -------------------------------------------------------------------------------------------
def _row_exponents(NP, seed):
    """Independent per row in [-30, 30], so that taking another row's scale inside a tile is a gross error."""
    e = np.random.RandomState(seed).randint(-30, 31, size=NP)
    span = e.reshape(NP // 16, 16).max(1) - e.reshape(NP // 16, 16).min(1)
    assert np.all(span >= 20), "every 16-row tile must span at least 20 binades"
    return e


def _legal_operands(NP, M, seed):
    rng = np.random.RandomState(seed)
    A = R.digits(R.quantize(np.tril(rng.uniform(-1.0, 1.0, size=(NP, NP)))))
    B = R.digits(R.quantize(rng.uniform(0.0, 1.0, size=(M, NP))))
    return A, B


@pytest.mark.parametrize("M", [64, 192])
@pytest.mark.parametrize("NP", [2048, 2112, 4096])
def test_gemm_random_legal_digits(debug_engine, NP, M):
    A, B = _legal_operands(NP, M, seed=NP + M)
    e = _row_exponents(NP, seed=NP)
    wscale = R.scale_of_exponent(e)
    part = debug_engine.debug_i8_gemm(R.pack_w(A), wscale, R.pack_k(B), NP, M)
    assert part.shape == ((NP + 127) // 128, M)
    _report(f"NP = {NP}, M = {M}, legal digits", part, R.level_sums(A, B), e, wscale)


def test_gemm_full_range_digits(debug_engine):
    """Digits the packers never produce: every plane uniform over [-128, 127], the leading ones included."""
    NP, M = 2112, 192
    rng = np.random.RandomState(9)
    A = rng.randint(-128, 128, size=(S, NP, NP)).astype(np.int8) * np.tril(np.ones((NP, NP), dtype=np.int8))[None]
    B = rng.randint(-128, 128, size=(S, M, NP)).astype(np.int8)
    e = _row_exponents(NP, seed=10)
    wscale = R.scale_of_exponent(e)
    part = debug_engine.debug_i8_gemm(R.pack_w(A), wscale, R.pack_k(B), NP, M)
    _report("NP = 2112, M = 192, full-range digits", part, R.level_sums(A, B), e, wscale)


def test_gemm_single_plane_pairs(debug_engine):
    """Only plane s of W and plane t of k* non-zero: exactly the pairs with s + t <= S - 1 contribute, each at level s + t."""
    NP, M = 2112, 64
    rng = np.random.RandomState(21)
    a = rng.randint(-128, 128, size=(NP, NP)).astype(np.int8) * np.tril(np.ones((NP, NP), dtype=np.int8))
    b = rng.randint(-128, 128, size=(M, NP)).astype(np.int8)
    e = _row_exponents(NP, seed=22)
    wscale = R.scale_of_exponent(e)
    kept = [(s, t) for s in range(S) for t in range(S - s)]
    assert len(kept) == 28
    worst = 0.0
    for s, t in kept + [(3, 4), (S - 1, S - 1), (1, S - 1)]:
        A = np.zeros((S, NP, NP), dtype=np.int8)
        B = np.zeros((S, M, NP), dtype=np.int8)
        A[s], B[t] = a, b
        part = debug_engine.debug_i8_gemm(R.pack_w(A), wscale, R.pack_k(B), NP, M)
        L = R.level_sums(A, B)
        if s + t <= S - 1:
            assert np.any(L[s + t]) and not np.any(np.delete(L, s + t, axis=0))
            model = R.order_model_part(L, wscale)
            units = R.part_error_units(part, R.exact_part(L, e))
            worst = max(worst, units)
            assert units <= R.PART_BOUND_UNITS, (s, t, units)
            assert np.array_equal(part, model), (s, t)
            assert np.all(part > 0)
        else:
            assert not np.any(L)
            assert np.array_equal(part, np.zeros_like(part)), (s, t, "a dropped pair contributes")
    print(f"28 kept pairs: max error {worst:.3f} of {R.PART_BOUND_UNITS} x 2^-53 x exact, all bitwise equal to the order model; "
          f"3 dropped pairs: part == 0")


def test_gemm_single_entries_around_the_tiling_boundaries(debug_engine):
    """W with ONE non-zero entry (through the packer), k* with one non-zero train point per candidate: the entry meets exactly the
    candidates whose point is its column, in its row's chunk — or nobody, when it lies past the diagonal."""
    NP = N = 2112
    M = 64
    rng = np.random.RandomState(31)
    positions = [
        (1000, 320), (1000, 383), (1000, 384), (1000, 0), (1000, 63), (1000, 64),        # first / last column of a 64-step
        (16 * 80 + 3, 16 * 80 + 3), (16 * 83 + 5, 16 * 83 + 5),                            # diagonal of an even / odd 16-row block
        (32 * 41, 32 * 41), (32 * 41 + 31, 32 * 41 + 31), (0, 0), (63, 63), (64, 64),      # ... of an odd 32-row block, its ends
        (2111, 2111), (2111, 0), (2111, 2048), (2048, 2047), (2079, 2079),                 # the ragged chunk (two waves of four)
        (643, 644), (1000, 1001), (1023, 1024), (2110, 2111), (0, 1),                      # just past the diagonal: nothing
    ]
    for row, col in positions:
        W = np.zeros((NP, NP))
        W[row, col] = rng.uniform(0.5, 1.0) * 2.0 ** int(rng.randint(-20, 20))
        Wd, wexp, wscale = debug_engine.debug_i8_pack_w(W, N)
        e = R.row_exponents(W, N)
        A = R.unpack_w(Wd, NP)
        assert np.array_equal(R.undigits(A), R.w_quantized(W, N, e)) and np.array_equal(wexp, e)
        points = np.clip(col - 32 + np.arange(M), 0, NP - 1)   # candidate j's only train point
        K = np.zeros((M, NP))
        K[np.arange(M), points] = rng.uniform(0.1, 1.0, M)
        B = R.digits(R.quantize(K))
        part = debug_engine.debug_i8_gemm(Wd, wscale, R.pack_k(B), NP, M)
        L = R.level_sums(A, B)
        hit = np.zeros_like(part, dtype=bool)
        if col <= row:
            hit[row // 128, points == col] = True
            assert hit.sum() >= 1
        assert np.array_equal(part != 0.0, hit), (row, col, np.argwhere((part != 0.0) != hit)[:5])
        model = R.order_model_part(L, wscale)
        units = R.part_error_units(part, R.exact_part(L, e))
        assert units <= R.PART_BOUND_UNITS and np.array_equal(part, model), (row, col, units)
    print(f"{len(positions)} single entries: non-zero outputs exactly where expected, all bitwise equal to the order model")


def _free_device_bytes():
    """hipMemGetInfo of the HIP runtime this process already runs on (the one libgpbo is linked against)."""
    path = "libamdhip64.so"
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    hip = ctypes.CDLL(path)
    free_b, total_b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = hip.hipMemGetInfo(ctypes.byref(free_b), ctypes.byref(total_b))
    assert rc == 0, f"hipMemGetInfo: {rc}"
    return free_b.value


def _constant_lower_triangle_buffer(NP, digit):
    """The W buffer with `digit` in every plane of every entry of the lower triangle (built in place: the [S, NP, NP] array of
    i8_reference.pack_w would be 1.9 GB at NP = 16384)."""
    first, total = R.wd_steps(NP // 16)
    buf = np.full((total, S, 4, 16, 16), digit, dtype=np.int8)     # [step][plane][g][item][byte]
    g, item, byte = np.meshgrid(np.arange(4), np.arange(16), np.arange(16), indexing="ij")
    for b in range(NP // 16):
        last = b // 4                                              # the step that holds the block's diagonal
        past = (64 * last + 16 * g + byte) > (16 * b + item)
        buf[first[b] + last][:, past] = 0
    return buf.reshape(-1)


@pytest.mark.parametrize("digit", [-128, 127])
def test_gemm_int32_level_sums_at_their_bound(debug_engine, digit):
    """NP = 16384, every digit of both operands -128 (+127), the leading planes included: level l of row i sums (l + 1) (i + 1)
    products of 128^2; the top one, 7 x 128^2 x 16384 = 1 879 048 192, is the largest an int32 level sum can get."""
    NP, M = 16384, 64
    assert S * 128 * 128 * NP == 1879048192 < 2 ** 31
    need = 2e9                                                     # W digits 0.94 GB, the rest is small
    free_b = _free_device_bytes()
    if free_b < need:
        pytest.skip(f"the NP = 16384 operands need about {need / 1e9:.0f} GB of device memory; {free_b / 1e9:.1f} GB are free")
    # the builder against the reference's packer, where that one is affordable
    small = np.full((S, 192, 192), digit, dtype=np.int8) * np.tril(np.ones((192, 192), dtype=np.int8))[None]
    assert np.array_equal(_constant_lower_triangle_buffer(192, digit), R.pack_w(small))
    L1 = R.level_sums(small, np.full((S, 1, 192), digit, dtype=np.int8))
    assert all(L1[l, i, 0] == (l + 1) * digit * digit * (i + 1) for l in range(S) for i in range(192))   # the closed form
    Wd = _constant_lower_triangle_buffer(NP, digit)
    Kd = np.full(M * NP * S, digit, dtype=np.int8)
    e = _row_exponents(NP, seed=5)
    wscale = R.scale_of_exponent(e)
    part = debug_engine.debug_i8_gemm(Wd, wscale, Kd, NP, M)
    L = ((np.arange(S) + 1)[:, None, None] * (digit * digit) * (np.arange(NP) + 1)[None, :, None]).astype(np.int64)   # [S][NP][1]
    assert L.max() == S * digit * digit * NP and (digit != -128 or L.max() == 1879048192)
    assert np.all(part == part[:, :1]), "every candidate holds the same digits"
    _report(f"NP = 16384, every digit {digit}", part[:, :1], L, e, wscale)


# ---- non-finite and edge candidates, end to end -------------------------------------------------------------------------
def _posterior(engine, path, ym, ys):
    if path is None:
        os.environ.pop("GPBO_POST_KERNEL", None)
    else:
        os.environ["GPBO_POST_KERNEL"] = path
    try:
        return engine.posterior(0, ym, ys)
    finally:
        os.environ.pop("GPBO_POST_KERNEL", None)


def _apriori_sd_bound(gp, Xc):
    """Worst case of |sd_i8 - sd_f64| / s_y from the scheme alone: both operands are rounded at 2^-55 of their scale, so
    |dv_i| <= 2^-55 (sum_j |W_ij| k*_j-free part + max_j |W_ij| sum_j k*_j), d(sum v^2) <= 2 sum_i |v_i| |dv_i|, d sd = d var / (2 sd).
    (Rounding errors do not line up: what is measured is about a hundredth of it.)"""
    from scipy.linalg import solve_triangular

    N = gp.X.shape[0]
    W = solve_triangular(gp.L, np.eye(N), lower=True)
    Kt = O.kernel_matrix(gp.kind, Xc, gp.X, gp.length_scale)
    V = W @ Kt.T
    sd = np.sqrt(1.0 - np.einsum("ij,ij->j", V, V))
    dv = 2.0 ** -55 * (np.abs(W).sum(1)[:, None] + np.abs(W).max(1)[:, None] * Kt.sum(1)[None, :])
    return float(np.max(2.0 * (np.abs(V) * dv).sum(0) / (2.0 * sd)))


# The 1e-12 bar against the fp64 GEMM is the one tests/test_gpu_int8_shape.py holds, on Matern-2.5, d = 8, length scale 0.7, noise 1e-4.
# The scheme's truncation error grows with the row sums of |W| = |L^-1|, so the bar belongs to models of that conditioning: the
# Matern case below is that model, the RBF case (a smoother kernel, a worse-conditioned K at equal length scale) takes the length
# scale 0.4, and the test asserts from the oracle's own factor that the a-priori worst case of either stays below 1e-11: the worst
# case lets all N = 2100 rounding errors of a row line up, independent ones add up to about 1 / sqrt(N) = 1 / 46 of that, which
# leaves the bar a factor of four.
@pytest.mark.parametrize("kernel,ls", [(O.MATERN25, 0.7), (O.RBF, 0.4)])
def test_non_finite_and_edge_candidates_end_to_end(engine, debug_engine, kernel, ls):
    N, M, d = 2100, 3000, 8
    rng = np.random.RandomState(50 + kernel)
    X = rng.uniform(size=(N, d))
    y = np.sin(3.0 * X.sum(1)) + 0.1 * rng.standard_normal(N)
    Xc = rng.uniform(size=(M, d))
    Xc[5, 1] = np.nan                                          # the first NaN
    Xc[1700] = np.nan
    Xc[2998, 3] = np.nan
    Xc[100, 0] = np.inf
    Xc[2200, 2] = -np.inf
    Xc[300] = X[17]                                            # a copy of a training point
    far = 2999
    Xc[far] = 1e3                                              # every k* underflows to 0
    gp = O.fit_fixed_theta(kernel, X, y, ls, 1e-4)
    with np.errstate(all="ignore"):
        mu_o, sd_o = O.predict(gp, Xc)
    assert np.isnan(mu_o[[5, 1700, 2998]]).all() and np.isnan(sd_o[[5, 1700, 2998]]).all()
    assert np.isfinite(mu_o[[300, far]]).all() and np.isfinite(sd_o[[300, far]]).all()
    apriori = _apriori_sd_bound(gp, Xc[np.isfinite(sd_o)])
    print(f"kernel {kernel}: a-priori worst case of |sd_i8 - sd_f64| / s_y = {apriori:.2e}")
    assert apriori <= 1e-11, apriori
    yn, ym, ys = O.normalize_targets(y)
    debug_engine.fit(X, yn, kernel, ls, 1e-4)
    debug_engine.set_candidates(Xc)
    mu3, sd3 = _posterior(debug_engine, "3", ym, ys)
    for name, eng in (("debug build", debug_engine), ("product", engine)):
        eng.fit(X, yn, kernel, ls, 1e-4)
        eng.set_candidates(Xc)
        mu8, sd8 = _posterior(eng, None, ym, ys)               # NP = 2112: the int8 route
        fin = np.isfinite(sd3)
        d_sd = float(np.max(np.abs(sd8[fin] - sd3[fin])) / ys)
        print(f"kernel {kernel}, {name}: NaN mu {int(np.isnan(mu8).sum())} (oracle {int(np.isnan(mu_o).sum())}), NaN sd "
              f"{int(np.isnan(sd8).sum())} (oracle {int(np.isnan(sd_o).sum())}), max |sd_i8 - sd_f64| / s_y = {d_sd:.3e}, "
              f"sd[far] / s_y - 1 = {sd8[far] / ys - 1.0:.3e}, mu[far] - y_mean = {mu8[far] - ym:.3e}")
        assert np.array_equal(np.isnan(mu8), np.isnan(mu_o)), "mu: the oracle's NaN pattern"
        assert np.array_equal(np.isnan(sd8), np.isnan(sd_o)), "sd: the oracle's NaN pattern"
        assert np.array_equal(mu8, mu3, equal_nan=True), "mu: the fp64 path's bits"
        assert np.array_equal(np.isnan(sd8), np.isnan(sd3)) and d_sd <= 1e-12, d_sd
        assert mu8[far] == ym and abs(sd8[far] - ys) <= 1e-12 * ys
        bi, bv, si, sv, vals = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
        assert bi == 5 and np.isnan(bv), "arg-best: the first NaN"
        assert np.array_equal(np.isnan(vals), np.isnan(mu_o))
