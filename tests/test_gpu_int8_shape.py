"""GPU (-m gpu): the int8 posterior GEMM on v_mfma_i32_16x16x64_i8 (posterior_i8.hip) — k steps of 64 train points, two 16-row
blocks x four 16-candidate blocks per wave — against the fp64 slab GEMM (GPBO_POST_KERNEL=3, debug build) at the bar of
test_gpu_int8_posterior.py: mu bitwise equal, sigma within 1e-12 of s_y.

  * NP = 2048, 2112 (N = 2100: ragged last 128-row chunk) and 4096, each with M = 3 000 (a partial slab) and M = 2^16;
  * N = 2080 (NP = 2112, 66 blocks of 32 rows): the model ends in the middle of the last 64-step, so the last step of a wave is
    half past the diagonal for an even 32-row block (64: rows 2048 ... 2079, the step's columns 2080 ... 2111 are padding) and
    for an odd one (65: all rows padding), besides the even blocks of every chunk, whose diagonal lies in the step's lower half."""
import os

import numpy as np
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu


def _posterior(engine, path, ym, ys):
    if path is None:
        os.environ.pop("GPBO_POST_KERNEL", None)
    else:
        os.environ["GPBO_POST_KERNEL"] = path
    try:
        return engine.posterior(0, ym, ys)
    finally:
        os.environ.pop("GPBO_POST_KERNEL", None)


def _against_fp64(debug_engine, N, M, d=8, seed=31):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    y = np.sin(3.0 * X.sum(1)) + 0.1 * rng.standard_normal(N)
    Xc = np.random.RandomState(seed + 1).uniform(size=(M, d))
    yn, ym, ys = O.normalize_targets(y)
    debug_engine.fit(X, yn, O.MATERN25, 0.7, 1e-4)
    debug_engine.set_candidates(Xc)
    mu8, sd8 = _posterior(debug_engine, None, ym, ys)
    mu3, sd3 = _posterior(debug_engine, "3", ym, ys)
    d_sd = float(np.max(np.abs(sd8 - sd3)) / ys)
    print(f"N = {N}, M = {M}: max |sd_i8 - sd_f64| / s_y = {d_sd:.3e}, mu bitwise equal: {np.array_equal(mu8, mu3)}")
    assert np.array_equal(mu8, mu3), "mu does not go through the GEMM: bitwise the fp64 path's"
    assert np.all(np.isfinite(sd8)) and d_sd <= 1e-12, d_sd


@pytest.mark.parametrize("M", [3000, 1 << 16])
@pytest.mark.parametrize("N", [2048, 2100, 4096])      # NP = 2048, 2112, 4096
def test_k_steps_of_64_match_the_fp64_gemm(debug_engine, N, M):
    _against_fp64(debug_engine, N, M)


def test_last_step_half_past_the_diagonal(debug_engine):
    _against_fp64(debug_engine, 2080, 3000, seed=37)
