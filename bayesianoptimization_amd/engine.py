"""GpEngine — thin Python owner of one libgpbo context (one GPU, one HIP stream).

Slot 0 holds the target GP, slots 1.. the constraint GPs; the candidate matrix is uploaded once and
stays resident in HBM across posterior / acquisition calls.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json

import numpy as np

from . import _lib
from ._lib import dptr, iptr

RBF, MATERN25, MATERN15, MATERN05 = 0, 1, 2, 3
UCB, EI, POI, LOG_EI = 0, 1, 2, 3      # enum gpbo_acq (LOG_EI: never with constraints, never in evolve_mixed)
LOG_CEI, LOG_FEAS = 5, 6               # log EI + sum_j log p_j; sum_j log p_j alone, >= 1 constraint (4 is unassigned; neither in evolve_mixed)
F64, F32 = 0, 1

TIMING_NAMES = ("fit", "posterior_main", "posterior_finalize", "acq_argbest", "kmat", "cholesky", "trtri")


def advance_mt19937(random_state, n_words: int, lib=None):
    """Advance a legacy MT19937 `RandomState` by `n_words` 32-bit outputs WITHOUT generating them: whole 624-word blocks by
    the polynomial jump the device generator uses (gpbo_mt19937_jump_blocks, host code: x^J mod phi applied to the state),
    the rest by position.  What `n_words // 2` calls of `random_sample()` would leave behind, bit for bit — a rank that
    generated only ITS rows of a candidate matrix on its GPU uses it to leave its RandomState where the reference's
    `space.random_sample(M, random_state)` would (tests/test_mt_jump_host.py checks it against NumPy, no GPU needed)."""
    lib = lib or _lib.load_library()
    name, key, pos, has_gauss, cached = random_state.get_state(legacy=True)
    if name != "MT19937":
        raise TypeError("advance_mt19937 needs an MT19937 RandomState")
    n_words = int(n_words)
    avail = 624 - int(pos)
    if n_words <= avail:
        random_state.set_state((name, key, int(pos) + n_words, has_gauss, cached))
        return
    n_blocks = (n_words - avail + 623) // 624
    key_in = np.ascontiguousarray(key, dtype=np.uint32)
    key_out = np.empty(624, dtype=np.uint32)
    rc = lib.gpbo_mt19937_jump_blocks(key_in.ctypes.data_as(C.POINTER(C.c_uint32)), n_blocks,
                                      key_out.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != _lib.GPBO_OK:
        _lib.raise_for_status(lib, None, rc)
    random_state.set_state((name, key_out, (n_words - avail - 1) % 624 + 1, has_gauss, cached))


_INT_ARRAYS: dict = {}      # ctypes array types by length (creating one costs ~2 us per call)


def _is_scaled(amplitude, white) -> bool:
    """Does (amplitude, white) ask for a scaled model (gpbo_fit_scaled / gpbo_lml_scaled)?  1 and 0 are the unit model's calls."""
    return float(amplitude) != 1.0 or float(white) != 0.0


def _model_arrays(X, y_norm, length_scale, check=True):
    """(X, y_norm, length scales) as the library reads them: contiguous float64, y flat, the scales 1-D.  check: a fit's two refusals."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if check and X.ndim != 2:
        raise ValueError("X must be 2-D (n_samples, n_features)")
    y_norm = np.ascontiguousarray(y_norm, dtype=np.float64).ravel()
    if check and y_norm.shape[0] != X.shape[0]:
        raise ValueError("X and y have inconsistent numbers of samples")
    return X, y_norm, np.ascontiguousarray(np.atleast_1d(np.asarray(length_scale, dtype=np.float64)))


def _argbest_frame(lb, ub, k_seeds, n_values=None):
    """The arrays every arg-best call hands to the library: (lb, ub, n_c, seed_idx, seed_val, ys).  lb / ub: contiguous float64 or None,
    n_c their count; the seed records hold at least one entry (-1 / NaN: none); ys: room for `n_values` values (None: not asked for)."""
    lb = np.ascontiguousarray(np.atleast_1d(np.asarray(lb, dtype=np.float64))) if lb is not None else None
    ub = np.ascontiguousarray(np.atleast_1d(np.asarray(ub, dtype=np.float64))) if ub is not None else None
    n_c = 0 if lb is None else lb.shape[0]
    if n_c and (ub is None or ub.shape[0] != n_c):
        raise ValueError("lb and ub must have the same length")
    seed_idx = np.full(max(k_seeds, 1), -1, dtype=np.int64)
    seed_val = np.full(max(k_seeds, 1), np.nan)
    return lb, ub, n_c, seed_idx, seed_val, (None if n_values is None else np.empty(n_values))


def path_winners(x, f) -> dict:
    """Per draw the winning run of `ascend_paths`: x (S, K, d), f (S, K) -> winner (S,) = the start with the largest finite f, ties
    to the lowest start (-1: none is finite), x_best (S, d), f_best (S,) (NaN where winner is -1)."""
    x, f = np.asarray(x, dtype=np.float64), np.asarray(f, dtype=np.float64)
    key = np.where(np.isfinite(f), f, -np.inf)
    winner = key.argmax(axis=1).astype(np.int64)          # the first index of the maximum
    rows = np.arange(f.shape[0])
    ok = np.isfinite(f[rows, winner])
    x_best = np.where(ok[:, None], x[rows, winner], np.nan)
    f_best = np.where(ok, f[rows, winner], np.nan)
    return {"winner": np.where(ok, winner, -1), "x_best": x_best, "f_best": f_best}


class GpEngine:
    """One engine context = one GPU, one HIP stream, 8 model slots (0 = target GP, 1.. = constraint GPs) and one resident
    candidate matrix.  Calls are synchronous from the host's point of view unless noted (`posterior(fetch=False)` only
    enqueues); a context is not thread-safe — the lockstep helpers keep every device call on the serving thread."""

    def __init__(self, device: int = 0, debug: bool = False):
        # debug=True: the context lives in libgpbo_dbg.so (same sources + gpbo_debug_* entry points and the kernel A/B
        # environment switches) — tests and scripts only
        self._lib = _lib.load_debug_library() if debug else _lib.load_library()
        self.debug = bool(debug)
        h = C.c_void_p()
        rc = self._lib.gpbo_create(int(device), C.byref(h))
        if rc != _lib.GPBO_OK:
            _lib.raise_for_status(self._lib, None, rc)
        self._h = h
        self.device = int(device)
        self._init_state()

    def _init_state(self):
        """Every host-side attribute of an engine whose context exists (a device group: its first device's)."""
        self.n_candidates = 0
        self.world_size = 1
        self.rank = 0
        self._serial: dict[int, int] = {}    # slot -> number of times its factorisation was rewritten
        self._overlap_depth = 0              # > 0 inside overlapped_fits()
        self._pending_fits: set[int] = set()  # slots with a gpbo_fit_begin not yet waited for
        self._pending_inputs: dict[int, tuple] = {}   # ... and the arrays that fit reads until it is waited for
        self._scaled: dict[int, tuple[float, float]] = {}   # slot -> (amplitude, white) of its scaled fit (absent: 1, 0)
        self._n_obs: dict[int, tuple[int, int]] = {}   # slot -> (observations, dimensions) of its fit: the path draws' shapes
        self._cand_dim = None                # columns of the resident candidates the engine generated itself
        self._resident = False               # (device groups: the candidate shards are in place)
        self.last_polish: dict = {}          # nit / nfev / rounds of the last polish_seeds
        self.timing = True                   # the calls record their HIP event pairs (set_timing)

    # -- lifecycle ---------------------------------------------------------------------------
    def __deepcopy__(self, memo):
        # a context is a device resource, not data: estimators that get deep-copied (sklearn.base.clone, bayes_opt's
        # ConstantLiar copying a constrained target space) keep pointing at the same engine
        return self

    __copy__ = lambda self: self  # noqa: E731

    def __reduce__(self):
        raise TypeError("GpEngine holds a GPU context and cannot be pickled; create one per process (GpEngine(device))")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpbo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, info=0):
        if rc != _lib.GPBO_OK:
            _lib.raise_for_status(self._lib, self._h, rc, info)

    def synchronize(self):
        self._settle()
        self._check(self._lib.gpbo_synchronize(self._h))

    def device_info(self) -> dict:
        buf = C.create_string_buffer(1024)
        self._check(self._lib.gpbo_device_info(self._h, buf, 1024))
        return json.loads(buf.value.decode())

    # -- fit ---------------------------------------------------------------------------------
    def fit(self, X, y_norm, kernel: int, length_scale, noise: float, slot: int = 0, precision: int = F64,
            amplitude: float = 1.0, white: float = 0.0):
        """K + noise*I -> L, W = L^-1, alpha, at fixed theta (sklearn _gpr.py:346-364).
        amplitude / white other than 1 / 0: the scaled model amplitude * k + (white + noise) * I (ConstantKernel * k + WhiteKernel
        under an estimator whose alpha is `noise`; gpbo_fit_scaled) — the slot's posteriors then carry amplitude and white."""
        scaled = _is_scaled(amplitude, white)
        X, y_norm, ls = _model_arrays(X, y_norm, length_scale)
        info = C.c_int(0)
        self._settle(slot)
        self._touch(slot)
        self._n_obs[int(slot)] = (int(X.shape[0]), int(X.shape[1]))      # sample_paths checks the shapes of its draws against it
        if scaled:
            # gpbo_fit_begin has no scaled twin: inside overlapped_fits() a scaled fit runs here and now, on the context's own stream
            # (its slot is settled above; the fits pending on OTHER slots keep running on their streams and are waited for as usual)
            self._scaled.pop(int(slot), None)
            rc = self._lib.gpbo_fit_scaled(self._h, int(slot), dptr(X), dptr(y_norm), X.shape[0], X.shape[1], int(kernel), dptr(ls),
                                           int(ls.shape[0]), float(amplitude), float(white), float(noise), int(precision),
                                           C.byref(info))
            self._check(rc, info.value)
            self._scaled[int(slot)] = (float(amplitude), float(white))
            return self._touch(slot)
        self._scaled.pop(int(slot), None)
        if self._overlap_depth > 0:
            # inside overlapped_fits(): enqueue on the slot's own stream and return; waited for (and checked) at the end
            # of the block or by the first call that reads the slot
            rc = self._lib.gpbo_fit_begin(self._h, int(slot), dptr(X), dptr(y_norm), X.shape[0], X.shape[1], int(kernel),
                                          dptr(ls), int(ls.shape[0]), float(noise), int(precision))
            self._check(rc)
            self._pending_fits.add(int(slot))
            # gpbo_fit_begin copies X / y asynchronously: the arrays it was given stay referenced until the fit is waited for
            self._pending_inputs[int(slot)] = (X, y_norm, ls)
            return self._touch(slot)
        rc = self._lib.gpbo_fit(self._h, int(slot), dptr(X), dptr(y_norm), X.shape[0], X.shape[1], int(kernel),
                                dptr(ls), int(ls.shape[0]), float(noise), int(precision), C.byref(info))
        self._check(rc, info.value)
        return self._touch(slot)

    @contextlib.contextmanager
    def overlapped_fits(self):
        """`fit()` calls inside the block are enqueued on their slots' own streams (gpbo_fit_begin) and overlap on the
        device — the target GP and the constraint GPs of one suggest() (bayes_opt/acquisition.py:84-86).  Leaving the
        block waits for all of them; a kernel matrix that is not positive definite raises there (np.linalg.LinAlgError
        with sklearn's hint, as fit() does).  Any call that reads a slot in between waits for that slot first.  A scaled fit
        (amplitude / white given) is not enqueued: it completes inside its fit() call and raises there."""
        self._overlap_depth += 1
        try:
            yield self
        except BaseException:
            # something else failed inside the block: still leave no fit in flight, but let THAT error propagate
            self._overlap_depth -= 1
            if self._overlap_depth == 0:
                try:
                    self.wait_fits()
                except Exception:  # noqa: BLE001
                    pass
            raise
        else:
            self._overlap_depth -= 1
            if self._overlap_depth == 0:
                self.wait_fits()

    def wait_fits(self):
        """Wait for every pending gpbo_fit_begin; all are waited for before the first failure is raised."""
        first = None
        for slot in sorted(self._pending_fits):
            try:
                self._wait_fit(slot)
            except Exception as e:  # noqa: BLE001
                first = first or e
        if first is not None:
            raise first

    def _wait_fit(self, slot: int):
        self._pending_fits.discard(int(slot))
        info = C.c_int(0)
        rc = self._lib.gpbo_fit_wait(self._h, int(slot), C.byref(info))
        self._pending_inputs.pop(int(slot), None)
        self._check(rc, info.value)

    def _settle(self, slot=None):
        """Before a call reads or rewrites a slot (None: any slot): its pending fit, if any, has to be complete."""
        if not self._pending_fits:
            return
        if slot is None:
            self.wait_fits()
        elif int(slot) in self._pending_fits:
            self._wait_fit(int(slot))

    def fit_append(self, x_new, y_norm, slot: int = 0, amplitude: float = 1.0, white: float = 0.0):
        """Grow the slot's fitted model by the rows `x_new` at unchanged kernel/length scale/noise (gpbo_fit_append);
        `y_norm` = ALL normalised targets, old and new.  `x_new` may be empty (new targets for the same inputs).
        The slot keeps the amplitude and white of its fit: the two arguments say which model the caller believes it is growing,
        and anything else than the slot's own is refused."""
        self._settle(slot)
        if (float(amplitude), float(white)) != self._scaled.get(int(slot), (1.0, 0.0)):
            raise ValueError("fit_append: amplitude / white differ from the slot's fitted model")
        y_norm = np.ascontiguousarray(y_norm, dtype=np.float64).ravel()
        x_new = np.ascontiguousarray(x_new, dtype=np.float64)
        if x_new.ndim != 2:
            raise ValueError("x_new must be 2-D (n_new, n_features)")
        info = C.c_int(0)
        self._touch(slot)
        rc = self._lib.gpbo_fit_append(self._h, int(slot), dptr(x_new) if x_new.shape[0] else None, x_new.shape[0],
                                       x_new.shape[1], dptr(y_norm), y_norm.shape[0], C.byref(info))
        self._check(rc, info.value)
        self._n_obs[int(slot)] = (int(y_norm.shape[0]), int(x_new.shape[1]))
        return self._touch(slot)

    def lml_batch(self, X, y_norm, kernel: int, length_scales, noise: float, eval_gradient=True, reuse_inputs=False):
        """[(lml, grad)] for every row of `length_scales` (n_theta x n_ls), evaluated side by side on the device
        (gpbo_lml_batch); each entry is bitwise what `lml()` returns for that row.  Model slots are not touched.
        reuse_inputs=True: (X, y_norm) are the arrays of the previous call and are not uploaded again."""
        vals, grads = self.lml_batch_arrays(X, y_norm, kernel, length_scales, noise, eval_gradient, reuse_inputs)
        return [(float(vals[i]), grads[i].copy()) for i in range(vals.shape[0])]

    def lml_batch_arrays(self, X, y_norm, kernel: int, length_scales, noise: float, eval_gradient=True, reuse_inputs=False):
        """`lml_batch` as two arrays — values (n_theta,) and gradients (n_theta, n_ls): what a theta-search round needs, without
        the per-lane tuples (a round is ~50-100 us of device time at small N: every microsecond of Python around it shows)."""
        self._settle()
        ls = np.ascontiguousarray(np.atleast_2d(np.asarray(length_scales, dtype=np.float64)))
        n, n_ls = ls.shape
        vals = np.zeros(n)
        grads = np.zeros((n, n_ls))
        infos = _INT_ARRAYS.get(n)
        if infos is None:
            infos = _INT_ARRAYS[n] = C.c_int * n
        if reuse_inputs:
            xp = yp = None
        else:
            X = np.ascontiguousarray(X, dtype=np.float64)
            y_norm = np.ascontiguousarray(y_norm, dtype=np.float64).ravel()
            xp, yp = dptr(X), dptr(y_norm)
        rc = self._lib.gpbo_lml_batch(self._h, n, xp, yp, X.shape[0], X.shape[1], int(kernel), dptr(ls), n_ls, float(noise),
                                      int(bool(eval_gradient)), dptr(vals), dptr(grads), infos())
        if rc:
            self._check(rc)
        return vals, grads

    def lml_search_rounds(self, X, y_norm, kernel: int, n_ls: int, noise: float):
        """`round(scales (n <= 8, n_ls)) -> (values (n,), gradients (n, n_ls))` for the rounds of ONE theta search: the inputs are
        uploaded by the first round and stay resident (gpbo_lml_batch with X = y = NULL afterwards), and everything a round needs
        around the library call — the length-scale block, the result arrays, their ctypes pointers — is made once here instead of
        per round (a round at N <= 64 is a 41 us kernel: the ~10 us of argument handling around it showed).  The arrays returned are
        the frame's own: valid until the next round."""
        self._settle()
        X = np.ascontiguousarray(X, dtype=np.float64)
        y_norm = np.ascontiguousarray(y_norm, dtype=np.float64).ravel()
        N, d = int(X.shape[0]), int(X.shape[1])
        ls = np.ones((8, n_ls))
        vals = np.zeros(8)
        grads = np.zeros((8, n_ls))
        infos = (C.c_int * 8)()
        p_ls, p_vals, p_grads = dptr(ls), dptr(vals), dptr(grads)
        xp, yp = [dptr(X)], [dptr(y_norm)]
        call, h, kind, nz, ck = self._lib.gpbo_lml_batch, self._h, int(kernel), float(noise), self._check

        def one_round(scales):
            n = scales.shape[0]
            ls[:n] = scales
            rc = call(h, n, xp[0], yp[0], N, d, kind, p_ls, n_ls, nz, 1, p_vals, p_grads, infos)
            xp[0] = yp[0] = None              # (X, y_norm stay referenced by this closure for the search's lifetime)
            if rc:
                ck(rc)
            return vals[:n], grads[:n]

        return one_round

    def lml_batch_scaled_arrays(self, X, y_norm, kernel: int, length_scales, amplitudes, whites, noise: float, eval_gradient=True,
                                reuse_inputs=False):
        """`lml_batch_arrays` for scaled models (gpbo_lml_batch_scaled): row i is amplitudes[i] * k(length_scales[i]) + (whites[i] +
        noise) * I.  Values (n_theta,) and gradients (n_theta, n_ls + 2) in [log amplitude, log length_scale ..., log white], each
        lane bitwise what `lml(..., scaled=True)` returns for that row.  Model slots are not touched."""
        self._settle()
        ls = np.ascontiguousarray(np.atleast_2d(np.asarray(length_scales, dtype=np.float64)))
        n, n_ls = ls.shape
        amp = np.ascontiguousarray(np.asarray(amplitudes, dtype=np.float64).ravel())
        wh = np.ascontiguousarray(np.asarray(whites, dtype=np.float64).ravel())
        if amp.shape[0] != n or wh.shape[0] != n:
            raise ValueError("amplitudes and whites need one entry per row of length_scales")
        vals = np.zeros(n)
        grads = np.zeros((n, n_ls + 2))
        infos = _INT_ARRAYS.get(n)
        if infos is None:
            infos = _INT_ARRAYS[n] = C.c_int * n
        if reuse_inputs:
            xp = yp = None
        else:
            X = np.ascontiguousarray(X, dtype=np.float64)
            y_norm = np.ascontiguousarray(y_norm, dtype=np.float64).ravel()
            xp, yp = dptr(X), dptr(y_norm)
        rc = self._lib.gpbo_lml_batch_scaled(self._h, n, xp, yp, X.shape[0], X.shape[1], int(kernel), dptr(ls), n_ls, dptr(amp),
                                             dptr(wh), float(noise), int(bool(eval_gradient)), dptr(vals), dptr(grads), infos())
        if rc:
            self._check(rc)
        return vals, grads

    def lml_search_rounds_scaled(self, X, y_norm, kernel: int, n_ls: int, noise: float):
        """`lml_search_rounds` for a scaled model: `round(params (n <= 8, n_ls + 2)) -> (values (n,), gradients (n, n_ls + 2))`, a row
        of `params` and of the gradients in the device's order [amplitude, length_scale ..., white] (gpbo_lml_batch_scaled).  Same
        frame: inputs resident after the first round, arrays and pointers made once, results valid until the next round."""
        self._settle()
        X = np.ascontiguousarray(X, dtype=np.float64)
        y_norm = np.ascontiguousarray(y_norm, dtype=np.float64).ravel()
        N, d = int(X.shape[0]), int(X.shape[1])
        ls = np.ones((8, n_ls))
        amp, wh = np.ones(8), np.zeros(8)
        vals = np.zeros(8)
        grads = np.zeros((8, n_ls + 2))
        infos = (C.c_int * 8)()
        p_ls, p_amp, p_wh, p_vals, p_grads = dptr(ls), dptr(amp), dptr(wh), dptr(vals), dptr(grads)
        xp, yp = [dptr(X)], [dptr(y_norm)]
        call, h, kind, nz, ck = self._lib.gpbo_lml_batch_scaled, self._h, int(kernel), float(noise), self._check

        def one_round(params):
            n = params.shape[0]
            amp[:n] = params[:, 0]
            ls[:n] = params[:, 1:1 + n_ls]
            wh[:n] = params[:, 1 + n_ls]
            rc = call(h, n, xp[0], yp[0], N, d, kind, p_ls, n_ls, p_amp, p_wh, nz, 1, p_vals, p_grads, infos)
            xp[0] = yp[0] = None              # (X, y_norm stay referenced by this closure for the search's lifetime)
            if rc:
                ck(rc)
            return vals[:n], grads[:n]

        return one_round

    def _touch(self, slot: int) -> int:
        """Every call that rewrites a slot's factorisation bumps its serial; an estimator compares the serial it got
        from its last fit with `fit_serial(slot)` to know whether the slot still holds ITS model."""
        self._serial[int(slot)] = self._serial.get(int(slot), 0) + 1
        return self._serial[int(slot)]

    def fit_serial(self, slot: int = 0) -> int:
        return self._serial.get(int(slot), 0)

    def lml(self, X, y_norm, kernel: int, length_scale, noise: float, eval_gradient=True, slot: int = 0,
            amplitude: float = 1.0, white: float = 0.0, scaled=None):
        """(log marginal likelihood, d/dlog(length_scale)) at theta (sklearn _gpr.py:575-652). Clobbers the slot's fit.
        amplitude / white other than 1 / 0: of the scaled model amplitude * k + (white + noise) * I (gpbo_lml_scaled), the gradient
        in [log amplitude, log length_scale ..., log white].  scaled=True asks for that form whatever the two values are (a search
        over amplitude passes through 1)."""
        self._settle(slot)
        X, y_norm, ls = _model_arrays(X, y_norm, length_scale, check=False)
        val = C.c_double(0.0)
        self._scaled.pop(int(slot), None)
        self._n_obs.pop(int(slot), None)      # the slot is left unfitted
        if scaled or (scaled is None and _is_scaled(amplitude, white)):
            grad = np.zeros(ls.shape[0] + 2)
            info = C.c_int(0)
            self._touch(slot)
            rc = self._lib.gpbo_lml_scaled(self._h, int(slot), dptr(X), dptr(y_norm), X.shape[0], X.shape[1], int(kernel), dptr(ls),
                                           int(ls.shape[0]), float(amplitude), float(white), float(noise), int(bool(eval_gradient)),
                                           C.byref(val), dptr(grad), C.byref(info))
            self._check(rc, info.value)
            return (val.value, grad) if eval_gradient else val.value
        grad = np.zeros(ls.shape[0])
        info = C.c_int(0)
        self._touch(slot)
        rc = self._lib.gpbo_lml(self._h, int(slot), dptr(X), dptr(y_norm), X.shape[0], X.shape[1], int(kernel),
                                dptr(ls), int(ls.shape[0]), float(noise), int(bool(eval_gradient)), C.byref(val),
                                dptr(grad), C.byref(info))
        self._check(rc, info.value)
        return (val.value, grad) if eval_gradient else val.value

    def _square(self, fn, slot, n):
        out = np.empty((n, n), dtype=np.float64)
        self._check(fn(self._h, int(slot), dptr(out)))
        return out

    def get_K(self, n, slot=0):
        self._settle(slot)
        return self._square(self._lib.gpbo_get_K, slot, n)

    def get_L(self, n, slot=0):
        self._settle(slot)
        return self._square(self._lib.gpbo_get_L, slot, n)

    def get_Linv(self, n, slot=0):
        self._settle(slot)
        return self._square(self._lib.gpbo_get_Linv, slot, n)

    def get_alpha(self, n, slot=0):
        self._settle(slot)
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.gpbo_get_alpha(self._h, int(slot), dptr(out)))
        return out

    # -- candidates / posterior ------------------------------------------------------------------
    def set_candidates(self, Xc):
        Xc = np.ascontiguousarray(Xc, dtype=np.float64)
        if Xc.ndim != 2:
            raise ValueError("candidates must be 2-D (M, d)")
        self._check(self._lib.gpbo_set_candidates(self._h, dptr(Xc), Xc.shape[0], Xc.shape[1]))
        self.n_candidates = Xc.shape[0]

    def generate_candidates(self, M: int, lo, hi, seed: int):
        """Throughput mode: M x d uniforms in [lo, hi) generated on the device (Philox); NOT the reference's stream."""
        lo = np.ascontiguousarray(lo, dtype=np.float64).ravel()
        hi = np.ascontiguousarray(hi, dtype=np.float64).ravel()
        if lo.shape != hi.shape:
            raise ValueError("lo and hi must have the same length")
        self._check(self._lib.gpbo_generate_candidates(self._h, int(M), lo.shape[0], dptr(lo), dptr(hi),
                                                       int(seed) & 0xFFFFFFFFFFFFFFFF))
        self.n_candidates = int(M)
        self._cand_dim = lo.shape[0]

    def generate_candidates_trust_region(self, M: int, centre, lo, hi, sv, shift, bits: int, mask_threshold: int, mask_key: int):
        """Trust-region mode (gpbo_generate_candidates_trust_region; include/gpbo.h has the definition of an element): M rows equal
        to `centre` except where a Philox mask under `mask_key` marks a coordinate (word < `mask_threshold`, 0 .. 2^32; a row the
        mask leaves empty gets one column), which takes the row's point of the scrambled Sobol sequence `sv` (d, bits) uint32 /
        `shift` (d,) uint32 (turbo.sobol_tables) mapped into [lo, hi].  Quasi-random, NOT the reference's stream; draws nothing on
        the host.  ValueError: a shape or dtype that does not fit, and every refusal of the library (M, bits, the threshold, a
        non-finite or inverted box) — the resident candidates then stay as they were."""
        centre = np.ascontiguousarray(centre, dtype=np.float64)
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        if centre.ndim != 1 or centre.shape[0] < 1 or lo.shape != centre.shape or hi.shape != centre.shape:
            raise ValueError("centre, lo and hi must be 1-D of one length d >= 1")
        d = centre.shape[0]
        if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)):
            raise ValueError("bits must be an integer")
        sv, shift = np.asarray(sv), np.asarray(shift)
        if sv.dtype != np.uint32 or shift.dtype != np.uint32:
            raise ValueError("sv and shift must be uint32 arrays")
        if sv.shape != (d, int(bits)) or shift.shape != (d,):
            raise ValueError("sv must be (d, bits) and shift (d,)")
        mask_threshold, mask_key = int(mask_threshold), int(mask_key)
        if not 0 <= mask_threshold <= 2 ** 32:
            raise ValueError("mask_threshold must be in [0, 2^32]")
        sv, shift = np.ascontiguousarray(sv), np.ascontiguousarray(shift)
        u32 = C.POINTER(C.c_uint32)
        self._check(self._lib.gpbo_generate_candidates_trust_region(
            self._h, int(M), d, dptr(centre), dptr(lo), dptr(hi), sv.ctypes.data_as(u32), int(bits), shift.ctypes.data_as(u32),
            mask_threshold, mask_key & 0xFFFFFFFFFFFFFFFF))
        self.n_candidates = int(M)
        self._cand_dim = d

    def debug_generate_ms(self):
        """gpbo_debug_generate_ms (debug build): kernel ms of the last `generate_candidates` / `generate_candidates_trust_region`."""
        self._need_debug("gpbo_debug_generate_ms")
        ms = C.c_float(0.0)
        self._check(self._lib.gpbo_debug_generate_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def generate_candidates_like(self, M: int, lo, hi, random_state):
        """Index-parity mode: what `np.column_stack([random_state.uniform(lo[t], hi[t], M) for t in range(d)])`
        would be, generated on the device from `random_state`'s MT19937 state; `random_state` (a legacy
        np.random.RandomState) is advanced exactly as those draws would advance it."""
        lo = np.ascontiguousarray(lo, dtype=np.float64).ravel()
        hi = np.ascontiguousarray(hi, dtype=np.float64).ravel()
        if lo.shape != hi.shape:
            raise ValueError("lo and hi must have the same length")
        if not np.all(np.isfinite(hi - lo)):
            raise OverflowError("Range exceeds valid bounds")        # as RandomState.uniform
        name, key, pos, has_gauss, cached = random_state.get_state(legacy=True)
        if name != "MT19937":
            raise TypeError("generate_candidates_like needs an MT19937 RandomState")
        key = np.ascontiguousarray(key, dtype=np.uint32).copy()
        cpos = C.c_int(int(pos))
        self._check(self._lib.gpbo_generate_candidates_mt19937(
            self._h, int(M), lo.shape[0], dptr(lo), dptr(hi), key.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(cpos)))
        random_state.set_state((name, key, cpos.value, has_gauss, cached))
        self.n_candidates = int(M)
        self._cand_dim = lo.shape[0]

    def generate_candidate_rows_like(self, M: int, lo, hi, random_state, row_begin: int, row_end: int):
        """Rows [row_begin, row_end) of the matrix `generate_candidates_like(M, lo, hi, random_state)` would leave resident
        — this rank's block of ONE reference stream in the one-process-per-GPU mode (gpbo_generate_candidate_rows_mt19937:
        every column's run of rows starts at a jump-ahead state, nothing is generated twice, nothing crosses PCIe).  Every
        rank passes a RandomState in the same state; every rank's is advanced past the WHOLE matrix — on the host, by the
        same polynomial jump (advance_mt19937) — so the ranks' streams stay in step without exchanging anything."""
        lo = np.ascontiguousarray(lo, dtype=np.float64).ravel()
        hi = np.ascontiguousarray(hi, dtype=np.float64).ravel()
        if lo.shape != hi.shape:
            raise ValueError("lo and hi must have the same length")
        if not np.all(np.isfinite(hi - lo)):
            raise OverflowError("Range exceeds valid bounds")
        name, key, pos, has_gauss, cached = random_state.get_state(legacy=True)
        if name != "MT19937":
            raise TypeError("generate_candidate_rows_like needs an MT19937 RandomState")
        key = np.ascontiguousarray(key, dtype=np.uint32).copy()
        self._check(self._lib.gpbo_generate_candidate_rows_mt19937(
            self._h, int(M), lo.shape[0], int(row_begin), int(row_end), dptr(lo), dptr(hi),
            key.ctypes.data_as(C.POINTER(C.c_uint32)), int(pos), None, None))
        advance_mt19937(random_state, 2 * int(M) * lo.shape[0], self._lib)
        self.n_candidates = int(row_end) - int(row_begin)
        self._cand_dim = lo.shape[0]

    def get_candidate_rows(self, idx, d: int):
        idx = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int64)
        out = np.empty((idx.shape[0], d))
        self._check(self._lib.gpbo_get_candidate_rows(self._h, iptr(idx), idx.shape[0], dptr(out)))
        return out

    #: the column-group assembly below exists on a single device only (a device group samples mixed spaces on the host)
    mixed_device_sampling = True

    def generate_candidates_mixed(self, M: int, groups, random_state):
        """`space.random_sample(M, random_state)` of a space with float AND integer / categorical parameters, resident on
        the device: `groups` = [(kind, col0, ncols, lo, hi, param)] in key order (kind 0 float, 1 int, 2 categorical).
        Runs of float groups are generated on the device from the caller's MT19937 state (gpbo_generate_candidate_columns_
        mt19937; the state comes back advanced); an int / categorical parameter is drawn by ITS OWN `random_sample` on the
        host from exactly that position (RandomState.randint: masked rejection sampling, its word consumption depends on
        the values) and uploaded as its columns (gpbo_set_candidate_columns).  Matrix and RandomState end up bit for bit
        where the reference's loop (target_space.py:593-600) leaves them."""
        name, key, pos, has_gauss, cached = random_state.get_state(legacy=True)
        if name != "MT19937":
            raise TypeError("generate_candidates_mixed needs an MT19937 RandomState")
        M = max(1, int(M))
        d_total = sum(g[2] for g in groups)
        key = np.ascontiguousarray(key, dtype=np.uint32).copy()
        cpos = C.c_int(int(pos))
        i = 0
        while i < len(groups):
            kind, col0, ncols, lo, hi, param = groups[i]
            if kind == 0:
                j = i
                while j + 1 < len(groups) and groups[j + 1][0] == 0:      # a run of float parameters: one device call
                    j += 1
                lo_v = np.ascontiguousarray(np.concatenate([np.atleast_1d(g[3]) for g in groups[i:j + 1]]), dtype=np.float64)
                hi_v = np.ascontiguousarray(np.concatenate([np.atleast_1d(g[4]) for g in groups[i:j + 1]]), dtype=np.float64)
                if not np.all(np.isfinite(hi_v - lo_v)):
                    raise OverflowError("Range exceeds valid bounds")
                self._check(self._lib.gpbo_generate_candidate_columns_mt19937(
                    self._h, M, d_total, int(col0), int(lo_v.shape[0]), dptr(lo_v), dptr(hi_v),
                    key.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(cpos)))
                i = j + 1
                continue
            random_state.set_state((name, key, cpos.value, has_gauss, cached))
            vals = np.ascontiguousarray(np.asarray(param.random_sample(M, random_state), dtype=np.float64).reshape(M, ncols))
            self._check(self._lib.gpbo_set_candidate_columns(self._h, dptr(vals), M, d_total, int(col0), int(ncols)))
            _, key, p2, has_gauss, cached = random_state.get_state(legacy=True)
            key = np.ascontiguousarray(key, dtype=np.uint32).copy()
            cpos = C.c_int(int(p2))
            i += 1
        random_state.set_state((name, key, cpos.value, has_gauss, cached))
        self.n_candidates = M
        self._cand_dim = d_total

    def transform_candidates(self, groups):
        """TargetSpace.kernel_transform over the resident candidates, on the device (gpbo_transform_candidates): the
        posterior sees round()ed integer columns and the reference's one-hot categorical columns; get_candidate_rows keeps
        returning the rows as drawn."""
        n = len(groups)
        kinds = (C.c_int * n)(*[int(g[0]) for g in groups])
        col0 = (C.c_int * n)(*[int(g[1]) for g in groups])
        ncols = (C.c_int * n)(*[int(g[2]) for g in groups])
        self._check(self._lib.gpbo_transform_candidates(self._h, n, kinds, col0, ncols))

    def posterior(self, slot=0, y_mean=0.0, y_std=1.0, fetch=True):
        """mu, sd for the resident candidates (sklearn _gpr.py:443-494). fetch=False keeps them on device."""
        self._settle(slot)
        M = self.n_candidates
        mu = np.empty(M) if fetch else None
        sd = np.empty(M) if fetch else None
        self._check(self._lib.gpbo_posterior(self._h, int(slot), float(y_mean), float(y_std), dptr(mu), dptr(sd)))
        return mu, sd

    def posterior_refresh(self, slot=0, y_mean=0.0, y_std=1.0, fetch=True, return_route=False):
        """`posterior()` after `fit_append()`: where the slot's resident posterior was valid for the current candidates and only
        row appends (at most 16 rows, no padding crossing) have touched the slot since, it is UPDATED — one k* generation against
        the appended rows of W, O(M N d) — instead of recomputed (gpbo_posterior_refresh); in every other case this is
        `posterior()`.  return_route=True: (mu, sd, route), route 1 = the update ran, 0 = the full pass."""
        self._settle(slot)
        M = self.n_candidates
        mu = np.empty(M) if fetch else None
        sd = np.empty(M) if fetch else None
        route = C.c_int(0)
        self._check(self._lib.gpbo_posterior_refresh(self._h, int(slot), float(y_mean), float(y_std), dptr(mu), dptr(sd),
                                                     C.byref(route)))
        return (mu, sd, int(route.value)) if return_route else (mu, sd)

    def _path_inputs(self, who, omega, phase, weights, eps, slot):
        """The draws of `sample_paths` / `ascend_paths` as contiguous float64 arrays, checked against each other and against the
        slot's fit; with the fit's (observations, dimensions)."""
        self._settle(slot)
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        phase = np.ascontiguousarray(phase, dtype=np.float64).ravel()
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        eps = np.ascontiguousarray(eps, dtype=np.float64)
        if omega.ndim != 2 or weights.ndim != 2 or eps.ndim != 2:
            raise ValueError(f"{who}: omega (F, d), weights (S, F) and eps (S, N) must be 2-D")
        F, S = omega.shape[0], weights.shape[0]
        if phase.shape[0] != F or weights.shape[1] != F or eps.shape[0] != S:
            raise ValueError(f"{who}: phase (F,), weights (S, F) and eps (S, N) do not fit omega (F, d)")
        shape = self._n_obs.get(int(slot))
        if shape is None:
            raise _lib.GpboError(f"{who}: model slot has not been fitted")
        if (eps.shape[1], omega.shape[1]) != shape:
            raise ValueError(f"{who}: eps (S, {eps.shape[1]}) / omega (F, {omega.shape[1]}) do not fit the slot's model of "
                             f"{shape[0]} observations in {shape[1]} dimensions")
        return omega, phase, weights, eps, shape

    def sample_paths(self, omega, phase, weights, eps, slot=0, y_mean=0.0, y_std=1.0, index_offset=0, return_values=False):
        """S = weights.shape[0] <= 16 function draws from the slot's posterior over the resident candidates and each draw's
        maximiser (gpbo_sample_paths: Matheron's rule over F random Fourier features; include/gpbo.h has the formulas).
        omega (F, d): frequencies in turns per unit of the length-scaled input; phase (F,): turns; weights (S, F); eps (S, N): the
        noise draws in normalised-target units.  Returns (best_idx (S,) int64, best_val (S,), values (S, M) or None).  A reader:
        the slot's fit, its resident posterior and the candidates stay as they were."""
        omega, phase, weights, eps, _ = self._path_inputs("sample_paths", omega, phase, weights, eps, slot)
        F, S = omega.shape[0], weights.shape[0]
        M = max(int(self.n_candidates), 0)
        best_idx = np.empty(max(S, 1), dtype=np.int64)
        best_val = np.empty(max(S, 1))
        values = np.empty((S, M)) if return_values and S >= 1 and M >= 1 else None
        self._check(self._lib.gpbo_sample_paths(self._h, int(slot), float(y_mean), float(y_std), int(S), int(F), dptr(omega),
                                                dptr(phase), dptr(weights), dptr(eps), int(index_offset), iptr(best_idx),
                                                dptr(best_val), dptr(values)))
        return best_idx[:S], best_val[:S], values

    def sample_paths_constrained(self, draws, lb, ub, y_mean, y_std, index_offset=0, return_values=False):
        """Constrained Thompson sampling over the resident candidates (gpbo_sample_paths_constrained; include/gpbo.h has the rule):
        `draws` is a list of 1 + C tuples (omega, phase, weights, eps) as `sample_paths` takes them, entry j for slot j — the
        objective in slot 0, constraint j in slot j; all with the same S and F.  lb / ub (C,), y_mean / y_std (1 + C,).  Per draw s
        the best objective value among the candidates the constraint draws call feasible, else the candidate of least total
        violation.  Returns (idx (S,) int64, val (S,), viol (S,), feasible (S,) bool, values (1 + C, S, M) or None, viol_all
        (S, M) or None).  A reader, as `sample_paths`."""
        who = "sample_paths_constrained"
        draws = list(draws)
        n_slots = len(draws)
        lb = np.ascontiguousarray(lb, dtype=np.float64).ravel()
        ub = np.ascontiguousarray(ub, dtype=np.float64).ravel()
        y_mean = np.ascontiguousarray(y_mean, dtype=np.float64).ravel()
        y_std = np.ascontiguousarray(y_std, dtype=np.float64).ravel()
        if n_slots < 2 or any(len(t) != 4 for t in draws):
            raise ValueError(f"{who}: draws must be a list of 1 + C tuples (omega, phase, weights, eps), C >= 1")
        if lb.shape[0] != n_slots - 1 or ub.shape[0] != n_slots - 1 or y_mean.shape[0] != n_slots or y_std.shape[0] != n_slots:
            raise ValueError(f"{who}: lb / ub must have {n_slots - 1} entries, y_mean / y_std {n_slots}")
        if n_slots > _lib.MAX_MODELS:
            raise ValueError(f"{who}: n_constraints out of range [1, {_lib.MAX_MODELS - 1}]")
        parts = [self._path_inputs(who, *draws[j], j) for j in range(n_slots)]
        F, S = parts[0][0].shape[0], parts[0][2].shape[0]
        if any(p[0].shape[0] != F or p[2].shape[0] != S for p in parts):
            raise ValueError(f"{who}: every slot's draws must have the same S and F")
        omega = np.ascontiguousarray(np.concatenate([p[0].ravel() for p in parts]))
        phase = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
        weights = np.ascontiguousarray(np.concatenate([p[2].ravel() for p in parts]))
        eps = np.ascontiguousarray(np.concatenate([p[3].ravel() for p in parts]))
        M = max(int(self.n_candidates), 0)
        n = max(S, 1)
        best_idx = np.empty(n, dtype=np.int64)
        best_val, best_viol = np.empty(n), np.empty(n)
        feasible = np.zeros(n, dtype=np.int32)
        keep = return_values and S >= 1 and M >= 1
        values = np.empty((n_slots, S, M)) if keep else None
        viol_all = np.empty((S, M)) if keep else None
        self._check(self._lib.gpbo_sample_paths_constrained(
            self._h, n_slots - 1, dptr(y_mean), dptr(y_std), dptr(lb), dptr(ub), int(S), int(F), dptr(omega), dptr(phase),
            dptr(weights), dptr(eps), int(index_offset), iptr(best_idx), dptr(best_val), dptr(best_viol),
            feasible.ctypes.data_as(C.POINTER(C.c_int)), dptr(values), dptr(viol_all)))
        return best_idx[:S], best_val[:S], best_viol[:S], feasible[:S].astype(bool), values, viol_all

    def ascend_paths(self, omega, phase, weights, eps, box_lo, box_hi, n_starts=4, starts=None, max_iter=-1, slot=0, y_mean=0.0,
                     y_std=1.0, index_offset=0, return_gradient=False):
        """The S draws of `sample_paths`, each climbed from K starts to a local maximiser inside [box_lo, box_hi] in ONE launch
        (gpbo_ascend_paths: a workgroup per (draw, start), evaluations and the projected L-BFGS of `polish_seeds` inside it;
        include/gpbo.h has the formulas).  starts=None: K = n_starts and the starts are each draw's K best resident candidates
        (what `sample_paths` evaluates; `best_idx` / `best_val` are its answers, bit for bit).  starts (S, K, d): no candidates
        are needed, `best_idx` / `best_val` are None.  max_iter < 0: 15 000 iterations; 0: the value and gradient at the (clipped)
        starts, no search.  Returns a dict:
            x (S, K, d), f (S, K) = the draw's value at x, status (S, K) 0 / 1 converged, 2 iteration limit or non-finite start, 3
            line search exhausted, n_eval (S, K), start_idx (S, K) candidate indices (+ index_offset) or -1, g (S, K, d) with
            return_gradient, best_idx, best_val;
            winner (S,), x_best (S, d), f_best (S,): per draw the run with the largest finite f, ties to the lowest start
            (winner -1, NaN rows: no run of the draw has a finite value).
        A reader: the slot's fit, its resident posterior and the candidates stay as they were."""
        omega, phase, weights, eps, shape = self._path_inputs("ascend_paths", omega, phase, weights, eps, slot)
        F, S = omega.shape[0], weights.shape[0]
        d = int(shape[1])
        lo = np.ascontiguousarray(box_lo, dtype=np.float64).ravel()
        hi = np.ascontiguousarray(box_hi, dtype=np.float64).ravel()
        if lo.shape[0] != d or hi.shape[0] != d:
            raise ValueError(f"ascend_paths: box_lo / box_hi must have {d} entries")
        if starts is not None:
            starts = np.ascontiguousarray(starts, dtype=np.float64)
            if starts.ndim != 3 or starts.shape[0] != S or starts.shape[2] != d:
                raise ValueError(f"ascend_paths: starts must be (S = {S}, K, d = {d})")
            K = int(starts.shape[1])
        else:
            K = int(n_starts)
        R = max(S, 1) * max(K, 1)
        best_idx = np.empty(max(S, 1), dtype=np.int64) if starts is None else None
        best_val = np.empty(max(S, 1)) if starts is None else None
        x = np.empty((R, d))
        f = np.empty(R)
        g = np.empty((R, d)) if return_gradient else None
        status = np.zeros(R, dtype=np.int32)
        n_eval = np.zeros(R, dtype=np.int32)
        start_idx = np.empty(R, dtype=np.int64)
        self._check(self._lib.gpbo_ascend_paths(self._h, int(slot), float(y_mean), float(y_std), int(S), int(F), dptr(omega),
                                                dptr(phase), dptr(weights), dptr(eps), K, dptr(starts), dptr(lo), dptr(hi),
                                                int(max_iter), int(index_offset), iptr(best_idx), dptr(best_val), dptr(x), dptr(f),
                                                dptr(g), status.ctypes.data_as(C.POINTER(C.c_int)),
                                                n_eval.ctypes.data_as(C.POINTER(C.c_int)), iptr(start_idx)))
        out = {"x": x.reshape(S, K, d), "f": f.reshape(S, K), "status": status.reshape(S, K), "n_eval": n_eval.reshape(S, K),
               "start_idx": start_idx.reshape(S, K), "best_idx": None if best_idx is None else best_idx[:S],
               "best_val": None if best_val is None else best_val[:S]}
        if return_gradient:
            out["g"] = g.reshape(S, K, d)
        out.update(path_winners(out["x"], out["f"]))
        return out

    def predict(self, Xc, slot=0, y_mean=0.0, y_std=1.0):
        self.set_candidates(Xc)
        return self.posterior(slot, y_mean, y_std, fetch=True)

    def take_negative_variance_flag(self):
        """True when a posterior / predict since the last call clipped a NEGATIVE variance — sklearn's warning
        condition (_gpr.py:479-485); clears the flag (gpbo_take_negative_variance_flag)."""
        seen = C.c_int(0)
        self._check(self._lib.gpbo_take_negative_variance_flag(self._h, C.byref(seen)))
        return bool(seen.value)

    def predict_cov(self, Xc, slot=0, y_mean=0.0, y_std=1.0):
        """(mu (M,), cov (M,M)) as GaussianProcessRegressor.predict(return_cov=True) (gpbo_predict_cov)."""
        self._settle(slot)
        Xc = np.ascontiguousarray(Xc, dtype=np.float64)
        M, d = Xc.shape
        mu, cov = np.empty(M), np.empty((M, M))
        self._check(self._lib.gpbo_predict_cov(self._h, int(slot), dptr(Xc), M, d, float(y_mean), float(y_std),
                                               dptr(mu), dptr(cov)))
        self.n_candidates = M
        self._resident = False
        return mu, cov

    def predict_grad(self, Xc, slot=0, y_mean=0.0, y_std=1.0):
        """(mu (M,), sd (M,), dmu (M,d), dsd (M,d)) for a small host batch (M <= 256): gpbo_predict_grad."""
        self._settle(slot)
        Xc = np.ascontiguousarray(Xc, dtype=np.float64)
        M, d = Xc.shape
        mu, sd = np.empty(M), np.empty(M)
        dmu, dsd = np.empty((M, d)), np.empty((M, d))
        self._check(self._lib.gpbo_predict_grad(self._h, int(slot), dptr(Xc), M, d, float(y_mean), float(y_std),
                                                dptr(mu), dptr(sd), dptr(dmu), dptr(dsd)))
        self.n_candidates = M
        self._resident = False       # (device groups: the first device's candidate buffer was re-used)
        return mu, sd, dmu, dsd

    def polish_seeds(self, acq: int, param: float, y_max, lb, ub, y_means, y_stds, seeds, box, max_iter: int = 0):
        """gpbo_polish_seeds: the local searches of one suggest() in one call.  Returns (x (S,d), f (S,), status (S,) — 0/1
        converged, 2 SciPy's success = False —, rounds)."""
        self._settle()
        seeds = np.ascontiguousarray(seeds, dtype=np.float64)
        S, d = seeds.shape
        lb = np.ascontiguousarray(np.atleast_1d(np.asarray(lb, dtype=np.float64))) if lb is not None else None
        ub = np.ascontiguousarray(np.atleast_1d(np.asarray(ub, dtype=np.float64))) if ub is not None else None
        n_c = 0 if lb is None else lb.shape[0]
        ym = np.ascontiguousarray(np.atleast_1d(np.asarray(y_means, dtype=np.float64)))
        ys = np.ascontiguousarray(np.atleast_1d(np.asarray(y_stds, dtype=np.float64)))
        if ym.shape[0] != 1 + n_c or ys.shape[0] != 1 + n_c:
            raise ValueError("one (y_mean, y_std) per model slot")
        lo = np.ascontiguousarray(np.asarray(box, dtype=np.float64)[:, 0])
        hi = np.ascontiguousarray(np.asarray(box, dtype=np.float64)[:, 1])
        x = np.empty((S, d))
        f = np.empty(S)
        status = np.zeros(S, dtype=np.int32)
        self.last_polish = {"nit": np.zeros(S, dtype=np.int32), "nfev": np.zeros(S, dtype=np.int32)}
        rounds = C.c_int(0)
        self._check(self._lib.gpbo_polish_seeds(self._h, int(acq), float(param), float(0.0 if y_max is None else y_max), n_c,
                                                dptr(lb), dptr(ub), dptr(ym), dptr(ys), dptr(seeds), S, d, dptr(lo), dptr(hi),
                                                int(max_iter), dptr(x), dptr(f), status.ctypes.data_as(C.POINTER(C.c_int)),
                                                C.byref(rounds), self.last_polish["nit"].ctypes.data_as(C.POINTER(C.c_int)),
                                                self.last_polish["nfev"].ctypes.data_as(C.POINTER(C.c_int))))
        self.last_polish["rounds"] = rounds.value
        self.n_candidates = S        # the candidate buffer held the rounds' trial points (at most S of them)
        self._resident = False
        return x, f, status, rounds.value

    @staticmethod
    def _groups_arrays(groups):
        n = len(groups)
        return ((C.c_int * n)(*[int(g[0]) for g in groups]), (C.c_int * n)(*[int(g[1]) for g in groups]),
                (C.c_int * n)(*[int(g[2]) for g in groups]), n)

    def evolve_mixed(self, acq: int, param: float, y_max, y_mean: float, y_std: float, groups, bounds, init, random_state,
                     maxiter: int = 1000):
        """gpbo_evolve_mixed: `DifferentialEvolutionSolver(func, bounds, init=init, polish=False, rng=random_state).solve()` of a
        mixed-space smart stage (SciPy 1.15, best1bin) with the walk and its evaluations — -base_acq of slot 0's posterior at
        kernel_transform(x), `groups` = [(kind, col0, ncols, ...)] as for transform_candidates — on the device.  Returns
        (x, fun, nit, nfev, success); `random_state` (a legacy MT19937 RandomState) is left where SciPy's solver would leave it."""
        self._settle(0)
        name, key, pos, has_gauss, cached = random_state.get_state(legacy=True)
        if name != "MT19937":
            raise TypeError("evolve_mixed needs an MT19937 RandomState")
        bounds = np.asarray(bounds, dtype=np.float64)
        lo, hi = np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])
        init = np.ascontiguousarray(init, dtype=np.float64)
        S, D = init.shape
        kinds, col0, ncols, n = self._groups_arrays(groups)
        key = np.ascontiguousarray(key, dtype=np.uint32).copy()
        cpos = C.c_int(int(pos))
        x = np.empty(D)
        f, nit, nfev, ok = C.c_double(0.0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.gpbo_evolve_mixed(
            self._h, int(acq), float(param), float(0.0 if y_max is None else y_max), float(y_mean), float(y_std), n, kinds, col0,
            ncols, dptr(lo), dptr(hi), dptr(init), S, D, int(maxiter), key.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(cpos),
            dptr(x), C.byref(f), C.byref(nit), C.byref(nfev), C.byref(ok)))
        random_state.set_state((name, key, cpos.value, has_gauss, cached))
        return x, f.value, nit.value, nfev.value, bool(ok.value)

    def debug_evolve_eval(self, acq: int, param: float, y_max, y_mean: float, y_std: float, groups, points):
        """gpbo_debug_evolve_eval: the device walk's objective at each row of `points` (n, D)."""
        self._need_debug("debug_evolve_eval")
        self._settle(0)
        points = np.ascontiguousarray(points, dtype=np.float64)
        n, D = points.shape
        kinds, col0, ncols, ng = self._groups_arrays(groups)
        out = np.empty(n)
        self._check(self._lib.gpbo_debug_evolve_eval(self._h, int(acq), float(param), float(0.0 if y_max is None else y_max),
                                                     float(y_mean), float(y_std), ng, kinds, col0, ncols, dptr(points), n, D,
                                                     dptr(out)))
        return out

    def debug_evolve_walk(self, weights, targets, groups, bounds, init, key, pos, maxiter=1000, budget=256,
                          nan_below=-np.inf, inf_above=np.inf):
        """gpbo_debug_evolve_walk: the device walk over the analytic objective (tests/de_walk.py: analytic).  Returns a dict
        with x, fun, nit, nfev, success, key, pos, launches."""
        self._need_debug("debug_evolve_walk")
        bounds = np.asarray(bounds, dtype=np.float64)
        lo, hi = np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])
        init = np.ascontiguousarray(init, dtype=np.float64)
        S, D = init.shape
        w = np.ascontiguousarray(weights, dtype=np.float64)
        a = np.ascontiguousarray(targets, dtype=np.float64)
        kinds, col0, ncols, n = self._groups_arrays(groups)
        key = np.ascontiguousarray(key, dtype=np.uint32).copy()
        cpos = C.c_int(int(pos))
        x = np.empty(D)
        f, nit, nfev, ok, launches = C.c_double(0.0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.gpbo_debug_evolve_walk(
            self._h, dptr(w), dptr(a), float(nan_below), float(inf_above), n, kinds, col0, ncols, dptr(lo), dptr(hi), dptr(init),
            S, D, int(maxiter), int(budget), key.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(cpos), dptr(x), C.byref(f),
            C.byref(nit), C.byref(nfev), C.byref(ok), C.byref(launches)))
        return {"x": x, "fun": f.value, "nit": nit.value, "nfev": nfev.value, "success": bool(ok.value), "key": key,
                "pos": cpos.value, "launches": launches.value}

    # -- acquisition -----------------------------------------------------------------------------
    def acq_argbest(self, acq: int, param: float, y_max: float = 0.0, lb=None, ub=None, k_seeds: int = 0,
                    index_offset: int = 0, return_values: bool = False):
        """ys = -acq [* p_c]; returns (best_idx, best_val, seed_idx, seed_val, ys|None)."""
        lb, ub, n_c, seed_idx, seed_val, ys = _argbest_frame(lb, ub, k_seeds, self.n_candidates if return_values else None)
        best_idx, best_val = C.c_int64(0), C.c_double(0.0)
        rc = self._lib.gpbo_acq_argbest(self._h, int(acq), float(param), float(y_max if y_max is not None else 0.0),
                                        n_c, dptr(lb), dptr(ub), int(k_seeds), int(index_offset),
                                        C.byref(best_idx), C.byref(best_val), iptr(seed_idx), dptr(seed_val),
                                        dptr(ys))
        self._check(rc)
        return best_idx.value, best_val.value, seed_idx[:k_seeds], seed_val[:k_seeds], ys

    def mes_argbest(self, y_star, k_seeds: int = 0, index_offset: int = 0, return_values: bool = False):
        """Max-value entropy search over the resident candidates (gpbo_mes_argbest; include/gpbo.h has the formulas): ys = -a, a
        the mean over the S <= 64 sampled maxima `y_star` (raw target units) of h((y* - mu) / sd), from slot 0's resident
        posterior.  Returns (best_idx, best_val, seed_idx, seed_val, ys|None) as `acq_argbest`.  A reader: the fit, the resident
        posterior and the candidates stay as they were."""
        y_star = np.ascontiguousarray(np.atleast_1d(np.asarray(y_star, dtype=np.float64)))
        if y_star.ndim != 1:
            raise ValueError("mes_argbest: y_star must be one-dimensional")
        k_seeds = int(k_seeds)
        _lb, _ub, _n_c, seed_idx, seed_val, ys = _argbest_frame(None, None, k_seeds, self.n_candidates if return_values else None)
        best_idx, best_val = C.c_int64(0), C.c_double(0.0)
        self._check(self._lib.gpbo_mes_argbest(self._h, int(y_star.shape[0]), dptr(y_star), k_seeds, int(index_offset),
                                               C.byref(best_idx), C.byref(best_val), iptr(seed_idx), dptr(seed_val), dptr(ys)))
        return best_idx.value, best_val.value, seed_idx[:k_seeds], seed_val[:k_seeds], ys

    def kg_argbest(self, points, k_seeds: int = 0, index_offset: int = 0, y_mean: float = 0.0, y_std: float = 1.0,
                   return_values: bool = False, return_point_means: bool = False):
        """Knowledge gradient over the resident candidates (gpbo_kg_argbest; include/gpbo.h has the formulas): ys = -KG, the
        expected rise of the maximum of the posterior mean over the candidate itself and the J <= 64 reference `points` (J, d),
        parameter space, from observing the candidate — from slot 0's resident posterior; `y_mean` / `y_std` are those of the pass
        that left it.  Returns (best_idx, best_val, seed_idx, seed_val, ys|None) as `acq_argbest`, with `return_point_means` a
        sixth entry: the posterior mean at the points (J,).  A reader: the fit, the resident posterior and the candidates stay as
        they were.  A fit pending on slot 0 (`overlapped_fits`) is waited for first, as every reader of a slot does; the new fit has
        no posterior over the candidates, so the call is then refused as such."""
        points = np.ascontiguousarray(np.asarray(points, dtype=np.float64))
        if points.ndim != 2:
            raise ValueError("kg_argbest: points must be two-dimensional (J, d)")
        k_seeds = int(k_seeds)
        self._settle(0)
        _lb, _ub, _n_c, seed_idx, seed_val, ys = _argbest_frame(None, None, k_seeds, self.n_candidates if return_values else None)
        mu_points = np.empty(points.shape[0]) if return_point_means else None
        best_idx, best_val = C.c_int64(0), C.c_double(0.0)
        self._check(self._lib.gpbo_kg_argbest(self._h, dptr(points), int(points.shape[0]), int(points.shape[1]), float(y_mean),
                                              float(y_std), k_seeds, int(index_offset), C.byref(best_idx), C.byref(best_val),
                                              iptr(seed_idx), dptr(seed_val), dptr(ys), dptr(mu_points)))
        out = (best_idx.value, best_val.value, seed_idx[:k_seeds], seed_val[:k_seeds], ys)
        return out + (mu_points,) if return_point_means else out

    def ehvi_argbest(self, levels, cell_lo, cell_hi, k_seeds: int = 0, index_offset: int = 0, return_values: bool = False):
        """Expected hypervolume improvement over the resident candidates (gpbo_ehvi_argbest; include/gpbo.h has the formulas, the
        conventions and the order of the sum): ys = -EHVI for m = 2 or 3 maximised objectives, objective j from slot j's resident
        posterior (raw target units).  `levels`: m rows of strictly increasing values, the last +inf (a sequence of m 1-D arrays, or
        one (m, L) array whose rows end at their first +inf); `cell_lo` / `cell_hi` (K, m): the boxes of the non-dominated region
        as level indices, lo < hi (`multiobjective.box_decomposition` makes all three).  Returns (best_idx, best_val, seed_idx,
        seed_val, ys|None) as `mes_argbest`.  A reader: the fits, the resident posteriors and the candidates stay as they were.  A
        fit pending on one of the slots (`overlapped_fits`) is waited for first, as every reader of a slot does; the new fit has no
        posterior over the candidates, so the call is then refused as such."""
        m, n_levels, table, lo8, hi8 = self._ehvi_frame("ehvi_argbest", levels, cell_lo, cell_hi)
        k_seeds = int(k_seeds)
        for j in range(m):
            self._settle(j)
        _lb, _ub, _n_c, seed_idx, seed_val, ys = _argbest_frame(None, None, k_seeds, self.n_candidates if return_values else None)
        best_idx, best_val = C.c_int64(0), C.c_double(0.0)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.gpbo_ehvi_argbest(self._h, m, n_levels.ctypes.data_as(C.POINTER(C.c_int)), dptr(table), int(lo8.shape[0]),
                                                lo8.ctypes.data_as(u8), hi8.ctypes.data_as(u8), k_seeds, int(index_offset),
                                                C.byref(best_idx), C.byref(best_val), iptr(seed_idx), dptr(seed_val), dptr(ys)))
        return best_idx.value, best_val.value, seed_idx[:k_seeds], seed_val[:k_seeds], ys

    @staticmethod
    def _ehvi_frame(who, levels, cell_lo, cell_hi):
        """The levels and boxes of `ehvi_argbest` / `cehvi_argbest` as the library reads them: (m, n_levels (m,) intc, the level table
        (m, GPBO_MAX_EHVI_LEVELS), cell_lo, cell_hi (K, m) uint8), else ValueError."""
        rows = [np.asarray(r, dtype=np.float64).ravel() for r in levels]
        m = len(rows)
        rows = [r[:int(np.argmax(np.isposinf(r))) + 1] if np.isposinf(r).any() else r for r in rows]      # a row ends at its first +inf
        if not 2 <= m <= _lib.MAX_EHVI_OBJECTIVES:
            raise ValueError(f"{who}: levels must have 2 or 3 rows, one per objective")
        if any(not 2 <= r.shape[0] <= _lib.MAX_EHVI_LEVELS for r in rows):
            raise ValueError(f"{who}: a row of levels needs 2 to {_lib.MAX_EHVI_LEVELS} entries")
        lo = np.ascontiguousarray(np.asarray(cell_lo, dtype=np.int64))
        hi = np.ascontiguousarray(np.asarray(cell_hi, dtype=np.int64))
        if lo.ndim != 2 or lo.shape != hi.shape or lo.shape[1] != m:
            raise ValueError(f"{who}: cell_lo and cell_hi must both be (K, m)")
        if lo.size and (min(lo.min(), hi.min()) < 0 or max(lo.max(), hi.max()) > 255):
            raise ValueError(f"{who}: a cell index is not a level index")
        table = np.zeros((m, _lib.MAX_EHVI_LEVELS))
        n_levels = np.zeros(m, dtype=np.intc)
        for j, r in enumerate(rows):
            table[j, :r.shape[0]] = r
            n_levels[j] = r.shape[0]
        return m, n_levels, table, np.ascontiguousarray(lo.astype(np.uint8)), np.ascontiguousarray(hi.astype(np.uint8))

    def cehvi_argbest(self, levels, cell_lo, cell_hi, lb, ub, log_form: bool = True, k_seeds: int = 0, index_offset: int = 0,
                      return_values: bool = False):
        """Feasibility-weighted expected hypervolume improvement over the resident candidates (gpmo_cehvi_argbest; include/gpmo.h has
        the formulas, the conventions and the order of every sum): `ehvi_argbest`'s EHVI E for the same `levels` / `cell_lo` /
        `cell_hi`, and s = the sum of the C constraints' log feasibilities — constraint j from slot m + j's resident posterior and
        (lb[j], ub[j]), infinite sides allowed.  log_form: ys = -(log E + s); else ys = -(E exp(s)).  Returns (best_idx, best_val,
        seed_idx, seed_val, ys|None) as `ehvi_argbest`.  A reader: the fits, the resident posteriors and the candidates stay as they
        were; a fit pending on one of the slots is waited for first."""
        who = "cehvi_argbest"
        m, n_levels, table, lo8, hi8 = self._ehvi_frame(who, levels, cell_lo, cell_hi)
        k_seeds = int(k_seeds)
        lb, ub, n_c, seed_idx, seed_val, ys = _argbest_frame(lb, ub, k_seeds, self.n_candidates if return_values else None)
        if n_c < 1:
            raise ValueError(f"{who}: lb and ub must name at least one constraint")
        for j in range(min(m + n_c, _lib.MAX_MODELS)):
            self._settle(j)
        best_idx, best_val = C.c_int64(0), C.c_double(0.0)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.gpmo_cehvi_argbest(self._h, m, n_levels.ctypes.data_as(C.POINTER(C.c_int)), dptr(table), int(lo8.shape[0]),
                                                 lo8.ctypes.data_as(u8), hi8.ctypes.data_as(u8), n_c, dptr(lb), dptr(ub),
                                                 int(bool(log_form)), k_seeds, int(index_offset), C.byref(best_idx),
                                                 C.byref(best_val), iptr(seed_idx), dptr(seed_val), dptr(ys)))
        return best_idx.value, best_val.value, seed_idx[:k_seeds], seed_val[:k_seeds], ys

    @staticmethod
    def _greedy_groups(who, draws, message):
        """G of `draws` — per slot a list of tuples (omega, phase, weights, eps), G >= 1 of them in every slot —, else ValueError:
        `message` for lists that are not that, then G's range."""
        G = len(draws[0])
        if G < 1 or any(len(groups) != G for groups in draws) or any(len(t) != 4 for groups in draws for t in groups):
            raise ValueError(f"{who}: {message}")
        if G > _lib.MAX_QNEI_GROUPS:
            raise ValueError(f"{who}: n_groups out of range [1, {_lib.MAX_QNEI_GROUPS}]")
        return G

    def _greedy_inputs(self, who, slotted):
        """The draws of a greedy call as it hands them down: `slotted`, a list of (slot, that slot's groups), each group checked as
        `_path_inputs` checks it against its slot and all of one S and F.  Returns (omega, phase, weights, eps, S, F, d), the four
        flat and concatenated slot-major, then group-major (csrc/greedy.h: GreedyDraws)."""
        parts = [self._path_inputs(who, *t, slot) for slot, groups in slotted for t in groups]
        F, S = parts[0][0].shape[0], parts[0][2].shape[0]
        if any(p[0].shape[0] != F or p[2].shape[0] != S for p in parts):
            raise ValueError(f"{who}: every group's draws must have the same S and F")
        omega, phase, weights, eps = (np.ascontiguousarray(np.concatenate([p[k].ravel() for p in parts])) for k in range(4))
        return omega, phase, weights, eps, int(S), int(F), int(parts[0][4][1])

    @staticmethod
    def _greedy_points(who, points, d, noun, count, whose):
        """A greedy call's point set (`noun`: pending / base; `count`: what its docstring calls their number) as (float64 array or
        None, number of points); it must be (n, d) to fit `whose` (the slot's model / the slots' models)."""
        if points is None:
            return None, 0
        points = np.ascontiguousarray(np.asarray(points, dtype=np.float64))
        if points.ndim != 2:
            raise ValueError(f"{who}: {noun} must be two-dimensional ({count}, d)")
        n = int(points.shape[0])
        if n and points.shape[1] != d:
            raise ValueError(f"{who}: {noun} ({count}, {points.shape[1]}) does not fit the {whose} in {d} dimensions")
        return (points, n) if n else (None, 0)

    def qnei_greedy(self, groups, q, noisy=True, y_best=0.0, pending=None, slot=0, y_mean=0.0, y_std=1.0, index_offset=0,
                    return_values=False, return_keys=False):
        """A batch of q resident candidates by greedy noisy expected improvement over T joint posterior draws (gpbo_qnei_greedy;
        include/gpbo.h has the formulas, the conventions and the order of every sum).  `groups`: a list of G <= 16 tuples (omega,
        phase, weights, eps) as `sample_paths` takes them, all with the same S <= 16 and F; draw t = g S + s is `sample_paths`' draw s
        of group g, the same bits.  noisy: every draw's incumbent is its own maximum over the training points; else `y_best` (finite)
        is every draw's.  pending (P <= 64, d) or None: points suggested but not yet observed, absorbed into the incumbents first.
        Returns (pick_idx (q,) int64, pick_gain (q,), baseline (T,), values (T, M) or None, keys (q, M) or None).  A reader, as
        `sample_paths`."""
        who = "qnei_greedy"
        groups = list(groups)
        G = self._greedy_groups(who, [groups], "groups must be a non-empty list of tuples (omega, phase, weights, eps)")
        omega, phase, weights, eps, S, F, d = self._greedy_inputs(who, [(slot, groups)])
        pending, P = self._greedy_points(who, pending, d, "pending", "P", "slot's model")
        q = int(q)
        T, M = G * S, max(int(self.n_candidates), 0)
        n = max(q, 1)
        pick_idx = np.empty(n, dtype=np.int64)
        pick_gain = np.empty(n)
        baseline = np.empty(max(T, 1))
        values = np.empty((T, M)) if return_values and T >= 1 and M >= 1 else None
        keys = np.empty((q, M)) if return_keys and q >= 1 and M >= 1 else None
        self._check(self._lib.gpbo_qnei_greedy(self._h, int(slot), float(y_mean), float(y_std), G, int(S), int(F), dptr(omega),
                                               dptr(phase), dptr(weights), dptr(eps), int(bool(noisy)), float(y_best), dptr(pending),
                                               P, int(d), q, int(index_offset), iptr(pick_idx), dptr(pick_gain), dptr(baseline),
                                               dptr(values), dptr(keys)))
        return pick_idx[:q], pick_gain[:q], baseline[:T], values, keys

    def qnehvi_greedy(self, draws, q, ref, base=None, y_mean=(0.0, 0.0), y_std=(1.0, 1.0), index_offset=0, return_values=False,
                      return_keys=False, return_fronts=False):
        """A batch of q resident candidates by greedy noisy expected hypervolume improvement over T joint posterior draws of two
        objectives (gpbo_qnhvi_greedy; include/gpbo.h has the formulas, the conventions and the order of every sum).  `draws`:
        two lists, objective j's (slot j's) G <= 16 tuples (omega, phase, weights, eps) as `qnei_greedy` takes them, all with the
        same G, S <= 16 and F.  ref (2,) finite; base (n_base <= 16384, d) or None: the observed points followed by the pending
        ones — every draw's front is built from the draw's values there.  y_mean / y_std: (2,) per objective.
        Returns a dict: "index" (q,) int64, "gain" (q,), and — None unless asked for — "values" (2, T, M), "base_values"
        (2, T, n_base) (with `return_values`), "keys" (q, M), "front_size" (2, T) int32 and "fronts" (2, T, 128, 2) (before the
        first pick | after the last; rows past a front's size are unspecified).  A front of more than 128 points is
        NotImplementedError.  A reader, as `sample_paths`."""
        who = "qnehvi_greedy"
        draws = [list(g) for g in draws]
        if len(draws) != 2:
            raise ValueError(f"{who}: draws must hold two lists of groups, one per objective")
        G = self._greedy_groups(who, draws, "each objective needs the same non-empty list of tuples (omega, phase, weights, eps)")
        omega, phase, weights, eps, S, F, d = self._greedy_inputs(who, list(enumerate(draws)))
        base, B = self._greedy_points(who, base, d, "base", "n_base", "slots' models")
        ref = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).ravel())
        y_mean = np.ascontiguousarray(np.asarray(y_mean, dtype=np.float64).ravel())
        y_std = np.ascontiguousarray(np.asarray(y_std, dtype=np.float64).ravel())
        if ref.shape[0] != 2 or y_mean.shape[0] != 2 or y_std.shape[0] != 2:
            raise ValueError(f"{who}: ref, y_mean and y_std must hold one value per objective")
        q = int(q)
        T, M = G * S, max(int(self.n_candidates), 0)
        n = max(q, 1)
        L = _lib.MAX_QNEHVI_FRONT
        pick_idx = np.empty(n, dtype=np.int64)
        pick_gain = np.empty(n)
        values = np.empty((2, T, M)) if return_values and M >= 1 else None
        base_values = np.empty((2, T, B)) if return_values else None
        keys = np.empty((q, M)) if return_keys and q >= 1 and M >= 1 else None
        front_size = np.zeros((2, T), dtype=np.int32) if return_fronts else None
        fronts = np.empty((2, T, L, 2)) if return_fronts else None
        self._check(self._lib.gpbo_qnhvi_greedy(self._h, dptr(y_mean), dptr(y_std), G, int(S), int(F), dptr(omega), dptr(phase),
                                                 dptr(weights), dptr(eps), dptr(ref), dptr(base), B, int(d), q, int(index_offset),
                                                 iptr(pick_idx), dptr(pick_gain),
                                                 None if front_size is None else front_size.ctypes.data_as(C.POINTER(C.c_int)),
                                                 dptr(fronts), dptr(values), dptr(base_values) if B else None, dptr(keys)))
        return {"index": pick_idx[:q], "gain": pick_gain[:q], "values": values, "base_values": base_values, "keys": keys,
                "front_size": front_size, "fronts": fronts}

    def cnei_greedy(self, draws, q, lb, ub, y_floor, base=None, y_mean=None, y_std=None, index_offset=0, return_values=False,
                    return_keys=False):
        """A batch of q resident candidates by greedy noisy expected improvement UNDER CONSTRAINTS, over T joint posterior draws of
        the objective and every constraint (gpbo_cnei_greedy; include/gpbo.h has the rule).  `draws`: 1 + C lists, slot j's G <= 16
        tuples (omega, phase, weights, eps) as `qnei_greedy` takes them — the objective in slot 0, constraint j in slot j —, all
        with the same G, S <= 16 and F.  lb / ub (C,); y_mean / y_std (1 + C,) (None: 0 / 1 everywhere); y_floor finite: the
        incumbent of a draw in which no base point is feasible.  base (n_base <= 16384, d) or None: the observed points followed
        by the pending ones.
        Returns a dict: "index" (q,) int64, "gain" (q,), "feasible" (q,) the share of draws that call each pick feasible,
        "baseline" (T,), and — None unless asked for — "values" (1 + C, T, M) the RAW draws, "viol" (T, M), "base_values"
        (1 + C, T, n_base) (with `return_values`), "keys" (q, M).  A reader, as `sample_paths`."""
        who = "cnei_greedy"
        draws = [list(g) for g in draws]
        n_slots = len(draws)
        if n_slots < 2:
            raise ValueError(f"{who}: draws must hold 1 + C lists of groups, C >= 1: the objective's, then each constraint's")
        if n_slots > _lib.MAX_MODELS:
            raise ValueError(f"{who}: n_constraints out of range [1, {_lib.MAX_MODELS - 1}]")
        G = self._greedy_groups(who, draws, "each slot needs the same non-empty list of tuples (omega, phase, weights, eps)")
        lb = np.ascontiguousarray(lb, dtype=np.float64).ravel()
        ub = np.ascontiguousarray(ub, dtype=np.float64).ravel()
        y_mean = np.zeros(n_slots) if y_mean is None else np.ascontiguousarray(y_mean, dtype=np.float64).ravel()
        y_std = np.ones(n_slots) if y_std is None else np.ascontiguousarray(y_std, dtype=np.float64).ravel()
        if lb.shape[0] != n_slots - 1 or ub.shape[0] != n_slots - 1 or y_mean.shape[0] != n_slots or y_std.shape[0] != n_slots:
            raise ValueError(f"{who}: lb / ub must have {n_slots - 1} entries, y_mean / y_std {n_slots}")
        omega, phase, weights, eps, S, F, d = self._greedy_inputs(who, list(enumerate(draws)))
        base, B = self._greedy_points(who, base, d, "base", "n_base", "slots' models")
        q = int(q)
        T, M = G * S, max(int(self.n_candidates), 0)
        n = max(q, 1)
        pick_idx = np.empty(n, dtype=np.int64)
        pick_gain, pick_feasible = np.empty(n), np.empty(n)
        baseline = np.empty(max(T, 1))
        keep = return_values and T >= 1 and M >= 1
        values = np.empty((n_slots, T, M)) if keep else None
        viol = np.empty((T, M)) if keep else None
        base_values = np.empty((n_slots, T, B)) if return_values else None
        keys = np.empty((q, M)) if return_keys and q >= 1 and M >= 1 else None
        self._check(self._lib.gpbo_cnei_greedy(self._h, n_slots - 1, dptr(y_mean), dptr(y_std), dptr(lb), dptr(ub), G, int(S), int(F),
                                               dptr(omega), dptr(phase), dptr(weights), dptr(eps), float(y_floor), dptr(base), B,
                                               int(d), q, int(index_offset), iptr(pick_idx), dptr(pick_gain), dptr(pick_feasible),
                                               dptr(baseline), dptr(values), dptr(viol), dptr(base_values) if B else None,
                                               dptr(keys)))
        return {"index": pick_idx[:q], "gain": pick_gain[:q], "feasible": pick_feasible[:q], "baseline": baseline[:T],
                "values": values, "viol": viol, "base_values": base_values, "keys": keys}

    def cnehvi_greedy(self, draws, q, lb, ub, ref, base=None, y_mean=None, y_std=None, index_offset=0, return_values=False,
                      return_keys=False, return_fronts=False):
        """A batch of q resident candidates by greedy noisy expected hypervolume improvement of two objectives UNDER NOISY
        CONSTRAINTS, over T joint posterior draws of every slot (gpmo_cnhvi_greedy; include/gpmo.h has the rule).  `draws`: 2 + C
        lists, slot j's G <= 16 tuples (omega, phase, weights, eps) as `qnei_greedy` takes them — the objectives in slots 0 and 1,
        constraint j in slot 2 + j —, all with the same G, S <= 16 and F.  lb / ub (C,); ref (2,) finite; y_mean / y_std (2 + C,)
        (None: 0 / 1 everywhere); base (n_base <= 16384, d) or None: the observed points followed by the pending ones.
        Returns a dict as `cnei_greedy`'s — "index" (q,) int64, "gain" (q,), "feasible" (q,) the share of draws that call each pick
        feasible, and, None unless asked for, "values" (2 + C, T, M) the RAW draws, "viol" (T, M), "base_values" (2 + C, T, n_base)
        (with `return_values`), "keys" (q, M) — plus the fronts as `qnehvi_greedy`'s: "front_size" (2, T) int32 and "fronts"
        (2, T, 128, 2).  A front of more than 128 points is NotImplementedError.  A reader, as `sample_paths`."""
        who = "cnehvi_greedy"
        draws = [list(g) for g in draws]
        n_slots = len(draws)
        if n_slots < 3:
            raise ValueError(f"{who}: draws must hold 2 + C lists of groups, C >= 1: the two objectives', then each constraint's")
        if n_slots > _lib.MAX_MODELS:
            raise ValueError(f"{who}: n_constraints out of range [1, {_lib.MAX_MODELS - 2}]")
        G = self._greedy_groups(who, draws, "each slot needs the same non-empty list of tuples (omega, phase, weights, eps)")
        lb = np.ascontiguousarray(lb, dtype=np.float64).ravel()
        ub = np.ascontiguousarray(ub, dtype=np.float64).ravel()
        ref = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).ravel())
        y_mean = np.zeros(n_slots) if y_mean is None else np.ascontiguousarray(y_mean, dtype=np.float64).ravel()
        y_std = np.ones(n_slots) if y_std is None else np.ascontiguousarray(y_std, dtype=np.float64).ravel()
        if lb.shape[0] != n_slots - 2 or ub.shape[0] != n_slots - 2 or y_mean.shape[0] != n_slots or y_std.shape[0] != n_slots:
            raise ValueError(f"{who}: lb / ub must have {n_slots - 2} entries, y_mean / y_std {n_slots}")
        if ref.shape[0] != 2:
            raise ValueError(f"{who}: ref must hold one value per objective")
        omega, phase, weights, eps, S, F, d = self._greedy_inputs(who, list(enumerate(draws)))
        base, B = self._greedy_points(who, base, d, "base", "n_base", "slots' models")
        q = int(q)
        T, M = G * S, max(int(self.n_candidates), 0)
        n = max(q, 1)
        L = _lib.MAX_QNEHVI_FRONT
        pick_idx = np.empty(n, dtype=np.int64)
        pick_gain, pick_feasible = np.empty(n), np.empty(n)
        keep = return_values and T >= 1 and M >= 1
        values = np.empty((n_slots, T, M)) if keep else None
        viol = np.empty((T, M)) if keep else None
        base_values = np.empty((n_slots, T, B)) if return_values else None
        keys = np.empty((q, M)) if return_keys and q >= 1 and M >= 1 else None
        front_size = np.zeros((2, T), dtype=np.int32) if return_fronts else None
        fronts = np.empty((2, T, L, 2)) if return_fronts else None
        self._check(self._lib.gpmo_cnhvi_greedy(self._h, n_slots - 2, dptr(y_mean), dptr(y_std), dptr(lb), dptr(ub), G, int(S), int(F),
                                                dptr(omega), dptr(phase), dptr(weights), dptr(eps), dptr(ref), dptr(base), B, int(d),
                                                q, int(index_offset), iptr(pick_idx), dptr(pick_gain), dptr(pick_feasible),
                                                None if front_size is None else front_size.ctypes.data_as(C.POINTER(C.c_int)),
                                                dptr(fronts), dptr(values), dptr(viol), dptr(base_values) if B else None, dptr(keys)))
        return {"index": pick_idx[:q], "gain": pick_gain[:q], "feasible": pick_feasible[:q], "values": values, "viol": viol,
                "base_values": base_values, "keys": keys, "front_size": front_size, "fronts": fronts}

    def debug_cnhvi_stage_ms(self):
        """gpbo_debug_cnhvi_stage_ms (debug build): kernel ms of the last `cnehvi_greedy`'s stages, (draws, front build, greedy steps)."""
        self._need_debug("gpbo_debug_cnhvi_stage_ms")
        ms = (C.c_float * 3)()
        self._check(self._lib.gpbo_debug_cnhvi_stage_ms(self._h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    def debug_cnei_stage_ms(self):
        """gpbo_debug_cnei_stage_ms (debug build): kernel ms of the last `cnei_greedy`'s stages, (draws and baselines, greedy steps)."""
        self._need_debug("gpbo_debug_cnei_stage_ms")
        ms = (C.c_float * 2)()
        self._check(self._lib.gpbo_debug_cnei_stage_ms(self._h, ms))
        return float(ms[0]), float(ms[1])

    def debug_qnehvi_fronts(self, base_values, ref, insert_values=None):
        """gpbo_debug_qnehvi_fronts (debug build): the product's front build on base_values (2, T, n) against ref (2,), then its
        update rule with insert_values (2, T, n_insert), in order: (front_size (T,) int32, fronts (T, 128, 2))."""
        self._need_debug("gpbo_debug_qnehvi_fronts")
        bv = np.ascontiguousarray(np.asarray(base_values, dtype=np.float64))
        if bv.ndim != 3 or bv.shape[0] != 2:
            raise ValueError("debug_qnehvi_fronts: base_values must be (2, T, n)")
        T, n = int(bv.shape[1]), int(bv.shape[2])
        n_insert = 0
        iv = None
        if insert_values is not None:
            iv = np.ascontiguousarray(np.asarray(insert_values, dtype=np.float64))
            if iv.ndim != 3 or iv.shape[:2] != (2, T):
                raise ValueError("debug_qnehvi_fronts: insert_values must be (2, T, n_insert)")
            n_insert = int(iv.shape[2])
        ref = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).ravel())
        size = np.zeros(max(T, 1), dtype=np.int32)
        fronts = np.empty((max(T, 1), _lib.MAX_QNEHVI_FRONT, 2))
        self._check(self._lib.gpbo_debug_qnehvi_fronts(self._h, T, n, dptr(bv) if n else None, dptr(ref), n_insert,
                                                       dptr(iv) if n_insert else None, size.ctypes.data_as(C.POINTER(C.c_int)),
                                                       dptr(fronts)))
        return size[:T], fronts[:T]

    def debug_qnehvi_stage_ms(self):
        """gpbo_debug_qnehvi_stage_ms (debug build): kernel ms of the last `qnehvi_greedy`'s stages, (draws, front build, greedy
        steps)."""
        self._need_debug("gpbo_debug_qnehvi_stage_ms")
        ms = (C.c_float * 3)()
        self._check(self._lib.gpbo_debug_qnehvi_stage_ms(self._h, ms))
        return tuple(float(v) for v in ms)

    def debug_ehvi_ms(self):
        """gpbo_debug_ehvi_ms (debug build): kernel ms of the last `ehvi_argbest`'s value kernel (tables and cell sum)."""
        self._need_debug("gpbo_debug_ehvi_ms")
        ms = C.c_float(0.0)
        self._check(self._lib.gpbo_debug_ehvi_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def debug_kg_lines(self, a, b):
        """gpbo_debug_kg_lines (debug build): the envelope of `kg_argbest` alone on R sets of n lines, a / b (R, n) intercepts /
        slopes: (R,) E[max_j (a_j + b_j Z)] - max_j a_j."""
        self._need_debug("gpbo_debug_kg_lines")
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float64)))
        b = np.ascontiguousarray(np.atleast_2d(np.asarray(b, dtype=np.float64)))
        if a.shape != b.shape:
            raise ValueError("debug_kg_lines: a and b must have one shape (R, n_lines)")
        out = np.empty(a.shape[0])
        self._check(self._lib.gpbo_debug_kg_lines(self._h, dptr(a), dptr(b), int(a.shape[0]), int(a.shape[1]), dptr(out)))
        return out

    def debug_kg_stage_ms(self):
        """gpbo_debug_kg_stage_ms (debug build): kernel ms of the last `kg_argbest`'s stages, (points, covariances, envelopes)."""
        self._need_debug("gpbo_debug_kg_stage_ms")
        ms = (C.c_float * 3)()
        self._check(self._lib.gpbo_debug_kg_stage_ms(self._h, ms))
        return tuple(float(v) for v in ms)

    def debug_qnei_stage_ms(self):
        """gpbo_debug_qnei_stage_ms (debug build): kernel ms of the last `qnei_greedy`'s stages, (draws and baselines, greedy steps)."""
        self._need_debug("gpbo_debug_qnei_stage_ms")
        ms = (C.c_float * 2)()
        self._check(self._lib.gpbo_debug_qnei_stage_ms(self._h, ms))
        return tuple(float(v) for v in ms)

    # -- timing / probes (debug_* and the latency / hybrid probes need GpEngine(debug=True)) ----------------------------
    def _need_debug(self, what: str):
        if not getattr(self, "debug", False):
            raise _lib.GpboError(f"{what} is a debug entry point: create the engine with GpEngine(device, debug=True) (libgpbo_dbg.so)")

    def debug_fail_next_acq(self):
        """Fault injection (debug build): the next comm_acq_argbest behaves as if this rank's local pass had failed."""
        self._need_debug("gpbo_debug_fail_next_acq")
        self._check(self._lib.gpbo_debug_fail_next_acq(self._h))

    def set_timing(self, on: bool):
        """gpbo_set_timing: whether the calls record their HIP event pairs (what `last_timings()` reads; a new engine does).
        A record is a marker packet on the stream: a 0.1 ms step notices its eight."""
        self._check(self._lib.gpbo_set_timing(self._h, 1 if on else 0))
        self.timing = bool(on)

    def last_timings(self) -> dict:
        ms = (C.c_float * 8)()
        self._check(self._lib.gpbo_last_timings(self._h, ms, 8))
        return {n: float(ms[i]) for i, n in enumerate(TIMING_NAMES)}

    def debug_cholesky(self, A, variant=3, iters=1):
        """The device Cholesky alone (gpbo_debug_cholesky): returns (L lower n x n, dinv [n/64][64][64], stamps[16], ms, info)."""
        self._need_debug("gpbo_debug_cholesky")
        A = np.ascontiguousarray(A, dtype=np.float64)
        n = A.shape[0]
        Lo = np.empty((n, n))
        dinv = np.empty((n // 64, 64, 64))
        stamps = np.zeros(16, dtype=np.int64)
        ms, info = C.c_double(0.0), C.c_int(0)
        self._check(self._lib.gpbo_debug_cholesky(self._h, dptr(A), n, int(variant), int(iters), dptr(Lo), dptr(dinv),
                                                  stamps.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(ms), C.byref(info)))
        return np.tril(Lo), dinv, stamps, ms.value, info.value

    def debug_select(self, ys, k, variant=1, iters=0):
        """The selection launches alone over `ys` (gpbo_debug_select): (idx (k,), vals (k,), first_nan, ms per selection)."""
        self._need_debug("gpbo_debug_select")
        ys = np.ascontiguousarray(ys, dtype=np.float64)
        idx = np.empty(int(k), dtype=np.int64)
        vals = np.empty(int(k))
        first_nan, ms = C.c_int64(-1), C.c_float(0.0)
        self._check(self._lib.gpbo_debug_select(self._h, dptr(ys), ys.shape[0], int(k), int(variant), int(iters),
                                                idx.ctypes.data_as(C.POINTER(C.c_int64)), dptr(vals), C.byref(first_nan), C.byref(ms)))
        return idx, vals, int(first_nan.value), float(ms.value)

    def latency_probe(self, n=16):
        self._need_debug("gpbo_debug_latency_probe")
        out = np.zeros(32, dtype=np.int64)
        self._check(self._lib.gpbo_debug_latency_probe(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), int(n)))
        return out[:n]

    def debug_gemm(self, A, B, C_in=None, alpha=1.0, beta=0.0, b_trans=False):
        self._need_debug("gpbo_debug_gemm")
        A = np.ascontiguousarray(A, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        m, k = A.shape
        n = B.shape[0] if b_trans else B.shape[1]
        Cm = np.zeros((m, n)) if C_in is None else np.ascontiguousarray(C_in, dtype=np.float64).copy()
        self._check(self._lib.gpbo_debug_gemm(self._h, m, n, k, float(alpha), dptr(A), dptr(B), int(b_trans),
                                              float(beta), dptr(Cm)))
        return Cm

    # the stages of the int8 posterior pass alone (posterior_i8.hip; S = 7 digit planes, operands as raw int8 in fragment order).
    # I8_S and _i8_wd_bytes restate i8_digits.h's I8_S and i8_wd_block: tests/test_i8_reference_host.py holds them to the header.
    I8_S = 7

    @staticmethod
    def _i8_wd_bytes(NP: int) -> int:
        q = NP // 64
        return (NP // 16 + 2 * q * (q - 1)) * GpEngine.I8_S * 64 * 16

    def debug_i8_pack_w(self, W, N: int):
        """wd_row_scale_kernel + wd_pack_kernel on W (NP x NP): (digit buffer int8, row exponents int32, row scales)."""
        self._need_debug("gpbo_debug_i8_pack_w")
        W = np.ascontiguousarray(W, dtype=np.float64)
        NP = W.shape[0]
        if W.ndim != 2 or W.shape[1] != NP or NP % 64 or not 64 <= NP <= 16384:
            raise ValueError("debug_i8_pack_w: W must be NP x NP, NP a multiple of 64 in [64, 16384]")
        Wd = np.empty(self._i8_wd_bytes(NP), dtype=np.int8)
        wexp = np.empty(NP, dtype=np.int32)
        wscale = np.empty(NP)
        self._check(self._lib.gpbo_debug_i8_pack_w(self._h, dptr(W), int(N), NP, Wd.ctypes.data_as(C.c_void_p),
                                                   wexp.ctypes.data_as(C.POINTER(C.c_int)), dptr(wscale)))
        return Wd, wexp, wscale

    def debug_i8_kstar_digits(self, NP: int, m0: int, ldk: int):
        """The k* generation of slot 0's model (padded size NP) for the resident candidates [m0, m0 + ldk): (digit slab int8,
        fp64 slab [NP][ldk], partial means [2][ceil(NP / 256)][ldk]: digit branch, fp64 branch).  The library refuses an NP that is
        not the fitted model's before it writes."""
        self._need_debug("gpbo_debug_i8_kstar_digits")
        if NP % 64 or not 64 <= NP <= 16384 or ldk < 64:
            raise ValueError("debug_i8_kstar_digits: NP a multiple of 64 in [64, 16384], ldk >= 64")
        Kd = np.empty(int(ldk) * NP * self.I8_S, dtype=np.int8)
        kst = np.empty((NP, int(ldk)))
        mu_part = np.empty((2, (NP + 255) // 256, int(ldk)))
        self._check(self._lib.gpbo_debug_i8_kstar_digits(self._h, int(NP), int(m0), int(ldk), Kd.ctypes.data_as(C.c_void_p), dptr(kst),
                                                         dptr(mu_part)))
        return Kd, kst, mu_part

    def debug_i8_gemm(self, Wd, wscale, Kd, NP: int, M: int):
        """posterior_i8_kernel on raw operands: part [ceil(NP / 128)][M]."""
        self._need_debug("gpbo_debug_i8_gemm")
        Wd = np.ascontiguousarray(Wd, dtype=np.int8)
        Kd = np.ascontiguousarray(Kd, dtype=np.int8)
        wscale = np.ascontiguousarray(wscale, dtype=np.float64)
        if NP % 64 or not 64 <= NP <= 16384 or M % 64 or M < 64:
            raise ValueError("debug_i8_gemm: NP a multiple of 64 in [64, 16384], M a multiple of 64")
        if Wd.size != self._i8_wd_bytes(NP) or Kd.size != M * NP * self.I8_S or wscale.size != NP:
            raise ValueError("debug_i8_gemm: operand sizes do not match NP and M")
        part = np.empty(((NP + 127) // 128, M))
        self._check(self._lib.gpbo_debug_i8_gemm(self._h, Wd.ctypes.data_as(C.c_void_p), dptr(wscale), Kd.ctypes.data_as(C.c_void_p),
                                                 NP, M, dptr(part)))
        return part

    def gemm_bench(self, m, n, k, b_trans=True, a_trans=False, lower_only=False, iters=10) -> dict:
        self._need_debug("gpbo_debug_gemm_bench")
        out = np.zeros(2)
        self._check(self._lib.gpbo_debug_gemm_bench(self._h, int(m), int(n), int(k), int(b_trans), int(a_trans),
                                                    int(lower_only), int(iters), dptr(out)))
        return {"ms": float(out[0]), "tflops": float(out[1])}

    def mfma_f64_peak(self, iters=20000) -> float:
        out = C.c_double(0.0)
        self._check(self._lib.gpbo_mfma_f64_peak(self._h, int(iters), C.byref(out)))
        return out.value

    def mfma_f64_probe(self, iters=20000, waves_per_simd=1, mode=0) -> dict:
        out = np.zeros(4)
        self._check(self._lib.gpbo_mfma_f64_probe(self._h, int(iters), int(waves_per_simd), int(mode), dptr(out)))
        return {"tflops": out[0], "cycles_per_mfma": out[1], "shader_mhz": out[2], "ms": out[3]}

    def hybrid_probe(self, iters=2000, cfg=2) -> dict:
        self._need_debug("gpbo_hybrid_probe")
        out = np.zeros(3)
        self._check(self._lib.gpbo_hybrid_probe(self._h, int(iters), int(cfg), dptr(out)))
        return {"ms": out[0], "mfma_tflops": out[1], "valu_tflops": out[2]}

    def hbm_copy_peak(self, nbytes=1 << 30) -> float:
        out = C.c_double(0.0)
        self._check(self._lib.gpbo_hbm_copy_peak(self._h, int(nbytes), C.byref(out)))
        return out.value

    # -- RCCL ----------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = _lib.load_library()
        buf = C.create_string_buffer(128)
        rc = lib.gpbo_comm_unique_id(buf)
        if rc != _lib.GPBO_OK:
            _lib.raise_for_status(lib, None, rc)
        return buf.raw

    def comm_init(self, unique_id: bytes, world_size: int, rank: int):
        assert len(unique_id) == 128
        self._check(self._lib.gpbo_comm_init(self._h, unique_id, int(world_size), int(rank)))
        self.world_size, self.rank = int(world_size), int(rank)

    def comm_acq_argbest(self, acq: int, param: float, y_max: float = 0.0, lb=None, ub=None, k_seeds: int = 0,
                         index_offset: int = 0, return_values: bool = False):
        """`acq_argbest` over the union of every rank's shard (gpbo_comm_acq_argbest): the shard's records are packed on
        the device, all-gathered over RCCL and merged identically on every rank.  Same return tuple; `ys` is this
        rank's shard."""
        lb, ub, n_c, seed_idx, seed_val, ys = _argbest_frame(lb, ub, k_seeds, self.n_candidates if return_values else None)
        best_idx, best_val = C.c_int64(0), C.c_double(0.0)
        rc = self._lib.gpbo_comm_acq_argbest(self._h, int(acq), float(param), float(y_max if y_max is not None else 0.0),
                                             n_c, dptr(lb), dptr(ub), int(k_seeds), int(index_offset),
                                             C.byref(best_idx), C.byref(best_val), iptr(seed_idx), dptr(seed_val), dptr(ys))
        self._check(rc)
        return best_idx.value, best_val.value, seed_idx[:k_seeds], seed_val[:k_seeds], ys

    def comm_allreduce_max(self, value: float) -> float:
        """Drain this rank's stream, then the maximum of `value` over all ranks (barrier + max-over-ranks timing)."""
        v = np.array([float(value)])
        self._check(self._lib.gpbo_comm_allreduce_max(self._h, dptr(v)))
        return float(v[0])

    def comm_allgather_best(self, vals, idxs):
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        idxs = np.ascontiguousarray(idxs, dtype=np.int64)
        n = vals.shape[0]
        all_vals = np.empty(n * self.world_size)
        all_idxs = np.empty(n * self.world_size, dtype=np.int64)
        self._check(self._lib.gpbo_comm_allgather_best(self._h, dptr(vals), iptr(idxs), n, dptr(all_vals),
                                                       iptr(all_idxs)))
        return all_vals, all_idxs


class GroupEngine(GpEngine):
    """G GPUs of one node behind the GpEngine interface, in ONE process (gpbo_group_*).

    The model slots are replicated (every device factorises the same GP — deterministic, so the factors are identical),
    the resident candidate matrix is block-partitioned in index order (device r keeps rows [r M / G, (r + 1) M / G)),
    and `acq_argbest` ends in ONE exchange: each shard's 1 + k (value, global index) records, packed on the device,
    all-gathered over RCCL and merged identically on every rank.  Everything that is not M-scaled — single-point and
    finite-difference predicts of the host optimisers, the LML evaluations of the theta search, the parity accessors —
    runs on the first device's context through the inherited methods.

    `devices` listing a GPU more than once gives virtual ranks (several shards on one GPU, merged on the host): the
    single-GPU rehearsal of the sharded path.  `collective` says which exchange the group uses.
    """

    def __init__(self, devices):
        devices = [int(x) for x in devices]
        if not devices:
            raise ValueError("GroupEngine needs at least one device")
        self._lib = _lib.load_library()
        arr = (C.c_int * len(devices))(*devices)
        g = C.c_void_p()
        rc = self._lib.gpbo_group_create(len(devices), arr, C.byref(g))
        if rc != _lib.GPBO_OK:
            _lib.raise_for_status(self._lib, None, rc)
        self._g = g
        self._h = self._member(0)     # borrowed: the first device's context
        self.devices = devices
        self.device = devices[0]
        # as a single engine's: fits are synchronous on every device and scaled kernels refused, so _pending_fits and _scaled stay
        # empty and overlapped_fits() is a plain block; _resident: the shards are in place (a small predict on device 0 clobbers them)
        self._init_state()
        self.world_size = len(devices)
        self.collective = self._lib.gpbo_group_collective(g).decode()
        self._orphans = []          # arrays of failed calls (see _gcheck)

    def close(self):
        if getattr(self, "_g", None):
            self._lib.gpbo_group_destroy(self._g)
            self._g = None
            self._h = None

    def _gcheck(self, rc, info=0, borrowed=()):
        """`borrowed`: the host arrays the call handed to the group's worker threads.  After a failed call — above all one that
        missed its deadline, where a worker may still be inside the job (include/gpbo.h: the caller's arrays must outlive the
        group then) — they stay referenced until close()."""
        if rc != _lib.GPBO_OK:
            if borrowed:
                self._orphans.append(borrowed)
            _lib.raise_for_status(self._lib, None, rc, info, group=self._g)

    def _member(self, r: int):
        """The context of member r (borrowed from the group, as `_h` is member 0's)."""
        return C.c_void_p(self._lib.gpbo_group_ctx(self._g, int(r)))

    def per_device_info(self) -> list:
        """`device_info()` of every device of the group: PCI bus id, rank / world and what RCCL says its communicator has
        (ncclCommCount) — a multi-GPU bench line quotes these, not what the launcher asked for."""
        out = []
        for r in range(self.world_size):
            buf = C.create_string_buffer(1024)
            self._check(self._lib.gpbo_device_info(self._member(r), buf, 1024))
            out.append(json.loads(buf.value.decode()))
        return out

    def set_timing(self, on: bool):
        for r in range(self.world_size):
            self._check(self._lib.gpbo_set_timing(self._member(r), 1 if on else 0))
        self.timing = bool(on)

    def per_device_timings(self) -> list:
        """`last_timings()` of every device of the group (HIP events on each device's own stream): a straggler shows here."""
        out = []
        for r in range(self.world_size):
            ms = (C.c_float * 8)()
            self._check(self._lib.gpbo_last_timings(self._member(r), ms, 8))
            out.append({n: float(ms[i]) for i, n in enumerate(TIMING_NAMES)})
        return out

    def synchronize(self):
        self._gcheck(self._lib.gpbo_group_synchronize(self._g))

    @contextlib.contextmanager
    def overlapped_fits(self):
        """gpbo_group_fit factorises on every device and returns when all are done: nothing is left in flight, so the
        block is a plain block (the single-device engine overlaps the slots' fits here)."""
        yield self

    def take_negative_variance_flag(self):
        """OR of the clipped-variance flags of ALL member devices (a sharded posterior runs on every one of them);
        clears each.  Same warning condition as the single-device path (sklearn _gpr.py:479-485)."""
        any_seen = False
        for r in range(self.world_size):
            seen = C.c_int(0)
            self._check(self._lib.gpbo_take_negative_variance_flag(self._member(r), C.byref(seen)))
            any_seen = any_seen or bool(seen.value)
        return any_seen

    def member_timings(self, rank: int) -> dict:
        ms = (C.c_float * 8)()
        self._check(self._lib.gpbo_last_timings(self._member(rank), ms, 8))
        return {n: float(ms[i]) for i, n in enumerate(TIMING_NAMES)}

    def shard(self, rank: int) -> tuple[int, int]:
        a, b = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        self._gcheck(self._lib.gpbo_group_shard(self._g, int(rank), iptr(a), iptr(b)))
        return int(a[0]), int(b[0])

    # -- replicated model ----------------------------------------------------------------------
    def _refuse_scaled(self, amplitude, white):
        if _is_scaled(amplitude, white):
            raise NotImplementedError("a device group has no scaled-kernel (ConstantKernel / WhiteKernel) path")

    def lml(self, X, y_norm, kernel: int, length_scale, noise: float, eval_gradient=True, slot: int = 0,
            amplitude: float = 1.0, white: float = 0.0, scaled=None):
        if scaled:
            self._refuse_scaled(0.0, 0.0)
        self._refuse_scaled(amplitude, white)
        return super().lml(X, y_norm, kernel, length_scale, noise, eval_gradient, slot)

    def fit(self, X, y_norm, kernel: int, length_scale, noise: float, slot: int = 0, precision: int = F64,
            amplitude: float = 1.0, white: float = 0.0):
        self._refuse_scaled(amplitude, white)
        X, y_norm, ls = _model_arrays(X, y_norm, length_scale)
        info = C.c_int(0)
        self._touch(slot)
        rc = self._lib.gpbo_group_fit(self._g, int(slot), dptr(X), dptr(y_norm), X.shape[0], X.shape[1], int(kernel),
                                      dptr(ls), int(ls.shape[0]), float(noise), int(precision), C.byref(info))
        self._gcheck(rc, info.value, borrowed=(X, y_norm, ls, info))
        return self._touch(slot)

    def fit_append(self, x_new, y_norm, slot: int = 0, amplitude: float = 1.0, white: float = 0.0):
        self._refuse_scaled(amplitude, white)
        y_norm = np.ascontiguousarray(y_norm, dtype=np.float64).ravel()
        x_new = np.ascontiguousarray(x_new, dtype=np.float64)
        if x_new.ndim != 2:
            raise ValueError("x_new must be 2-D (n_new, n_features)")
        info = C.c_int(0)
        self._touch(slot)
        rc = self._lib.gpbo_group_fit_append(self._g, int(slot), dptr(x_new) if x_new.shape[0] else None, x_new.shape[0],
                                             x_new.shape[1], dptr(y_norm), y_norm.shape[0], C.byref(info))
        self._gcheck(rc, info.value, borrowed=(x_new, y_norm, info))
        return self._touch(slot)

    def lml_batch_scaled_arrays(self, X, y_norm, kernel: int, length_scales, amplitudes, whites, noise: float, eval_gradient=True,
                                reuse_inputs=False):
        self._refuse_scaled(0.0, 0.0)      # (gpbo_group_lml_batch takes unit models only)

    def lml_search_rounds_scaled(self, X, y_norm, kernel: int, n_ls: int, noise: float):
        self._refuse_scaled(0.0, 0.0)

    def lml_batch_arrays(self, X, y_norm, kernel: int, length_scales, noise: float, eval_gradient=True, reuse_inputs=False):
        """The lanes of one lockstep round of the theta search spread over the group's devices (gpbo_group_lml_batch: lane
        i on device i mod G; inputs made resident on every device by the first call of a search).  Same return value as
        GpEngine.lml_batch_arrays, every lane bitwise what `lml()` returns on one device; `last_lane_devices` says where
        each lane ran.  (`lml_batch`, inherited, is built on this: both forms of a round go through the group.)"""
        X = np.ascontiguousarray(X, dtype=np.float64)
        y_norm = np.ascontiguousarray(y_norm, dtype=np.float64).ravel()
        ls = np.ascontiguousarray(np.atleast_2d(np.asarray(length_scales, dtype=np.float64)))
        n, n_ls = ls.shape
        vals = np.zeros(n)
        grads = np.zeros((n, n_ls))
        infos = (C.c_int * n)()
        where = (C.c_int * n)()
        rc = self._lib.gpbo_group_lml_batch(self._g, n, None if reuse_inputs else dptr(X), None if reuse_inputs else dptr(y_norm),
                                            X.shape[0], X.shape[1], int(kernel), dptr(ls), n_ls, float(noise),
                                            int(bool(eval_gradient)), dptr(vals), dptr(grads), infos, where)
        self._gcheck(rc, borrowed=(X, y_norm, ls, vals, grads, infos, where))
        self.last_lane_devices = list(where)
        return vals, grads

    # -- sharded candidates ----------------------------------------------------------------------
    def set_candidates(self, Xc):
        Xc = np.ascontiguousarray(Xc, dtype=np.float64)
        if Xc.ndim != 2:
            raise ValueError("candidates must be 2-D (M, d)")
        n_real = Xc.shape[0]
        if n_real < self.world_size:
            # fewer rows than devices: pad by repeating the last row (an equal value never beats the lower index, and
            # the copies are dropped from every result)
            pad = np.repeat(Xc[-1:], self.world_size - n_real, axis=0)
            Xc = np.ascontiguousarray(np.vstack([Xc, pad]))
        self._gcheck(self._lib.gpbo_group_set_candidates(self._g, dptr(Xc), Xc.shape[0], Xc.shape[1]), borrowed=(Xc,))
        self.n_candidates = n_real
        self._M_pad = Xc.shape[0]
        self._cand_dim = Xc.shape[1]
        self._resident = True

    mixed_device_sampling = False      # a device group samples spaces with int / categorical parameters on the host

    def generate_candidates(self, M: int, lo, hi, seed: int):
        raise NotImplementedError("the Philox throughput generator is per device; a device group draws the reference's "
                                  "stream (device_sampling='auto' / False)")

    def generate_candidates_trust_region(self, M: int, centre, lo, hi, sv, shift, bits: int, mask_threshold: int, mask_key: int):
        raise NotImplementedError("a device group has no trust-region generator (gpbo_generate_candidates_trust_region is per "
                                  "context); use a single device")

    def generate_candidates_like(self, M: int, lo, hi, random_state):
        """The reference's candidate matrix from `random_state` (one uniform(lo_j, hi_j, M) per column, in order —
        target_space.py:593-600, parameter.py:86-87): every device generates ITS row block from the caller's MT19937
        state by jump-ahead (gpbo_group_generate_candidates_mt19937); fewer rows than devices: host draw + upload."""
        lo = np.ascontiguousarray(lo, dtype=np.float64).ravel()
        hi = np.ascontiguousarray(hi, dtype=np.float64).ravel()
        if lo.shape != hi.shape:
            raise ValueError("lo and hi must have the same length")
        if not np.all(np.isfinite(hi - lo)):
            raise OverflowError("Range exceeds valid bounds")        # as RandomState.uniform
        n = max(1, int(M))
        if n < self.world_size:
            Xc = np.empty((n, lo.shape[0]))
            for j in range(lo.shape[0]):
                Xc[:, j] = random_state.uniform(lo[j], hi[j], n)
            self.set_candidates(Xc)
            return
        name, key, pos, has_gauss, cached = random_state.get_state(legacy=True)
        if name != "MT19937":
            raise TypeError("generate_candidates_like needs an MT19937 RandomState")
        key = np.ascontiguousarray(key, dtype=np.uint32).copy()
        cpos = C.c_int(int(pos))
        self._gcheck(self._lib.gpbo_group_generate_candidates_mt19937(
            self._g, n, lo.shape[0], dptr(lo), dptr(hi), key.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(cpos)),
            borrowed=(lo, hi, key, cpos))
        random_state.set_state((name, key, cpos.value, has_gauss, cached))
        self.n_candidates = n
        self._M_pad = n
        self._cand_dim = lo.shape[0]
        self._resident = True

    def get_candidate_rows(self, idx, d: int):
        idx = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int64)
        out = np.empty((idx.shape[0], d))
        self._need_resident()
        self._gcheck(self._lib.gpbo_group_get_candidate_rows(self._g, iptr(idx), idx.shape[0], dptr(out)))
        return out

    def _need_resident(self):
        if not self._resident:
            raise _lib.GpboError("the group's candidate shards are not resident (call set_candidates first; a small-batch "
                                 "predict re-uses the first device's candidate buffer)")

    def posterior(self, slot=0, y_mean=0.0, y_std=1.0, fetch=True):
        self._need_resident()
        M = self._M_pad
        mu = np.empty(M) if fetch else None
        sd = np.empty(M) if fetch else None
        self._gcheck(self._lib.gpbo_group_posterior(self._g, int(slot), float(y_mean), float(y_std), dptr(mu), dptr(sd)))
        return (mu[:self.n_candidates], sd[:self.n_candidates]) if fetch else (None, None)

    def sample_paths(self, omega, phase, weights, eps, slot=0, y_mean=0.0, y_std=1.0, index_offset=0, return_values=False):
        raise NotImplementedError("a device group has no path sampler (gpbo_sample_paths is per context); use a single device")

    def sample_paths_constrained(self, draws, lb, ub, y_mean, y_std, index_offset=0, return_values=False):
        raise NotImplementedError("a device group has no constrained path sampler (gpbo_sample_paths_constrained is per context); "
                                  "use a single device")

    def ascend_paths(self, omega, phase, weights, eps, box_lo, box_hi, n_starts=4, starts=None, max_iter=-1, slot=0, y_mean=0.0,
                     y_std=1.0, index_offset=0, return_gradient=False):
        raise NotImplementedError("a device group has no path ascent (gpbo_ascend_paths is per context); use a single device")

    def mes_argbest(self, y_star, k_seeds: int = 0, index_offset: int = 0, return_values: bool = False):
        raise NotImplementedError("a device group has no max-value entropy search (gpbo_mes_argbest is per context); use a single device")

    def kg_argbest(self, points, k_seeds: int = 0, index_offset: int = 0, y_mean: float = 0.0, y_std: float = 1.0,
                   return_values: bool = False, return_point_means: bool = False):
        raise NotImplementedError("a device group has no knowledge gradient (gpbo_kg_argbest is per context); use a single device")

    def ehvi_argbest(self, levels, cell_lo, cell_hi, k_seeds: int = 0, index_offset: int = 0, return_values: bool = False):
        raise NotImplementedError("a device group has no expected hypervolume improvement (gpbo_ehvi_argbest is per context); "
                                  "use a single device")

    def qnei_greedy(self, groups, q, noisy=True, y_best=0.0, pending=None, slot=0, y_mean=0.0, y_std=1.0, index_offset=0,
                    return_values=False, return_keys=False):
        raise NotImplementedError("a device group has no batch noisy expected improvement (gpbo_qnei_greedy is per context); "
                                  "use a single device")

    def qnehvi_greedy(self, draws, q, ref, base=None, y_mean=(0.0, 0.0), y_std=(1.0, 1.0), index_offset=0, return_values=False,
                      return_keys=False, return_fronts=False):
        raise NotImplementedError("a device group has no batch noisy expected hypervolume improvement (gpbo_qnhvi_greedy is per "
                                  "context); use a single device")

    def cnei_greedy(self, draws, q, lb, ub, y_floor, base=None, y_mean=None, y_std=None, index_offset=0, return_values=False,
                    return_keys=False):
        raise NotImplementedError("a device group has no constrained batch noisy expected improvement (gpbo_cnei_greedy is per "
                                  "context); use a single device")

    def cehvi_argbest(self, levels, cell_lo, cell_hi, lb, ub, log_form: bool = True, k_seeds: int = 0, index_offset: int = 0,
                      return_values: bool = False):
        raise NotImplementedError("a device group has no constrained expected hypervolume improvement (gpmo_cehvi_argbest is per "
                                  "context); use a single device")

    def cnehvi_greedy(self, draws, q, lb, ub, ref, base=None, y_mean=None, y_std=None, index_offset=0, return_values=False,
                      return_keys=False, return_fronts=False):
        raise NotImplementedError("a device group has no constrained batch noisy expected hypervolume improvement (gpmo_cnhvi_greedy "
                                  "is per context); use a single device")

    def posterior_refresh(self, slot=0, y_mean=0.0, y_std=1.0, fetch=True, return_route=False):
        raise NotImplementedError("a device group has no posterior refresh path (gpbo_posterior_refresh is per context); "
                                  "call posterior() after fit_append()")

    def predict(self, Xc, slot=0, y_mean=0.0, y_std=1.0, sharded=None):
        """Small batches (the host optimisers' points) run on the first device; from `world_size * 4096` rows on the
        batch is sharded like the random stage."""
        Xc = np.ascontiguousarray(Xc, dtype=np.float64)
        if sharded is None:
            sharded = Xc.shape[0] >= 4096 * self.world_size
        if sharded:
            self.set_candidates(Xc)
            return self.posterior(slot, y_mean, y_std, fetch=True)
        self._resident = False
        M = Xc.shape[0]
        mu, sd = np.empty(M), np.empty(M)
        self._check(self._lib.gpbo_predict(self._h, int(slot), dptr(Xc), M, Xc.shape[1], float(y_mean), float(y_std),
                                           dptr(mu), dptr(sd)))
        return mu, sd

    def acq_argbest(self, acq: int, param: float, y_max: float = 0.0, lb=None, ub=None, k_seeds: int = 0,
                    index_offset: int = 0, return_values: bool = False):
        if index_offset:
            raise ValueError("a device group numbers its candidates globally; index_offset must be 0")
        self._need_resident()
        lb, ub, n_c, seed_idx, seed_val, ys = _argbest_frame(lb, ub, k_seeds, self._M_pad if return_values else None)
        best_idx, best_val = np.zeros(1, dtype=np.int64), np.zeros(1)
        rc = self._lib.gpbo_group_acq_argbest(self._g, int(acq), float(param), float(y_max if y_max is not None else 0.0),
                                              n_c, dptr(lb), dptr(ub), int(k_seeds), iptr(best_idx), dptr(best_val),
                                              iptr(seed_idx), dptr(seed_val), dptr(ys))
        self._gcheck(rc, borrowed=(lb, ub, best_idx, best_val, seed_idx, seed_val, ys))
        seed_idx, seed_val = seed_idx[:k_seeds], seed_val[:k_seeds]
        if self._M_pad != self.n_candidates:      # drop the padding copies of the last row
            keep = seed_idx < self.n_candidates
            n_keep = int(keep.sum())
            seed_idx = np.concatenate([seed_idx[keep], np.full(k_seeds - n_keep, -1, dtype=np.int64)])
            seed_val = np.concatenate([seed_val[keep], np.full(k_seeds - n_keep, np.nan)])
            ys = ys[:self.n_candidates] if ys is not None else None
        return int(best_idx[0]), float(best_val[0]), seed_idx, seed_val, ys
