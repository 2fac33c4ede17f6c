"""Plain-Python restatement of the differential evolution walk the mixed-space smart stage asks SciPy for
(bayes_opt/acquisition.py:375-396: DifferentialEvolutionSolver(func, bounds, init=population, polish=False, rng=random_state)
with every other argument at its default: best1bin, mutation=(0.5, 1) dithered, recombination=0.7, updating='immediate',
tol=0.01, atol=0, maxiter=1000).  Every draw is spelled out on the MT19937 words of the legacy RandomState, so this module is
the specification csrc/evolve.hip implements: tests/test_evolve_host.py holds it to SciPy bit for bit, tests/test_gpu_evolve.py
holds the device to it.  Not a test module (no test_ prefix)."""
from __future__ import annotations

import numpy as np

_UPPER, _LOWER, _MATRIX_A = np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x9908B0DF)


def _twist(mt):
    """One MT19937 regeneration of the 624-word state, in the serial loop's order: [0, 227) from the old words, [227, 454)
    and [454, 623) from words of the new block 227 positions back, 623 from the new words 0 and 396."""
    def f(cur, nxt, far):
        y = (cur & _UPPER) | (nxt & _LOWER)
        return far ^ (y >> np.uint32(1)) ^ np.where((y & np.uint32(1)) != 0, _MATRIX_A, np.uint32(0)).astype(np.uint32)

    new = mt.copy()
    new[0:227] = f(mt[0:227], mt[1:228], mt[397:624])
    new[227:454] = f(mt[227:454], mt[228:455], new[0:227])
    new[454:623] = f(mt[454:623], mt[455:624], new[227:396])
    new[623] = f(mt[623:624], new[0:1], new[396:397])[0]
    return new


def _temper(mt):
    y = mt.copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return [int(v) for v in y]


class Words:
    """The 32-bit outputs of a legacy RandomState's MT19937 from (key, pos); the block is regenerated lazily, as NumPy does."""

    def __init__(self, key, pos):
        self.key = np.asarray(key, dtype=np.uint32).copy()
        self.pos = int(pos)
        self._out = _temper(self.key)

    def next32(self) -> int:
        if self.pos >= 624:
            self.key = _twist(self.key)
            self._out = _temper(self.key)
            self.pos = 0
        w = self._out[self.pos]
        self.pos += 1
        return w

    def double(self) -> float:                      # random_standard_uniform: 53 bits from two words
        a, b = self.next32() >> 5, self.next32() >> 6
        return (a * 67108864.0 + b) / 9007199254740992.0

    def interval(self, mx: int) -> int:             # random_interval: masked rejection (shuffle; randint's bounded draw alike)
        if mx == 0:
            return 0
        mask = mx
        for s in (1, 2, 4, 8, 16):
            mask |= mask >> s
        while True:
            v = self.next32() & mask
            if v <= mx:
                return v


def pairwise_sum(a) -> float:
    """NumPy's float64 add.reduce of a contiguous vector: 8 accumulators below 128 values, recursive halves above."""
    a = [float(v) for v in a]

    def pw(lo, n):
        if n < 8:
            res = 0.0
            for i in range(n):
                res += a[lo + i]
            return res
        if n <= 128:
            r = a[lo:lo + 8]
            i = 8
            while i < n - (n % 8):
                for j in range(8):
                    r[j] += a[lo + i + j]
                i += 8
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            while i < n:
                res += a[lo + i]
                i += 1
            return res
        n2 = n // 2
        n2 -= n2 % 8
        return pw(lo, n2) + pw(lo + n2, n - n2)

    return pw(0, len(a))


def mean_std(e):
    """(np.mean(e), np.std(e)) op by op."""
    n = len(e)
    m = pairwise_sum(e) / n
    dev = [(float(v) - m) * (float(v) - m) for v in e]
    return m, float(np.sqrt(pairwise_sum(dev) / n))


def converged(e) -> bool:
    if any(np.isinf(v) for v in e):
        return False
    m, s = mean_std(e)
    return bool(s <= 0 + 0.01 * abs(m))


def argmin(e) -> int:
    """np.argmin: the first NaN, else the first smallest value."""
    best = 0
    for i in range(len(e)):
        if e[i] != e[i]:
            return i
        if e[i] < e[best]:
            best = i
    return best


def walk(func, bounds, init, key, pos, maxiter: int = 1000):
    """The solver's solve() with polish=False; func(x (D,)) -> float.  Returns a dict with x, fun, nit, nfev, success, the
    final population (in parameter space) and energies, and the MT19937 (key, pos) afterwards."""
    bounds = np.asarray(bounds, dtype=np.float64)
    lo, hi = bounds[:, 0], bounds[:, 1]
    arg1 = 0.5 * (lo + hi)
    arg2 = np.fabs(lo - hi)
    with np.errstate(divide="ignore"):
        recip = 1 / arg2
    recip[~np.isfinite(recip)] = 0
    rng = Words(key, pos)
    pop = np.clip((np.asarray(init, dtype=np.float64) - arg1) * recip + 0.5, 0, 1)
    S, D = pop.shape
    energies = [np.inf] * S
    perm = list(range(S))
    nfev = 0

    def scale(u):
        return arg1 + (u - 0.5) * arg2

    def promote():
        k = argmin(energies)
        energies[0], energies[k] = energies[k], energies[0]
        pop[[0, k], :] = pop[[k, 0], :]

    def full_pass():
        nonlocal nfev
        for i in range(S):
            energies[i] = float(func(scale(pop[i])))
        nfev += S
        promote()

    if all(np.isinf(v) for v in energies):
        full_pass()
    nit, success = 0, False
    for nit in range(1, maxiter + 1):
        if all(np.isinf(v) for v in energies):
            full_pass()
        s = 0.5 + (1.0 - 0.5) * rng.double()
        for c in range(S):
            fill = rng.interval(D - 1)                # randint(0, D): no word when D == 1
            for i in range(S - 1, 0, -1):             # shuffle of the persistent index array
                j = rng.interval(i)
                perm[i], perm[j] = perm[j], perm[i]
            r = [v for v in perm[:6] if v != c][:2]
            bprime = pop[0] + s * (pop[r[0]] - pop[r[1]])
            cross = np.array([rng.double() for _ in range(D)]) < 0.7
            cross[fill] = True
            trial = np.where(cross, bprime, pop[c])
            oob = (trial > 1) | (trial < 0)
            for t in np.flatnonzero(oob):
                trial[t] = rng.double()
            energy = float(func(scale(trial)))
            nfev += 1
            if energy <= energies[c]:
                pop[c] = trial
                energies[c] = energy
                if energy <= energies[0]:
                    promote()
        if converged(energies):
            success = True
            break
    return {"x": scale(pop[0]), "fun": energies[0], "nit": nit, "nfev": nfev, "success": success,
            "population": scale(pop), "energies": np.array(energies), "key": rng.key, "pos": rng.pos}


def analytic(weights, targets, rounded):
    """The fixed objective gpbo_debug_evolve_walk evaluates: sum_t w_t (g_t(x_t) - a_t)^2 left to right, g_t = rint where
    `rounded[t]`, identity elsewhere."""
    w = [float(v) for v in weights]
    a = [float(v) for v in targets]
    r = [bool(v) for v in rounded]

    def f(x):
        s = 0.0
        for t in range(len(w)):
            g = float(np.rint(x[t])) if r[t] else float(x[t])
            dl = g - a[t]
            s = s + w[t] * (dl * dl)
        return s

    return f
