"""Test infrastructure for constrained greedy batch noisy expected improvement (gpbo_cnei_greedy / suggest_constrained_qnei; never
imported by the product): the rule of include/gpbo.h restated in NumPy over GIVEN value arrays, the shared cases of the host and the
GPU tests, and CneiFakeEngine.

values (1 + C, T, n): slot 0 the objective's draws, slot j constraint j's, at n points.  Per draw t and point x
    viol_t(x) = scbo_truth.violations' sum: max(max(lb_j - c, c - ub_j), 0) / y_std_j added in constraint order, a NaN kept
    g_t(x)    = NaN if f_t(x) or viol_t(x) is NaN;  f_t(x) if viol_t(x) == 0;  -inf otherwise
    m_t       = fmax(y_floor, the fmax fold in index order of g_t(base_i))
and the steps are qnei_truth.greedy's on g.  pick_feasible[j] = (the number of t with g_t(pick_j) > -inf) / T, NaN for a NaN pick."""
import functools

import numpy as np

import matern_family_truth as F
import paths_truth as P
import qnei_truth as Q
import scbo_truth as ST
from bayesianoptimization_amd.engine import F32
from bayesianoptimization_amd.thompson import spectral_draw

NOISE = 1e-2
BAR, MARGIN = 1e-9, 8.0
INF = np.inf
KINDS = (F.MATERN25, F.RBF, F.MATERN15, F.MATERN05)


def masked(f, viol):
    """g (T, n) from the objective's values f (T, n) and viol (T, n)"""
    f, viol = np.asarray(f, dtype=np.float64), np.asarray(viol, dtype=np.float64)
    g = np.where(viol == 0.0, f, -np.inf)
    return np.where(np.isnan(f) | np.isnan(viol), np.nan, g)


def baseline(g_base, y_floor):
    """m_t (T,) before the first pick from g at the base points (T, B), B >= 0"""
    g_base = np.asarray(g_base, dtype=np.float64)
    m = np.full(g_base.shape[0], float(y_floor))
    for i in range(g_base.shape[1]):
        m = np.fmax(m, g_base[:, i])
    return m


def greedy(g, m0, q, index_offset=0):
    """qnei_truth.greedy on the masked values: (pick_idx, pick_gain, keys (q, M), m after the last pick)"""
    with np.errstate(invalid="ignore"):      # -inf - m_t and -inf - (-inf): the term is 0 either way
        return Q.greedy(g, m0, q, index_offset)


def pick_feasible(g, local_idx, gain):
    """(q,): the share of draws with g_t(pick) > -inf; NaN where the pick was a NaN pick (its gain is NaN)"""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        share = np.array([np.count_nonzero(g[:, i] > -np.inf) / float(g.shape[0]) for i in local_idx])
    return np.where(np.isnan(gain), np.nan, share)


def rule(values, base_values, lb, ub, y_std, y_floor, q, index_offset=0):
    """The whole call on given RAW values (1 + C, T, M) and base values (1 + C, T, B): a dict like the engine's."""
    values = np.asarray(values, dtype=np.float64)
    viol = ST.violations(values, lb, ub, y_std)
    g = masked(values[0], viol)
    T = values.shape[1]
    if base_values is None or np.shape(base_values)[2] == 0:
        g_base = np.empty((T, 0))
    else:
        base_values = np.asarray(base_values, dtype=np.float64)
        g_base = masked(base_values[0], ST.violations(base_values, lb, ub, y_std))
    m0 = baseline(g_base, y_floor)
    idx, gain, keys, m = greedy(g, m0, q, index_offset)
    return {"index": idx, "gain": gain, "feasible": pick_feasible(g, idx - index_offset, gain), "baseline": m0, "keys": keys,
            "viol": viol, "masked": g, "masked_base": g_base, "final": m}


def length_scale(d, per_dim, j):
    s = 0.5 * np.sqrt(d) * (1.0 + 0.15 * j)
    return s * np.geomspace(0.75, 1.33, d) if per_dim else np.array([s])


class Case:
    """1 + C slots' data, fits' arguments, G groups of draws per slot, candidates, base points and bounds (computed once, shared,
    never changed).  Slot j: Ns[j] observations, kind kinds[j], its own length scales, y_mean = 3.5 - j, y_std = 0.4 + 0.3 j.  The
    base points are the objective's observed points (as many as fit) and then uniform pending ones.  The bounds are the
    (lo, hi) quantiles of the TRUTH's constraint values over the candidates; `floor_quantile` is the quantile of the truth's
    objective values that serves as y_floor."""

    def __init__(self, C, Ns, M, Fn, d, G, S, B, kinds=None, per_dim=False, scaled_slot=None, f32_slot=None, seed=0,
                 quantiles=(0.2, 0.8), floor_quantile=0.5, picks=False, share=(0.2, 0.8)):
        self.C, self.M, self.F, self.d, self.G, self.S, self.B = C, M, Fn, d, G, S, B
        self.T = G * S
        self.Ns = [Ns] * (1 + C) if np.isscalar(Ns) else list(Ns)
        self.kinds = [KINDS[j % 4] for j in range(1 + C)] if kinds is None else list(kinds)
        self.quantiles, self.floor_quantile, self.picks, self.share = quantiles, floor_quantile, picks, share
        rs = np.random.RandomState(6000 + seed + 7 * C + M + Fn)
        self.Xc = rs.uniform(size=(M, d))
        self.y_mean = np.array([3.5 - j for j in range(1 + C)])
        self.y_std = np.array([0.4 + 0.3 * j for j in range(1 + C)])
        self.slots, self.draws = [], []
        for j in range(1 + C):
            N = self.Ns[j]
            X, y = F.data(N, d, seed=seed + 17 * N + d + 101 * j)
            yn = (y - y.mean()) / y.std()
            amplitude, white = (2.5, 1e-3) if j == scaled_slot else (1.0, 0.0)
            self.slots.append(dict(X=X, yn=yn, kind=self.kinds[j], ls=length_scale(d, per_dim, j), amplitude=amplitude, white=white,
                                   precision=F32 if j == f32_slot else 0))
            groups = []
            for _ in range(G):
                omega, phase = spectral_draw(self.kinds[j], Fn, d, rs)
                groups.append((omega, phase, rs.standard_normal((S, Fn)), rs.standard_normal((S, N)) * np.sqrt(NOISE + white)))
            self.draws.append(groups)
        n_obs = min(B, self.Ns[0])
        self.base = np.vstack([self.slots[0]["X"][:n_obs], rs.uniform(size=(B - n_obs, d))]) if B else None
        self.what = f"C={C} N={self.Ns} M={M} F={Fn} d={d} {G}x{S} B={B}"

    def route(self, fn):
        """(1 + C, T, M + B): every slot's draws at the candidates | the base points"""
        pts = self.Xc if not self.B else np.vstack([self.Xc, self.base])
        out = []
        for j, s in enumerate(self.slots):
            eta = (NOISE + s["white"]) / s["amplitude"]
            out.append(Q.group_values(fn, s["kind"], s["X"], s["yn"], s["ls"], eta, self.draws[j], pts, self.y_mean[j], self.y_std[j],
                                      s["amplitude"]))
        return np.array(out)

    def err_of(self, f, ref, j):
        ref_n = (ref - self.y_mean[j]) / self.y_std[j]
        return float(np.max(np.abs(f - ref)) / (self.y_std[j] * max(1.0, float(np.max(np.abs(ref_n))))))

    def references(self):
        """ref (1 + C, T, M + B) by paths_cho, and per slot the bar max(1e-9, 8 x the spread of the two NumPy routes)"""
        self.ref = self.route(P.paths_cho)
        other = self.route(P.paths_winv)
        self.own = [self.err_of(other[j], self.ref[j], j) for j in range(1 + self.C)]
        self.bars = [max(BAR, MARGIN * o) for o in self.own]
        t = self.ref[:, :, :self.M]
        self.lb = np.array([np.quantile(t[j], self.quantiles[0]) if self.quantiles[0] > 0 else -INF for j in range(1, 1 + self.C)])
        self.ub = np.array([np.quantile(t[j], self.quantiles[1]) if self.quantiles[1] < 1 else INF for j in range(1, 1 + self.C)])
        self.y_floor = float(np.quantile(t[0], self.floor_quantile))
        return self

    def scale(self, j):
        """the size of one unit of the parity norm in slot j's raw values"""
        return self.y_std[j] * max(1.0, float(np.abs((self.ref[j] - self.y_mean[j]) / self.y_std[j]).max()))

    def near_a_bound(self):
        """(T, M + B) bool: a truth constraint value within the slot's bar x scale of one of its bounds — the only (draw, point)
        pairs whose feasibility the device may call otherwise"""
        near = np.zeros(self.ref.shape[1:], dtype=bool)
        for j in range(1, 1 + self.C):
            tol = self.bars[j] * self.scale(j)
            near |= (np.abs(self.ref[j] - self.lb[j - 1]) <= tol) | (np.abs(self.ref[j] - self.ub[j - 1]) <= tol)
        return near

    def truth(self, q):
        return rule(self.ref[:, :, :self.M], self.ref[:, :, self.M:], self.lb, self.ub, self.y_std, self.y_floor, q)

    def fit(self, eng, Xc=None):
        for j, s in enumerate(self.slots):
            scaled = {} if (s["amplitude"], s["white"]) == (1.0, 0.0) else {"amplitude": s["amplitude"], "white": s["white"]}
            eng.fit(s["X"], s["yn"], s["kind"], s["ls"], NOISE, slot=j, precision=s["precision"], **scaled)
        eng.set_candidates(self.Xc if Xc is None else Xc)

    def run(self, eng, q, draws=None, **kw):
        kw.setdefault("lb", self.lb)
        kw.setdefault("ub", self.ub)
        kw.setdefault("y_floor", self.y_floor)
        kw.setdefault("base", self.base)
        kw.setdefault("return_values", True)
        kw.setdefault("return_keys", True)
        lb, ub, y_floor = kw.pop("lb"), kw.pop("ub"), kw.pop("y_floor")
        return eng.cnei_greedy(self.draws if draws is None else draws, q, lb, ub, y_floor, y_mean=self.y_mean, y_std=self.y_std, **kw)


#: name -> Case arguments: the edges of the code (N per slot, M, F, d, G x S, n_base)
CASES = {
    # M odd: one candidate per score thread
    "c1-n65,64-m63-f64-d2-2x5-b66": dict(C=1, Ns=(65, 64), M=63, Fn=64, d=2, G=2, S=5, B=66, picks=True),
    # M even, two score workgroups, a scaled constraint slot, kinds differing per slot
    "c2-n130,65,64-m514-f65-d5-3x16-b194": dict(C=2, Ns=(130, 65, 64), M=514, Fn=65, d=5, G=3, S=16, B=194, per_dim=True,
                                                scaled_slot=1, quantiles=(0.1, 0.9), picks=True),
    # all eight slots, T = 1, m_t = y_floor
    "c7-n64-m63-f63-d3-1x1-b0": dict(C=7, Ns=64, M=63, Fn=63, d=3, G=1, S=1, B=0, quantiles=(0.05, 0.95)),
    # T = 256, an F32 objective slot
    "c1-n64-m63-f64-d3-16x16-b66": dict(C=1, Ns=64, M=63, Fn=64, d=3, G=16, S=16, B=66, f32_slot=0, picks=True),
    # the wide path_eval workgroup
    "c1-n65,64-m131075-f63-d2-2x1-b65": dict(C=1, Ns=(65, 64), M=(1 << 17) + 3, Fn=63, d=2, G=2, S=1, B=65),
    # a bound tight enough that some draws have no feasible base point (the floor case: its share is the named exception)
    "floor-c1-n65,64-m63-f64-d2-2x5-b66": dict(C=1, Ns=(65, 64), M=63, Fn=64, d=2, G=2, S=5, B=66, quantiles=(0.0, 0.03),
                                               floor_quantile=0.05, share=None),
}
PICK_CASES = [k for k, v in CASES.items() if v.get("picks")]
FLOOR_CASE = "floor-c1-n65,64-m63-f64-d2-2x5-b66"


@functools.lru_cache(maxsize=None)
def case_of(name):
    return Case(**CASES[name]).references()


class CneiFakeEngine(ST.ScboFakeEngine):
    """scbo_truth.ScboFakeEngine (TEST DOUBLE ONLY) + cnei_greedy = `paths_cho` per slot and `rule`; records what it was handed."""

    def cnei_greedy(self, draws, q, lb, ub, y_floor, base=None, y_mean=None, y_std=None, index_offset=0, return_values=False,
                    return_keys=False):
        draws = [list(g) for g in draws]
        self.calls.append(("cnei_greedy", len(draws) - 1, len(draws[0]), np.shape(draws[0][0][2])[0], int(q)))
        self.cnei_args = dict(draws=draws, lb=np.array(lb), ub=np.array(ub), y_floor=float(y_floor),
                              base=None if base is None else np.array(base), y_mean=np.array(y_mean), y_std=np.array(y_std))
        pts = self.Xc if base is None else np.vstack([self.Xc, base])
        vals = []
        for j, groups in enumerate(draws):
            X, kernel, length_scale, noise = self.inputs[j]
            vals.append(Q.group_values(P.paths_cho, kernel, X, self.targets[j], length_scale, noise, groups, pts, y_mean[j], y_std[j]))
        vals = np.array(vals)
        M = self.Xc.shape[0]
        out = rule(vals[:, :, :M], vals[:, :, M:], np.asarray(lb), np.asarray(ub), np.asarray(y_std), y_floor, int(q), index_offset)
        self.cnei_values, self.cnei_base_values = vals[:, :, :M], vals[:, :, M:]
        return {"index": out["index"], "gain": out["gain"], "feasible": out["feasible"], "baseline": out["baseline"],
                "values": vals[:, :, :M] if return_values else None, "viol": out["viol"] if return_values else None,
                "base_values": vals[:, :, M:] if return_values else None, "keys": out["keys"] if return_keys else None}
