"""
Cases, draws, metrics and yardsticks of the generator checks at every time gap (tests/test_gpu_generator_gaps.py): the kernel -> state
space model generators of csrc/mf_sde.hip (mf_sde_matern_transitions_*, mf_sde_transitions_*, mf_sde_piecewise_transitions_* and their
reverse modes, mf_sde_matern_prior_chol_grad_*) in float32 AND float64, and the fused GPR log-likelihood in float64.

The rule is that of tests/helpers/kl_fp32_cases.py: a kernel is compared with an exact reference (tests/helpers/generator_exact.py,
mpmath at 80 digits) on the inputs it saw, and its error may be FP32_FACTOR x the error of the SAME arithmetic evaluated in the SAME
precision on the CPU - the larger of SEEDS draws (DEFAULT_SEED + i), never below FP32_FLOOR = 2^-24 in float32 and 2^-53 in float64.
The factor covers what the CPU evaluation cannot reproduce: the accumulation order of copies that form Q differently
(mf_row_gpr.hpp) and fused multiply-adds in them (mf_sde.hip itself is compiled without contraction).  The yardsticks are committed
in tests/helpers/generator_fp_table.py; scripts/generator_fp_yardsticks.py prints that file (CPU only).  Nothing here is derived
from a GPU's output.

The arithmetic is that of ``Comp::build``, ``build_osc`` and ``comp_chol`` of csrc/mf_sde.hip, statement by statement, on numpy
arrays of the dtype under test: the product A P, then (A P) A^T, subtract, add the jitter, symmetrise, column Cholesky; the 4 x 4
and 6 x 6 Kronecker forms of an oscillator are multiplied out in full.  The reverse modes run the same statements on ``Dual``
(value + three tangents, the operators of the kernels' Dual2 / Dual3: ONE reciprocal per division, sqrt' = 0.5 / sqrt) and contract
the tangents with the weights in the kernels' order.

ASSUMPTION about the device's elementary functions: exp, sin and cos are correctly rounded here (``rounded_fn``: through mpmath, so
that the table does not depend on the machine's libm or on numpy's SIMD paths), the device's are not.  Every draw is therefore also
evaluated with each of the three results moved ``ULP_NUDGE`` = 1 ulp up and down (all 27
combinations; 3 without an oscillator), and the largest error is kept.  A result at an argument of exactly zero (exp 0 = 1,
sin 0 = 0, cos 0 = 1, which the zero-gap pass-through of the kernels relies on) is not moved, nor is an exp that underflowed to zero.

Draws: lengthscale U(0.8, 1.6), variance U(0.5, 1.5), period U(1, 3), weights U(0.5, 1.5) with random signs on A [K, K] and on the
lower triangle of the factor; lam = sqrt(order) / lengthscale and omega = 2 pi / period are formed in float64; everything is rounded
to the dtype.  Time gaps: ``GAPS``.  Metrics, all PER STEP:
    A         max |A - A*| / max |A*|
    Q, Q0     max_ij |Q - Q*|_ij / sqrt(Pinf_ii Pinf_jj)      (Q at the jitter ``JITTER[dtype]``, Q0 at jitter 0)
    LLt       L L^T against Q* in the Q metric                (at the jitter)
    L         max |L - L*| / max |L*|
    g*_theta  |g - g*| / S_theta,  S = sum |w_ij| |dX_ij / dtheta|   (g: both weights, gA: w_A alone, gC: w_C alone)
The Q metric is the floor of the formula Pinf - A Pinf A^T: it stays a few ulp at every gap and needs no positive definiteness.
The factor and the gradients through it are judged at the jitter only, where every squared pivot of the CPU evaluation stays
>= 0.9 jitter for every draw, gap, component kind and nudge - ``yardstick`` asserts it, so no case is left out.
"""
import functools
import math

import mpmath as mp
import numpy as np

from helpers import generator_exact as E
from helpers.kl_fp32_cases import DEFAULT_SEED, FP32_FACTOR, FP32_FLOOR, SEEDS  # noqa: F401  (one rule, one set of numbers)

DTYPES = {"f32": np.float32, "f64": np.float64}
FLOOR = {"f32": FP32_FLOOR, "f64": 2.0 ** -53}
# f32: the jitter tests/test_gpu_gpr_grad.py::test_fused_backward_fp32 calls "what fp32 can carry"
JITTER = {"f32": 1e-4, "f64": 1e-10}
ULP_NUDGE = 1
GAPS = (0.0, 2.0 ** -24, 2.0 ** -20, 2.0 ** -16, 2.0 ** -13, 2.0 ** -10, 2.0 ** -7, 2.0 ** -5, 2.0 ** -3, 0.5, 3.0, 40.0, 1e10)
# (order, osc): every component kind the generators know but the pure rotation (order 0 with an oscillator: no Q to cancel)
KINDS = [(0, 0), (1, 0), (3, 0), (5, 0), (1, 1), (3, 1), (5, 1), (1, 2), (3, 2), (5, 2)]
PRIOR_ORDERS = (1, 3, 5)
FORWARD_NAMES = ("A", "Q0", "Q", "LLt", "L")
PARAMS = E.PARAMS
# (no "gC_omega": R(th) Pinf R(th)^T = Pinf, so Q and its factor do not depend on omega at all - S = 0, the slot has no scale; the
# omega tangent through comp_chol is judged in "g_omega", whose scale comes from A)
GRAD_NAMES = tuple(f"{g}_{p}" for g in ("g", "gA", "gC") for p in PARAMS if (g, p) != ("gC", "omega"))


def jitter_of(dt_name):
    """The jitter as the kernel of that precision receives it (a float32 kernel rounds its ``float jitter`` argument)."""
    return float(DTYPES[dt_name](JITTER[dt_name]))


# ---- draws -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def draw(i, dt_name, order, osc):
    """Draw ``i`` (seed DEFAULT_SEED + i) of one component kind: a dict of Python floats ``lam``, ``var``, ``omega`` and float64
    arrays ``w_a`` [K, K], ``w_c`` [K, K] (lower triangle), all representable in the dtype.  Read-only."""
    rng = np.random.default_rng(DEFAULT_SEED + i)
    dtype = DTYPES[dt_name]
    k = E.size(order, osc)
    ls, var, period = rng.uniform(0.8, 1.6), rng.uniform(0.5, 1.5), rng.uniform(1.0, 3.0)
    w = rng.uniform(0.5, 1.5, size=(2, 6, 6)) * rng.choice([-1.0, 1.0], size=(2, 6, 6))

    def r(x):
        return np.asarray(x).astype(dtype).astype(np.float64)
    w_a, w_c = r(w[0, :k, :k]), np.tril(r(w[1, :k, :k]))
    w_a.setflags(write=False)
    w_c.setflags(write=False)
    return {"lam": float(r(math.sqrt(order) / ls)) if order else 0.0, "var": float(r(var)),
            "omega": float(r(2.0 * math.pi / period)) if osc else 0.0, "w_a": w_a, "w_c": w_c}


# ---- the kernels' arithmetic on numpy arrays ---------------------------------------------------------------------------------------------
class Dual:
    """Dual2 / Dual3 of csrc/mf_sde.hip on arrays: ``v`` and the tangents ``t`` = [d/dlam, d/dvar, d/domega]."""

    def __init__(self, v, t=None):
        self.v = v
        self.t = [np.zeros_like(v) for _ in range(3)] if t is None else t

    def __add__(self, o):
        return Dual(self.v + o.v, [a + b for a, b in zip(self.t, o.t)])

    def __sub__(self, o):
        return Dual(self.v - o.v, [a - b for a, b in zip(self.t, o.t)])

    def __neg__(self):
        return Dual(-self.v, [-a for a in self.t])

    def __mul__(self, o):
        return Dual(self.v * o.v, [a * o.v + self.v * b for a, b in zip(self.t, o.t)])

    def __truediv__(self, o):
        r = self.v.dtype.type(1) / o.v
        q = self.v * r
        return Dual(q, [(a - q * b) * r for a, b in zip(self.t, o.t)])


class Arith:
    """How the statements below see a number: plain arrays (the forward kernels) or ``Dual`` (the reverse modes)."""

    def __init__(self, dtype, shape, dual):
        self.dtype, self.shape, self.dual = dtype, shape, dual

    def const(self, x):
        v = np.full(self.shape, x, dtype=self.dtype)
        return Dual(v) if self.dual else v

    def seed(self, v, slot):
        """An input; in dual mode with a unit tangent in ``slot`` (None: none)."""
        v = np.broadcast_to(np.asarray(v, dtype=self.dtype), self.shape).copy()
        if not self.dual:
            return v
        d = Dual(v)
        if slot is not None:
            d.t[slot] = np.ones_like(v)
        return d

    def val(self, x):
        return x.v if self.dual else x

    def fn(self, x, value, deriv):
        """f(x) with the given (possibly nudged) value array and derivative array: t_exp / t_sin / t_cos of the kernels."""
        return Dual(value, [deriv * a for a in x.t]) if self.dual else value

    def sqrt(self, x):
        if not self.dual:
            return np.sqrt(x)
        r = np.sqrt(x.v)
        h = self.dtype(0.5) / r
        return Dual(r, [h * a for a in x.t])


@functools.lru_cache(maxsize=None)
def _exact_fn(name, x):
    with mp.workdps(60):
        return float(getattr(mp, name)(mp.mpf(x)))


def rounded_fn(name, x):
    """exp / sin / cos of an array, correctly rounded (to float64, then to the array's dtype)."""
    x = np.asarray(x)
    flat = [_exact_fn(name, float(v)) for v in x.astype(np.float64).ravel()]
    return np.array(flat, dtype=np.float64).reshape(x.shape).astype(x.dtype)


def nudged(value, arg, steps):
    """``value`` moved ULP_NUDGE ulp up where ``steps`` > 0 and down where ``steps`` < 0, except where the argument is exactly zero
    and where the value is (exp underflowed: at a gap of 1e10 the transition is exactly zero on any implementation)."""
    up, down = value, value
    for _ in range(ULP_NUDGE):
        up = np.nextafter(up, np.asarray(np.inf, dtype=value.dtype))
        down = np.nextafter(down, np.asarray(-np.inf, dtype=value.dtype))
    steps = np.broadcast_to(np.asarray(steps), value.shape)
    return np.where((arg == 0) | (value == 0), value, np.where(steps > 0, up, np.where(steps < 0, down, value)))


def matern_block(ar, km, lam, var, dt, n_exp):
    """Comp<T, km>::build: (A, P) as [km][km] lists."""
    x = -(lam * dt)
    e_val = nudged(rounded_fn("exp", ar.val(x)), ar.val(x), n_exp)
    e = ar.fn(x, e_val, e_val)
    zero, one = ar.const(0.0), ar.const(1.0)
    p = [[zero for _ in range(km)] for _ in range(km)]
    if km == 1:
        return [[e]], [[var]]
    if km == 2:
        a = [[e * (one + lam * dt), e * dt], [-e * lam * lam * dt, e * (one - lam * dt)]]
        p[0][0], p[1][1] = var, var * lam * lam
        return a, p
    l2 = lam * lam
    l3 = l2 * lam
    nil = [[lam, one, zero], [zero, lam, one], [-l3, -ar.const(3.0) * l2, -ar.const(2.0) * lam]]
    nil2 = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            acc = zero
            for m in range(3):
                acc = acc + nil[i][m] * nil[m][j]
            nil2[i][j] = acc
    h = ar.const(0.5) * dt * dt
    a = [[e * ((one if i == j else zero) + nil[i][j] * dt + nil2[i][j] * h) for j in range(3)] for i in range(3)]
    l23 = l2 / ar.const(3.0)
    p[0][0] = var
    p[0][2] = -var * l23
    p[2][0] = -var * l23
    p[1][1] = var * l23
    p[2][2] = var * l2 * l2
    return a, p


def component_block(ar, order, osc, lam, var, omega, dt, nudge):
    """Comp::build or build_osc: (A, P) as [K][K] lists; ``nudge`` = ulp steps of (exp, sin, cos)."""
    km = E.matern_size(order)
    a_m, p_m = matern_block(ar, km, lam, var, dt, nudge[0])
    if not osc:
        return a_m, p_m
    th = omega * dt
    s_val = nudged(rounded_fn("sin", ar.val(th)), ar.val(th), nudge[1])
    c_val = nudged(rounded_fn("cos", ar.val(th)), ar.val(th), nudge[2])
    c, s = ar.fn(th, c_val, -s_val), ar.fn(th, s_val, c_val)
    rot = [[c, -s], [s, c]]
    zero = ar.const(0.0)
    k = 2 * km
    a = [[None] * k for _ in range(k)]
    p = [[None] * k for _ in range(k)]
    for i in range(km):
        for j in range(km):
            for pp in range(2):
                for q in range(2):
                    row, col = (pp * km + i, q * km + j) if osc == 2 else (i * 2 + pp, j * 2 + q)
                    a[row][col] = a_m[i][j] * rot[pp][q]
                    p[row][col] = p_m[i][j] if pp == q else zero
    return a, p


def comp_chol(ar, a, p, jitter, want_chol=True):
    """comp_chol: (Q, L, squared pivots) - L is zero where Q is all zero; NaN where a pivot is not positive."""
    k = len(a)
    zero = ar.const(0.0)
    ap = [[None] * k for _ in range(k)]
    for i in range(k):
        for j in range(k):
            acc = zero
            for m in range(k):
                acc = acc + a[i][m] * p[m][j]
            ap[i][j] = acc
    q = [[None] * k for _ in range(k)]
    for i in range(k):
        for j in range(k):
            acc = zero
            for m in range(k):
                acc = acc + ap[i][m] * a[j][m]
            q[i][j] = p[i][j] - acc + (jitter if i == j else zero)
    half = ar.const(0.5)
    for i in range(k):
        for j in range(i):
            q[i][j] = q[j][i] = half * (q[i][j] + q[j][i])
    if not want_chol:
        return q, None, None
    low = [[zero for _ in range(k)] for _ in range(k)]
    pivots = []
    for j in range(k):
        s = q[j][j]
        for m in range(j):
            s = s - low[j][m] * low[j][m]
        pivots.append(ar.val(s))
        ljj = ar.sqrt(s)
        low[j][j] = ljj
        for i in range(j + 1, k):
            v = q[i][j]
            for m in range(j):
                v = v - low[i][m] * low[j][m]
            low[i][j] = v / ljj
    all_zero = np.ones(ar.shape, dtype=bool)
    for i in range(k):
        for j in range(k):
            all_zero &= ar.val(q[i][j]) == 0
    return q, low, (pivots, all_zero)


def _stack(mat, ar):
    return np.stack([np.stack([ar.val(x) for x in row], axis=-1) for row in mat], axis=-2)


def _nudges(osc):
    steps = (-ULP_NUDGE, 0, ULP_NUDGE)
    return [(a, b, c) for a in steps for b in (steps if osc else (0,)) for c in (steps if osc else (0,))]


def forward_numpy(dt_name, order, osc, lam, var, omega, dt, jitter, nudge=(0, 0, 0)):
    """(A, Q, L, squared pivots [.., K] or None) of the forward kernels' arithmetic in the dtype, arrays over the shape of ``dt``;
    order 0: Q = jitter I and L = sqrt(jitter) I exactly, as emit_g writes them."""
    dtype = DTYPES[dt_name]
    dt = np.asarray(dt, dtype=dtype)
    ar = Arith(dtype, dt.shape, False)
    a, p = component_block(ar, order, osc, ar.seed(0.0 if order == 0 else lam, None), ar.seed(var, None), ar.seed(omega, None), dt,
                           nudge)
    k = len(a)
    with np.errstate(all="ignore"):
        if order == 0:
            eye = np.broadcast_to(np.eye(k, dtype=dtype), dt.shape + (k, k))
            return _stack(a, ar), eye * dtype(jitter), eye * np.sqrt(dtype(jitter)), None
        q, low, (pivots, all_zero) = comp_chol(ar, a, p, ar.const(jitter))
        low = np.where(all_zero[..., None, None], dtype(0), _stack(low, ar))
    return _stack(a, ar), _stack(q, ar), low, np.stack(pivots, axis=-1)


def grad_numpy(dt_name, order, osc, lam, var, omega, dt, jitter, w_a, w_c, nudge=(0, 0, 0)):
    """out [.., 3] of the reverse kernels' arithmetic (grad_component / contract3) in the dtype: d/d(lam, var, omega) of
    <w_a, A> + <w_c, tril chol Q>; ``w_a`` / ``w_c`` [.., K, K] or None."""
    dtype = DTYPES[dt_name]
    dt = np.asarray(dt, dtype=dtype)
    ar = Arith(dtype, dt.shape, True)
    a, p = component_block(ar, order, osc, ar.seed(0.0 if order == 0 else lam, 0), ar.seed(var, 1), ar.seed(omega, 2),
                           ar.seed(dt, None), nudge)
    k = len(a)
    g = [np.zeros(dt.shape, dtype=dtype) for _ in range(3)]
    with np.errstate(all="ignore"):
        if w_a is not None:
            w_a = np.asarray(w_a, dtype=dtype)
            for i in range(k):
                for j in range(k):
                    for s in range(3):
                        g[s] = g[s] + w_a[..., i, j] * a[i][j].t[s]
        if w_c is not None and order != 0:
            w_c = np.asarray(w_c, dtype=dtype)
            _, low, (_, all_zero) = comp_chol(ar, a, p, ar.const(jitter))
            for i in range(k):
                for j in range(i + 1):
                    for s in range(3):
                        g[s] = np.where(all_zero, g[s], g[s] + w_c[..., i, j] * low[i][j].t[s])
    if order == 0:
        g[0] = np.zeros_like(g[0])
    if not osc:
        g[2] = np.zeros_like(g[2])
    return np.stack(g, axis=-1)


def prior_grad_numpy(dt_name, order, lam, var, jitter, w_c):
    """out [2] of prior_component's arithmetic: d/d(lam, var) of <w_c, tril chol(Pinf + jitter I)>."""
    dtype = DTYPES[dt_name]
    ar = Arith(dtype, (), True)
    _, p = matern_block(ar, E.matern_size(order), ar.seed(lam, 0), ar.seed(var, 1), ar.seed(1.0, None), 0)
    k = len(p)
    a = [[ar.const(0.0) for _ in range(k)] for _ in range(k)]
    _, low, _ = comp_chol(ar, a, p, ar.const(jitter))
    w_c = np.asarray(w_c, dtype=dtype)
    g = [dtype(0), dtype(0)]
    for i in range(k):
        for j in range(i + 1):
            for s in range(2):
                g[s] = g[s] + w_c[i, j] * low[i][j].t[s]
    return np.array(g)


# ---- metrics against the exact reference -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_step(dt_name, order, osc, i, gap):
    """The exact tensors of draw ``i`` at ``gap`` in the form the metrics need - float64 (hi, lo) pairs (generator_exact.split) of
    A, Q0, Q, L, the scales, and per weight set ("g", "gA", "gC") the exact gradient and its scale S per parameter ("g_mp", ..: the
    gradient as mpf, for sums over steps).  Read-only."""
    d = draw(i, dt_name, order, osc)
    jit = jitter_of(dt_name)
    c = E.component(order, osc, d["lam"], d["var"], d["omega"], gap, jit)
    c0 = E.component(order, osc, d["lam"], d["var"], d["omega"], gap, 0.0, False)
    k = len(c["A"])
    pd = np.array([[float(c["Pinf"][a][a]) for a in range(k)]])
    out = {"A": E.split(c["A"]), "Q0": E.split(c0["Q"]), "Q": E.split(c["Q"]), "L": E.split(c["L"]),
           "A_scale": max(abs(float(x)) for row in c["A"] for x in row), "L_scale": max(abs(float(x)) for row in c["L"] for x in row),
           "Q_scale": np.sqrt(pd.T * pd)}
    for name, (w_a, w_c) in {"g": (d["w_a"], d["w_c"]), "gA": (d["w_a"], None), "gC": (None, d["w_c"])}.items():
        _, ds, scale = E.weighted(c, w_a, w_c)
        out[name] = (E.split([ds[p] for p in PARAMS]), np.array([float(scale[p]) for p in PARAMS]))
        out[name + "_mp"] = [ds[p] for p in PARAMS]
    return out


def _diff(got, pair):
    return np.abs((np.asarray(got, dtype=np.float64) - pair[0]) - pair[1])


def _rel(err, scale):
    """err / scale with 0 / 0 = 0 (an exact zero that came out as zero) and x / 0 = inf."""
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, err / scale)


def forward_errors(ex, a=None, q0=None, q=None, low=None):
    """The forward metrics of ONE step: ``ex`` from ``exact_step``, the kernel's (or the CPU evaluation's) [.., K, K] tensors, any
    leading shape (the nudges); the largest over the leading axes.  A NaN counts as an infinite error."""
    out = {}

    def worst(x):
        return float(np.max(np.where(np.isnan(x), np.inf, x)))
    if a is not None:
        out["A"] = worst(_rel(_diff(a, ex["A"]), ex["A_scale"]))
    if q0 is not None:
        out["Q0"] = worst(_rel(_diff(q0, ex["Q0"]), ex["Q_scale"]))
    if q is not None:
        out["Q"] = worst(_rel(_diff(q, ex["Q"]), ex["Q_scale"]))
    if low is not None:
        low = np.asarray(low, dtype=np.float64)
        out["LLt"] = worst(_rel(_diff(low @ np.swapaxes(low, -1, -2), ex["Q"]), ex["Q_scale"]))
        out["L"] = worst(_rel(_diff(low, ex["L"]), ex["L_scale"]))
    return out


def grad_errors(ex, which, got):
    """{"<which>_<param>": |g - g*| / S} of ONE step for ``got`` [.., 3] (weights of ``which`` in "g", "gA", "gC")."""
    err = _rel(_diff(got, ex[which][0]), ex[which][1])
    err = np.where(np.isnan(err), np.inf, err).reshape(-1, 3).max(axis=0)
    return {f"{which}_{p}": float(err[s]) for s, p in enumerate(PARAMS) if f"{which}_{p}" in GRAD_NAMES}


@functools.lru_cache(maxsize=None)
def cpu_evaluation(dt_name, order, osc, i, gaps=GAPS):
    """The kernels' arithmetic in the dtype on draw ``i``: arrays [gap, nudge, ...] of A, Q0, Q, L, the squared pivots (None for order
    0) and the three gradients.  Read-only."""
    d = draw(i, dt_name, order, osc)
    jit = jitter_of(dt_name)
    nd = np.array(_nudges(osc))
    dt = np.broadcast_to(np.array(gaps, dtype=DTYPES[dt_name])[:, None], (len(gaps), len(nd)))
    nudge = tuple(nd[None, :, s] for s in range(3))
    hyper = (d["lam"], d["var"], d["omega"])
    a, q0, _, _ = forward_numpy(dt_name, order, osc, *hyper, dt, 0.0, nudge)
    _, q, low, pivots = forward_numpy(dt_name, order, osc, *hyper, dt, jit, nudge)
    out = {"A": a, "Q0": q0, "Q": q, "L": low, "pivots": pivots}
    for which, (w_a, w_c) in {"g": (d["w_a"], d["w_c"]), "gA": (d["w_a"], None), "gC": (None, d["w_c"])}.items():
        out[which] = grad_numpy(dt_name, order, osc, *hyper, dt, jit, w_a, w_c, nudge)
    return out


def yardstick(dt_name, order, osc, gap, seeds=SEEDS, gaps=GAPS):
    """{tensor: the largest error of the CPU evaluation over the draws and the nudges}, floored; asserts the pivot condition.
    (``gaps``: the gaps evaluated together - elementwise, so the result does not depend on it.)"""
    jit = jitter_of(dt_name)
    gi = gaps.index(gap)
    worst = {}
    for i in range(seeds):
        ev = cpu_evaluation(dt_name, order, osc, i, gaps)
        ex = exact_step(dt_name, order, osc, i, gap)
        if ev["pivots"] is not None:
            assert np.all(ev["pivots"][gi] >= 0.9 * jit), ("squared pivot below 0.9 jitter", dt_name, order, osc, gap, i,
                                                           ev["pivots"][gi])
        errs = [forward_errors(ex, ev["A"][gi], ev["Q0"][gi], ev["Q"][gi], ev["L"][gi])]
        errs += [grad_errors(ex, which, ev[which][gi]) for which in ("g", "gA", "gC")]
        for e in errs:
            for name, v in e.items():
                worst[name] = max(worst.get(name, FLOOR[dt_name]), v)
    return worst


# ---- the stationary prior's factor ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_prior(dt_name, order, i):
    d = draw(i, dt_name, order, 0)
    ds, scale = E.weighted_prior(E.prior(order, d["lam"], d["var"], jitter_of(dt_name)), d["w_c"])
    return E.split([ds[p] for p in ("lam", "var")]), np.array([float(scale[p]) for p in ("lam", "var")])


def prior_errors(ex, got):
    err = _rel(_diff(got, ex[0]), ex[1])
    err = np.where(np.isnan(err), np.inf, err).reshape(-1, 2).max(axis=0)
    return {"g_lam": float(err[0]), "g_var": float(err[1])}


def prior_yardstick(dt_name, order, seeds=SEEDS):
    worst = {}
    for i in range(seeds):
        d = draw(i, dt_name, order, 0)
        got = prior_grad_numpy(dt_name, order, d["lam"], d["var"], jitter_of(dt_name), d["w_c"])
        for name, v in prior_errors(exact_prior(dt_name, order, i), got).items():
            worst[name] = max(worst.get(name, FLOOR[dt_name]), v)
    return worst


def keys():
    return [(dt_name, order, osc, gap) for dt_name in DTYPES for order, osc in KINDS for gap in GAPS]


# ---- the fused GPR log-likelihood, float64 -------------------------------------------------------------------------------------------------
# Three copies of the closed forms (mf_sde.hip; mf_gpr_fused.hpp: the register route, d <= 6; mf_row_gpr.hpp: the row route, which
# forms Q term by term) are each judged against the exact Gaussian log density of the chain, not against each other.  One series;
# the gaps are GAPS without 0 (time points must increase) and 1e10, each twice, shuffled: 22 gaps, T = 23 points (sums of these
# gaps are exact in float64, so the kernel's t[k+1] - t[k] recovers them).  Yardstick: oracle.numpy_oracle.kf_log_likelihood in
# float64 on the float64 closed-form A and chol Q (forward_numpy), |value - exact| / |exact|, the larger of SEEDS draws, floor 2^-53.
GPR_GAPS = tuple(g for g in GAPS if g not in (0.0, 1e10)) * 2
GPR_SIGNATURES = [("single", (5,)), ("single", (3, 3)), ("single", (5, 5)), ("single", (5, 5, 5)), ("multi", (5, 5, 5))]
GPR_CHUNKS = (0, 3)


@functools.lru_cache(maxsize=None)
def gpr_draw(i, sig):
    """Draw ``i`` of a GPR case: per component the hyper-parameters of ``draw((i + c) % SEEDS, "f64", order, 0)``; time points, gaps,
    observations [T, m] and the noise variance.  Read-only."""
    kind, orders = sig
    rng = np.random.default_rng(DEFAULT_SEED + i)
    gaps = np.array(GPR_GAPS)[rng.permutation(len(GPR_GAPS))]
    t = np.concatenate([[0.0], np.cumsum(gaps)])
    assert np.array_equal(np.diff(t), gaps)
    m = len(orders) if kind == "multi" else 1
    y = rng.normal(size=(len(t), m))
    comps = [draw((i + c) % SEEDS, "f64", order, 0) for c, order in enumerate(orders)]
    return {"t": t, "gaps": gaps, "y": y, "noise": float(rng.uniform(0.05, 0.2)), "lam": [c["lam"] for c in comps],
            "var": [c["var"] for c in comps], "orders": orders, "m": m}


def gpr_emission(sig):
    kind, orders = sig
    sizes = [E.matern_size(o) for o in orders]
    h = np.zeros((len(orders) if kind == "multi" else 1, sum(sizes)))
    for c, off in enumerate(np.cumsum([0] + sizes[:-1])):
        h[c if kind == "multi" else 0, off] = 1.0
    return h


@functools.lru_cache(maxsize=None)
def gpr_exact(i, sig):
    """The exact log density of the observations (mpf): the chain's joint law by P_{k+1} = A P A^T + Q, P_0 = Pinf + jitter I."""
    g = gpr_draw(i, sig)
    jit = jitter_of("f64")
    with mp.workdps(E.DPS):
        steps = [[E.component(o, 0, lam, var, 0.0, float(gap), jit, False)
                  for o, lam, var in zip(g["orders"], g["lam"], g["var"])] for gap in g["gaps"]]
        h = mp.matrix(gpr_emission(sig).tolist())
        d, m, n = h.cols, h.rows, len(g["t"])
        p = E.block_diag([c["Pinf"] for c in steps[0]]) + mp.mpf(jit) * mp.eye(d)
        cov = mp.zeros(n * m, n * m)
        for k in range(n):
            cross = p                                        # Cov(x_j, x_k) for j = k, k + 1, ...
            for j in range(k, n):
                blk = h * cross * h.T
                for a in range(m):
                    for b in range(m):
                        cov[j * m + a, k * m + b] = blk[a, b]
                        cov[k * m + b, j * m + a] = blk[a, b]
                if j + 1 < n:
                    cross = E.block_diag([c["A"] for c in steps[j]]) * cross
            if k + 1 < n:
                a_k = E.block_diag([c["A"] for c in steps[k]])
                p = a_k * p * a_k.T + E.block_diag([c["Q"] for c in steps[k]])
        for k in range(n * m):
            cov[k, k] += mp.mpf(g["noise"])
        low = mp.cholesky(cov)
        yv = mp.matrix([float(v) for v in g["y"].ravel()])
        z = mp.lu_solve(low, yv)                             # (triangular: solved exactly as it stands)
        log_det = 2 * mp.fsum(mp.log(low[k, k]) for k in range(n * m))
        return -(mp.fsum(v * v for v in z) + log_det + n * m * mp.log(2 * mp.pi)) / 2


def gpr_materialised(i, sig):
    """(mu0, chol P0, A, b, chol Q, H, y, R^-1) in float64: forward_numpy's A and chol Q, numpy's Cholesky of Pinf + jitter I."""
    g = gpr_draw(i, sig)
    jit = jitter_of("f64")
    h = gpr_emission(sig)
    d, n = h.shape[1], len(g["gaps"])
    a_s, chol_q, p0 = np.zeros((n, d, d)), np.zeros((n, d, d)), np.zeros((d, d))
    off = 0
    for o, lam, var in zip(g["orders"], g["lam"], g["var"]):
        k = E.matern_size(o)
        a, _, low, _ = forward_numpy("f64", o, 0, lam, var, 0.0, g["gaps"], jit)
        a_s[:, off:off + k, off:off + k], chol_q[:, off:off + k, off:off + k] = a, low
        ar = Arith(np.float64, (), False)
        _, p = matern_block(ar, k, ar.seed(lam, None), ar.seed(var, None), ar.seed(1.0, None), 0)
        p0[off:off + k, off:off + k] = _stack(p, ar)
        off += k
    chol_p0 = np.linalg.cholesky(p0 + jit * np.eye(d))
    return (np.zeros(d), chol_p0, a_s, np.zeros((n, d)), chol_q, np.broadcast_to(h, (n + 1,) + h.shape).copy(), g["y"],
            np.eye(g["m"]) / g["noise"])


def gpr_error(value, i, sig):
    """|value - exact| / |exact| for a float64 log-likelihood of draw ``i``."""
    exact = gpr_exact(i, sig)
    hi, lo = E.split(exact)
    return float(abs((float(value) - hi) - lo) / abs(hi))


def gpr_yardstick(sig, seeds=SEEDS):
    from oracle import numpy_oracle as O
    worst = FLOOR["f64"]
    for i in range(seeds):
        worst = max(worst, gpr_error(O.kf_log_likelihood(*gpr_materialised(i, sig), per_series=True), i, sig))
    return worst
