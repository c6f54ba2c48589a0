"""
Exact (mpmath, 80 digits) transitions of the SDE kernel components and their hyper-parameter derivatives - TEST INFRASTRUCTURE,
NOT PRODUCT CODE.  Host only.

The generators of csrc/mf_sde.hip (and their copies in mf_gpr_fused.hpp / mf_row_gpr.hpp) form Q = Pinf - A Pinf A^T, which
cancels at short time gaps: the true smallest eigenvalue of Q reaches 2.5e-30 at dt = 2^-20, far below what float64 or
numpy.longdouble resolve.  This module evaluates the same mathematical objects at ``DPS`` digits, so that a kernel, and the CPU
evaluation of its arithmetic that serves as a yardstick (tests/helpers/generator_fp_cases.py), can both be measured against the truth.

One generalised component: ``order`` in {0, 1, 3, 5} (0: constant, else Matern-order/2), ``osc`` in {0, 1, 2} (0: none,
1: Matern (x) R(omega dt), 2: R(omega dt) (x) Matern), ``lam = sqrt(order) / lengthscale``, ``var``, ``omega = 2 pi / period``.
The inputs are Python floats: the float32- or float64-representable values the kernel saw.

    A     = exp(F dt)  in closed form: e^{-lam dt} (I + N dt + N^2 dt^2 / 2) with N = F + lam I nilpotent, Kronecker product with
            R(th) = [[cos th, -sin th], [sin th, cos th]]  (``feedback`` builds F for the check against mp.expm)
    Pinf  = the stationary covariance
    Q     = Pinf - A Pinf A^T + jitter I;  jitter I EXACTLY for order 0 (a constant or a pure rotation adds no noise)
    L     = the lower Cholesky factor of Q, zero for an all-zero Q
    d/d(lam, var, omega) of every entry of A and L by ``mp.diff`` (central differences at twice the working precision)

``weighted`` contracts them with weights:  s = <w_A, A> + <w_C, tril L>,  ds/dtheta,  and the scale
S_theta = sum |w_ij| |dX_ij / dtheta| that a gradient's error is measured against.  ``prior`` does the same for chol(Pinf + jitter I).
"""
import functools

import mpmath as mp
import numpy as np

DPS = 80
PARAMS = ("lam", "var", "omega")


def matern_size(order):
    return 1 if order == 0 else (order + 1) // 2


def size(order, osc):
    return matern_size(order) * (2 if osc else 1)


def _zeros(k):
    return [[mp.mpf(0) for _ in range(k)] for _ in range(k)]


def _eye(k):
    return [[mp.mpf(1 if i == j else 0) for j in range(k)] for i in range(k)]


def _mul(a, b):
    k = len(a)
    return [[mp.fsum(a[i][l] * b[l][j] for l in range(k)) for j in range(k)] for i in range(k)]


def _transpose(a):
    return [list(r) for r in zip(*a)]


def _kron(a, b):
    na, nb = len(a), len(b)
    return [[a[i][j] * b[p][q] for j in range(na) for q in range(nb)] for i in range(na) for p in range(nb)]


def matern_feedback(order, lam):
    if order == 0:
        return [[mp.mpf(0)]]
    if order == 1:
        return [[-lam]]
    if order == 3:
        return [[mp.mpf(0), mp.mpf(1)], [-lam ** 2, -2 * lam]]
    return [[mp.mpf(0), mp.mpf(1), mp.mpf(0)], [mp.mpf(0), mp.mpf(0), mp.mpf(1)], [-lam ** 3, -3 * lam ** 2, -3 * lam]]


def feedback(order, osc, lam, omega):
    """F of ds = F s dt + noise, as an mp.matrix: F_M (x) I2 + I (x) W for osc = 1, I2 (x) F_M + W (x) I for osc = 2,
    W = [[0, -omega], [omega, 0]]."""
    with mp.workdps(DPS):
        lam, omega = mp.mpf(0 if order == 0 else lam), mp.mpf(omega)
        f = matern_feedback(order, lam)
        if osc:
            k = len(f)
            w = [[mp.mpf(0), -omega], [omega, mp.mpf(0)]]
            pair = (_kron(f, _eye(2)), _kron(_eye(k), w)) if osc == 1 else (_kron(_eye(2), f), _kron(w, _eye(k)))
            f = [[x + y for x, y in zip(r1, r2)] for r1, r2 in zip(*pair)]
        return mp.matrix(f)


def _matern_pinf(order, lam, var):
    if order <= 1:
        return [[var]]
    if order == 3:
        return [[var, mp.mpf(0)], [mp.mpf(0), var * lam ** 2]]
    k = var * lam ** 2 / 3
    return [[var, mp.mpf(0), -k], [mp.mpf(0), k, mp.mpf(0)], [-k, mp.mpf(0), var * lam ** 4]]


def _cholesky(q):
    k = len(q)
    low = _zeros(k)
    if all(q[i][j] == 0 for i in range(k) for j in range(k)):
        return low
    for j in range(k):
        s = q[j][j] - mp.fsum(low[j][l] ** 2 for l in range(j))
        if s <= 0:
            raise ArithmeticError("generator_exact: Q is not positive definite at the working precision")
        low[j][j] = mp.sqrt(s)
        for i in range(j + 1, k):
            low[i][j] = (q[i][j] - mp.fsum(low[i][l] * low[j][l] for l in range(j))) / low[j][j]
    return low


def _build(order, osc, lam, var, omega, dt, jitter, want_chol=True):
    """(A, Pinf, Q, L) as nested lists of mpf, at the precision of the caller's context."""
    if order == 0:
        lam = mp.mpf(0)
    km = matern_size(order)
    f = matern_feedback(order, lam)
    nil = [[f[i][j] + (lam if i == j else 0) for j in range(km)] for i in range(km)]
    nil2 = _mul(nil, nil)
    e = mp.exp(-lam * dt)
    a = [[e * ((1 if i == j else 0) + nil[i][j] * dt + nil2[i][j] * dt * dt / 2) for j in range(km)] for i in range(km)]
    p = _matern_pinf(order, lam, var)
    if osc:
        th = omega * dt
        rot = [[mp.cos(th), -mp.sin(th)], [mp.sin(th), mp.cos(th)]]
        a, p = (_kron(a, rot), _kron(p, _eye(2))) if osc == 1 else (_kron(rot, a), _kron(_eye(2), p))
    k = len(a)
    if order == 0:
        q = [[jitter if i == j else mp.mpf(0) for j in range(k)] for i in range(k)]
    else:
        apa = _mul(_mul(a, p), _transpose(a))
        q = [[p[i][j] - (apa[i][j] + apa[j][i]) / 2 + (jitter if i == j else 0) for j in range(k)] for i in range(k)]
    return a, p, q, (_cholesky(q) if want_chol else None)


def _entrywise_derivative(fn, x, count):
    """d/dx of the ``count`` entries of the list ``fn(x)``: ``mp.diff`` entry by entry, every evaluation of ``fn`` shared."""
    seen = {}

    def entry(z, i):
        if z not in seen:
            seen[z] = fn(z)
        return seen[z][i]
    return [mp.diff(lambda z, i=i: entry(z, i), x) for i in range(count)]


def _flat(a, low):
    k = len(a)
    return [a[i][j] for i in range(k) for j in range(k)] + [low[i][j] for i in range(k) for j in range(k)]


def _unflat(v, k):
    return [[v[i * k + j] for j in range(k)] for i in range(k)], [[v[k * k + i * k + j] for j in range(k)] for i in range(k)]


@functools.lru_cache(maxsize=None)
def component(order, osc, lam, var, omega, dt, jitter, grad=True):
    """The exact tensors of one component at one time gap: a dict of nested lists of mpf - "A", "Pinf", "Q", "L" and, with ``grad``,
    "dA" / "dL": {"lam" | "var" | "omega": [K][K]} (all zero for d/dlam of order 0 and d/domega without an oscillator).
    Cached: treat the result as read-only."""
    with mp.workdps(DPS):
        args = dict(lam=mp.mpf(lam), var=mp.mpf(var), omega=mp.mpf(omega))
        dt, jitter = mp.mpf(dt), mp.mpf(jitter)
        a, p, q, low = _build(order, osc, args["lam"], args["var"], args["omega"], dt, jitter)
        out = {"A": a, "Pinf": p, "Q": q, "L": low}
        if not grad:
            return out
        k = len(a)
        out["dA"], out["dL"] = {}, {}
        for name in PARAMS:
            if (name == "lam" and order == 0) or (name == "omega" and not osc):
                out["dA"][name], out["dL"][name] = _zeros(k), _zeros(k)
                continue

            def fn(z, name=name):
                kw = dict(args)
                kw[name] = z
                return _flat(*_build(order, osc, kw["lam"], kw["var"], kw["omega"], dt, jitter)[::3])
            out["dA"][name], out["dL"][name] = _unflat(_entrywise_derivative(fn, args[name], 2 * k * k), k)
        return out


@functools.lru_cache(maxsize=None)
def prior(order, lam, var, jitter):
    """chol(Pinf + jitter I) of a Matern component and its derivatives: {"L0", "dL0": {"lam" | "var": [K][K]}}."""
    with mp.workdps(DPS):
        args = dict(lam=mp.mpf(lam), var=mp.mpf(var))
        jitter = mp.mpf(jitter)
        k = matern_size(order)

        def factor(lam, var):
            p = _matern_pinf(order, lam, var)
            return _cholesky([[p[i][j] + (jitter if i == j else 0) for j in range(k)] for i in range(k)])
        out = {"L0": factor(**args), "dL0": {}}
        for name in ("lam", "var"):
            def fn(z, name=name):
                kw = dict(args)
                kw[name] = z
                low = factor(kw["lam"], kw["var"])
                return [low[i][j] for i in range(k) for j in range(k)]
            flat = _entrywise_derivative(fn, args[name], k * k)
            out["dL0"][name] = [[flat[i * k + j] for j in range(k)] for i in range(k)]
        return out


def _contract(w, x):
    k = len(x)
    return mp.fsum(mp.mpf(float(w[i][j])) * x[i][j] for i in range(k) for j in range(k))


def _scale(w, x):
    k = len(x)
    return mp.fsum(abs(mp.mpf(float(w[i][j])) * x[i][j]) for i in range(k) for j in range(k))


def weighted(comp, w_a=None, w_c=None):
    """``(s, {theta: ds/dtheta}, {theta: S_theta})`` of a ``component`` result for weights ``w_a`` [K][K] on A and ``w_c`` [K][K]
    (its lower triangle) on the factor; either may be None."""
    with mp.workdps(DPS):
        k = len(comp["A"])
        tril = None if w_c is None else [[float(w_c[i][j]) if j <= i else 0.0 for j in range(k)] for i in range(k)]
        parts = [(w, x, dx) for w, x, dx in ((w_a, comp["A"], comp["dA"]), (tril, comp["L"], comp["dL"])) if w is not None]
        s = mp.fsum(_contract(w, x) for w, x, _ in parts)
        ds = {name: mp.fsum(_contract(w, dx[name]) for w, _, dx in parts) for name in PARAMS}
        scale = {name: mp.fsum(_scale(w, dx[name]) for w, _, dx in parts) for name in PARAMS}
        return s, ds, scale


def weighted_prior(pri, w_c):
    """``({theta: ds/dtheta}, {theta: S_theta})`` of s = <w_c, tril chol(Pinf + jitter I)> for a ``prior`` result."""
    with mp.workdps(DPS):
        k = len(pri["L0"])
        tril = [[float(w_c[i][j]) if j <= i else 0.0 for j in range(k)] for i in range(k)]
        return ({name: _contract(tril, pri["dL0"][name]) for name in ("lam", "var")},
                {name: _scale(tril, pri["dL0"][name]) for name in ("lam", "var")})


def block_diag(blocks):
    """Nested lists [k_i][k_i] of mpf -> the block-diagonal mp.matrix of a concatenation."""
    d = sum(len(b) for b in blocks)
    out = mp.zeros(d, d)
    off = 0
    for b in blocks:
        for i, row in enumerate(b):
            for j, x in enumerate(row):
                out[off + i, off + j] = x
        off += len(b)
    return out


def split(x):
    """An mpf (or a nested list of them) as two float64 arrays ``hi + lo``: ``(got - hi) - lo`` is then ``got - x`` to about
    2^-106 |x|, evaluated in float64 - ``got - float(x)`` alone would carry the rounding of the reference itself."""
    with mp.workdps(DPS):
        arr = np.array(x, dtype=object)
        hi = np.vectorize(float, otypes=[np.float64])(arr)
        rest = arr - np.vectorize(mp.mpf, otypes=[object])(hi)
        return hi, np.vectorize(float, otypes=[np.float64])(rest)


def error(got, exact):
    """``|got - exact|`` elementwise in float64, ``exact`` an mpf or nested lists of them shaped like ``got``."""
    hi, lo = split(exact)
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)
