"""
GPU tests of ``mf_nlsde_euler_maruyama_*``, ``mf_nlsde_linearize_*`` and ``mf_nlsde_drift_difference_*`` (csrc/mf_nlsde.hip) through the
raw C ABI, with a guard region around every output and workspace, against the long double references of
tests/helpers/sde_closed_forms.py.

Euler-Maruyama, ``(B, T, D)`` = (1, 2, 1): one step; (3, 5, 1); (70, 37, 2): a partial second wavefront and a partial step tile, run on
a uniform and on a non-uniform grid and again with the noise and the output one and two elements past a 16-byte boundary (the aligned
chunks then straddle both ends of every row; (5, 150, 3) runs at one and at three elements: float32 has all three residues); (130, 130, 4): several tiles in time, more than one block, a full ``L``; and two
shapes of our own, (2, 200, 1) and (5, 150, 3): several tiles at the two state dimensions the others leave to one tile.  Inputs:
``dt <= 0.02``, ``|x0| <= 1.5``, the largest eigenvalue of ``q`` is 1; ``make_em_case`` confirms on the CPU that the long double
recurrence stays finite with ``|x| < 3``.  The check is PER STEP, not along the trajectory (the double well amplifies rounding by
``exp(4 t)``): ``out[k + 1]`` against one long double step from the kernel's own ``out[k]`` and the rounded noise.

Quadrature kernels, ``(B, N)`` = (1, 1), (3, 37), (2, 130), (2, 300) and ``nq`` = 1, 10, 20, 32: against the closed forms (``nq >= 4``: the
rule is exact for these polynomials) or the discretised sum in long double (``nq = 1``).  Every case with ``N >= 2`` has one point with
``S <= 0`` and one with a NaN variance, both in series 0.

Tolerances are measured (``sde_closed_forms.allowed``): the yardstick - the same step, the same Gauss-Hermite sum in numpy in the working
dtype - against long double, as errors scaled by the summed magnitudes of the terms; the kernel is allowed 8 x the yardstick's
largest scaled error with a floor of 8 eps.  Every test prints its largest ratio.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import sde_closed_forms as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 64, -77.25
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
LAM = 2.0
EM_CASES = [((1, 2, 1), "uniform", 0), ((3, 5, 1), "uniform", 0), ((70, 37, 2), "uniform", 0), ((70, 37, 2), "nonuniform", 0),
            ((70, 37, 2), "nonuniform", 1), ((130, 130, 4), "uniform", 0), ((2, 200, 1), "uniform", 0), ((5, 150, 3), "nonuniform", 1), ((70, 37, 2), "nonuniform", 2),
            ((5, 150, 3), "nonuniform", 3)]
QUAD_SHAPES = [(1, 1), (3, 37), (2, 130), (2, 300)]
NQS = [1, 10, 20, 32]


def tt(x, dtype):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def guarded(shape, dtype, offset=0):
    """A buffer of ``shape`` that starts ``offset`` elements into its allocation, with sentinels in front of it and behind it."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[offset:offset + n].view(shape)


def guards_intact(buf, shape, offset=0):
    n = int(np.prod(shape))
    return bool(torch.all(buf[:offset] == SENTINEL)) and bool(torch.all(buf[offset + n:] == SENTINEL))


def need_reference(dtype):
    if dtype == torch.float64 and not SC.longdouble_ok():
        pytest.skip("numpy.longdouble is no wider than a double here: no reference for the float64 accuracy")


def doubles(xs):
    return (ctypes.c_double * len(xs))(*[float(x) for x in xs])


def stream():
    return _lib.stream_ptr(torch.device(DEV))


# ---- Euler-Maruyama --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_em_case(shape, grid_kind, dtype_name):
    """Inputs rounded to the working dtype; the long double recurrence from them is confirmed finite with ``|x| < 3`` for both drifts."""
    bsz, tn, d = shape
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(1000 * bsz + 10 * tn + d)
    steps = rng.uniform(0.002, 0.02, tn - 1) if grid_kind == "nonuniform" else np.full(tn - 1, 0.02)
    grid = np.concatenate([[0.25], 0.25 + np.cumsum(steps)]).astype(npd)
    base = rng.standard_normal((d, d))
    q = base @ base.T + 0.1 * np.eye(d)
    q = q / np.linalg.eigvalsh(q)[-1]
    chol = np.linalg.cholesky(q)
    x0 = rng.uniform(-1.5, 1.5, (bsz, d)).astype(npd)
    noise = rng.standard_normal((bsz, tn - 1, d)).astype(npd)
    chol_t = chol.astype(npd)                                                      # what the kernel holds
    for drift_id in (0, 1):
        path = SC.em_path(drift_id, npd(LAM), x0, grid, noise, chol_t)
        assert np.all(np.isfinite(path)) and float(np.max(np.abs(path))) < 3.0
    return dict(grid=grid, chol=chol, chol_t=chol_t, x0=x0, noise=noise)


def run_em(case, shape, dtype, drift_id, noise, offset=0):
    bsz, tn, d = shape
    out_buf, out = guarded((bsz, tn, d), dtype, offset)
    noise_buf, noise_t = guarded((bsz, tn - 1, d), dtype, offset)
    noise_t.copy_(tt(noise, dtype))
    held = [tt(case["x0"], dtype), tt(case["grid"], dtype)]
    packed = doubles([case["chol"][i, j] for i in range(d) for j in range(i + 1)])
    rc = _lib.call_rc("mf_nlsde_euler_maruyama", dtype, bsz, tn, d, drift_id, doubles([LAM]) if drift_id == 0 else None, packed,
                      _lib.ptr(held[0]), _lib.ptr(held[1]), _lib.ptr(noise_t), _lib.ptr(out), stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(out_buf, (bsz, tn, d), offset) and guards_intact(noise_buf, (bsz, tn - 1, d), offset)
    assert torch.equal(noise_t, tt(noise, dtype))                                  # the input stream is read only
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("drift_id", [0, 1], ids=["ou", "double_well"])
@pytest.mark.parametrize("shape,grid_kind,offset", EM_CASES, ids=lambda v: "B%dT%dD%d" % v if isinstance(v, tuple) else str(v))
def test_euler_maruyama_per_step(shape, grid_kind, offset, drift_id, dtype):
    need_reference(dtype)
    npd = NP[dtype]
    case = make_em_case(shape, grid_kind, np.dtype(npd).name)
    out = run_em(case, shape, dtype, drift_id, case["noise"], offset)
    assert out.shape == shape and np.array_equal(out[:, 0], case["x0"])            # bitwise
    assert np.all(np.isfinite(out))
    dts = case["grid"][1:] - case["grid"][:-1]                                     # in the working dtype, as the kernel forms them
    prev, xi = out[:, :-1], case["noise"]
    ref, mag = SC.em_step(drift_id, npd(LAM), prev, xi, dts[None, :], case["chol_t"])
    yard, _ = SC.em_step(drift_id, npd(LAM), prev, xi, dts[None, :], case["chol_t"], npd)
    bound = SC.allowed(SC.scaled_error(yard, ref, mag, npd), npd)
    err = float(np.max(SC.scaled_error(out[:, 1:], ref, mag, npd)))
    print(f"largest scaled error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape,grid_kind", [((70, 37, 2), "nonuniform"), ((130, 130, 4), "uniform")], ids=["B70T37D2", "B130T130D4"])
def test_euler_maruyama_ou_without_noise_is_the_product(shape, grid_kind, dtype):
    """``x0 prod_k (1 - lam dt_k)``.  A step ``x + (-lam x) dt`` rounds three times with relative size at most ``1 + 2 lam dt`` each,
    below 1.1 eps per rounding at ``lam dt <= 0.04``: after k steps a relative error of at most 3.3 k eps; 4 (k + 1) eps is allowed."""
    need_reference(dtype)
    npd = NP[dtype]
    case = make_em_case(shape, grid_kind, np.dtype(npd).name)
    out = run_em(case, shape, dtype, 0, np.zeros_like(case["noise"]))
    dts = (case["grid"][1:] - case["grid"][:-1]).astype(SC.LD)
    factors = np.concatenate([[SC.LD(1)], np.cumprod(1 - SC.LD(npd(LAM)) * dts)])
    want = case["x0"].astype(SC.LD)[:, None, :] * factors[None, :, None]
    allowed = 4 * (np.arange(shape[1]) + 1)[None, :, None] * float(np.finfo(npd).eps) * np.abs(want)
    excess = np.abs(out.astype(SC.LD) - want) / allowed
    print(f"largest error / allowance: {float(np.max(excess)):.3f}")
    assert float(np.max(excess)) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_euler_maruyama_single_time_point_and_empty_batch(dtype):
    x0 = tt(np.array([[0.5, -0.25], [1.0, 0.125]]), dtype)
    out_buf, out = guarded((2, 1, 2), dtype)
    rc = _lib.call_rc("mf_nlsde_euler_maruyama", dtype, 2, 1, 2, 1, None, doubles([1.0, 0.0, 1.0]), _lib.ptr(x0), None, None, _lib.ptr(out),
                      stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(out_buf, (2, 1, 2)) and torch.equal(out[:, 0], x0)
    assert _lib.call_rc("mf_nlsde_euler_maruyama", dtype, 0, 5, 2, 1, None, doubles([1.0, 0.0, 1.0]), None, None, None, None, stream()) == 0


# ---- the quadrature kernels ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_quad_case(shape, nq, drift_id, dtype_name):
    """Inputs rounded to the working dtype, the bad points, and references, magnitudes and yardstick of the seven sums, shared by the
    tests of both kernels."""
    bsz, n = shape
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(100 * bsz + n + 7 * nq + drift_id)
    m = rng.uniform(-1.5, 1.5, shape).astype(npd)
    s = rng.uniform(0.05, 0.6, shape).astype(npd)
    a, b = rng.standard_normal(shape).astype(npd), rng.standard_normal(shape).astype(npd)
    times = np.concatenate([[0.5], 0.5 + np.cumsum(rng.uniform(0.002, 0.02, n))]).astype(npd)
    bad = np.zeros(shape, dtype=bool)
    if n >= 2:
        s[0, 0], s[0, n - 1] = (0.0 if nq % 20 else -0.25), np.nan
        bad[0, 0] = bad[0, n - 1] = True
    safe = np.where(bad, npd(1), s)
    lam = npd(LAM)
    ref = SC.reference_sums(drift_id, lam, nq, m, safe, a, b)
    mag = SC.gh_magnitudes(drift_id, lam, nq, m, safe, a, b)
    yard = SC.gh_sums(drift_id, lam, nq, m, safe, a, b, npd)
    return dict(m=m, s=s, a=a, b=b, times=times, bad=bad, ref=ref, mag=mag, yard=yard)


def rule_args(nq):
    nodes, weights = np.polynomial.hermite.hermgauss(nq)
    return nq, doubles(nodes), doubles(weights)


def params_of(drift_id):
    return doubles([LAM]) if drift_id == 0 else None


def ratio(x, ref, mag, yard, good, npd, what):
    bound = SC.allowed(SC.scaled_error(np.asarray(yard)[good], np.asarray(ref)[good], np.asarray(mag)[good], npd), npd)
    err = float(np.max(SC.scaled_error(np.asarray(x)[good], np.asarray(ref)[good], np.asarray(mag)[good], npd), initial=0.0))
    assert err <= bound, (what, err, bound)
    return err / bound


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("drift_id", [0, 1], ids=["ou", "double_well"])
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=lambda v: "B%dN%d" % v)
def test_linearize(shape, nq, drift_id, dtype):
    need_reference(dtype)
    npd = NP[dtype]
    case = make_quad_case(shape, nq, drift_id, np.dtype(npd).name)
    bsz, n = shape
    chol_l = 0.8
    bufs = [guarded(s, dtype) for s in ((bsz, n, 1, 1), (bsz, n, 1), (bsz, n, 1, 1))]
    held = [tt(case["times"], dtype), tt(case["m"], dtype), tt(case["s"], dtype)]
    rc = _lib.call_rc("mf_nlsde_linearize", dtype, bsz, n, drift_id, params_of(drift_id), chol_l, *rule_args(nq), *[_lib.ptr(t) for t in held],
                      *[_lib.ptr(view) for _, view in bufs], stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert all(guards_intact(buf, view.shape) for buf, view in bufs)
    a_s, b_s, c_s = (view.cpu().numpy().reshape(shape) for _, view in bufs)
    good = ~case["bad"]
    assert np.all(np.isnan(a_s[~good])) and np.all(np.isnan(b_s[~good]))            # NaN at the bad points and nowhere else
    assert np.all(np.isfinite(a_s[good])) and np.all(np.isfinite(b_s[good])) and np.all(np.isfinite(c_s))
    dts = (case["times"][1:] - case["times"][:-1])[None, :]
    dts = np.broadcast_to(dts, shape)
    ref = SC.linearize_from_sums(case["ref"][0], case["ref"][1], case["m"], dts, npd(chol_l), SC.LD)
    mag = SC.linearize_magnitudes(case["mag"][0], case["mag"][1], case["m"], dts, npd(chol_l))
    yard = SC.linearize_from_sums(case["yard"][0], case["yard"][1], case["m"], dts, npd(chol_l), npd)
    everywhere = np.ones(shape, dtype=bool)
    worst = max(ratio(a_s, ref[0], mag[0], yard[0], good, npd, "A"), ratio(b_s, ref[1], mag[1], yard[1], good, npd, "b"),
                ratio(c_s, ref[2], np.broadcast_to(mag[2], shape), yard[2], everywhere, npd, "chol Q"))
    print(f"largest error / bound: {worst:.3f}")


def run_drift_difference(case, shape, dtype, drift_id, nq, scale, grads=True):
    bsz, n = shape
    s_buf, total = guarded((bsz,), dtype)
    g_bufs = [guarded(shape, dtype) for _ in range(4)] if grads else []
    ws_bytes = int(_lib.load().mf_nlsde_drift_difference_workspace_bytes(bsz, n))
    assert ws_bytes == bsz * ((n + 255) // 256) * 8
    ws_buf = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    held = [tt(case[k], dtype) for k in ("m", "s", "a", "b")]
    g_ptrs = [_lib.ptr(view) for _, view in g_bufs] if grads else [None] * 4
    rc = _lib.call_rc("mf_nlsde_drift_difference", dtype, bsz, n, drift_id, params_of(drift_id), *rule_args(nq), scale,
                      *[_lib.ptr(t) for t in held], _lib.ptr(total), *g_ptrs, ctypes.c_void_p(ws_buf.data_ptr()), ws_bytes, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(s_buf, (bsz,)) and all(guards_intact(buf, shape) for buf, _ in g_bufs)
    assert bool(torch.all(ws_buf[ws_bytes:] == 0x5A))
    return total.cpu().numpy(), [view.cpu().numpy() for _, view in g_bufs]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("drift_id", [0, 1], ids=["ou", "double_well"])
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=lambda v: "B%dN%d" % v)
def test_drift_difference(shape, nq, drift_id, dtype):
    need_reference(dtype)
    npd = NP[dtype]
    case = make_quad_case(shape, nq, drift_id, np.dtype(npd).name)
    scale = float(npd(0.01 / 0.7))
    total, grads = run_drift_difference(case, shape, dtype, drift_id, nq, scale)
    again, _ = run_drift_difference(case, shape, dtype, drift_id, nq, scale)
    alone, _ = run_drift_difference(case, shape, dtype, drift_id, nq, scale, grads=False)
    assert total.tobytes() == again.tobytes() == alone.tobytes()                    # the same bits on every call
    good = ~case["bad"]
    worst = 0.0
    for got, idx, what in zip(grads, (3, 4, 5, 6), ("g_m", "g_S", "g_A", "g_b")):
        assert np.all(np.isnan(got[~good])) and np.all(np.isfinite(got[good])), what
        worst = max(worst, ratio(got, case["ref"][idx] * SC.LD(scale), case["mag"][idx] * SC.LD(scale), case["yard"][idx] * npd(scale), good,
                                 npd, what))
    series_bad = case["bad"].any(axis=1)
    assert np.array_equal(np.isnan(total), series_bad)                              # only the series of a bad point is NaN
    ok = ~series_bad
    ref_sum = (case["ref"][2] * SC.LD(scale)).sum(axis=1)
    mag_sum = (case["mag"][2] * SC.LD(scale)).sum(axis=1)
    yard_sum = np.sum((case["yard"][2] * npd(scale)).astype(npd), axis=1, dtype=npd)
    if ok.any():
        worst = max(worst, ratio(total, ref_sum, mag_sum, yard_sum, ok, npd, "sum"))
    print(f"largest error / bound: {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_drift_difference_single_bad_point_and_empty_series(dtype):
    case = dict(m=np.zeros((1, 1)), s=np.zeros((1, 1)), a=np.ones((1, 1)), b=np.ones((1, 1)))
    total, grads = run_drift_difference(case, (1, 1), dtype, 1, 10, 1.0)
    assert np.isnan(total[0]) and all(np.isnan(g[0, 0]) for g in grads)
    s_buf, out = guarded((3,), dtype)
    rc = _lib.call_rc("mf_nlsde_drift_difference", dtype, 3, 0, 1, None, *rule_args(10), 1.0, None, None, None, None, _lib.ptr(out), None, None,
                      None, None, None, 0, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(s_buf, (3,)) and bool(torch.all(out == 0))
