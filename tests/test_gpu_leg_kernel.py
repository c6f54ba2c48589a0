"""
GPU tests of ``mf_sde_leg_transitions_*`` and ``mf_sde_leg_transitions_grad_*`` (csrc/mf_leg.hip) through the raw C ABI, with a guard
region behind every output, against the long double reference of tests/helpers/leg_closed_forms.py.

State dimensions 1, 2, 3, 6, 7, 15, 16: one below and one at every edge of the lane layout (groups of 1, 2, 4, 8 and 16 lanes per
step).  ``(B, n)`` = (3, 37): a partial last wavefront and wavefronts that straddle two series; (2, 130): more than one block per
series in the reverse mode at every group width; (1, 1).  Gaps are drawn per step from {1e-5, 1e-3, 0.1, 1, 10, 40}, so that
neighbouring steps of one wavefront need different numbers of squarings; one step has a gap of 1e10.

Tolerances are measured per case (``leg_closed_forms.allowed``): the yardstick - the same chain in the working dtype in numpy - against
the reference, in float64 the larger of that and scipy.linalg.expm's error; the kernel is allowed 8 x that with a floor of
8 d eps (reverse mode: the floor scaled by the summed magnitudes of the per-step terms).  Every test prints its largest ratio.
"""
import numpy as np
import pytest
import scipy.linalg
import torch

from markovflow_amd import _lib
from helpers import leg_closed_forms as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 64, -77.25
JITTER = 1e-6
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
DIMS = [1, 2, 3, 6, 7, 15, 16]
SHAPES = [(3, 37), (2, 130), (1, 1)]
GAPS = np.array([1e-5, 1e-3, 0.1, 1.0, 10.0, 40.0])


def tt(x, dtype):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def guards_intact(*bufs):
    return all(b is None or bool(torch.all(b[-GUARD:] == SENTINEL)) for b in bufs)


def need_reference(dtype):
    if dtype == torch.float64 and not LC.longdouble_ok():
        pytest.skip("numpy.longdouble is no wider than a double here: no reference for the float64 accuracy")


def draw_feedback(rng, d, count, dtype, near_identity=False):
    """``count`` feedback matrices rounded to ``dtype`` (the kernel's input IS the rounded matrix)."""
    out = []
    for _ in range(count):
        n_mat = np.eye(d) + 0.3 * rng.standard_normal((d, d)) if near_identity else rng.standard_normal((d, d))
        out.append(LC.feedback(n_mat, rng.standard_normal((d, d))).astype(NP[dtype]))
    return np.stack(out)


def run_forward(dtype, f_dev, per_series, dt_dev, jitter, d, want_chol, want_cov):
    bsz, n = dt_dev.shape
    bufs = [guarded((bsz, n, d, d), dtype) if w else (None, None) for w in (True, want_chol, want_cov)]
    rc = _lib.call_rc("mf_sde_leg_transitions", dtype, bsz, n, d, _lib.ptr(f_dev), int(per_series), _lib.ptr(dt_dev), jitter,
                      *[_lib.ptr(v) for _, v in bufs], _lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(*[b for b, _ in bufs])
    return [None if v is None else v.cpu().numpy() for _, v in bufs]


def run_reverse(dtype, f_dev, per_series, dt_dev, jitter, d, g_a, g_c):
    bsz, n = dt_dev.shape
    buf, out = guarded((bsz, d, d), dtype)
    ws_bytes = int(_lib.load().mf_sde_leg_transitions_grad_workspace_bytes(bsz, n, d, dt_dev.element_size()))
    ws_buf = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = _lib.call_rc("mf_sde_leg_transitions_grad", dtype, bsz, n, d, _lib.ptr(f_dev), int(per_series), _lib.ptr(dt_dev), jitter,
                      _lib.ptr(g_a), _lib.ptr(g_c), _lib.ptr(out), _lib.ptr(ws_buf), ws_bytes, _lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(buf) and bool(torch.all(ws_buf[ws_bytes:] == 0x5A))
    return out.clone()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("per_series", [False, True], ids=["shared", "per_series"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}n{s[1]}")
@pytest.mark.parametrize("d", DIMS)
def test_forward(d, shape, per_series, dtype):
    need_reference(dtype)
    bsz, n = shape
    npd = NP[dtype]
    rng = np.random.default_rng(1000 * d + 10 * bsz + n + int(per_series))
    f_np = draw_feedback(rng, d, bsz if per_series else 1, dtype)
    gaps = GAPS[rng.integers(0, len(GAPS), size=(bsz, n))].astype(npd)
    if n > 2:
        gaps[bsz - 1, n // 2] = npd(1e10)
    f_steps = np.repeat(f_np, n, axis=0) if per_series else np.broadcast_to(f_np[0], (bsz * n, d, d))
    flat = gaps.reshape(-1)
    ref = LC.forward(f_steps, flat, JITTER)
    yard = LC.forward_errors(*LC.forward(f_steps, flat, JITTER, npd)[:3], ref)
    other = None
    if dtype == torch.float64:
        sp = np.stack([scipy.linalg.expm(float(g) * f) for g, f in zip(flat, f_steps)])
        other = LC.forward_errors(sp, None, None, ref)["A"]
    f_dev, dt_dev = tt(f_np if per_series else f_np[0], dtype), tt(gaps, dtype)
    worst = 0.0
    for want_chol, want_cov in ((False, False), (True, False), (False, True), (True, True)):
        a, low, q = run_forward(dtype, f_dev, per_series, dt_dev, JITTER, d, want_chol, want_cov)
        err = LC.forward_errors(a.reshape(-1, d, d), None if q is None else q.reshape(-1, d, d),
                                None if low is None else low.reshape(-1, d, d), ref)
        for name, e in err.items():
            bound = LC.allowed(yard[name], d, npd, other if name == "A" else None)
            worst = max(worst, float(np.max(e / bound)))
            assert np.all(e <= bound), (name, want_chol, want_cov, float(np.max(e / bound)))
        if low is not None:
            assert np.all(np.triu(low, 1) == 0)
        if q is not None:
            assert np.array_equal(q, np.swapaxes(q, -1, -2))
    if n > 2:                                                     # the gap of 1e10: A -> 0, Q -> (1 + jitter) I
        big = (bsz - 1) * n + n // 2
        assert np.max(np.abs(a.reshape(-1, d, d)[big])) < 1e-6
        assert np.max(np.abs(q.reshape(-1, d, d)[big] - (1 + JITTER) * np.eye(d))) < 1e-5
    print(f"forward d={d} B={bsz} n={n} per_series={per_series} {np.dtype(npd).name}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_zero_process_noise_and_nan_gap(dtype):
    d, bsz, n = 6, 2, 20
    rng = np.random.default_rng(7)
    f_np = LC.feedback(np.zeros((d, d)), rng.standard_normal((d, d))).astype(NP[dtype])      # N = 0: Q is exactly zero
    gaps = rng.uniform(0.05, 3.0, (bsz, n)).astype(NP[dtype])
    gaps[1, 7] = np.nan
    a, low, q = run_forward(dtype, tt(f_np, dtype), False, tt(gaps, dtype), 0.0, d, True, True)
    bad = np.zeros((bsz, n), dtype=bool)
    bad[1, 7] = True
    assert np.all(np.isnan(a[bad])) and np.all(np.isnan(q[bad]))
    assert np.all(np.isnan(low[bad][:, np.tril_indices(d)[0], np.tril_indices(d)[1]])) and np.all(np.triu(low[bad], 1) == 0)
    assert np.all(np.isfinite(a[~bad])) and np.all(q[~bad] == 0) and np.all(low[~bad] == 0)


def test_return_codes():
    dtype, d = torch.float64, 3
    f_dev, dt_dev = tt(np.zeros((d, d)), dtype), tt(np.ones((2, 5)), dtype)
    out = torch.zeros((2, 5, d, d), dtype=dtype, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))
    call = lambda *a: _lib.call_rc("mf_sde_leg_transitions", dtype, *a, st)
    assert call(2, 5, 17, _lib.ptr(f_dev), 0, _lib.ptr(dt_dev), 0.0, _lib.ptr(out), None, None) == -100
    assert call(2, 5, 0, _lib.ptr(f_dev), 0, _lib.ptr(dt_dev), 0.0, _lib.ptr(out), None, None) == -3
    assert call(-1, 5, d, _lib.ptr(f_dev), 0, _lib.ptr(dt_dev), 0.0, _lib.ptr(out), None, None) == -1
    assert call(2, -5, d, _lib.ptr(f_dev), 0, _lib.ptr(dt_dev), 0.0, _lib.ptr(out), None, None) == -2
    assert call(2, 5, d, None, 0, _lib.ptr(dt_dev), 0.0, _lib.ptr(out), None, None) == -4
    assert call(2, 5, d, _lib.ptr(f_dev), 0, None, 0.0, _lib.ptr(out), None, None) == -6
    assert call(2, 5, d, _lib.ptr(f_dev), 0, _lib.ptr(dt_dev), 0.0, None, None, None) == -8
    assert call(0, 5, d, None, 0, None, 0.0, None, None, None) == 0
    assert call(2, 0, d, None, 0, None, 0.0, None, None, None) == 0
    grad = lambda *a: _lib.call_rc("mf_sde_leg_transitions_grad", dtype, *a, st)
    g_out = torch.zeros((2, d, d), dtype=dtype, device=DEV)
    ws_bytes = int(_lib.load().mf_sde_leg_transitions_grad_workspace_bytes(2, 5, d, 8))
    assert ws_bytes > 0 and int(_lib.load().mf_sde_leg_transitions_grad_workspace_bytes(2, 5, 17, 8)) == 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    base = (2, 5, d, _lib.ptr(f_dev), 0, _lib.ptr(dt_dev), 0.0, _lib.ptr(out), None)
    assert grad(2, 5, 17, *base[3:], _lib.ptr(g_out), _lib.ptr(ws), ws_bytes) == -100
    assert grad(*base, None, _lib.ptr(ws), ws_bytes) == -10
    assert grad(*base, _lib.ptr(g_out), None, ws_bytes) == -11
    assert grad(*base, _lib.ptr(g_out), _lib.ptr(ws), ws_bytes - 1) == -12
    assert grad(0, 5, d, None, 0, None, 0.0, None, None, None, None, 0) == 0
    assert grad(*base, _lib.ptr(g_out), _lib.ptr(ws), ws_bytes) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("per_series", [False, True], ids=["shared", "per_series"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}n{s[1]}")
@pytest.mark.parametrize("d", DIMS)
def test_reverse(d, shape, per_series, dtype):
    need_reference(dtype)
    bsz, n = shape
    npd = NP[dtype]
    rng = np.random.default_rng(2000 * d + 10 * bsz + n + int(per_series))
    f_np = draw_feedback(rng, d, bsz if per_series else 1, dtype, near_identity=True)
    gaps = rng.uniform(0.05, 3.0, (bsz, n)).astype(npd)
    g_a = rng.standard_normal((bsz, n, d, d)).astype(npd)
    g_c = rng.standard_normal((bsz, n, d, d)).astype(npd)
    garbage = g_c + np.triu(1e3 * rng.standard_normal((d, d)), 1).astype(npd)       # the strict upper triangle must not matter
    f_dev, dt_dev = tt(f_np if per_series else f_np[0], dtype), tt(gaps, dtype)
    worst = 0.0
    for use_a, use_c in ((True, False), (False, True), (True, True)):
        out = run_reverse(dtype, f_dev, per_series, dt_dev, JITTER, d, tt(g_a, dtype) if use_a else None,
                          tt(garbage, dtype) if use_c else None)
        again = run_reverse(dtype, f_dev, per_series, dt_dev, JITTER, d, tt(g_a, dtype) if use_a else None,
                            tt(garbage, dtype) if use_c else None)
        assert torch.equal(out, again)
        out = out.cpu().numpy()
        for b in range(bsz):
            f_b = f_np[b] if per_series else f_np[0]
            ga, gc = (g_a[b] if use_a else None), (g_c[b] if use_c else None)
            ref = LC.reverse_terms(f_b, gaps[b], JITTER, ga, gc)
            yard = LC.reverse_terms(f_b, gaps[b], JITTER, ga, gc, npd)
            bound = LC.reverse_allowed(ref, yard.sum(axis=0), d, npd)
            err = float(np.abs(out[b].astype(LC.LD) - ref.sum(axis=0)).max())
            worst = max(worst, err / bound)
            assert err <= bound, (use_a, use_c, b, err / bound)
    print(f"reverse d={d} B={bsz} n={n} per_series={per_series} {np.dtype(npd).name}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("d", [2, 6, 13])
def test_carried_form_contract_float32(d):
    """At a gap of 1e-5 in float32, ``I - A A^T`` from a correctly rounded ``A`` is wrong by more than 1e-4 relative (or not positive
    definite) - shown here on the CPU first - while the kernel's ``Q`` holds the measured tolerance: the carried form's contract."""
    rng = np.random.default_rng(31 + d)
    f_np = draw_feedback(rng, d, 1, torch.float32)[0]
    gaps = np.full(8, 1e-5, dtype=np.float32)
    ref = LC.forward(f_np, gaps, 0.0)
    a32 = ref[0].astype(np.float32)                                       # A rounded correctly to float32
    naive = np.eye(d, dtype=np.float32) - a32 @ np.swapaxes(a32, -1, -2)
    naive_err = float(np.max(np.abs(naive.astype(LC.LD) - ref[1]).max(axis=(-1, -2)) / np.abs(ref[1]).max(axis=(-1, -2))))
    with np.errstate(invalid="ignore"):
        not_pd = bool(np.any(np.isnan(LC.cholesky(naive)[0])))
    print(f"d={d}: I - A A^T in float32 at dt = 1e-5: relative error {naive_err:.2e}, Cholesky fails: {not_pd}")
    assert naive_err > 1e-4 or not_pd
    yard = LC.forward_errors(*LC.forward(f_np, gaps, 0.0, np.float32)[:3], ref)
    _, low, q = run_forward(torch.float32, tt(f_np, torch.float32), False, tt(gaps[None], torch.float32), 0.0, d, True, True)
    err = LC.forward_errors(None, q.reshape(-1, d, d), low.reshape(-1, d, d), ref)
    for name in ("Q", "L"):
        assert np.all(err[name] <= LC.allowed(yard[name], d, np.float32)), (name, err[name])
