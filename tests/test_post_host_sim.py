"""
The arithmetic of the streamed posterior-chain kernels WITHOUT a GPU: tests/host_sim/post_sim.cpp compiles the kernels' own
step functions (markovflow_amd/csrc/mf_post_math.hpp, `__host__ __device__`) for the CPU and runs the three passes - reversed
partitioned elimination per chunk, Kogge-Stone scan over the chunk summaries, emit - lane by lane, with the kernels' chunk
convention.  Checked against the numpy restatement of /root/reference/markovflow/kalman_filter.py:109-182
(oracle.numpy_oracle.kf_posterior_ssm), all five tensors, rtol 1e-9.  What this does NOT cover is the kernels' memory side
(LDS-DMA streams, stores): that is tests/test_gpu_posterior_streamed.py.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import numpy_oracle as O

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
LIB = os.path.join(HERE, "libmf_post_sim.so")
SRC = os.path.join(HERE, "post_sim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "..", "markovflow_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("mf_post_math.hpp", "mf_grad_math.hpp", "mf_kernels.hpp", "mf_small.hpp")]


def _lib():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    stale = not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in [SRC] + HDRS)
    if stale:
        subprocess.check_call([hipcc, "-O1", "-std=c++17", "-shared", "-fPIC", "--offload-arch=gfx950", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    for fn in (lib.mf_post_host_sim_f64, lib.mf_post_host_sim_f32):
        fn.restype = ctypes.c_int
        fn.argtypes = ([ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8 +
                       [ctypes.c_int, ctypes.c_int64] + [ctypes.c_void_p] * 5)
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _draw(rng, bsz, t, d, m, per_step, diag, noise):
    """``(mu0, cholP0, A, b, cholQ, H, y, R^-1)`` of the host tests: transitions ``diag I + noise N``."""
    a = diag * np.eye(d) + noise * rng.normal(size=(bsz, t - 1, d, d))
    cq = np.tril(0.1 * rng.normal(size=(bsz, t - 1, d, d))) + 0.5 * np.eye(d)
    cp0 = np.tril(0.1 * rng.normal(size=(bsz, d, d))) + np.eye(d)
    mu0 = rng.normal(size=(bsz, d))
    b = 0.1 * rng.normal(size=(bsz, t - 1, d))
    h = rng.normal(size=(bsz, t, m, d))
    y = rng.normal(size=(bsz, t, m))
    if per_step:
        r = rng.normal(size=(bsz, t, m, m))
        r_inv = r @ np.swapaxes(r, -1, -2) + np.eye(m)
    else:
        r = rng.normal(size=(m, m))
        r_inv = r @ r.T + np.eye(m)
    return mu0, cp0, a, b, cq, h, y, np.ascontiguousarray(r_inv)


def _entry(lib, base, dtype):
    return getattr(lib, base + ("_f32" if dtype == np.float32 else "_f64"))


def post_host_sim(mu0, cp0, a, b, cq, h, y, r_inv, per_step, length, dtype=np.float64):
    """The three passes in ``dtype`` (numpy float64 or float32) on chunks of ``length`` transitions: ``(return code, (mu0', cholP0',
    A', b', cholQ'))``, the outputs as float64 arrays (NaN where nothing was written)."""
    bsz, t, m, d = h.shape
    ins = [np.ascontiguousarray(x, dtype=dtype) for x in (mu0, cp0, a, b, cq, h, y, r_inv)]
    ap, bp, cqp, mp, cpp = (np.full_like(ins[i], np.nan) for i in (2, 3, 4, 0, 1))
    rc = _entry(_lib(), "mf_post_host_sim", dtype)(bsz, t, d, m, *[_p(x) for x in ins], int(per_step), length, _p(ap), _p(mp), _p(bp),
                                                   _p(cpp), _p(cqp))
    return rc, tuple(x.astype(np.float64) for x in (mp, cpp, ap, bp, cqp))


def grad_host_sim(mu0, cp0, a, b, cq, h, y, r_inv, per_step, length, w, dtype=np.float64):
    """The streamed backward in ``dtype``: ``(return code, (g_mu0, g_cholP0, g_A, g_b, g_cholQ, g_H, g_y, Omega))`` as float64."""
    bsz, t, m, d = h.shape
    ins = [np.ascontiguousarray(x, dtype=dtype) for x in (mu0, cp0, a, b, cq, h, y, r_inv)]
    outs = [np.full_like(x, np.nan) for x in ins[:7]] + [np.full((bsz, t, m, m), np.nan, dtype=dtype)]
    wv = np.ascontiguousarray(w, dtype=dtype)
    rc = _entry(_grad_lib(), "mf_grad_host_sim", dtype)(bsz, t, d, m, *[_p(x) for x in ins], int(per_step), length, _p(wv),
                                                        *[_p(x) for x in outs])
    return rc, tuple(x.astype(np.float64) for x in outs)


POST_SHAPES = [
    (2, 30, 3, 1, 7, False), (2, 30, 6, 1, 5, False), (3, 101, 6, 2, 8, True), (1, 200, 4, 3, 3, False), (2, 2, 6, 1, 1, False),
    (2, 50, 1, 1, 49, False), (2, 50, 2, 1, 60, False), (1, 600, 6, 1, 4, False), (2, 65, 5, 1, 1, False),
]
FLOAT_SANITY = 1e-4     # of a tensor's maximum: a cap that catches a broken float instantiation, not a yardstick (measured: <= 6e-6)


def _to_float32(arrays):
    return [np.asarray(x).astype(np.float32).astype(np.float64) for x in arrays]


def _assert_float_close(names, got, want):
    for name, g, w in zip(names, got, want):
        assert np.all(np.isfinite(g)), name
        err = np.abs(g - w).max() / np.abs(w).max()
        print(f"  float host simulation {name}: {err:.3g} of the tensor's maximum")
        assert err <= FLOAT_SANITY, (name, err)


@pytest.mark.parametrize("bsz,t,d,m,length,per_step", POST_SHAPES)
def test_three_passes_on_the_host_agree_with_the_oracle(bsz, t, d, m, length, per_step):
    mu0, cp0, a, b, cq, h, y, r_inv = _draw(np.random.default_rng(7), bsz, t, d, m, per_step, 0.9, 0.05)
    want = O.kf_posterior_ssm(mu0, cp0, a, b, cq, h, y, r_inv)
    rc, (mp, cpp, ap, bp, cqp) = post_host_sim(mu0, cp0, a, b, cq, h, y, r_inv, per_step, length)
    assert rc == 0
    for name, g, w in zip(("mu0", "cholP0", "A", "b", "cholQ"), (mp, cpp, ap, bp, cqp), want):
        np.testing.assert_allclose(g, w, rtol=1e-9, atol=1e-12, err_msg=name)


def test_host_simulation_flags_a_singular_process_covariance():
    lib = _lib()
    rng = np.random.default_rng(3)
    bsz, t, d, m = 1, 40, 3, 1
    a = 0.5 * np.eye(d) + np.zeros((bsz, t - 1, d, d))
    cq = np.tile(np.eye(d), (bsz, t - 1, 1, 1))
    cq[0, 17] = 0.0
    args = [np.zeros((bsz, d)), np.tile(np.eye(d), (bsz, 1, 1)), a, np.zeros((bsz, t - 1, d)), cq, rng.normal(size=(bsz, t, m, d)),
            rng.normal(size=(bsz, t, m)), np.eye(m)]
    outs = [np.zeros_like(a), np.zeros((bsz, d)), np.zeros((bsz, t - 1, d)), np.zeros((bsz, d, d)), np.zeros_like(cq)]
    rc = lib.mf_post_host_sim_f64(bsz, t, d, m, *[_p(x) for x in args], 0, 8, *[_p(x) for x in outs])
    assert rc == 1


@pytest.mark.parametrize("bsz,t,d,m,length,per_step", POST_SHAPES)
def test_three_passes_on_the_host_in_float_follow_the_double_run(bsz, t, d, m, length, per_step):
    """mf_post_host_sim_f32: the same run_m<T, D> with float buffers, on float32-representable inputs, against the double run."""
    ins = _to_float32(_draw(np.random.default_rng(7), bsz, t, d, m, per_step, 0.9, 0.05))
    rc64, want = post_host_sim(*ins, per_step, length)
    rc32, got = post_host_sim(*ins, per_step, length, dtype=np.float32)
    assert rc64 == 0 and rc32 == 0
    _assert_float_close(("mu0", "cholP0", "A", "b", "cholQ"), got, want)


# ---- the streamed backward of log_likelihood (csrc/mf_grad_math.hpp) ------------------------------------------------------------
def _grad_lib():
    lib = _lib()
    for fn in (lib.mf_grad_host_sim_f64, lib.mf_grad_host_sim_f32):
        fn.restype = ctypes.c_int
        fn.argtypes = ([ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8 +
                       [ctypes.c_int, ctypes.c_int64] + [ctypes.c_void_p] * 9)
    return lib


def _dense_log_likelihood(mu0, cp0, a_s, b_s, cq, h, y, r_inv):
    """log N(y; H mu, H Sigma H^T + blockdiag(R_k)) of ONE series through the dense precision of the chain (the block form of
    /root/reference/markovflow/state_space_model.py:431-483) - plain differentiable torch; r_inv [m, m] or [n, m, m]."""
    import torch
    n, d, m = a_s.shape[0] + 1, mu0.shape[0], h.shape[1]
    eye = torch.eye(d, dtype=mu0.dtype)
    qinv = [torch.cholesky_solve(eye, cp0)] + [torch.cholesky_solve(eye, cq[k]) for k in range(n - 1)]
    prec = torch.zeros(n * d, n * d, dtype=mu0.dtype)
    means = [mu0]
    for k in range(n):
        blk = qinv[k]
        if k < n - 1:
            j = qinv[k + 1] @ a_s[k]
            blk = blk + a_s[k].T @ j
            prec[(k + 1) * d:(k + 2) * d, k * d:(k + 1) * d] = -j
            prec[k * d:(k + 1) * d, (k + 1) * d:(k + 2) * d] = -j.T
            means.append(a_s[k] @ means[k] + b_s[k])
        prec[k * d:(k + 1) * d, k * d:(k + 1) * d] = blk
    hm = torch.block_diag(*[h[i] for i in range(n)])
    r_blocks = [torch.linalg.inv(r_inv if r_inv.dim() == 2 else r_inv[i]) for i in range(n)]
    cov_y = hm @ torch.linalg.inv(prec) @ hm.T + torch.block_diag(*r_blocks)
    res = y.reshape(-1) - hm @ torch.cat(means)
    return -0.5 * (res @ torch.linalg.solve(cov_y, res) + torch.linalg.slogdet(cov_y)[1] + n * m * np.log(2 * np.pi))


GRAD_SHAPES = [
    (2, 12, 3, 1, 4, False), (2, 17, 6, 1, 5, False), (2, 21, 6, 2, 8, True), (1, 30, 4, 3, 3, False), (2, 2, 6, 1, 1, False),
    (2, 9, 1, 1, 50, False), (1, 40, 6, 1, 1, False), (2, 26, 5, 2, 7, False), (2, 14, 2, 1, 2, True),
]


@pytest.mark.parametrize("bsz,t,d,m,length,per_step", GRAD_SHAPES)
def test_streamed_backward_on_the_host_agrees_with_dense_autograd(bsz, t, d, m, length, per_step):
    """Three passes of the posterior chain, start moments per chunk from the two sides of every chunk boundary, then the forward
    pass with the pairwise marginals in registers: every gradient of sum_s w_s log p(y_s) against torch autograd of the dense
    log-likelihood (the precision's gradient through the quadratic form only: its log-determinant is the caller's)."""
    import torch
    rng = np.random.default_rng(11)
    mu0, cp0, a, b, cq, h, y, r_inv = _draw(rng, bsz, t, d, m, per_step, 0.8, 0.1)
    w = rng.uniform(0.5, 1.5, size=bsz)
    rc, got = grad_host_sim(mu0, cp0, a, b, cq, h, y, r_inv, per_step, length, w)
    outs = dict(zip(("gmu0", "gC0", "gA", "gb", "gC", "gH", "gy", "gOm"), got))
    assert rc == 0
    leaves = [torch.tensor(x, requires_grad=True) for x in (mu0, cp0, a, b, cq, h, y, r_inv)]
    total = 0.0
    for s in range(bsz):
        ri = leaves[7][s] if per_step else leaves[7]
        total = total + w[s] * _dense_log_likelihood(*[v[s] for v in leaves[:7]], ri)
    total.backward()
    want = [v.grad.numpy() for v in leaves]
    for name, g, ref in zip(("mu0", "cholP0", "A", "b", "cholQ", "H", "y"), list(outs.values())[:7], want[:7]):
        if name in ("cholP0", "cholQ"):
            ref = np.tril(ref)
        np.testing.assert_allclose(g, ref, rtol=1e-7, atol=1e-9, err_msg=name)
    # d/dR^-1: -1/2 Omega from the quadratic forms, + 1/2 R from the log-determinant (which the kernel leaves to the caller)
    om = outs["gOm"]
    if per_step:
        got = -0.5 * om + 0.5 * w[:, None, None, None] * np.linalg.inv(r_inv)
    else:
        got = -0.5 * om.sum(axis=(0, 1)) + 0.5 * w.sum() * t * np.linalg.inv(r_inv)
    np.testing.assert_allclose(got, 0.5 * (want[7] + np.swapaxes(want[7], -1, -2)), rtol=1e-7, atol=1e-9, err_msg="R^-1")


@pytest.mark.parametrize("bsz,t,d,m,length,per_step", GRAD_SHAPES)
def test_streamed_backward_on_the_host_in_float_follows_the_double_run(bsz, t, d, m, length, per_step):
    """mf_grad_host_sim_f32 on float32-representable inputs against the double run, all eight gradient tensors."""
    rng = np.random.default_rng(11)
    ins = _to_float32(_draw(rng, bsz, t, d, m, per_step, 0.8, 0.1))
    w = _to_float32([rng.uniform(0.5, 1.5, size=bsz)])[0]
    rc64, want = grad_host_sim(*ins, per_step, length, w)
    rc32, got = grad_host_sim(*ins, per_step, length, w, dtype=np.float32)
    assert rc64 == 0 and rc32 == 0
    _assert_float_close(("mu0", "cholP0", "A", "b", "cholQ", "H", "y", "Omega"), got, want)
