"""
The arithmetic of the LatentExponentiallyGenerated transition kernels (markovflow_amd/csrc/mf_leg_math.hpp) built for the CPU
(tests/host_sim/leg_sim.cpp: the host group holds all rows of a step) and run step by step, forward and reverse, against the long
double reference of tests/helpers/leg_closed_forms.py - no GPU, no sanitizer, nothing preloaded.

Tolerances are measured: per case the yardstick (the same chain in the working dtype in numpy) against the reference, in float64
the larger of that and scipy.linalg.expm's error; the code is allowed 8 x that with a floor of 8 d eps (reverse mode: the floor
scaled by the summed magnitudes of the per-step terms).  See ``leg_closed_forms.allowed``.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg

from helpers import leg_closed_forms as LC

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
LIB = os.path.join(HERE, "libmf_leg_sim.so")
SRC = os.path.join(HERE, "leg_sim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "..", "markovflow_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("mf_leg_math.hpp", "mf_small.hpp")]
GAPS = np.array([1e-5, 1e-3, 0.1, 1.0, 10.0, 40.0])
JITTER = 1e-6
_cache = {}


def _lib():
    if "lib" in _cache:
        return _cache["lib"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    stale = not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in [SRC] + HDRS)
    if stale:
        subprocess.check_call([hipcc, "-O1", "-std=c++17", "-shared", "-fPIC", "--offload-arch=gfx950", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    for name, scalar in (("mf_leg_host_sim_f64", ctypes.c_double), ("mf_leg_host_sim_f32", ctypes.c_float)):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, scalar, ctypes.c_int] + [ctypes.c_void_p] * 6
    _cache["lib"] = lib
    return lib


def run_sim(dtype, f_mat, gaps, jitter, extra=0, g_a=None, g_c=None, reverse=False):
    lib = _lib()
    d, k = f_mat.shape[-1], gaps.shape[0]
    f_mat, gaps = np.ascontiguousarray(f_mat, dtype=dtype), np.ascontiguousarray(gaps, dtype=dtype)
    outs = [np.full((k, d, d), np.nan, dtype=dtype) for _ in range(4)]
    ptr = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    g_a = None if g_a is None else np.ascontiguousarray(g_a, dtype=dtype)
    g_c = None if g_c is None else np.ascontiguousarray(g_c, dtype=dtype)
    fn = lib.mf_leg_host_sim_f64 if dtype == np.float64 else lib.mf_leg_host_sim_f32
    rc = fn(d, k, ptr(f_mat), ptr(gaps), float(jitter), int(extra), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(g_a), ptr(g_c),
            ptr(outs[3]) if reverse else None)
    assert rc == 0
    return outs


def draw(d, dtype, seed):
    rng = np.random.default_rng(seed)
    f_mat = LC.feedback(rng.standard_normal((d, d)), rng.standard_normal((d, d))).astype(dtype)
    return rng, f_mat


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [1, 2, 6, 7, 16])
def test_forward_against_reference(d, dtype):
    if dtype == np.float64 and not LC.longdouble_ok():
        pytest.skip("numpy.longdouble is no wider than a double here: no reference for the float64 accuracy")
    _, f_mat = draw(d, dtype, 100 + d)
    gaps = GAPS.astype(dtype)
    ref = LC.forward(f_mat, gaps, JITTER)
    yard = LC.forward_errors(*LC.forward(f_mat, gaps, JITTER, dtype)[:3], ref)
    other = None
    if dtype == np.float64:
        sp = np.stack([scipy.linalg.expm(float(g) * f_mat) for g in gaps])
        other = LC.forward_errors(sp, None, None, ref)["A"]
    for extra in (0, 3):
        a, q, low, _ = run_sim(dtype, f_mat, gaps, JITTER, extra)
        err = LC.forward_errors(a, q, low, ref)
        for name in ("A", "Q", "L"):
            bound = LC.allowed(yard[name], d, dtype, other if name == "A" else None)
            print(f"d={d} {np.dtype(dtype).name} extra={extra} {name}: ratio to the yardstick bound {np.max(err[name] / bound):.3f}")
            assert np.all(err[name] <= bound), (name, err[name], bound)
        assert np.all(np.triu(low, 1) == 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [1, 2, 6, 7, 16])
def test_reverse_against_reference(d, dtype):
    if dtype == np.float64 and not LC.longdouble_ok():
        pytest.skip("numpy.longdouble is no wider than a double here: no reference for the float64 accuracy")
    rng = np.random.default_rng(200 + d)
    n_mat = np.eye(d) + 0.3 * rng.standard_normal((d, d))
    f_mat = LC.feedback(n_mat, rng.standard_normal((d, d))).astype(dtype)
    gaps = rng.uniform(0.05, 3.0, 9).astype(dtype)
    g_a, g_c = rng.standard_normal((9, d, d)).astype(dtype), rng.standard_normal((9, d, d)).astype(dtype)
    for use_a, use_c in ((True, False), (False, True), (True, True)):
        ga, gc = (g_a if use_a else None), (g_c if use_c else None)
        ref = LC.reverse_terms(f_mat, gaps, JITTER, ga, gc)
        yard = LC.reverse_terms(f_mat, gaps, JITTER, ga, gc, dtype)
        bound = LC.reverse_allowed(ref, yard.sum(axis=0), d, dtype)
        for extra in (0, 2):
            terms = run_sim(dtype, f_mat, gaps, JITTER, extra, ga, gc, reverse=True)[3]
            err = float(np.abs(terms.astype(LC.LD).sum(axis=0) - ref.sum(axis=0)).max())
            print(f"d={d} {np.dtype(dtype).name} gA={use_a} gC={use_c} extra={extra}: error / bound {err / bound:.3f}")
            assert err <= bound


def test_zero_process_noise_and_non_finite_gap():
    d = 6
    rng = np.random.default_rng(5)
    r_mat = rng.standard_normal((d, d))
    f_mat = LC.feedback(np.zeros((d, d)), r_mat).astype(np.float64)       # N = 0: a rotation, Q exactly zero without jitter
    gaps = np.array([0.3, np.nan, 2.0, np.inf])
    g_a = rng.standard_normal((4, d, d))
    a, q, low, terms = run_sim(np.float64, f_mat, gaps, 0.0, 1, g_a, rng.standard_normal((4, d, d)), reverse=True)
    for k in (0, 2):
        assert np.all(q[k] == 0) and np.all(low[k] == 0) and np.all(np.isfinite(a[k]))
        assert np.all(np.isfinite(terms[k]))
    only_a = run_sim(np.float64, f_mat, gaps, 0.0, 1, g_a, None, reverse=True)[3]
    assert np.array_equal(terms[0], only_a[0]) and np.array_equal(terms[2], only_a[2])   # an all-zero Q contributes through gA only
    for k in (1, 3):
        assert np.all(np.isnan(a[k])) and np.all(np.isnan(q[k]))
