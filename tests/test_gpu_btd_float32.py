"""
float32 of the block-tridiagonal operators on every route of the shipped build: ``cholesky``, ``solve``, ``dense_mult``,
``abs_log_det``, the blocks of the inverse, ``upper_diagonal_lower`` (plain, and with the posterior chain's extras in both layouts)
and the fused ``mf_btd_logdet_quad_f32`` - the float32 instantiations of the kernels tests/test_gpu_block_tri_diag.py,
tests/test_gpu_btd_parallel.py, tests/test_gpu_large_d_ops.py and tests/test_gpu_wave.py pin in float64 and only smoke-test in
float32 (rtol 2e-3 there: four orders of magnitude above what float32 is entitled to).

Through the public API on float32 tensors made from float32-rounded draws.  Every case asserts its route from the public planning
functions and, with the ``abi_calls`` spy, that the expected ``mf_btd_*`` entry point ran in float32 and returned 0.  Judged as
tests/helpers/btd_fp32_cases.py states: against the sequential closed form in float64 on the inputs the kernel saw, within
FP32_FACTOR x the error of the closed forms in float32 on the CPU (tests/helpers/btd_fp32_table.py).  The strict upper triangles
of the returned factors are exactly zero, as the float64 tests require (they compare with ``np.tril`` of the oracle's).

What would be caught: a lost Newton step of a reciprocal square root (1e-4 .. 1e-6 of every pivot), a Schur complement accumulated
from a stale pivot on one level of the hierarchy or in a ragged last chunk (the shapes cut the time axis with a ragged tail, over
one, two and three levels), a sub-diagonal block of the inverse taken from the wrong neighbour.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from helpers import btd_fp32_cases as C
from helpers import btd_fp32_table as TABLE
from helpers.btd_fp32_cases import abi_calls  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64


def tt(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), dtype=F32, device=DEV)


def report(what, errs, yard):
    """Print every figure, then assert: measured error <= FP32_FACTOR x the closed forms' in float32."""
    assert set(errs) == set(yard), (sorted(errs), sorted(yard))
    worst = max(errs[name] / yard[name] for name in errs)
    for name, e in errs.items():
        print(f"  fp32 {what} {name}: error {e:.3g} (closed form in float32 {yard[name]:.3g}, ratio {e / yard[name]:.2f})")
    print(f"  fp32 {what}: worst ratio {worst:.2f}")
    for name, e in errs.items():
        assert e <= C.FP32_FACTOR * yard[name], (what, name, e, yard[name])


def assert_route(route, d, t, bsz):
    """The predicate of the route, from the public planning functions with elem_size 4."""
    lib = _lib.load()
    ws = (int(lib.mf_btd_cholesky_workspace_bytes(bsz, t, d, 4)), int(lib.mf_btd_solve_workspace_bytes(bsz, bsz, t, d, 4)),
          int(lib.mf_btd_diag_of_inverse_workspace_bytes(bsz, t, d, 4)), int(lib.mf_btd_udl_workspace_bytes(bsz, t, d, 4)))
    cover = int(lib.mf_row_operators_cover(bsz, t, d, 4))
    if route == "sweep":                   # one lane per series
        assert d <= 9 and ws == (0, 0, 0, 0) and cover == 1
    elif route == "lane_par":              # a lane per chunk
        assert d <= 4 and min(ws) > 0 and cover == 1
    elif route == "row_par":               # a 16-lane row per chunk
        assert 5 <= d <= 9 and min(ws) > 0 and cover == 1
    elif route == "row":
        assert 10 <= d <= 15 and cover == 1
    elif route == "tile":
        assert 10 <= d <= 15 and t == 1 and cover == 0
    elif route == "wave":
        assert 16 <= d <= 32 and cover == 0
    else:
        assert route == "panel" and 33 <= d <= 64 and cover == 0
    if d <= 15:                            # the helper's restatement of the plan is the library's
        assert (C.par_len0(bsz, t, d) > 0) == (ws[0] > 0) == (ws[1] > 0) == (ws[2] > 0)
    return cover == 1


def took(calls, name):
    """``name`` ran in float32 and returned 0; nothing was called in float64, nothing returned an error; then forget the calls."""
    assert name in C.ran(calls, F32), (name, calls)
    assert [c for c in calls if c[2] != 0 or c[1] == F64] == [], calls
    del calls[:]


def strictly_lower(x):
    return float(torch.triu(x, diagonal=1).abs().max()) == 0.0


@pytest.mark.parametrize("route,d,t,bsz", C.CASES)
def test_matrix_operators_fp32(abi_calls, route, d, t, bsz):
    """cholesky, symmetric dense_mult, upper_diagonal_lower, _udl(eta) in both layouts."""
    chain_layout = assert_route(route, d, t, bsz)
    diag, sub, x, eta, want = C.spd_reference(d, t, bsz)
    sym = mfa.SymmetricBlockTriDiagonal(tt(diag), tt(sub))
    errs = {}
    chol = sym.cholesky
    took(abi_calls, "mf_btd_cholesky")
    assert chol.block_diagonal.dtype == F32 and strictly_lower(chol.block_diagonal)
    errs["chol.diag"] = C.error("chol.diag", chol.block_diagonal, want["chol.diag"], t, d)
    errs["sym.mult"] = C.error("sym.mult", sym.dense_mult(tt(x)), want["sym.mult"], t, d)
    took(abi_calls, "mf_btd_matvec")
    if t > 1:
        errs["chol.sub"] = C.error("chol.sub", chol.block_sub_diagonal, want["chol.sub"], t, d)
        u_t, chol_d = sym.upper_diagonal_lower()
        took(abi_calls, "mf_btd_udl")
        assert strictly_lower(chol_d.block_diagonal) and chol_d.block_sub_diagonal is None
        assert torch.equal(u_t.block_diagonal, torch.eye(d, dtype=F32, device=DEV).expand(bsz, t, d, d))
        errs["udl.u_t"] = C.error("udl.u_t", u_t.block_sub_diagonal, want["udl.u_t"], t, d)
        errs["udl.chol_d"] = C.error("udl.chol_d", chol_d.block_diagonal, want["udl.chol_d"], t, d)
        got = sym._udl(tt(eta))
        took(abi_calls, "mf_btd_udl")
        assert strictly_lower(got[1]) and strictly_lower(got[3])
        for name, g in zip(("eta.u_t", "eta.chol_d", "eta.m_post", "eta.chol_dinv"), got):
            errs[name] = C.error(name, g, want[name], t, d)
    report(f"btd {route} d={d} T={t} B={bsz}", errs, {k: v for k, v in TABLE.BTD[(route, d, t, bsz)].items() if k in C.names_of(t)[0]})
    if t > 1 and chain_layout:
        # the same quantities in the layout of a posterior chain: transitions -U^T, (mu0', b'), (cholP0', cholQ')
        a_post, none, (mu0, offs), (cp0, cq) = sym._udl(tt(eta), chain=True)
        took(abi_calls, "mf_btd_udl")
        assert none is None and strictly_lower(cp0) and strictly_lower(cq)
        errs = {"eta.u_t": C.error("eta.u_t", -a_post, want["eta.u_t"], t, d),
                "eta.m_post": C.error("eta.m_post", torch.cat([mu0[:, None], offs], dim=1), want["eta.m_post"], t, d),
                "eta.chol_dinv": C.error("eta.chol_dinv", torch.cat([cp0[:, None], cq], dim=1), want["eta.chol_dinv"], t, d)}
        report(f"btd chain layout {route} d={d} T={t} B={bsz}", errs, {k: TABLE.BTD[(route, d, t, bsz)][k] for k in errs})
    elif t > 1:
        # the MFMA engines do not write the chain layout: -101, raised (include/markovflow_amd.h, mf_btd_udl)
        with pytest.raises(NotImplementedError):
            sym._udl(tt(eta), chain=True)
        assert [(name, rc) for name, _, rc in abi_calls if rc != 0] == [("mf_btd_udl", -101)]


@pytest.mark.parametrize("route,d,t,bsz", C.CASES)
def test_factor_operators_fp32(abi_calls, route, d, t, bsz):
    """solve and dense_mult in both transposes, abs_log_det, the blocks of the inverse - on a factor drawn directly."""
    assert_route(route, d, t, bsz)
    ldiag, lsub, rhs, want = C.factor_reference(d, t, bsz)
    low = mfa.LowerTriangularBlockTriDiagonal(tt(ldiag), tt(lsub))
    r = tt(rhs)
    errs = {}
    for name, transpose in (("solve", False), ("solve_t", True)):
        errs[name] = C.error(name, low.solve(r, transpose_left=transpose), want[name], t, d)
        took(abi_calls, "mf_btd_solve")
    for name, transpose in (("mult", False), ("mult_t", True)):
        errs[name] = C.error(name, low.dense_mult(r, transpose_left=transpose), want[name], t, d)
        took(abi_calls, "mf_btd_matvec")
    logdet = low.abs_log_det()
    took(abi_calls, "mf_btd_logdet")
    assert logdet.dtype == F32 and tuple(logdet.shape) == (bsz,)
    errs["logdet"] = C.error("logdet", logdet, want["logdet"], t, d)
    inv_d, inv_s = low._diag_and_sub_of_inverse(want_sub=True)
    took(abi_calls, "mf_btd_diag_of_inverse")
    errs["inv.diag"] = C.error("inv.diag", inv_d, want["inv.diag"], t, d)
    if t > 1:
        errs["inv.sub"] = C.error("inv.sub", inv_s, want["inv.sub"], t, d)
    else:
        assert inv_s is None
    alone = low.block_diagonal_of_inverse()
    took(abi_calls, "mf_btd_diag_of_inverse")
    errs["inv.diag"] = max(errs["inv.diag"], C.error("inv.diag", alone, want["inv.diag"], t, d))
    report(f"btd factor {route} d={d} T={t} B={bsz}", errs, {k: v for k, v in TABLE.BTD[(route, d, t, bsz)].items() if k in C.names_of(t)[1]})


@pytest.mark.parametrize("route,d,t,bsz", C.NO_SUB_CASES)
def test_block_diagonal_matrix_fp32(abi_calls, route, d, t, bsz):
    """The same generator without a sub-diagonal: every block is a chain of its own."""
    diag, sub, x, _, want = C.spd_reference(d, t, bsz, C.DEFAULT_SEED, False)
    assert sub is None
    sym = mfa.SymmetricBlockTriDiagonal(tt(diag))
    chol = sym.cholesky
    took(abi_calls, "mf_btd_cholesky")
    assert chol.block_sub_diagonal is None and strictly_lower(chol.block_diagonal)
    errs = {"chol.diag": C.error("chol.diag", chol.block_diagonal, want["chol.diag"], t, d),
            "sym.mult": C.error("sym.mult", sym.dense_mult(tt(x)), want["sym.mult"], t, d)}
    took(abi_calls, "mf_btd_matvec")
    report(f"btd no sub-diagonal {route} d={d} T={t} B={bsz}", errs, TABLE.NO_SUB[(route, d, t, bsz)])


def logdet_quad(d, t, bsz, diag, sub, rhs):
    """``(return code, out [B], info word)`` of mf_btd_logdet_quad_f32 with the workspace its query names."""
    dev = torch.device(DEV)
    ws_bytes = int(_lib.load().mf_btd_logdet_quad_workspace_bytes(bsz, t, d, 4))
    ws = _lib.workspace(ws_bytes, dev)
    out = torch.full((bsz,), float("nan"), dtype=F32, device=DEV)
    info = _lib.new_info(dev)
    rc = _lib.call_rc("mf_btd_logdet_quad", F32, bsz, t, d, _lib.ptr(diag), _lib.ptr(sub), _lib.ptr(rhs), _lib.ptr(out), _lib.ptr(ws),
                      ws_bytes, _lib.ptr(info), _lib.stream_ptr(dev))
    return rc, out, int(info.item())


@pytest.mark.parametrize("route,d,t,bsz", C.LOGDET_QUAD_CASES)
def test_logdet_quad_fp32(abi_calls, route, d, t, bsz):
    """The fused 1/2 |L^-1 r|^2 - log|L| (nothing in Python calls the float32 instantiation)."""
    diag, sub, x, want = C.logdet_quad_reference(d, t, bsz)
    rc, out, info = logdet_quad(d, t, bsz, tt(diag), tt(sub), tt(x))
    assert rc == 0 and info == 0 and abi_calls == [("mf_btd_logdet_quad", F32, 0)]
    report(f"logdet_quad {route} d={d} T={t} B={bsz}", {"logdet_quad": C.error("logdet_quad", out, want, t, d)},
           {"logdet_quad": TABLE.LOGDET_QUAD[(route, d, t, bsz)]})


@pytest.mark.parametrize("d,t,bsz", C.LOGDET_QUAD_UNSUPPORTED)
def test_logdet_quad_fp32_beyond_the_register_kernels(d, t, bsz):
    """-100, "state dimension not instantiated for this entry point" (include/markovflow_amd.h), and nothing written."""
    diag, sub, x, _ = C.draw_spd(C.DEFAULT_SEED, d, t, bsz)
    rc, out, info = logdet_quad(d, t, bsz, tt(diag), tt(sub), tt(x))
    assert rc == -100 and info == 0 and bool(torch.isnan(out).all())
