"""
GPU tests of ``mf_ssm_log_pdf_*`` / ``mf_ssm_log_pdf_grad_*`` (csrc/mf_logpdf.hip) through the raw C ABI, guard regions around the states and
their adjoint, against tests/helpers/log_pdf_closed_forms.py.  CASES are ``(d, S, B, T, chunks, element offset of states / g_states)``; ``T`` as
a string is taken in tiles of ``240 / (d sizeof)`` steps: no transition; one; one step either side of a tile (the adjoint's rows fill or
overflow their last tile); S below a group of 16, across it and across a wavefront; ragged explicit chunks (11, 11, 9 at d = 2 in float64;
7, 7, 6 at d = 9) and what ``chunks = 0`` picks (5 chunks of 8 at T = 40).  Bound per output: 8 x the yardstick's scaled error, floor 8 eps.
"""
import ctypes

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import log_pdf_closed_forms as LF
from helpers import sde_closed_forms as SC
from test_gpu_nlsde_kernel import DEV, DTYPES, GUARD, NP, guarded, guards_intact, need_reference, stream, tt

pytestmark = pytest.mark.gpu
CASES = [(1, 1, 1, 1, 0, 0), (2, 3, 3, 2, 0, 1), (6, 17, 3, "tile-1", 0, 0), (6, 3, 1, "tile+1", 0, 1), (1, 17, 1, "tile+1", 2, 0),
         (9, 65, 3, "tile", 1, 1), (2, 65, 1, "2tile+1", 3, 0), (6, 17, 3, 40, 0, 0), (9, 3, 3, 20, 3, 1)]


def steps(t, d, dtype):
    tile = 240 // (d * torch.empty((), dtype=dtype).element_size())
    return t if isinstance(t, int) else {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2tile+1": 2 * tile + 1}[t]


def run(case, shape, dtype, chunks, offset=0, want=(True, True, True), upper=0.0):
    """``{output: numpy}`` of one value call and one grad call; ``want``: the value, g_states, the parameter adjoints."""
    bsz, s, t, d = shape
    chain = [tt(case[k], dtype) for k in ("mu0", "cp0", "a", "b", "cq")]
    for k in (1, 4):                                                               # garbage above the diagonal is never read
        chain[k] = chain[k] + upper * torch.triu(torch.ones_like(chain[k]), 1)
    x_buf, x = guarded((s, bsz, t, d), dtype, offset)
    gx_buf, g_x = guarded((s, bsz, t, d), dtype, offset)
    x.copy_(tt(case["x"], dtype))
    g, out = tt(case["g"], dtype), torch.empty((s, bsz), dtype=dtype, device=DEV)
    g_p = [torch.full_like(c, -77.25) for c in chain]
    ptrs = [_lib.ptr(c) if c.numel() else None for c in chain]
    size, res, lib = out.element_size(), {}, _lib.load()

    def workspace(query):
        nbytes = int(query(bsz, s, t, d, size, chunks))
        buf = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
        return buf, ctypes.c_void_p(buf.data_ptr()) if nbytes else None, nbytes

    if want[0]:
        ws, ws_ptr, nbytes = workspace(lib.mf_ssm_log_pdf_workspace_bytes)
        assert _lib.call_rc("mf_ssm_log_pdf", dtype, bsz, s, t, d, *ptrs, _lib.ptr(x), _lib.ptr(out), ws_ptr, nbytes, chunks, stream()) == 0
        assert bool(torch.all(ws[nbytes:] == 0x5A))
        res["out"] = out.cpu().numpy()
    if want[1] or want[2]:
        ws, ws_ptr, nbytes = workspace(lib.mf_ssm_log_pdf_grad_workspace_bytes)
        outs = [_lib.ptr(g_x) if want[1] else None] + [_lib.ptr(p) if want[2] and p.numel() else None for p in g_p]
        assert _lib.call_rc("mf_ssm_log_pdf_grad", dtype, bsz, s, t, d, *ptrs, _lib.ptr(x), _lib.ptr(g), *outs, ws_ptr, nbytes, chunks,
                            stream()) == 0
        assert bool(torch.all(ws[nbytes:] == 0x5A))
        if want[1]:
            res["g_x"] = g_x.cpu().numpy()
        if want[2]:
            res.update({name: p.cpu().numpy() for name, p in zip(LF.OUTPUTS[2:], g_p)})
    torch.cuda.synchronize()
    assert guards_intact(x_buf, (s, bsz, t, d), offset) and guards_intact(gx_buf, (s, bsz, t, d), offset)
    assert torch.equal(x, tt(case["x"], dtype))                                    # the states are read only
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("d,s,bsz,t,chunks,offset", CASES)
def test_value_and_adjoints_against_long_double(d, s, bsz, t, chunks, offset, dtype):
    need_reference(dtype)
    npd, t = NP[dtype], steps(t, d, dtype)
    case = LF.make_case(bsz, s, t, d, np.dtype(npd).name)
    got = run(case, (bsz, s, t, d), dtype, chunks, offset)
    ratios = {}
    for name in LF.OUTPUTS:
        err = float(np.max(SC.scaled_error(got[name], case["ref"][name], case["mag"][name], npd), initial=0.0))
        ratios[name] = err / case["bound"][name]
    print("largest scaled error over its bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0
    for name in ("g_cp0", "g_cq"):
        assert not np.any(np.triu(got[name], 1))                                   # zeros are written above the diagonal


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("s", [17, 65])
def test_outputs_have_the_same_bits_however_they_are_asked_for(s, dtype):
    bsz, t, d, chunks = 3, 12, 6, 3
    case = LF.make_case(bsz, s, t, d, np.dtype(NP[dtype]).name)
    full = run(case, (bsz, s, t, d), dtype, chunks)
    again = run(case, (bsz, s, t, d), dtype, chunks, upper=3.5)                    # a second launch, garbage above the diagonals
    only_x = run(case, (bsz, s, t, d), dtype, chunks, want=(False, True, False))
    only_p = run(case, (bsz, s, t, d), dtype, chunks, want=(False, False, True))
    other = run(case, (bsz, s, t, d), dtype, 1, want=(False, True, True))          # the adjoints do not depend on the chunks
    for name in LF.OUTPUTS:
        for res in (again, only_x, only_p, other):
            assert name not in res or np.array_equal(full[name], res[name]), name
    alone = {k: (v[:, 1:2] if k in ("x", "g") else v[1:2]) for k, v in case.items() if k not in ("ref", "mag", "bound")}
    single = run({k: np.ascontiguousarray(v) for k, v in alone.items()}, (1, s, t, d), dtype, chunks)
    for name in LF.OUTPUTS:                                                        # a series alone: its bits in the batch
        assert np.array_equal(single[name], full[name][:, 1:2] if name in ("out", "g_x") else full[name][1:2]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_argument_errors_and_workspace_queries(dtype):
    case = LF.make_case(3, 65, 12, 6, np.dtype(NP[dtype]).name)
    held = [tt(case[k], dtype) for k in ("mu0", "cp0", "a", "b", "cq", "x", "g")]
    p = [_lib.ptr(v) for v in held]
    out, g_x = torch.empty((65, 3), dtype=dtype, device=DEV), torch.empty((65, 3, 12, 6), dtype=dtype, device=DEV)
    g_p = [_lib.ptr(torch.empty_like(v)) for v in held[:5]]

    def value(bsz=3, s=65, t=12, d=6, x=p[5], chunks=1, dst=_lib.ptr(out)):
        return _lib.call_rc("mf_ssm_log_pdf", dtype, bsz, s, t, d, *p[:5], x, dst, None, 0, chunks, stream())

    def grad(d=6, g=p[6], gx=_lib.ptr(g_x), gp=g_p, chunks=1):
        return _lib.call_rc("mf_ssm_log_pdf_grad", dtype, 3, 65, 12, d, *p[:6], g, gx, *gp, None, 0, chunks, stream())

    assert (value(bsz=-1), value(s=-1), value(t=0), value(d=0), value(d=10), value(x=None), value(chunks=-1)) == (-1, -2, -3, -4, -100, -10, -14)
    assert value(bsz=0, x=None) == 0 and value(s=0, x=None) == 0 and value(dst=None) == 0 and value(chunks=3) == -12
    assert (grad(d=10), grad(g=None), grad(gp=g_p[:2] + [None] + g_p[3:]), grad(chunks=-1)) == (-100, -11, -15, -20)
    assert grad(gx=None, gp=[None] * 5) == 0 and grad() == -18                    # two blocks of 64 samples need their slabs
    lib, size = _lib.load(), out.element_size()
    assert [lib.mf_ssm_log_pdf_workspace_bytes(3, 65, 12, 6, size, c) for c in (1, 3)] == [0, 3 * 195 * size]
    assert [lib.mf_ssm_log_pdf_grad_workspace_bytes(3, s, 12, 6, size, 0) for s in (64, 65)] == [0, 2 * (3 * 42 + 3 * 11 * 78) * size]
