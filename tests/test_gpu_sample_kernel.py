"""
GPU tests of ``mf_ssm_sample_*`` (csrc/mf_sample.hip) through the raw C ABI, guard regions around ``out``, ``eps`` and the workspace, against
the long double recursion of tests/helpers/sample_closed_forms.py.  CASES are ``(B, S, T, d, chunks, element offset of eps / out, full
cholQ block)``: no transition; one step; ``r % B`` with S != B; a partial second wavefront, odd d, rows off the 16-byte boundary; the
largest d; chunks of 17, 17, 16 (again with a FULL block: the lower triangle times an orthogonal matrix); ragged chunks, misaligned; more
chunks than steps; whatever ``chunks = 0`` picks.

Bound (``sde_closed_forms.allowed``): the largest error scaled by the magnitude recursion is at most 8 x the numpy yardstick's, floor 8
eps, along the whole trajectory; the partitioned cases' other association is at most three sums of the same magnitude, inside the
floor's 64 eps.  ``|A|`` of a Matern chain is not contractive, so that magnitude holds late steps loosely: the rule is applied again with
the magnitude of ONE step on the reference's states (``local_magnitude``).  Every test prints both ratios.
"""
import ctypes

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import sample_closed_forms as SF
from helpers import sde_closed_forms as SC
from test_gpu_nlsde_kernel import DEV, DTYPES, GUARD, NP, guarded, guards_intact, need_reference, stream, tt

pytestmark = pytest.mark.gpu
CASES = [(1, 1, 1, 1, 0, 0, False), (1, 1, 2, 1, 1, 0, False), (2, 3, 5, 2, 1, 0, False), (3, 70, 37, 3, 1, 1, False),
         (1, 2, 20, 9, 1, 0, False), (2, 5, 50, 6, 3, 0, False), (2, 5, 50, 6, 3, 0, True), (3, 70, 37, 3, 4, 1, False),
         (1, 2, 2, 4, 3, 0, False), (2, 16, 200, 6, 0, 0, False)]


def run_sample(case, shape, dtype, chunks, offset):
    bsz, s, t, d = shape
    full = (s, bsz, t, d)
    out_buf, out = guarded(full, dtype, offset)
    eps_buf, eps = guarded(full, dtype, offset)
    eps.copy_(tt(case["eps"], dtype))
    held = [tt(case[k], dtype) for k in ("mu0", "cp0", "a", "b", "cq")]
    ws_bytes = int(_lib.load().mf_ssm_sample_workspace_bytes(bsz, s, t, d, out.element_size(), chunks))
    ws_buf = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = _lib.call_rc("mf_ssm_sample", dtype, bsz, s, t, d, *[_lib.ptr(x) if x.numel() else None for x in held], _lib.ptr(eps),
                      _lib.ptr(out), ctypes.c_void_p(ws_buf.data_ptr()) if ws_bytes else None, ws_bytes, chunks, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(out_buf, full, offset) and guards_intact(eps_buf, full, offset)
    assert bool(torch.all(ws_buf[ws_bytes:] == 0x5A))
    assert torch.equal(eps, tt(case["eps"], dtype))                                # the input stream is read only
    return out.cpu().numpy(), ws_bytes


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("bsz,s,t,d,chunks,offset,full_block", CASES)
def test_sample_against_long_double(bsz, s, t, d, chunks, offset, full_block, dtype):
    need_reference(dtype)
    npd = NP[dtype]
    case = SF.make_case(bsz, s, t, d, np.dtype(npd).name, full_block)
    out, ws_bytes = run_sample(case, (bsz, s, t, d), dtype, chunks, offset)
    assert (ws_bytes > 0) == (chunks > 1 or (chunks == 0 and t >= 64))             # the regime the case is meant to reach
    err = float(np.max(SC.scaled_error(out, case["ref"], case["mag"], npd)))
    local = float(np.max(SC.scaled_error(out, case["ref"], case["local"], npd)))
    print(f"largest scaled error {err:.3e}, bound {case['bound']:.3e}, ratio {err / case['bound']:.3f}; by the local magnitude "
          f"{local:.3e}, bound {case['local_bound']:.3e}, ratio {local / case['local_bound']:.3f}")
    assert err <= case["bound"] and local <= case["local_bound"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_argument_errors_and_workspace_query(dtype):
    case = SF.make_case(2, 3, 5, 2, np.dtype(NP[dtype]).name)
    held = [tt(case[k], dtype) for k in ("mu0", "cp0", "a", "b", "cq", "eps")]
    out = torch.empty((3, 2, 5, 2), dtype=dtype, device=DEV)
    ptrs = [_lib.ptr(x) for x in held]

    def rc(bsz=2, s=3, t=5, d=2, eps=ptrs[5], chunks=1):
        return _lib.call_rc("mf_ssm_sample", dtype, bsz, s, t, d, *ptrs[:5], eps, _lib.ptr(out), None, 0, chunks, stream())

    assert (rc(bsz=-1), rc(s=-1), rc(t=0), rc(d=0), rc(d=10), rc(eps=None), rc(chunks=-1)) == (-1, -2, -3, -4, -100, -10, -14)
    assert rc(bsz=0, eps=None) == 0 and rc(s=0, eps=None) == 0 and rc(chunks=3) == 0      # no workspace: the sweep, not an error
    query = _lib.load().mf_ssm_sample_workspace_bytes
    size = out.element_size()
    assert query(2, 5, 50, 6, size, 1) == 0
    assert query(2, 5, 50, 6, size, 3) == 2 * (36 * 2 + 2 * 6 * 10) * size         # Phi per (series, chunk), v and x_in per (trajectory, chunk)
