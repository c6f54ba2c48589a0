"""
GPU tests of ``mf_ssm_kl_from_moments_{f64,f32}`` (csrc/mf_wave.hpp: wave_ssm_kl_terms_kernel + row_sums_kernel): KL(q1 || q2) at
16 <= d <= 32 from q1's moments, one wavefront per (series, block).  ``StateSpaceModel.kl_divergence`` takes the one-walk kernel at
these state dimensions, so the entry point is reached through the raw ABI (its own inputs: moments by the explicit float64
recursion in numpy, not by the package) and through ``_kl_divergence_operators``.  Exact and padded tile counts (d = 16, 32 /
17, 24, 31), one block (every tensor over the transitions NULL), the ``has_next`` edge of the last block, more series than one
round of wavefronts.  float64 against the numpy oracle at the tolerance tests/test_gpu_wave.py applies to the same quantity;
float32 against the operator form in float64 on the inputs the kernel saw, within FP32_FACTOR x the float32 evaluation of the same
form (tests/helpers/kl_fp32_cases.py).
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from oracle import numpy_oracle as O
from helpers import kl_closed_forms as KC
from helpers import kl_fp32_cases as C
from helpers import kl_fp32_table as TABLE
from helpers.kl_fp32_cases import abi_calls  # noqa: F401  (fixture)
from test_gpu_kalman import DEV, nn, tt

pytestmark = pytest.mark.gpu
CASES = [(d, bsz, t) for d in C.FROM_MOMENTS_DIMS for bsz, t in C.FROM_MOMENTS_SHAPES]


def from_moments(dtype, kw1, kw2, covs_1, cross_1, mean_diff):
    """The raw entry point on the given arrays; ``out`` and the workspace are NaN beforehand and every out[s] must be finite."""
    bsz, t, d = mean_diff.shape
    g = lambda x: tt(x, dtype)                                # noqa: E731
    over_time = [None] * 4 if t == 1 else [g(kw1["chol_q"]), g(kw2["a_s"]), g(kw2["chol_q"]), g(cross_1)]
    args = [g(kw1["chol_p0"]), over_time[0], g(kw2["chol_p0"]), over_time[1], over_time[2], g(covs_1), over_time[3], g(mean_diff)]
    out = torch.full((bsz,), float("nan"), dtype=dtype, device=DEV)
    ws = torch.full((bsz * t,), float("nan"), dtype=dtype, device=DEV)
    ws_bytes = int(_lib.load().mf_ssm_kl_from_moments_workspace_bytes(bsz, t, d, out.element_size()))
    assert ws_bytes == ws.numel() * ws.element_size()
    _lib.call("mf_ssm_kl_from_moments", dtype, bsz, t, d, *[_lib.ptr(a) for a in args], _lib.ptr(out), _lib.ptr(ws), ws_bytes,
              _lib.stream_ptr(out.device))
    res = nn(out)
    assert np.isfinite(res).all()
    return res


def with_junk(kw1, kw2):
    """What the entry point promises not to read, as NaN: everything but the diagonals of q1's factors, the strict upper triangles
    of q2's."""
    d = kw1["chol_p0"].shape[-1]
    off = ~np.eye(d, dtype=bool)
    upper = np.triu(np.ones((d, d), dtype=bool), 1)
    j1, j2 = {k: v.copy() for k, v in kw1.items()}, {k: v.copy() for k, v in kw2.items()}
    for key in ("chol_p0", "chol_q"):
        j1[key][..., off] = np.nan
        j2[key][..., upper] = np.nan
    return j1, j2


@pytest.mark.parametrize("d,bsz,t", CASES)
def test_from_moments_fp64_against_the_oracle(abi_calls, d, bsz, t):
    kw1, kw2, covs_1, cross_1, mean_diff = C.draw_from_moments(C.DEFAULT_SEED, d, bsz, t, False)
    want = O.ssm_kl_divergence(tuple(kw1[k] for k in KC.CHAIN), tuple(kw2[k] for k in KC.CHAIN))
    got = from_moments(torch.float64, kw1, kw2, covs_1, cross_1, mean_diff)
    np.testing.assert_allclose(got, want, rtol=1e-8)
    # the contract of the header: the result does not change (not in one bit) with NaN where nothing is read
    j1, j2 = with_junk(kw1, kw2)
    assert np.array_equal(from_moments(torch.float64, j1, j2, covs_1, cross_1, mean_diff), got)
    if t == 1:
        return        # (StateSpaceModel, like the reference's, needs a transition: one block is reached through the raw ABI only)
    # the same chains through the method that composes the moments with the entry point
    q1 = mfa.StateSpaceModel(*(tt(kw1[k]) for k in KC.CHAIN))
    q2 = mfa.StateSpaceModel(*(tt(kw2[k]) for k in KC.CHAIN))
    del abi_calls[:]
    np.testing.assert_allclose(nn(q1._kl_divergence_operators(q2)), want, rtol=1e-8)
    ran = C.ran(abi_calls, torch.float64)
    assert "mf_ssm_kl_from_moments" in ran and "mf_ssm_kl_divergence" not in ran


@pytest.mark.parametrize("d,bsz,t", CASES)
def test_from_moments_fp32_within_the_yardstick(d, bsz, t):
    args = C.draw_from_moments(C.DEFAULT_SEED, d, bsz, t, True)
    want = C.from_moments_closed_form(*args, torch.float64)
    got = from_moments(torch.float32, *args)
    err, yard = KC.value_error(got, want, t, d), TABLE.FROM_MOMENTS[(d, bsz, t)]
    print(f"  fp32 from_moments d={d} B={bsz} T={t}: error {err:.3g} (closed form in float32 {yard:.3g}, ratio {err / yard:.2f})")
    assert err <= C.FP32_FACTOR * yard
    j1, j2 = with_junk(args[0], args[1])
    assert np.array_equal(from_moments(torch.float32, j1, j2, *args[2:]), got)
