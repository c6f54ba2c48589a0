"""
float32 of the local step of ``KalmanFilter.log_likelihood().backward()`` at d <= 15: ``mf_kf_loglik_grad_f32`` - kf_grad_kernel
(one lane per series and time point, d <= 6), row::row_kf_grad_kernel (d = 7..15, one to four outputs) and the tile route for more
than four outputs - the float32 instantiations of what tests/test_gpu_gradients.py pins in float64.  Through the raw entry point on
float32-rounded EXACT smoothed moments (dense Gaussian conditioning on the CPU), with the emission model: g_H, g_y, g_omega, shared
and per-step precisions, per-series weights and weights = NULL, T = 1, into buffers full of NaN; and through the public API on the
three-kernel route, where the gradients must be the closed forms of the float32 moments the GPU's own smoother produced.

Judged as tests/helpers/loglik_fp32_cases.py states: against the local forms of Fisher's identity in float64
(tests/helpers/loglik_grad_closed_forms.py, pinned on the CPU by tests/test_loglik_grad_closed_forms_host.py) on the inputs the kernel
saw, within FP32_FACTOR x the error of the same forms evaluated in float32 on the CPU (tests/helpers/loglik_fp32_table.py: LOCAL).

That the assertions can fail (CPU, the float32 evaluation standing in for the kernel with ONE defect, draw DEFAULT_SEED, measured
error / yardstick per tensor; the bar is FP32_FACTOR = 4):
    local, (6, 3, 9, 2) shared R:   no defect                           every tensor <= 1.0
                                    Psi without the  - X A^T  term      cholQ 1.6e+06, the others unchanged
                                    Omega unweighted                    Omega 1.1e+06
    local, (9, 3, 13, 5) per step:  no defect                           every tensor <= 0.76
                                    Psi without the  - X A^T  term      cholQ 1.8e+06
                                    Omega unweighted                    Omega 5.3e+05
    streamed (tests/test_gpu_grad_streamed.py), (6, 3, 70, 2) on 5 chunks, L = 14: mf_grad_host_sim_f32 as it is <= 0.88;
    the last transition of every chunk but the last skipped (its gradients stay at a zeroed buffer's 0):
    A 4.1e+05, b 6.2e+05, cholQ 4.6e+05.  A term worth 1e-3 of a gradient, which the 5e-3 these yardsticks replace let
    through, is 500 x a yardstick of 2e-6.
The defective code is not kept.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib, kalman_filter as kfm
from helpers import loglik_fp32_cases as C
from helpers import loglik_fp32_table as TABLE
from helpers import loglik_grad_closed_forms as LC
from helpers.kl_fp32_cases import abi_calls  # noqa: F401  (fixture)
from test_gpu_kalman import DEV, tt

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64

LOCAL_PARAMS = ([s + (per_step, False) for s in C.LOCAL_LANE_CASES + C.LOCAL_ROW_CASES for per_step in (False, True)]
                + [s + (False, True) for s in C.LOCAL_NULL_WEIGHT_CASES])


def local_step_abi(kw, r_inv, moments, weights, per_step):
    """Call mf_kf_loglik_grad_f32 directly, every output buffer pre-filled with NaN: ``(return code, info, the eight outputs)``."""
    ins = [tt(kw[k], F32) for k in C.KEYS] + [tt(r_inv, F32)]
    bsz, t, m, d = ins[5].shape
    mom = [tt(x, F32) for x in moments]
    outs = [torch.full_like(x, float("nan")) for x in ins[:7]] + [torch.full((bsz, t, m, m), float("nan"), dtype=F32, device=DEV)]
    info = _lib.new_info(torch.device(DEV))
    p = lambda x: None if x is None or x.numel() == 0 else _lib.ptr(x)      # noqa: E731  (T = 1: no transitions, NULL)
    rc = _lib.call_rc("mf_kf_loglik_grad", F32, bsz, t, d, m, *[p(x) for x in ins], int(per_step), *[p(x) for x in mom],
                      *[p(x) for x in outs], p(None if weights is None else tt(weights, F32)), p(info),
                      _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, int(info.item()), outs


def judge_local(what, d, m, t, bsz, per_step, null_weights):
    kw, r_inv, weights, moments, want, want_unit = C.local_reference(d, m, t, bsz, per_step)
    rc, info, got = local_step_abi(kw, r_inv, moments, None if null_weights else weights, per_step)
    assert rc == 0 and info == 0
    for name, g in zip(C.GRAD_NAMES, got):
        assert g.dtype == F32 and not bool(torch.isnan(g).any()), name
        if name in ("cholP0", "cholQ") and g.numel():
            assert float(torch.triu(g, diagonal=1).abs().max()) == 0.0, name
    errs = C.errors(C.GRAD_NAMES, got, want_unit if null_weights else want)
    assert set(errs) == set(C.GRAD_NAMES) - (set() if t > 1 else {"A", "b", "cholQ"})
    # (weights = NULL: the forms with w = 1 round once less than the weighted ones the yardstick was measured on)
    C.report(f"{what} d={d} m={m} T={t} B={bsz} per_step={per_step} weights={'NULL' if null_weights else 'given'}", errs,
             TABLE.LOCAL[(d, m, t, bsz, per_step)])


@pytest.mark.parametrize("d,m,t,bsz,per_step,null_weights", LOCAL_PARAMS)
def test_local_gradient_kernel_fp32(d, m, t, bsz, per_step, null_weights):
    judge_local("local step", d, m, t, bsz, per_step, null_weights)


@pytest.mark.parametrize("per_step", [False, True])
@pytest.mark.parametrize("d,m,t,bsz", C.LOCAL_TILE_CASES)
def test_local_gradient_tile_route_small_d_fp32(d, m, t, bsz, per_step):
    """More than four outputs at d <= 15 take the tile kernel (big_kf_grad_f32) whatever the state dimension."""
    judge_local("local step, tile route", d, m, t, bsz, per_step, False)


@pytest.mark.parametrize("d,m,t,bsz", C.API_CASES)
def test_log_likelihood_backward_fp32_three_kernel_route(abi_calls, d, m, t, bsz):
    """Posterior chain -> moments -> local step, through the autograd function on float32 leaves with the series weighted
    differently.  Composition check: with the float32 moments the GPU's own smoother produced, the gradients are the local forms
    (in float64) of those moments, within the local step's own float32 allowance.  The distance to dense autograd in float64 is
    printed, not asserted: it is the smoother's float32 error carried through the forms, which
    tests/test_gpu_posterior_streamed.py and tests/test_gpu_kl_float32.py judge piece by piece."""
    kw, r_inv_drawn, weights = C.draw(C.DEFAULT_SEED, d, m, t, bsz, False)
    # the factor of the case's own R: how far E[r] = y - H m cancels, and with it the float32 error of g_H and g_y, depends on the
    # noise level, so the yardstick of this shape holds for the precision it was measured with (0.4 I + 0.1 11^T: 3 - 5 x more)
    chol_r = tt(np.linalg.cholesky(np.linalg.inv(r_inv_drawn)), F32)
    leaves = [tt(kw[k], F32).requires_grad_(True) for k in C.KEYS]
    kf = mfa.KalmanFilter(mfa.StateSpaceModel(*leaves[:5]), mfa.EmissionModel(leaves[5]), leaves[6], chol_r)
    per_series = kf._per_series()[0]                    # what log_likelihood() sums (plus constants that carry no gradient here)
    del abi_calls[:]
    torch.sum(per_series * tt(weights, F32)).backward()
    assert ("mf_kf_loglik_grad", F32, 0) in abi_calls
    assert not any(name == "mf_kf_loglik_grad_streamed" and rc == 0 for name, _, rc in abi_calls)
    got = [x.grad for x in leaves]
    assert all(g.dtype == F32 for g in got)
    with torch.no_grad():
        r_inv = kf._r_inv.detach()
        raw = kfm._RawFilter(mfa.StateSpaceModel(*(x.detach() for x in leaves[:5])), mfa.EmissionModel(leaves[5].detach()),
                             leaves[6].detach(), r_inv)            # the filter the backward builds
        moments = [x.double().cpu().numpy() for x in raw.posterior_state_space_model()._moments(want_sub=True)]
    r_inv64 = r_inv.double().cpu().numpy()
    want = LC.local_gradients_numpy(kw, r_inv64, moments, weights, F64)
    for name, g in zip(C.GRAD_NAMES[:7], got):
        if name in ("cholP0", "cholQ"):
            assert float(torch.triu(g, diagonal=1).abs().max()) == 0.0, name
    dense = C.dense_autograd(kw, r_inv64, weights, False)
    for name, e in C.errors(C.GRAD_NAMES[:7], got, dense[:7]).items():
        print(f"  fp32 three-kernel route d={d} m={m} T={t} B={bsz} {name}: {e:.3g} from dense autograd in float64 (not asserted)")
    C.report(f"three-kernel route d={d} m={m} T={t} B={bsz}", C.errors(C.GRAD_NAMES[:7], got, want[:7]),
             TABLE.LOCAL[(d, m, t, bsz, False)])
