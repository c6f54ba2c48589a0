"""
``StateSpaceModel.log_pdf`` on the fused kernels (csrc/mf_logpdf.hip): one ``mf_ssm_log_pdf`` call, one ``mf_ssm_log_pdf_grad`` call in
``backward()`` that computes only what the tape wants, the composition beyond d = 9 and on the CPU, the density ratio moved with it.  Chains
and bounds are tests/helpers/log_pdf_closed_forms.py's: two float64 evaluations, each within the bound of the reference, differ by at most twice it.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from helpers import log_pdf_closed_forms as LF
from test_gpu_kalman import DEV, nn, tt

pytestmark = pytest.mark.gpu
F64 = torch.float64
KEYS = ("mu0", "cp0", "a", "b", "cq")


@pytest.fixture
def calls(monkeypatch):
    seen, real = type("Calls", (list,), {})(), _lib.call_rc                       # the entry points in call order, and each one's last arguments
    seen.args = {}

    def spy(base, *args):
        seen.append(base)
        seen.args[base] = args
        return real(base, *args)

    monkeypatch.setattr(_lib, "call_rc", spy)
    return seen


def close(got, want, case, name):
    tol = 2 * case["bound"][name] * case["mag"][name].astype(np.float64).reshape(want.shape)
    return bool(np.all(np.abs(nn(got) - nn(want)) <= tol))


@pytest.mark.parametrize("lead", [(2, 2), ()])
def test_value_in_one_call_and_every_gradient_in_one_more(calls, lead):
    s = int(np.prod(lead))
    case = LF.make_case(3, s, 12, 3, "float64")
    leaves = [tt(case[k]).requires_grad_(True) for k in KEYS]
    x = tt(case["x"]).reshape(lead + (3, 12, 3)).requires_grad_(True)
    ssm = mfa.StateSpaceModel(*leaves)
    got = ssm.log_pdf(x)
    assert calls.count("mf_ssm_log_pdf") == 1 and tuple(got.shape) == lead + (3,)
    want = ssm._log_pdf_composed(x)
    assert calls.count("mf_ssm_log_pdf") == 1 and close(got, want, case, "out")
    g = tt(case["g"]).reshape(lead + (3,))
    want_grads = torch.autograd.grad(want, [x] + leaves, g)
    assert "mf_ssm_log_pdf_grad" not in calls
    got_grads = torch.autograd.grad(got, [x] + leaves, g)
    assert calls.count("mf_ssm_log_pdf_grad") == 1
    for name, a, b in zip(LF.OUTPUTS[1:], got_grads, want_grads):
        assert a.shape == b.shape and close(a, torch.tril(b) if name in ("g_cp0", "g_cq") else b, case, name), name
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(ssm.log_pdf(x).sum(), x, create_graph=True)


def test_only_the_states_under_the_tape_computes_no_parameter_adjoint(calls):
    case = LF.make_case(3, 4, 12, 3, "float64")
    x = tt(case["x"]).requires_grad_(True)
    mfa.StateSpaceModel(*[tt(case[k]) for k in KEYS]).log_pdf(x).backward(tt(case["g"]))
    args = calls.args["mf_ssm_log_pdf_grad"]                                       # (dtype, B, S, T, d, chain x 5, states, g, g_states, ...)
    assert calls.count("mf_ssm_log_pdf_grad") == 1 and args[12] is not None and all(a is None for a in args[13:18])
    assert close(x.grad, tt(case["ref"]["g_x"].astype(np.float64)), case, "g_x")


def test_state_dimension_ten_and_a_cpu_chain_take_the_composition(calls):
    kern = mfa.Sum([mfa.Matern52(0.9, 1.3), mfa.Matern52(0.5, 0.7), mfa.Matern52(1.4, 0.4), mfa.Matern12(0.5, 0.4)], jitter=1e-9)
    ssm = kern.state_space_model(torch.linspace(0.0, 2.0, 12, dtype=F64, device=DEV)[None])
    assert ssm.state_dim == 10 and bool(torch.isfinite(ssm.log_pdf(ssm.sample((5,)))).all())
    case = LF.make_case(3, 4, 12, 3, "float64")
    cpu = mfa.StateSpaceModel(*[torch.tensor(case[k]) for k in KEYS]).log_pdf(torch.tensor(case["x"]))
    assert not cpu.is_cuda and not any(name.startswith("mf_ssm_log_pdf") for name in calls)
    fused = mfa.StateSpaceModel(*[tt(case[k]) for k in KEYS]).log_pdf(tt(case["x"]))
    assert calls.count("mf_ssm_log_pdf") == 1 and close(fused, cpu, case, "out")


def test_the_density_ratio_makes_two_forward_calls(calls):
    z = tt([[0.0, 0.4, 1.1, 1.5, 2.3, 3.0], [0.2, 0.5, 0.9, 1.8, 2.2, 2.9]])
    model = mfa.ImportanceWeightedVI(mfa.Matern32(0.9, 1.3, device=DEV), z, mfa.Bernoulli(), 3)
    with torch.no_grad():
        u = model.dist_q.sample((3,))
    ratio = model.posterior._log_density_ratio(u.requires_grad_(True))
    assert calls.count("mf_ssm_log_pdf") == 2 and tuple(ratio.shape) == (3, 2)
    ratio.sum().backward()
    assert calls.count("mf_ssm_log_pdf_grad") == 2 and bool(torch.isfinite(u.grad).all())
