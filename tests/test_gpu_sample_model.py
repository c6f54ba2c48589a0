"""
``StateSpaceModel.sample`` on the fused sampler (csrc/mf_sample.hip): one ``mf_ssm_sample`` call outside the tape, the composed route under it
and beyond d = 9, the same trajectories under one seed on both, and the posterior's Matheron draws (two ``sample`` calls) moved with it.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from helpers import sample_closed_forms as SF
from test_gpu_kalman import DEV, nn, random_ssm, tt

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAMES = ("mu0", "chol_p0", "a_s", "b_s", "chol_q")


@pytest.fixture
def calls(monkeypatch):
    seen, real = [], _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *args: (seen.append(base), real(base, *args))[1])
    return seen


@pytest.mark.parametrize("s,batch,t,d", [(4, (2,), 20, 3), (3, (), 7, 1)])
def test_sample_is_the_recursion_in_one_call(rng, calls, s, batch, t, d):
    kw = random_ssm(rng, batch, t, d, 1, well=True)
    ssm = mfa.StateSpaceModel(*[tt(kw[k]) for k in NAMES])
    full = (s,) + batch + (t, d)
    torch.manual_seed(5)
    got = ssm.sample((s,))
    torch.manual_seed(5)
    eps = nn(torch.randn(full + (1,), dtype=F64, device=DEV))[..., 0]
    assert calls.count("mf_ssm_sample") == 1 and "mf_ssm_marginal_means" not in calls
    flat = [kw[k].reshape((-1,) + kw[k].shape[len(batch):]) for k in NAMES]
    want = SF.recursion(*flat, eps.reshape(s, -1, t, d), np.float64).reshape(full)
    np.testing.assert_allclose(nn(got), want, rtol=0, atol=1e-12 * float(np.abs(want).max()))


def test_taped_chain_keeps_the_composed_route(rng, calls):
    kw = random_ssm(rng, (2,), 20, 3, 1, well=True)
    torch.manual_seed(7)
    taped = mfa.StateSpaceModel(*[tt(kw[k]).requires_grad_(True) for k in NAMES]).sample(4)
    assert taped.requires_grad and "mf_ssm_sample" not in calls
    torch.manual_seed(7)
    plain = mfa.StateSpaceModel(*[tt(kw[k]) for k in NAMES]).sample(4)
    assert calls.count("mf_ssm_sample") == 1
    assert float((taped.detach() - plain).abs().max()) <= 1e-10


def test_posterior_trajectories_reach_the_kernel_twice(calls, monkeypatch):
    t_train, y = tt([[0.0, 0.4, 1.1, 1.5, 2.3, 3.0]]), tt([[[0.3], [-0.2], [0.8], [1.1], [0.1], [-0.5]]])
    gpr = mfa.GaussianProcessRegression((t_train, y), mfa.Matern52(0.9, 1.3), chol_obs_covariance=0.3 * torch.eye(1, dtype=F64, device=DEV))
    t_new, post = tt([[-0.7, 0.2, 0.9, 1.3, 2.0, 2.9, 3.8]]), gpr.posterior
    torch.manual_seed(9)
    new_s, cond_s = post.sample_state_trajectories(t_new, 3)
    assert tuple(new_s.shape) == (3, 1, 7, 3) and calls.count("mf_ssm_sample") == 2

    def composed(self, sample_shape):
        shape = (sample_shape,) if isinstance(sample_shape, int) else tuple(sample_shape)
        full = shape + tuple(self.batch_shape) + self.event_shape
        return self._sample_composed(torch.randn(full + (1,), dtype=F64, device=DEV))

    monkeypatch.setattr(mfa.StateSpaceModel, "sample", composed)
    torch.manual_seed(9)
    new_c, cond_c = post.sample_state_trajectories(t_new, 3)
    assert calls.count("mf_ssm_sample") == 2
    assert float((new_s - new_c).abs().max()) <= 1e-10 and float((cond_s - cond_c).abs().max()) <= 1e-10


def test_state_dimension_ten_takes_the_composed_route(calls):
    kern = mfa.Sum([mfa.Matern52(0.9, 1.3), mfa.Matern52(0.5, 0.7), mfa.Matern52(1.4, 0.4), mfa.Matern12(0.5, 0.4)], jitter=1e-9)
    assert kern.state_dim == 10
    times = torch.linspace(0.0, 2.0, 12, dtype=F64, device=DEV)[None]
    draw = kern.state_space_model(times).sample((5,))
    assert tuple(draw.shape) == (5, 1, 12, 10) and bool(torch.isfinite(draw).all())
    assert "mf_ssm_sample" not in calls and "mf_ssm_marginal_means" in calls
