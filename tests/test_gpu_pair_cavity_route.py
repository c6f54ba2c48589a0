"""GPU tests of the route to ``mf_pair_cavity_*``: ``models.pair_cavity`` sends HIP tensors with an even ``2d <= 18`` to ``pair_cavity_hip``
and everything else to ``pair_cavity_torch``, and ``SparsePowerExpectationPropagation`` reaches the kernel through it.  The tolerance is
that of tests/test_gpu_pair_cavity_kernel.py, with the torch route evaluated on the device."""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import models as MM
from helpers import pair_cavity_exact as X

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def tensors(case, lead):
    return [torch.tensor(case[k], dtype=torch.float64, device=DEV).reshape(lead + case[k].shape[2:]) for k in X.KEYS]


def test_small_pairs_on_hip_take_the_kernel_whatever_the_batch_shape_and_large_ones_the_torch_composition():
    case = X.draw(1, 6, 4)
    args = tensors(case, (2, 3))
    got, hip, composed = MM.pair_cavity(*args), MM.pair_cavity_hip(*args), MM.pair_cavity_torch(*args)
    assert [tuple(t.shape) for t in got] == [(2, 3, 4), (2, 3, 4, 4), (2, 3)]
    assert all(torch.equal(a, b) for a, b in zip(got, hip)), "pair_cavity is pair_cavity_hip, bit for bit"
    want = X.exact(case)
    flat = lambda out: {k: t.reshape(want[k].shape).cpu().numpy() for k, t in zip(X.OUTPUTS, out)}      # noqa: E731
    failures = X.within_four("route (2, 3), n = 4", flat(got), flat(composed), want)
    assert not failures, "; ".join(failures)
    args = tensors(X.draw(1, 6, 20), (2, 3))                  # a pair of twenty takes the torch composition
    assert all(torch.equal(a, b) for a, b in zip(MM.pair_cavity(*args), MM.pair_cavity_torch(*args)))


def test_the_sparse_power_ep_model_reaches_the_kernel():
    rng = np.random.default_rng(2)
    x = torch.tensor(np.sort(rng.uniform(0.0, 10.0, size=(1, 33))), dtype=torch.float64, device=DEV)
    y = torch.tensor(rng.integers(0, 2, size=(1, 33, 1)), dtype=torch.float64, device=DEV)
    z = torch.linspace(1.0, 9.0, 5, dtype=torch.float64, device=DEV)[None]
    model = mfa.SparsePowerExpectationPropagation(mfa.Matern32(1.5, 1.0, device=DEV), z, mfa.Bernoulli(), learning_rate=0.5, alpha=0.5)
    for _ in range(2):                      # sites away from zero
        model.update_sites((x, y))
    got = model.compute_cavity_state_pairs(x)
    with torch.no_grad():
        want = MM.pair_cavity_hip(*model._pair_marginals(model.dist_q), model.nat1, model.nat2, model.alpha * model.fraction_sites(x))
    assert bool(torch.isfinite(got[1]).all()) and float(model.nat2.abs().max()) > 0.0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
