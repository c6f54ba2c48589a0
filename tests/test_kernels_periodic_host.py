"""
CPU tests of the periodic and quasi-periodic kernels (markovflow_amd/kernels.py: Constant, HarmonicOscillator, Product,
SDEKernel.__mul__): construction, shapes and the differentiable torch restatement of the generator's closed forms
(`_torch_transitions`, the route of CPU tensors under a gradient) against tests/helpers/periodic_closed_forms.py.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from helpers import periodic_closed_forms as PC

MATERN = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}
LS, VAR_M, VAR_O, PERIOD = 0.7, 1.3, 0.8, 1.7


def quasi_periodic(order, osc, **kw):
    """Matern * HarmonicOscillator in the list order that gives Kronecker order `osc`, and the helper's description of it."""
    parts = [MATERN[order](LS, VAR_M), mfa.HarmonicOscillator(VAR_O, PERIOD)]
    kern = mfa.Product(parts if osc == 1 else parts[::-1], **kw)
    return kern, {"order": order, "ls": LS, "var": VAR_M * VAR_O, "period": PERIOD, "osc": osc}


def test_constructor_validation():
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            mfa.Constant(bad)
        with pytest.raises(ValueError):
            mfa.HarmonicOscillator(bad, 1.0)
        with pytest.raises(ValueError):
            mfa.HarmonicOscillator(1.0, bad)
    with pytest.raises(ValueError):
        mfa.HarmonicOscillator(torch.tensor([1.0, 2.0]), torch.tensor([1.0, -2.0]))
    with pytest.raises(AssertionError):
        mfa.Constant(1.0, output_dim=0)
    with pytest.raises(AssertionError):
        mfa.HarmonicOscillator(1.0, 1.0, jitter=-1.0)
    with pytest.raises(AssertionError):
        mfa.Product([])
    with pytest.raises(AssertionError):                       # the output-dimension assertion of the reference's Product
        mfa.Product([mfa.Matern32(1.0, 1.0, output_dim=2), mfa.HarmonicOscillator(1.0, 1.0)])
    with pytest.raises(TypeError):
        mfa.Product([mfa.Matern32(1.0, 1.0), 3.0])
    k = mfa.HarmonicOscillator(2.0, 0.5)
    assert float(k.variance) == 2.0 and float(k.period) == 0.5 and float(mfa.Constant(3.0).variance) == 3.0


def test_state_dim_and_steady_state_covariance():
    c, h = mfa.Constant(1.5), mfa.HarmonicOscillator(VAR_O, PERIOD)
    assert c.state_dim == 1 and h.state_dim == 2
    np.testing.assert_array_equal(c.steady_state_covariance.numpy(), [[1.5]])
    np.testing.assert_array_equal(h.steady_state_covariance.numpy(), VAR_O * np.eye(2))
    np.testing.assert_array_equal(c.feedback_matrix.numpy(), [[0.0]])
    om = 2 * np.pi / PERIOD
    np.testing.assert_allclose(h.feedback_matrix.numpy(), [[0.0, -om], [om, 0.0]], rtol=1e-15)
    for order in (1, 3, 5):
        for osc in (1, 2):
            kern, comp = quasi_periodic(order, osc)
            assert kern.state_dim == PC.size(comp) == (order + 1)
            _, _, p = PC.component_transitions(comp, np.array([0.1]))
            np.testing.assert_allclose(kern.steady_state_covariance.numpy(), p, rtol=1e-14)
            np.testing.assert_allclose(float(kern.variance), VAR_M * VAR_O, rtol=1e-15)
    # the two Kronecker orders differ beyond one Matern state
    assert not np.array_equal(quasi_periodic(3, 1)[0].steady_state_covariance.numpy(),
                              quasi_periodic(3, 2)[0].steady_state_covariance.numpy())
    # per-series hyper-parameters carry their batch shape
    hb = mfa.HarmonicOscillator(torch.tensor([1.0, 2.0, 3.0]), torch.tensor([0.5, 0.6, 0.7]))
    kb = mfa.Matern52(0.9, 1.1) * hb
    assert tuple(hb.steady_state_covariance.shape) == (3, 2, 2) and tuple(kb.steady_state_covariance.shape) == (3, 6, 6)
    assert tuple(kb.feedback_matrix.shape) == (3, 6, 6)


def test_mul_and_constant_factors():
    m, h, c = mfa.Matern32(LS, VAR_M), mfa.HarmonicOscillator(VAR_O, PERIOD), mfa.Constant(2.5)
    k = m * h
    assert isinstance(k, mfa.Product) and k.kernels == [m, h] and k.state_dim == 4 and k._osc == 1
    assert (h * m)._osc == 2
    with pytest.raises(AssertionError):
        mfa.Matern32(1.0, 1.0, output_dim=2) * h
    scaled = mfa.Product([c, m, h, mfa.Constant(2.0)])
    assert scaled.state_dim == 4 and float(scaled.variance) == pytest.approx(2.5 * VAR_M * VAR_O * 2.0, rel=1e-15)
    dts = torch.tensor([[0.1, 0.4]], dtype=torch.float64)
    a0, _, q0 = k._torch_transitions(dts, False, True)
    a1, _, q1 = scaled._torch_transitions(dts, False, True)
    np.testing.assert_allclose(a1.numpy(), a0.numpy(), rtol=1e-15)
    np.testing.assert_allclose(q1.numpy(), 5.0 * q0.numpy(), rtol=1e-13, atol=1e-16)
    # a Constant factor on a Matern alone: a plain Matern component with a scaled variance
    cm = c * m
    assert cm.state_dim == 2 and cm._osc == 0 and cm.order == 3
    np.testing.assert_allclose(cm._torch_transitions(dts, False, True)[2].numpy(),
                               2.5 * m._torch_transitions(dts, False, True)[2].numpy(), rtol=1e-13)


@pytest.mark.parametrize("make", [
    lambda: mfa.Matern32(1.0, 1.0) * mfa.Matern12(1.0, 1.0),
    lambda: mfa.Product([mfa.Matern52(1.0, 1.0), mfa.HarmonicOscillator(1.0, 1.0), mfa.Matern52(1.0, 1.0)]),
    lambda: mfa.HarmonicOscillator(1.0, 1.0) * mfa.HarmonicOscillator(1.0, 2.0),
    lambda: mfa.Product([mfa.Sum([mfa.Matern12(1.0, 1.0), mfa.Matern32(1.0, 1.0)]), mfa.HarmonicOscillator(1.0, 1.0)]),
    lambda: mfa.Product([mfa.Matern12(1.0, 1.0) * mfa.HarmonicOscillator(1.0, 1.0), mfa.Constant(1.0)]),
    lambda: mfa.Product([mfa.IndependentMultiOutput([mfa.Matern12(1.0, 1.0)]), mfa.Constant(1.0)]),
], ids=["matern-matern", "two-materns-and-oscillator", "two-oscillators", "sum-child", "product-child", "multi-output-child"])
def test_unsupported_products_raise(make):
    with pytest.raises(NotImplementedError, match="at most one"):
        make()


def test_sum_over_mixed_components():
    qp, _ = quasi_periodic(5, 1)
    kern = mfa.Constant(0.4) + qp + mfa.Matern32(0.9, 0.6)          # Sum(Sum(Constant, Product), Matern32)
    assert isinstance(kern, mfa.Sum) and kern.state_dim == 9
    comps = kern._components()
    assert [(c.order, c._osc) for c in comps] == [(0, 0), (5, 1), (3, 0)]
    t = torch.linspace(0.0, 1.0, 5, dtype=torch.float64).expand(2, 5)
    h = kern.generate_emission_model(t).emission_matrix
    want = np.zeros(9)
    want[[0, 1, 7]] = 1.0
    assert tuple(h.shape) == (2, 5, 1, 9)
    np.testing.assert_array_equal(h.numpy(), np.broadcast_to(want, (2, 5, 1, 9)))
    for osc in (1, 2):
        prod = quasi_periodic(3, osc)[0]
        he = prod.generate_emission_model(t).emission_matrix.numpy()
        np.testing.assert_array_equal(he, np.broadcast_to([1.0, 0.0, 0.0, 0.0], (2, 5, 1, 4)))
    assert kern.jitter_matrix.shape == (9, 9) and tuple(kern.initial_mean((2,)).shape) == (2, 9)
    np.testing.assert_allclose(kern.steady_state_covariance.numpy()[1:7, 1:7], qp.steady_state_covariance.numpy(), rtol=0)
    multi = mfa.IndependentMultiOutput([mfa.HarmonicOscillator(1.0, 2.0), qp])
    assert multi.state_dim == 8 and multi.output_dim == 2
    assert tuple(multi.generate_emission_model(t).emission_matrix.shape) == (2, 5, 2, 8)


def test_torch_transitions_vs_closed_forms(rng):
    dt = 0.05 + rng.exponential(0.2, size=(3, 12))
    dts = torch.tensor(dt)
    jit = 1e-6
    cases = [(mfa.Constant(1.5, jitter=jit), [{"order": 0, "var": 1.5, "osc": 0}]),
             (mfa.HarmonicOscillator(VAR_O, PERIOD, jitter=jit), [{"order": 0, "var": VAR_O, "period": PERIOD, "osc": 1}])]
    for order in (1, 3, 5):
        for osc in (1, 2):
            kern, comp = quasi_periodic(order, osc, jitter=jit)
            cases.append((kern, [comp]))
    qp, comp = quasi_periodic(5, 2)
    cases.append((mfa.Sum([mfa.Constant(0.4), qp, mfa.Matern32(0.9, 0.6)], jitter=jit),
                  [{"order": 0, "var": 0.4, "osc": 0}, comp, {"order": 3, "ls": 0.9, "var": 0.6, "osc": 0}]))
    for kern, comps in cases:
        a_ref, q_ref, p_ref = PC.concat_transitions(comps, dt, jitter=jit)
        a_s, chol, q_s = kern._torch_transitions(dts, True, True)
        np.testing.assert_allclose(a_s.numpy(), a_ref, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(q_s.numpy(), q_ref, rtol=1e-10, atol=1e-13)
        cc = chol.numpy()
        np.testing.assert_allclose(cc @ np.swapaxes(cc, -1, -2), q_ref, rtol=1e-10, atol=1e-13)
        assert np.all(np.triu(cc, 1) == 0)
        np.testing.assert_allclose(kern.steady_state_covariance.numpy(), p_ref, rtol=1e-14)
    # order 0 with a zero jitter: Q is exactly zero and the zero factor passes through
    a_s, chol, q_s = (mfa.HarmonicOscillator(VAR_O, PERIOD) + mfa.Matern12(1.0, 1.0))._torch_transitions(dts, True, True)
    assert torch.all(q_s[..., :2, :2] == 0) and torch.all(chol[..., :2, :] == 0) and torch.all(chol[..., 2, 2] > 0)
    # per-series hyper-parameters
    per, var = np.array([0.9, 1.7, 2.6]), np.array([0.5, 1.0, 1.5])
    kern = mfa.Matern52(LS, VAR_M) * mfa.HarmonicOscillator(torch.tensor(var), torch.tensor(per))
    a_s, _, q_s = kern._torch_transitions(dts, False, True)
    for s in range(3):
        comp = {"order": 5, "ls": LS, "var": VAR_M * var[s], "period": per[s], "osc": 1}
        a_ref, q_ref, _ = PC.component_transitions(comp, dt[s])
        np.testing.assert_allclose(a_s[s].numpy(), a_ref, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(q_s[s].numpy(), q_ref, rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("osc", [1, 2])
def test_feedback_matrix_is_the_kronecker_sum(rng, osc):
    """A_k = exp(F dt_k) holds for the Kronecker SUM of the children's feedback matrices (the reference's Kronecker product
    does not satisfy it)."""
    kern, _ = quasi_periodic(3, osc)
    dts = torch.tensor(0.05 + rng.exponential(0.2, size=(7,)))
    a_s = kern._torch_transitions(dts, False, False)[0]
    expm = torch.linalg.matrix_exp(kern.feedback_matrix * dts[:, None, None])
    np.testing.assert_allclose(expm.numpy(), a_s.numpy(), rtol=1e-10, atol=1e-14)
    f1, f2 = [k.feedback_matrix for k in kern.kernels]
    reference_form = torch.kron(f1, f2)
    assert not np.allclose(torch.linalg.matrix_exp(reference_form * dts[0]).numpy(), a_s[0].numpy(), rtol=1e-3)


def test_torch_transitions_gradcheck():
    # (gaps at which chol Q is well conditioned: at 0.05 the central differences of gradcheck itself are rounding noise of 1e-5)
    dts = torch.tensor([[0.3, 0.55, 0.9]], dtype=torch.float64)
    w = torch.linspace(-1.0, 1.0, 3 * 36, dtype=torch.float64).reshape(1, 3, 6, 6)

    def fn(ls, var_m, var_o, period):
        kern = mfa.Matern52(ls, var_m, jitter=1e-8) * mfa.HarmonicOscillator(var_o, period)
        a_s, chol, q_s = mfa.Sum([kern], jitter=1e-8)._torch_transitions(dts, True, True)
        return a_s, chol, q_s

    leaves = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (LS, VAR_M, VAR_O, PERIOD)]
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6, rtol=1e-5)
    # and through the route a user takes: CPU tensors under a gradient go to the torch ops, not to the device
    kern = mfa.Matern52(leaves[0], leaves[1]) * mfa.HarmonicOscillator(leaves[2], leaves[3])
    a_s, q_s = kern.transition_statistics(None, dts)
    (torch.sum(w * a_s) + torch.sum(w * q_s)).backward()
    assert all(x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs()) > 0 for x in leaves)


def test_generator_argument_errors_without_touching_the_gpu():
    """mf_sde_transitions_*: invalid arguments are refused before any launch, by the negative position of the argument; -100
    when the staging image of 64 d x d blocks exceeds the LDS limit (d = 18 in fp64)."""
    import ctypes
    from markovflow_amd import _lib
    lib = _lib.load()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)                                            # noqa: E731
    some = ctypes.c_void_p(8)                                                                # (never dereferenced)
    for fn in (lib.mf_sde_transitions_f64, lib.mf_sde_transitions_grad_f64, lib.mf_sde_transitions_f32):
        call = lambda b, n, nc, o, r, lam=None: fn(b, n, nc, o, r, lam, None, None, 0, None, 0.0, None, None, None, None)   # noqa: E731
        assert call(-1, 4, 1, ints(0), ints(0)) == -1
        assert call(1, -4, 1, ints(0), ints(0)) == -2
        assert call(1, 4, 0, ints(0), ints(0)) == -3 and call(1, 4, 17, ints(*[1] * 17), ints(*[0] * 17)) == -3
        assert call(1, 4, 2, ints(0, 2), ints(1, 2)) == -4 and call(1, 4, 1, None, ints(0)) == -4
        assert call(1, 4, 2, ints(0, 5), ints(3, 0)) == -5 and call(1, 4, 1, ints(0), None) == -5
        assert call(1, 4, 2, ints(0, 5), ints(1, 2)) == -6
        assert call(1, 4, 2, ints(0, 5), ints(1, 2), some) == -7
        assert call(0, 4, 2, ints(0, 5), ints(1, 2)) == 0 and call(1, 0, 2, ints(0, 5), ints(1, 2)) == 0
    assert lib.mf_sde_transitions_f64(1, 4, 3, ints(5, 5, 5), ints(1, 1, 1), some, some, None, 0, some, 0.0, some, None, None, None) == -8
    assert lib.mf_sde_transitions_f64(1, 4, 3, ints(5, 5, 5), ints(1, 1, 1), some, some, some, 0, some, 0.0, some, None, None, None) == -100
