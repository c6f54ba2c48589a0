"""
Host tests of ``Gaussian(variance=tensor)`` and ``StudentT(scale=tensor)``: the constructor, the softplus parametrisation, which models
refuse them, and the CPU torch methods differentiated in the parameter against a central finite difference in float64.
"""
import pytest
import torch

import markovflow_amd as mfa

F64 = torch.float64
Z = torch.linspace(0.5, 5.5, 5, dtype=F64).expand(2, 5).contiguous()


def test_the_constructor_takes_a_float_or_a_tensor_and_the_softplus_round_trips():
    assert mfa.Gaussian(0.3).variance == 0.3 and mfa.Gaussian(0.3).trainable_variables == ()
    assert mfa.StudentT(scale=0.7).scale == 0.7 and mfa.StudentT(scale=0.7)._params()[:2] == (0.7, 3.0)
    for lik, name, start in ((mfa.Gaussian(variance=torch.tensor(0.3, dtype=F64)), "variance", 0.3),
                             (mfa.StudentT(scale=torch.tensor([0.3, 25.0], dtype=F64)), "scale", [0.3, 25.0])):
        (leaf,) = lik.trainable_variables
        assert leaf is getattr(lik, "unconstrained_" + name) and leaf.is_leaf and leaf.requires_grad and leaf.dtype == F64
        value = getattr(lik, name)
        assert value.requires_grad and torch.allclose(value.detach(), torch.tensor(start, dtype=F64), rtol=4 * 2.0 ** -52, atol=0.0)
    for bad in (torch.tensor(0.0), torch.tensor([1.0, -1.0]), torch.tensor(float("nan")), torch.tensor(1, dtype=torch.int64)):
        with pytest.raises((ValueError, TypeError)):
            mfa.Gaussian(variance=bad)


def test_only_the_single_output_svgp_takes_a_tensor_parameter():
    lik = lambda: mfa.Gaussian(variance=torch.tensor([0.5, 1.5], dtype=F64))          # noqa: E731
    k = lambda: mfa.Matern32(1.0, 1.0, dtype=F64)                                      # noqa: E731
    x, y = torch.rand(2, 7, dtype=F64).sort(-1).values * 6, torch.zeros(2, 7, 1, dtype=F64)
    refused = [lambda: mfa.SparseVariationalGaussianProcess(mfa.IndependentMultiOutput([k(), k()]), lik(), Z),
               lambda: mfa.SparseVariationalGaussianProcess(mfa.IndependentMultiOutputStack([k(), k()]), lik(), Z[:, None].expand(2, 2, 5)),
               lambda: mfa.SparseVariationalGaussianProcess(k(), mfa.Gaussian(variance=torch.ones(3, dtype=F64)), Z),
               lambda: mfa.SparseVariationalGaussianProcess(k(), mfa.Gaussian(variance=torch.tensor(1.0)), Z),
               lambda: mfa.SparseCVIGaussianProcess(k(), Z, lik()),
               lambda: mfa.SparsePowerExpectationPropagation(k(), Z, lik()),
               lambda: mfa.ImportanceWeightedVI(k(), Z, lik(), 4),
               lambda: mfa.CVIGaussianProcess((x, y), k(), lik()),
               lambda: mfa.PowerExpectationPropagation((x, y), k(), lik()),
               lambda: mfa.VariationalGaussianProcess((x, y), k(), lik()),
               lambda: lik().pep_site_update(y, y + 1, y, 1.0, 1.0, y.clone(), y.clone(), y.clone()),
               lambda: lik()._kernel_args()]
    for i, make in enumerate(refused):
        with pytest.raises((NotImplementedError, ValueError), match="tensor|float"):
            make()
            pytest.fail(f"case {i} was accepted")


@pytest.mark.parametrize("name", ["gaussian", "student-t"])
def test_cpu_variational_expectations_differentiate_in_the_parameter(name):
    gen = torch.Generator().manual_seed(7)
    fmu, y = torch.randn(2, 9, 1, dtype=F64, generator=gen), torch.randn(2, 9, 1, dtype=F64, generator=gen)
    fvar = torch.rand(2, 9, 1, dtype=F64, generator=gen) + 0.1
    start = torch.tensor([0.6, 1.4], dtype=F64)
    make = (lambda t: mfa.Gaussian(variance=t)) if name == "gaussian" else (lambda t: mfa.StudentT(scale=t, df=4.0))
    lik = make(start)
    total = lambda l: (l.variational_expectations(fmu, fvar, y).sum() + l.log_prob(fmu, y).sum()        # noqa: E731
                       + sum(t.sum() for t in l.predict_mean_and_var(fmu, fvar))
                       + mfa.likelihoods.torch_predict_log_density(l, fmu, fvar, y).sum())
    (grad,) = torch.autograd.grad(total(lik), lik.trainable_variables)
    h = 1e-5
    for b in range(2):                             # d / d theta_b by a central difference, chained through the softplus by hand
        step = torch.zeros(2, dtype=F64)
        step[b] = h
        with torch.no_grad():
            fd = (total(make(start + step)) - total(make(start - step))) / (2 * h)
            chain = torch.sigmoid(lik.trainable_variables[0][b])          # d softplus
        assert abs(float(grad[b]) - float(fd * chain)) <= 1e-7 * (1.0 + abs(float(fd))), (b, float(grad[b]), float(fd * chain))
