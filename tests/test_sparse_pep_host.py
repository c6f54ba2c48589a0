"""
CPU tests of sparse power expectation propagation: ``sparse_pep_site_update_torch`` and ``pair_cavity`` of markovflow_amd/models.py
against the numpy statement of tests/helpers/sparse_pep_closed_forms.py, the local form of the site normaliser against the
leave-one-out posteriors of the dense loop, the Gaussian fixed point, and the argument checks of the Python layer and of
``mf_lik_sparse_pep_site_update_*`` (which return before any launch).

Tolerances (float64).  The torch composition sums a segment with ``index_add_``, the helper in the kernel's order, and the two project
``fvar`` in different orders, so the comparison carries the sensitivity of (I, g1, g2) to a rounding of ``fvar``: at most 130 terms of
order one per segment, rounding 130 eps = 3e-14 of the magnitude, times a condition number of the discretised derivatives that stays
below 1e3 on these inputs - rtol 1e-10 of the largest magnitude in the tensor (atol = rtol x that magnitude).  The normaliser's two
forms meet through a dense inverse of K_uu and dense ``2d x 2d`` inverses: the project's state-space-against-dense tolerance, rtol
1e-6 / atol 1e-7.  The Gaussian fixed point is a closed form: rtol 1e-12.
"""
import ctypes
import re
import os

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import models as MM
from helpers import likelihood_closed_forms as L
from helpers import sparse_pep_closed_forms as SP

NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
M32 = [dict(order=3, ls=1.0, var=1.0, period=None, osc=0)]
Z5 = np.array([0.6, 1.9, 3.1, 4.2, 5.5])
LAYOUT = ((0, 1, 65, 64), (63, 2, 0, 65))          # two series of 130 points in four segments
FN = "mf_lik_sparse_pep_site_update"


def make(name, nq=20):
    params = L.LIKELIHOODS[name][1]
    if name == L.GAUSSIAN:
        return mfa.Gaussian(variance=params[0], num_gauss_hermite_points=nq)
    if name == L.BERNOULLI:
        return mfa.Bernoulli(num_gauss_hermite_points=nq)
    if name == L.POISSON:
        return mfa.Poisson(num_gauss_hermite_points=nq)
    return mfa.StudentT(scale=params[0], df=params[1], num_gauss_hermite_points=nq)


def t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def inputs(name, two_d=4, seed=0, layout=LAYOUT):
    return SP.random_case(name, two_d, layout, seed)


def close(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaNs in different places"
    scale = float(np.nanmax(np.abs(want))) if np.isfinite(want).any() else 0.0
    np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), rtol=0, atol=1e-10 * (scale + 1.0), err_msg=what)


@pytest.mark.parametrize("lr", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("name", NAMES)
def test_torch_composition_against_the_helper(name, alpha, lr):
    d = inputs(name)
    d["c"][1, 70] = -1e6                      # series 1, last segment: an undefined point
    d["cav_cov"][0, 2] = np.nan               # series 0, segment 2: a cavity that does not exist
    sites = [t64(d[k]).clone() for k in ("nat1", "nat2", "log_norm")]
    led_sum, fmu, fvar, led = MM.sparse_pep_site_update_torch(make(name), t64(d["w"]), t64(d["c"]), t64(d["y"]), torch.tensor(d["indices"]),
                                                              t64(d["cav_mean"]), t64(d["cav_cov"]), alpha, lr, *sites,
                                                              seg_const=t64(d["seg_const"]))
    for b in range(2):
        want = SP.segment_pep_update(L.LIKELIHOODS[name], d["w"][b], d["c"][b], d["y"][b], d["offsets"][b], d["cav_mean"][b],
                                     d["cav_cov"][b], alpha, lr, d["nat1"][b], d["nat2"][b], d["log_norm"][b], d["seg_const"][b])
        assert list(want["skipped"]) == [[False, False, True, False], [False, False, False, True]][b]
        for key, got in (("nat1", sites[0]), ("nat2", sites[1]), ("log_norm", sites[2]), ("led_sum", led_sum), ("fmu", fmu),
                         ("fvar", fvar), ("led", led)):
            close(f"{name} series {b} {key}", got[b].numpy(), want[key])
        for s in np.flatnonzero(want["skipped"]):
            for key, got in (("nat1", sites[0]), ("nat2", sites[1]), ("log_norm", sites[2])):
                assert np.array_equal(got[b, s].numpy(), d[key][b, s]), "an undefined segment keeps its sites bit for bit"
            assert np.isnan(float(led_sum[b, s]))
    # the empty segments decay by 1 - lr alpha (log_norm: plus lr seg_const)
    keep = 1.0 - lr * alpha
    np.testing.assert_allclose(sites[0][0, 0].numpy(), keep * d["nat1"][0, 0], rtol=1e-15)
    np.testing.assert_allclose(float(sites[2][1, 2]), keep * d["log_norm"][1, 2] + lr * d["seg_const"][1, 2], rtol=1e-14)
    assert float(led_sum[0, 0]) == 0.0
    # evaluation only: the same per-point numbers and sums, no site touched
    again = MM.sparse_pep_site_update_torch(make(name), t64(d["w"]), t64(d["c"]), t64(d["y"]), torch.tensor(d["indices"]),
                                            t64(d["cav_mean"]), t64(d["cav_cov"]), alpha, lr, None, None, None)
    for a, b in zip(again, (led_sum, fmu, fvar, led)):
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("name", [L.BERNOULLI, L.GAUSSIAN])
def test_local_site_normaliser_is_the_leave_one_out_ratio(name, alpha):
    """Gamma_s = G(m_c, S_c) - G(m_s, S_s) against log Z(q with t_s^(1 - beta_s)) - log Z(q) from M + 1 dense posteriors, after a
    few steps of the dense loop (some segments hold several points, the last of Z5's none or few); then ``pair_cavity`` of the model
    against both."""
    x, y = L.draw_series(L.LIKELIHOODS[name], M32, 33, seed=1)
    _, run = SP.dense_sparse_pep(L.LIKELIHOODS[name], M32, x, y, Z5, alpha, 0.5, iterations=4)
    assert float(np.abs(run.nat2).max()) > 1e-3
    loo = run.leave_one_out()
    cm, cc, gamma = run.cavity()
    np.testing.assert_allclose(gamma, loo, rtol=1e-6, atol=1e-7)
    assert float(np.abs(loo[run.counts > 0]).min()) > 1e-4, "the comparison is not one of zeros"
    mu, sigma = run.posterior()
    pm, pc = SP.SC.pair_marginals(mu, sigma, run.pinf, run.d)
    got = MM.pair_cavity(t64(pm), t64(pc), t64(run.nat1), t64(run.nat2), t64(run.beta))
    np.testing.assert_allclose(got[0].numpy(), cm, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got[1].numpy(), cc, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got[2].numpy(), loo, rtol=1e-6, atol=1e-7)


def test_pair_cavity_without_a_positive_definite_precision_is_nan_for_that_pair_only():
    rng = np.random.default_rng(3)
    a = rng.normal(size=(3, 4, 4))
    cov = t64(a @ a.transpose(0, 2, 1) + 0.5 * np.eye(4))
    mean, nat1 = t64(rng.normal(size=(3, 4))), t64(rng.normal(size=(3, 4)))
    nat2 = torch.zeros(3, 4, 4, dtype=torch.float64)
    nat2[1] = -100.0 * torch.eye(4, dtype=torch.float64)          # pair 1: removing half of this site leaves a negative precision
    beta = t64([0.5, 0.5, 0.0])
    cm, cc, gamma = MM.pair_cavity(mean, cov, nat1, nat2, beta)
    assert bool(torch.isnan(cm[1]).all()) and bool(torch.isnan(cc[1]).all()) and bool(torch.isnan(gamma[1]))
    assert bool(torch.isfinite(cm[[0, 2]]).all()) and bool(torch.isfinite(cc[[0, 2]]).all()) and bool(torch.isfinite(gamma[[0, 2]]).all())
    # beta = 0: the cavity is the marginal and the ratio is one
    np.testing.assert_allclose(cm[2].numpy(), mean[2].numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(cc[2].numpy(), cov[2].numpy(), rtol=1e-10, atol=1e-12)
    assert abs(float(gamma[2])) < 1e-12


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.25])
def test_gaussian_likelihood_steps_geometrically_whatever_the_cavity(alpha):
    """L2 = -alpha / (2 variance) and L1 = alpha y / variance at every cavity, so n steps at lr = 1 from zero sites leave
    (1 - (1 - alpha)^n) sum_k (y_k / variance, -1 / (2 variance)) projected through w_k - with a fresh random cavity at every step."""
    var = L.LIKELIHOODS[L.GAUSSIAN][1][0]
    d = inputs(L.GAUSSIAN)
    w, y, idx = t64(d["w"]), t64(d["y"]), torch.tensor(d["indices"])
    sites = [torch.zeros_like(t64(d[k])) for k in ("nat1", "nat2", "log_norm")]
    flat = (idx + torch.arange(2)[:, None] * 4).reshape(-1)
    full1 = torch.zeros(8, 4, dtype=torch.float64).index_add_(0, flat, (y[..., None] * w / var).reshape(-1, 4)).reshape(2, 4, 4)
    full2 = torch.zeros(8, 4, 4, dtype=torch.float64).index_add_(
        0, flat, (-0.5 / var * w[..., :, None] * w[..., None, :]).reshape(-1, 4, 4)).reshape(2, 4, 4, 4)
    for n in range(1, 6):
        fresh = inputs(L.GAUSSIAN, seed=10 + n)
        MM.sparse_pep_site_update_torch(make(L.GAUSSIAN), w, t64(d["c"]), y, idx, t64(fresh["cav_mean"]), t64(fresh["cav_cov"]), alpha,
                                        1.0, *sites)
        factor = 1.0 - (1.0 - alpha) ** n
        np.testing.assert_allclose(sites[0].numpy(), factor * full1.numpy(), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(sites[1].numpy(), factor * full2.numpy(), rtol=1e-12, atol=1e-13)


def test_argument_checks_of_the_python_layer():
    lik, kern = mfa.Bernoulli(), mfa.Matern32(1.0, 1.0, device="cpu")
    z = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64)
    for alpha in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            mfa.SparsePowerExpectationPropagation(kern, z, lik, alpha=alpha)
    for lr in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="learning_rate"):
            mfa.SparsePowerExpectationPropagation(kern, z, lik, learning_rate=lr)
    with pytest.raises(TypeError, match="Likelihood"):
        mfa.SparsePowerExpectationPropagation(kern, z, "bernoulli")
    with pytest.raises(ValueError, match="sorted"):
        mfa.SparsePowerExpectationPropagation(kern, z.flip(0), lik)
    model = mfa.SparsePowerExpectationPropagation(kern, z, lik)
    assert model.learning_rate == 1.0 and model.alpha == 1.0 and mfa.models.SparsePowerExpectationPropagation is type(model)
    assert isinstance(model, MM._SparseSitesGaussianProcess) and issubclass(mfa.SparseCVIGaussianProcess, MM._SparseSitesGaussianProcess)
    assert tuple(model.nat1.shape) == (4, 4) and tuple(model.nat2.shape) == (4, 4, 4) and tuple(model.log_norm.shape) == (4,)
    assert all(float(t.abs().max()) == 0.0 for t in (model.nat1, model.nat2, model.log_norm))
    x = torch.tensor([0.5, 0.2, 1.5], dtype=torch.float64)
    with pytest.raises(ValueError, match="time_points must be sorted"):
        model.update_sites((x, torch.zeros(3, 1, dtype=torch.float64)))
    with pytest.raises(ValueError, match="observations must have shape"):
        model.update_sites((x, torch.zeros(3, dtype=torch.float64)))
    d = inputs(L.BERNOULLI)
    args = [t64(d[k]) for k in ("w", "c", "y")] + [torch.tensor(d["indices"])] + [t64(d[k]) for k in ("cav_mean", "cav_cov")]
    n1, n2, ln = (t64(d[k]) for k in ("nat1", "nat2", "log_norm"))
    for alpha in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            MM.sparse_pep_site_update_torch(lik, *args, alpha, 0.5, n1, n2, ln)
    with pytest.raises(ValueError, match="learning_rate"):
        MM.sparse_pep_site_update_torch(lik, *args, 0.5, 1.5, n1, n2, ln)
    for sites in ((n1, n2, None), (n1, None, ln), (None, n2, ln), (None, None, ln)):
        with pytest.raises(ValueError, match="given together"):
            MM.sparse_pep_site_update_torch(lik, *args, 0.5, 0.5, *sites)
        with pytest.raises(ValueError, match="given together"):
            MM.sparse_pep_site_update_hip(lik, args[0], args[1], args[2], torch.tensor(d["offsets"]), args[4], args[5], 0.5, 0.5, *sites)
    assert all(np.array_equal(t.numpy(), d[k]) for t, k in ((n1, "nat1"), (n2, "nat2"), (ln, "log_norm")))


def test_symbols_are_declared_bound_and_exported():
    assert FN in _lib._SIGS and len(_lib._SIGS[FN][1]) == 31
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "markovflow_amd.h")).read()
    lib = _lib.load()
    for suf in ("_f64", "_f32"):
        assert FN + suf in _lib.exported_symbols()
        assert re.search(r"\bint " + FN + suf + r"\(", header)
        assert getattr(lib, FN + suf).restype is ctypes.c_int
    assert "SparsePowerExpectationPropagation" in mfa.__all__


def test_entry_point_return_codes_without_touching_the_gpu():
    """Every argument check returns before a launch: the negative position of the argument in the signature."""
    lib = _lib.load()
    arr = lambda *v: (ctypes.c_double * len(v))(*v)       # noqa: E731
    x, w = np.polynomial.hermite.hermgauss(20)
    nodes, weights, var = arr(*x), arr(*w), arr(0.5)
    one = ctypes.c_void_p(8)                               # a non-NULL pointer that is never dereferenced: the checks return first
    for suf, size in (("_f64", 8), ("_f32", 4)):
        fn = getattr(lib, FN + suf)
        row = 4 * 5 // 2 + 4 + 1

        def call(bsz=2, n=130, segs=4, two_d=4, lik=0, params=var, nq=20, nd=nodes, wt=weights, alpha=0.5, lr=0.5, ins=(one,) * 6,
                 const=None, tiles=5, tab=(one,) * 3, nbytes=5 * row * size, sites=(one,) * 3, outs=(None,) * 4):
            return fn(bsz, n, segs, two_d, lik, params, nq, nd, wt, alpha, lr, *ins, const, tiles, *tab, nbytes, *sites, *outs, None)

        assert call(bsz=-1) == -1 and call(n=-1) == -2 and call(segs=0) == -3
        for two_d in (0, 1, 3, 5, 20, -2):
            assert call(two_d=two_d) == -100
        assert call(lik=7) == -5 and call(params=None) == -6 and call(nq=0) == -7 and call(nq=33) == -7
        assert call(nd=None) == -8 and call(wt=None) == -9
        for alpha in (0.0, -1.0, 1.5, float("nan")):
            assert call(alpha=alpha) == -10
        for lr in (-0.5, 1.5, float("nan")):
            assert call(lr=lr) == -11
        for i in range(6):
            assert call(ins=(one,) * i + (None,) + (one,) * (5 - i)) == -(12 + i)
        assert call(tiles=-1) == -19 and call(tiles=2 ** 31) == -19 and call(n=0) == -19
        for i in range(3):
            assert call(tab=(one,) * i + (None,) + (one,) * (2 - i)) == -(20 + i)
        assert call(nbytes=5 * row * size - 1) == -23 and call(nbytes=0) == -23
        assert call(sites=(None, one, one)) == -24 and call(sites=(one, None, one)) == -25 and call(sites=(one, one, None)) == -26
        assert call(sites=(None, None, one)) == -24 and call(sites=(one, None, None)) == -25
        assert call(sites=(None,) * 3) == 0                # evaluation only with no output: nothing asked for
        assert call(bsz=0) == 0
        assert call(bsz=0, alpha=2.0) == -10               # checked before the empty batch returns
