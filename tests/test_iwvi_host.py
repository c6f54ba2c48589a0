"""
CPU tests of importance-weighted VI: the numpy statement of ``mf_lik_iw_log_weights_*`` (tests/helpers/iwvi_closed_forms.py) against
central differences of itself, ``iw_log_likelihood_torch`` and ``iw_merged_time_points`` of markovflow_amd/models.py against it, the
symbols of the new entry point, and its argument checks (which return before any launch).

Tolerances (float64).  Central differences: h = 1e-4, rtol 1e-5 / atol 1e-7, the budget of
``test_elbo_backward_gives_the_lengthscale_gradient_through_the_composed_route`` (tests/test_gpu_svgp.py) - here a segment's value is below
1e4 in magnitude and good to a few eps of it, so rounding is 1e-12 x 1e4 / 1e-4 = 1e-7 x (a gradient of order 10 or more), and the
truncation h^2 / 6 x sum_n l'''_n w_n^3 stays below 1e-8.  The torch composition against the helper: both evaluate the same
expressions in float64 and differ in the order of the sums only: rtol 1e-12 / atol 1e-13, as the SVGP composition against its helper
(tests/test_gpu_svgp.py).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import models as MM
from helpers import iwvi_closed_forms as IW
from helpers import likelihood_closed_forms as L

NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
LAYOUT = ((0, 1, 65, 64), (63, 2, 0, 65))          # two series of 130 points in four segments (M = 3)
FN = "mf_lik_iw_log_weights"
K = 3


def make(name):
    params = L.LIKELIHOODS[name][1]
    if name == L.GAUSSIAN:
        return mfa.Gaussian(variance=params[0])
    if name == L.BERNOULLI:
        return mfa.Bernoulli()
    if name == L.POISSON:
        return mfa.Poisson()
    return mfa.StudentT(scale=params[0], df=params[1])


def t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def helper(name, case, b, u_post=None, states=None):
    u_post = case["u_post"][:, b] if u_post is None else u_post
    states = case["states"][:, b] if states is None else states
    return IW.iw_log_weights(L.LIKELIHOODS[name], case["h"], case["w"][b], case["y"][b], case["offsets"][b], states, u_post)


@pytest.mark.parametrize("name", NAMES)
def test_helper_adjoint_against_central_differences_of_its_own_value(name):
    case = IW.random_case(name, 4, LAYOUT, K, seed=1, h=[1.0, 1.0])
    step = 1e-4
    for b in range(2):
        base = helper(name, case, b)
        assert float(np.abs(base["g_u"]).max()) > 1.0
        fd = np.zeros_like(base["g_u"])
        for m in range(3):
            for i in range(2):
                up, down = case["u_post"][:, b].copy(), case["u_post"][:, b].copy()
                up[:, m, i] += step                      # every sample at once: a sample's value depends on its own u_post only
                down[:, m, i] -= step
                hi, lo = helper(name, case, b, u_post=up), helper(name, case, b, u_post=down)
                fd[:, m, i] = (hi["log_lik"].sum(-1) - lo["log_lik"].sum(-1)) / (2 * step)
        np.testing.assert_allclose(base["g_u"], fd, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name", NAMES)
def test_torch_composition_and_its_autograd_gradient_against_the_helper(name):
    case = IW.random_case(name, 4, LAYOUT, K, seed=2, h=[1.0, 1.0])
    u_post = t64(case["u_post"]).requires_grad_(True)
    got = MM.iw_log_likelihood_torch(make(name), t64(case["h"]), t64(case["w"]), t64(case["y"]), torch.tensor(case["indices"]),
                                     t64(case["states"]), u_post)
    assert tuple(got.shape) == (K, 2)
    (grad,) = torch.autograd.grad(got.sum(), u_post)
    for b in range(2):
        want = helper(name, case, b)
        np.testing.assert_allclose(got[:, b].detach().numpy(), want["log_lik"].sum(-1), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(grad[:, b].numpy(), want["g_u"], rtol=1e-12, atol=1e-13)
    # final samples, no correction
    final = case["states"][:, :, :130]
    got = MM.iw_log_likelihood_torch(make(name), t64(case["h"]), None, t64(case["y"]), None, t64(final), None)
    for b in range(2):
        want = IW.iw_log_weights(L.LIKELIHOODS[name], case["h"], None, case["y"][b], case["offsets"][b], final[:, b], None)
        np.testing.assert_allclose(got[:, b].numpy(), want["log_lik"].sum(-1), rtol=1e-12, atol=1e-13)


def test_with_the_prior_at_the_inducing_rows_the_correction_vanishes():
    case = IW.random_case(L.BERNOULLI, 6, LAYOUT, K, seed=3)
    for b in range(2):
        rows = IW.rows_of(case["offsets"][b])[1]
        same = helper(L.BERNOULLI, case, b, u_post=case["prior_z"][:, b])
        final = IW.iw_log_weights(L.LIKELIHOODS[L.BERNOULLI], case["h"], None, case["y"][b], case["offsets"][b],
                                  case["states"][:, b, rows], None)
        assert np.array_equal(same["log_lik"], final["log_lik"])


def test_merged_time_points_are_sorted_and_follow_the_row_formulas():
    rng = np.random.default_rng(4)
    z = np.sort(rng.uniform(0.5, 5.5, size=(2, 5)), axis=-1)
    x = np.sort(rng.uniform(0.0, 6.0, size=(2, 40)), axis=-1)
    x[1, :7] = np.linspace(0.01, 0.3, 7)                   # series 1: several points before the first inducing point
    x[0] = np.sort(np.where(x[0] > z[0, -1], 0.5 * x[0], x[0]))          # series 0: none after the last
    offsets = np.stack([np.concatenate([[0], np.searchsorted(x[b], z[b], side="right"), [40]]) for b in range(2)]).astype(np.int64)
    merged = MM.iw_merged_time_points(t64(x), t64(z), torch.tensor(offsets)).numpy()
    assert merged.shape == (2, 45)
    for b in range(2):
        assert np.array_equal(merged[b], np.sort(np.concatenate([x[b], z[b]])))
        seg, rows_x, rows_z = IW.rows_of(offsets[b])
        assert np.array_equal(merged[b, rows_x], x[b]) and np.array_equal(merged[b, rows_z], z[b])
        assert np.array_equal(rows_z, offsets[b, 1:-1] + np.arange(5)) and np.array_equal(rows_x, np.arange(40) + seg)
    # a point on an inducing point precedes it
    tie = MM.iw_merged_time_points(t64([[0.5, 1.0, 2.0]]), t64([[1.0, 3.0]]), torch.tensor([[0, 2, 3, 3]])).numpy()
    assert np.array_equal(tie, [[0.5, 1.0, 1.0, 2.0, 3.0]])


def _cpu_chain(m=3, d=2):
    eye = torch.eye(d, dtype=torch.float64)
    return mfa.StateSpaceModel(torch.zeros(d, dtype=torch.float64), eye.clone(), (0.5 * eye).expand(m - 1, d, d).contiguous(),
                               torch.zeros(m - 1, d, dtype=torch.float64), eye.expand(m - 1, d, d).contiguous())


def test_argument_checks_of_the_python_layer():
    kern = mfa.Matern32(1.0, 1.0, device="cpu")
    z = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="num_importance_samples"):
            mfa.ImportanceWeightedVI(kern, z, mfa.Bernoulli(), bad, initial_distribution=_cpu_chain())
    with pytest.raises(TypeError, match="Likelihood"):
        mfa.ImportanceWeightedVI(kern, z, "bernoulli", 4, initial_distribution=_cpu_chain())
    with pytest.raises(TypeError):
        mfa.ImportanceWeightedVI(kern, z, mfa.Bernoulli(), 4, num_data=10)          # no num_data, as in the reference
    model = mfa.ImportanceWeightedVI(kern, z, mfa.Bernoulli(), 4, initial_distribution=_cpu_chain())
    assert isinstance(model, mfa.SparseVariationalGaussianProcess) and model.num_data is None
    assert isinstance(model.posterior, mfa.ImportanceWeightedPosteriorProcess) and model.posterior.num_importance_samples == 4
    assert isinstance(model.posterior.proposal_process, mfa.ConditionalProcess)
    assert model.posterior.proposal_process.gauss_markov_model is model.dist_q and model.posterior.likelihood is model.likelihood
    x = torch.tensor([0.5, 0.2, 1.5], dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        model.posterior.predict_f(x)
    with pytest.raises(NotImplementedError):
        model.posterior.predict_state(x)
    with pytest.raises(NotImplementedError):
        model.predict_f(x)
    for method in (model.posterior.sample_f, model.posterior.sample_state, model.posterior.sample_state_trajectories):
        with pytest.raises(ValueError, match="input_data"):
            method(x, 2)
    with pytest.raises(ValueError, match="observations must have shape"):
        model.elbo((x, torch.zeros(3, dtype=torch.float64)))
    with pytest.raises(ValueError, match="batch shape"):
        model.elbo((x[None], torch.zeros(1, 3, 1, dtype=torch.float64)))
    with pytest.raises(ValueError, match="float32"):
        model.dregs_objective((x.float(), torch.zeros(3, 1)))
    case = IW.random_case(L.BERNOULLI, 20, LAYOUT, K, seed=5)
    with pytest.raises(NotImplementedError, match="2d = 20"):
        MM.iw_log_likelihood(mfa.Bernoulli(), t64(case["h"]), t64(case["w"]), t64(case["y"]), torch.tensor(case["offsets"]),
                             t64(case["states"]), t64(case["u_post"]))
    case = IW.random_case(L.BERNOULLI, 4, LAYOUT, K, seed=5)
    for name in ("states", "w", "h"):
        args = {k: t64(case[k]) for k in ("h", "w", "y", "states", "u_post")}
        args[name].requires_grad_(True)
        with pytest.raises(NotImplementedError, match="no adjoint"):
            MM.iw_log_likelihood(mfa.Bernoulli(), args["h"], args["w"], args["y"], torch.tensor(case["offsets"]), args["states"],
                                 args["u_post"])


def test_symbols_are_declared_bound_and_exported():
    assert FN in _lib._SIGS and len(_lib._SIGS[FN][1]) == 21
    assert FN + "_workspace_bytes" in _lib._PLAIN
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "markovflow_amd.h")).read()
    lib = _lib.load()
    for suf in ("_f64", "_f32"):
        assert FN + suf in _lib.exported_symbols()
        assert re.search(r"\bint " + FN + suf + r"\(", header)
        assert getattr(lib, FN + suf).restype is ctypes.c_int
    assert re.search(r"\bsize_t " + FN + r"_workspace_bytes\(", header) and FN + "_workspace_bytes" in _lib.exported_symbols()
    assert "ImportanceWeightedVI" in mfa.__all__ and "ImportanceWeightedPosteriorProcess" in mfa.__all__
    assert mfa.models.ImportanceWeightedVI is mfa.ImportanceWeightedVI
    assert mfa.posterior.ImportanceWeightedPosteriorProcess is mfa.ImportanceWeightedPosteriorProcess
    assert int(lib.mf_version()) == 8
    assert MM.IW_SAMPLE_CHUNK == 8


def test_workspace_bytes():
    size = _lib.load().mf_lik_iw_log_weights_workspace_bytes
    assert int(size(7, 5, 4, 8)) == 7 * 5 * 5 * 8 and int(size(7, 5, 18, 4)) == 7 * 5 * 19 * 4 and int(size(1, 1, 2, 8)) == 24
    for two_d in (0, 1, 3, 5, 17, 20, -2):
        assert int(size(7, 5, two_d, 8)) == 0
    assert int(size(0, 5, 4, 8)) == 0 and int(size(-1, 5, 4, 8)) == 0 and int(size(7, 0, 4, 8)) == 0 and int(size(7, 5, 4, 0)) == 0


def test_entry_point_return_codes_without_touching_the_gpu():
    """Every argument check returns before a launch: the negative position of the argument in the signature."""
    lib = _lib.load()
    var = (ctypes.c_double * 1)(0.5)
    one = ctypes.c_void_p(8)                               # a non-NULL pointer that is never dereferenced: the checks return first
    for suf, size in (("_f64", 8), ("_f32", 4)):
        fn = getattr(lib, FN + suf)
        row = 4 + 1

        def call(bsz=2, n=130, segs=4, two_d=4, k=3, lik=0, params=var, ins=(one,) * 5, u_post=one, tiles=5, tab=(one,) * 3,
                 nbytes=5 * 3 * row * size, outs=(None, None)):
            return fn(bsz, n, segs, two_d, k, lik, params, *ins, u_post, tiles, *tab, nbytes, *outs, None)

        assert call(bsz=-1) == -1 and call(n=-1) == -2 and call(segs=0) == -3
        for two_d in (0, 1, 3, 5, 20, -2):
            assert call(two_d=two_d) == -100
        assert call(k=-1) == -5 and call(k=2 ** 31) == -5
        assert call(lik=7) == -6 and call(lik=-1) == -6 and call(params=None) == -7
        assert call(lik=3, params=(ctypes.c_double * 3)(1.0, -2.0, 0.0)) == -7
        assert call(lik=1, params=None) == 0               # Bernoulli and Poisson take no parameters; no output: nothing asked for
        assert call(tiles=-1) == -14 and call(tiles=2 ** 31) == -14 and call(n=0) == -14          # tiles without points
        assert call(tiles=2 ** 30, k=17) == -14            # more blocks than a grid holds
        assert call(outs=(None, one), u_post=None) == -20  # the adjoint needs the draw it belongs to
        # from here on an output is asked for: the NULL checks
        both = (one, one)
        for i in range(5):
            assert call(ins=(one,) * i + (None,) + (one,) * (4 - i), outs=both) == -(8 + i)
        # w may be NULL beside a NULL u_post: the next check is reached
        assert call(ins=(one, None, one, one, one), u_post=None, tab=(None, one, one), outs=(one, None)) == -15
        for i in range(3):
            assert call(tab=(one,) * i + (None,) + (one,) * (2 - i), outs=both) == -(15 + i)
        assert call(nbytes=5 * 3 * row * size - 1, outs=both) == -18 and call(nbytes=0, outs=both) == -18
        assert call(bsz=0, outs=both) == 0 and call(k=0, outs=both) == 0
        assert call(bsz=0, two_d=3, outs=both) == -100     # checked before the empty batch returns
