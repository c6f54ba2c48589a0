"""
``VariationalGaussianProcess`` (mirror of ``markovflow/models/variational.py:30-223``, zero mean function) is the reference's basic
model: ``q`` is a trainable ``StateSpaceModel`` on the states at the data points themselves.  The data term of its ELBO is ONE call
of ``mf_lik_dense_expectations_*`` on the marginals of ``q`` (two passes over tiles of 64 points, two derivatives per point kept), its
adjoint onto those marginals ONE call of ``mf_lik_dense_expectations_adjoint_*``; the KL term is ``StateSpaceModel.kl_divergence``.
``dense_expected_log_likelihood(_torch)`` is that data term as a function.
"""
from typing import Optional, Tuple

import torch

from .. import _lib
from ..emission_model import EmissionModel
from ..kernels import SDEKernel
from ..likelihoods import Likelihood
from ..posterior import ConditionalProcess
from ..state_space_model import StateSpaceModel
from ._common import (_PredictLogDensity, _check_dense_data, _check_shapes, _differentiable_once, _launch, _new_outputs,
                      _refuse_factor_analysis, _refuse_non_stationary, _refuse_stack, _require_likelihood, _workspace)


# ---- VGP: the dense ELBO data term -------------------------------------------------------------------------------------------------
DENSE_EXPECT_MAX_D = 12         # mf_lik_dense_expectations_*: the largest state dimension
DENSE_EXPECT_TILE = 64          # points per tile of its pass 1


class _DenseExpectedLogLikelihood(torch.autograd.Function):
    """Value ``[B]``; the forward keeps the per-point derivatives ``g_mu``, ``g_var`` (2 values per point), the backward expands them
    onto the marginals with ONE call of ``mf_lik_dense_expectations_adjoint_*`` that carries ``grad_out`` as its weight."""

    @staticmethod
    def forward(ctx, means, covs, likelihood, h, y):
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        bsz, n, d = h.shape
        dtype, dev = h.dtype, h.device
        with torch.no_grad():
            new = _new_outputs((bsz,), dtype, dev)
            ve_sum, g_mu, g_var = new(True), new(want, n), new(want, n)
            ws, ws_bytes = _workspace(_lib.load().mf_lik_dense_expectations_workspace_bytes, dev, bsz, n, h.element_size())
            _launch("mf_lik_dense_expectations", dtype, dev, bsz, n, d, *likelihood._kernel_args(), h, means.detach(), covs.detach(),
                    y, ws, ws_bytes, ve_sum, g_mu, g_var)
        if want:
            ctx.save_for_backward(h, g_mu, g_var)
        return ve_sum

    @staticmethod
    def backward(ctx, grad_out):
        _differentiable_once("dense_expected_log_likelihood", "adjoints")
        h, g_mu, g_var = ctx.saved_tensors
        bsz, n, d = h.shape
        new = _new_outputs((bsz, n), h.dtype, h.device)
        g_means, g_covs = new(ctx.needs_input_grad[0], d), new(ctx.needs_input_grad[1], d, d)
        _launch("mf_lik_dense_expectations_adjoint", h.dtype, h.device, bsz, n, d, h, g_mu, g_var, grad_out, g_means, g_covs)
        return g_means, g_covs, None, None, None


def _check_dense(what: str, likelihood: Likelihood, h: torch.Tensor, y: torch.Tensor, means: torch.Tensor, covs: torch.Tensor):
    _require_likelihood(likelihood)
    if h.dim() < 2:
        raise ValueError(f"{what}: h must have shape batch + [N, d], got {tuple(h.shape)}")
    if h.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {h.dtype}")
    batch, n, d = tuple(h.shape[:-2]), h.shape[-2], h.shape[-1]
    _check_shapes(what, dict(y=(y, batch + (n,)), means=(means, batch + (n, d)), covs=(covs, batch + (n, d, d))))
    _lib.same_dtype_device(h, what, y=y, means=means, covs=covs)
    return batch, n, d


def dense_expected_log_likelihood(likelihood: Likelihood, h: torch.Tensor, y: torch.Tensor, means: torch.Tensor,
                                  covs: torch.Tensor) -> torch.Tensor:
    """``sum_k E_q log p(y_k | f_k)`` per series, ``batch_shape``, for a ``q`` with its own marginal at every data point:
    ``fmu = h_k . m_k`` and ``fvar = h_k^T P_k h_k`` (``h [.., N, d]`` the emission rows, ``y [.., N]``, ``means [.., N, d]``,
    ``covs [.., N, d, d]``): ONE call of ``mf_lik_dense_expectations_*`` on HIP tensors, ``d <= 12``.  Differentiable ONCE in ``means``
    and ``covs`` (an unconstrained matrix: the gradient is ``g_var h h^T``) - the forward keeps two derivatives per point, the backward
    is ONE call of ``mf_lik_dense_expectations_adjoint_*`` with ``grad_out`` as its weight; not differentiable in ``h``."""
    batch, n, d = _check_dense("dense_expected_log_likelihood", likelihood, h, y, means, covs)
    if d > DENSE_EXPECT_MAX_D:
        raise NotImplementedError(f"dense_expected_log_likelihood: d = {d} is outside 1, ..., {DENSE_EXPECT_MAX_D}; "
                                  "use dense_expected_log_likelihood_torch")
    if torch.is_grad_enabled() and (h.requires_grad or y.requires_grad):
        raise NotImplementedError("dense_expected_log_likelihood has no adjoint onto h and y: use dense_expected_log_likelihood_torch")
    out = _DenseExpectedLogLikelihood.apply(means.reshape(-1, n, d), covs.reshape(-1, n, d, d), likelihood,
                                            h.detach().reshape(-1, n, d).contiguous(), y.detach().reshape(-1, n).contiguous())
    return out.reshape(batch)


def dense_expected_log_likelihood_torch(likelihood: Likelihood, h: torch.Tensor, y: torch.Tensor, means: torch.Tensor,
                                        covs: torch.Tensor) -> torch.Tensor:
    """The same quantity as a torch composition, differentiable by autograd: ``EmissionModel.project_state_marginals_to_f``,
    ``likelihood.variational_expectations`` and a sum over the points.  It runs on CPU tensors, it is the model's route for
    ``d > 12``, and it is what the kernel pair is measured against."""
    _check_dense("dense_expected_log_likelihood_torch", likelihood, h, y, means, covs)
    fmu, fvar = EmissionModel(h[..., None, :]).project_state_marginals_to_f(means, covs)
    return torch.sum(likelihood.variational_expectations(fmu, fvar, y[..., None]), dim=-1)


class VariationalGaussianProcess(_PredictLogDensity):
    """GP prior, general likelihood, a free-form Gaussian chain ``q`` on the states at the data points themselves, held as a trainable
    ``StateSpaceModel`` (markovflow/models/variational.py:30-223; zero mean function and plain float likelihood parameters - the
    reference takes a ``mean_function`` and gpflow likelihoods with trainable parameters -, a batch of series as leading dimensions).
    The ELBO is ``sum_i E_q log p(y_i | f_i) - KL[q || p]``; ``q`` is trained with any torch optimiser on ``trainable_variables`` or
    with ``ssm_natgrad.SSMNaturalGradient`` on ``dist_q``."""

    def __init__(self, input_data: Tuple[torch.Tensor, torch.Tensor], kernel: SDEKernel, likelihood: Likelihood,
                 initial_distribution: Optional[StateSpaceModel] = None) -> None:
        """
        :param input_data: ``(time_points [batch + [num_data]], observations [batch + [num_data, 1]])``, strictly increasing time
            points, at least two (a ``StateSpaceModel`` needs a transition).
        :param initial_distribution: the initial ``q`` on the data points; the prior by default.
        """
        time_points, observations = input_data
        if not isinstance(kernel, SDEKernel):
            raise TypeError("kernel must be a markovflow_amd.kernels.SDEKernel")
        _refuse_non_stationary(kernel, "VariationalGaussianProcess")
        _refuse_factor_analysis(kernel, "VariationalGaussianProcess")
        _refuse_stack(kernel, "VariationalGaussianProcess")
        _require_likelihood(likelihood)
        _check_dense_data(time_points, observations)
        if time_points.shape[-1] < 2:
            raise ValueError("VariationalGaussianProcess needs at least two data points (a chain needs a transition)")
        if time_points.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {time_points.dtype}")
        _lib.same_dtype_device(observations, type(self).__name__, time_points=time_points)
        if bool((time_points[..., 1:] <= time_points[..., :-1]).any()):
            raise ValueError("time_points must be strictly increasing")
        if initial_distribution is None:
            initial_distribution = kernel.state_space_model(time_points)
        elif not isinstance(initial_distribution, StateSpaceModel):
            raise TypeError("initial_distribution must be a StateSpaceModel")
        if (tuple(initial_distribution.batch_shape) != tuple(time_points.shape[:-1])
                or initial_distribution.num_transitions + 1 != time_points.shape[-1]
                or initial_distribution.state_dim != kernel.state_dim):
            raise ValueError("initial_distribution must be a chain on the time points: batch shape "
                             f"{tuple(time_points.shape[:-1])}, {time_points.shape[-1]} states of dimension {kernel.state_dim}")
        self._kernel = kernel
        self._likelihood = likelihood
        self._time_points = time_points
        self._observations = observations
        self._dist_q = initial_distribution.create_trainable_copy()
        self._posterior = ConditionalProcess(posterior_dist=self._dist_q, kernel=kernel, conditioning_time_points=time_points)
        with torch.no_grad():      # the emission rows and the observations as the kernel reads them: once, not per elbo()
            self._h = kernel.generate_emission_model(time_points).emission_matrix[..., 0, :].contiguous()
            self._y = observations[..., 0].contiguous()

    @property
    def time_points(self) -> torch.Tensor:
        return self._time_points

    @property
    def observations(self) -> torch.Tensor:
        return self._observations

    @property
    def dist_p(self) -> StateSpaceModel:
        """The prior chain on the data points, rebuilt on every access (variational.py:193-198)."""
        return self._kernel.state_space_model(self._time_points)

    @property
    def dist_q(self) -> StateSpaceModel:
        """The variational chain, a trainable copy: its leaves are ``trainable_variables``."""
        return self._dist_q

    @property
    def posterior(self) -> ConditionalProcess:
        return self._posterior

    @property
    def trainable_variables(self) -> Tuple[torch.Tensor, ...]:
        """The leaves of ``dist_q``: ``(mu0, chol_P0, As, offsets, chol_Qs)``."""
        return self._dist_q.trainable_variables

    def _fused(self) -> bool:
        return self._time_points.is_cuda and self._kernel.state_dim <= DENSE_EXPECT_MAX_D

    def _expected_log_likelihood(self) -> torch.Tensor:
        """``sum_i E_q log p(y_i | f_i)`` per series, ``batch_shape``."""
        means, covs = self._dist_q.marginals
        route = dense_expected_log_likelihood if self._fused() else dense_expected_log_likelihood_torch
        return route(self._likelihood, self._h, self._y, means, covs)

    def elbo(self) -> torch.Tensor:
        """``sum_i E_q log p(y_i | f_i) - KL[q || p]``, summed over the batch (variational.py:129-152).  HIP tensors with ``d <= 12``:
        the marginals of ``dist_q`` under the tape, ONE call of ``mf_lik_dense_expectations_*`` whose two derivatives per point the
        backward expands with ONE call of ``mf_lik_dense_expectations_adjoint_*``, and the KL with its adjoints; otherwise
        ``dense_expected_log_likelihood_torch``.  The kernel's hyper-parameters enter through ``dist_p`` in the KL only (the emission
        rows of the SDE kernels are constants), so the ELBO is differentiable in them on either route."""
        ve = torch.sum(self._expected_log_likelihood())
        return ve - torch.sum(self._dist_q.kl_divergence(self.dist_p))

    def loss(self) -> torch.Tensor:
        """``-elbo`` (variational.py:218-222)."""
        return -self.elbo()

    def predict_f(self, new_time_points: torch.Tensor, full_output_cov: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """Posterior mean and variance of ``f`` at ``new_time_points`` (sorted), ``batch + [num_new, 1]`` each."""
        with torch.no_grad():
            return self._posterior.predict_f(new_time_points, full_output_cov)

    _predict_f = predict_f          # (``predict_log_density`` predicts outside the tape, as ``predict_f`` does)
