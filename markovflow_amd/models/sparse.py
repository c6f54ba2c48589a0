"""
The inducing-point models; their fused ops are the functions of ``segmented_ops.py``.

``SparseCVIGaussianProcess`` (mirror of ``markovflow/models/sparse_variational_cvi.py:38-313``, zero mean function) carries
``M + 1`` multivariate sites on the pairs of neighbouring inducing states instead of one site per data point: the chain has ``M``
blocks, and the ``N`` data points enter ``update_sites`` through ONE launch of ``mf_lik_sparse_cvi_site_update_*``.

``SparsePowerExpectationPropagation`` (mirror of ``markovflow/models/sparse_pep.py:78-560``, zero mean function) has the same sites
with a normaliser each, updated by power EP: the batched pair cavity and ONE call of ``mf_lik_sparse_pep_site_update_*``.

``SparseVariationalGaussianProcess`` (mirror of ``markovflow/models/sparse_variational.py:31-270``, zero mean function) holds ``q`` on
the inducing points as a trainable ``StateSpaceModel``; the data term of its ELBO and the adjoint onto the pair marginals of ``q`` are
ONE call of ``mf_lik_sparse_expectations_*``, the KL term is ``StateSpaceModel.kl_divergence``.

``ImportanceWeightedVI`` (mirror of ``markovflow/models/iwvi.py:29-173``, zero mean function) subclasses it: ``K`` proposals drawn by
Matheron's rule, whose assembly from one prior draw, the ``K`` evaluations of ``log p(y_n | f_n)`` at every data point and the adjoint
onto the draw from ``q`` are ONE call of ``mf_lik_iw_log_weights_*``.
"""
from typing import Optional, Tuple

import math

import torch

from .. import _lib, conditionals
from ..kernels import FactorAnalysisKernel, IndependentMultiOutputStack, SDEKernel, StackKernel, _version_key
from ..likelihoods import Likelihood
from ..posterior import ConditionalProcess, ImportanceWeightedPosteriorProcess
from ..ssm_gaussian_transformations import naturals_to_ssm_params
from ..state_space_model import StateSpaceModel
from ._common import (_PredictLogDensity, _refuse_factor_analysis, _refuse_non_stationary, _refuse_stack, _require_likelihood, gradient_correction,
                      gradient_transformation_mean_var_to_expectation)
from .segmented_ops import (SPARSE_FACTOR_LATENTS, SPARSE_FACTOR_MAX_OUTPUTS, SPARSE_MULTI_MIN_TWO_D, SPARSE_SITE_MAX_TWO_D,
                            _sparse_point_marginals, iw_log_likelihood, iw_log_likelihood_torch, iw_merged_time_points, pair_cavity,
                            sparse_cvi_site_update_hip, sparse_cvi_site_update_torch, sparse_expectation_tiles,
                            sparse_expected_log_likelihood, sparse_expected_log_likelihood_torch,
                            sparse_factor_expected_log_likelihood, sparse_factor_expected_log_likelihood_torch,
                            sparse_factor_site_projections, sparse_multi_expected_log_likelihood,
                            sparse_multi_expected_log_likelihood_torch, sparse_multi_output_expected_log_likelihood_torch,
                            sparse_multi_site_projections, sparse_pep_site_update_hip, sparse_pep_site_update_torch,
                            sparse_site_projections, sparse_stack_expected_log_likelihood,
                            sparse_stack_expected_log_likelihood_torch, sparse_stack_instantiated)


class _SparseGaussianProcess(_PredictLogDensity):
    """What the inducing-point models share: the validated kernel, likelihood and inducing points, the checks on a data set,
    the cache of the per-point projections, the stationary prior beyond the ends of the chain and ``predict_log_density``."""

    _multi_latent = False      # True in the one model that projects a marginal per latent function of the likelihood
    _multi_output = False      # True in the one model that takes one observed series per output of the kernel

    def __init__(self, kernel: SDEKernel, likelihood: Likelihood, inducing_points: torch.Tensor, min_inducing: int) -> None:
        if not isinstance(kernel, SDEKernel):
            raise TypeError("kernel must be a markovflow_amd.kernels.SDEKernel")
        _refuse_non_stationary(kernel, type(self).__name__)
        if not self._multi_output:
            _refuse_factor_analysis(kernel, type(self).__name__)
            _refuse_stack(kernel, type(self).__name__)
        elif isinstance(kernel, StackKernel) and not isinstance(kernel, IndependentMultiOutputStack):
            raise NotImplementedError(f"{type(self).__name__} takes a StackKernel with its multi-output emission only: use "
                                      "IndependentMultiOutputStack")
        _require_likelihood(likelihood, multi_latent=self._multi_latent)
        if likelihood.latent_dim > 1 and likelihood.latent_dim != kernel.output_dim:
            raise ValueError(f"the likelihood has latent_dim = {likelihood.latent_dim}, the kernel has output_dim = "
                             f"{kernel.output_dim}: a multi-latent likelihood needs one output of the kernel per latent function")
        if (not isinstance(inducing_points, torch.Tensor) or inducing_points.dim() < 1
                or inducing_points.shape[-1] < min_inducing):
            raise ValueError("inducing_points must be a tensor of shape batch + [num_inducing] with at least "
                             + {1: "one point", 2: "two points"}[min_inducing])
        if inducing_points.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {inducing_points.dtype}")
        if bool((inducing_points[..., 1:] < inducing_points[..., :-1]).any()):
            raise ValueError("inducing_points must be sorted")
        if isinstance(kernel, StackKernel):        # lead + [K, M]: one set of inducing points per chain
            kernel._check_batch(inducing_points.shape[:-1], "inducing_points")
        self._kernel = kernel
        self._likelihood = likelihood
        self.inducing_inputs = inducing_points
        self._projection_cache = None

    def _check_data(self, input_data: Tuple[torch.Tensor, torch.Tensor], what: str) -> Tuple[torch.Tensor, torch.Tensor]:
        time_points, observations = input_data
        if isinstance(self._kernel, StackKernel):
            return self._check_stack_data(time_points, observations, what)
        outputs = self._kernel.output_dim
        # one observed series per output of the kernel: the one model that says so, a likelihood with ONE latent function
        per_output = self._multi_output and outputs > 1 and self._likelihood.latent_dim == 1
        if observations.dim() < 2 or not (observations.shape[-1] == 1 or (per_output and observations.shape[-1] == outputs)):
            raise ValueError(f"{what}: observations must have shape batch + [num_data, 1]"
                             + (f" or batch + [num_data, {outputs}] (one series per output of the kernel)" if per_output else "")
                             + f", got {tuple(observations.shape)}")
        if tuple(time_points.shape) != tuple(observations.shape[:-1]):
            raise ValueError(f"{what}: time_points must have shape observations.shape[:-1]")
        if tuple(time_points.shape[:-1]) != tuple(self.inducing_inputs.shape[:-1]):
            raise ValueError(f"{what}: the data must carry the batch shape of the inducing points, "
                             f"{tuple(self.inducing_inputs.shape[:-1])}, got {tuple(time_points.shape[:-1])}")
        _lib.same_dtype_device(self.inducing_inputs, f"{type(self).__name__}.{what}", time_points=time_points,
                               observations=observations)
        return time_points, observations

    def _check_stack_data(self, time_points: torch.Tensor, observations: torch.Tensor, what: str):
        """The data of a stack kernel with ``K`` chains: time points ``lead + [K, N]`` - every chain has its own, as it has its own
        inducing points - and observations ``lead + [N, 1]`` under a ``K``-latent likelihood or ``lead + [N, K]`` (one series per
        output) under a one-latent likelihood."""
        chains = self._kernel.num_kernels
        batch = tuple(self.inducing_inputs.shape[:-1])
        if time_points.dim() < 2 or tuple(time_points.shape[:-1]) != batch:
            raise ValueError(f"{what}: time_points must have shape {batch} + [num_data] (the batch shape of the inducing points, "
                             f"which ends in the {chains} chains of the kernel), got {tuple(time_points.shape)}")
        columns = 1 if self._likelihood.latent_dim > 1 else chains
        expected = batch[:-1] + (time_points.shape[-1], columns)
        if tuple(observations.shape) != expected:
            raise ValueError(f"{what}: observations must have shape {expected} (" + ("one column under a likelihood with "
                             f"{chains} latent functions" if columns == 1 else "one series per output of the kernel")
                             + f"), got {tuple(observations.shape)}")
        _lib.same_dtype_device(self.inducing_inputs, f"{type(self).__name__}.{what}", time_points=time_points,
                               observations=observations)
        return time_points, observations

    def _compute_projections(self, time_points: torch.Tensor):
        """What ``_projections`` keeps for a data tensor (computed under ``no_grad``)."""
        raise NotImplementedError

    def _projections(self, time_points: torch.Tensor):
        """``_compute_projections`` of the data, kept until the data, the inducing points or a hyper-parameter of the kernel is
        replaced or written in place (tensor identity, data pointer and version counter, as the filter caches)."""
        sources = ([time_points, self.inducing_inputs] + [x for comp in self._kernel._components() for x in comp._leaves()]
                   + list(self._emission_sources()))
        key = tuple(_version_key(x) for x in sources)
        cached = self._projection_cache
        if (cached is not None and None not in key and cached[0] == key and len(cached[1]) == len(sources)
                and all(a is b for a, b in zip(cached[1], sources))):          # (the cache holds the tensors: ids are not reused)
            return cached[2]
        with torch.no_grad():
            out = self._compute_projections(time_points)
        self._projection_cache = (key, sources, out)
        return out

    def _emission_sources(self) -> Tuple[torch.Tensor, ...]:
        """The hyper-parameters of the kernel's emission that are not hyper-parameters of its chain (a ``FactorAnalysisKernel``'s
        loading matrix): part of the key of ``_projections`` whenever the projections depend on them."""
        return tuple(getattr(self._kernel, "_emission_leaves", tuple)())

    def _stationary_prior(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(m0, P0)`` of the kernel on the inducing points' batch, dtype and device: the outer neighbour of the first and the
        last pair."""
        z = self.inducing_inputs
        m0 = self._kernel.initial_mean(tuple(z.shape[:-1])).to(dtype=z.dtype, device=z.device)
        p0 = self._kernel.initial_covariance(z[..., :1]).to(dtype=z.dtype, device=z.device)
        return m0, p0

    def _predict_f(self, new_time_points: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.posterior.predict_f(new_time_points)


class _SparseSitesGaussianProcess(_SparseGaussianProcess):
    """What the two site-based inducing-point models share: ``M + 1`` Gaussian sites in natural form on the pairs
    ``v_m = [u_{m-1}, u_m]`` of neighbouring inducing states, ``q(s) = p(s) prod_m t_m(v_m)`` (pairs ``0`` and ``M`` have the stationary
    prior as their outer neighbour) - the sites, the chains ``dist_p`` / ``dist_q`` on the inducing points, the posterior process, the
    pair marginals, the sorted-data rule and the per-point projections."""

    def __init__(self, kernel: SDEKernel, inducing_points: torch.Tensor, likelihood: Likelihood, learning_rate: float) -> None:
        super().__init__(kernel, likelihood, inducing_points, min_inducing=1)
        if not 0.0 <= float(learning_rate) <= 1.0:
            raise ValueError(f"learning_rate must lie in [0, 1], got {learning_rate}")
        self.learning_rate = float(learning_rate)
        # sparse_variational_cvi.py:131-137
        batch, two_d = tuple(inducing_points.shape[:-1]), 2 * kernel.state_dim
        shape = batch + (inducing_points.shape[-1] + 1, two_d)
        self.nat1 = torch.zeros(shape, dtype=inducing_points.dtype, device=inducing_points.device)
        self.nat2 = torch.zeros(shape + (two_d,), dtype=inducing_points.dtype, device=inducing_points.device)
        self._sorted_data = None           # the data tensor last found sorted, and its (data pointer, version)

    @property
    def _chain_points(self) -> torch.Tensor:
        """The time points of ``dist_p`` / ``dist_q``: the inducing points - and for ``M = 1``, since a ``StateSpaceModel`` needs a
        transition (as the reference's, state_space_model.py:111-116), a second state ``APPROX_INF`` to the right of the only one:
        the stationary prior, independent of everything (``A = 0``, ``Q = P_inf``), which no site touches and which adds nothing to
        the KL divergence.  The pair ``(u_0, that state)`` IS pair ``M``, whose outer neighbour is the stationary prior."""
        z = self.inducing_inputs
        if z.shape[-1] > 1:
            return z
        return torch.cat([z, z + conditionals.APPROX_INF], dim=-1)

    @property
    def dist_p(self) -> StateSpaceModel:
        """The prior chain on the inducing points (sparse_variational_cvi.py:301-306; ``M = 1``: see ``_chain_points``)."""
        return self._kernel.state_space_model(self._chain_points)

    @property
    def dist_q(self) -> StateSpaceModel:
        """The posterior chain on the inducing points: the sites' diagonal halves of neighbouring pairs summed onto the prior
        naturals, the off-diagonal block times two, then ``naturals_to_ssm_params`` (sparse_variational_cvi.py:139-174)."""
        prec = self.dist_p.precision
        sd = self._kernel.state_dim
        nat1, nat2 = self.nat1, self.nat2
        lik_nat1 = nat1[..., 1:, :sd] + nat1[..., :-1, sd:]
        lik_nat2_diag = nat2[..., 1:, :sd, :sd] + nat2[..., :-1, sd:, sd:]
        lik_nat2_sub = nat2[..., 1:-1, sd:, :sd]
        if self.inducing_inputs.shape[-1] == 1:           # the second state of ``_chain_points`` carries no site
            lik_nat1 = torch.cat([lik_nat1, torch.zeros_like(lik_nat1)], dim=-2)
            lik_nat2_diag = torch.cat([lik_nat2_diag, torch.zeros_like(lik_nat2_diag)], dim=-3)
            lik_nat2_sub = torch.zeros_like(lik_nat2_diag[..., :1, :, :])
        theta_diag = -0.5 * prec.block_diagonal + lik_nat2_diag
        theta_sub = -prec.block_sub_diagonal + 2.0 * lik_nat2_sub
        a_s, offsets, chol_p0, chol_q, mu0 = naturals_to_ssm_params(lik_nat1, theta_diag, theta_sub)
        return StateSpaceModel(initial_mean=mu0, chol_initial_covariance=chol_p0, state_transitions=a_s, state_offsets=offsets,
                               chol_process_covariances=chol_q)

    @property
    def posterior(self) -> ConditionalProcess:
        """Posterior process for prediction at any time points (sparse_variational_cvi.py:232-239)."""
        return ConditionalProcess(posterior_dist=self.dist_q, kernel=self._kernel, conditioning_time_points=self._chain_points)

    # ---- data --------------------------------------------------------------------------------------------------------------------
    def _check_data(self, input_data: Tuple[torch.Tensor, torch.Tensor], what: str) -> Tuple[torch.Tensor, torch.Tensor]:
        time_points, observations = super()._check_data(input_data, what)
        # the data must be sorted (one pass over the data and one read-back: once per data tensor and version, not once per step)
        key = _version_key(time_points)
        known = self._sorted_data
        if known is None or known[0] is not time_points or key is None or known[1] != key:
            if bool((time_points[..., 1:] < time_points[..., :-1]).any()):
                raise ValueError(f"{what}: time_points must be sorted")
            self._sorted_data = (time_points, key)
        return time_points, observations

    def _fused(self, time_points: torch.Tensor) -> bool:
        return time_points.is_cuda and 2 * self._kernel.state_dim <= SPARSE_SITE_MAX_TWO_D

    def _compute_projections(self, time_points: torch.Tensor):
        """``sparse_site_projections`` of the data."""
        return sparse_site_projections(self._kernel, time_points, self.inducing_inputs)

    def _pair_marginals(self, dist_q: StateSpaceModel) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(m_pair [.., M+1, 2d], S_pair [.., M+1, 2d, 2d])`` of ``dist_q``, the stationary prior beyond both ends."""
        pair_mean, pair_cov = conditionals.pairwise_marginals(dist_q, *self._stationary_prior())
        segs = self.inducing_inputs.shape[-1] + 1                             # (``M = 1``: the pairs of the real state only, see ``_chain_points``)
        return pair_mean[..., :segs, :], pair_cov[..., :segs, :, :]


class SparseCVIGaussianProcess(_SparseSitesGaussianProcess):
    """GP prior, general likelihood, Gaussian posterior on the states ``u = s(z)`` at ``M`` inducing points, parameterised by
    ``M + 1`` Gaussian sites in natural form on the pairs ``v_m = [u_{m-1}, u_m]`` of neighbouring inducing states,
    ``q(s) = p(s) prod_m t_m(v_m)``; pairs ``0`` and ``M`` have the stationary prior as their outer neighbour.  A data point with
    ``z_{m-1} < x <= z_m`` contributes to site ``m`` through the conditional ``p(f(x) | v_m)`` (sparse_variational_cvi.py:38-313;
    zero mean function, plain float likelihood parameters, a batch of series as leading dimensions)."""

    def __init__(self, kernel: SDEKernel, inducing_points: torch.Tensor, likelihood: Likelihood, learning_rate: float = 0.1) -> None:
        """
        :param inducing_points: ``batch + [num_inducing]``, sorted.
        :param likelihood: a ``markovflow_amd.likelihoods.Likelihood``.
        :param learning_rate: the step ``rho`` of ``update_sites``, in [0, 1].
        """
        super().__init__(kernel, inducing_points, likelihood, learning_rate)

    def _site_kernel(self, time_points, observations, dist_q, update: bool):
        """ONE launch of ``mf_lik_sparse_cvi_site_update_*``: the in-place site update, or (``update`` False) its projection-only
        mode, which returns ``(fmu, fvar, ve)``, ``batch + [N]`` each."""
        w, c, _, offsets = self._projections(time_points)
        pair_mean, pair_cov = self._pair_marginals(dist_q)
        if update:
            return sparse_cvi_site_update_hip(self._likelihood, w, c, observations[..., 0], offsets, pair_mean, pair_cov,
                                              self.learning_rate, self.nat1, self.nat2)
        return sparse_cvi_site_update_hip(self._likelihood, w, c, observations[..., 0], offsets, pair_mean, pair_cov, 0.0, None, None,
                                          want_outputs=True)

    # ---- inference ---------------------------------------------------------------------------------------------------------------
    def local_objective(self, Fmu: torch.Tensor, Fvar: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        """The variational expectations, ``[..., 1] -> [...]`` (sparse_variational_cvi.py:260-268)."""
        return self._likelihood.variational_expectations(Fmu, Fvar, Y)

    def local_objective_and_gradients(self, Fmu: torch.Tensor, Fvar: torch.Tensor, Y: torch.Tensor
                                      ) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        """The summed local objective and its gradients with respect to ``[mu, var + mu^2]`` (sparse_variational_cvi.py:241-258;
        the reference's tape is the derivative pair the likelihood computes with the value)."""
        fmu, fvar = Fmu.detach(), Fvar.detach()
        with torch.no_grad():
            ve, g_mu, g_var = self._likelihood._expectations(fmu, fvar, Y)
        return torch.sum(ve), gradient_transformation_mean_var_to_expectation((fmu, fvar), (g_mu, g_var))

    def update_sites(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> None:
        """One joint CVI step on the sites, in place: ``theta_m <- (1 - rho) theta_m + rho g_m`` with ``g_m`` the gradients of the
        variational expectations of the segment's points, projected back onto the pair through ``p(f_k | v_m)``
        (sparse_variational_cvi.py:176-221).  HIP tensors with ``2d <= 18``: the pair marginals of ``dist_q``, the cached per-point
        projections and ONE launch of ``mf_lik_sparse_cvi_site_update_*``; ``2d > 18``: ``sparse_cvi_site_update_torch``."""
        time_points, observations = self._check_data(input_data, "update_sites")
        with torch.no_grad():
            if self._fused(time_points):
                self._site_kernel(time_points, observations, self.dist_q, update=True)
                return
            w, c, indices, _ = self._projections(time_points)
            pair_mean, pair_cov = self._pair_marginals(self.dist_q)
            sparse_cvi_site_update_torch(self._likelihood, w, c, observations[..., 0], indices, pair_mean, pair_cov,
                                         self.learning_rate, self.nat1, self.nat2)

    def classic_elbo(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``sum_i E_q log p(y_i | f_i) - KL[q(u) || p(u)]`` (sparse_variational_cvi.py:270-292).  Without a gradient on HIP tensors
        the expectations come from the site kernel's projection-only mode; with a kernel hyper-parameter that requires a gradient
        every piece takes its differentiable route (pair marginals under the tape, ``conditional_predict``'s torch branch, the
        likelihood's autograd function, the KL adjoints): ``loss(...).backward()`` gives the hyper-parameter gradients with the
        sites held fixed."""
        time_points, observations = self._check_data(input_data, "classic_elbo")
        dist_q = self.dist_q
        if self._fused(time_points) and not self._kernel._needs_grad():
            with torch.no_grad():
                ve = self._site_kernel(time_points, observations, dist_q, update=False)[2]
        else:
            pair_mean, pair_cov = self._pair_marginals(dist_q)
            s_mean, s_cov = conditionals.conditional_predict(time_points, self.inducing_inputs, self._kernel, pair_mean, pair_cov)
            fmu, fvar = self._kernel.generate_emission_model(time_points).project_state_marginals_to_f(s_mean, s_cov)
            ve = self._likelihood.variational_expectations(fmu, fvar, observations)
        return torch.sum(ve) - torch.sum(dist_q.kl_divergence(self.dist_p))

    def loss(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``-classic_elbo`` (sparse_variational_cvi.py:223-230)."""
        return -self.classic_elbo(input_data)


class SparsePowerExpectationPropagation(_SparseSitesGaussianProcess):
    """GP prior, general likelihood, Gaussian posterior on the states at ``M`` inducing points with ``M + 1`` Gaussian sites
    ``t_m(v) = exp(nat1_m . v + v^T nat2_m v + log_norm_m)`` on the pairs ``v_m = [u_{m-1}, u_m]`` of neighbouring inducing states,
    updated by power expectation propagation (markovflow/models/sparse_pep.py:78-560; zero mean function, plain float likelihood
    parameters, a batch of series as leading dimensions).  The ``n_m`` data points with ``z_{m-1} < x <= z_m`` share site ``m``: each
    owns the fraction ``1 / n_m`` of it, so its cavity removes ``beta_m = alpha / n_m`` of the site from the pair marginal of ``q``,
    and it sees the cavity through the conditional ``p(f(x) | v_m)``.  ``energy`` is the (power) EP approximation of the log marginal
    likelihood.

    The site normaliser.  The reference builds ``M + 1`` leave-one-out chains and takes ``log Z(q with t_m^(1 - beta_m)) - log Z(q)``
    for every segment (sparse_pep.py:418-429).  That ratio is ``E_q[t_m(v_m)^(-beta_m)]``, an integral over the pair ``v_m`` alone:
    with the marginal ``N(m, S)`` of ``q`` on the pair and its cavity ``N(m_c, S_c)`` it equals ``exp(Gamma_m)``,
    ``Gamma_m = G(m_c, S_c) - G(m, S)``, ``G(m, S) = (log det S + m^T S^-1 m) / 2`` - the ``2d``-dimensional form of the dense model's
    ``G(mu_c, v_c) - G(m, s)`` - so it comes from the two factorisations the cavity needs anyway, and segment ``m`` adds
    ``n_m Gamma_m`` to its summed log expected density.

    Deviations from the reference:
      * the power is the integral's, as in ``PowerExpectationPropagation``: the local objective and its derivatives are those of
        ``log int p^alpha q``; the reference calls the gradients with ``alpha = 1`` and multiplies the summed step by ``alpha``
        (sparse_pep.py:338, 374).  The two agree at ``alpha = 1``;
      * the sites start at zero (the reference starts ``nat2`` at ``-1e-10 I``);
      * a segment with an undefined update - a cavity precision that is not positive definite, a point whose ``fvar`` or
        ``1 + fvar g2`` is not positive, a non-finite sum - is SKIPPED: its three site tensors stay as they are;
      * the site normaliser is the local integral above, not ``M + 1`` chains; ``log_norm`` is a blended site tensor updated in the
        same call as ``nat1`` / ``nat2`` (from the ``q`` before the step, as the dense model's), and ``compute_log_norm`` returns the
        per-segment sums WITHOUT the reference's division by ``alpha``, which ``energy`` applies."""

    def __init__(self, kernel: SDEKernel, inducing_points: torch.Tensor, likelihood: Likelihood, learning_rate: float = 1.0,
                 alpha: float = 1.0) -> None:
        """
        :param inducing_points: ``batch + [num_inducing]``, sorted.
        :param likelihood: a ``markovflow_amd.likelihoods.Likelihood``.
        :param learning_rate: the damping of ``update_sites``, in [0, 1].
        :param alpha: the power, in (0, 1].
        """
        super().__init__(kernel, inducing_points, likelihood, learning_rate)
        if not 0.0 < float(alpha) <= 1.0:
            raise ValueError(f"alpha must lie in (0, 1], got {alpha}")
        self.alpha = float(alpha)
        self.log_norm = torch.zeros(self.nat1.shape[:-1], dtype=inducing_points.dtype, device=inducing_points.device)

    def _compute_projections(self, time_points: torch.Tensor):
        """``sparse_site_projections`` of the data and, on the device, the tile table of the kernel pair."""
        w, c, indices, offsets = sparse_site_projections(self._kernel, time_points, self.inducing_inputs)
        tiles = sparse_expectation_tiles(offsets) if time_points.is_cuda else None
        return w, c, indices, offsets, tiles

    def _data(self, input_data, what: str):
        """The checked data, sorted in every series, with its cached projections."""
        time_points, observations = self._check_data(input_data, what)
        return time_points, observations, self._projections(time_points)

    # ---- the cavity --------------------------------------------------------------------------------------------------------------
    def compute_num_data_per_interval(self, time_points: torch.Tensor) -> torch.Tensor:
        """The number ``n_m`` of data points in every segment, ``batch + [M + 1]`` (sparse_pep.py:450-462)."""
        offsets = self._projections(time_points)[3]
        return (offsets[..., 1:] - offsets[..., :-1]).to(self.inducing_inputs.dtype)

    def fraction_sites(self, time_points: torch.Tensor) -> torch.Tensor:
        """``1 / n_m`` per segment, 0 for an empty one, ``batch + [M + 1]`` (sparse_pep.py:176-195)."""
        counts = self.compute_num_data_per_interval(time_points)
        return torch.where(counts > 0, 1.0 / counts.clamp(min=1.0), torch.zeros_like(counts))

    def _cavity(self, time_points: torch.Tensor, dist_q: StateSpaceModel):
        """``(cav_mean, cav_cov, seg_const)``: the pair cavity of every segment with ``beta_m = alpha / n_m`` and ``n_m Gamma_m``."""
        counts = self.compute_num_data_per_interval(time_points)
        pair_mean, pair_cov = self._pair_marginals(dist_q)
        cav_mean, cav_cov, gamma = pair_cavity(pair_mean, pair_cov, self.nat1, self.nat2, self.alpha * self.fraction_sites(time_points))
        return cav_mean, cav_cov, torch.where(counts > 0, counts * gamma, torch.zeros_like(gamma))

    def compute_cavity_state_pairs(self, time_points: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The cavity of every pair, ``(batch + [M + 1, 2d], batch + [M + 1, 2d, 2d])``: the marginal of
        ``q(s) / t_m(v_m)^(alpha / n_m)`` on ``v_m`` (sparse_pep.py:251-285, before the projection to the data); NaN where the cavity
        precision is not positive definite.  The segment counts are those of ``time_points``."""
        with torch.no_grad():
            return self._cavity(time_points, self.dist_q)[:2]

    def compute_cavity(self, time_points: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The cavity marginals of ``f`` at the data, ``batch + [N, 1]`` each (sparse_pep.py:304-314)."""
        with torch.no_grad():
            w, c, indices = self._projections(time_points)[:3]
            cav_mean, cav_cov, _ = self._cavity(time_points, self.dist_q)
            fmu, fvar, _ = _sparse_point_marginals(w, c, indices, cav_mean, cav_cov, cav_mean.shape[-2])
            return fmu[..., None], fvar[..., None]

    # ---- inference ---------------------------------------------------------------------------------------------------------------
    def local_objective(self, Fmu: torch.Tensor, Fvar: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        """``log E_{N(f | Fmu, Fvar)} p(y | f)^alpha``, ``[..., 1] -> [...]`` (sparse_pep.py:164-166)."""
        return self._likelihood.log_expected_density(Fmu, Fvar, Y, alpha=self.alpha)

    def local_objective_gradients(self, Fmu: torch.Tensor, Fvar: torch.Tensor, Y: torch.Tensor
                                  ) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        """The local objective, ``[...]``, and the corrected gradients ``(L1, L2)``, ``[..., 1]`` each (sparse_pep.py:168-174; the
        power is the model's, class docstring)."""
        obj, grads = self._likelihood.grad_log_expected_density(Fmu, Fvar, Y, alpha=self.alpha)
        return obj, gradient_correction((Fmu, Fvar), grads)

    def _site_step(self, input_data, what: str, update: bool) -> torch.Tensor:
        """``dist_q``, its pair marginals, the batched cavity and ONE call of ``mf_lik_sparse_pep_site_update_*`` (``2d <= 18`` on the
        device; otherwise ``sparse_pep_site_update_torch``): the in-place step, or (``update`` False) the evaluation-only mode.
        Returns the per-segment ``sum I + n Gamma``, ``batch + [M + 1]`` (evaluation only)."""
        time_points, observations, (w, c, indices, offsets, tiles) = self._data(input_data, what)
        with torch.no_grad():
            cav_mean, cav_cov, seg_const = self._cavity(time_points, self.dist_q)
            sites = (self.nat1, self.nat2, self.log_norm) if update else (None, None, None)
            if self._fused(time_points):
                led_sum = sparse_pep_site_update_hip(self._likelihood, w, c, observations[..., 0], offsets, cav_mean, cav_cov, self.alpha,
                                                     self.learning_rate, *sites, seg_const=seg_const, tiles=tiles,
                                                     want_led_sum=not update)[0]
            else:
                led_sum = sparse_pep_site_update_torch(self._likelihood, w, c, observations[..., 0], indices, cav_mean, cav_cov,
                                                       self.alpha, self.learning_rate, *sites, seg_const=seg_const)[0]
            return None if update else led_sum + seg_const

    def update_sites(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> None:
        """One power-EP step on the sites, in place (sparse_pep.py:316-380, 473-487): ``dist_q``, its pair marginals, the batched
        pair cavity and ONE call of ``mf_lik_sparse_pep_site_update_*`` on HIP tensors with ``2d <= 18``
        (``sparse_pep_site_update_torch`` for ``2d > 18``)."""
        self._site_step(input_data, "update_sites", update=True)

    def compute_log_norm(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """The site normalisers from the current ``q``, per segment, ``batch + [M + 1]``: ``sum_k I_k + n_m Gamma_m`` with the
        objective at the cavity (sparse_pep.py:382-448, class docstring); NaN for a segment whose update is undefined."""
        return self._site_step(input_data, "compute_log_norm", update=False)

    def energy(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """The power-EP energy per series, ``batch`` (sparse_pep.py:489-495): ``dist_q.normalizer() - dist_p.normalizer()
        + (1 / alpha) sum_m log_norm_m`` with the normalisers computed afresh from the current ``q``.  Not differentiable."""
        with torch.no_grad():
            log_norm = torch.sum(self.compute_log_norm(input_data), dim=-1)
            return self.dist_q.normalizer() - self.dist_p.normalizer() + log_norm / self.alpha

    def classic_elbo(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``sum_i E_q log p(y_i | f_i) - KL[q(u) || p(u)]`` (sparse_pep.py:520-542; for testing, not for optimisation)."""
        time_points, observations = self._check_data(input_data, "classic_elbo")
        dist_q = self.dist_q
        fmu, fvar = self.posterior.predict_f(time_points)
        ve = self._likelihood.variational_expectations(fmu, fvar, observations)
        return torch.sum(ve) - torch.sum(dist_q.kl_divergence(self.dist_p))

    def loss(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``-classic_elbo`` (sparse_pep.py:497-504)."""
        return -self.classic_elbo(input_data)


def _sorted_series(time_points: torch.Tensor) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """``(order, sorted time points)``: the stable permutation that sorts every series, or ``(None, time_points)`` for sorted data."""
    if not bool((time_points[..., 1:] < time_points[..., :-1]).any()):
        return None, time_points
    order = torch.argsort(time_points, dim=-1, stable=True)
    return order, torch.gather(time_points, -1, order)


class SparseVariationalGaussianProcess(_SparseGaussianProcess):
    """GP prior, general likelihood, a free-form Gaussian posterior ``q(s(z))`` on the states at ``M`` inducing points held as a
    trainable ``StateSpaceModel`` (markovflow/models/sparse_variational.py:31-270; zero mean function, plain float likelihood
    parameters, a batch of series as leading dimensions).  The ELBO is ``scale sum_i E_q log p(y_i | f_i) - KL[q(s(z)) || p(s(z))]``;
    ``q`` is trained with any torch optimiser on ``trainable_variables`` or with ``ssm_natgrad.SSMNaturalGradient`` on ``dist_q``.

    A likelihood with ``L = latent_dim > 1`` latent functions (``MultiStageLikelihood``) takes a kernel with ``output_dim = L``
    (``IndependentMultiOutput``): the observations stay ``batch + [N, 1]``, every point is projected once per latent
    (``sparse_multi_site_projections``), the data term is ONE call of ``mf_lik_sparse_multi_expectations_*`` and ``predict_f`` returns
    ``batch + [num_new, L]``.

    A likelihood with ONE latent function on a kernel with ``P > 1`` outputs also takes observations ``batch + [N, P]``, one series
    per output, the likelihood applied to each.  With a ``FactorAnalysisKernel`` (``f = A(t) B g``, ``L`` latents) the projections of
    the pair onto the latents are cached (``sparse_factor_site_projections``; they do not depend on ``B``), the mixing weights
    ``kernel.mixing_weights`` are evaluated on every ``elbo`` call under the tape, and the data term with its adjoints onto the pair
    marginals AND the mixing weights is ONE call of ``mf_lik_sparse_factor_expectations_*`` (HIP tensors, ``L`` in 2, 3, 4,
    ``2L <= 2d <= 18``, no hyper-parameter of the chain under the tape; otherwise ``sparse_factor_expected_log_likelihood_torch``):
    the loading matrix trains on the fused path.  Any other multi-output kernel takes
    ``sparse_multi_output_expected_log_likelihood_torch``.  Observations ``batch + [N, 1]`` keep the single-output path whatever the
    kernel (a weight function's own parameters are seen on the ``[N, P]`` routes only).

    An ``IndependentMultiOutputStack`` of ``K`` kernels keeps ``K`` independent chains of dimension ``d = max d_k`` with ``K`` as the
    last batch dimension: inducing points ``lead + [K, M]``, time points ``lead + [K, N]``, ``dist_q`` / ``dist_p`` / the KL /
    ``SSMNaturalGradient`` on batch ``lead + [K]``, ``predict_f`` ``lead + [num_new, K]``.  Observations ``lead + [N, 1]`` under a
    ``K``-latent likelihood couple the chains at every point: the data term is ONE call of ``mf_lik_stack_expectations_*`` when the
    tensors are HIP tensors, ``2d <= 18``, the likelihood is instantiated (``MultiStageLikelihood``, ``HeteroscedasticGaussian``), no
    kernel hyper-parameter is under the tape and the chains of every series share their inducing points and data times;
    otherwise ``sparse_stack_expected_log_likelihood_torch``.  Observations ``lead + [N, K]`` under a one-latent likelihood are
    ``K`` decoupled problems: ``mf_lik_sparse_expectations_*`` on the batch of chains, per-output inducing points allowed."""

    _multi_latent = True
    _multi_output = True

    def __init__(self, kernel: SDEKernel, likelihood: Likelihood, inducing_points: torch.Tensor, num_data: Optional[int] = None,
                 initial_distribution: Optional[StateSpaceModel] = None) -> None:
        """
        :param inducing_points: ``batch + [num_inducing]``, sorted, at least two (a ``StateSpaceModel`` needs a transition).
        :param num_data: the total number of observations per series when ``elbo`` is fed minibatches.
        :param initial_distribution: the initial ``q`` on the inducing points; the prior by default.
        """
        super().__init__(kernel, likelihood, inducing_points, min_inducing=2)
        self._route = "multi" if likelihood.latent_dim > 1 else "single"    # (``_data_route`` of the data last seen)
        if isinstance(kernel, StackKernel):
            self._route = "stack" if likelihood.latent_dim > 1 else "stack_outputs"
        if num_data is not None and not num_data > 0:
            raise ValueError(f"num_data must be positive, got {num_data}")
        self.num_data = num_data
        if initial_distribution is None:
            initial_distribution = kernel.state_space_model(inducing_points)
        elif not isinstance(initial_distribution, StateSpaceModel):
            raise TypeError("initial_distribution must be a StateSpaceModel")
        if (tuple(initial_distribution.batch_shape) != tuple(inducing_points.shape[:-1])
                or initial_distribution.num_transitions + 1 != inducing_points.shape[-1]
                or initial_distribution.state_dim != kernel.state_dim):
            raise ValueError("initial_distribution must be a chain on the inducing points: batch shape "
                             f"{tuple(inducing_points.shape[:-1])}, {inducing_points.shape[-1]} states of dimension {kernel.state_dim}")
        self._dist_q = initial_distribution.create_trainable_copy()
        self._posterior = ConditionalProcess(posterior_dist=self._dist_q, kernel=kernel, conditioning_time_points=inducing_points)

    @property
    def time_points(self) -> torch.Tensor:
        """The inducing points (sparse_variational.py:194-202)."""
        return self.inducing_inputs

    @property
    def dist_p(self) -> StateSpaceModel:
        """The prior chain on the inducing points, rebuilt on every access (sparse_variational.py:225-230)."""
        return self._kernel.state_space_model(self.inducing_inputs)

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

    # ---- data --------------------------------------------------------------------------------------------------------------------
    @property
    def _multi(self) -> bool:
        """A likelihood with several latent functions: the multi-latent projections and data term."""
        return self._likelihood.latent_dim > 1

    def _data_route(self, observations: torch.Tensor) -> str:
        """What the observations' last dimension selects: ``"single"`` (``[N, 1]``, one latent), ``"multi"`` (``[N, 1]``, a
        multi-latent likelihood), ``"factor"`` (``[N, P]`` on a ``FactorAnalysisKernel``) or ``"outputs"`` (``[N, P]`` on any other
        kernel with ``P`` outputs)."""
        if isinstance(self._kernel, StackKernel):
            return "stack" if self._multi else "stack_outputs"
        if observations.shape[-1] == 1:
            return "multi" if self._multi else "single"
        return "factor" if isinstance(self._kernel, FactorAnalysisKernel) else "outputs"

    def _emission_needs_grad(self) -> bool:
        """A hyper-parameter of the emission under the tape (the loading matrix of a ``FactorAnalysisKernel``)."""
        return torch.is_grad_enabled() and any(x.requires_grad for x in super()._emission_sources())

    def _emission_sources(self) -> Tuple[torch.Tensor, ...]:
        # (the projections onto the latents of a FactorAnalysisKernel do not depend on its loading matrix: a step on it keeps them)
        return () if self._route == "factor" else super()._emission_sources()

    def _fused(self, time_points: torch.Tensor) -> bool:
        two_d = 2 * self._kernel.state_dim
        if not (time_points.is_cuda and two_d <= SPARSE_SITE_MAX_TWO_D and not self._kernel._needs_grad()):
            return False
        if self._route == "factor":
            latents = self._kernel.latent_dim
            return latents in SPARSE_FACTOR_LATENTS and two_d >= 2 * latents and self._kernel.output_dim <= SPARSE_FACTOR_MAX_OUTPUTS
        if self._route == "outputs":           # (no fused multi-output term for a kernel that is not a FactorAnalysisKernel)
            return False
        if self._route == "single":            # the loading matrix under the tape: w and c are part of the graph
            return not self._emission_needs_grad()
        return two_d >= SPARSE_MULTI_MIN_TWO_D

    def _compute_projections(self, time_points: torch.Tensor):
        """``(order | None, w, c, indices, offsets, tiles)`` of the data: the permutation that sorts each series (None for sorted
        data), ``sparse_site_projections`` of the sorted points (``sparse_multi_site_projections`` for a multi-latent likelihood or
        multi-output observations: ``w`` and ``c`` carry one row per latent or output; ``sparse_factor_site_projections`` for a
        ``FactorAnalysisKernel`` with multi-output observations: ``wg``, ``cg`` of the latents) and the tile table."""
        if self._route in ("stack", "stack_outputs"):
            return self._compute_stack_projections(time_points)
        order, time_points = _sorted_series(time_points)
        project = {"single": sparse_site_projections, "multi": sparse_multi_site_projections,
                   "outputs": sparse_multi_site_projections, "factor": sparse_factor_site_projections}[self._route]
        w, c, indices, offsets = project(self._kernel, time_points, self.inducing_inputs)
        tiles = sparse_expectation_tiles(offsets) if time_points.is_cuda else None
        return order, w, c, indices, offsets, tiles

    def _compute_stack_projections(self, time_points: torch.Tensor):
        """``(order | None, w, c, indices, offsets, tiles, shared)`` of data ``lead + [K, N]`` on a stack kernel:
        ``sparse_site_projections`` on the stacked batch (every chain sorted on its own time points), ``w [.., K, N, 2d]``,
        ``c [.., K, N]``.  ``shared``: the ``K`` chains of every series have equal inducing points, equal data times and one sorting
        permutation, so they share ONE segmentation (one read-back, kept with the projections) - the coupled route's tile table is
        then that of chain 0's offsets; the per-output route's is that of the batch of chains."""
        order, x = _sorted_series(time_points)
        w, c, indices, offsets = sparse_site_projections(self._kernel, x, self.inducing_inputs)
        shared, tiles = False, None
        if self._route == "stack":
            z = self.inducing_inputs
            same = (z == z[..., :1, :]).all() & (x == x[..., :1, :]).all()
            if order is not None:
                same = same & (order == order[..., :1, :]).all()
            shared = bool(same)
            if shared and time_points.is_cuda:
                tiles = sparse_expectation_tiles(offsets[..., 0, :].contiguous())
        elif time_points.is_cuda:
            tiles = sparse_expectation_tiles(offsets)
        return order, w, c, indices, offsets, tiles, shared

    def _stack_expected_log_likelihood(self, time_points: torch.Tensor, observations: torch.Tensor, pair_mean, pair_cov
                                       ) -> torch.Tensor:
        """The data term on a stack kernel, ``lead + [M + 1]`` (coupled) or ``lead + [K, M + 1]`` (one series per output)."""
        kernel, lik = self._kernel, self._likelihood
        two_d = 2 * kernel.state_dim
        on_device = time_points.is_cuda and two_d <= SPARSE_SITE_MAX_TWO_D and not kernel._needs_grad()
        if kernel._needs_grad():
            # a hyper-parameter under the tape: w and c are part of the graph
            order, x = _sorted_series(time_points)
            proj, cov, indices = conditionals._conditional_statistics(x, self.inducing_inputs, kernel)
            h = kernel.generate_emission_model(x).emission_matrix
            w, c = (h @ proj)[..., 0, :], (h @ cov @ h.transpose(-1, -2))[..., 0, 0]
            offsets = tiles = None
            shared = False
        else:
            order, w, c, indices, offsets, tiles, shared = self._projections(time_points)
        if self._route == "stack_outputs":
            # K decoupled chains: the single-latent term on the batch lead + [K]
            y = observations.transpose(-1, -2)
            if order is not None:
                y = torch.gather(y, -1, order)
            if on_device:
                return sparse_expected_log_likelihood(lik, w, c, y.contiguous(), offsets, pair_mean, pair_cov, tiles=tiles)
            return sparse_expected_log_likelihood_torch(lik, w, c, y, indices, pair_mean, pair_cov)
        y = observations[..., 0]
        if on_device and shared and sparse_stack_instantiated(lik, kernel.num_kernels, two_d):
            if order is not None:
                y = torch.gather(y, -1, order[..., 0, :])
            return sparse_stack_expected_log_likelihood(lik, w, c, y, offsets[..., 0, :].contiguous(), pair_mean, pair_cov, tiles=tiles)
        return sparse_stack_expected_log_likelihood_torch(lik, w, c, y, indices, pair_mean, pair_cov, orders=order)

    def _multi_output_expected_log_likelihood(self, time_points: torch.Tensor, observations: torch.Tensor, pair_mean, pair_cov
                                              ) -> torch.Tensor:
        """The data term for observations ``batch + [N, P]``, ``P`` the kernel's output dimension."""
        kernel, factor = self._kernel, self._route == "factor"
        fused = self._fused(time_points)
        if not fused and kernel._needs_grad():
            # a hyper-parameter of the chain under the tape: the projections are part of the graph
            order, x = _sorted_series(time_points)
            proj, cov, indices = conditionals._conditional_statistics(x, self.inducing_inputs, kernel)
            h = (kernel.latent_emission_model(x) if factor else kernel.generate_emission_model(x)).emission_matrix
            w, c = h @ proj, (h @ cov @ h.transpose(-1, -2) if factor else torch.sum((h @ cov) * h, dim=-1))
        else:
            order, w, c, indices, offsets, tiles = self._projections(time_points)
            x = time_points if order is None else torch.gather(time_points, -1, order)
        y = observations
        if order is not None:
            y = torch.gather(y, -2, order[..., None].expand(y.shape))
        if not factor:
            return sparse_multi_output_expected_log_likelihood_torch(self._likelihood, w, c, y, indices, pair_mean, pair_cov)
        mix = kernel.mixing_weights(x)             # on every call, under the tape of the loading matrix and the weight function
        if fused:
            return sparse_factor_expected_log_likelihood(self._likelihood, w, c, mix, y, offsets, pair_mean, pair_cov, tiles=tiles)
        return sparse_factor_expected_log_likelihood_torch(self._likelihood, w, c, mix, y, indices, pair_mean, pair_cov)

    def _pair_marginals(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(m_pair [.., M+1, 2d], S_pair [.., M+1, 2d, 2d])`` of ``dist_q`` - under the tape when its leaves require a gradient -
        with the stationary prior beyond both ends."""
        return conditionals.pairwise_marginals(self._dist_q, *self._stationary_prior())

    def _expected_log_likelihood(self, time_points: torch.Tensor, observations: torch.Tensor) -> torch.Tensor:
        """``sum_i E_q log p(y_i | f_i)`` per pair, ``batch + [M + 1]``."""
        pair_mean, pair_cov = self._pair_marginals()
        multi = self._multi
        route = self._data_route(observations)
        if route != self._route:                   # the cached projections are the other route's
            self._route, self._projection_cache = route, None
        if route in ("stack", "stack_outputs"):
            return self._stack_expected_log_likelihood(time_points, observations, pair_mean, pair_cov)
        if route in ("factor", "outputs"):
            return self._multi_output_expected_log_likelihood(time_points, observations, pair_mean, pair_cov)
        if self._fused(time_points):
            order, w, c, _, offsets, tiles = self._projections(time_points)
            y = observations[..., 0]
            if order is not None:
                y = torch.gather(y, -1, order)
            fused = sparse_multi_expected_log_likelihood if multi else sparse_expected_log_likelihood
            return fused(self._likelihood, w, c, y, offsets, pair_mean, pair_cov, tiles=tiles)
        if self._kernel._needs_grad() or self._emission_needs_grad():
            # a hyper-parameter under the tape: w and c are part of the graph
            order, time_points = _sorted_series(time_points)
            proj, cov, indices = conditionals._conditional_statistics(time_points, self.inducing_inputs, self._kernel)
            h = self._kernel.generate_emission_model(time_points).emission_matrix
            if multi:
                w, c = h @ proj, torch.sum((h @ cov) * h, dim=-1)
            else:
                w, c = (h @ proj)[..., 0, :], (h @ cov @ h.transpose(-1, -2))[..., 0, 0]
        else:
            order, w, c, indices, _, _ = self._projections(time_points)
        y = observations[..., 0]
        if order is not None:
            y = torch.gather(y, -1, order)
        composed = sparse_multi_expected_log_likelihood_torch if multi else sparse_expected_log_likelihood_torch
        return composed(self._likelihood, w, c, y, indices, pair_mean, pair_cov)

    # ---- inference ---------------------------------------------------------------------------------------------------------------
    def elbo(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``scale sum_i E_q log p(y_i | f_i) - KL[q(s(z)) || p(s(z))]``, summed over the batch; ``scale = num_data / minibatch size``
        when ``num_data`` is set (sparse_variational.py:149-192).  The data need not be sorted: a minibatch is a random subset; each
        series is sorted on a copy (a stable argsort, cached with the projections), so the ELBO of shuffled data has the bits of the
        sorted data's.  HIP tensors with ``2d <= 18`` and no kernel hyper-parameter under the tape: the pair marginals of ``dist_q``
        under the tape, ONE call of ``mf_lik_sparse_expectations_*`` whose adjoints the backward reuses, and the KL adjoints;
        otherwise ``sparse_expected_log_likelihood_torch``."""
        time_points, observations = self._check_data(input_data, "elbo")
        ve = torch.sum(self._expected_log_likelihood(time_points, observations))
        kl = torch.sum(self._dist_q.kl_divergence(self.dist_p))
        if self.num_data is not None:
            ve = ve * (float(self.num_data) / time_points.shape[-1])
        return ve - kl

    def loss(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``-elbo`` (sparse_variational.py:250-260)."""
        return -self.elbo(input_data)

    def predict_f(self, new_time_points: torch.Tensor, full_output_cov: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """Posterior mean and variance of ``f`` at ``new_time_points`` (sorted), ``batch + [num_new, L]`` each, ``L`` the kernel's
        output dimension (1 unless the likelihood is a multi-latent one or the kernel has several outputs).  The latent processes
        of a ``FactorAnalysisKernel``: ``posterior.predict_state`` and
        ``kernel.latent_emission_model(t).project_state_marginals_to_f``."""
        with torch.no_grad():
            return self._posterior.predict_f(new_time_points, full_output_cov)

    _predict_f = predict_f          # (``predict_log_density`` predicts outside the tape here, as ``predict_f`` does)

    def predict_log_density(self, input_data: Tuple[torch.Tensor, torch.Tensor], full_output_cov: bool = False) -> torch.Tensor:
        if isinstance(self._kernel, StackKernel):
            raise NotImplementedError("predict_log_density is not supported on a stack kernel (several latents or several outputs "
                                      "per point)")
        if input_data[1].dim() >= 1 and input_data[1].shape[-1] != 1:
            raise NotImplementedError("predict_log_density: observations with several outputs per point are not supported")
        return super().predict_log_density(input_data, full_output_cov)


class ImportanceWeightedVI(SparseVariationalGaussianProcess):
    """Importance-weighted VI (markovflow/models/iwvi.py:29-173; Domke and Sheldon 2018; zero mean function): the SVGP model with the
    bound ``L_K = log (1/K) sum_k w_k``, ``w_k = p(y | s_k) p(u_k) / q(u_k)``, ``(s_k, u_k) ~ q(u) p(s | u)``, which tightens with
    ``K`` towards ``log p(y)``.  The proposals are drawn by Matheron's rule; on HIP tensors with ``2d <= 18`` and no kernel
    hyper-parameter under the tape their assembly, the ``K`` evaluations of the likelihood at every data point and the adjoint onto
    the draw from ``q`` are ONE call of ``mf_lik_iw_log_weights_*``."""

    _multi_latent = False      # (the importance weights are written for one latent function ...
    _multi_output = False      # ... and one observed series)

    def __init__(self, kernel: SDEKernel, inducing_points: torch.Tensor, likelihood: Likelihood, num_importance_samples: int,
                 initial_distribution: Optional[StateSpaceModel] = None) -> None:
        super().__init__(kernel, likelihood, inducing_points, None, initial_distribution)
        self._posterior = ImportanceWeightedPosteriorProcess(num_importance_samples, self._dist_q, kernel, inducing_points, likelihood)
        self._merged_cache = None

    @property
    def posterior(self) -> ImportanceWeightedPosteriorProcess:
        return self._posterior

    def predict_f(self, new_time_points: torch.Tensor, full_output_cov: bool = False):
        """Not available in closed form (posterior.py:772-786): use ``posterior.expected_value`` or ``posterior.sample_f``."""
        return self._posterior.predict_f(new_time_points, full_output_cov)

    _predict_f = predict_f

    def _merged(self, projections, time_points: torch.Tensor) -> torch.Tensor:
        """``iw_merged_time_points`` of the (sorted) data, kept as long as the cached projections are."""
        cached = self._merged_cache
        if cached is not None and cached[0] is projections:
            return cached[1]
        order, offsets = projections[0], projections[4]
        with torch.no_grad():
            x = time_points if order is None else torch.gather(time_points, -1, order)
            merged = iw_merged_time_points(x, self.inducing_inputs, offsets)
        self._merged_cache = (projections, merged)
        return merged

    def log_weights(self, input_data: Tuple[torch.Tensor, torch.Tensor], stop_gradient: bool = False, what: str = "log_weights"
                    ) -> torch.Tensor:
        """``log w_k``, ``[K]``, summed over the batch - the batch is one model, as in the SVGP ``elbo``: one prior draw on the merged
        time points, one (reparameterised) draw from ``q``, the data term and ``log p(u) - log q(u)``.  Both routes make the same
        two draws in the same order."""
        time_points, observations = self._check_data(input_data, what)
        k = self._posterior.num_importance_samples
        projections = self._projections(time_points)
        order, w, _, indices, offsets, tiles = projections
        merged = self._merged(projections, time_points)
        y = observations[..., 0]
        if order is not None:
            y = torch.gather(y, -1, order)
        h = self._kernel.generate_emission_model(merged[..., :1]).emission_matrix.reshape(-1, self._kernel.state_dim)[0]
        fused = self._fused(time_points)
        if not fused and self._kernel._needs_grad():
            # a hyper-parameter under the tape: w is part of the graph
            x = time_points if order is None else torch.gather(time_points, -1, order)
            proj, _, indices = conditionals._conditional_statistics(x, self.inducing_inputs, self._kernel)
            w = (self._kernel.generate_emission_model(x).emission_matrix @ proj)[..., 0, :]
        prior = self._kernel.state_space_model(merged).sample((k,))
        u_post = self._dist_q.sample((k,))
        if fused:
            log_lik = iw_log_likelihood(self._likelihood, h, w, y, offsets, prior, u_post, tiles=tiles)
        else:
            log_lik = iw_log_likelihood_torch(self._likelihood, h, w, y, indices, prior, u_post)
        log_w = log_lik + self._posterior._log_density_ratio(u_post, stop_gradient)
        return torch.sum(log_w.reshape(k, -1), dim=-1)

    def elbo(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``logsumexp_k(log w_k) - log K`` (iwvi.py:109-141): a stochastic lower bound of ``log p(y)``, tighter than the SVGP ELBO for
        ``K > 1``.  The data need not be sorted (a stable argsort on a copy, cached with the projections)."""
        log_w = self.log_weights(input_data, False, "elbo")
        return torch.logsumexp(log_w, dim=0) - math.log(log_w.shape[0])

    def dregs_objective(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """A scalar whose gradient is the doubly-reparameterised (DReG) estimator (iwvi.py:143-173): ``sum_k stop_grad(softmax(log w))_k^2
        log w_k`` with ``q`` stopped inside ``log q(u)`` only - for the variational parameters; ``elbo`` for the hyper-parameters."""
        log_w = self.log_weights(input_data, True, "dregs_objective")
        return torch.sum(torch.square(torch.softmax(log_w, dim=0).detach()) * log_w)
