"""
Thin model harness over the Kalman path: ``GaussianProcessRegression`` (mirror of
``markovflow/models/gaussian_process_regression.py:29-160``, the direct caller of ``KalmanFilter`` in the reference).
Only what drives the hot path is mirrored: construction from ``(time_points, observations)`` and an SDE kernel,
``log_likelihood`` / ``loss``, the posterior state space model and ``posterior`` (prediction at new time points,
``markovflow_amd/posterior.py``); mean functions and training loops belong to the reference's outer layers.

``CVIGaussianProcess`` (mirror of ``markovflow/models/variational_cvi.py:32-460``: ``GaussianProcessWithSitesBase`` +
``CVIGaussianProcess`` with a zero mean function) is the site-based model for non-Gaussian likelihoods
(``markovflow_amd/likelihoods.py``): its ``update_sites`` is the filter route's posterior chain followed by ONE launch of
``mf_lik_cvi_site_update_*``.

``PowerExpectationPropagation`` (mirror of ``markovflow/models/pep.py:28-261``, zero mean function) shares the sites, ``dist_q`` and
the sites filter with it; its ``update_sites`` is the same posterior chain followed by ONE launch of ``mf_lik_pep_site_update_*``
(cavity, log expected density with two derivatives, gradient correction, site normaliser, power / damping step), and ``energy()`` is
the EP approximation of the log marginal likelihood.

``SparseCVIGaussianProcess`` (mirror of ``markovflow/models/sparse_variational_cvi.py:38-313``, zero mean function) carries
``M + 1`` multivariate sites on the pairs of neighbouring inducing states instead of one site per data point: the chain has ``M``
blocks, and the ``N`` data points enter ``update_sites`` through ONE launch of ``mf_lik_sparse_cvi_site_update_*`` (projection onto
the bracketing pair, expectations, back-projection and the segmented sum).

``SparseVariationalGaussianProcess`` (mirror of ``markovflow/models/sparse_variational.py:31-270``, zero mean function) holds ``q`` on
the inducing points as a trainable ``StateSpaceModel``; the data term of its ELBO and the adjoint onto the pair marginals of ``q`` are
ONE call of ``mf_lik_sparse_expectations_*`` (two passes, tile-parallel), the KL term is ``StateSpaceModel.kl_divergence``.

``ImportanceWeightedVI`` (mirror of ``markovflow/models/iwvi.py:29-173``, zero mean function) subclasses it: ``K`` proposals drawn by
Matheron's rule, whose assembly from one prior draw, the ``K`` evaluations of ``log p(y_n | f_n)`` at every data point and the adjoint
onto the draw from ``q`` are ONE call of ``mf_lik_iw_log_weights_*`` (two passes, tile-parallel, no atomics).

``VariationalGaussianProcess`` (mirror of ``markovflow/models/variational.py:30-223``, zero mean function) is the reference's basic
model: ``q`` is a trainable ``StateSpaceModel`` on the states at the data points themselves.  The data term of its ELBO is ONE call
of ``mf_lik_dense_expectations_*`` on the marginals of ``q`` (two passes over tiles of 64 points, two derivatives per point kept), its
adjoint onto those marginals ONE call of ``mf_lik_dense_expectations_adjoint_*``; the KL term is ``StateSpaceModel.kl_divergence``.

``SpatioTemporalSparseVariational`` (mirror of ``markovflow/models/spatio_temporal_variational.py:109-357``, zero mean function) is
the SVGP model for a product kernel ``k_s(x, x') k_t(t, t')``: ``q`` is a trainable chain of state dimension ``Ms d_t <= 64`` on the
inducing times.  The data term of its ELBO, the adjoints onto the pair marginals of ``q`` and the per-point adjoints onto the
spatial weights and temporal projections are ONE call of ``mf_lik_st_expectations_*`` (csrc/mf_st.hip).
"""
from typing import Optional, Tuple

import ctypes
import math

import torch

from . import _lib, conditionals
from .emission_model import EmissionModel
from .kalman_filter import KalmanFilter, KalmanFilterWithSites, UnivariateGaussianSitesNat
from .kernels import (ST_MAX_STATE_DIM, IndependentMultiOutput, NonStationaryKernel, SDEKernel, SparseSpatioTemporalKernel,
                      _MaternBase, _version_key)
from .likelihoods import Gaussian, Likelihood, torch_log_expected_density
from .posterior import AnalyticPosteriorProcess, ConditionalProcess, ImportanceWeightedPosteriorProcess
from .ssm_gaussian_transformations import naturals_to_ssm_params
from .state_space_model import StateSpaceModel


def _refuse_non_stationary(kernel, who: str) -> None:
    """Every model but ``GaussianProcessRegression`` takes stationary kernels only: the sparse and site-based models put the
    stationary prior (``_stationary_prior``) at both ends of their chains, which is only right for a stationary kernel."""
    if isinstance(kernel, NonStationaryKernel):
        raise NotImplementedError(f"{who} supports stationary kernels only: a non-stationary kernel ({type(kernel).__name__}) is "
                                  "supported by GaussianProcessRegression alone")


def _all_matern(comps) -> bool:
    """True when every component is a plain Matérn kernel - what the fused ``mf_gpr_matern_*`` kernels generate.  A component of
    order 0 or with an oscillator (``Constant``, ``HarmonicOscillator``, ``Product``) takes the materialised route."""
    return all(isinstance(c, _MaternBase) for c in comps)


def _gpr_partition(bsz: int, nt: int, chunks: int, lanes: int = 65536):
    """``(chunks to ask for, chunks per series P, transitions per chunk L)`` of the fused GPR forward - THE one place the Python
    side derives it (forward, backward and posterior chain all start from the same summaries).  Mirrors
    ``lds_partition()`` of csrc/mf_inst.hip for an EXPLICIT chunk count, which is what every caller passes down; the C side
    re-checks that ``(P, L)`` tile the ``nt`` transitions and refuses (-101) otherwise."""
    want = chunks if chunks > 0 else max(1, min(-(-lanes // max(bsz, 1)), max(nt // 4, 1)))
    want = max(1, min(want, nt))
    length = -(-nt // want)
    return want, -(-nt // length), length


class _GprFusedLogLik(torch.autograd.Function):
    """Per-series log-likelihood of GP regression (without the chain-independent constants) as a differentiable function of the
    stacked hyper-parameters ``lam`` (= sqrt(order) / lengthscale), ``var`` and the noise precision, with the kernel -> state space
    model step fused into BOTH directions: forward ``mf_gpr_matern_loglik_*`` on an explicit time partition (its chunk summaries
    stay in the workspace), backward ``mf_gpr_matern_loglik_grad_*`` (csrc/mf_gpr_grad.hpp: boundary scans on those summaries, an
    emit pass and a gradient pass that generate the transitions in registers) followed by the generator's backward
    (``mf_sde_matern_transitions_grad_packed_*``, and ``mf_sde_matern_prior_chol_grad_*`` for the stationary prior's factor, which
    the kernels generate themselves), which reduces the gradients of the transitions to the hyper-parameters.  Reference: TensorFlow reverse mode through
    models/gaussian_process_regression.py:150-160, kernels/matern.py, sde_kernel.py:421-446."""

    @staticmethod
    def forward(ctx, lam_t, var_t, rinv, t, y, orders, per_series, jitter, chunks):
        bsz, n = t.shape
        d = sum((o + 1) // 2 for o in orders)
        nt = n - 1
        lib = _lib.load()
        want, parts, length = _gpr_partition(bsz, nt, chunks)
        ws_bytes = int(lib.mf_kf_loglik_workspace_bytes(bsz, n, d, t.element_size(), want))
        ws = _lib.workspace(ws_bytes, t.device)
        out = torch.empty(bsz, dtype=t.dtype, device=t.device)
        info = _lib.pivot_info(t.device)
        c_orders = (ctypes.c_int * len(orders))(*orders)
        lam_c, var_c, rinv_c = lam_t.detach().contiguous(), var_t.detach().contiguous(), rinv.detach().contiguous()
        rc = _lib.call_rc("mf_gpr_matern_loglik", t.dtype, bsz, n, len(orders), c_orders, _lib.ptr(lam_c), _lib.ptr(var_c),
                          int(per_series), _lib.ptr(t), _lib.ptr(y), _lib.ptr(rinv_c), jitter, 0.0, _lib.ptr(out), _lib.ptr(ws),
                          ws_bytes, info, want, None, None, _lib.stream_ptr(t.device))
        _lib.check(rc, "mf_gpr_matern_loglik")
        _lib.raise_on_info(info, "GaussianProcessRegression.log_likelihood", t.device)
        ctx.save_for_backward(lam_c, var_c, rinv_c, t, y)
        ctx.meta = (orders, per_series, jitter, d)
        ctx.fwd = (ws, parts, length)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lam_c, var_c, rinv_c, t, y = ctx.saved_tensors
        orders, per_series, jitter, d = ctx.meta
        # (the summaries are only READ by the backward kernels and live as long as the graph node: a second backward through the
        # same node - retain_graph=True, per-parameter gradient loops - starts from them again)
        ws_f, parts, length = ctx.fwd
        bsz, n = t.shape
        lib = _lib.load()
        c_orders = (ctypes.c_int * len(orders))(*orders)
        with torch.no_grad():
            # one packed record per transition: the diagonal blocks of g_A | the lower triangles of those of g_cholQ (16-B padded parts)
            esz = t.element_size()
            sizes = [(o + 1) // 2 for o in orders]
            pad = lambda nel: -(-nel * esz // 16) * 16 // esz                                         # noqa: E731
            rec = pad(sum(k * k for k in sizes)) + pad(sum(k * (k + 1) // 2 for k in sizes))
            g_packed = torch.empty((bsz, n - 1, rec), dtype=t.dtype, device=t.device)
            g_cp0 = torch.empty((bsz, d, d), dtype=t.dtype, device=t.device)
            g_om = torch.empty((bsz, n), dtype=t.dtype, device=t.device)
            ws_bytes = int(lib.mf_gpr_matern_loglik_grad_workspace_bytes(bsz, n, d, t.element_size(), parts))
            ws = _lib.workspace(ws_bytes, t.device)
            info = _lib.pivot_info(t.device)
            w = grad_out.reshape(bsz).contiguous()
            rc = _lib.call_rc("mf_gpr_matern_loglik_grad", t.dtype, bsz, n, len(orders), c_orders, _lib.ptr(lam_c), _lib.ptr(var_c),
                              int(per_series), _lib.ptr(t), _lib.ptr(y), _lib.ptr(rinv_c), jitter, _lib.ptr(w), _lib.ptr(g_packed),
                              _lib.ptr(g_cp0), _lib.ptr(g_om), _lib.ptr(ws), ws_bytes, info, _lib.ptr(ws_f), parts, length,
                              _lib.stream_ptr(t.device))
            _lib.check(rc, "mf_gpr_matern_loglik_grad")
            _lib.raise_on_info(info, "GaussianProcessRegression.log_likelihood (backward)", t.device)
            dt = (t[:, 1:] - t[:, :-1]).contiguous()
            part = torch.empty((bsz, n - 1, len(orders), 2), dtype=t.dtype, device=t.device)
            _lib.call("mf_sde_matern_transitions_grad_packed", t.dtype, bsz, n - 1, len(orders), c_orders, _lib.ptr(lam_c),
                      _lib.ptr(var_c), int(per_series), _lib.ptr(dt), jitter, _lib.ptr(g_packed), _lib.ptr(part),
                      _lib.stream_ptr(t.device))
            prior = torch.empty((bsz, len(orders), 2), dtype=t.dtype, device=t.device)
            _lib.call("mf_sde_matern_prior_chol_grad", t.dtype, bsz, len(orders), c_orders, _lib.ptr(lam_c), _lib.ptr(var_c),
                      int(per_series), jitter, _lib.ptr(g_cp0), _lib.ptr(prior), _lib.stream_ptr(t.device))
            g = torch.sum(part, dim=1) + prior                           # [B, ncomp, 2]
            if not per_series:
                g = torch.sum(g, dim=0)
            g_rinv = (-0.5 * torch.sum(g_om)).reshape(1, 1)
        return g[..., 0].contiguous(), g[..., 1].contiguous(), g_rinv, None, None, None, None, None, None


class GaussianProcessRegression:
    """GP regression as a Kalman filter on the kernel's state space model (gaussian_process_regression.py:29-160)."""

    def __init__(self, input_data: Tuple[torch.Tensor, torch.Tensor], kernel: SDEKernel,
                 chol_obs_covariance: Optional[torch.Tensor] = None) -> None:
        """
        :param input_data: ``(time_points [batch + [num_data]], observations [batch + [num_data, observation_dim]])``.
        :param chol_obs_covariance: ``[observation_dim, observation_dim]`` Cholesky factor of the noise covariance
            (default: identity, as in the reference).
        """
        time_points, observations = input_data
        obs_dim = observations.shape[-1]
        if chol_obs_covariance is None:
            chol_obs_covariance = torch.eye(obs_dim, dtype=observations.dtype, device=observations.device)
        if tuple(chol_obs_covariance.shape) != (obs_dim, obs_dim):
            raise ValueError("chol_obs_covariance must have shape [observation_dim, observation_dim]")
        if tuple(time_points.shape) != tuple(observations.shape[:-1]):
            raise ValueError("time_points must have shape observations.shape[:-1]")
        # one dtype and one device for the whole model, as the reference's default_float() (a float32 buffer handed to a
        # float64 kernel would be read past its end)
        _lib.same_dtype_device(observations, "GaussianProcessRegression", time_points=time_points,
                               chol_obs_covariance=chol_obs_covariance)
        self._kernel = kernel
        self._time_points = time_points
        self._observations = observations
        self._chol_obs_covariance = chol_obs_covariance

    @property
    def time_points(self) -> torch.Tensor:
        return self._time_points

    @property
    def observations(self) -> torch.Tensor:
        return self._observations

    @property
    def kernel(self) -> SDEKernel:
        return self._kernel

    @property
    def _kalman(self) -> KalmanFilter:
        """gaussian_process_regression.py:112-124 (no mean function: residuals = observations)."""
        return KalmanFilter(
            state_space_model=self._kernel.state_space_model(self._time_points),
            emission_model=self._kernel.generate_emission_model(self._time_points),
            observations=self._observations,
            chol_obs_covariance=self._chol_obs_covariance,
        )

    # time partitions per series of the fused kernel (0 = automatic) and optional hipEvent_t pair around its level-0 kernel
    _chunks = 0
    _prof_events = (None, None)
    fused = True    # set False to force the materialised route (kernel tensors -> KalmanFilter)

    def invalidate_hyperparameter_cache(self) -> None:
        """Forget the hyper-parameter tensors the fused route keeps between calls.  They are re-derived automatically when a
        source tensor (a lengthscale, a variance, the noise factor) is REPLACED or written in place through torch (tensor identity
        + autograd version counter); a write that bypasses the version counter - ``lengthscale.data.clamp_()``, ``set_()`` - is
        invisible to that check: call this after such a write."""
        self._fused_cache = None
        for comp in self._kernel._components():
            if isinstance(comp, _MaternBase):
                comp._lambda_cached = None      # (the components keep sqrt(order) / lengthscale per lengthscale version)
            else:
                comp.invalidate_cache()         # (a Product hands it on to its Matérn factor)

    fused_backward = True    # set False to force the materialised route whenever a gradient is required

    def _fused_differentiable(self, comps, multi, rows, m, d) -> Optional[torch.Tensor]:
        """The fused route when a hyper-parameter or the noise requires a gradient: ``_GprFusedLogLik`` (forward AND backward with the
        kernel -> state space model step fused; d <= 6: one or two components, one output, chains of more than 64 points).  ``None``:
        the materialised, differentiable route runs (row signatures, observations that require a gradient, short chains)."""
        n = self._time_points.shape[-1]
        if not _all_matern(comps):
            return None
        if (not self.fused_backward or rows or multi or m != 1 or d > 6 or n <= 64 or self._observations.requires_grad
                or self._time_points.requires_grad):
            return None
        dtype, dev = self._observations.dtype, self._observations.device
        batch = tuple(self._time_points.shape[:-1])
        t = self._time_points.reshape(-1, n).to(dtype).contiguous()
        y = self._observations.reshape(-1, n).contiguous()
        bsz = t.shape[0]
        nt = n - 1
        if bsz == 0 or _gpr_partition(bsz, nt, self._chunks)[1] < 2:
            return None                     # a single chunk per series leaves no summaries to start the backward from
        lam = [c._lambda.to(dtype=dtype, device=dev) for c in comps]
        var = [c._variance_t.to(dtype=dtype, device=dev) for c in comps]
        per_series = any(x.dim() > 0 for x in lam + var)
        if per_series:
            lam_t = torch.stack([x.expand(batch).reshape(-1) for x in lam], dim=-1)
            var_t = torch.stack([x.expand(batch).reshape(-1) for x in var], dim=-1)
        else:
            lam_t, var_t = torch.stack(lam), torch.stack(var)
        chol = self._chol_obs_covariance.to(dtype=dtype, device=dev)
        rinv = (1.0 / (chol * chol)).reshape(1, 1)
        log_det_rinv = torch.log(rinv[0, 0])
        orders = tuple(c.order for c in comps)
        out = _GprFusedLogLik.apply(lam_t, var_t, rinv, t, y, orders, per_series, self._kernel._jitter, self._chunks)
        const = -0.5 * math.log(2 * math.pi) * n * m + 0.5 * n * log_det_rinv
        return (out + const).reshape(batch)

    def _fused_log_likelihood_per_series(self) -> Optional[torch.Tensor]:
        """Per-series log-likelihood through ``mf_gpr_matern_loglik_*`` (kernel -> SSM generation fused into the Kalman
        sweep: 16 bytes per step instead of the materialised tensors); ``None`` when the kernel / shapes are not covered."""
        comps = self._kernel._components()
        multi = isinstance(self._kernel, IndependentMultiOutput)
        m = self._observations.shape[-1]
        d = self._kernel.state_dim
        if not _all_matern(comps):
            return None
        # register kernels (d <= 6): one or two components, one output; row kernels (7 <= d <= 15): any concatenation, one
        # output (Sum) or one per component (IndependentMultiOutput, up to four; eight for d >= 10) - BASELINE config 4 is 3 x Matern-5/2, 3 outputs
        rows = 7 <= d <= 15 and len(comps) <= 15 and (m == len(comps) <= (8 if d >= 10 else 4) if multi else m == 1)
        if not self.fused or not self._observations.is_cuda or not (rows or (not multi and len(comps) <= 2 and m == 1)):
            return None
        if torch.is_grad_enabled() and (self._kernel._needs_grad() or self._chol_obs_covariance.requires_grad
                                        or self._observations.requires_grad):
            return self._fused_differentiable(comps, multi, rows, m, d)
        batch = tuple(self._time_points.shape[:-1])
        n, dtype, dev = self._time_points.shape[-1], self._observations.dtype, self._observations.device
        t = self._time_points.reshape(-1, n).to(dtype).contiguous()
        y = self._observations.reshape(-1, n, m).contiguous()
        bsz = t.shape[0]
        if bsz == 0 or n < 1:
            return None
        # the kernel's hyper-parameter tensors ([B, ncomp] or [ncomp]), the noise precision and its log-determinant: a dozen
        # small launches - at config 4's size more host time (0.25 ms) than the whole sweep takes on the device - so they are
        # kept until a source tensor is replaced or written in place (tensor identity + autograd version counter)
        sources = [c._lengthscale_t for c in comps] + [c._variance_t for c in comps] + [self._chol_obs_covariance]
        key = (dtype, dev, batch) + tuple(x._version for x in sources)
        cached = getattr(self, "_fused_cache", None)
        if (cached is not None and cached[0] == key and len(cached[1]) == len(sources)
                and all(a is b for a, b in zip(cached[1], sources))):          # (the cache holds the tensors: ids are not reused)
            per_series, lam_t, var_t, chol, rinv, log_det_rinv = cached[2:]
        else:
            lam = [c._lambda.to(dtype=dtype, device=dev) for c in comps]
            var = [c._variance_t.to(dtype=dtype, device=dev) for c in comps]
            per_series = any(x.dim() > 0 for x in lam + var)
            if per_series:
                lam_t = torch.stack([x.expand(batch).reshape(-1) for x in lam], dim=-1).contiguous()
                var_t = torch.stack([x.expand(batch).reshape(-1) for x in var], dim=-1).contiguous()
            else:
                lam_t, var_t = torch.stack(lam).contiguous(), torch.stack(var).contiguous()
            chol = self._chol_obs_covariance.to(dtype=dtype, device=dev)
            if m == 1:
                rinv = (1.0 / (chol * chol)).reshape(1, 1).contiguous()
                log_det_rinv = torch.log(rinv[0, 0])
            else:
                rinv = torch.cholesky_inverse(chol.reshape(m, m)).contiguous()
                log_det_rinv = -2.0 * torch.sum(torch.log(torch.diagonal(chol.reshape(m, m))))
            self._fused_cache = (key, sources, per_series, lam_t, var_t, chol, rinv, log_det_rinv)
        lib = _lib.load()
        ws_bytes = int(lib.mf_kf_loglik_workspace_bytes(bsz, n, d, t.element_size(), self._chunks))
        if ws_bytes == 0:
            return None
        ws = _lib.workspace(ws_bytes, dev)
        out = torch.empty(bsz, dtype=dtype, device=dev)
        info = _lib.pivot_info(dev)
        orders = (ctypes.c_int * len(comps))(*[c.order for c in comps])
        tail = (self._kernel._jitter, 0.0, _lib.ptr(out), _lib.ptr(ws), ws_bytes, info, self._chunks, self._prof_events[0],
                self._prof_events[1], _lib.stream_ptr(dev))
        head = (bsz, n, len(comps), orders, _lib.ptr(lam_t), _lib.ptr(var_t), int(per_series), _lib.ptr(t), _lib.ptr(y))
        if multi:
            rc = _lib.call_rc("mf_gpr_matern_multi_loglik", dtype, *head, m, _lib.ptr(rinv), *tail)
        else:
            rc = _lib.call_rc("mf_gpr_matern_loglik", dtype, *head, _lib.ptr(rinv), *tail)
        if rc == -101:
            return None                     # component signature not instantiated: materialise instead
        _lib.check(rc, "mf_gpr_matern_loglik")
        _lib.raise_on_info(info, "GaussianProcessRegression.log_likelihood", dev)
        const = -0.5 * math.log(2 * math.pi) * n * m + 0.5 * n * log_det_rinv
        return (out + const).reshape(batch)

    def log_likelihood(self) -> torch.Tensor:
        """``log p(y | ϑ)`` summed over the batch (gaussian_process_regression.py:150-160)."""
        per_series = self._fused_log_likelihood_per_series()
        if per_series is not None:
            return _lib.checked(torch.sum(per_series))
        return self._kalman.log_likelihood()

    def loss(self) -> torch.Tensor:
        return -self.log_likelihood()

    @property
    def posterior(self) -> AnalyticPosteriorProcess:
        """Posterior process for inference at new time points (gaussian_process_regression.py:130-148)."""
        return AnalyticPosteriorProcess(
            posterior_dist=self.posterior_state_space_model(),
            kernel=self._kernel,
            conditioning_time_points=self._time_points,
            chol_obs_covariance=self._chol_obs_covariance,
        )

    def _fused_posterior_chain(self) -> Optional[StateSpaceModel]:
        """The posterior chain with the kernel -> state space model step fused (``mf_gpr_matern_loglik_*`` on an explicit partition
        for its chunk summaries, then ``mf_gpr_matern_posterior_chain_*``): no prior tensors in memory.  ``None`` where the fused
        kernels do not apply (row signatures, several outputs, d > 6, short chains, gradients required)."""
        comps = self._kernel._components()
        d, m, n = self._kernel.state_dim, self._observations.shape[-1], self._time_points.shape[-1]
        if not _all_matern(comps):
            return None
        if (not self.fused or not self.fused_backward or not self._observations.is_cuda or isinstance(self._kernel, IndependentMultiOutput)
                or len(comps) > 2 or m != 1 or d > 6 or n <= 64):
            return None
        if torch.is_grad_enabled() and (self._kernel._needs_grad() or self._chol_obs_covariance.requires_grad):
            return None
        dtype, dev = self._observations.dtype, self._observations.device
        batch = tuple(self._time_points.shape[:-1])
        t = self._time_points.reshape(-1, n).to(dtype).contiguous()
        y = self._observations.reshape(-1, n).contiguous()
        bsz, nt = t.shape[0], n - 1
        if bsz == 0 or bsz >= 2048:
            return None
        want, parts, length = _gpr_partition(bsz, nt, self._chunks, lanes=49152)                     # three wavefronts per CU
        if parts < 2:
            return None
        with torch.no_grad():
            lam = [c._lambda.to(dtype=dtype, device=dev) for c in comps]
            var = [c._variance_t.to(dtype=dtype, device=dev) for c in comps]
            per_series = any(x.dim() > 0 for x in lam + var)
            if per_series:
                lam_t = torch.stack([x.expand(batch).reshape(-1) for x in lam], dim=-1).contiguous()
                var_t = torch.stack([x.expand(batch).reshape(-1) for x in var], dim=-1).contiguous()
            else:
                lam_t, var_t = torch.stack(lam).contiguous(), torch.stack(var).contiguous()
            chol = self._chol_obs_covariance.to(dtype=dtype, device=dev)
            rinv = (1.0 / (chol * chol)).reshape(1, 1).contiguous()
            lib = _lib.load()
            esz = t.element_size()
            orders = (ctypes.c_int * len(comps))(*[c.order for c in comps])
            ws_f = _lib.workspace(int(lib.mf_kf_loglik_workspace_bytes(bsz, n, d, esz, want)), dev)
            val = torch.empty(bsz, dtype=dtype, device=dev)
            info = _lib.pivot_info(dev)
            rc = _lib.call_rc("mf_gpr_matern_loglik", dtype, bsz, n, len(comps), orders, _lib.ptr(lam_t), _lib.ptr(var_t),
                              int(per_series), _lib.ptr(t), _lib.ptr(y), _lib.ptr(rinv), self._kernel._jitter, 0.0, _lib.ptr(val),
                              _lib.ptr(ws_f), ws_f.numel(), info, want, None, None, _lib.stream_ptr(dev))
            if rc == -101:
                return None
            _lib.check(rc, "mf_gpr_matern_loglik")
            wsb = int(lib.mf_gpr_matern_posterior_chain_workspace_bytes(bsz, n, d, esz, parts))
            if wsb == 0:
                return None
            ws = _lib.workspace(wsb, dev)
            a_p = torch.empty((bsz, nt, d, d), dtype=dtype, device=dev)
            cq_p = torch.empty_like(a_p)
            b_p = torch.empty((bsz, nt, d), dtype=dtype, device=dev)
            mu0_p = torch.empty((bsz, d), dtype=dtype, device=dev)
            cp0_p = torch.empty((bsz, d, d), dtype=dtype, device=dev)
            rc = _lib.call_rc("mf_gpr_matern_posterior_chain", dtype, bsz, n, len(comps), orders, _lib.ptr(lam_t), _lib.ptr(var_t),
                              int(per_series), _lib.ptr(t), _lib.ptr(y), _lib.ptr(rinv), self._kernel._jitter, _lib.ptr(a_p),
                              _lib.ptr(mu0_p), _lib.ptr(b_p), _lib.ptr(cp0_p), _lib.ptr(cq_p), _lib.ptr(ws), wsb, info, _lib.ptr(ws_f),
                              parts, length, _lib.stream_ptr(dev))
            if rc == -101:
                return None
            _lib.check(rc, "mf_gpr_matern_posterior_chain")
            _lib.raise_on_info(info, "GaussianProcessRegression.posterior_state_space_model", dev)
        return StateSpaceModel(initial_mean=mu0_p.reshape(batch + (d,)), chol_initial_covariance=cp0_p.reshape(batch + (d, d)),
                               state_transitions=a_p.reshape(batch + (nt, d, d)), state_offsets=b_p.reshape(batch + (nt, d)),
                               chol_process_covariances=cq_p.reshape(batch + (nt, d, d)))

    def posterior_state_space_model(self) -> StateSpaceModel:
        """The smoothed chain on the training time points (what the reference's ``posterior`` is built from, :138-144)."""
        fused = self._fused_posterior_chain()
        return fused if fused is not None else self._kalman.posterior_state_space_model()


def back_project_nats(nat1: torch.Tensor, nat2: torch.Tensor, C: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Natural parameters ``[theta_1, theta_2]`` of a Gaussian in ``f`` (sufficient statistics ``[f, f^2]``) as the rank-one natural
    parameters of the degenerate Gaussian in ``g`` with ``f = C g``: ``[theta_1 C, theta_2 C^T C]`` (variational_cvi.py:423-445).

    :param nat1: ``batch + [N, 1]``; :param nat2: ``batch + [N, 1]``; :param C: ``batch + [N, 1, D]``.
    :return: ``batch + [N, D]`` and ``batch + [N, D, D]``.
    """
    if nat1.shape[-1] != 1 or tuple(nat2.shape) != tuple(nat1.shape) or tuple(C.shape[:-1]) != tuple(nat1.shape):
        raise ValueError(f"back_project_nats: nat1 {tuple(nat1.shape)}, nat2 {tuple(nat2.shape)} must be [..., N, 1] and C "
                         f"{tuple(C.shape)} [..., N, 1, D]")
    bp_nat1 = torch.sum(C * nat1[..., None], dim=-2)
    bp_nat2 = torch.sum(nat2[..., None, None] * C[..., None] * C[..., None, :], dim=-3)
    return bp_nat1, bp_nat2


def gradient_transformation_mean_var_to_expectation(inputs: Tuple[torch.Tensor, torch.Tensor],
                                                    grads: Tuple[torch.Tensor, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Gradients with respect to ``[mu, var]`` into gradients with respect to the expectation parameters ``[mu, var + mu^2]``
    (variational_cvi.py:448-460)."""
    return grads[0] - 2.0 * grads[1] * inputs[0], grads[1]


class _GaussianProcessWithSites:
    """What the site-based models share (variational_cvi.py:32-216, ``GaussianProcessWithSitesBase``; zero mean function): a GP
    prior, a general likelihood and a Gaussian posterior ``q(s) = p(s) prod_k t_k(f_k)`` parameterised by univariate Gaussian sites
    in natural form - the data, the sites, ``dist_p`` / ``dist_q``, the sites filter and its log-likelihood, prediction."""

    def __init__(self, input_data: Tuple[torch.Tensor, torch.Tensor], kernel: SDEKernel, likelihood: Likelihood,
                 learning_rate: float) -> None:
        time_points, observations = input_data
        if observations.dim() < 2 or observations.shape[-1] != 1:
            raise ValueError(f"observations must have shape batch + [num_data, 1], got {tuple(observations.shape)}")
        if tuple(time_points.shape) != tuple(observations.shape[:-1]):
            raise ValueError("time_points must have shape observations.shape[:-1]")
        if not isinstance(likelihood, Likelihood):
            raise TypeError("likelihood must be a markovflow_amd.likelihoods.Likelihood")
        if not 0.0 <= float(learning_rate) <= 1.0:
            raise ValueError(f"learning_rate must lie in [0, 1], got {learning_rate}")
        _refuse_non_stationary(kernel, type(self).__name__)
        _lib.same_dtype_device(observations, type(self).__name__, time_points=time_points)
        self._kernel = kernel
        self._likelihood = likelihood
        self._time_points = time_points
        self._observations = observations
        self.learning_rate = float(learning_rate)
        # variational_cvi.py:98-103
        self.sites = UnivariateGaussianSitesNat(nat1=torch.zeros_like(observations),
                                                nat2=torch.full_like(observations, -1e-10)[..., None],
                                                log_norm=torch.zeros_like(observations))

    @property
    def time_points(self) -> torch.Tensor:
        return self._time_points

    @property
    def conditioning_points(self) -> torch.Tensor:
        return self._time_points

    @property
    def observations(self) -> torch.Tensor:
        return self._observations

    @property
    def kernel(self) -> SDEKernel:
        return self._kernel

    @property
    def likelihood(self) -> Likelihood:
        return self._likelihood

    @property
    def dist_p(self) -> StateSpaceModel:
        """The prior chain on the training time points (variational_cvi.py:211-216)."""
        return self._kernel.state_space_model(self._time_points)

    @property
    def dist_q(self) -> StateSpaceModel:
        """The posterior chain on the training time points by the conjugate update of the natural parameters, prior + back-projected
        sites, then ``naturals_to_ssm_params`` (variational_cvi.py:105-135)."""
        prec = self.dist_p.precision
        h = self._kernel.generate_emission_model(self._time_points).emission_matrix
        bp_nat1, bp_nat2 = back_project_nats(self.sites.nat1, self.sites.nat2[..., 0], h)
        theta_diag = -0.5 * prec.block_diagonal + bp_nat2
        a_s, offsets, chol_p0, chol_q, mu0 = naturals_to_ssm_params(bp_nat1, theta_diag, -prec.block_sub_diagonal)
        return StateSpaceModel(initial_mean=mu0, chol_initial_covariance=chol_p0, state_transitions=a_s, state_offsets=offsets,
                               chol_process_covariances=chol_q)

    @property
    def posterior_kalman(self) -> KalmanFilterWithSites:
        """The filter over the prior chain and the sites (variational_cvi.py:137-144)."""
        return KalmanFilterWithSites(state_space_model=self.dist_p,
                                     emission_model=self._kernel.generate_emission_model(self._time_points), sites=self.sites)

    @property
    def posterior(self) -> ConditionalProcess:
        """Posterior process for prediction away from the training time points (variational_cvi.py:146-153)."""
        return ConditionalProcess(posterior_dist=self.dist_q, kernel=self._kernel, conditioning_time_points=self._time_points)

    def log_likelihood(self) -> torch.Tensor:
        """Log marginal likelihood of the model whose likelihood terms are the Gaussian sites (variational_cvi.py:155-161);
        differentiable with respect to the kernel's hyper-parameters through the filter's backward (the sites carry no graph)."""
        return self.posterior_kalman.log_likelihood()

    def elbo(self) -> torch.Tensor:
        """variational_cvi.py:370-379."""
        return self.log_likelihood()

    def loss(self) -> torch.Tensor:
        return -self.log_likelihood()

    def _project(self, dist: StateSpaceModel) -> Tuple[torch.Tensor, torch.Tensor]:
        """Marginals of ``f`` at the training time points, ``batch + [N, 1]`` each."""
        means, covs = dist.marginals
        return self._kernel.generate_emission_model(self._time_points).project_state_marginals_to_f(means, covs)

    def predict_log_density(self, input_data: Tuple[torch.Tensor, torch.Tensor], full_output_cov: bool = False) -> torch.Tensor:
        """Log density of new data ``(time_points, observations)`` under the posterior, ``batch + [num_new]``
        (variational_cvi.py:406-420)."""
        if full_output_cov:
            raise NotImplementedError("predict_log_density: the likelihoods are univariate (marginal variances only)")
        new_times, new_obs = input_data
        f_mean, f_var = self.posterior.predict_f(new_times)
        return self._likelihood.predict_log_density(f_mean, f_var, new_obs)


class CVIGaussianProcess(_GaussianProcessWithSites):
    """GP prior, general likelihood, Gaussian posterior parameterised by univariate Gaussian sites in natural form,
    ``q(s) = p(s) prod_k t_k(f_k)``, updated by conjugate-computation variational inference (Khan & Lin 2017):
    ``theta <- (1 - rho) theta + rho g`` with ``g`` the gradient of the variational expectations in the expectation parameters
    (variational_cvi.py:32-420; zero mean function)."""

    def __init__(self, input_data: Tuple[torch.Tensor, torch.Tensor], kernel: SDEKernel, likelihood: Likelihood,
                 learning_rate: float = 0.1) -> None:
        """
        :param input_data: ``(time_points [batch + [num_data]], observations [batch + [num_data, 1]])``.
        :param likelihood: a ``markovflow_amd.likelihoods.Likelihood``.
        :param learning_rate: the step ``rho`` of ``update_sites``, in [0, 1].
        """
        super().__init__(input_data, kernel, likelihood, learning_rate)

    def local_objective(self, Fmu: torch.Tensor, Fvar: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        """The variational expectations, ``[..., 1] -> [...]`` (variational_cvi.py:321-330)."""
        return self._likelihood.variational_expectations(Fmu, Fvar, Y)

    def local_objective_and_gradients(self, Fmu: torch.Tensor, Fvar: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        """The summed local objective and its gradients with respect to ``[mu, var + mu^2]`` (variational_cvi.py:332-349; the
        reference's tape is the derivative pair the likelihood computes with the value)."""
        fmu, fvar = Fmu.detach(), Fvar.detach()
        with torch.no_grad():
            ve, g_mu, g_var = self._likelihood._expectations(fmu, fvar, self._observations)
        return torch.sum(ve), gradient_transformation_mean_var_to_expectation((fmu, fvar), (g_mu, g_var))

    def update_sites(self) -> None:
        """One joint CVI step on the sites, in place (variational_cvi.py:351-368).  The marginals of ``f`` at the training points
        come from the filter route's posterior chain - the distribution ``posterior.predict_f(time_points)`` describes, without
        the interpolation to "new" points - and the step itself is one launch of ``mf_lik_cvi_site_update_*``."""
        with torch.no_grad():
            fmu, fvar = self._project(self.posterior_kalman.posterior_state_space_model())
            self._likelihood.cvi_site_update(fmu, fvar, self._observations, self.learning_rate, self.sites.nat1, self.sites.nat2)

    def classic_elbo(self) -> torch.Tensor:
        """``sum_i E_q log p(y_i | f_i) - KL[q(s) || p(s)]`` (variational_cvi.py:381-404; for testing, not for optimisation)."""
        dist_q = self.dist_q
        fmu, fvar = self._project(dist_q)
        ve = torch.sum(self._likelihood.variational_expectations(fmu, fvar, self._observations))
        return ve - torch.sum(dist_q.kl_divergence(self.dist_p))


def gradient_correction(inputs: Tuple[torch.Tensor, torch.Tensor], grads: Tuple[torch.Tensor, torch.Tensor]
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The EP step in natural parameters from the derivatives ``(g1, g2)`` of the log expected density in the mean, taken at the
    cavity ``inputs = (mu, var)`` (pep.py:250-261): ``L2 = 1 / (2 (var + 1 / g2))``, ``L1 = 2 L2 (g1 / g2 - mu)``, written without
    the division by ``g2``: ``den = 1 + var g2``, ``L2 = g2 / (2 den)``, ``L1 = (g1 - mu g2) / den``."""
    den = 1.0 + inputs[1] * grads[1]
    return (grads[0] - inputs[0] * grads[1]) / den, 0.5 * grads[1] / den


class PowerExpectationPropagation(_GaussianProcessWithSites):
    """GP prior, general likelihood, Gaussian posterior ``q(s) = p(s) prod_k t_k(f_k)`` with univariate Gaussian sites
    ``t_k(f) = exp(nat1 f + nat2 f^2 + log_norm)`` updated by power expectation propagation (pep.py:28-261, zero mean function;
    Seeger 2005, Minka 2004): remove the fraction ``alpha`` of a site from the posterior marginal (the cavity), match the moments
    of cavity x ``p(y | f)^alpha`` through the derivatives of the log expected density, and step with damping ``learning_rate``.
    ``energy()`` is the (power) EP approximation of the log marginal likelihood.

    Deviations from the reference:
      * the power: ``Likelihood.log_expected_density`` IS ``log int p^alpha q`` (the reference's ignores ``alpha``, or returns
        ``alpha log int p q`` for its Gaussian); at ``alpha = 1`` this model is the reference's;
      * ``update_sites(site_indices=None)`` updates EVERY site (in the reference the mask is then all zeros and nothing moves);
      * ``compute_log_norm`` evaluates the objective at the CAVITY, as ``update_sites`` does and as the energy assumes (the
        reference's evaluates it at the posterior marginals, pep.py:171);
      * a site whose cavity or correction is undefined (``fvar``, ``1 / v_c`` or ``1 + v_c g2`` not positive, a non-finite result) is
        SKIPPED; the reference would write NaN into it."""

    def __init__(self, input_data: Tuple[torch.Tensor, torch.Tensor], kernel: SDEKernel, likelihood: Likelihood,
                 learning_rate: float = 1.0, alpha: float = 1.0) -> None:
        """
        :param input_data: ``(time_points [batch + [num_data]], observations [batch + [num_data, 1]])``.
        :param likelihood: a ``markovflow_amd.likelihoods.Likelihood``.
        :param learning_rate: the damping of ``update_sites``, in [0, 1].
        :param alpha: the power, in (0, 1].
        """
        super().__init__(input_data, kernel, likelihood, learning_rate)
        if not 0.0 < float(alpha) <= 1.0:
            raise ValueError(f"alpha must lie in (0, 1], got {alpha}")
        self.alpha = float(alpha)

    def local_objective(self, Fmu: torch.Tensor, Fvar: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        """``log E_{N(f | Fmu, Fvar)} p(y | f)^alpha``, ``[..., 1] -> [...]`` (pep.py:99-101)."""
        return self._likelihood.log_expected_density(Fmu, Fvar, Y, alpha=self.alpha)

    def local_objective_gradients(self, Fmu: torch.Tensor, Fvar: torch.Tensor) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        """The local objective at the training observations, ``batch + [N]``, and the corrected gradients ``(L1, L2)``,
        ``batch + [N, 1]`` (pep.py:103-109)."""
        obj, grads = self._likelihood.grad_log_expected_density(Fmu, Fvar, self._observations, alpha=self.alpha)
        return obj, gradient_correction((Fmu, Fvar), grads)

    def compute_cavity_from_marginals(self, marginals: Tuple[torch.Tensor, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """The cavity marginals of ``f`` at the training points, ``batch + [N, 1]`` each, from the STATE marginals
        ``(means [.., N, d], covs [.., N, d, d])`` of ``q``.  The reference (pep.py:120-148) goes through ``d x d`` natural
        parameters - marginal to natural form, minus ``alpha`` times the back-projected site, back to moments, projected by ``H``;
        the site touches the state through ``f = h . s`` only, so by Sherman-Morrison that is the scalar statement on the marginal
        ``N(m, s)`` of ``f``:  ``1 / v_c = 1 / s + 2 alpha nat2``,  ``mu_c = v_c (m / s - alpha nat1)``.  NaN where ``1 / v_c`` is
        not positive."""
        with torch.no_grad():
            return self._scalar_cavity(*self._f_marginals(marginals))

    def _f_marginals(self, marginals: Tuple[torch.Tensor, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """The state marginals projected to ``f`` at the training points, ``batch + [N, 1]`` each."""
        return self._kernel.generate_emission_model(self._time_points).project_state_marginals_to_f(marginals[0], marginals[1])

    def _scalar_cavity(self, fmu: torch.Tensor, fvar: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        prec = 1.0 / fvar + 2.0 * self.alpha * self.sites.nat2[..., 0]
        ok = (fvar > 0) & (prec > 0)
        cav_var = torch.where(ok, 1.0 / prec, torch.full_like(fmu, float("nan")))
        return cav_var * (fmu / fvar - self.alpha * self.sites.nat1), cav_var

    def compute_cavity(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """The marginals of ``q(f) / t_n(f_n)^alpha`` at ``f_n`` for every data point (pep.py:150-157)."""
        return self.compute_cavity_from_marginals(self.dist_q.marginals)

    def compute_log_norm(self) -> torch.Tensor:
        """The site normalisers from the current ``q``, ``batch + [N]``: ``I(mu_c, v_c) + G(mu_c, v_c) - G(m, s)`` with
        ``G(mu, v) = (log v + mu^2 / v) / 2`` - the objective at the CAVITY (class docstring), one ``mf_lik_*`` launch.  A point
        whose cavity does not exist (``1 / v_c`` not positive) has no normaliser: NaN at that point, as in ``compute_cavity``.
        (``update_sites`` skips such a point; here nothing is skipped, because a sum without it would not be the energy.)"""
        return self._log_norm(self.dist_q)

    def _log_norm(self, dist_q: StateSpaceModel) -> torch.Tensor:
        with torch.no_grad():
            fmu, fvar = self._f_marginals(dist_q.marginals)
            cav_mu, cav_var = self._scalar_cavity(fmu, fvar)
            obj = self.local_objective(cav_mu, cav_var, self._observations)
            log_norm_cav = 0.5 * (torch.log(cav_var) + cav_mu * cav_mu / cav_var)
            log_norm_marg = 0.5 * (torch.log(fvar) + fmu * fmu / fvar)
            return obj + log_norm_cav[..., 0] - log_norm_marg[..., 0]

    def _update_flags(self, site_indices: torch.Tensor) -> torch.Tensor:
        """The byte mask ``batch + [N]`` of ``update_sites``: 1 at the chosen points of every series.  Built by comparison, not by an
        indexed store, so that no index can write outside the mask."""
        if site_indices.dim() != 1 or site_indices.dtype.is_floating_point or site_indices.dtype == torch.bool:
            raise ValueError("update_sites: site_indices must be a 1-D integer tensor")
        n = self._observations.shape[-2]
        if site_indices.numel() and not (-n <= int(site_indices.min()) and int(site_indices.max()) < n):
            raise IndexError(f"update_sites: site_indices must lie in [-{n}, {n}) for {n} data points")
        idx = site_indices.to(device=self._observations.device, dtype=torch.long)
        idx = torch.where(idx < 0, idx + n, idx)
        flags = (torch.arange(n, device=idx.device)[:, None] == idx[None, :]).any(dim=-1).to(torch.uint8)
        return flags.expand(self._observations.shape[:-1]).contiguous()

    def update_sites(self, site_indices: Optional[torch.Tensor] = None) -> None:
        """One power-EP step on the sites, in place (pep.py:179-215).  The marginals of ``f`` come from the filter route's posterior
        chain, as in ``CVIGaussianProcess.update_sites``; cavity, log expected density with its derivatives, gradient correction,
        normaliser and the power / damping step are ONE launch of ``mf_lik_pep_site_update_*``.

        :param site_indices: a 1-D integer tensor of point indices, applied to every series; None: all points.  Indices follow
            torch's convention - ``-N <= i < N``, a negative one counts from the end, repeats are allowed - and anything outside
            that range raises IndexError on either device (for indices held on the device the check is one host read)."""
        with torch.no_grad():
            update = None if site_indices is None else self._update_flags(site_indices)
            fmu, fvar = self._project(self.posterior_kalman.posterior_state_space_model())
            self._likelihood.pep_site_update(fmu, fvar, self._observations, self.alpha, self.learning_rate, self.sites.nat1,
                                             self.sites.nat2, self.sites.log_norm, update)

    def energy(self) -> torch.Tensor:
        """The power-EP energy per series, ``batch`` (pep.py:223-230): ``dist_q.normalizer() - dist_p.normalizer()
        + (1 / alpha) sum_n log_norm_n`` with the normalisers computed afresh from the current ``q``.  Not differentiable.  A series
        with a point whose cavity does not exist has no energy: NaN for that series (``compute_log_norm``), the others are unaffected."""
        with torch.no_grad():
            dist_q = self.dist_q
            log_norm = torch.sum(self._log_norm(dist_q), dim=-1)
            return dist_q.normalizer() - self.dist_p.normalizer() + log_norm / self.alpha


SPARSE_SITE_MAX_TWO_D = 18      # mf_lik_sparse_cvi_site_update_*: 2 d <= 18, the range of the lane-per-point conditional kernels


def sparse_site_projections(kernel: SDEKernel, time_points: torch.Tensor, inducing_points: torch.Tensor
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """What the sparse site update needs of every data point, none of it depending on the sites: ``w_k = H P_k``
    (``batch + [N, 2d]``), ``c_k = H T_k H^T`` (``batch + [N]``) from ``conditional_statistics`` (sparse_variational_cvi.py:192-194),
    the index of the pair that brackets the point (``batch + [N]``; ``z_{m-1} < x <= z_m`` belongs to pair ``m``) and the segment
    offsets ``batch + [M + 2]`` (offset ``m`` counts the ``x <= z_{m-1}``; 0 and ``N`` at the ends).  Both sets of time points must
    be sorted."""
    proj, cov, indices = conditionals._conditional_statistics(time_points, inducing_points, kernel)
    h = kernel.generate_emission_model(time_points).emission_matrix                         # [.., N, 1, d]
    w = (h @ proj)[..., 0, :]
    c = (h @ cov @ h.transpose(-1, -2))[..., 0, 0]
    return w.contiguous(), c.contiguous(), indices, _site_offsets(time_points, inducing_points)


def _site_offsets(time_points: torch.Tensor, inducing_points: torch.Tensor) -> torch.Tensor:
    """The segment offsets ``batch + [M + 2]`` of ``sparse_site_projections``."""
    x = time_points.to(inducing_points.dtype).contiguous()
    inner = torch.searchsorted(x, inducing_points.contiguous(), right=True)
    zero = torch.zeros_like(inner[..., :1])
    offsets = torch.cat([zero, inner, torch.full_like(zero, x.shape[-1])], dim=-1)
    return offsets.contiguous()


def _sparse_point_marginals(w: torch.Tensor, c: torch.Tensor, indices: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor,
                            segs: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per point ``fmu = w . m_s`` and ``fvar = c + w^T S_s w`` (``[.., N]`` each) with ``(m_s, S_s)`` the marginal of the pair the
    point belongs to (``indices [.., N]``), and one flat segment index over the batch, ``series * segs + pair`` (``[B N]``)."""
    two_d = w.shape[-1]
    m = torch.gather(pair_mean, -2, indices[..., None].expand(tuple(indices.shape) + (two_d,)))
    cov = torch.gather(pair_cov, -3, indices[..., None, None].expand(tuple(indices.shape) + (two_d, two_d)))
    fmu = torch.sum(w * m, dim=-1)
    fvar = c + torch.sum(w * torch.sum(cov * w[..., None, :], dim=-1), dim=-1)
    series = torch.arange(math.prod(indices.shape[:-1]), device=indices.device).reshape(tuple(indices.shape[:-1]) + (1,))
    return fmu, fvar, (indices + series * segs).reshape(-1)


def sparse_cvi_site_update_torch(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor, indices: torch.Tensor,
                                 pair_mean: torch.Tensor, pair_cov: torch.Tensor, learning_rate: float, nat1: torch.Tensor,
                                 nat2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The sparse CVI step as a torch composition (sparse_variational_cvi.py:176-221), IN PLACE on ``nat1 [.., M+1, 2d]`` and
    ``nat2 [.., M+1, 2d, 2d]``: per point ``fmu = w . m_s``, ``fvar = c + w^T S_s w`` with ``(m_s, S_s)`` the marginal of the pair the
    point belongs to, the gradients of the variational expectations in ``[mu, var + mu^2]``, ``back_project_nats`` through ``w`` and
    ``index_add_`` over the segment index; ``nat <- (1 - lr) nat + lr sum``.  What ``mf_lik_sparse_cvi_site_update_*`` fuses: it
    runs on CPU tensors as a function (the model itself needs the HIP chain kernels, as every model here), it is the model's route
    for ``2d > 18``, and it is what the kernel is measured against.  ``w [.., N, 2d]``, ``c``, ``y``, ``indices``
    ``[.., N]``.  Returns ``(fmu, fvar, ve)``, ``[.., N]`` each."""
    two_d = w.shape[-1]
    lr = float(learning_rate)
    with torch.no_grad():
        fmu, fvar, flat = _sparse_point_marginals(w, c, indices, pair_mean, pair_cov, nat1.shape[-2])
        ve, g_mu, g_var = likelihood._expectations(fmu[..., None], fvar[..., None], y[..., None])
        bad = ~(fvar > 0)
        fmu, fvar = (torch.where(bad, torch.full_like(v, float("nan")), v) for v in (fmu, fvar))
        g1, g2 = gradient_transformation_mean_var_to_expectation((fmu[..., None], fvar[..., None]), (g_mu, g_var))
        theta1, theta2 = back_project_nats(g1, g2, w[..., None, :])
        sum1 = torch.zeros_like(nat1).reshape(-1, two_d).index_add_(0, flat, theta1.reshape(-1, two_d))
        sum2 = torch.zeros_like(nat2).reshape(-1, two_d, two_d).index_add_(0, flat, theta2.reshape(-1, two_d, two_d))
        nat1.mul_(1.0 - lr).add_(lr * sum1.reshape(nat1.shape))
        nat2.mul_(1.0 - lr).add_(lr * sum2.reshape(nat2.shape))
    return fmu, fvar, ve[..., 0]


def sparse_cvi_site_update_hip(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor, offsets: torch.Tensor,
                               pair_mean: torch.Tensor, pair_cov: torch.Tensor, learning_rate: float, nat1: Optional[torch.Tensor],
                               nat2: Optional[torch.Tensor], want_outputs: bool = False):
    """ONE launch of ``mf_lik_sparse_cvi_site_update_*`` on HIP tensors (``2d <= 18``): what ``sparse_cvi_site_update_torch``
    computes, with the segment ``offsets [.., M + 2]`` in place of the per-point index; ``nat1`` / ``nat2`` (contiguous) are updated
    IN PLACE, or both ``None``: projection only.  ``want_outputs``: return ``(fmu, fvar, ve)``, ``[.., N]`` each (else three Nones)."""
    dtype, dev = w.dtype, w.device
    n, two_d, segs = w.shape[-2], w.shape[-1], offsets.shape[-1] - 1
    bsz = offsets.numel() // (segs + 1)
    if nat1 is not None and not (nat1.is_contiguous() and nat2.is_contiguous()):
        raise ValueError("sparse_cvi_site_update_hip: nat1 and nat2 must be contiguous")
    outs = tuple(torch.empty(tuple(w.shape[:-1]), dtype=dtype, device=dev) for _ in range(3)) if want_outputs else (None, None, None)
    _lib.call("mf_lik_sparse_cvi_site_update", dtype, bsz, n, segs, two_d, *likelihood._kernel_args(), _lib.ptr(offsets.contiguous()),
              _lib.ptr(w.contiguous()), _lib.ptr(c.contiguous()), _lib.ptr(y.contiguous()), _lib.ptr(pair_mean.contiguous()),
              _lib.ptr(pair_cov.contiguous()), float(learning_rate), _lib.ptr(nat1), _lib.ptr(nat2), *[_lib.ptr(o) for o in outs],
              _lib.stream_ptr(dev))
    if nat1 is not None:
        # the kernel wrote through raw pointers: tell torch, so that whatever keys a cache on (tensor, version) sees the write
        torch.autograd.graph.increment_version(nat1)
        torch.autograd.graph.increment_version(nat2)
    return outs


class _SparseGaussianProcess:
    """What the inducing-point models share: the validated kernel, likelihood and inducing points, the checks on a data set,
    the cache of the per-point projections, the stationary prior beyond the ends of the chain and ``predict_log_density``."""

    def __init__(self, kernel: SDEKernel, likelihood: Likelihood, inducing_points: torch.Tensor, min_inducing: int) -> None:
        if not isinstance(kernel, SDEKernel):
            raise TypeError("kernel must be a markovflow_amd.kernels.SDEKernel")
        _refuse_non_stationary(kernel, type(self).__name__)
        if not isinstance(likelihood, Likelihood):
            raise TypeError("likelihood must be a markovflow_amd.likelihoods.Likelihood")
        if (not isinstance(inducing_points, torch.Tensor) or inducing_points.dim() < 1
                or inducing_points.shape[-1] < min_inducing):
            raise ValueError("inducing_points must be a tensor of shape batch + [num_inducing] with at least "
                             + {1: "one point", 2: "two points"}[min_inducing])
        if inducing_points.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {inducing_points.dtype}")
        if bool((inducing_points[..., 1:] < inducing_points[..., :-1]).any()):
            raise ValueError("inducing_points must be sorted")
        self._kernel = kernel
        self._likelihood = likelihood
        self.inducing_inputs = inducing_points
        self._projection_cache = None

    @property
    def kernel(self) -> SDEKernel:
        return self._kernel

    @property
    def likelihood(self) -> Likelihood:
        return self._likelihood

    def _check_data(self, input_data: Tuple[torch.Tensor, torch.Tensor], what: str) -> Tuple[torch.Tensor, torch.Tensor]:
        time_points, observations = input_data
        if observations.dim() < 2 or observations.shape[-1] != 1:
            raise ValueError(f"{what}: observations must have shape batch + [num_data, 1], got {tuple(observations.shape)}")
        if tuple(time_points.shape) != tuple(observations.shape[:-1]):
            raise ValueError(f"{what}: time_points must have shape observations.shape[:-1]")
        if tuple(time_points.shape[:-1]) != tuple(self.inducing_inputs.shape[:-1]):
            raise ValueError(f"{what}: the data must carry the batch shape of the inducing points, "
                             f"{tuple(self.inducing_inputs.shape[:-1])}, got {tuple(time_points.shape[:-1])}")
        _lib.same_dtype_device(self.inducing_inputs, f"{type(self).__name__}.{what}", time_points=time_points,
                               observations=observations)
        return time_points, observations

    def _compute_projections(self, time_points: torch.Tensor):
        """What ``_projections`` keeps for a data tensor (computed under ``no_grad``)."""
        raise NotImplementedError

    def _projections(self, time_points: torch.Tensor):
        """``_compute_projections`` of the data, kept until the data, the inducing points or a hyper-parameter of the kernel is
        replaced or written in place (tensor identity, data pointer and version counter, as the filter caches)."""
        sources = [time_points, self.inducing_inputs] + [x for comp in self._kernel._components() for x in comp._leaves()]
        key = tuple(_version_key(x) for x in sources)
        cached = self._projection_cache
        if (cached is not None and None not in key and cached[0] == key and len(cached[1]) == len(sources)
                and all(a is b for a, b in zip(cached[1], sources))):          # (the cache holds the tensors: ids are not reused)
            return cached[2]
        with torch.no_grad():
            out = self._compute_projections(time_points)
        self._projection_cache = (key, sources, out)
        return out

    def _stationary_prior(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(m0, P0)`` of the kernel on the inducing points' batch, dtype and device: the outer neighbour of the first and the
        last pair."""
        z = self.inducing_inputs
        m0 = self._kernel.initial_mean(tuple(z.shape[:-1])).to(dtype=z.dtype, device=z.device)
        p0 = self._kernel.initial_covariance(z[..., :1]).to(dtype=z.dtype, device=z.device)
        return m0, p0

    def _predict_f(self, new_time_points: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.posterior.predict_f(new_time_points)

    def predict_log_density(self, input_data: Tuple[torch.Tensor, torch.Tensor], full_output_cov: bool = False) -> torch.Tensor:
        """Log density of new data ``(time_points, observations)`` under the posterior, ``batch + [num_new]``
        (sparse_variational.py:262-270)."""
        if full_output_cov:
            raise NotImplementedError("predict_log_density: the likelihoods are univariate (marginal variances only)")
        new_times, new_obs = input_data
        f_mean, f_var = self._predict_f(new_times)
        return self._likelihood.predict_log_density(f_mean, f_var, new_obs)


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


# ---- sparse power EP ----------------------------------------------------------------------------------------------------------------
def sparse_pep_site_update_torch(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor, indices: torch.Tensor,
                                 cav_mean: torch.Tensor, cav_cov: torch.Tensor, alpha: float, learning_rate: float,
                                 nat1: Optional[torch.Tensor], nat2: Optional[torch.Tensor], log_norm: Optional[torch.Tensor],
                                 seg_const: Optional[torch.Tensor] = None
                                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The sparse power-EP step as a torch composition (sparse_pep.py:316-380, 473-487), IN PLACE on ``nat1 [.., M+1, 2d]``,
    ``nat2 [.., M+1, 2d, 2d]`` and ``log_norm [.., M+1]`` (all three ``None``: evaluation only).  Per point, with ``(m_c, S_c)`` the
    CAVITY of the pair the point belongs to (``indices [.., N]``): ``fmu = w . m_c``, ``fvar = c + w^T S_c w``; ``I, g1, g2`` of
    ``log int p(y | f)^alpha N(f | fmu, fvar) df``; ``den = 1 + fvar g2`` (Gaussian: in closed form, as ``torch_pep_site_update``),
    ``L2 = g2 / (2 den)``, ``L1 = (g1 - fmu g2) / den``.  A point where ``fvar`` or ``den`` is not positive or a value is not finite
    is undefined and contributes NaN.  Per segment, by ``index_add_`` over the segment index: ``sum L2 w w^T``, ``sum L1 w``,
    ``sum I``; if all of them (the last with ``seg_const [.., M+1]`` added) are finite, ``pep = (1 - alpha) old + sum``,
    ``new = (1 - lr) old + lr pep``; otherwise the segment's sites stay as they are.  What ``mf_lik_sparse_pep_site_update_*``
    fuses: it runs on CPU tensors, it is the model's route for ``2d > 18``, and it is what the kernel pair is measured against.
    Returns ``(led_sum [.., M+1], fmu, fvar, led [.., N])``: the raw ``sum I`` (NaN for an undefined segment), and per point the
    cavity marginal (NaN where ``fvar`` is not positive) and ``I``."""
    two_d, segs = w.shape[-1], cav_mean.shape[-2]
    alpha, lr = Likelihood._check_alpha("sparse_pep_site_update_torch", alpha), float(learning_rate)
    if not 0.0 <= lr <= 1.0:
        raise ValueError(f"sparse_pep_site_update_torch: learning_rate must lie in [0, 1], got {learning_rate}")
    sites = (nat1, nat2, log_norm)
    if any(t is None for t in sites) and not all(t is None for t in sites):
        raise ValueError("sparse_pep_site_update_torch: nat1, nat2 and log_norm are given together, or all None (evaluation only)")
    with torch.no_grad():
        fmu, fvar, flat = _sparse_point_marginals(w, c, indices, cav_mean, cav_cov, segs)
        led, g1, g2 = (t[..., 0] for t in torch_log_expected_density(likelihood, fmu[..., None], fvar[..., None], y[..., None], alpha))
        if isinstance(likelihood, Gaussian):
            den = (likelihood.variance / alpha) / (likelihood.variance / alpha + fvar)
        else:
            den = 1.0 + fvar * g2
        l2, l1 = 0.5 * g2 / den, (g1 - fmu * g2) / den
        nan = torch.full_like(fmu, float("nan"))
        inside = fvar > 0
        defined = inside & (den > 0) & torch.isfinite(l2) & torch.isfinite(l1) & torch.isfinite(led)
        l2, l1, row = (torch.where(defined, v, nan) for v in (l2, l1, led))
        fmu, fvar = torch.where(inside, fmu, nan), torch.where(inside, fvar, nan)
        batch = tuple(cav_mean.shape[:-2])
        rows = math.prod(batch) * segs
        sum2 = torch.zeros((rows, two_d, two_d), dtype=w.dtype, device=w.device).index_add_(
            0, flat, (l2[..., None, None] * w[..., :, None] * w[..., None, :]).reshape(-1, two_d, two_d)).reshape(batch + (segs, two_d, two_d))
        sum1 = torch.zeros((rows, two_d), dtype=w.dtype, device=w.device).index_add_(
            0, flat, (l1[..., None] * w).reshape(-1, two_d)).reshape(batch + (segs, two_d))
        led_sum = torch.zeros(rows, dtype=w.dtype, device=w.device).index_add_(0, flat, row.reshape(-1)).reshape(batch + (segs,))
        if nat1 is not None:
            total = led_sum if seg_const is None else led_sum + seg_const
            ok = torch.isfinite(sum2).all(dim=-1).all(dim=-1) & torch.isfinite(sum1).all(dim=-1) & torch.isfinite(total)
            for t, step, keep in ((nat2, sum2, ok[..., None, None]), (nat1, sum1, ok[..., None]), (log_norm, total, ok)):
                t.copy_(torch.where(keep, (1.0 - lr) * t + lr * ((1.0 - alpha) * t + step), t))
    return led_sum, fmu, fvar, led


def sparse_pep_site_update_hip(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor, offsets: torch.Tensor,
                               cav_mean: torch.Tensor, cav_cov: torch.Tensor, alpha: float, learning_rate: float,
                               nat1: Optional[torch.Tensor], nat2: Optional[torch.Tensor], log_norm: Optional[torch.Tensor],
                               seg_const: Optional[torch.Tensor] = None, tiles=None, want_led_sum: bool = False,
                               want_outputs: bool = False):
    """ONE call of ``mf_lik_sparse_pep_site_update_*`` on HIP tensors (``2d <= 18``): what ``sparse_pep_site_update_torch`` computes,
    with the segment ``offsets [.., M + 2]`` in place of the per-point index and ``tiles = sparse_expectation_tiles(offsets)`` when the
    caller keeps it.  ``nat1`` / ``nat2`` / ``log_norm`` (contiguous) are updated IN PLACE, or all ``None``: evaluation only.
    Returns ``(led_sum | None, fmu | None, fvar | None, led | None)`` as ``want_led_sum`` / ``want_outputs`` ask."""
    dtype, dev = w.dtype, w.device
    n, two_d, segs = w.shape[-2], w.shape[-1], offsets.shape[-1] - 1
    batch = tuple(offsets.shape[:-1])
    bsz = offsets.numel() // (segs + 1)
    alpha = Likelihood._check_alpha("sparse_pep_site_update_hip", alpha)
    sites = (nat1, nat2, log_norm)
    if any(t is None for t in sites) and not all(t is None for t in sites):
        raise ValueError("sparse_pep_site_update_hip: nat1, nat2 and log_norm are given together, or all None (evaluation only)")
    if nat1 is not None and not all(t.is_contiguous() for t in sites):
        raise ValueError("sparse_pep_site_update_hip: nat1, nat2 and log_norm must be contiguous")
    num_tiles, tile_seg, seg_tile = sparse_expectation_tiles(offsets) if tiles is None else tiles
    led_sum = torch.empty(batch + (segs,), dtype=dtype, device=dev) if want_led_sum else None
    outs = tuple(torch.empty(tuple(w.shape[:-1]), dtype=dtype, device=dev) for _ in range(3)) if want_outputs else (None, None, None)
    # (the row of the workspace is the SVGP entry point's, and so is the size function: include/markovflow_amd.h)
    ws_bytes = int(_lib.load().mf_lik_sparse_expectations_workspace_bytes(num_tiles, two_d, w.element_size()))
    ws = _lib.workspace(ws_bytes, dev)
    _lib.call("mf_lik_sparse_pep_site_update", dtype, bsz, n, segs, two_d, *likelihood._kernel_args(), alpha, float(learning_rate),
              _lib.ptr(offsets.contiguous()), _lib.ptr(w.contiguous()), _lib.ptr(c.contiguous()), _lib.ptr(y.contiguous()),
              _lib.ptr(cav_mean.contiguous()), _lib.ptr(cav_cov.contiguous()),
              _lib.ptr(None if seg_const is None else seg_const.contiguous()), num_tiles, _lib.ptr(tile_seg), _lib.ptr(seg_tile),
              _lib.ptr(ws), ws_bytes, _lib.ptr(nat1), _lib.ptr(nat2), _lib.ptr(log_norm), _lib.ptr(led_sum),
              *[_lib.ptr(o) for o in outs], _lib.stream_ptr(dev))
    if nat1 is not None:
        # the kernels wrote through raw pointers: tell torch, so that whatever keys a cache on (tensor, version) sees the write
        for t in sites:
            torch.autograd.graph.increment_version(t)
    return (led_sum,) + outs


def pair_cavity(pair_mean: torch.Tensor, pair_cov: torch.Tensor, nat1: torch.Tensor, nat2: torch.Tensor, beta: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The cavity of every pair of neighbouring inducing states and the log of ``E_q[t^(-beta)]``: with the marginal ``N(m, S)`` of
    ``q`` on a pair (``pair_mean [.., S, 2d]``, ``pair_cov [.., S, 2d, 2d]``), its site ``t(v) = exp(nat1 . v + v^T nat2 v + ...)`` and
    the fraction ``beta [.., S]`` of the site to remove, the cavity ``N(m_c, S_c)`` has precision ``S^-1 + 2 beta nat2`` and linear
    term ``S^-1 m - beta nat1`` (sparse_pep.py:251-293), and ``Gamma = G(m_c, S_c) - G(m, S)`` with
    ``G(m, S) = (log det S + m^T S^-1 m) / 2``.  Batched torch: two Cholesky factorisations per pair, none of which raises - a pair
    whose marginal or cavity precision is not positive definite gets NaN in all three results.
    Returns ``(cav_mean, cav_cov, gamma [.., S])``."""
    eye = torch.eye(pair_cov.shape[-1], dtype=pair_cov.dtype, device=pair_cov.device).expand(pair_cov.shape)
    chol_s, info_s = torch.linalg.cholesky_ex(pair_cov, check_errors=False)
    prec = _lib.chol_solve(chol_s, eye)
    lin = _lib.chol_solve(chol_s, pair_mean[..., None])[..., 0]
    cav_prec = prec + 2.0 * beta[..., None, None] * nat2
    cav_prec = 0.5 * (cav_prec + cav_prec.transpose(-1, -2))
    cav_lin = lin - beta[..., None] * nat1
    chol_c, info_c = torch.linalg.cholesky_ex(cav_prec, check_errors=False)
    cav_cov = _lib.chol_solve(chol_c, eye)
    cav_mean = _lib.chol_solve(chol_c, cav_lin[..., None])[..., 0]
    g_marg = torch.sum(torch.log(torch.diagonal(chol_s, dim1=-2, dim2=-1)), dim=-1) + 0.5 * torch.sum(pair_mean * lin, dim=-1)
    g_cav = -torch.sum(torch.log(torch.diagonal(chol_c, dim1=-2, dim2=-1)), dim=-1) + 0.5 * torch.sum(cav_mean * cav_lin, dim=-1)
    bad = (info_s != 0) | (info_c != 0)
    nan = float("nan")
    return (cav_mean.masked_fill(bad[..., None], nan), cav_cov.masked_fill(bad[..., None, None], nan),
            (g_cav - g_marg).masked_fill(bad, nan))


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


# ---- SVGP: the ELBO's data term ----------------------------------------------------------------------------------------------------
SPARSE_EXPECT_TILE = 64         # mf_lik_sparse_expectations_*: points per tile of pass 1


def sparse_expectation_tiles(offsets: torch.Tensor, tile: int = SPARSE_EXPECT_TILE) -> Tuple[int, torch.Tensor, torch.Tensor]:
    """The tile table of ``mf_lik_sparse_expectations_*`` from the segment ``offsets [.., S + 1]``: the number of tiles (ONE read-back:
    callers cache the table with the projections), ``tile_seg [num_tiles]`` - the flat segment ``series * S + segment`` of every tile
    - and ``seg_tile [B S + 1]``, the first tile of every segment; flat int64 tensors on the offsets' device.  ``tile``: the points
    per tile (``ST_EXPECT_TILE`` for ``mf_lik_st_expectations_*``)."""
    lengths = (offsets[..., 1:] - offsets[..., :-1]).reshape(-1)
    per_segment = (lengths + (tile - 1)) // tile
    seg_tile = torch.cat([torch.zeros_like(per_segment[:1]), torch.cumsum(per_segment, dim=0)]).contiguous()
    num_tiles = int(seg_tile[-1])
    tile_seg = torch.repeat_interleave(torch.arange(per_segment.numel(), device=offsets.device), per_segment, output_size=num_tiles)
    return num_tiles, tile_seg.contiguous(), seg_tile


def _sparse_expectations_launch(likelihood: Likelihood, w, c, y, offsets, tiles, pair_mean, pair_cov, want_grads: bool):
    """ONE call of ``mf_lik_sparse_expectations_*``: ``(ve_sum [.., S], g_mean [.., S, 2d] | None, g_cov [.., S, 2d, 2d] | None)``."""
    dtype, dev = w.dtype, w.device
    n, two_d, segs = w.shape[-2], w.shape[-1], offsets.shape[-1] - 1
    batch = tuple(offsets.shape[:-1])
    bsz = offsets.numel() // (segs + 1)
    num_tiles, tile_seg, seg_tile = tiles
    ve_sum = torch.empty(batch + (segs,), dtype=dtype, device=dev)
    g_mean = torch.empty(batch + (segs, two_d), dtype=dtype, device=dev) if want_grads else None
    g_cov = torch.empty(batch + (segs, two_d, two_d), dtype=dtype, device=dev) if want_grads else None
    ws_bytes = int(_lib.load().mf_lik_sparse_expectations_workspace_bytes(num_tiles, two_d, w.element_size()))
    ws = _lib.workspace(ws_bytes, dev)
    _lib.call("mf_lik_sparse_expectations", dtype, bsz, n, segs, two_d, *likelihood._kernel_args(), _lib.ptr(offsets.contiguous()),
              _lib.ptr(w.contiguous()), _lib.ptr(c.contiguous()), _lib.ptr(y.contiguous()), _lib.ptr(pair_mean.contiguous()),
              _lib.ptr(pair_cov.contiguous()), num_tiles, _lib.ptr(tile_seg), _lib.ptr(seg_tile), _lib.ptr(ws), ws_bytes,
              _lib.ptr(ve_sum), _lib.ptr(g_mean), _lib.ptr(g_cov), _lib.stream_ptr(dev))
    return ve_sum, g_mean, g_cov


class _SparseExpectedLogLikelihood(torch.autograd.Function):
    """Value ``batch + [M + 1]``; the adjoints onto the pair marginals come out of the same launch and wait for the backward."""

    @staticmethod
    def forward(ctx, pair_mean, pair_cov, likelihood, w, c, y, offsets, tiles):
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        with torch.no_grad():
            ve_sum, g_mean, g_cov = _sparse_expectations_launch(likelihood, w.detach(), c.detach(), y.detach(), offsets, tiles,
                                                                pair_mean.detach(), pair_cov.detach(), want)
        if want:
            ctx.save_for_backward(g_mean, g_cov)
        return ve_sum

    @staticmethod
    def backward(ctx, grad_out):
        if torch.is_grad_enabled():
            raise RuntimeError("sparse_expected_log_likelihood is differentiable once: its backward uses the adjoints computed in "
                               "the forward and has no second-order support (create_graph=True)")
        g_mean, g_cov = ctx.saved_tensors
        return (grad_out[..., None] * g_mean if ctx.needs_input_grad[0] else None,
                grad_out[..., None, None] * g_cov if ctx.needs_input_grad[1] else None, None, None, None, None, None, None)


def sparse_expected_log_likelihood(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor, offsets: torch.Tensor,
                                   pair_mean: torch.Tensor, pair_cov: torch.Tensor, tiles=None) -> torch.Tensor:
    """``sum_k E_q log p(y_k | f_k)`` per pair of neighbouring inducing states, ``batch + [M + 1]``, with ``fmu = w_k . m_s`` and
    ``fvar = c_k + w_k^T S_s w_k`` for the points ``offsets[s] <= k < offsets[s + 1]`` of pair ``s`` (``w [.., N, 2d]``, ``c``, ``y``
    ``[.., N]``, ``offsets [.., M + 2]``, ``pair_mean [.., M + 1, 2d]``, ``pair_cov [.., M + 1, 2d, 2d]``): ONE call of
    ``mf_lik_sparse_expectations_*`` on HIP tensors, ``2d <= 18``.  Differentiable ONCE in ``pair_mean`` and ``pair_cov`` (an
    unconstrained matrix: the gradient is symmetric) - the backward multiplies the adjoints the forward computed beside the value,
    there is no second launch; not differentiable in ``w`` and ``c``.  ``tiles``: ``sparse_expectation_tiles(offsets)`` when the
    caller keeps it."""
    if not isinstance(likelihood, Likelihood):
        raise TypeError("likelihood must be a markovflow_amd.likelihoods.Likelihood")
    two_d, segs = w.shape[-1], offsets.shape[-1] - 1
    batch = tuple(offsets.shape[:-1])
    if two_d > SPARSE_SITE_MAX_TWO_D or two_d % 2:
        raise NotImplementedError(f"sparse_expected_log_likelihood: 2d = {two_d} is outside 2, 4, ..., {SPARSE_SITE_MAX_TWO_D}; "
                                  "use sparse_expected_log_likelihood_torch")
    expect = dict(w=(w, batch + (w.shape[-2], two_d)), c=(c, batch + (w.shape[-2],)), y=(y, batch + (w.shape[-2],)),
                  pair_mean=(pair_mean, batch + (segs, two_d)), pair_cov=(pair_cov, batch + (segs, two_d, two_d)))
    for name, (t, shape) in expect.items():
        if tuple(t.shape) != shape:
            raise ValueError(f"sparse_expected_log_likelihood: {name} has shape {tuple(t.shape)}, expected {shape}")
    _lib.same_dtype_device(w, "sparse_expected_log_likelihood", c=c, y=y, pair_mean=pair_mean, pair_cov=pair_cov)
    if torch.is_grad_enabled() and (w.requires_grad or c.requires_grad):
        raise NotImplementedError("sparse_expected_log_likelihood has no adjoint onto w and c (a kernel hyper-parameter under the "
                                  "tape): use sparse_expected_log_likelihood_torch")
    if tiles is None:
        tiles = sparse_expectation_tiles(offsets)
    return _SparseExpectedLogLikelihood.apply(pair_mean, pair_cov, likelihood, w, c, y, offsets, tiles)


def sparse_expected_log_likelihood_torch(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                                         indices: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor) -> torch.Tensor:
    """The same quantity as a torch composition, differentiable by autograd in ``pair_mean``, ``pair_cov``, ``w`` and ``c``: gathers
    of the pair marginals by the per-point pair index (``indices [.., N]``), ``likelihood.variational_expectations`` and
    ``index_add_`` over the segments.  It runs on CPU tensors, it is the models' route for ``2d > 18`` and for a kernel
    hyper-parameter under the tape, and it is what ``mf_lik_sparse_expectations_*`` is measured against."""
    fmu, fvar, flat = _sparse_point_marginals(w, c, indices, pair_mean, pair_cov, pair_mean.shape[-2])
    ve = likelihood.variational_expectations(fmu[..., None], fvar[..., None], y[..., None])
    out = torch.zeros(math.prod(pair_mean.shape[:-1]), dtype=ve.dtype, device=ve.device).index_add(0, flat, ve.reshape(-1))
    return out.reshape(pair_mean.shape[:-1])


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
    ``q`` is trained with any torch optimiser on ``trainable_variables`` or with ``ssm_natgrad.SSMNaturalGradient`` on ``dist_q``."""

    def __init__(self, kernel: SDEKernel, likelihood: Likelihood, inducing_points: torch.Tensor, num_data: Optional[int] = None,
                 initial_distribution: Optional[StateSpaceModel] = None) -> None:
        """
        :param inducing_points: ``batch + [num_inducing]``, sorted, at least two (a ``StateSpaceModel`` needs a transition).
        :param num_data: the total number of observations per series when ``elbo`` is fed minibatches.
        :param initial_distribution: the initial ``q`` on the inducing points; the prior by default.
        """
        super().__init__(kernel, likelihood, inducing_points, min_inducing=2)
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
    def _fused(self, time_points: torch.Tensor) -> bool:
        return (time_points.is_cuda and 2 * self._kernel.state_dim <= SPARSE_SITE_MAX_TWO_D and not self._kernel._needs_grad())

    def _compute_projections(self, time_points: torch.Tensor):
        """``(order | None, w, c, indices, offsets, tiles)`` of the data: the permutation that sorts each series (None for sorted
        data), ``sparse_site_projections`` of the sorted points and the tile table."""
        order, time_points = _sorted_series(time_points)
        w, c, indices, offsets = sparse_site_projections(self._kernel, time_points, self.inducing_inputs)
        tiles = sparse_expectation_tiles(offsets) if time_points.is_cuda else None
        return order, w, c, indices, offsets, tiles

    def _pair_marginals(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(m_pair [.., M+1, 2d], S_pair [.., M+1, 2d, 2d])`` of ``dist_q`` - under the tape when its leaves require a gradient -
        with the stationary prior beyond both ends."""
        return conditionals.pairwise_marginals(self._dist_q, *self._stationary_prior())

    def _expected_log_likelihood(self, time_points: torch.Tensor, observations: torch.Tensor) -> torch.Tensor:
        """``sum_i E_q log p(y_i | f_i)`` per pair, ``batch + [M + 1]``."""
        pair_mean, pair_cov = self._pair_marginals()
        if self._fused(time_points):
            order, w, c, _, offsets, tiles = self._projections(time_points)
            y = observations[..., 0]
            if order is not None:
                y = torch.gather(y, -1, order)
            return sparse_expected_log_likelihood(self._likelihood, w, c, y, offsets, pair_mean, pair_cov, tiles=tiles)
        if self._kernel._needs_grad():
            # a hyper-parameter under the tape: w and c are part of the graph
            order, time_points = _sorted_series(time_points)
            proj, cov, indices = conditionals._conditional_statistics(time_points, self.inducing_inputs, self._kernel)
            h = self._kernel.generate_emission_model(time_points).emission_matrix
            w, c = (h @ proj)[..., 0, :], (h @ cov @ h.transpose(-1, -2))[..., 0, 0]
        else:
            order, w, c, indices, _, _ = self._projections(time_points)
        y = observations[..., 0]
        if order is not None:
            y = torch.gather(y, -1, order)
        return sparse_expected_log_likelihood_torch(self._likelihood, w, c, y, indices, pair_mean, pair_cov)

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
        """Posterior mean and variance of ``f`` at ``new_time_points`` (sorted), ``batch + [num_new, 1]`` each."""
        with torch.no_grad():
            return self._posterior.predict_f(new_time_points, full_output_cov)

    _predict_f = predict_f          # (``predict_log_density`` predicts outside the tape here, as ``predict_f`` does)


# ---- importance-weighted VI: the data term of the log weights ----------------------------------------------------------------------
IW_SAMPLE_CHUNK = 8             # mf_lik_iw_log_weights_*: samples per block of pass 1


def _segments_of(offsets: torch.Tensor, n: int) -> torch.Tensor:
    """The segment of every point ``0 ... n - 1`` from the segment ``offsets [.., S + 1]``: the number of inner offsets ``<= n``."""
    points = torch.arange(n, device=offsets.device).expand(tuple(offsets.shape[:-1]) + (n,)).contiguous()
    return torch.searchsorted(offsets[..., 1:-1].contiguous(), points, right=True)


def iw_merged_time_points(time_points_sorted: torch.Tensor, inducing_points: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """The merged, sorted time points ``[.., N + M]`` of the data (``[.., N]``, sorted) and the inducing points (``[.., M]``) in the
    layout of ``mf_lik_iw_log_weights_*``: data point ``n`` of segment ``s`` at row ``n + s``, inducing point ``m`` at row
    ``offsets[m + 1] + m`` (``offsets [.., M + 2]`` of ``sparse_site_projections``: points with ``x <= z_m`` precede ``z_m``).  Two
    scatters, no argsort."""
    n, m = time_points_sorted.shape[-1], inducing_points.shape[-1]
    rows_x = torch.arange(n, device=offsets.device) + _segments_of(offsets, n)
    rows_z = offsets[..., 1:-1] + torch.arange(m, device=offsets.device)
    merged = torch.empty(tuple(offsets.shape[:-1]) + (n + m,), dtype=inducing_points.dtype, device=inducing_points.device)
    merged.scatter_(-1, rows_x, time_points_sorted.to(inducing_points.dtype))
    merged.scatter_(-1, rows_z, inducing_points)
    return merged


def _iw_log_weights_launch(likelihood: Likelihood, h, w, y, offsets, tiles, states, u_post, want_value: bool, want_grad: bool):
    """ONE call of ``mf_lik_iw_log_weights_*``: ``(log_lik [K, .., S] | None, g_u [K, .., M, d] | None)``."""
    dtype, dev = states.dtype, states.device
    k, d, segs = states.shape[0], states.shape[-1], offsets.shape[-1] - 1
    n = y.shape[-1]
    batch = tuple(offsets.shape[:-1])
    bsz = offsets.numel() // (segs + 1)
    num_tiles, tile_seg, seg_tile = tiles
    log_lik = torch.empty((k,) + batch + (segs,), dtype=dtype, device=dev) if want_value else None
    g_u = torch.empty((k,) + batch + (segs - 1, d), dtype=dtype, device=dev) if want_grad else None
    ws_bytes = int(_lib.load().mf_lik_iw_log_weights_workspace_bytes(num_tiles, k, 2 * d, states.element_size()))
    ws = _lib.workspace(ws_bytes, dev)
    _lib.call("mf_lik_iw_log_weights", dtype, bsz, n, segs, 2 * d, k, likelihood._id, likelihood._c_params(),
              _lib.ptr(offsets.contiguous()), _lib.ptr(None if w is None else w.contiguous()), _lib.ptr(y.contiguous()),
              _lib.ptr(h.contiguous()), _lib.ptr(states.contiguous()), _lib.ptr(None if u_post is None else u_post.contiguous()),
              num_tiles, _lib.ptr(tile_seg), _lib.ptr(seg_tile), _lib.ptr(ws), ws_bytes, _lib.ptr(log_lik), _lib.ptr(g_u),
              _lib.stream_ptr(dev))
    return log_lik, g_u


class _IWLogLikelihood(torch.autograd.Function):
    """Value ``[K, batch...]``; the adjoint onto ``u_post`` comes out of the same launch and waits for the backward."""

    @staticmethod
    def forward(ctx, u_post, likelihood, h, w, y, offsets, tiles, states):
        want = ctx.needs_input_grad[0]
        with torch.no_grad():
            log_lik, g_u = _iw_log_weights_launch(likelihood, h.detach(), w.detach(), y.detach(), offsets, tiles, states.detach(),
                                                  u_post.detach(), True, want)
        if want:
            ctx.save_for_backward(g_u)
        return torch.sum(log_lik, dim=-1)

    @staticmethod
    def backward(ctx, grad_out):
        if torch.is_grad_enabled():
            raise RuntimeError("iw_log_likelihood is differentiable once: its backward uses the adjoint computed in the forward and "
                               "has no second-order support (create_graph=True)")
        (g_u,) = ctx.saved_tensors
        return (grad_out[..., None, None] * g_u,) + (None,) * 7


def iw_log_likelihood(likelihood: Likelihood, h: torch.Tensor, w: Optional[torch.Tensor], y: torch.Tensor, offsets: torch.Tensor,
                      states: torch.Tensor, u_post: Optional[torch.Tensor], tiles=None) -> torch.Tensor:
    """``sum_n log p(y_n | f_n)`` of ``K`` samples, ``[K, batch...]``: ONE call of ``mf_lik_iw_log_weights_*`` on HIP tensors, ``2d <= 18``.
    With ``u_post [K, .., M, d]`` (a draw from ``q`` at the inducing points) ``states [K, .., N + M, d]`` is a prior draw on
    ``iw_merged_time_points`` and the kernel applies Matheron's correction through ``w [.., N, 2d]`` (``sparse_site_projections``),
    ``f_n = h . prior(x_n) - w[n, :d] . (prior(z_-) - u_-) - w[n, d:] . (prior(z_+) - u_+)``; ``u_post`` = None: ``states [K, .., N, d]`` holds
    final samples (``w`` is not read).  ``h [d]`` is the emission row, ``y [.., N]``, ``offsets [.., M + 2]``.  Differentiable ONCE in
    ``u_post`` - the backward multiplies the adjoint the forward computed beside the value, there is no second launch; not
    differentiable in ``states``, ``w`` and ``h``.  ``tiles``: ``sparse_expectation_tiles(offsets)`` when the caller keeps it."""
    if not isinstance(likelihood, Likelihood):
        raise TypeError("likelihood must be a markovflow_amd.likelihoods.Likelihood")
    d, segs = states.shape[-1], offsets.shape[-1] - 1
    batch, k, n = tuple(offsets.shape[:-1]), states.shape[0], y.shape[-1]
    if 2 * d > SPARSE_SITE_MAX_TWO_D:
        raise NotImplementedError(f"iw_log_likelihood: 2d = {2 * d} is outside 2, 4, ..., {SPARSE_SITE_MAX_TWO_D}; use "
                                  "iw_log_likelihood_torch")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (states, w, h)):
        raise NotImplementedError("iw_log_likelihood has no adjoint onto states, w and h (a kernel hyper-parameter under the tape): "
                                  "use iw_log_likelihood_torch")
    rows = n if u_post is None else n + segs - 1
    expect = dict(h=(h, (d,)), y=(y, batch + (n,)), states=(states, (k,) + batch + (rows, d)))
    if u_post is not None:
        expect.update(w=(w, batch + (n, 2 * d)), u_post=(u_post, (k,) + batch + (segs - 1, d)))
    for name, (t, shape) in expect.items():
        if t is None or tuple(t.shape) != shape:
            raise ValueError(f"iw_log_likelihood: {name} has shape {None if t is None else tuple(t.shape)}, expected {shape}")
    _lib.same_dtype_device(states, "iw_log_likelihood", h=h, w=w if u_post is not None else None, y=y, u_post=u_post)
    if tiles is None:
        tiles = sparse_expectation_tiles(offsets)
    if u_post is None:
        with torch.no_grad():
            return torch.sum(_iw_log_weights_launch(likelihood, h, None, y, offsets, tiles, states, None, True, False)[0], dim=-1)
    return _IWLogLikelihood.apply(u_post, likelihood, h, w, y, offsets, tiles, states)


def iw_log_likelihood_torch(likelihood: Likelihood, h: torch.Tensor, w: Optional[torch.Tensor], y: torch.Tensor,
                            indices: Optional[torch.Tensor], states: torch.Tensor, u_post: Optional[torch.Tensor]) -> torch.Tensor:
    """The same quantity as a torch composition, differentiable by autograd in everything: gathers of the data rows and the inducing
    rows of the prior draw (from ``indices [.., N]``, the pair every point belongs to), the two ``w . delta`` products, the emission
    product and ``likelihood.log_prob``.  It runs on CPU tensors, it is the models' route for ``2d > 18`` and for a kernel
    hyper-parameter under the tape, and it is what ``mf_lik_iw_log_weights_*`` is measured against."""
    d, n = states.shape[-1], y.shape[-1]
    lead = (states.shape[0],) + tuple(y.shape[:-1])
    if u_post is None:
        f = torch.sum(states * h, dim=-1)
    else:
        m = u_post.shape[-2]
        z_index = torch.arange(m, device=indices.device).expand(tuple(indices.shape[:-1]) + (m,)).contiguous()
        rows_z = torch.searchsorted(indices.contiguous(), z_index, right=True) + z_index          # offsets[m + 1] + m
        rows_x = indices + torch.arange(n, device=indices.device)
        pick = lambda src, idx: torch.gather(src, -2, idx.expand(lead + (idx.shape[-1],))[..., None].expand(lead + (idx.shape[-1], d)))  # noqa: E731
        delta = pick(states, rows_z) - u_post
        pad = torch.zeros_like(delta[..., :1, :])
        delta = torch.cat([pad, delta, pad], dim=-2)          # beyond both ends the correction vanishes
        f = (torch.sum(pick(states, rows_x) * h, dim=-1) - torch.sum(w[..., :d] * pick(delta, indices), dim=-1)
             - torch.sum(w[..., d:] * pick(delta, indices + 1), dim=-1))
    return torch.sum(likelihood.log_prob(f[..., None], y.expand(lead + (n,))[..., None]), dim=-1)


class ImportanceWeightedVI(SparseVariationalGaussianProcess):
    """Importance-weighted VI (markovflow/models/iwvi.py:29-173; Domke and Sheldon 2018; zero mean function): the SVGP model with the
    bound ``L_K = log (1/K) sum_k w_k``, ``w_k = p(y | s_k) p(u_k) / q(u_k)``, ``(s_k, u_k) ~ q(u) p(s | u)``, which tightens with
    ``K`` towards ``log p(y)``.  The proposals are drawn by Matheron's rule; on HIP tensors with ``2d <= 18`` and no kernel
    hyper-parameter under the tape their assembly, the ``K`` evaluations of the likelihood at every data point and the adjoint onto
    the draw from ``q`` are ONE call of ``mf_lik_iw_log_weights_*``."""

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
            ve_sum = torch.empty((bsz,), dtype=dtype, device=dev)
            g_mu = torch.empty((bsz, n), dtype=dtype, device=dev) if want else None
            g_var = torch.empty((bsz, n), dtype=dtype, device=dev) if want else None
            ws_bytes = int(_lib.load().mf_lik_dense_expectations_workspace_bytes(bsz, n, h.element_size()))
            ws = _lib.workspace(ws_bytes, dev)
            _lib.call("mf_lik_dense_expectations", dtype, bsz, n, d, *likelihood._kernel_args(), _lib.ptr(h),
                      _lib.ptr(means.detach().contiguous()), _lib.ptr(covs.detach().contiguous()), _lib.ptr(y), _lib.ptr(ws), ws_bytes,
                      _lib.ptr(ve_sum), _lib.ptr(g_mu), _lib.ptr(g_var), _lib.stream_ptr(dev))
        if want:
            ctx.save_for_backward(h, g_mu, g_var)
        return ve_sum

    @staticmethod
    def backward(ctx, grad_out):
        if torch.is_grad_enabled():
            raise RuntimeError("dense_expected_log_likelihood is differentiable once: its backward uses the adjoints computed in "
                               "the forward and has no second-order support (create_graph=True)")
        h, g_mu, g_var = ctx.saved_tensors
        bsz, n, d = h.shape
        g_means = torch.empty((bsz, n, d), dtype=h.dtype, device=h.device) if ctx.needs_input_grad[0] else None
        g_covs = torch.empty((bsz, n, d, d), dtype=h.dtype, device=h.device) if ctx.needs_input_grad[1] else None
        _lib.call("mf_lik_dense_expectations_adjoint", h.dtype, bsz, n, d, _lib.ptr(h), _lib.ptr(g_mu), _lib.ptr(g_var),
                  _lib.ptr(grad_out.contiguous()), _lib.ptr(g_means), _lib.ptr(g_covs), _lib.stream_ptr(h.device))
        return g_means, g_covs, None, None, None


def _check_dense(what: str, likelihood: Likelihood, h: torch.Tensor, y: torch.Tensor, means: torch.Tensor, covs: torch.Tensor):
    if not isinstance(likelihood, Likelihood):
        raise TypeError("likelihood must be a markovflow_amd.likelihoods.Likelihood")
    if h.dim() < 2:
        raise ValueError(f"{what}: h must have shape batch + [N, d], got {tuple(h.shape)}")
    if h.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {h.dtype}")
    batch, n, d = tuple(h.shape[:-2]), h.shape[-2], h.shape[-1]
    expect = dict(y=(y, batch + (n,)), means=(means, batch + (n, d)), covs=(covs, batch + (n, d, d)))
    for name, (t, shape) in expect.items():
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {shape}")
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


class VariationalGaussianProcess:
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
        if not isinstance(likelihood, Likelihood):
            raise TypeError("likelihood must be a markovflow_amd.likelihoods.Likelihood")
        if observations.dim() < 2 or observations.shape[-1] != 1:
            raise ValueError(f"observations must have shape batch + [num_data, 1], got {tuple(observations.shape)}")
        if tuple(time_points.shape) != tuple(observations.shape[:-1]):
            raise ValueError("time_points must have shape observations.shape[:-1]")
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
    def kernel(self) -> SDEKernel:
        return self._kernel

    @property
    def likelihood(self) -> Likelihood:
        return self._likelihood

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

    def predict_log_density(self, input_data: Tuple[torch.Tensor, torch.Tensor], full_output_cov: bool = False) -> torch.Tensor:
        """Log density of new data ``(time_points, observations)`` under the posterior, ``batch + [num_new]``."""
        if full_output_cov:
            raise NotImplementedError("predict_log_density: the likelihoods are univariate (marginal variances only)")
        new_times, new_obs = input_data
        f_mean, f_var = self.predict_f(new_times)
        return self._likelihood.predict_log_density(f_mean, f_var, new_obs)


# ---- the spatio-temporal sparse variational model: the ELBO's data term ------------------------------------------------------------
ST_EXPECT_TILE = 256            # mf_lik_st_expectations_*: points per workspace row of pass 1 (four groups of 64)


def _st_dims(what: str, a: torch.Tensor, wt: torch.Tensor) -> Tuple[int, int]:
    """``(Ms, two_dt)`` of the spatial weights and temporal projections, checked against the kernel's range."""
    ms, two_dt = a.shape[-1], wt.shape[-1]
    if ms < 1 or two_dt < 2 or two_dt % 2 or ms * (two_dt // 2) > ST_MAX_STATE_DIM:
        raise NotImplementedError(f"{what}: Ms = {ms}, 2 d_t = {two_dt} is outside Ms >= 1, d_t >= 1, Ms d_t <= {ST_MAX_STATE_DIM}")
    return ms, two_dt


def _st_check(what: str, likelihood, a, wt, c, y, lead, segs, pair_mean, pair_cov) -> Tuple[int, int]:
    if not isinstance(likelihood, Likelihood):
        raise TypeError("likelihood must be a markovflow_amd.likelihoods.Likelihood")
    ms, two_dt = _st_dims(what, a, wt)
    n, pair = a.shape[-2], ms * two_dt
    expect = dict(a=(a, lead + (n, ms)), wt=(wt, lead + (n, two_dt)), c=(c, lead + (n,)), pair_mean=(pair_mean, lead + (segs, pair)),
                  pair_cov=(pair_cov, lead + (segs, pair, pair)))
    if y is not None:
        expect["y"] = (y, lead + (n,))
    for name, (t, shape) in expect.items():
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {shape}")
    _lib.same_dtype_device(a, what, wt=wt, c=c, y=y, pair_mean=pair_mean, pair_cov=pair_cov)
    return ms, two_dt


def _st_expectations_launch(likelihood: Likelihood, a, wt, c, y, offsets, tiles, pair_mean, pair_cov, want_value: bool = False,
                            want_grads: bool = False, want_point: bool = False, want_marginals: bool = False):
    """ONE call of ``mf_lik_st_expectations_*``: ``(ve_sum, g_mean, g_cov, g_a, g_wt, g_c, fmu, fvar)``, None for what was not asked."""
    dtype, dev = a.dtype, a.device
    n, ms, two_dt, segs = a.shape[-2], a.shape[-1], wt.shape[-1], offsets.shape[-1] - 1
    pair = ms * two_dt
    batch = tuple(offsets.shape[:-1])
    bsz = offsets.numel() // (segs + 1)
    num_tiles, tile_seg, seg_tile = tiles
    new = lambda want, *shape: torch.empty(batch + shape, dtype=dtype, device=dev) if want else None      # noqa: E731
    ve_sum = new(want_value, segs)
    g_mean, g_cov = new(want_grads, segs, pair), new(want_grads, segs, pair, pair)
    g_a, g_wt, g_c = new(want_point, n, ms), new(want_point, n, two_dt), new(want_point, n)
    fmu, fvar = new(want_marginals, n), new(want_marginals, n)
    ws_bytes = int(_lib.load().mf_lik_st_expectations_workspace_bytes(num_tiles, ms, two_dt, a.element_size())) \
        if want_value or want_grads else 0
    ws = _lib.workspace(ws_bytes, dev)
    # (contiguous copies are held in locals until the call has been issued: a pointer keeps no tensor alive)
    offsets, a, wt, c, pair_mean, pair_cov = (t.contiguous() for t in (offsets, a, wt, c, pair_mean, pair_cov))
    y = None if y is None else y.contiguous()
    _lib.call("mf_lik_st_expectations", dtype, bsz, n, segs, ms, two_dt, *likelihood._kernel_args(), _lib.ptr(offsets),
              _lib.ptr(a), _lib.ptr(wt), _lib.ptr(c), _lib.ptr(y), _lib.ptr(pair_mean), _lib.ptr(pair_cov),
              num_tiles, _lib.ptr(tile_seg), _lib.ptr(seg_tile), _lib.ptr(ws), ws_bytes, _lib.ptr(ve_sum), _lib.ptr(g_mean),
              _lib.ptr(g_cov), _lib.ptr(g_a), _lib.ptr(g_wt), _lib.ptr(g_c), _lib.ptr(fmu), _lib.ptr(fvar), _lib.stream_ptr(dev))
    return ve_sum, g_mean, g_cov, g_a, g_wt, g_c, fmu, fvar


class _STExpectedLogLikelihood(torch.autograd.Function):
    """Value ``batch + [M + 1]``; every adjoint that is needed comes out of the same launch and waits for the backward."""

    @staticmethod
    def forward(ctx, pair_mean, pair_cov, a, wt, c, likelihood, y, offsets, tiles):
        want_grads = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        want_point = any(ctx.needs_input_grad[2:5])
        with torch.no_grad():
            out = _st_expectations_launch(likelihood, a.detach(), wt.detach(), c.detach(), y.detach(), offsets, tiles,
                                          pair_mean.detach(), pair_cov.detach(), True, want_grads, want_point)
        ctx.want = (want_grads, want_point)
        ctx.save_for_backward(*[t for t in out[1:6] if t is not None], offsets)
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        if torch.is_grad_enabled():
            raise RuntimeError("st_expected_log_likelihood is differentiable once: its backward uses the adjoints computed in the "
                               "forward and has no second-order support (create_graph=True)")
        saved = list(ctx.saved_tensors)
        offsets = saved.pop()
        grads = [None] * 5
        if ctx.want[0]:
            g_mean, g_cov = saved[:2]
            saved = saved[2:]
            grads[0] = grad_out[..., None] * g_mean if ctx.needs_input_grad[0] else None
            grads[1] = grad_out[..., None, None] * g_cov if ctx.needs_input_grad[1] else None
        if ctx.want[1]:
            g_a, g_wt, g_c = saved
            per_point = torch.gather(grad_out, -1, _segments_of(offsets, g_c.shape[-1]))      # the point's segment
            grads[2] = per_point[..., None] * g_a if ctx.needs_input_grad[2] else None
            grads[3] = per_point[..., None] * g_wt if ctx.needs_input_grad[3] else None
            grads[4] = per_point * g_c if ctx.needs_input_grad[4] else None
        return tuple(grads) + (None, None, None, None)


def st_expected_log_likelihood(likelihood: Likelihood, a: torch.Tensor, wt: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                               offsets: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor, tiles=None) -> torch.Tensor:
    """``sum_k E_q log p(y_k | f_k)`` per pair of neighbouring inducing states, ``batch + [M + 1]``, for a chain of ``Ms`` copies of a
    ``d_t``-dimensional temporal state (``D = Ms d_t <= 64``): with ``W_k[half D + s d_t + i] = a_k[s] wt_k[half d_t + i]``,
    ``fmu = W_k . m_s`` and ``fvar = c_k + W_k^T S_s W_k`` for the points ``offsets[s] <= k < offsets[s + 1]`` of pair ``s``
    (``a [.., N, Ms]``, ``wt [.., N, 2 d_t]``, ``c``, ``y`` ``[.., N]``, ``offsets [.., M + 2]``, ``pair_mean [.., M + 1, 2D]``,
    ``pair_cov [.., M + 1, 2D, 2D]``).  ONE call of ``mf_lik_st_expectations_*`` on HIP tensors.  Differentiable ONCE in ``pair_mean``,
    ``pair_cov`` (an unconstrained matrix: the gradient is symmetric), ``a``, ``wt`` and ``c`` - the backward multiplies the adjoints
    the forward computed beside the value by ``grad_out`` (of the segment, or of the point's segment); there is no second launch.
    ``tiles``: ``sparse_expectation_tiles(offsets, ST_EXPECT_TILE)`` when the caller keeps it."""
    segs = offsets.shape[-1] - 1
    _st_check("st_expected_log_likelihood", likelihood, a, wt, c, y, tuple(offsets.shape[:-1]), segs, pair_mean, pair_cov)
    if tiles is None:
        tiles = sparse_expectation_tiles(offsets, ST_EXPECT_TILE)
    return _STExpectedLogLikelihood.apply(pair_mean, pair_cov, a, wt, c, likelihood, y, offsets, tiles)


def _st_kron_rows(a: torch.Tensor, wt: torch.Tensor) -> torch.Tensor:
    """``W [B N, 2 Ms d_t]`` with ``W[k, half D + s d_t + i] = a[k, s] wt[k, half d_t + i]``, the batch flattened."""
    ms, two_dt = a.shape[-1], wt.shape[-1]
    return (wt.reshape(tuple(a.shape[:-1]) + (2, 1, two_dt // 2)) * a[..., None, :, None]).reshape(-1, ms * two_dt)


def _st_torch_marginals(a, wt, c, indices, pair_mean, pair_cov) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per point ``fmu`` and ``fvar`` (``[.., N]`` each) and the flat segment index ``[B N]`` in differentiable torch: ``W`` is
    ``O(N 2D)``, the symmetrised pair covariance is applied segment by segment (one matrix product per non-empty segment), never
    gathered per point."""
    pair, segs = a.shape[-1] * wt.shape[-1], pair_mean.shape[-2]
    lead, n = tuple(a.shape[:-2]), a.shape[-2]
    w = _st_kron_rows(a, wt)
    series = torch.arange(math.prod(lead), device=indices.device).reshape(lead + (1,))
    flat = (indices + series * segs).reshape(-1)
    mean = pair_mean.reshape(-1, pair)
    sbar = (0.5 * (pair_cov + pair_cov.transpose(-1, -2))).reshape(-1, pair, pair)
    fmu = torch.sum(w * mean[flat], dim=-1)
    order = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=mean.shape[0]).tolist()
    chunks, start = [], 0
    w_sorted = w[order]
    for s, count in enumerate(counts):
        if count:
            rows = w_sorted[start:start + count]
            chunks.append(torch.sum(rows * (rows @ sbar[s]), dim=-1))
            start += count
    quad_sorted = torch.cat(chunks) if chunks else w.new_zeros(0)
    quad = quad_sorted[torch.argsort(order)]
    return fmu.reshape(lead + (n,)), c + quad.reshape(lead + (n,)), flat


def st_expected_log_likelihood_torch(likelihood: Likelihood, a: torch.Tensor, wt: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                                     indices: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor) -> torch.Tensor:
    """The same quantity as a torch composition with the per-point pair index (``indices [.., N]``) in place of the offsets,
    differentiable by autograd in ``pair_mean``, ``pair_cov``, ``a``, ``wt`` and ``c``.  It runs on CPU tensors and is what
    ``mf_lik_st_expectations_*`` is measured against.  Memory is ``O(N 2D)`` plus one ``2D x 2D`` product per non-empty segment."""
    _st_check("st_expected_log_likelihood_torch", likelihood, a, wt, c, y, tuple(indices.shape[:-1]), pair_mean.shape[-2], pair_mean,
              pair_cov)
    fmu, fvar, flat = _st_torch_marginals(a, wt, c, indices, pair_mean, pair_cov)
    ve = likelihood.variational_expectations(fmu[..., None], fvar[..., None], y[..., None])
    out = torch.zeros(math.prod(pair_mean.shape[:-1]), dtype=ve.dtype, device=ve.device).index_add(0, flat, ve.reshape(-1))
    return out.reshape(pair_mean.shape[:-1])


def st_point_marginals(a: torch.Tensor, wt: torch.Tensor, c: torch.Tensor, offsets: torch.Tensor, pair_mean: torch.Tensor,
                       pair_cov: torch.Tensor, tiles=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(fmu, fvar)``, ``[.., N]`` each, of the points of ``st_expected_log_likelihood``: the kernel's projection-only mode on HIP
    tensors (NaN in both where ``fvar`` is not positive), torch otherwise.  Not differentiable."""
    segs = offsets.shape[-1] - 1
    _st_check("st_point_marginals", Gaussian(), a, wt, c, None, tuple(offsets.shape[:-1]), segs, pair_mean, pair_cov)
    with torch.no_grad():
        if a.is_cuda:
            if tiles is None:
                tiles = sparse_expectation_tiles(offsets, ST_EXPECT_TILE)
            return _st_expectations_launch(Gaussian(), a, wt, c, None, offsets, tiles, pair_mean, pair_cov, want_marginals=True)[6:]
        fmu, fvar, _ = _st_torch_marginals(a, wt, c, _segments_of(offsets, a.shape[-2]), pair_mean, pair_cov)
        return fmu, fvar


# ---- the spatio-temporal sparse CVI model: the site update ---------------------------------------------------------------------------
def _st_check_sites(what: str, a, lead, segs: int, pair: int, learning_rate, nat1, nat2) -> float:
    for name, t, shape in (("nat1", nat1, lead + (segs, pair)), ("nat2", nat2, lead + (segs, pair, pair))):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError(f"{what}: {name} must be a tensor of shape {shape}")
    _lib.same_dtype_device(a, what, nat1=nat1, nat2=nat2)
    lr = float(learning_rate)
    if not 0.0 <= lr <= 1.0:
        raise ValueError(f"{what}: learning_rate must lie in [0, 1], got {learning_rate}")
    return lr


def st_cvi_site_update_torch(likelihood: Likelihood, a: torch.Tensor, wt: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                             indices: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor, learning_rate: float,
                             nat1: torch.Tensor, nat2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The spatio-temporal CVI step as a torch composition (spatio_temporal_variational.py:509-552), IN PLACE on
    ``nat1 [.., Mt+1, 2D]`` and ``nat2 [.., Mt+1, 2D, 2D]``: the marginals of ``_st_torch_marginals``, the likelihood's
    ``(ve, gm, gv)``, ``gradient_transformation_mean_var_to_expectation`` (``g1 = gm - 2 gv fmu``, ``g2 = gv``),
    ``theta_1 = sum_k g1_k W_k`` over the per-point pair index (``indices [.., N]``) and ``theta_2 = sum_k gv_k W_k W_k^T`` formed
    segment by segment as ``W_s^T diag(gv) W_s`` (memory ``O(N 2D)`` plus one ``2D x 2D`` product per non-empty segment, never
    ``[N, 2D, 2D]``); ``nat <- (1 - lr) nat + lr sum``.  A point with ``fvar`` not positive has NaN in its marginals and makes the
    sites of its segment NaN, as in ``sparse_cvi_site_update_torch``.  What ``mf_lik_st_cvi_site_update_*`` fuses: it runs on CPU
    tensors, it is the model's route there and it is what the kernel is measured against.  Returns ``(ve_sum [.., Mt+1], fmu, fvar
    [.., N])``."""
    segs = pair_mean.shape[-2]
    lead = tuple(indices.shape[:-1])
    ms, two_dt = _st_check("st_cvi_site_update_torch", likelihood, a, wt, c, y, lead, segs, pair_mean, pair_cov)
    pair = ms * two_dt
    lr = _st_check_sites("st_cvi_site_update_torch", a, lead, segs, pair, learning_rate, nat1, nat2)
    with torch.no_grad():
        fmu, fvar, flat = _st_torch_marginals(a, wt, c, indices, pair_mean, pair_cov)
        ve, g_mu, g_var = likelihood._expectations(fmu[..., None], fvar[..., None], y[..., None])
        nan = torch.full_like(fvar, float("nan"))
        bad = ~(fvar > 0)
        fmu, fvar = torch.where(bad, nan, fmu), torch.where(bad, nan, fvar)
        ve, g_mu, g_var = (torch.where(bad[..., None], nan[..., None], v) for v in (ve, g_mu, g_var))
        g1, g2 = gradient_transformation_mean_var_to_expectation((fmu[..., None], fvar[..., None]), (g_mu, g_var))
        w = _st_kron_rows(a, wt)
        rows_total = math.prod(lead) * segs
        sum1 = torch.zeros(rows_total, pair, dtype=w.dtype, device=w.device).index_add_(0, flat, g1.reshape(-1, 1) * w)
        sum2 = torch.zeros(rows_total, pair, pair, dtype=w.dtype, device=w.device)
        order = torch.argsort(flat, stable=True)
        w_sorted, g2_sorted = w[order], g2.reshape(-1, 1)[order]
        start = 0
        for s, count in enumerate(torch.bincount(flat, minlength=rows_total).tolist()):
            if count:
                rows = w_sorted[start:start + count]
                sum2[s] = rows.transpose(-1, -2) @ (g2_sorted[start:start + count] * rows)
                start += count
        ve_sum = torch.zeros(rows_total, dtype=w.dtype, device=w.device).index_add_(0, flat, ve.reshape(-1))
        nat1.mul_(1.0 - lr).add_(lr * sum1.reshape(nat1.shape))
        nat2.mul_(1.0 - lr).add_(lr * sum2.reshape(nat2.shape))
    return ve_sum.reshape(lead + (segs,)), fmu, fvar


def st_cvi_site_update_hip(likelihood: Likelihood, a: torch.Tensor, wt: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                           offsets: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor, learning_rate: float,
                           nat1: torch.Tensor, nat2: torch.Tensor, tiles=None, want_outputs: bool = False):
    """ONE call of ``mf_lik_st_cvi_site_update_*`` on HIP tensors (``Ms d_t <= 64``): what ``st_cvi_site_update_torch`` computes,
    with the segment ``offsets [.., Mt + 2]`` in place of the per-point index; ``nat1`` / ``nat2`` (contiguous) are updated IN
    PLACE.  ``want_outputs``: return ``(ve_sum [.., Mt+1], fmu, fvar [.., N])`` (else three Nones).  ``tiles``:
    ``sparse_expectation_tiles(offsets, ST_EXPECT_TILE)`` when the caller keeps it."""
    what = "st_cvi_site_update_hip"
    segs = offsets.shape[-1] - 1
    lead = tuple(offsets.shape[:-1])
    ms, two_dt = _st_check(what, likelihood, a, wt, c, y, lead, segs, pair_mean, pair_cov)
    lr = _st_check_sites(what, a, lead, segs, ms * two_dt, learning_rate, nat1, nat2)
    if not (nat1.is_contiguous() and nat2.is_contiguous()):
        raise ValueError(f"{what}: nat1 and nat2 must be contiguous")
    dtype, dev, n = a.dtype, a.device, a.shape[-2]
    bsz = offsets.numel() // (segs + 1)
    if tiles is None:
        tiles = sparse_expectation_tiles(offsets, ST_EXPECT_TILE)
    num_tiles, tile_seg, seg_tile = tiles
    new = lambda *shape: torch.empty(lead + shape, dtype=dtype, device=dev) if want_outputs else None      # noqa: E731
    outs = (new(segs), new(n), new(n))
    ws_bytes = int(_lib.load().mf_lik_st_cvi_site_update_workspace_bytes(num_tiles, ms, two_dt, a.element_size()))
    ws = _lib.workspace(ws_bytes, dev)
    # (contiguous copies are held in locals until the call has been issued: a pointer keeps no tensor alive)
    offsets, a, wt, c, y, pair_mean, pair_cov = (t.contiguous() for t in (offsets, a, wt, c, y, pair_mean, pair_cov))
    _lib.call("mf_lik_st_cvi_site_update", dtype, bsz, n, segs, ms, two_dt, *likelihood._kernel_args(), _lib.ptr(offsets),
              _lib.ptr(a), _lib.ptr(wt), _lib.ptr(c), _lib.ptr(y), _lib.ptr(pair_mean), _lib.ptr(pair_cov), num_tiles,
              _lib.ptr(tile_seg), _lib.ptr(seg_tile), _lib.ptr(ws), ws_bytes, lr, _lib.ptr(nat1), _lib.ptr(nat2),
              *[_lib.ptr(o) for o in outs], _lib.stream_ptr(dev))
    # the kernel wrote through raw pointers: tell torch, so that whatever keys a cache on (tensor, version) sees the write
    torch.autograd.graph.increment_version(nat1)
    torch.autograd.graph.increment_version(nat2)
    return outs


class _SpatioTemporalData:
    """What the two spatio-temporal models share, mixed in ahead of their inducing-point base: the checks on ``(X, Y)`` with time in
    the last column of ``X``, the sort-on-a-copy rule, the cache of the per-point projections ``(a, wt, c)``, the pair marginals of
    ``dist_q`` with the float64 limit of the chain operators, the ELBO's data term and the predictions."""

    @property
    def inducing_time(self) -> torch.Tensor:
        return self.inducing_inputs

    @property
    def inducing_space(self) -> torch.Tensor:
        return self._kernel.inducing_space

    # ---- data --------------------------------------------------------------------------------------------------------------------
    def _check_data(self, input_data: Tuple[torch.Tensor, torch.Tensor], what: str) -> Tuple[torch.Tensor, torch.Tensor]:
        inputs, observations = input_data
        self._check_inputs(inputs, what)
        if observations.dim() < 2 or observations.shape[-1] != 1 or tuple(observations.shape[:-1]) != tuple(inputs.shape[:-1]):
            raise ValueError(f"{what}: observations must have shape inputs.shape[:-1] + [1], got {tuple(observations.shape)}")
        _lib.same_dtype_device(self.inducing_inputs, f"{type(self).__name__}.{what}", observations=observations)
        return inputs, observations

    def _check_inputs(self, inputs: torch.Tensor, what: str) -> None:
        width = self.inducing_space.shape[-1] + 1
        if inputs.dim() < 2 or inputs.shape[-1] != width:
            raise ValueError(f"{what}: inputs must have shape batch + [num_data, {width}] (time in the last column), got "
                             f"{tuple(inputs.shape)}")
        if tuple(inputs.shape[:-2]) != tuple(self.inducing_inputs.shape[:-1]):
            raise ValueError(f"{what}: the data must carry the batch shape of the inducing times, "
                             f"{tuple(self.inducing_inputs.shape[:-1])}, got {tuple(inputs.shape[:-2])}")
        _lib.same_dtype_device(self.inducing_inputs, f"{type(self).__name__}.{what}", inputs=inputs)

    def _fused(self, inputs: torch.Tensor) -> bool:
        """HIP tensors take the kernel, whatever requires a gradient (``Ms d_t <= 64`` holds by construction)."""
        return inputs.is_cuda

    def _hyper_leaves(self):
        return ([x for comp in self._kernel._components() for x in comp._leaves()] + list(self._kernel.kernel_space._leaves())
                + [self._kernel.inducing_space])

    def _hyper_needs_grad(self) -> bool:
        return torch.is_grad_enabled() and any(x.requires_grad for x in self._hyper_leaves())

    def _projections(self, inputs: torch.Tensor):
        """``_compute_projections`` of the data, kept until the data, the inducing times, the inducing locations or a hyper-parameter
        of either kernel is replaced or written in place (tensor identity, data pointer and version counter)."""
        sources = [inputs, self.inducing_inputs] + self._hyper_leaves()
        key = tuple(_version_key(x) for x in sources)
        cached = self._projection_cache
        if (cached is not None and None not in key and cached[0] == key and len(cached[1]) == len(sources)
                and all(a is b for a, b in zip(cached[1], sources))):
            return cached[2]
        with torch.no_grad():
            out = self._compute_projections(inputs)
        self._projection_cache = (key, sources, out)
        return out

    def _compute_projections(self, inputs: torch.Tensor):
        """``(order | None, a, wt, c, indices, offsets, tiles)`` of the data: the permutation that sorts each series by time (None
        for sorted data), the spatial weights ``a = L^-1 K_s(Z_s, x)``, ``sparse_site_projections`` of the temporal kernel,
        ``c = K_s(x, x) - |a|^2 (1 - ct)`` and the row table.  Differentiable when called under the tape."""
        space, times = inputs[..., :-1], inputs[..., -1]
        order, times = _sorted_series(times)
        if order is not None:
            space = torch.gather(space, -2, order[..., None].expand(space.shape))
        kernel = self._kernel
        if kernel.kernel_time._needs_grad():
            proj, cov, indices = conditionals._conditional_statistics(times, self.inducing_inputs, kernel.kernel_time)
            h = kernel.kernel_time.generate_emission_model(times).emission_matrix
            wt, ct = (h @ proj)[..., 0, :], (h @ cov @ h.transpose(-1, -2))[..., 0, 0]
            with torch.no_grad():
                offsets = _site_offsets(times, self.inducing_inputs)
        else:
            wt, ct, indices, offsets = sparse_site_projections(kernel.kernel_time, times, self.inducing_inputs)
        a = kernel.space_weights(space)
        c = kernel.kernel_space.K_diag(space) - torch.sum(a * a, dim=-1) * (1.0 - ct)
        tiles = sparse_expectation_tiles(offsets, ST_EXPECT_TILE) if inputs.is_cuda else None
        return order, a.contiguous(), wt.contiguous(), c.contiguous(), indices, offsets, tiles

    def _pair_marginals(self, dist_q: Optional[StateSpaceModel] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(m_pair [.., Mt+1, 2D], S_pair [.., Mt+1, 2D, 2D])`` of ``dist_q`` (the model's own by default) with the stationary
        prior beyond both ends."""
        self._check_chain_limit()
        return conditionals.pairwise_marginals(self.dist_q if dist_q is None else dist_q, *self._stationary_prior())

    def _check_chain_limit(self) -> None:
        limit = _lib.load().mf_max_state_dim_f64_tile_ops()
        if self.inducing_inputs.dtype == torch.float64 and self._kernel.state_dim > limit:
            # mf_lik_st_expectations_* carries Ms d_t <= 64; the chain's marginals, their adjoint and the KL do not
            raise NotImplementedError(f"{type(self).__name__}: the chain operators (marginals, KL divergence and their "
                                      f"adjoints) carry state dimensions up to {limit} in float64, Ms d_t = {self._kernel.state_dim}")

    def _expected_log_likelihood(self, inputs: torch.Tensor, observations: torch.Tensor,
                                 dist_q: Optional[StateSpaceModel] = None) -> torch.Tensor:
        """``sum_i E_q log p(y_i | f_i)`` per pair, ``batch + [Mt + 1]``."""
        pair_mean, pair_cov = self._pair_marginals(dist_q)
        # a hyper-parameter under the tape: the projections are part of the graph, and the kernel's per-point adjoints carry it
        proj = self._compute_projections(inputs) if self._hyper_needs_grad() else self._projections(inputs)
        order, a, wt, c, indices, offsets, tiles = proj
        y = observations[..., 0]
        if order is not None:
            y = torch.gather(y, -1, order)
        if self._fused(inputs):
            return st_expected_log_likelihood(self._likelihood, a, wt, c, y, offsets, pair_mean, pair_cov, tiles=tiles)
        return st_expected_log_likelihood_torch(self._likelihood, a, wt, c, y, indices, pair_mean, pair_cov)

    def space_time_predict_f(self, inputs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Posterior mean and variance of ``f`` at ``inputs [.., N, Dx + 1]`` (any order in time), ``batch + [N, 1]`` each
        (spatio_temporal_variational.py:149-183; the same numbers up to rounding, without an ``Ms x Ms`` Cholesky per point)."""
        self._check_inputs(inputs, "space_time_predict_f")
        with torch.no_grad():
            order, a, wt, c, _, offsets, tiles = self._projections(inputs)
            fmu, fvar = st_point_marginals(a, wt, c, offsets, *self._pair_marginals(), tiles=tiles)
            if order is not None:
                inverse = torch.argsort(order, dim=-1)
                fmu, fvar = torch.gather(fmu, -1, inverse), torch.gather(fvar, -1, inverse)
            return fmu[..., None], fvar[..., None]

    def predict_log_density(self, input_data: Tuple[torch.Tensor, torch.Tensor], full_output_cov: bool = False) -> torch.Tensor:
        """Log density of new data ``(inputs, observations)`` under the posterior, ``batch + [num_new]``
        (spatio_temporal_variational.py:238-246)."""
        if full_output_cov:
            raise NotImplementedError("predict_log_density: the likelihoods are univariate (marginal variances only)")
        inputs, observations = self._check_data(input_data, "predict_log_density")
        f_mean, f_var = self.space_time_predict_f(inputs)
        return self._likelihood.predict_log_density(f_mean, f_var, observations)


class SpatioTemporalSparseVariational(_SpatioTemporalData, _SparseGaussianProcess):
    """Sparse variational GP with the product kernel ``k((x, t), (x', t')) = k_s(x, x') k_t(t, t')``
    (markovflow/models/spatio_temporal_variational.py:109-357): space is marginalised to ``Ms`` inducing locations, time to ``Mt``
    inducing times, and ``q`` is a trainable ``StateSpaceModel`` of state dimension ``Ms d_t <= 64`` on the inducing times
    (``kernels.SparseSpatioTemporalKernel``).  The ELBO is ``scale sum_i E_q log p(y_i | f_i) - KL[q || p]``; train ``q`` with any torch
    optimiser on ``trainable_variables`` or with ``ssm_natgrad.SSMNaturalGradient`` on ``dist_q``, and the hyper-parameters of both
    kernels by giving their tensors ``requires_grad_()``.

    The data are ``(X [.., N, Dx + 1], Y [.., N, 1])`` with TIME IN THE LAST COLUMN of ``X``; leading batch dimensions go on
    ``inducing_time`` and the data, ``inducing_space`` and both kernels are shared by the series.  The model has a zero mean function
    and plain-float likelihood parameters, as every model here.  As in the reference the conditional of ``f(x, t)`` given the state
    at ``t`` is that of a temporal kernel with unit variance: put the signal variance into ``kernel_space``.

    ``mf_lik_st_expectations_*`` and the kernel class carry ``Ms d_t <= 64`` in both dtypes; the chain operators under ``elbo`` - the
    marginals of ``dist_q``, their adjoint and the KL divergence - carry state dimensions up to 64 in float32 and up to 32 in float64
    (``mf_max_state_dim_f64_tile_ops()``): a float64 model with ``Ms d_t > 32`` raises ``NotImplementedError`` in ``elbo`` until they
    reach 64 there too."""

    def __init__(self, inducing_space: torch.Tensor, inducing_time: torch.Tensor, kernel_space, kernel_time: SDEKernel,
                 likelihood: Likelihood, num_data: Optional[int] = None,
                 initial_distribution: Optional[StateSpaceModel] = None) -> None:
        """
        :param inducing_space: ``[Ms, Dx]``.
        :param inducing_time: ``batch + [Mt]``, sorted, at least two.
        :param kernel_space: a ``markovflow_amd.spatial_kernels.SpatialKernel``.
        :param kernel_time: a stationary ``markovflow_amd.kernels.SDEKernel`` with one output; ``Ms d_t <= 64``.
        :param num_data: the total number of observations per series when ``elbo`` is fed minibatches.
        :param initial_distribution: the initial ``q`` on the inducing times; the prior by default.
        """
        kernel = SparseSpatioTemporalKernel(kernel_space, kernel_time, inducing_space)
        super().__init__(kernel, likelihood, inducing_time, min_inducing=2)
        _lib.same_dtype_device(inducing_time, "SpatioTemporalSparseVariational", inducing_space=inducing_space)
        if num_data is not None and not num_data > 0:
            raise ValueError(f"num_data must be positive, got {num_data}")
        self.num_data = num_data
        if initial_distribution is None:
            initial_distribution = kernel.state_space_model(inducing_time)
        elif not isinstance(initial_distribution, StateSpaceModel):
            raise TypeError("initial_distribution must be a StateSpaceModel")
        if (tuple(initial_distribution.batch_shape) != tuple(inducing_time.shape[:-1])
                or initial_distribution.num_transitions + 1 != inducing_time.shape[-1]
                or initial_distribution.state_dim != kernel.state_dim):
            raise ValueError("initial_distribution must be a chain on the inducing times: batch shape "
                             f"{tuple(inducing_time.shape[:-1])}, {inducing_time.shape[-1]} states of dimension {kernel.state_dim}")
        self._dist_q = initial_distribution.create_trainable_copy()
        self._posterior = ConditionalProcess(posterior_dist=self._dist_q, kernel=kernel, conditioning_time_points=inducing_time)

    @property
    def dist_p(self) -> StateSpaceModel:
        """The prior chain on the inducing times, rebuilt on every access."""
        return self._kernel.state_space_model(self.inducing_inputs)

    @property
    def dist_q(self) -> StateSpaceModel:
        """The variational chain, a trainable copy of the prior chain: its leaves are ``trainable_variables``."""
        return self._dist_q

    @property
    def posterior(self) -> ConditionalProcess:
        """The posterior process of the ``Ms`` whitened outputs at the inducing locations."""
        return self._posterior

    @property
    def trainable_variables(self) -> Tuple[torch.Tensor, ...]:
        """The leaves of ``dist_q``: ``(mu0, chol_P0, As, offsets, chol_Qs)``."""
        return self._dist_q.trainable_variables

    # ---- inference ---------------------------------------------------------------------------------------------------------------
    def elbo(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``scale sum_i E_q log p(y_i | f_i) - KL[q || p]``, summed over the batch; ``scale = num_data / minibatch size`` when
        ``num_data`` is set (spatio_temporal_variational.py:209-236).  The data need not be sorted by time: each series is sorted on
        a copy (a stable argsort, cached with the projections), so the ELBO of shuffled data has the bits of the sorted data's.  On
        HIP tensors: the pair marginals of ``dist_q`` under the tape and ONE call of ``mf_lik_st_expectations_*`` whose adjoints the
        backward reuses - also with a hyper-parameter of either kernel under the tape, through the per-point adjoints."""
        inputs, observations = self._check_data(input_data, "elbo")
        ve = torch.sum(self._expected_log_likelihood(inputs, observations))
        kl = torch.sum(self._dist_q.kl_divergence(self.dist_p))
        if self.num_data is not None:
            ve = ve * (float(self.num_data) / inputs.shape[-2])
        return ve - kl

    def loss(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``-elbo`` (spatio_temporal_variational.py:185-192)."""
        return -self.elbo(input_data)


class SpatioTemporalSparseCVI(_SpatioTemporalData, _SparseSitesGaussianProcess):
    """The site-based variant of ``SpatioTemporalSparseVariational`` (markovflow/models/spatio_temporal_variational.py:360-587): the
    same product kernel, inducing locations and inducing times, with ``q(u) = p(u) prod_m t_m(v_m)`` - ``Mt + 1`` Gaussian sites in
    natural form (``nat1 [.., Mt+1, 2D]``, ``nat2 [.., Mt+1, 2D, 2D]``, ``D = Ms d_t``) on the pairs ``v_m = [u_{m-1}, u_m]`` of
    neighbouring inducing states, pairs ``0`` and ``Mt`` with the stationary prior as their outer neighbour.  ``update_sites`` is one
    conjugate-computation VI step on all sites; ``elbo`` is ``scale sum_i E_q log p(y_i | f_i) - KL[q || p]`` and trains the
    hyper-parameters of both kernels with the sites held fixed.  Data, batch dimensions, the zero mean function and the role of
    ``kernel_space``'s variance are those of ``SpatioTemporalSparseVariational``.

    ``mf_lik_st_cvi_site_update_*`` carries ``Ms d_t <= 64`` in both dtypes; ``dist_q`` - the block-tridiagonal Cholesky, the blocks
    of the inverse and the solve under ``naturals_to_ssm_params`` - its marginals and the KL divergence carry state dimensions up
    to 64 in float32 and up to 32 in float64 (``mf_max_state_dim_f64_tile_ops()``): a float64 model with ``Ms d_t > 32`` raises
    ``NotImplementedError`` in ``update_sites``, ``elbo`` and the predictions."""

    def __init__(self, inducing_space: torch.Tensor, inducing_time: torch.Tensor, kernel_space, kernel_time: SDEKernel,
                 likelihood: Likelihood, num_data: Optional[int] = None, learning_rate: float = 0.1) -> None:
        """
        :param inducing_space: ``[Ms, Dx]``.
        :param inducing_time: ``batch + [Mt]``, sorted, at least two.
        :param kernel_space: a ``markovflow_amd.spatial_kernels.SpatialKernel``.
        :param kernel_time: a stationary ``markovflow_amd.kernels.SDEKernel`` with one output; ``Ms d_t <= 64``.
        :param num_data: the total number of observations per series when ``elbo`` is fed minibatches (it does not enter
            ``update_sites``, as in the reference).
        :param learning_rate: the step ``rho`` of ``update_sites``, in [0, 1].
        """
        kernel = SparseSpatioTemporalKernel(kernel_space, kernel_time, inducing_space)
        super().__init__(kernel, inducing_time, likelihood, learning_rate)
        if inducing_time.shape[-1] < 2:
            raise ValueError("inducing_points must be a tensor of shape batch + [num_inducing] with at least two points")
        _lib.same_dtype_device(inducing_time, "SpatioTemporalSparseCVI", inducing_space=inducing_space)
        if num_data is not None and not num_data > 0:
            raise ValueError(f"num_data must be positive, got {num_data}")
        self.num_data = num_data

    # ---- inference ---------------------------------------------------------------------------------------------------------------
    local_objective = SparseCVIGaussianProcess.local_objective
    local_objective_and_gradients = SparseCVIGaussianProcess.local_objective_and_gradients

    def projection_inducing_states_to_observations(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """The projection of the pair of inducing states that brackets a point onto the conditional mean of ``f`` there, the dense
        ``P A`` of the reference, ``batch + [N, 1, 2D]`` in the order of the data (spatio_temporal_variational.py:494-507):
        ``W_k[half D + s d_t + i] = a_k[s] wt_k[half d_t + i]``.  Differentiable in the hyper-parameters of both kernels when one of
        them is under the tape.  For users and tests; ``update_sites`` never forms it."""
        inputs, _ = self._check_data(input_data, "projection_inducing_states_to_observations")
        order, a, wt = (self._compute_projections(inputs) if self._hyper_needs_grad() else self._projections(inputs))[:3]
        w = _st_kron_rows(a, wt).reshape(tuple(a.shape[:-1]) + (1, a.shape[-1] * wt.shape[-1]))
        if order is not None:
            inverse = torch.argsort(order, dim=-1)
            w = torch.gather(w, -3, inverse[..., None, None].expand(w.shape))
        return w

    def update_sites(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> None:
        """One joint CVI step on the sites, in place: ``theta_m <- (1 - rho) theta_m + rho g_m`` with ``g_m`` the gradients of the
        variational expectations of the segment's points in the expectation parameters, projected back onto the pair through
        ``p(f_k | v_m)`` (spatio_temporal_variational.py:509-552).  The data need not be sorted by time: each series is sorted on a
        copy, cached with the projections, and the observations are permuted alike.  HIP tensors: the pair marginals of ``dist_q``,
        the cached per-point projections and ONE call of ``mf_lik_st_cvi_site_update_*``; CPU tensors:
        ``st_cvi_site_update_torch``."""
        inputs, observations = self._check_data(input_data, "update_sites")
        with torch.no_grad():
            pair_mean, pair_cov = self._pair_marginals()
            order, a, wt, c, indices, offsets, tiles = self._projections(inputs)
            y = observations[..., 0]
            if order is not None:
                y = torch.gather(y, -1, order)
            if self._fused(inputs):
                st_cvi_site_update_hip(self._likelihood, a, wt, c, y, offsets, pair_mean, pair_cov, self.learning_rate, self.nat1,
                                       self.nat2, tiles=tiles)
            else:
                st_cvi_site_update_torch(self._likelihood, a, wt, c, y, indices, pair_mean, pair_cov, self.learning_rate, self.nat1,
                                         self.nat2)

    def elbo(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``scale sum_i E_q log p(y_i | f_i) - KL[q || p]``, summed over the batch; ``scale = num_data / minibatch size`` when
        ``num_data`` is set (spatio_temporal_variational.py:209-236).  On HIP tensors the data term is ONE call of
        ``mf_lik_st_expectations_*``, also with a hyper-parameter of either kernel under the tape: its per-point adjoints, the pair
        marginals of ``dist_q`` under the tape and the KL adjoints give ``loss(...).backward()`` the hyper-parameter gradients with
        the sites held fixed."""
        inputs, observations = self._check_data(input_data, "elbo")
        self._check_chain_limit()
        dist_q = self.dist_q
        ve = torch.sum(self._expected_log_likelihood(inputs, observations, dist_q))
        kl = torch.sum(dist_q.kl_divergence(self.dist_p))
        if self.num_data is not None:
            ve = ve * (float(self.num_data) / inputs.shape[-2])
        return ve - kl

    def loss(self, input_data: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """``-elbo`` (spatio_temporal_variational.py:185-192)."""
        return -self.elbo(input_data)
