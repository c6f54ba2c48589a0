"""
The models for a product kernel ``k_s(x, x') k_t(t, t')`` and their functional layer (``st_*``).

``SpatioTemporalSparseVariational`` (mirror of ``markovflow/models/spatio_temporal_variational.py:109-357``, zero mean function) is
the SVGP model: ``q`` is a trainable chain of state dimension ``Ms d_t <= 64`` on the inducing times.  The data term of its ELBO, the
adjoints onto the pair marginals of ``q`` and the per-point adjoints onto the spatial weights and temporal projections are ONE call
of ``mf_lik_st_expectations_*`` (csrc/mf_st.hip).

``SpatioTemporalSparseCVI`` (mirror of ``markovflow/models/spatio_temporal_variational.py:360-587``, zero mean function) is its
site-based variant: ``Mt + 1`` Gaussian sites on the pairs of neighbouring inducing states, updated by ONE call of
``mf_lik_st_cvi_site_update_*``; its ``elbo`` shares ``mf_lik_st_expectations_*``.
"""
from typing import Optional, Tuple

import math

import torch

from .. import _lib, conditionals
from ..kernels import ST_MAX_STATE_DIM, SDEKernel, SparseSpatioTemporalKernel, _version_key
from ..likelihoods import Gaussian, Likelihood
from ..posterior import ConditionalProcess
from ..state_space_model import StateSpaceModel
from ._common import (_check_shapes, _differentiable_once, _launch, _new_outputs, _require_likelihood, _workspace, _written_in_place,
                      gradient_transformation_mean_var_to_expectation)
from .segmented_ops import _segments_of, _site_offsets, sparse_expectation_tiles, sparse_site_projections
from .sparse import SparseCVIGaussianProcess, _SparseGaussianProcess, _SparseSitesGaussianProcess, _sorted_series


# ---- the spatio-temporal sparse variational model: the ELBO's data term ------------------------------------------------------------
ST_EXPECT_TILE = 256            # mf_lik_st_expectations_*: points per workspace row of pass 1 (four groups of 64)


def _st_dims(what: str, a: torch.Tensor, wt: torch.Tensor) -> Tuple[int, int]:
    """``(Ms, two_dt)`` of the spatial weights and temporal projections, checked against the kernel's range."""
    ms, two_dt = a.shape[-1], wt.shape[-1]
    if ms < 1 or two_dt < 2 or two_dt % 2 or ms * (two_dt // 2) > ST_MAX_STATE_DIM:
        raise NotImplementedError(f"{what}: Ms = {ms}, 2 d_t = {two_dt} is outside Ms >= 1, d_t >= 1, Ms d_t <= {ST_MAX_STATE_DIM}")
    return ms, two_dt


def _st_check(what: str, likelihood, a, wt, c, y, lead, segs, pair_mean, pair_cov) -> Tuple[int, int]:
    _require_likelihood(likelihood)
    ms, two_dt = _st_dims(what, a, wt)
    n, pair = a.shape[-2], ms * two_dt
    expect = dict(a=(a, lead + (n, ms)), wt=(wt, lead + (n, two_dt)), c=(c, lead + (n,)), pair_mean=(pair_mean, lead + (segs, pair)),
                  pair_cov=(pair_cov, lead + (segs, pair, pair)))
    if y is not None:
        expect["y"] = (y, lead + (n,))
    _check_shapes(what, expect)
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
    new = _new_outputs(batch, dtype, dev)
    ve_sum = new(want_value, segs)
    g_mean, g_cov = new(want_grads, segs, pair), new(want_grads, segs, pair, pair)
    g_a, g_wt, g_c = new(want_point, n, ms), new(want_point, n, two_dt), new(want_point, n)
    fmu, fvar = new(want_marginals, n), new(want_marginals, n)
    ws, ws_bytes = _workspace(_lib.load().mf_lik_st_expectations_workspace_bytes, dev, num_tiles, ms, two_dt, a.element_size()) \
        if want_value or want_grads else (None, 0)
    _launch("mf_lik_st_expectations", dtype, dev, bsz, n, segs, ms, two_dt, *likelihood._kernel_args(), offsets, a, wt, c, y,
            pair_mean, pair_cov, num_tiles, tile_seg, seg_tile, ws, ws_bytes, ve_sum, g_mean, g_cov, g_a, g_wt, g_c, fmu, fvar)
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
        _differentiable_once("st_expected_log_likelihood", "adjoints")
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
    new = _new_outputs(lead, dtype, dev)
    outs = (new(want_outputs, segs), new(want_outputs, n), new(want_outputs, n))
    ws, ws_bytes = _workspace(_lib.load().mf_lik_st_cvi_site_update_workspace_bytes, dev, num_tiles, ms, two_dt, a.element_size())
    _launch("mf_lik_st_cvi_site_update", dtype, dev, bsz, n, segs, ms, two_dt, *likelihood._kernel_args(), offsets, a, wt, c, y,
            pair_mean, pair_cov, num_tiles, tile_seg, seg_tile, ws, ws_bytes, lr, nat1, nat2, *outs)
    _written_in_place(nat1, nat2)
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
        if not full_output_cov:         # (which the shared method refuses, as ever before it looks at the data)
            input_data = self._check_data(input_data, "predict_log_density")
        return super().predict_log_density(input_data, full_output_cov)

    _predict_f = space_time_predict_f


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
