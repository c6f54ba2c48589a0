"""
The functional layer on pairs of neighbouring inducing states: what the inducing-point models (``sparse.py``) and the importance-
weighted posterior (``posterior.py``) launch, as documented public functions.  The ``N`` data points are cut into ``M + 1`` segments by
the ``M`` inducing points (``offsets [.., M + 2]``), every point sees the pair ``v_m = [u_{m-1}, u_m]`` that brackets it through the
conditional ``p(f(x) | v_m)`` (``w``, ``c`` of ``sparse_site_projections``), and a kernel sums over the points of a segment.  Each op
has a ``*_hip`` wrapper or launcher around ONE C entry point, a ``*_torch`` composition that runs on CPU tensors and is what the
kernel is measured against, and - where it is differentiable - a ``torch.autograd.Function`` whose backward reuses the adjoints the
forward launch wrote:

  * ``sparse_cvi_site_update_{torch,hip}``: ``mf_lik_sparse_cvi_site_update_*`` (projection onto the bracketing pair, expectations,
    back-projection and the segmented sum; in place on the sites);
  * ``sparse_pep_site_update_{torch,hip}`` and ``pair_cavity``: ``mf_lik_sparse_pep_site_update_*`` (tile-parallel kernel pair);
  * ``sparse_expected_log_likelihood(_torch)``: ``mf_lik_sparse_expectations_*`` (two passes, tile-parallel), the SVGP data term;
  * ``sparse_multi_expected_log_likelihood(_torch)``: ``mf_lik_sparse_multi_expectations_*``, the same term for a likelihood with
    several latent functions per observation (``sparse_multi_site_projections``: one dense projection per latent);
  * ``sparse_stack_expected_log_likelihood(_torch)``: ``mf_lik_stack_expectations_*``, the same term on ``K`` STACKED chains
    (``IndependentMultiOutputStack``: ``w [.., K, N, 2d]``, one pair marginal of ``2d`` per chain, not one of ``K 2d``);
  * ``sparse_factor_expected_log_likelihood(_torch)``: ``mf_lik_sparse_factor_expectations_*``, the same term for ``P`` observed series
    per point mixed from the ``L`` latents of a ``FactorAnalysisKernel`` (``sparse_factor_site_projections``: the pair projected onto
    the latents), with the adjoint onto the mixing weights; ``sparse_multi_output_expected_log_likelihood_torch``: the plain
    multi-output term of any kernel with ``P`` outputs (torch only);
  * ``iw_log_likelihood(_torch)``: ``mf_lik_iw_log_weights_*`` (two passes, tile-parallel, no atomics), the data term of the
    importance weights with Matheron's correction assembled in the kernel.

The four tile-parallel SVGP terms share their plumbing: ``_expectations_launch`` is the body of the four
``_sparse_*_expectations_launch`` (outputs, workspace, ONE call), ``_ExpectedLogLikelihood`` the autograd function of the single,
multi and stack terms (the factor term's sibling adds the ``mix`` adjoint), and the compositions are built from ``_gather_pairs``,
``_flat_segments`` and ``_segment_sum``.
"""
from typing import Optional, Tuple

import math

import torch

from .. import _lib, conditionals
from ..kernels import SDEKernel
from ..likelihoods import Gaussian, Likelihood, torch_log_expected_density
from ._common import (_check_shapes, _differentiable_once, _launch, _new_outputs, _require_likelihood, _workspace, _written_in_place,
                      back_project_nats, gradient_transformation_mean_var_to_expectation)


SPARSE_SITE_MAX_TWO_D = 18      # mf_lik_sparse_cvi_site_update_*: 2 d <= 18, the range of the lane-per-point conditional kernels
SPARSE_MULTI_MIN_TWO_D = 6      # mf_lik_sparse_multi_expectations_*: three latents of one state each at the least


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


def _gather_pairs(pair_mean: torch.Tensor, pair_cov: torch.Tensor, indices: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(m_s [.., N, 2d], S_s [.., N, 2d, 2d])``: the marginal of the pair every point belongs to (``indices [.., N]``)."""
    two_d = pair_mean.shape[-1]
    return (torch.gather(pair_mean, -2, indices[..., None].expand(tuple(indices.shape) + (two_d,))),
            torch.gather(pair_cov, -3, indices[..., None, None].expand(tuple(indices.shape) + (two_d, two_d))))


def _flat_segments(indices: torch.Tensor, segs: int) -> torch.Tensor:
    """One flat segment index over the batch, ``series * segs + pair`` (``[B N]``), from the per-point pair index ``[.., N]``."""
    series = torch.arange(math.prod(indices.shape[:-1]), device=indices.device).reshape(tuple(indices.shape[:-1]) + (1,))
    return (indices + series * segs).reshape(-1)


def _segment_sum(ve: torch.Tensor, flat: torch.Tensor, shape) -> torch.Tensor:
    """The per-point values ``ve`` added per segment (``flat``: ``_flat_segments`` of the points), as a tensor of ``shape``."""
    return torch.zeros(math.prod(shape), dtype=ve.dtype, device=ve.device).index_add(0, flat, ve.reshape(-1)).reshape(tuple(shape))


def _sparse_point_marginals(w: torch.Tensor, c: torch.Tensor, indices: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor,
                            segs: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per point ``fmu = w . m_s`` and ``fvar = c + w^T S_s w`` (``[.., N]`` each) with ``(m_s, S_s)`` the marginal of the pair the
    point belongs to (``indices [.., N]``), and one flat segment index over the batch, ``series * segs + pair`` (``[B N]``)."""
    m, cov = _gather_pairs(pair_mean, pair_cov, indices)
    fmu = torch.sum(w * m, dim=-1)
    fvar = c + torch.sum(w * torch.sum(cov * w[..., None, :], dim=-1), dim=-1)
    return fmu, fvar, _flat_segments(indices, segs)


def _segments_of(offsets: torch.Tensor, n: int) -> torch.Tensor:
    """The segment of every point ``0 ... n - 1`` from the segment ``offsets [.., S + 1]``: the number of inner offsets ``<= n``."""
    points = torch.arange(n, device=offsets.device).expand(tuple(offsets.shape[:-1]) + (n,)).contiguous()
    return torch.searchsorted(offsets[..., 1:-1].contiguous(), points, right=True)


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
    new = _new_outputs(tuple(w.shape[:-2]), dtype, dev)
    outs = (new(want_outputs, n), new(want_outputs, n), new(want_outputs, n))
    _launch("mf_lik_sparse_cvi_site_update", dtype, dev, bsz, n, segs, two_d, *likelihood._kernel_args(), offsets, w, c, y, pair_mean,
            pair_cov, float(learning_rate), nat1, nat2, *outs)
    if nat1 is not None:
        _written_in_place(nat1, nat2)
    return outs


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
    led_sum = _new_outputs(batch, dtype, dev)(want_led_sum, segs)
    new = _new_outputs(tuple(w.shape[:-2]), dtype, dev)
    outs = (new(want_outputs, n), new(want_outputs, n), new(want_outputs, n))
    # (the row of the workspace is the SVGP entry point's, and so is the size function: include/markovflow_amd.h)
    ws, ws_bytes = _workspace(_lib.load().mf_lik_sparse_expectations_workspace_bytes, dev, num_tiles, two_d, w.element_size())
    _launch("mf_lik_sparse_pep_site_update", dtype, dev, bsz, n, segs, two_d, *likelihood._kernel_args(), alpha, float(learning_rate),
            offsets, w, c, y, cav_mean, cav_cov, seg_const, num_tiles, tile_seg, seg_tile, ws, ws_bytes, nat1, nat2, log_norm, led_sum,
            *outs)
    if nat1 is not None:
        _written_in_place(*sites)
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


def _expectations_launch(base: str, likelihood: Likelihood, dims, inputs, offsets, tiles, pair_mean, pair_cov, want_grads: bool,
                         chains=(), ws_dims=(), extra=None):
    """ONE call of the tile-parallel SVGP entry point ``base``, the body of the four launchers below.  ``dims``: its dimension
    arguments after the batch size; ``inputs``: its per-point tensors, the projection ``[.., 2d]`` first; ``chains``: the axes of the
    adjoints between the series and the segments (the stack's ``K``); ``ws_dims``: what ``base_workspace_bytes`` takes between ``2d``
    and the element size; ``extra``: ``(want, *shape)`` of a per-series output after ``g_cov``.  Returns ``(ve_sum [.., S],
    g_mean [.., chains, S, 2d] | None, g_cov [.., chains, S, 2d, 2d] | None)`` and the extra output, if any."""
    first = inputs[0]
    dtype, dev = first.dtype, first.device
    two_d, segs = first.shape[-1], offsets.shape[-1] - 1
    batch = tuple(offsets.shape[:-1])
    num_tiles, tile_seg, seg_tile = tiles
    new, new_adjoint = _new_outputs(batch, dtype, dev), _new_outputs(batch + tuple(chains), dtype, dev)
    outs = (new(True, segs), new_adjoint(want_grads, segs, two_d), new_adjoint(want_grads, segs, two_d, two_d))
    if extra is not None:
        outs += (new(*extra),)
    ws, ws_bytes = _workspace(getattr(_lib.load(), base + "_workspace_bytes"), dev, num_tiles, two_d, *ws_dims, first.element_size())
    _launch(base, dtype, dev, offsets.numel() // (segs + 1), *dims, *likelihood._kernel_args(), offsets, *inputs, pair_mean, pair_cov,
            num_tiles, tile_seg, seg_tile, ws, ws_bytes, *outs)
    return outs


def _sparse_expectations_launch(likelihood: Likelihood, w, c, y, offsets, tiles, pair_mean, pair_cov, want_grads: bool):
    """ONE call of ``mf_lik_sparse_expectations_*``: ``(ve_sum [.., S], g_mean [.., S, 2d] | None, g_cov [.., S, 2d, 2d] | None)``."""
    return _expectations_launch("mf_lik_sparse_expectations", likelihood, (w.shape[-2], offsets.shape[-1] - 1, w.shape[-1]), (w, c, y),
                                offsets, tiles, pair_mean, pair_cov, want_grads)


class _ExpectedLogLikelihood(torch.autograd.Function):
    """The single-latent, multi-latent and stacked SVGP data terms: value ``batch + [M + 1]``; the adjoints onto the pair marginals
    come out of the same launch and wait for the backward.  ``launcher``: one of the ``_sparse_*_expectations_launch``; ``name``: the
    public function, for the messages; ``chains``: the number of axes of the pair marginals between the series and the segments
    (the stack's ``K``: 1), over which a segment's cotangent is broadcast."""

    @staticmethod
    def forward(ctx, pair_mean, pair_cov, launcher, name, chains, likelihood, w, c, y, offsets, tiles):
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        with torch.no_grad():
            ve_sum, g_mean, g_cov = launcher(likelihood, w.detach(), c.detach(), y.detach(), offsets, tiles, pair_mean.detach(),
                                             pair_cov.detach(), want)
        if want:
            ctx.save_for_backward(g_mean, g_cov)
        ctx.name, ctx.chains = name, chains
        return ve_sum

    @staticmethod
    def backward(ctx, grad_out):
        _differentiable_once(ctx.name, "adjoints")
        g_mean, g_cov = ctx.saved_tensors
        g = grad_out[(Ellipsis,) + (None,) * ctx.chains + (slice(None),)]       # a segment's cotangent goes to every chain of it
        return (g[..., None] * g_mean if ctx.needs_input_grad[0] else None,
                g[..., None, None] * g_cov if ctx.needs_input_grad[1] else None) + (None,) * 9


def sparse_expected_log_likelihood(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor, offsets: torch.Tensor,
                                   pair_mean: torch.Tensor, pair_cov: torch.Tensor, tiles=None) -> torch.Tensor:
    """``sum_k E_q log p(y_k | f_k)`` per pair of neighbouring inducing states, ``batch + [M + 1]``, with ``fmu = w_k . m_s`` and
    ``fvar = c_k + w_k^T S_s w_k`` for the points ``offsets[s] <= k < offsets[s + 1]`` of pair ``s`` (``w [.., N, 2d]``, ``c``, ``y``
    ``[.., N]``, ``offsets [.., M + 2]``, ``pair_mean [.., M + 1, 2d]``, ``pair_cov [.., M + 1, 2d, 2d]``): ONE call of
    ``mf_lik_sparse_expectations_*`` on HIP tensors, ``2d <= 18``.  Differentiable ONCE in ``pair_mean`` and ``pair_cov`` (an
    unconstrained matrix: the gradient is symmetric) - the backward multiplies the adjoints the forward computed beside the value,
    there is no second launch; not differentiable in ``w`` and ``c``.  ``tiles``: ``sparse_expectation_tiles(offsets)`` when the
    caller keeps it."""
    _require_likelihood(likelihood)
    two_d, segs = w.shape[-1], offsets.shape[-1] - 1
    batch = tuple(offsets.shape[:-1])
    if two_d > SPARSE_SITE_MAX_TWO_D or two_d % 2:
        raise NotImplementedError(f"sparse_expected_log_likelihood: 2d = {two_d} is outside 2, 4, ..., {SPARSE_SITE_MAX_TWO_D}; "
                                  "use sparse_expected_log_likelihood_torch")
    _check_shapes("sparse_expected_log_likelihood",
                  dict(w=(w, batch + (w.shape[-2], two_d)), c=(c, batch + (w.shape[-2],)), y=(y, batch + (w.shape[-2],)),
                       pair_mean=(pair_mean, batch + (segs, two_d)), pair_cov=(pair_cov, batch + (segs, two_d, two_d))))
    _lib.same_dtype_device(w, "sparse_expected_log_likelihood", c=c, y=y, pair_mean=pair_mean, pair_cov=pair_cov)
    if torch.is_grad_enabled() and (w.requires_grad or c.requires_grad):
        raise NotImplementedError("sparse_expected_log_likelihood has no adjoint onto w and c (a kernel hyper-parameter under the "
                                  "tape): use sparse_expected_log_likelihood_torch")
    if tiles is None:
        tiles = sparse_expectation_tiles(offsets)
    return _ExpectedLogLikelihood.apply(pair_mean, pair_cov, _sparse_expectations_launch, "sparse_expected_log_likelihood", 0,
                                        likelihood, w, c, y, offsets, tiles)


def sparse_expected_log_likelihood_torch(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                                         indices: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor) -> torch.Tensor:
    """The same quantity as a torch composition, differentiable by autograd in ``pair_mean``, ``pair_cov``, ``w`` and ``c``: gathers
    of the pair marginals by the per-point pair index (``indices [.., N]``), ``likelihood.variational_expectations`` and
    ``index_add_`` over the segments.  It runs on CPU tensors, it is the models' route for ``2d > 18`` and for a kernel
    hyper-parameter under the tape, and it is what ``mf_lik_sparse_expectations_*`` is measured against."""
    fmu, fvar, flat = _sparse_point_marginals(w, c, indices, pair_mean, pair_cov, pair_mean.shape[-2])
    ve = likelihood.variational_expectations(fmu[..., None], fvar[..., None], y[..., None])
    return _segment_sum(ve, flat, pair_mean.shape[:-1])


# ---- SVGP with several latent functions per observation -----------------------------------------------------------------------------
def sparse_multi_site_projections(kernel: SDEKernel, time_points: torch.Tensor, inducing_points: torch.Tensor
                                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``sparse_site_projections`` for a kernel with ``L = kernel.output_dim`` outputs: one projection of the pair per latent,
    ``w [.., N, L, 2d] = H P_k`` and ``c [.., N, L] = diag(H T_k H^T)`` (the reference's ``full_output_cov=False``), with the same
    ``indices`` and ``offsets``.  The rows are dense: nothing is assumed about the emission matrix."""
    proj, cov, indices = conditionals._conditional_statistics(time_points, inducing_points, kernel)
    h = kernel.generate_emission_model(time_points).emission_matrix                         # [.., N, L, d]
    w = h @ proj
    c = torch.sum((h @ cov) * h, dim=-1)
    return w.contiguous(), c.contiguous(), indices, _site_offsets(time_points, inducing_points)


def _sparse_multi_point_marginals(w: torch.Tensor, c: torch.Tensor, indices: torch.Tensor, pair_mean: torch.Tensor,
                                  pair_cov: torch.Tensor, segs: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``_sparse_point_marginals`` per latent: ``fmu``, ``fvar`` ``[.., N, L]`` from ``w [.., N, L, 2d]``, ``c [.., N, L]``."""
    m, cov = _gather_pairs(pair_mean, pair_cov, indices)
    fmu = torch.sum(w * m[..., None, :], dim=-1)
    fvar = c + torch.sum(w * (w @ cov.transpose(-1, -2)), dim=-1)
    return fmu, fvar, _flat_segments(indices, segs)


def _sparse_multi_expectations_launch(likelihood: Likelihood, w, c, y, offsets, tiles, pair_mean, pair_cov, want_grads: bool):
    """ONE call of ``mf_lik_sparse_multi_expectations_*``: ``(ve_sum [.., S], g_mean [.., S, 2d] | None, g_cov [.., S, 2d, 2d] | None)``."""
    return _expectations_launch("mf_lik_sparse_multi_expectations", likelihood,
                                (w.shape[-3], offsets.shape[-1] - 1, w.shape[-1], w.shape[-2]), (w, c, y), offsets, tiles, pair_mean,
                                pair_cov, want_grads)


def sparse_multi_expected_log_likelihood(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                                         offsets: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor, tiles=None
                                         ) -> torch.Tensor:
    """``sparse_expected_log_likelihood`` for a likelihood with ``L = likelihood.latent_dim > 1`` latent functions: per point and
    latent ``fmu_l = w_kl . m_s`` and ``fvar_l = c_kl + w_kl^T S_s w_kl`` (``w [.., N, L, 2d]``, ``c [.., N, L]``, ``y [.., N]``), the
    likelihood's expectation over the ``L`` marginals, summed per pair, ``batch + [M + 1]``: ONE call of
    ``mf_lik_sparse_multi_expectations_*`` on HIP tensors, ``6 <= 2d <= 18``.  Differentiable ONCE in ``pair_mean`` and ``pair_cov``
    (the backward multiplies the adjoints the forward computed beside the value); not differentiable in ``w`` and ``c``."""
    _require_likelihood(likelihood, multi_latent=True)
    what = "sparse_multi_expected_log_likelihood"
    if w.dim() < 3:
        raise ValueError(f"{what}: w must have shape batch + [N, L, 2d], got {tuple(w.shape)}")
    n, latents, two_d, segs = w.shape[-3], w.shape[-2], w.shape[-1], offsets.shape[-1] - 1
    batch = tuple(offsets.shape[:-1])
    if latents != likelihood.latent_dim or latents < 2:
        raise ValueError(f"{what}: w carries {latents} latent rows per point, the likelihood has latent_dim = {likelihood.latent_dim} "
                         "(a likelihood with one latent takes sparse_expected_log_likelihood)")
    if two_d > SPARSE_SITE_MAX_TWO_D or two_d < SPARSE_MULTI_MIN_TWO_D or two_d % 2:
        raise NotImplementedError(f"{what}: 2d = {two_d} is outside {SPARSE_MULTI_MIN_TWO_D}, ..., {SPARSE_SITE_MAX_TWO_D}; use "
                                  "sparse_multi_expected_log_likelihood_torch")
    _check_shapes(what, dict(w=(w, batch + (n, latents, two_d)), c=(c, batch + (n, latents)), y=(y, batch + (n,)),
                             pair_mean=(pair_mean, batch + (segs, two_d)), pair_cov=(pair_cov, batch + (segs, two_d, two_d))))
    _lib.same_dtype_device(w, what, c=c, y=y, pair_mean=pair_mean, pair_cov=pair_cov)
    if torch.is_grad_enabled() and (w.requires_grad or c.requires_grad):
        raise NotImplementedError(f"{what} has no adjoint onto w and c (a kernel hyper-parameter under the tape): use "
                                  "sparse_multi_expected_log_likelihood_torch")
    if tiles is None:
        tiles = sparse_expectation_tiles(offsets)
    return _ExpectedLogLikelihood.apply(pair_mean, pair_cov, _sparse_multi_expectations_launch, what, 0, likelihood, w, c, y, offsets,
                                        tiles)


def sparse_multi_expected_log_likelihood_torch(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                                               indices: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor) -> torch.Tensor:
    """The same quantity as a torch composition, differentiable by autograd in ``pair_mean``, ``pair_cov``, ``w`` and ``c``: gathers
    of the pair marginals by the per-point pair index (``indices [.., N]``), ``likelihood.variational_expectations`` on ``[.., N, L]``
    and ``index_add_`` over the segments.  It runs on CPU tensors, it is the model's route for ``2d > 18`` and for a kernel
    hyper-parameter under the tape, and it is what ``mf_lik_sparse_multi_expectations_*`` is measured against."""
    fmu, fvar, flat = _sparse_multi_point_marginals(w, c, indices, pair_mean, pair_cov, pair_mean.shape[-2])
    ve = likelihood.variational_expectations(fmu, fvar, y[..., None])
    return _segment_sum(ve, flat, pair_mean.shape[:-1])


# ---- SVGP with several latent functions per observation on STACKED chains (IndependentMultiOutputStack) ----------------------------
SPARSE_STACK_SIGNATURES = ((3, 4), (2, 5))      # mf_lik_stack_expectations_*: the instantiated (latent_dim, likelihood id)


def sparse_stack_instantiated(likelihood: Likelihood, latents: int, two_d: int) -> bool:
    """Whether ``mf_lik_stack_expectations_*`` is instantiated for this likelihood on ``latents`` chains of ``2d = two_d``."""
    return ((latents, likelihood._id) in SPARSE_STACK_SIGNATURES and latents == likelihood.latent_dim
            and 2 <= two_d <= SPARSE_SITE_MAX_TWO_D and two_d % 2 == 0)


def _sparse_stack_check(what: str, likelihood, w, c, y, lead, segs, pair_mean, pair_cov, segmentation, per_chain: bool) -> None:
    _require_likelihood(likelihood, multi_latent=True)
    if w.dim() < 3:
        raise ValueError(f"{what}: w must have shape batch + [K, N, 2d], got {tuple(w.shape)}")
    latents, n, two_d = w.shape[-3], w.shape[-2], w.shape[-1]
    if latents != likelihood.latent_dim or latents < 2:
        raise ValueError(f"{what}: w carries {latents} chains, the likelihood has latent_dim = {likelihood.latent_dim} (a likelihood "
                         "with one latent takes sparse_expected_log_likelihood on the batch of chains)")
    name, seg = segmentation
    _check_shapes(what, {"w": (w, lead + (latents, n, two_d)), "c": (c, lead + (latents, n)), "y": (y, lead + (n,)),
                         "pair_mean": (pair_mean, lead + (latents, segs, two_d)),
                         "pair_cov": (pair_cov, lead + (latents, segs, two_d, two_d))})
    if per_chain and tuple(seg.shape) not in (lead + (n,), lead + (latents, n)):
        raise ValueError(f"{what}: {name} has shape {tuple(seg.shape)}, expected {lead + (n,)} or {lead + (latents, n)}")
    if not per_chain and tuple(seg.shape) != lead + (segs + 1,):
        raise ValueError(f"{what}: {name} has shape {tuple(seg.shape)}, expected {lead + (segs + 1,)}")
    _lib.same_dtype_device(w, what, c=c, y=y, pair_mean=pair_mean, pair_cov=pair_cov)


def _sparse_stack_expectations_launch(likelihood: Likelihood, w, c, y, offsets, tiles, pair_mean, pair_cov, want_grads: bool):
    """ONE call of ``mf_lik_stack_expectations_*``: ``(ve_sum [.., S], g_mean [.., K, S, 2d] | None, g_cov [.., K, S, 2d, 2d] | None)``."""
    latents = w.shape[-3]
    return _expectations_launch("mf_lik_stack_expectations", likelihood, (latents, w.shape[-2], offsets.shape[-1] - 1, w.shape[-1]),
                                (w, c, y), offsets, tiles, pair_mean, pair_cov, want_grads, chains=(latents,), ws_dims=(latents,))


def sparse_stack_expected_log_likelihood(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                                         offsets: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor, tiles=None
                                         ) -> torch.Tensor:
    """The SVGP data term of a likelihood with ``K = likelihood.latent_dim > 1`` latent functions on ``K`` STACKED chains that share
    one segmentation, ``sum_n E_q log p(y_n | f_n)`` per pair of neighbouring inducing points, ``lead + [M + 1]``: per point and
    latent ``fmu_k = w_kn . m_ks`` and ``fvar_k = c_kn + w_kn^T S_ks w_kn`` with the pair marginals of chain ``k``
    (``w [.., K, N, 2d]``, ``c [.., K, N]`` - ``sparse_site_projections`` on the stacked batch -, ``y [.., N]``,
    ``offsets [.., M + 2]``, ``pair_mean [.., K, M + 1, 2d]``, ``pair_cov [.., K, M + 1, 2d, 2d]``): ONE call of
    ``mf_lik_stack_expectations_*`` on HIP tensors, ``2d <= 18``, ``MultiStageLikelihood`` (``K = 3``) or ``HeteroscedasticGaussian``
    (``K = 2``).  Differentiable ONCE in ``pair_mean`` and ``pair_cov`` (the backward multiplies the adjoints the forward computed
    beside the value, there is no second launch); not differentiable in ``w`` and ``c``.  ``tiles``:
    ``sparse_expectation_tiles(offsets)`` when the caller keeps it."""
    what = "sparse_stack_expected_log_likelihood"
    segs = offsets.shape[-1] - 1
    lead = tuple(offsets.shape[:-1])
    _sparse_stack_check(what, likelihood, w, c, y, lead, segs, pair_mean, pair_cov, ("offsets", offsets), per_chain=False)
    latents, two_d = w.shape[-3], w.shape[-1]
    if not sparse_stack_instantiated(likelihood, latents, two_d):
        raise NotImplementedError(f"{what}: K = {latents}, 2d = {two_d}, {type(likelihood).__name__} is outside the instantiated "
                                  f"signatures (2d even in 2 ... {SPARSE_SITE_MAX_TWO_D}; MultiStageLikelihood, "
                                  "HeteroscedasticGaussian); use sparse_stack_expected_log_likelihood_torch")
    if torch.is_grad_enabled() and (w.requires_grad or c.requires_grad):
        raise NotImplementedError(f"{what} has no adjoint onto w and c (a kernel hyper-parameter under the tape): use "
                                  "sparse_stack_expected_log_likelihood_torch")
    if tiles is None:
        tiles = sparse_expectation_tiles(offsets)
    return _ExpectedLogLikelihood.apply(pair_mean, pair_cov, _sparse_stack_expectations_launch, what, 1, likelihood, w, c, y, offsets,
                                        tiles)


def sparse_stack_expected_log_likelihood_torch(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                                               indices: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor,
                                               orders: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The same quantity as a torch composition, differentiable by autograd in everything (``pair_mean``, ``pair_cov``, ``w``, ``c``):
    per chain the gathers of its pair marginals by the per-point pair index, ``likelihood.variational_expectations`` on
    ``[.., N, K]`` and ``index_add`` over the segments.  ``indices`` is ``[.., N]`` (one segmentation for the ``K`` chains) or
    ``[.., K, N]``: the chains need NOT share inducing points.  The data term of a point is then booked on the pair of chain 0 - the
    split over the pairs is chain 0's, the sum over them is the ELBO's data term whatever the chains' segmentations.
    ``orders [.., K, N]`` (optional): chain ``k``'s rows of ``w``, ``c`` and ``indices`` are in the order ``orders[.., k, :]`` of the
    data (each chain sorted on its own time points); the per-chain marginals are brought back to the data's order, that of ``y``,
    before the likelihood sees them.  It runs on CPU tensors, it is the model's route for ``2d > 18``, for a hyper-parameter under
    the tape and for chains that do not share their inducing or data times, and it is what ``mf_lik_stack_expectations_*`` is
    measured against."""
    what = "sparse_stack_expected_log_likelihood_torch"
    lead = tuple(y.shape[:-1])
    latents, segs = w.shape[-3], pair_mean.shape[-2]
    _sparse_stack_check(what, likelihood, w, c, y, lead, segs, pair_mean, pair_cov, ("indices", indices), per_chain=True)
    if indices.dim() == len(lead) + 1:
        indices = indices[..., None, :].expand(lead + (latents, indices.shape[-1]))
    fmu, fvar, _ = _sparse_point_marginals(w, c, indices, pair_mean, pair_cov, segs)            # [.., K, N] on the batch of chains
    booked = indices[..., 0, :]
    if orders is not None:
        inverse = torch.argsort(orders, dim=-1)
        fmu, fvar = torch.gather(fmu, -1, inverse), torch.gather(fvar, -1, inverse)
        booked = torch.gather(booked, -1, inverse[..., 0, :])
    ve = likelihood.variational_expectations(fmu.transpose(-1, -2), fvar.transpose(-1, -2), y[..., None])
    return _segment_sum(ve, _flat_segments(booked, segs), lead + (segs,))


# ---- SVGP with several observed series per point: multi-output kernels and the FactorAnalysis emission ------------------------------
SPARSE_FACTOR_LATENTS = (2, 3, 4)   # mf_lik_sparse_factor_expectations_*: the instantiated latent_dim (2d even in 2 L ... 18)
SPARSE_FACTOR_MAX_OUTPUTS = 1024    # ... and the largest number of observed series


def sparse_multi_output_expected_log_likelihood_torch(likelihood: Likelihood, w: torch.Tensor, c: torch.Tensor, y: torch.Tensor,
                                                      indices: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor
                                                      ) -> torch.Tensor:
    """The SVGP data term for a kernel with ``P`` outputs and a likelihood with ONE latent function, applied per output:
    ``sum_k sum_p E_q log p(y_kp | f_kp)`` per pair, ``batch + [M + 1]``, with ``fmu_p = w_kp . m_s`` and
    ``fvar_p = c_kp + w_kp^T S_s w_kp`` from the dense rows ``w [.., N, P, 2d]``, ``c [.., N, P]`` of ``sparse_multi_site_projections``
    and ``y [.., N, P]``.  A torch composition only (gathers, ``likelihood.variational_expectations``, ``index_add``), differentiable
    by autograd in ``pair_mean``, ``pair_cov``, ``w`` and ``c``; it runs on CPU tensors.  It is the model's route for multi-output
    observations on a kernel that is not a ``FactorAnalysisKernel``."""
    _require_likelihood(likelihood)
    _check_shapes("sparse_multi_output_expected_log_likelihood_torch", dict(c=(c, tuple(w.shape[:-1])), y=(y, tuple(w.shape[:-1]))))
    fmu, fvar, flat = _sparse_multi_point_marginals(w, c, indices, pair_mean, pair_cov, pair_mean.shape[-2])
    ve = torch.sum(likelihood.variational_expectations(fmu[..., None], fvar[..., None], y[..., None]), dim=-1)
    return _segment_sum(ve, flat, pair_mean.shape[:-1])


def sparse_factor_site_projections(kernel, time_points: torch.Tensor, inducing_points: torch.Tensor
                                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``sparse_site_projections`` onto the LATENT processes of a ``FactorAnalysisKernel`` with ``L`` latents: ``wg [.., N, L, 2d] =
    H_inner P_k`` and the full ``cg [.., N, L, L] = H_inner T_k H_inner^T``, with the same ``indices`` and ``offsets``.  None of it
    depends on the loading matrix or the weight function, so it is computed under ``no_grad`` and a model caches it."""
    with torch.no_grad():
        proj, cov, indices = conditionals._conditional_statistics(time_points, inducing_points, kernel)
        h = kernel.latent_emission_model(time_points).emission_matrix                       # [.., N, L, d]
        wg = h @ proj
        cg = h @ cov @ h.transpose(-1, -2)
        cg = 0.5 * (cg + cg.transpose(-1, -2))
        return wg.contiguous(), cg.contiguous(), indices, _site_offsets(time_points, inducing_points)


def _sparse_factor_check(what: str, likelihood, wg, cg, mix, y, lead, segs, pair_mean, pair_cov) -> None:
    _require_likelihood(likelihood)
    if wg.dim() < 3 or mix.dim() < 3:
        raise ValueError(f"{what}: wg must have shape batch + [N, L, 2d] and mix batch + [N, P, L], got {tuple(wg.shape)} and "
                         f"{tuple(mix.shape)}")
    n, latents, two_d, outputs = wg.shape[-3], wg.shape[-2], wg.shape[-1], mix.shape[-2]
    _check_shapes(what, dict(wg=(wg, lead + (n, latents, two_d)), cg=(cg, lead + (n, latents, latents)),
                             mix=(mix, lead + (n, outputs, latents)), y=(y, lead + (n, outputs)),
                             pair_mean=(pair_mean, lead + (segs, two_d)), pair_cov=(pair_cov, lead + (segs, two_d, two_d))))
    _lib.same_dtype_device(wg, what, cg=cg, mix=mix, y=y, pair_mean=pair_mean, pair_cov=pair_cov)


def _sparse_factor_expectations_launch(likelihood: Likelihood, wg, cg, mix, y, offsets, tiles, pair_mean, pair_cov, want_grads: bool,
                                       want_g_w: bool):
    """ONE call of ``mf_lik_sparse_factor_expectations_*``: ``(ve_sum [.., S], g_mean [.., S, 2d] | None, g_cov [.., S, 2d, 2d] | None,
    g_w [.., N, P, L] | None)``."""
    n, latents, outputs = wg.shape[-3], wg.shape[-2], mix.shape[-2]
    return _expectations_launch("mf_lik_sparse_factor_expectations", likelihood,
                                (n, offsets.shape[-1] - 1, wg.shape[-1], latents, outputs), (wg, cg, mix, y), offsets, tiles,
                                pair_mean, pair_cov, want_grads, extra=(want_g_w, n, outputs, latents))


class _SparseFactorExpectedLogLikelihood(torch.autograd.Function):
    """Value ``batch + [M + 1]``; the adjoints onto the pair marginals and - when ``mix`` requires a gradient - onto the mixing weights
    come out of the same launch and wait for the backward."""

    @staticmethod
    def forward(ctx, pair_mean, pair_cov, mix, likelihood, wg, cg, y, offsets, tiles):
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        want_w = ctx.needs_input_grad[2]
        with torch.no_grad():
            ve_sum, g_mean, g_cov, g_w = _sparse_factor_expectations_launch(likelihood, wg.detach(), cg.detach(), mix.detach(), y.detach(),
                                                                            offsets, tiles, pair_mean.detach(), pair_cov.detach(), want,
                                                                            want_w)
        ctx.want, ctx.want_w = want, want_w
        saved = ((g_mean, g_cov) if want else ()) + ((g_w, _segments_of(offsets, wg.shape[-3])) if want_w else ())
        ctx.save_for_backward(*saved)
        return ve_sum

    @staticmethod
    def backward(ctx, grad_out):
        _differentiable_once("sparse_factor_expected_log_likelihood", "adjoints")
        saved = list(ctx.saved_tensors)
        g_mean = g_cov = g_mix = None
        if ctx.want:
            g_mean, g_cov = saved[:2]
            saved = saved[2:]
        if ctx.want_w:
            g_w, segment = saved
            g_mix = torch.gather(grad_out, -1, segment)[..., None, None] * g_w       # every point takes its segment's cotangent
        return (grad_out[..., None] * g_mean if ctx.needs_input_grad[0] else None,
                grad_out[..., None, None] * g_cov if ctx.needs_input_grad[1] else None, g_mix, None, None, None, None, None, None)


def sparse_factor_expected_log_likelihood(likelihood: Likelihood, wg: torch.Tensor, cg: torch.Tensor, mix: torch.Tensor,
                                          y: torch.Tensor, offsets: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor,
                                          tiles=None) -> torch.Tensor:
    """The SVGP data term under a FactorAnalysis emission, ``sum_k sum_p E_q log p(y_kp | f_kp)`` per pair of neighbouring inducing
    states, ``batch + [M + 1]``: per point ``mu_g = wg m_s``, ``Sig_g = cg + wg S_s wg^T`` (``L`` projections of the pair), then per
    observed series ``fmu_p = W_p . mu_g``, ``fvar_p = W_p Sig_g W_p^T`` with ``W = mix [.., N, P, L]`` and the likelihood's scalar
    expectation at ``y [.., N, P]`` (``wg [.., N, L, 2d]``, ``cg [.., N, L, L]`` of ``sparse_factor_site_projections``): ONE call of
    ``mf_lik_sparse_factor_expectations_*`` on HIP tensors, ``L`` in 2, 3, 4, ``2d`` even in ``2L ... 18``, ``P <= 1024``.
    Differentiable ONCE in ``pair_mean``, ``pair_cov`` and ``mix``: the backward multiplies the adjoints the forward launch left
    behind (the adjoint onto ``mix`` is asked of the kernel only when ``mix`` requires a gradient), there is no second launch.  Not
    differentiable in ``wg`` and ``cg``.  ``tiles``: ``sparse_expectation_tiles(offsets)`` when the caller keeps it."""
    what = "sparse_factor_expected_log_likelihood"
    segs = offsets.shape[-1] - 1
    _sparse_factor_check(what, likelihood, wg, cg, mix, y, tuple(offsets.shape[:-1]), segs, pair_mean, pair_cov)
    latents, two_d, outputs = wg.shape[-2], wg.shape[-1], mix.shape[-2]
    if (latents not in SPARSE_FACTOR_LATENTS or two_d > SPARSE_SITE_MAX_TWO_D or two_d < 2 * latents or two_d % 2
            or not 1 <= outputs <= SPARSE_FACTOR_MAX_OUTPUTS):
        raise NotImplementedError(f"{what}: L = {latents}, 2d = {two_d}, P = {outputs} is outside L in {SPARSE_FACTOR_LATENTS}, 2d even "
                                  f"in 2L ... {SPARSE_SITE_MAX_TWO_D}, 1 <= P <= {SPARSE_FACTOR_MAX_OUTPUTS}; use "
                                  "sparse_factor_expected_log_likelihood_torch")
    if torch.is_grad_enabled() and (wg.requires_grad or cg.requires_grad):
        raise NotImplementedError(f"{what} has no adjoint onto wg and cg (a hyper-parameter of the chain under the tape): use "
                                  "sparse_factor_expected_log_likelihood_torch")
    if tiles is None:
        tiles = sparse_expectation_tiles(offsets)
    return _SparseFactorExpectedLogLikelihood.apply(pair_mean, pair_cov, mix, likelihood, wg, cg, y, offsets, tiles)


def sparse_factor_expected_log_likelihood_torch(likelihood: Likelihood, wg: torch.Tensor, cg: torch.Tensor, mix: torch.Tensor,
                                                y: torch.Tensor, indices: torch.Tensor, pair_mean: torch.Tensor, pair_cov: torch.Tensor
                                                ) -> torch.Tensor:
    """The same quantity as a torch composition, differentiable by autograd in everything (``pair_mean``, ``pair_cov``, ``mix``,
    ``wg``, ``cg``): gathers of the pair marginals by the per-point pair index (``indices [.., N]``), the two projections,
    ``likelihood.variational_expectations`` per observed series and ``index_add`` over the segments.  It runs on CPU tensors, it is
    the model's route for ``2d > 18``, for an ``L`` that is not instantiated and for a hyper-parameter of the chain under the tape, and
    it is what ``mf_lik_sparse_factor_expectations_*`` is measured against."""
    segs = pair_mean.shape[-2]
    _sparse_factor_check("sparse_factor_expected_log_likelihood_torch", likelihood, wg, cg, mix, y, tuple(indices.shape[:-1]), segs,
                         pair_mean, pair_cov)
    m, cov = _gather_pairs(pair_mean, pair_cov, indices)
    mu_g = (wg @ m[..., None])[..., 0]                                                     # [.., N, L]
    sig_g = cg + wg @ cov @ wg.transpose(-1, -2)                                           # [.., N, L, L]
    fmu = (mix @ mu_g[..., None])[..., 0]                                                  # [.., N, P]
    fvar = torch.sum((mix @ sig_g) * mix, dim=-1)
    ve = torch.sum(likelihood.variational_expectations(fmu[..., None], fvar[..., None], y[..., None]), dim=-1)
    return _segment_sum(ve, _flat_segments(indices, segs), pair_mean.shape[:-1])


# ---- importance-weighted VI: the data term of the log weights ----------------------------------------------------------------------
IW_SAMPLE_CHUNK = 8             # mf_lik_iw_log_weights_*: samples per block of pass 1


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
    new = _new_outputs((k,) + batch, dtype, dev)
    log_lik, g_u = new(want_value, segs), new(want_grad, segs - 1, d)
    ws, ws_bytes = _workspace(_lib.load().mf_lik_iw_log_weights_workspace_bytes, dev, num_tiles, k, 2 * d, states.element_size())
    _launch("mf_lik_iw_log_weights", dtype, dev, bsz, n, segs, 2 * d, k, likelihood._id, likelihood._c_params(), offsets, w, y, h,
            states, u_post, num_tiles, tile_seg, seg_tile, ws, ws_bytes, log_lik, g_u)
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
        _differentiable_once("iw_log_likelihood", "adjoint")
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
    _require_likelihood(likelihood)
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
    _check_shapes("iw_log_likelihood", expect)
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
