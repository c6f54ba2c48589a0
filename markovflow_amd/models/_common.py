"""
What every module of the package shares: the small functions of the site algebra (``back_project_nats``,
``gradient_transformation_mean_var_to_expectation``, ``gradient_correction``), the checks that every model and every fused op makes
in the same words, the ``predict_log_density`` mixin, and the ONE way a fused entry point of the C ABI is launched (``_launch`` with
its companions ``_new_outputs``, ``_workspace`` and ``_written_in_place``).
"""
from typing import Tuple

import torch

from .. import _lib
from ..kernels import NonStationaryKernel, SDEKernel, _refuse_factor_analysis, _refuse_stack  # noqa: F401  (the models import them from here)
from ..likelihoods import Likelihood


def _refuse_non_stationary(kernel, who: str) -> None:
    """Every model but ``GaussianProcessRegression`` takes stationary kernels only: the sparse and site-based models put the
    stationary prior (``_stationary_prior``) at both ends of their chains, which is only right for a stationary kernel."""
    if isinstance(kernel, NonStationaryKernel):
        raise NotImplementedError(f"{who} supports stationary kernels only: a non-stationary kernel ({type(kernel).__name__}) is "
                                  "supported by GaussianProcessRegression alone")


def _require_likelihood(likelihood, multi_latent: bool = False) -> None:
    """``multi_latent``: the caller projects one marginal per latent function; every other model and fused op is written for ONE."""
    if not isinstance(likelihood, Likelihood):
        raise TypeError("likelihood must be a markovflow_amd.likelihoods.Likelihood")
    if likelihood.latent_dim > 1 and not multi_latent:
        raise NotImplementedError(f"{type(likelihood).__name__} has {likelihood.latent_dim} latent functions per observation: only "
                                  "SparseVariationalGaussianProcess supports a likelihood with latent_dim > 1")


def _check_dense_data(time_points: torch.Tensor, observations: torch.Tensor) -> None:
    """The two checks on ``(time_points, observations)`` that the models with one state per data point make."""
    if observations.dim() < 2 or observations.shape[-1] != 1:
        raise ValueError(f"observations must have shape batch + [num_data, 1], got {tuple(observations.shape)}")
    if tuple(time_points.shape) != tuple(observations.shape[:-1]):
        raise ValueError("time_points must have shape observations.shape[:-1]")


def _check_shapes(what: str, expect: dict) -> None:
    """``expect``: ``{name: (tensor, shape)}``; a tensor that is missing (``None``) has no shape to agree."""
    for name, (t, shape) in expect.items():
        if t is None or tuple(t.shape) != shape:
            raise ValueError(f"{what}: {name} has shape {None if t is None else tuple(t.shape)}, expected {shape}")


def _differentiable_once(name: str, what: str) -> None:
    """Called first in the ``backward`` of an op whose adjoints come out of its forward launch: under ``create_graph=True`` there
    is nothing to differentiate them with."""
    if torch.is_grad_enabled():
        raise RuntimeError(f"{name} is differentiable once: its backward uses the {what} computed in the forward and has no "
                           "second-order support (create_graph=True)")


# ---- launching a fused entry point ---------------------------------------------------------------------------------------------------
def _launch(base: str, dtype: torch.dtype, dev: torch.device, *args) -> None:
    """``_lib.call(base, dtype, ...)`` on ``args`` in the order of the entry point's signature, the current stream of ``dev``
    appended.  Every tensor among them is made contiguous and passed as its device pointer; ``None`` (NULL) and scalars pass as
    they are.  A pointer keeps no tensor alive, and a contiguous copy that is dropped goes back to the caching allocator, which may
    hand the same block to the NEXT copy of that size - two pointers onto one buffer.  So the copies are held here until the call
    has returned."""
    held = [a.contiguous() if isinstance(a, torch.Tensor) else a for a in args]
    _lib.call(base, dtype, *[_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in held], _lib.stream_ptr(dev))


def _new_outputs(batch: Tuple[int, ...], dtype: torch.dtype, dev: torch.device):
    """``new(want, *shape)``: an uninitialised ``batch + shape`` tensor for an output that was asked for, ``None`` (NULL to the
    kernel) for one that was not."""
    return lambda want, *shape: torch.empty(batch + shape, dtype=dtype, device=dev) if want else None


def _workspace(size_fn, dev: torch.device, *dims):
    """``(ws, ws_bytes)`` as an entry point takes them, from its ``*_workspace_bytes`` function."""
    ws_bytes = int(size_fn(*dims))
    return _lib.workspace(ws_bytes, dev), ws_bytes


def _written_in_place(*tensors: torch.Tensor) -> None:
    """A kernel wrote these through raw pointers: tell torch, so that whatever keys a cache on (tensor, version) sees the write."""
    for t in tensors:
        torch.autograd.graph.increment_version(t)


class _PredictLogDensity:
    """Mixin of the models with a likelihood: ``kernel``, ``likelihood`` and ``predict_log_density`` on top of the class's
    ``_predict_f(new_time_points) -> (f_mean, f_var)``."""

    @property
    def kernel(self) -> SDEKernel:
        return self._kernel

    @property
    def likelihood(self) -> Likelihood:
        return self._likelihood

    def predict_log_density(self, input_data: Tuple[torch.Tensor, torch.Tensor], full_output_cov: bool = False) -> torch.Tensor:
        """Log density of new data ``(time_points, observations)`` under the posterior, ``batch + [num_new]``
        (variational_cvi.py:406-420, sparse_variational.py:262-270)."""
        if full_output_cov:
            raise NotImplementedError("predict_log_density: the likelihoods are univariate (marginal variances only)")
        new_times, new_obs = input_data
        f_mean, f_var = self._predict_f(new_times)
        return self._likelihood.predict_log_density(f_mean, f_var, new_obs)


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


def gradient_correction(inputs: Tuple[torch.Tensor, torch.Tensor], grads: Tuple[torch.Tensor, torch.Tensor]
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The EP step in natural parameters from the derivatives ``(g1, g2)`` of the log expected density in the mean, taken at the
    cavity ``inputs = (mu, var)`` (pep.py:250-261): ``L2 = 1 / (2 (var + 1 / g2))``, ``L1 = 2 L2 (g1 / g2 - mu)``, written without
    the division by ``g2``: ``den = 1 + var g2``, ``L2 = g2 / (2 den)``, ``L1 = (g1 - mu g2) / den``."""
    den = 1.0 + inputs[1] * grads[1]
    return (grads[0] - inputs[0] * grads[1]) / den, 0.5 * grads[1] / den
