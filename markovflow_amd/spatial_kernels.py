"""
Stationary kernels on a spatial input ``x in R^Dx``: what ``kernels.SparseSpatioTemporalKernel`` and
``models.SpatioTemporalSparseVariational`` take as ``kernel_space`` (the reference takes gpflow kernels there,
markovflow/models/spatio_temporal_variational.py:56).  Plain torch on any device, differentiable by autograd; they see ``Ms`` inducing
points and one weight row per data point, never an ``N x N`` matrix, and are not a hot path.
"""
import abc
import math
from typing import Optional, Sequence, Tuple, Union

import torch

Hyper = Union[float, Sequence[float], torch.Tensor]


class SpatialKernel(abc.ABC):
    """``k(x, x') = variance * rho(|(x - x') / lengthscales|)`` on the columns ``active_dims`` of the input.  ``variance`` is a scalar
    tensor, ``lengthscales`` a scalar or one value per active dimension; both are the ``trainable_variables`` (give them
    ``requires_grad_()`` to train them; they must stay positive)."""

    def __init__(self, variance: Hyper = 1.0, lengthscales: Hyper = 1.0, active_dims: Optional[Sequence[int]] = None, device=None,
                 dtype=torch.float64) -> None:
        as_tensor = lambda v: v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=dtype, device=device)  # noqa: E731
        self.variance = as_tensor(variance)
        self.lengthscales = as_tensor(lengthscales)
        if self.variance.dim() != 0 or self.lengthscales.dim() > 1:
            raise ValueError("variance must be a scalar and lengthscales a scalar or a vector with one value per active dimension")
        if not bool(self.variance > 0) or not bool((self.lengthscales > 0).all()):
            raise ValueError("variance and lengthscales must be positive")
        self.active_dims = None if active_dims is None else [int(i) for i in active_dims]
        if self.lengthscales.dim() == 1 and self.active_dims is not None and len(self.active_dims) != self.lengthscales.shape[0]:
            raise ValueError("lengthscales must have one value per active dimension")

    @property
    def trainable_variables(self) -> Tuple[torch.Tensor, ...]:
        return self.variance, self.lengthscales

    _leaves = trainable_variables.fget

    def _scaled(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() < 2:
            raise ValueError(f"spatial inputs must have shape [..., num_points, num_dims], got {tuple(x.shape)}")
        if self.active_dims is not None:
            x = x[..., self.active_dims]
        if self.lengthscales.dim() == 1 and self.lengthscales.shape[0] != x.shape[-1]:
            raise ValueError(f"{self.lengthscales.shape[0]} lengthscales for inputs of {x.shape[-1]} active dimensions")
        return x / self.lengthscales.to(dtype=x.dtype, device=x.device)

    def _sq_dist(self, x: torch.Tensor, x2: Optional[torch.Tensor]) -> torch.Tensor:
        """Scaled squared distances ``[..., N, N2]`` as a sum of squared differences: exact zeros on the diagonal."""
        xs = self._scaled(x)
        x2s = xs if x2 is None else self._scaled(x2)
        diff = xs[..., :, None, :] - x2s[..., None, :, :]
        return torch.sum(diff * diff, dim=-1)

    @abc.abstractmethod
    def _rho(self, r2: torch.Tensor) -> torch.Tensor:
        """The correlation as a function of the scaled squared distance."""

    def K(self, X: torch.Tensor, X2: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``[..., N, N2]`` (``X2 = X`` when omitted)."""
        r2 = self._sq_dist(X, X2)
        return self.variance.to(dtype=r2.dtype, device=r2.device) * self._rho(r2)

    def K_diag(self, X: torch.Tensor) -> torch.Tensor:
        """``[..., N]``: the variance."""
        return self.variance.to(dtype=X.dtype, device=X.device).expand(tuple(X.shape[:-1]))

    __call__ = K


def _safe_sqrt(r2: torch.Tensor) -> torch.Tensor:
    """``sqrt`` with a zero gradient at zero (the Matern kernels are differentiable there through their own form)."""
    positive = r2 > 0
    return torch.where(positive, torch.sqrt(torch.where(positive, r2, torch.ones_like(r2))), torch.zeros_like(r2))


class SquaredExponential(SpatialKernel):
    """``rho(r) = exp(-r^2 / 2)``."""

    def _rho(self, r2):
        return torch.exp(-0.5 * r2)


class Matern12(SpatialKernel):
    """``rho(r) = exp(-r)``."""

    def _rho(self, r2):
        return torch.exp(-_safe_sqrt(r2))


class Matern32(SpatialKernel):
    """``rho(r) = (1 + sqrt(3) r) exp(-sqrt(3) r)``."""

    def _rho(self, r2):
        z = math.sqrt(3.0) * _safe_sqrt(r2)
        return (1.0 + z) * torch.exp(-z)


class Matern52(SpatialKernel):
    """``rho(r) = (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)``."""

    def _rho(self, r2):
        z = math.sqrt(5.0) * _safe_sqrt(r2)
        return (1.0 + z + (5.0 / 3.0) * r2) * torch.exp(-z)
