"""
Natural-gradient optimiser for a variational ``StateSpaceModel`` (mirror of ``markovflow/ssm_natgrad.py:33-218``).

With ``eta`` the expectation parameters and ``theta`` the natural parameters of the Gaussian the chain describes, the natural gradient
of a loss ``L`` in ``theta`` is ``dL/d eta`` (Salimbeni, Eleftheriadis & Hensman 2018, eq. 10).  It is obtained by the chain rule
from the ordinary gradient in the chain's parameters: ``dL/d eta`` is the vector-Jacobian product of ``expectations_to_ssm_params``
with ``dL/d(ssm parameters)`` as cotangent.  The step is taken in ``theta`` and mapped back with ``naturals_to_ssm_params``; every
transform is the HIP-backed one of ``ssm_gaussian_transformations``.

Two departures from a literal port.  The transforms return ``(As, offsets, chol_P0, chol_Qs, mu0)`` while
``StateSpaceModel.trainable_variables`` is in constructor order ``(mu0, chol_P0, As, offsets, chol_Qs)``: cotangents and new values are
matched by NAME.  And the moving average of the Fisher norm is kept PER SERIES (shape ``batch_shape``), not as one scalar over the
batch: a series inside a batch evolves exactly as it does alone; for ``batch_shape = ()`` this is the reference.
"""
from typing import Callable, Optional

import torch

from .ssm_gaussian_transformations import (expectations_to_ssm_params, naturals_to_ssm_params, ssm_to_expectations,
                                           ssm_to_naturals)
from .state_space_model import StateSpaceModel

# the names of what the transforms return, in their order, and of ``StateSpaceModel.trainable_variables``, in the constructor's order
_PARAM_NAMES = ("state_transitions", "state_offsets", "chol_initial_covariance", "chol_process_covariances", "initial_mean")
_LEAF_NAMES = ("initial_mean", "chol_initial_covariance", "state_transitions", "state_offsets", "chol_process_covariances")
_CHOLESKY_NAMES = ("chol_initial_covariance", "chol_process_covariances")


class SSMNaturalGradient:
    """``theta <- theta - gamma dL/d eta``, or with momentum the Adam-like step on moving averages of the natural gradient and of
    its Fisher norm ``g~^T F g~ = sum g~ . dL/d theta`` (ssm_natgrad.py:176-208)."""

    def __init__(self, gamma: float = 0.1, momentum: bool = True, beta1: float = 0.9, beta2: float = 0.99,
                 epsilon: float = 1e-8) -> None:
        if not gamma > 0.0:
            raise ValueError(f"gamma must be positive, got {gamma}")
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"beta1 and beta2 must lie in [0, 1), got {beta1} and {beta2}")
        if not epsilon >= 0.0:
            raise ValueError(f"epsilon must not be negative, got {epsilon}")
        self.gamma = float(gamma)
        self._momentum = bool(momentum)
        self._beta1, self._beta2, self._epsilon = float(beta1), float(beta2), float(epsilon)
        self._ms = None                 # moving averages of the natural gradient, one per expectation parameter
        self._v = None                  # moving average of its Fisher norm, shape batch_shape
        self._step_counter = 1
        self._effective_lr: Optional[torch.Tensor] = None

    @property
    def effective_lr(self):
        """The step actually taken in ``theta`` per unit of averaged natural gradient: ``gamma`` without momentum, the debiased rate
        over ``sqrt(v) + epsilon`` (a tensor of shape ``batch_shape``) after a momentum step."""
        return self.gamma if self._effective_lr is None else self._effective_lr

    def minimize(self, loss_fn: Callable[[], torch.Tensor], ssm: StateSpaceModel) -> None:
        """One natural-gradient step on ``ssm`` - a trainable copy, updated IN PLACE - for the scalar ``loss_fn()``."""
        leaves = getattr(ssm, "trainable_variables", ())
        if not isinstance(ssm, StateSpaceModel) or len(leaves) != len(_LEAF_NAMES):
            raise ValueError("SSMNaturalGradient.minimize: ssm must be a StateSpaceModel made by create_trainable_copy()")
        leaf = dict(zip(_LEAF_NAMES, leaves))
        with torch.enable_grad():
            loss = loss_fn()
            grads = torch.autograd.grad(loss, leaves, allow_unused=True)
        grad = {name: torch.zeros_like(leaf[name]) if g is None else g for name, g in zip(_LEAF_NAMES, grads)}
        for name in _CHOLESKY_NAMES:                                   # the Cholesky leaves are lower-triangular
            grad[name] = torch.tril(grad[name])
        dl_dssm = tuple(grad[name] for name in _PARAM_NAMES)           # cotangents in the transforms' order, matched by name

        def pulled_back(transform, point):
            """The VJP of ``transform`` at ``point`` (detached, made leaves) with ``dl_dssm`` as cotangent."""
            point = tuple(p.detach().clone().requires_grad_(True) for p in point)
            with torch.enable_grad():
                params = transform(*point)
                return torch.autograd.grad(params, point, grad_outputs=dl_dssm, allow_unused=True)

        with torch.no_grad():
            etas = ssm_to_expectations(ssm)
            thetas = ssm_to_naturals(ssm)
        dl_detas = pulled_back(expectations_to_ssm_params, etas)
        if self._momentum:
            dl_dthetas = pulled_back(naturals_to_ssm_params, thetas)
        with torch.no_grad():
            if self._momentum:
                if self._ms is None:
                    self._ms = [torch.zeros_like(e) for e in etas]
                    self._v = torch.zeros(tuple(ssm.batch_shape), dtype=etas[0].dtype, device=etas[0].device)
                t = self._step_counter
                lr = self.gamma * (1.0 - self._beta2 ** t) ** 0.5 / (1.0 - self._beta1 ** t)
                self._ms = [m * self._beta1 + (1.0 - self._beta1) * g for m, g in zip(self._ms, dl_detas)]
                nb = len(ssm.batch_shape)
                norm = [torch.sum(g * gt, dim=tuple(range(nb, g.dim()))) for g, gt in zip(dl_detas, dl_dthetas)]
                norm = norm[0] + norm[1] + 2.0 * norm[2]              # the sub-diagonal blocks stand for both triangles
                self._v = self._v * self._beta2 + (1.0 - self._beta2) * norm
                rate = lr / (torch.sqrt(self._v) + self._epsilon)
                thetas_new = [th - rate.reshape(rate.shape + (1,) * (th.dim() - nb)) * m for th, m in zip(thetas, self._ms)]
                self._step_counter += 1
                self._effective_lr = rate
            else:
                thetas_new = [th - self.gamma * g for th, g in zip(thetas, dl_detas)]
            new_params = naturals_to_ssm_params(*thetas_new)
            for name, value in zip(_PARAM_NAMES, new_params):
                leaf[name].copy_(value)                             # in place: the version counters bump, the caches see it
