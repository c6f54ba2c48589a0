"""
Non-linear stochastic differential equations ``dx = f(x) dt + L dB`` (markovflow/sde/: ``sde.py``, ``drift.py``, ``sde_utils.py``,
flattened into one module as ``kernels.py`` and ``likelihoods.py`` flatten their packages):

* ``SDE`` with ``OrnsteinUhlenbeckSDE`` (``f = -lambda x``) and ``DoubleWellSDE`` (``f = 4 x (1 - x^2)``), ``LinearDrift``;
* ``euler_maruyama`` simulates paths;
* ``linearize_sde`` turns the SDE, linearised along a Gaussian path, into a ``StateSpaceModel``;
* ``squared_drift_difference_along_Gaussian_path`` is the Girsanov KL term of variational inference for diffusions.

Routing.  HIP tensors with a built-in SDE whose parameters are plain numbers take the kernels of ``csrc/mf_nlsde.hip``: one launch
for all steps of a simulation (state dimension up to 4), one launch for a linearisation, two for the drift difference with its four
derivatives.  CPU tensors, a subclass with its own Python ``drift``, a built-in whose ``decay`` or ``q`` is a tensor that requires a
gradient, and state dimensions above 4 take ``euler_maruyama_torch``, ``linearize_torch`` and ``squared_drift_difference_torch``:
the same arithmetic in torch, which is also what the kernels are timed against (scripts/bench_sde.py).

DEVIATIONS from the reference
* ``euler_maruyama`` takes the grid INCLUDING the start time: ``time_grid[0]`` is the time of ``x0`` and the grid may be non-uniform.
  The reference starts its clock at 0 implicitly and takes a homogeneous grid that begins at ``dt``; its output on ``grid`` is ours
  on ``[0, grid[:-1]]``.  The noise is an argument (or drawn with ``torch.randn`` under ``generator``): there is no in-kernel
  random number generator, so a run is reproducible from a torch seed.
* ``linearize_sde`` and the drift difference take ``(mean, covariance)`` tuples where the reference takes gpflow ``Gaussian``s.
* The drift difference supports leading batch dimensions and is differentiable once in the path and in the linear drift.
* ``LinearDrift.set_from_ssm`` keeps the batch dimensions of the chain (the reference squeezes a leading 1).
"""
import abc
import ctypes
import functools
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .state_space_model import StateSpaceModel

_MAX_POINTS = 32        # the rule travels in the kernel arguments
_MAX_FUSED_DIM = 4      # state dimension of the Euler-Maruyama kernel


@functools.lru_cache(maxsize=None)
def _host_rule(nq: int):
    """Nodes and weights of the ``nq`` point Gauss-Hermite rule (float64; the weights sum to sqrt(pi)), as numpy and for the C ABI."""
    if nq != int(nq) or not 1 <= int(nq) <= _MAX_POINTS:
        raise ValueError(f"the number of Gauss-Hermite points must be an integer in 1..{_MAX_POINTS}, got {nq}")
    nq = int(nq)
    nodes, weights = np.polynomial.hermite.hermgauss(nq)
    return nodes, weights, (ctypes.c_double * nq)(*nodes), (ctypes.c_double * nq)(*weights)


@functools.lru_cache(maxsize=None)
def _torch_rule(nq: int, dtype: torch.dtype, device: torch.device):
    nodes, weights, _, _ = _host_rule(nq)
    return (torch.as_tensor(nodes, dtype=dtype, device=device), torch.as_tensor(weights / math.sqrt(math.pi), dtype=dtype, device=device))


def _trainable(value) -> bool:
    return isinstance(value, torch.Tensor) and value.requires_grad


class SDE(abc.ABC):
    """``dx(t) = f(x(t), t) dt + l(x(t), t) dB(t)`` (sde.py:23-129)."""

    _id = -1            # the drift id the kernels take; a subclass with its own Python drift has none

    def __init__(self, state_dim: int = 1, num_gauss_hermite_points: int = 10) -> None:
        self._state_dim = int(state_dim)
        _host_rule(num_gauss_hermite_points)
        self.num_gauss_hermite_points = int(num_gauss_hermite_points)

    @property
    def state_dim(self) -> int:
        return self._state_dim

    @abc.abstractmethod
    def drift(self, x: torch.Tensor, t: Optional[torch.Tensor]) -> torch.Tensor:
        """``f(x, t)``: ``[n, state_dim]`` (``t`` ``[n, 1]`` or None) to ``[n, state_dim]``."""

    @abc.abstractmethod
    def diffusion(self, x: torch.Tensor, t: Optional[torch.Tensor]) -> torch.Tensor:
        """``l(x, t)``: ``[n, state_dim]`` to ``[n, state_dim, state_dim]``."""

    def gradient_drift(self, x: torch.Tensor, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``df/dx`` of a drift that acts element-wise, by autograd, with the shape of ``x`` (sde.py:73-88: the reference's tape
        likewise sums the drift's outputs).  Differentiable further when grad mode is on."""
        keep = torch.is_grad_enabled()
        with torch.enable_grad():
            xs = x if x.requires_grad else x.detach().requires_grad_(True)
            (grad,) = torch.autograd.grad(self.drift(xs, t).sum(), xs, create_graph=keep)
        return grad if keep else grad.detach()

    def _fusable(self) -> bool:
        """True when the kernels can stand for this SDE: a built-in drift with plain numbers for parameters."""
        return False

    def _drift_args(self):
        """``(drift id, host array of its parameters or None)``."""
        raise NotImplementedError

    def _moments(self, q_mean: torch.Tensor, q_covar: torch.Tensor, fn) -> torch.Tensor:
        if q_mean.dim() != 3 or tuple(q_covar.shape) != tuple(q_mean.shape) + (q_mean.shape[-1],):
            raise ValueError(f"expected q_mean [batch, num_states, state_dim] and q_covar [batch, num_states, state_dim, state_dim], "
                             f"got {tuple(q_mean.shape)} and {tuple(q_covar.shape)}")
        bsz, n, d = q_mean.shape
        x, w = _torch_rule(self.num_gauss_hermite_points, q_mean.dtype, q_mean.device)
        if d == 1:
            pts = _points(q_mean[..., 0], q_covar[..., 0, 0], x)                                # [B, N, nq]
            vals = fn(pts.reshape(-1, 1)).reshape(pts.shape)
            return _nan_outside(q_covar[..., 0, 0], torch.sum(w * vals, dim=-1))[..., None]
        # the tensor-product rule on the Cholesky factor (gpflow's mvnquad)
        grid = torch.cartesian_prod(*([x] * d)).reshape(-1, d)
        wts = torch.cartesian_prod(*([w] * d)).reshape(-1, d).prod(dim=-1)
        chol = torch.linalg.cholesky(q_covar)
        pts = q_mean[..., None, :] + math.sqrt(2.0) * torch.einsum("bnij,pj->bnpi", chol, grid)
        vals = fn(pts.reshape(-1, d)).reshape(pts.shape)
        return torch.sum(wts[:, None] * vals, dim=-2)

    def expected_drift(self, q_mean: torch.Tensor, q_covar: torch.Tensor) -> torch.Tensor:
        """``E_{N(q_mean, q_covar)} f(x)``, ``[batch, num_states, state_dim]`` (sde.py:90-110), by Gauss-Hermite quadrature."""
        return self._moments(q_mean, q_covar, lambda pts: self.drift(pts, None))

    def expected_gradient_drift(self, q_mean: torch.Tensor, q_covar: torch.Tensor) -> torch.Tensor:
        """``E_{N(q_mean, q_covar)} f'(x)``, ``[batch, num_states, state_dim]`` (sde.py:112-129)."""
        return self._moments(q_mean, q_covar, lambda pts: self.gradient_drift(pts, None))


class _ConstantDiffusionSDE(SDE):
    """What the two built-ins share: ``L = chol(q)``, ``q`` ``[D, D]``, kept as a tensor for the torch route and as host numbers
    for the kernels."""

    def __init__(self, q, num_gauss_hermite_points: int = 10) -> None:
        q = q if isinstance(q, torch.Tensor) else torch.as_tensor(q, dtype=torch.float64)
        if q.dim() != 2 or q.shape[0] != q.shape[1] or q.shape[0] < 1:
            raise ValueError(f"{type(self).__name__}: q must have shape [state_dim, state_dim], got {tuple(q.shape)}")
        super().__init__(state_dim=q.shape[0], num_gauss_hermite_points=num_gauss_hermite_points)
        self.q = q
        self._host_chol = None
        if not _trainable(q):
            q64 = q.detach().to("cpu", torch.float64).numpy()
            chol = np.linalg.cholesky(q64)                          # raises on a q that is not positive definite
            self._host_chol, self._host_q = chol, q64
            self._packed_chol = (ctypes.c_double * (len(chol) * (len(chol) + 1) // 2))(*[chol[i, j] for i in range(len(chol))
                                                                                         for j in range(i + 1)])

    def _chol(self, ref: torch.Tensor) -> torch.Tensor:
        if self._host_chol is not None:
            return torch.as_tensor(self._host_chol, dtype=ref.dtype, device=ref.device)
        return torch.linalg.cholesky(self.q.to(dtype=ref.dtype, device=ref.device))

    def diffusion(self, x: torch.Tensor, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        return torch.ones_like(x[..., None]) * self._chol(x)

    def _fusable(self) -> bool:
        cls = type(self)
        builtin = next(c for c in cls.__mro__ if c in (OrnsteinUhlenbeckSDE, DoubleWellSDE))
        own = all(getattr(cls, name) is getattr(builtin, name) for name in ("drift", "gradient_drift", "diffusion"))
        return own and self._host_chol is not None and not _trainable(self.q)


class OrnsteinUhlenbeckSDE(_ConstantDiffusionSDE):
    """``dx = -lambda x dt + chol(q) dB`` (sde.py:132-174)."""

    _id = 0

    def __init__(self, decay, q=((1.0,),), num_gauss_hermite_points: int = 10) -> None:
        super().__init__(q, num_gauss_hermite_points)
        self.decay = decay

    def _decay(self, ref: torch.Tensor):
        return self.decay.to(dtype=ref.dtype, device=ref.device) if isinstance(self.decay, torch.Tensor) else self.decay

    def drift(self, x: torch.Tensor, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        return -self._decay(x) * x

    def gradient_drift(self, x: torch.Tensor, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        return -self._decay(x) * torch.ones_like(x)

    def _fusable(self) -> bool:
        return super()._fusable() and not _trainable(self.decay)

    def _drift_args(self):
        return self._id, (ctypes.c_double * 1)(float(self.decay))


class DoubleWellSDE(_ConstantDiffusionSDE):
    """``dx = 4 x (1 - x^2) dt + chol(q) dB`` (sde.py:177-219)."""

    _id = 1

    def __init__(self, q=((1.0,),), num_gauss_hermite_points: int = 10) -> None:
        super().__init__(q, num_gauss_hermite_points)

    def drift(self, x: torch.Tensor, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        return 4.0 * x * (1.0 - x * x)

    def gradient_drift(self, x: torch.Tensor, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        return 4.0 - 12.0 * x * x

    def _drift_args(self):
        return self._id, None


class LinearDrift:
    """``f(x, t) = A_t x + b_t`` (drift.py:24-108): ``A`` ``batch + [num_transitions, D, D]``, ``b`` ``batch + [num_transitions, D]``."""

    def __init__(self, A: Optional[torch.Tensor] = None, b: Optional[torch.Tensor] = None) -> None:
        self.A = A
        self.b = b

    def set_from_ssm(self, ssm: StateSpaceModel, dt: float) -> None:
        """First order in ``dt``: ``A = (state_transitions - I) / dt``, ``b = state_offsets / dt``."""
        a_s = ssm.state_transitions
        self.A = (a_s - torch.eye(ssm.state_dim, dtype=a_s.dtype, device=a_s.device)) / dt
        self.b = ssm.state_offsets / dt

    def to_ssm(self, q: torch.Tensor, transition_times: torch.Tensor, initial_mean: torch.Tensor,
               initial_chol_covariance: torch.Tensor) -> StateSpaceModel:
        """``state_transitions = I + A dt_k``, ``state_offsets = b dt_k``, ``chol_process_covariances = q sqrt(dt_k)`` - ``q`` is
        the DIFFUSION ``[B, N, D, D]``, as in the reference."""
        if self.A is None or self.b is None:
            raise ValueError("LinearDrift.to_ssm: the linear drift is empty")
        a_d = self.A if self.A.dim() == 4 else self.A[None]
        b_d = self.b if self.b.dim() == 3 else self.b[None]
        q = q if q.dim() == 4 else q[None]
        initial_mean = initial_mean if initial_mean.dim() == 2 else initial_mean[None]
        initial_chol_covariance = initial_chol_covariance if initial_chol_covariance.dim() == 3 else initial_chol_covariance[None]
        bsz, n, d = b_d.shape
        if tuple(a_d.shape) != (bsz, n, d, d) or tuple(q.shape) != (bsz, n, d, d) or tuple(transition_times.shape) != (n + 1,):
            raise ValueError(f"LinearDrift.to_ssm: A {tuple(a_d.shape)}, b {tuple(b_d.shape)}, q {tuple(q.shape)} and transition_times "
                             f"{tuple(transition_times.shape)} do not agree")
        deltas = (transition_times[1:] - transition_times[:-1]).reshape(1, -1, 1)
        eye = torch.eye(d, dtype=a_d.dtype, device=a_d.device)
        return StateSpaceModel(initial_mean, initial_chol_covariance, a_d * deltas[..., None] + eye, b_d * deltas,
                               q * torch.sqrt(deltas)[..., None])


# ---- Gauss-Hermite helpers of the torch routes (state dimension 1) ---------------------------------------------------------------
def _points(m: torch.Tensor, var: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """``m + sqrt(2 var) x_i``, ``[..., nq]``; outside the domain the points of variance 1 (the caller overwrites the result)."""
    safe = torch.where(var > 0, var, torch.ones_like(var))
    return m[..., None] + torch.sqrt(2.0 * safe)[..., None] * x


def _nan_outside(var: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
    return torch.where(var > 0, value, torch.full_like(value, float("nan")))


def _eval(fn, pts: torch.Tensor) -> torch.Tensor:
    return fn(pts.reshape(-1, 1), None).reshape(pts.shape)


def _need_dim_one(sde: SDE, what: str) -> None:
    if sde.state_dim != 1:
        raise NotImplementedError(f"{what} supports state_dim == 1 only (as the reference), got an SDE of state_dim {sde.state_dim}")


def _scalar_q(sde: SDE, ref: torch.Tensor):
    q = getattr(sde, "q", None)
    if q is None:
        raise ValueError("the SDE has no spectral density `q`")
    return q.to(dtype=ref.dtype, device=ref.device).reshape(()) if isinstance(q, torch.Tensor) else float(q)


# ---- Euler-Maruyama --------------------------------------------------------------------------------------------------------------
def euler_maruyama_torch(sde: SDE, x0: torch.Tensor, time_grid: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """The recurrence of ``euler_maruyama`` as torch operations, about five per step; differentiable."""
    dts = time_grid[1:] - time_grid[:-1]
    sqs = torch.sqrt(dts)
    x, out = x0, [x0]
    for k in range(time_grid.shape[0] - 1):
        t = time_grid[k].expand(x0.shape[0], 1)
        x = x + sde.drift(x, t) * dts[k] + sqs[k] * (sde.diffusion(x, t) @ noise[:, k, :, None])[..., 0]
        out.append(x)
    return torch.stack(out, dim=1)


def euler_maruyama(sde: SDE, x0: torch.Tensor, time_grid: torch.Tensor, noise: Optional[torch.Tensor] = None,
                   generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """
    Simulate ``out[:, 0] = x0``, ``out[:, k + 1] = out[:, k] + f(out[:, k]) dt_k + sqrt(dt_k) L xi_k`` with
    ``dt_k = time_grid[k + 1] - time_grid[k]`` (sde_utils.py:29-84; see the module docstring for the grid convention).

    :param x0: ``[B, D]``, the state at ``time_grid[0]``.
    :param time_grid: ``[T]``, strictly increasing, possibly non-uniform (a non-positive step gives NaN from its square root).
    :param noise: ``[B, T - 1, D]`` standard normal draws; None: drawn with ``torch.randn`` under ``generator``.
    :return: ``[B, T, D]``.

    HIP tensors with a built-in SDE and ``D <= 4``: ONE launch of ``mf_nlsde_euler_maruyama_*`` for all steps.  That route is not
    differentiable - it is refused when grad mode is on and an input requires a gradient; ``euler_maruyama_torch`` is.
    """
    if x0.dim() != 2 or x0.shape[-1] != sde.state_dim:
        raise ValueError(f"euler_maruyama: x0 must have shape [num_batch, {sde.state_dim}], got {tuple(x0.shape)}")
    if time_grid.dim() != 1 or time_grid.shape[0] < 1:
        raise ValueError(f"euler_maruyama: time_grid must have shape [num_time_points], got {tuple(time_grid.shape)}")
    if x0.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {x0.dtype}")
    bsz, d = x0.shape
    steps = time_grid.shape[0] - 1
    if noise is None:
        noise = torch.randn((bsz, steps, d), dtype=x0.dtype, device=x0.device, generator=generator)
    elif tuple(noise.shape) != (bsz, steps, d):
        raise ValueError(f"euler_maruyama: noise must have shape {(bsz, steps, d)}, got {tuple(noise.shape)}")
    _lib.same_dtype_device(x0, "euler_maruyama", time_grid=time_grid, noise=noise)
    if not x0.is_cuda and steps > 0 and not bool((time_grid[1:] > time_grid[:-1]).all()):
        raise ValueError("euler_maruyama: time_grid must be strictly increasing")
    if not (x0.is_cuda and sde._fusable() and d <= _MAX_FUSED_DIM):
        return euler_maruyama_torch(sde, x0, time_grid, noise)
    if torch.is_grad_enabled() and (x0.requires_grad or noise.requires_grad or time_grid.requires_grad):
        raise NotImplementedError("euler_maruyama: the fused simulation is not differentiable and an input requires a gradient; "
                                  "use euler_maruyama_torch, detach() the inputs or wrap the call in torch.no_grad()")
    with torch.no_grad():
        x0c, grid, xi = x0.contiguous(), time_grid.contiguous(), noise.contiguous()
        out = torch.empty((bsz, steps + 1, d), dtype=x0.dtype, device=x0.device)
        drift_id, params = sde._drift_args()
        _lib.call("mf_nlsde_euler_maruyama", x0.dtype, bsz, steps + 1, d, drift_id, params, sde._packed_chol, _lib.ptr(x0c),
                  _lib.ptr(grid), _lib.ptr(xi), _lib.ptr(out), _lib.stream_ptr(x0.device))
    return out


# ---- linearisation ---------------------------------------------------------------------------------------------------------------
def linearize_torch(sde: SDE, transition_times: torch.Tensor, mean: torch.Tensor, var: torch.Tensor):
    """``(A, b, chol Q)``, each ``[B, N]``, from the path marginals ``mean``, ``var`` ``[B, N]`` of a one-dimensional SDE, as torch
    operations over ``[B, N, nq]`` temporaries: ``A = 1 + E f' dt``, ``b = (E f - E f' m) dt``, ``chol Q = L sqrt(dt)``."""
    x, w = _torch_rule(sde.num_gauss_hermite_points, mean.dtype, mean.device)
    dts = transition_times[1:] - transition_times[:-1]
    pts = _points(mean, var, x)
    e_f = torch.sum(w * _eval(sde.drift, pts), dim=-1)
    e_fp = torch.sum(w * _eval(sde.gradient_drift, pts), dim=-1)
    a_s = _nan_outside(var, 1.0 + e_fp * dts)
    b_s = _nan_outside(var, (e_f - e_fp * mean) * dts)
    chol = sde.diffusion(mean.reshape(-1, 1), None).reshape(mean.shape) * torch.sqrt(dts)
    return a_s, b_s, chol


def linearize_sde(sde: SDE, transition_times: torch.Tensor, linearization_path: Tuple[torch.Tensor, torch.Tensor],
                  initial_state: Tuple[torch.Tensor, torch.Tensor]) -> StateSpaceModel:
    """
    The SDE linearised along a Gaussian path as a ``StateSpaceModel`` (sde_utils.py:107-158), state dimension 1:
    ``A_k = 1 + E[f'] dt_k``, ``b_k = (E[f] - E[f'] m_k) dt_k``, ``chol Q_k = L sqrt(dt_k)`` with the expectations under
    ``N(m_k, S_k)`` by the SDE's Gauss-Hermite rule.

    :param transition_times: ``[N + 1]``.
    :param linearization_path: ``(mean [B, N, 1], covariance [B, N, 1, 1])`` (a missing batch dimension is added).
    :param initial_state: ``(mean [B, 1], covariance [B, 1, 1])``.

    A point whose variance is not positive gets NaN in its ``A`` and ``b``.  HIP tensors with a built-in SDE: one launch of
    ``mf_nlsde_linearize_*``, which writes the three tensors in the layout the chain takes.
    """
    _need_dim_one(sde, "linearize_sde")
    mean, cov = linearization_path
    mean0, cov0 = initial_state
    mean = mean if mean.dim() == 3 else mean[None]
    cov = cov if cov.dim() == 4 else cov[None]
    mean0 = mean0 if mean0.dim() == 2 else mean0[None]
    cov0 = cov0 if cov0.dim() == 3 else cov0[None]
    bsz, n = mean.shape[0], mean.shape[1]
    if tuple(mean.shape) != (bsz, n, 1) or tuple(cov.shape) != (bsz, n, 1, 1) or tuple(mean0.shape) != (bsz, 1) \
            or tuple(cov0.shape) != (bsz, 1, 1) or tuple(transition_times.shape) != (n + 1,):
        raise ValueError(f"linearize_sde: expected a path ([B, N, 1], [B, N, 1, 1]), an initial state ([B, 1], [B, 1, 1]) and "
                         f"transition_times [N + 1], got {tuple(mean.shape)}, {tuple(cov.shape)}, {tuple(mean0.shape)}, "
                         f"{tuple(cov0.shape)} and {tuple(transition_times.shape)}")
    _lib.same_dtype_device(mean, "linearize_sde", covariance=cov, initial_mean=mean0, initial_covariance=cov0,
                           transition_times=transition_times)
    chol0 = torch.sqrt(cov0)
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (mean, cov, transition_times))
    if mean.is_cuda and sde._fusable() and not needs_grad:
        with torch.no_grad():
            m, s, times = mean.contiguous(), cov.contiguous(), transition_times.contiguous()
            a_s, b_s, chol = torch.empty_like(s), torch.empty_like(m), torch.empty_like(s)
            drift_id, params = sde._drift_args()
            _, _, nodes, weights = _host_rule(sde.num_gauss_hermite_points)
            _lib.call("mf_nlsde_linearize", m.dtype, bsz, n, drift_id, params, float(sde._host_chol[0, 0]),
                      sde.num_gauss_hermite_points, nodes, weights, _lib.ptr(times), _lib.ptr(m), _lib.ptr(s), _lib.ptr(a_s),
                      _lib.ptr(b_s), _lib.ptr(chol), _lib.stream_ptr(m.device))
    else:
        a_s, b_s, chol = linearize_torch(sde, transition_times, mean[..., 0], cov[..., 0, 0])
        a_s, b_s, chol = a_s[..., None, None], b_s[..., None], chol[..., None, None]
    return StateSpaceModel(mean0, chol0, a_s, b_s, chol)


# ---- drift difference ------------------------------------------------------------------------------------------------------------
def squared_drift_difference_torch(sde_p: SDE, mean: torch.Tensor, var: torch.Tensor, a_d: torch.Tensor, b_d: torch.Tensor, dt: float,
                                   quadrature_pnts: int = 20) -> torch.Tensor:
    """``1/2 sum_k E_{N(m_k, S_k)} (A_k x + b_k - f(x))^2 dt / q`` over the last dimension of ``[..., N]`` inputs, as torch operations
    over ``[..., N, nq]`` temporaries; differentiable by autograd in everything, the SDE's parameters included."""
    x, w = _torch_rule(int(quadrature_pnts), mean.dtype, mean.device)
    pts = _points(mean, var, x)
    resid = (a_d[..., None] * pts + b_d[..., None]) - _eval(sde_p.drift, pts)
    per_point = _nan_outside(var, 0.5 * torch.sum(w * resid * resid, dim=-1) * (dt / _scalar_q(sde_p, mean)))
    return per_point.sum(dim=-1)


def _drift_difference_parts(sde_p: SDE, mean, var, a_d, b_d, scale: float, nq: int):
    """``(sum [B], g_m, g_S, g_A, g_b [B, N])`` from ``[B, N]`` inputs: the kernels on HIP tensors, the same sums in torch otherwise."""
    bsz, n = mean.shape
    if mean.is_cuda:
        outs = [torch.empty_like(mean) for _ in range(4)]
        total = torch.empty((bsz,), dtype=mean.dtype, device=mean.device)
        nbytes = int(_lib.load().mf_nlsde_drift_difference_workspace_bytes(bsz, n))
        ws = _lib.workspace(nbytes, mean.device)
        drift_id, params = sde_p._drift_args()
        _, _, nodes, weights = _host_rule(nq)
        _lib.call("mf_nlsde_drift_difference", mean.dtype, bsz, n, drift_id, params, nq, nodes, weights, scale, _lib.ptr(mean),
                  _lib.ptr(var), _lib.ptr(a_d), _lib.ptr(b_d), _lib.ptr(total), *[_lib.ptr(o) for o in outs],
                  None if ws is None else ctypes.c_void_p(ws.data_ptr()), nbytes, _lib.stream_ptr(mean.device))
        return (total, *outs)
    x, w = _torch_rule(nq, mean.dtype, mean.device)
    pts = _points(mean, var, x)
    resid = (a_d[..., None] * pts + b_d[..., None]) - _eval(sde_p.drift, pts)
    wr = w * resid
    wrs = wr * (a_d[..., None] - _eval(sde_p.gradient_drift, pts))
    sd = torch.sqrt(2.0 * torch.where(var > 0, var, torch.ones_like(var)))
    parts = (0.5 * torch.sum(wr * resid, dim=-1) * scale, torch.sum(wrs, dim=-1) * scale, torch.sum(wrs * x, dim=-1) / sd * scale,
             torch.sum(wr * pts, dim=-1) * scale, torch.sum(wr, dim=-1) * scale)
    value, g_m, g_s, g_a, g_b = (_nan_outside(var, part) for part in parts)
    return value.sum(dim=-1), g_m, g_s, g_a, g_b


class _DriftDifference(torch.autograd.Function):
    """The per-series value ``[B]`` with the four derivatives per point computed in the same pass and saved for the backward."""

    @staticmethod
    def forward(ctx, mean, var, a_d, b_d, sde_p, scale, nq):
        with torch.no_grad():
            total, g_m, g_s, g_a, g_b = _drift_difference_parts(sde_p, mean.detach().contiguous(), var.detach().contiguous(),
                                                                a_d.detach().contiguous(), b_d.detach().contiguous(), scale, nq)
        ctx.save_for_backward(g_m, g_s, g_a, g_b)
        return total

    @staticmethod
    def backward(ctx, grad_out):
        if torch.is_grad_enabled():
            raise RuntimeError("squared_drift_difference_along_Gaussian_path is differentiable once: its backward uses the "
                               "derivatives computed in the forward and has no second-order support (create_graph=True)")
        g = grad_out[..., None]
        return tuple(g * t for t in ctx.saved_tensors) + (None, None, None)


def squared_drift_difference_along_Gaussian_path(sde_p: SDE, linear_drift: LinearDrift, q: Tuple[torch.Tensor, torch.Tensor], dt: float,
                                                 quadrature_pnts: int = 20) -> torch.Tensor:
    """
    ``1/2 sum_k E_{N(m_k, S_k)}[(A_k x + b_k - f(x))^2] / q dt`` (sde_utils.py:161-228): the expected log density ratio between the
    linear drift and ``sde_p`` along the Gaussian path ``q = (mean batch + [N, 1], covariance batch + [N, 1, 1])``; with the linear
    drift of ``q`` itself, ``KL[q || p]``.  ``linear_drift.A`` is ``batch + [N, 1, 1]``, ``linear_drift.b`` ``batch + [N, 1]``.
    State dimension 1.  Returns shape ``batch``.

    Differentiable ONCE in the path and in the linear drift: the forward computes the four derivatives of the discretised sum per
    point alongside the value.  A point with ``S <= 0`` or NaN makes its series NaN.  An SDE with a Python drift of its own or with
    trainable parameters goes through ``squared_drift_difference_torch`` and plain autograd instead.
    """
    _need_dim_one(sde_p, "squared_drift_difference_along_Gaussian_path")
    mean, cov = q
    a_d, b_d = linear_drift.A, linear_drift.b
    if a_d is None or b_d is None:
        raise ValueError("squared_drift_difference_along_Gaussian_path: the linear drift is empty")
    if mean.dim() < 2 or mean.shape[-1] != 1 or tuple(cov.shape) != tuple(mean.shape) + (1,) or tuple(a_d.shape) != tuple(cov.shape) \
            or tuple(b_d.shape) != tuple(mean.shape):
        raise ValueError(f"squared_drift_difference_along_Gaussian_path: expected mean and b batch + [N, 1], covariance and A "
                         f"batch + [N, 1, 1], got {tuple(mean.shape)}, {tuple(b_d.shape)}, {tuple(cov.shape)}, {tuple(a_d.shape)}")
    if mean.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {mean.dtype}")
    _lib.same_dtype_device(mean, "squared_drift_difference_along_Gaussian_path", covariance=cov, A=a_d, b=b_d)
    nq = int(quadrature_pnts)
    _host_rule(nq)
    batch, n = tuple(mean.shape[:-2]), mean.shape[-2]
    flat = [t.reshape(-1, n) for t in (mean, cov, a_d, b_d)]
    if sde_p._fusable():
        out = _DriftDifference.apply(*flat, sde_p, float(dt) / float(sde_p._host_q[0, 0]), nq)
    else:
        out = squared_drift_difference_torch(sde_p, *flat, dt, nq)
    return out.reshape(batch)
