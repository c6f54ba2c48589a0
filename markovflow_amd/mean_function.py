"""
Mean functions (mirror of ``markovflow/mean_function.py``): ``ZeroMeanFunction``, ``LinearMeanFunction`` and the two that model known
interventions through the kernel's own SDE ``dμ/dt = F μ + u(t)`` - ``ImpulseMeanFunction`` (a state kick ``u_k δ(t − τ_k)``) and
``StepMeanFunction`` (a constant forcing ``u_k`` on ``(τ_k, τ_{k+1}]``).

For one series with actions at ``τ_0 ≤ … ≤ τ_{K−1}`` and a query time ``t`` let ``j(t) = #{k : τ_k < t}`` (strict: the reference's
``searchsorted(..., side="left")`` - a point exactly on an action time does not yet see that action).  Then

    ``j = 0``:  the state mean is exactly zero;
    ``j > 0``:  ``s(t) = a_k + exp(F (t − τ_k)) c_k``,  ``k = j − 1``,  ``μ(t) = H s(t)``,

with ``c_0 = r_0``, ``c_k = exp(F (τ_k − τ_{k−1})) c_{k−1} + r_k``; impulse: ``a = 0``, ``r = u``; step: ``a_k = −F⁻¹ u_k``,
``r_0 = −a_0``, ``r_k = a_{k−1} − a_k``.

Two routes compute it.  On a HIP device, for kernels made of generalised components (Matérn, ``Constant``, ``HarmonicOscillator``,
``Product``, and ``Sum`` / ``IndependentMultiOutput`` of them) whose hyper-parameters, like the times, are not under a gradient, the
fused route runs: ``mf_mean_response_*`` (csrc/mf_sde.hip) - a coefficient scan and one evaluation kernel that builds every block of
``exp(FΔ)`` in registers, so that nothing of size ``d × d`` per point is ever written - differentiable once in ``state_perturbations``
through ``mf_mean_response_grad_*``.  Everything else (CPU tensors, a ``LatentExponentiallyGenerated`` kernel, hyper-parameters or
times under a gradient) takes the same recurrence and evaluation in differentiable torch operations.  ``fused = False`` forces the
torch route.

Before the first action the reference forms ``exp(F · negative gap) · 0``, which is ``inf · 0 = NaN`` for a point long before it;
here the product is skipped and the mean is an exact zero there.  This deviation is deliberate.

A NaN time point gives a NaN mean on both routes (it sorts behind every action, as in ``torch.searchsorted``, and its gap is NaN).

Action times are assumed sorted ascending per series (ties allowed: impulses at one time add).  This is NOT checked: on the device
path a check would force a host synchronisation.
"""
import abc
import ctypes
from typing import Union

import torch

from . import _lib
from .kernels import (Constant, IndependentMultiOutput, LatentExponentiallyGenerated, NonStationaryKernel, Product, SDEKernel,
                      SparseSpatioTemporalKernel, Sum, _MaternBase, _refuse_stack, to_delta_time)
from .models._common import _differentiable_once, _launch, _workspace

fused = True    # set False to force the torch route (the same mathematics in differentiable torch operations)


class MeanFunction(abc.ABC):
    """A mean function ``μ(t)`` of the observations (mean_function.py:27-62)."""

    @abc.abstractmethod
    def __call__(self, time_points: torch.Tensor) -> torch.Tensor:
        """``time_points [..., num_data]`` -> ``[..., num_data, obs_dim]``."""


class ZeroMeanFunction(MeanFunction):
    """Zero everywhere (mean_function.py:65-87)."""

    def __init__(self, obs_dim: int) -> None:
        self._obs_dim = int(obs_dim)

    @property
    def output_dim(self) -> int:
        return self._obs_dim

    def __call__(self, time_points: torch.Tensor) -> torch.Tensor:
        return torch.zeros(tuple(time_points.shape) + (self._obs_dim,), dtype=time_points.dtype, device=time_points.device)


class LinearMeanFunction(MeanFunction):
    """``μ(t) = coefficient · t`` in every output (mean_function.py:90-114).  ``coefficient``: a float or a tensor, which may
    require a gradient."""

    def __init__(self, coefficient: Union[float, torch.Tensor], obs_dim: int = 1) -> None:
        self._coefficient = coefficient
        self._obs_dim = int(obs_dim)

    @property
    def coefficient(self):
        return self._coefficient

    @property
    def output_dim(self) -> int:
        return self._obs_dim

    def __call__(self, time_points: torch.Tensor) -> torch.Tensor:
        coef = self._coefficient
        if isinstance(coef, torch.Tensor):
            coef = coef.to(dtype=time_points.dtype, device=time_points.device)
        return (coef * time_points[..., None]).expand(tuple(time_points.shape) + (self._obs_dim,))


def _generalised(comps) -> bool:
    """True when every component is one the HIP generator builds: order in {0, 1, 3, 5}, ``_osc`` in {0, 1, 2}."""
    return all(not isinstance(c, LatentExponentiallyGenerated) and getattr(c, "order", None) in (0, 1, 3, 5)
               and getattr(c, "_osc", None) in (0, 1, 2) for c in comps)


def _output_map(kernel: SDEKernel):
    """The output that every component's first state is added to - the emission matrix as the 0/1 selector it is for the supported
    kernels (``Sum``: every component into its child's outputs; ``IndependentMultiOutput``: child ``i`` into output ``i``) - or
    ``None`` for a kernel whose emission matrix is not of that form."""
    if isinstance(kernel, IndependentMultiOutput):
        out, base = [], 0
        for k in kernel.kernels:
            sub = _output_map(k)
            if sub is None:
                return None
            out += [base + o for o in sub]
            base += k.output_dim
        return out
    if isinstance(kernel, Sum):
        out = []
        for k in kernel.kernels:
            sub = _output_map(k)
            if sub is None:
                return None
            out += sub
        return out
    if isinstance(kernel, (_MaternBase, Constant, Product)) and kernel.output_dim == 1:
        return [0]
    return None


class _MeanResponse(torch.autograd.Function):
    """``f [B, N, m]`` of ``mf_mean_response_*`` as a function of ``r`` and ``a`` (``[B, K, d]``; ``a`` may be ``None``), differentiable
    once: the map is linear, its backward is ``mf_mean_response_grad_*`` (deterministic, no atomics)."""

    @staticmethod
    def forward(ctx, r, a, tau, tp, lam_t, om_t, orders, oscs, out_map, m, per_series):
        bsz, k, d = r.shape
        n = tp.shape[-1]
        dtype, dev = r.dtype, r.device
        f = torch.empty((bsz, n, m), dtype=dtype, device=dev)
        coef = torch.empty((bsz, k, d), dtype=dtype, device=dev)
        nc = len(orders)
        ints = lambda xs: (ctypes.c_int * nc)(*xs)                               # noqa: E731
        _launch("mf_mean_response", dtype, dev, bsz, k, n, nc, ints(orders), ints(oscs), lam_t, om_t, int(per_series), tau,
                r.detach(), None if a is None else a.detach(), tp, m, ints(out_map), f, None, coef)
        ctx.save_for_backward(tau, tp, lam_t, om_t)
        ctx.meta = (orders, oscs, out_map, m, per_series, k, d, a is not None)
        return f

    @staticmethod
    def backward(ctx, g_f):
        _differentiable_once("_MeanResponse", "action bins and transitions")
        tau, tp, lam_t, om_t = ctx.saved_tensors
        orders, oscs, out_map, m, per_series, k, d, has_a = ctx.meta
        bsz, n = tp.shape
        dtype, dev = tp.dtype, tp.device
        nc = len(orders)
        ints = lambda xs: (ctypes.c_int * nc)(*xs)                               # noqa: E731
        g_r = torch.empty((bsz, k, d), dtype=dtype, device=dev)
        g_a = torch.empty_like(g_r) if has_a and ctx.needs_input_grad[1] else None
        ws, ws_bytes = _workspace(_lib.load().mf_mean_response_grad_workspace_bytes, dev, bsz, n, nc, d, tp.element_size())
        _launch("mf_mean_response_grad", dtype, dev, bsz, k, n, nc, ints(orders), ints(oscs), lam_t, om_t, int(per_series), tau, tp, m,
                ints(out_map), g_f, g_r, g_a, ws, ws_bytes)
        return (g_r, g_a) + (None,) * 9


class _ResponseMeanFunction(MeanFunction):
    """What ``ImpulseMeanFunction`` and ``StepMeanFunction`` share: the checks, the choice of the route and the two routes."""

    def __init__(self, action_times: torch.Tensor, state_perturbations: torch.Tensor, kernel: SDEKernel) -> None:
        who = type(self).__name__
        if not isinstance(kernel, SDEKernel):
            raise TypeError(f"{who}: kernel must be a markovflow_amd.kernels.SDEKernel")
        if isinstance(kernel, NonStationaryKernel):
            raise NotImplementedError(f"{who} supports stationary kernels only: a non-stationary kernel ({type(kernel).__name__}) "
                                      "has no single feedback matrix to propagate the actions with")
        if isinstance(kernel, SparseSpatioTemporalKernel):
            raise NotImplementedError(f"{who} does not support a SparseSpatioTemporalKernel")
        _refuse_stack(kernel, who)
        if not (isinstance(action_times, torch.Tensor) and isinstance(state_perturbations, torch.Tensor)):
            raise TypeError(f"{who}: action_times and state_perturbations must be tensors")
        if state_perturbations.dim() < 2 or tuple(action_times.shape) != tuple(state_perturbations.shape[:-1]):
            raise ValueError(f"{who}: action_times has shape {tuple(action_times.shape)}, expected state_perturbations.shape[:-1] = "
                             f"{tuple(state_perturbations.shape[:-1])}")
        if state_perturbations.shape[-1] != kernel.state_dim:
            raise ValueError(f"{who}: state_perturbations has last dimension {state_perturbations.shape[-1]}, expected the kernel's "
                             f"state dimension {kernel.state_dim}")
        if action_times.shape[-1] == 0:
            raise ValueError(f"{who}: there must be at least one action (num_actions = 0)")
        # (the kernel's hyper-parameters may have another dtype, as everywhere in the package: both routes cast them to the data's)
        _lib.same_dtype_device(state_perturbations, who, action_times=action_times)
        self._action_times = action_times
        self._state_perturbations = state_perturbations
        self._kernel = kernel

    @property
    def action_times(self) -> torch.Tensor:
        return self._action_times

    @property
    def state_perturbations(self) -> torch.Tensor:
        return self._state_perturbations

    @property
    def kernel(self) -> SDEKernel:
        return self._kernel

    @property
    def output_dim(self) -> int:
        return self._kernel.output_dim

    @abc.abstractmethod
    def _sources(self):
        """``(r, a)`` of the recurrence (``batch + [K, d]``; ``a`` may be ``None``), differentiable in ``state_perturbations``.
        Formed at every call: an in-place update of ``state_perturbations`` is seen by the next one."""

    def _use_fused(self, time_points: torch.Tensor) -> bool:
        kern, u, tau = self._kernel, self._state_perturbations, self._action_times
        if not fused or not (u.is_cuda and time_points.is_cuda) or time_points.numel() == 0:
            return False
        comps = kern._components()
        if not _generalised(comps) or len(comps) > 16 or _output_map(kern) is None or kern._needs_grad():
            return False
        return not (torch.is_grad_enabled() and (time_points.requires_grad or tau.requires_grad))

    def __call__(self, time_points: torch.Tensor) -> torch.Tensor:
        who = type(self).__name__
        u, tau = self._state_perturbations, self._action_times
        batch = tuple(tau.shape[:-1])
        if time_points.dim() < 1 or tuple(time_points.shape[:-1]) != batch:
            raise ValueError(f"{who}: time_points has shape {tuple(time_points.shape)}, expected the actions' batch shape {batch} + "
                             "[num_data]")
        _lib.same_dtype_device(u, who, time_points=time_points)
        r, a = self._sources()
        if self._use_fused(time_points):
            return self._fused_response(r, a, time_points)
        return self._torch_response(r, a, time_points)

    def _fused_response(self, r, a, time_points):
        kern, tau = self._kernel, self._action_times
        comps = kern._components()
        batch = tuple(tau.shape[:-1])
        k, n, d, m = tau.shape[-1], time_points.shape[-1], kern.state_dim, kern.output_dim
        dtype, dev = r.dtype, r.device
        zero = torch.zeros((), dtype=dtype, device=dev)
        hyper = [[c._lambda.to(dtype=dtype, device=dev) for c in comps],
                 [zero if c._omega is None else c._omega.to(dtype=dtype, device=dev) for c in comps]]
        per_series = any(x.dim() > 0 for group in hyper for x in group)
        if per_series:
            lam_t, om_t = (torch.stack([x.expand(batch).reshape(-1) for x in group], dim=-1).contiguous() for group in hyper)
        else:
            lam_t, om_t = (torch.stack(group).contiguous() for group in hyper)
        flat = lambda x, tail: None if x is None else x.reshape((-1,) + tail)         # noqa: E731
        f = _MeanResponse.apply(flat(r, (k, d)), flat(a, (k, d)), flat(tau.detach(), (k,)).contiguous(),
                                flat(time_points.detach(), (n,)).contiguous(), lam_t.detach(), om_t.detach(),
                                tuple(c.order for c in comps), tuple(c._osc for c in comps), tuple(_output_map(kern)), m,
                                bool(per_series))
        return f.reshape(batch + (n, m))

    def _torch_response(self, r, a, time_points):
        """The recurrence and the evaluation in differentiable torch operations (a Python loop over the ``K`` actions)."""
        kern, tau = self._kernel, self._action_times
        k, d = tau.shape[-1], kern.state_dim
        if time_points.is_cuda:
            transitions = kern.state_transitions
        else:       # (the public method would hand CPU pointers to the HIP library)
            transitions = lambda start, gaps: kern._torch_transitions(gaps, False, False)[0]      # noqa: E731
        coef = [r[..., 0, :]]
        if k > 1:
            a_s = transitions(tau[..., :-1], to_delta_time(tau))
            for i in range(1, k):
                coef.append((a_s[..., i - 1, :, :] @ coef[-1][..., None])[..., 0] + r[..., i, :])
        coef = torch.stack(coef, dim=-2)
        j = torch.searchsorted(tau.detach().contiguous(), time_points.detach().contiguous())          # #{k : tau_k < t}
        seen = j > 0
        idx = (j - 1).clamp(min=0)
        delta = torch.where(seen, time_points - torch.gather(tau, -1, idx), torch.zeros_like(time_points))
        gidx = idx[..., None].expand(tuple(idx.shape) + (d,))
        state = (transitions(time_points, delta) @ torch.gather(coef, -2, gidx)[..., None])[..., 0]
        if a is not None:
            state = state + torch.gather(a, -2, gidx)
        state = torch.where(seen[..., None], state, torch.zeros_like(state))           # (an exact zero, not a product with zero)
        # (a NaN time sorts last and its gap is NaN; an order-0 block [1] would not carry it, the fused route's does)
        state = torch.where(torch.isnan(time_points)[..., None], time_points[..., None], state)
        return kern.generate_emission_model(time_points.detach()).project_state_to_f(state)


class ImpulseMeanFunction(_ResponseMeanFunction):
    """The mean of ``dx/dt = F x + Σ_k u_k δ(t − τ_k) + L w`` (mean_function.py:117-258): every action kicks the state by
    ``u_k``, which then decays through the kernel's dynamics.  The effect of an action is seen only AFTER its time.

    :param action_times: ``batch + [num_actions]``, sorted ascending per series (not checked; ties allowed).
    :param state_perturbations: ``batch + [num_actions, state_dim]``; may require a gradient.
    :param kernel: the stationary kernel whose feedback matrix propagates the actions.

    Before the first action the mean is exactly zero (the reference's ``exp(F · negative gap) · 0`` is NaN far before it)."""

    def _sources(self):
        return self._state_perturbations, None


class StepMeanFunction(_ResponseMeanFunction):
    """The mean of ``dx/dt = F x + u(t) + L w`` with ``u(t) = u_k`` on ``(τ_k, τ_{k+1}]`` and zero up to ``τ_0``
    (mean_function.py:261-413); arguments as for ``ImpulseMeanFunction``.  Far behind an action the state mean tends to ``−F⁻¹ u_k``,
    so ``F`` must be invertible: a kernel with an order-0 component without an oscillator (a ``Constant``, a product of constants)
    is refused."""

    def __init__(self, action_times: torch.Tensor, state_perturbations: torch.Tensor, kernel: SDEKernel) -> None:
        super().__init__(action_times, state_perturbations, kernel)
        if any(getattr(c, "order", None) == 0 and getattr(c, "_osc", None) == 0 for c in kernel._components()):
            raise ValueError("StepMeanFunction: the kernel's feedback matrix is singular (a Constant component, or a product of "
                             "constants only), so the response -F^-1 u to a step does not exist")

    def _sources(self):
        u = self._state_perturbations
        f = self._kernel.feedback_matrix.to(dtype=u.dtype, device=u.device)
        a = -torch.linalg.solve(f, u.transpose(-1, -2)).transpose(-1, -2)             # a_k = -F^-1 u_k: K tiny solves, not hot
        return torch.cat([-a[..., :1, :], a[..., :-1, :] - a[..., 1:, :]], dim=-2), a
