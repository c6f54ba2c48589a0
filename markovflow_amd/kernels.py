"""
SDE kernels -> state space models on the MI355X: the step immediately before the Kalman path.

Mirror of the part of ``markovflow/kernels`` (reference) that generates the BASELINE configurations:
``SDEKernel`` / ``StationaryKernel`` (``kernels/sde_kernel.py:43-497``), ``Matern12`` / ``Matern32`` / ``Matern52``
(``kernels/matern.py``), ``ConcatKernel`` / ``Sum`` / ``IndependentMultiOutput`` (``sde_kernel.py:540-690,826-878``), with
the same method names and shapes.  The transition matrices ``A_k = exp(F Δt_k)`` and the Cholesky factors of
``Q_k = P∞ − A_k P∞ A_kᵀ`` are produced by one HIP kernel (``mf_sde_matern_transitions_*``) directly in the
``[batch, T−1, d, d]`` layout ``StateSpaceModel`` takes.

Periodic and quasi-periodic kernels: ``Constant`` (``kernels/constant.py``), ``HarmonicOscillator`` (``kernels/periodic.py``),
``Product`` (``sde_kernel.py:691-822``) and ``SDEKernel.__mul__`` (``:347-350``).  A product of at most one Matérn factor, at most
one ``HarmonicOscillator`` and any number of ``Constant`` factors is ONE generalised component - an order in {0, 1, 3, 5} (0: the
constant), an optional oscillator ``ω = 2π / period`` and the Kronecker order - whose ``A_k = A_k^M ⊗ R(ωΔt_k)`` (or ``R ⊗ A_k^M``)
and ``chol Q_k`` come from ``mf_sde_transitions_*``; ``Sum`` / ``IndependentMultiOutput`` concatenate such components like Matérn
ones.  Plain Matérn kernels keep the Matérn generator.

Piecewise-stationary kernels: ``NonStationaryKernel`` (``sde_kernel.py:499-537``) and ``PiecewiseKernel``
(``kernels/piecewise_stationary.py``) - ``K`` sorted change points, ``K + 1`` stationary kernels of one signature, the hyper-parameters
of a transition taken from the segment it STARTS in.  ``mf_sde_piecewise_transitions_*`` looks the segment up per lane and generates
``A_k``, ``chol Q_k`` in one launch; ``mf_sde_piecewise_transitions_grad_*`` is its reverse mode, with the sum over the steps of every
(series, segment) on the device in a fixed order.  Supported by ``GaussianProcessRegression`` only; see ``PiecewiseKernel`` for the
crossing rule and the other limitations.

The latent exponentially generated kernel: ``LatentExponentiallyGenerated`` (``kernels/latent_exp_generated.py``) - a dense,
trainable feedback matrix ``F = −½(N Nᵀ + R − Rᵀ)`` with ``P∞ = I``.  ``mf_sde_leg_transitions_*`` computes ``A_k = expm(Δt_k F)`` and
``chol Q_k`` by scaling and squaring on a group of lanes per step; ``mf_sde_leg_transitions_grad_*`` is its reverse mode.

The factor-analysis kernel: ``FactorAnalysisKernel`` (``sde_kernel.py:881-941``) - ``P`` observed processes mixed from ``L`` independent
latent kernels, ``f(t) = A(t) B g(t)``: the chain is ``IndependentMultiOutput``'s, the emission a ``ComposedPairEmissionModel``, and the
loading matrix ``B`` a trainable hyper-parameter of the emission alone (no generator depends on it).

Nothing else of the reference's kernels package (the Stack kernels, products of two Matérns) is mirrored.

Hyper-parameters are plain tensors / floats (the reference wraps them in ``gpflow.Parameter``); a hyper-parameter may also
carry ``batch_shape`` (one value per series), which the reference expresses with ``StackKernel``.
"""
import abc
import ctypes
import math
import weakref
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from .emission_model import ComposedPairEmissionModel, EmissionModel
from .gauss_markov import GaussMarkovDistribution
from .state_space_model import StateSpaceModel

Hyper = Union[float, torch.Tensor]


def to_delta_time(time_points: torch.Tensor) -> torch.Tensor:
    """``Δt_k = t_{k+1} − t_k`` (markovflow/utils.py ``to_delta_time``)."""
    return time_points[..., 1:] - time_points[..., :-1]


def _kron(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Kronecker product of the trailing matrices; leading dims broadcast (markovflow/utils.py ``kronecker_product``)."""
    out = a[..., :, None, :, None] * b[..., None, :, None, :]
    return out.reshape(tuple(out.shape[:-4]) + (out.shape[-4] * out.shape[-3], out.shape[-2] * out.shape[-1]))


def _block_diag(blocks: Sequence[torch.Tensor]) -> torch.Tensor:
    """Block-diagonal of matrices that share their leading dims (markovflow/utils.py ``block_diag``)."""
    lead = torch.broadcast_shapes(*[tuple(b.shape[:-2]) for b in blocks])
    d = sum(b.shape[-1] for b in blocks)
    out = torch.zeros(tuple(lead) + (d, d), dtype=blocks[0].dtype, device=blocks[0].device)
    off = 0
    for b in blocks:
        k = b.shape[-1]
        out[..., off:off + k, off:off + k] = b
        off += k
    return out


_CHOL_INDEX = {}    # (component orders, device) -> flat positions of the non-zero entries of chol(P_inf + jitter)


class SDEKernel(abc.ABC):
    """Kernel defined by a linear SDE ``dx = F x dt + L dβ`` (sde_kernel.py:43-351)."""

    def __init__(self, output_dim: int = 1, jitter: float = 0.0) -> None:
        assert output_dim > 0, "The output dimension must be positive"     # sde_kernel.py:127-129
        assert jitter >= 0.0, "jitter must be a non-negative float number."
        self._output_dim = output_dim
        self._jitter = float(jitter)

    @property
    def output_dim(self) -> int:
        return self._output_dim

    @property
    @abc.abstractmethod
    def state_dim(self) -> int:
        """Dimension of the state."""

    # -- what a concrete kernel provides -----------------------------------------------------------------------------
    @abc.abstractmethod
    def _components(self) -> List["SDEKernel"]:
        """The components whose block-diagonal concatenation is this kernel's state.  A component has an ``order`` in {0, 1, 3, 5}
        (0: constant; otherwise Matérn-order/2), ``_osc`` (0: no oscillator, 1: Matérn ⊗ R, 2: R ⊗ Matérn), the tensors ``_lambda``,
        ``_variance_t`` and ``_omega`` (None without an oscillator) and ``_leaves()``, the hyper-parameter tensors behind them."""

    @abc.abstractmethod
    def initial_mean(self, batch_shape) -> torch.Tensor:
        """``batch_shape + [state_dim]``."""

    @abc.abstractmethod
    def initial_covariance(self, initial_time_point: torch.Tensor) -> torch.Tensor:
        """``batch_shape + [state_dim, state_dim]``."""

    # -- generic machinery ---------------------------------------------------------------------------------------------
    @property
    def jitter_matrix(self) -> torch.Tensor:
        """``jitter · I`` (sde_kernel.py:332-340)."""
        ref = self._components()[0]._variance_t
        return self._jitter * torch.eye(self.state_dim, dtype=ref.dtype, device=ref.device)

    def _needs_grad(self) -> bool:
        return torch.is_grad_enabled() and any(x.requires_grad for c in self._components() for x in c._leaves())

    def _torch_transitions(self, time_deltas: torch.Tensor, want_chol: bool, want_cov: bool):
        """The same closed forms in differentiable torch ops: used only while a hyper-parameter requires a gradient (the
        HIP generator has no backward); the chain rule then runs  hyper-parameters -> (A, chol Q) -> log-likelihood, the
        last link being the Fisher-identity kernel of ``KalmanFilter``."""
        blocks_a, blocks_q = [], []
        dtm = time_deltas[..., None, None]
        comps = self._components()
        for c in comps:
            if not isinstance(c, _MaternBase):
                a, q = _general_transitions(c, time_deltas)
                blocks_a.append(a)
                blocks_q.append(q)
                continue
            lam = c._lambda.to(dtype=time_deltas.dtype, device=time_deltas.device)
            lam_b = lam[..., None, None, None] if lam.dim() > 0 else lam
            k = c.state_dim
            f, pinf = c.feedback_matrix.to(time_deltas), c.steady_state_covariance.to(time_deltas)
            eye = torch.eye(k, dtype=time_deltas.dtype, device=time_deltas.device)
            nil = f + (lam[..., None, None] if lam.dim() > 0 else lam) * eye          # nilpotent: (F + lam I)^k = 0
            nil_b = nil[..., None, :, :] if nil.dim() > 2 else nil
            a = eye + nil_b * dtm
            if k == 3:
                a = a + (nil_b @ nil_b) * (0.5 * dtm ** 2)
            a = a * torch.exp(-lam_b * dtm)
            p_b = pinf[..., None, :, :] if pinf.dim() > 2 else pinf
            q = p_b - a @ p_b @ a.transpose(-1, -2)
            blocks_a.append(a)
            blocks_q.append(0.5 * (q + q.transpose(-1, -2)))
        a_s = _block_diag(blocks_a)
        q_s = _block_diag(blocks_q) + self.jitter_matrix.to(time_deltas)
        if want_chol and any(c.order == 0 for c in comps):
            # an order-0 block is jitter I exactly: its factor is sqrt(jitter) I, zero for a zero jitter (the all-zero pass-through
            # of cholesky_or_zero) - block by block, since a Cholesky of the whole matrix would stop at the zero block
            facs = []
            for c, q in zip(comps, blocks_q):
                eye = torch.eye(c.state_dim, dtype=time_deltas.dtype, device=time_deltas.device)
                facs.append(math.sqrt(self._jitter) * eye if c.order == 0 else torch.linalg.cholesky(q + self._jitter * eye))
            chol = _block_diag([f.expand(tuple(time_deltas.shape) + tuple(f.shape[-2:])) for f in facs])
        else:
            chol = torch.linalg.cholesky(q_s) if want_chol else None
        return a_s, chol, (q_s if want_cov else None)

    def _device_transitions(self, time_deltas: torch.Tensor, want_chol: bool, want_cov: bool, transition_times=None):
        """(A, chol Q, Q) for ``time_deltas`` of shape ``batch_shape + [n]`` through the HIP kernel.  ``transition_times`` (the time
        every transition starts at) only matters to a ``NonStationaryKernel``."""
        comps = self._components()
        batch = tuple(time_deltas.shape[:-1])
        n, d = time_deltas.shape[-1], self.state_dim
        needs_grad = self._needs_grad()
        if needs_grad and (want_cov or not time_deltas.is_cuda or (torch.is_grad_enabled() and time_deltas.requires_grad)
                           or time_deltas.numel() == 0):
            # Q itself, or a gradient with respect to the time points, is asked for: differentiable torch ops
            return self._torch_transitions(time_deltas, want_chol, want_cov)
        dt = time_deltas.reshape(-1, n).contiguous()
        bsz = dt.shape[0]
        if not all(c._osc == 0 and c.order != 0 for c in comps):
            return self._general_device_transitions(comps, dt, batch, needs_grad, want_chol, want_cov)
        lam = [c._lambda.to(dtype=dt.dtype, device=dt.device) for c in comps]
        var = [c._variance_t.to(dtype=dt.dtype, device=dt.device) for c in comps]
        per_series = any(x.dim() > 0 for x in lam + var)
        if per_series:
            lam_t = torch.stack([x.expand(batch).reshape(-1) for x in lam], dim=-1).contiguous()
            var_t = torch.stack([x.expand(batch).reshape(-1) for x in var], dim=-1).contiguous()
        else:
            lam_t, var_t = torch.stack(lam).contiguous(), torch.stack(var).contiguous()
        if needs_grad:
            # hyper-parameters under a gradient (the GPR training step): HIP generator forward AND backward
            # (_MaternTransitions); lam_t / var_t were assembled from the leaves by differentiable torch ops above
            a_s, chol = _MaternTransitions.apply(dt, lam_t, var_t, tuple(c.order for c in comps), bool(per_series), float(self._jitter),
                                                 bool(want_chol))
            shape = batch + (n, d, d)
            return a_s.reshape(shape), (chol.reshape(shape) if want_chol else None), None
        orders = (ctypes.c_int * len(comps))(*[c.order for c in comps])
        a_s = torch.empty((bsz, n, d, d), dtype=dt.dtype, device=dt.device)
        chol = torch.empty_like(a_s) if want_chol else None
        cov = torch.empty_like(a_s) if want_cov else None
        _lib.call("mf_sde_matern_transitions", dt.dtype, bsz, n, len(comps), orders, _lib.ptr(lam_t), _lib.ptr(var_t),
                  int(per_series), _lib.ptr(dt), self._jitter, _lib.ptr(a_s), _lib.ptr(chol), _lib.ptr(cov),
                  _lib.stream_ptr(dt.device))
        shape = batch + (n, d, d)
        return (a_s.reshape(shape), None if chol is None else chol.reshape(shape),
                None if cov is None else cov.reshape(shape))

    def _general_device_transitions(self, comps, dt, batch, needs_grad, want_chol, want_cov):
        """``_device_transitions`` when a component is of order 0 or has an oscillator: ``mf_sde_transitions_*``, and under a
        gradient ``_SdeTransitions`` (its backward is ``mf_sde_transitions_grad_*``)."""
        bsz, n = dt.shape
        d = self.state_dim
        zero = torch.zeros((), dtype=dt.dtype, device=dt.device)
        hyper = [[c._lambda.to(dtype=dt.dtype, device=dt.device) for c in comps],
                 [c._variance_t.to(dtype=dt.dtype, device=dt.device) for c in comps],
                 [zero if c._omega is None else c._omega.to(dtype=dt.dtype, device=dt.device) for c in comps]]
        per_series = any(x.dim() > 0 for group in hyper for x in group)
        if per_series:
            lam_t, var_t, om_t = (torch.stack([x.expand(batch).reshape(-1) for x in group], dim=-1).contiguous() for group in hyper)
        else:
            lam_t, var_t, om_t = (torch.stack(group).contiguous() for group in hyper)
        orders, oscs = tuple(c.order for c in comps), tuple(c._osc for c in comps)
        shape = batch + (n, d, d)
        if needs_grad:
            a_s, chol = _SdeTransitions.apply(dt, lam_t, var_t, om_t, orders, oscs, bool(per_series), float(self._jitter),
                                              bool(want_chol))
            return a_s.reshape(shape), (chol.reshape(shape) if want_chol else None), None
        a_s = torch.empty((bsz, n, d, d), dtype=dt.dtype, device=dt.device)
        chol = torch.empty_like(a_s) if want_chol else None
        cov = torch.empty_like(a_s) if want_cov else None
        _lib.call("mf_sde_transitions", dt.dtype, bsz, n, len(comps), (ctypes.c_int * len(comps))(*orders),
                  (ctypes.c_int * len(comps))(*oscs), _lib.ptr(lam_t), _lib.ptr(var_t), _lib.ptr(om_t), int(per_series), _lib.ptr(dt),
                  self._jitter, _lib.ptr(a_s), _lib.ptr(chol), _lib.ptr(cov), _lib.stream_ptr(dt.device))
        return (a_s.reshape(shape), None if chol is None else chol.reshape(shape), None if cov is None else cov.reshape(shape))

    def state_transitions(self, transition_times: torch.Tensor, time_deltas: torch.Tensor) -> torch.Tensor:
        """``A_k = exp(F Δt_k)``, ``batch_shape + [num_transitions, state_dim, state_dim]`` (sde_kernel.py:299-310)."""
        return self._device_transitions(time_deltas, False, False, transition_times)[0]

    def process_covariances(self, transition_times: torch.Tensor, time_deltas: torch.Tensor) -> torch.Tensor:
        """``Q_k`` (sde_kernel.py:312-330)."""
        return self._device_transitions(time_deltas, False, True, transition_times)[2]

    def transition_statistics(self, transition_times: torch.Tensor, time_deltas: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(A_k, Q_k)`` with ``Q_k = P∞ − A_k P∞ A_kᵀ + jitter`` (sde_kernel.py:421-446)."""
        a_s, _, q_s = self._device_transitions(time_deltas, False, True, transition_times)
        return a_s, q_s

    def _lookup_times(self, times: torch.Tensor, conditioning_time_points: torch.Tensor) -> torch.Tensor:
        """The times at which the dynamics that hold AT ``times`` are looked up, for a process conditioned at
        ``conditioning_time_points`` (prediction, sampling): what is passed on as ``transition_times`` and to ``initial_covariance``.
        A stationary kernel ignores them; a ``NonStationaryKernel`` says here which dynamics hold before the first conditioning point
        (``times`` may hold ``-APPROX_INF``, the neighbour of a new point before it)."""
        return times

    def transition_statistics_from_time_points(self, time_points: torch.Tensor):
        """sde_kernel.py:253-265."""
        return self.transition_statistics(time_points[..., :-1], to_delta_time(time_points))

    def state_offsets(self, transition_times: torch.Tensor, time_deltas: torch.Tensor) -> torch.Tensor:
        """``b_k = (I − A_k) m`` for a state mean ``m`` (sde_kernel.py:460-475); zero for a zero mean."""
        mean = self.initial_mean(tuple(time_deltas.shape[:-1]))
        if not bool(torch.any(mean != 0)):
            return torch.zeros(tuple(time_deltas.shape) + (self.state_dim,), dtype=time_deltas.dtype, device=time_deltas.device)
        a_s = self.state_transitions(transition_times, time_deltas)
        m = mean[..., None, :].to(dtype=a_s.dtype, device=a_s.device)
        return m - torch.matmul(a_s, m[..., None])[..., 0]

    def state_space_model(self, time_points: torch.Tensor, lookup_times: Optional[torch.Tensor] = None) -> StateSpaceModel:
        """The chain this kernel induces on ``time_points`` (``batch_shape + [num_data]``, strictly increasing)
        (sde_kernel.py:153-171).  The Cholesky factors come straight from the device kernel (zero covariances pass
        through as zero, as in ``state_space_model_from_covariances``).  ``lookup_times`` (default: the time points themselves;
        see ``_lookup_times``) only matters to a ``NonStationaryKernel``: the time at which the dynamics of every point are looked up."""
        batch = tuple(time_points.shape[:-1])
        deltas = to_delta_time(time_points)
        lookup = time_points if lookup_times is None else lookup_times
        a_s, chol_q, _ = self._device_transitions(deltas, True, False, lookup[..., :-1])
        chol_p0 = self._initial_cholesky(batch, a_s.dtype, a_s.device)
        if chol_p0 is None:
            p0 = self.initial_covariance(lookup[..., 0:1]).to(dtype=a_s.dtype, device=a_s.device)
            p0 = p0.expand(batch + tuple(p0.shape[-2:])).contiguous()
            # (P-infinity + jitter is positive definite by construction: no info check, hence no host synchronisation)
            chol_p0 = _lib.checked_cholesky(p0, "SDEKernel.state_space_model (initial covariance)")
        return StateSpaceModel(
            initial_mean=self.initial_mean(batch).to(dtype=a_s.dtype, device=a_s.device).expand(batch + (self.state_dim,)).contiguous(),
            chol_initial_covariance=chol_p0,
            state_transitions=a_s,
            state_offsets=self.state_offsets(lookup[..., :-1], deltas).to(dtype=a_s.dtype),
            chol_process_covariances=chol_q,
        )

    def _initial_cholesky(self, batch, dtype, device):
        """``chol(P_inf + jitter I)`` of a concatenation of Matern components in closed form, ``batch + [d, d]`` - or None (the generic
        route: assemble P_inf, batched Cholesky).  The steady-state covariance of every Matern component is a 1 x 1, a diagonal 2 x 2 or
        an arrow-shaped 3 x 3 block (matern.py:27-518) whose factor is a handful of elementwise operations on the stacked
        hyper-parameters; assembling P_inf block by block by slice assignment and differentiating a batched Cholesky through torch
        is ~150 small launches of the ~320 of a training step at config 4's model (profiles/r05_config4_torch_ops.txt)."""
        comps = self._components()
        if not comps or not all(isinstance(c, _MaternBase) and c.order in (1, 3, 5) for c in comps):
            return None
        d, jit = self.state_dim, self._jitter
        rows, cols, vals = [], [], []
        offs, o = [], 0
        for c in comps:
            offs.append(o)
            o += c.state_dim
        for order in sorted({c.order for c in comps}):
            grp = [i for i, c in enumerate(comps) if c.order == order]
            lam = torch.stack([comps[i]._lambda.to(dtype=dtype, device=device).expand(batch) for i in grp], dim=-1)
            var = torch.stack([comps[i]._variance_t.to(dtype=dtype, device=device).expand(batch) for i in grp], dim=-1)
            base = [offs[i] for i in grp]
            l00 = torch.sqrt(var + jit)

            def put(dr, dc, v):
                rows.extend(b + dr for b in base)
                cols.extend(b + dc for b in base)
                vals.append(v)

            put(0, 0, l00)
            if order == 3:
                put(1, 1, torch.sqrt(var * lam ** 2 + jit))
            elif order == 5:
                kap = lam ** 2 / 3.0
                l20 = -(kap * var) / l00
                put(2, 0, l20)
                put(1, 1, torch.sqrt(kap * var + jit))
                put(2, 2, torch.sqrt(lam ** 4 * var + jit - l20 ** 2))
        flat = torch.zeros(tuple(batch) + (d * d,), dtype=dtype, device=device)
        key = (tuple(c.order for c in comps), str(device))
        index = _CHOL_INDEX.get(key)
        if index is None:       # (one small upload per kernel signature and device, not per model build)
            index = _CHOL_INDEX[key] = torch.tensor([r * d + c for r, c in zip(rows, cols)], dtype=torch.long, device=device)
        flat = flat.index_copy(-1, index, torch.cat(vals, dim=-1))
        return flat.reshape(tuple(batch) + (d, d))

    def build_finite_distribution(self, time_points: torch.Tensor) -> GaussMarkovDistribution:
        """sde_kernel.py:140-151."""
        return self.state_space_model(time_points)

    def generate_emission_model(self, time_points: torch.Tensor) -> EmissionModel:
        """``H = [1, 0, 0, …]`` tiled over the time points (sde_kernel.py:173-211)."""
        h = torch.zeros((self.output_dim, self.state_dim), dtype=time_points.dtype, device=time_points.device)
        h[:, 0] = 1.0
        return EmissionModel(h.expand(tuple(time_points.shape) + h.shape).contiguous())

    def __add__(self, other: "SDEKernel") -> "Sum":
        assert self.output_dim == other.output_dim                         # sde_kernel.py:342-345
        return Sum([self, other])

    def __mul__(self, other: "SDEKernel") -> "Product":
        assert self.output_dim == other.output_dim                         # sde_kernel.py:347-350
        return Product([self, other])


class _MaternTransitions(torch.autograd.Function):
    """``(A [B,n,d,d], chol Q [B,n,d,d])`` of a concatenation of Matern components as a differentiable function of the stacked
    hyper-parameters ``lam [B,ncomp] | [ncomp]`` (= sqrt(order) / lengthscale) and ``var`` - forward: the HIP generator
    (``mf_sde_matern_transitions_*``); backward: the same closed forms in forward mode inside one kernel per (series, transition)
    (``mf_sde_matern_transitions_grad_*``), summed over the transitions here.  The reference differentiates matern.py /
    sde_kernel.py:421-446 and a batched Cholesky through TensorFlow; the torch restatement of that (``_torch_transitions``) cost
    350 of the 373 ms of a GPR training step at B=1024, T=10000, d=6."""

    @staticmethod
    def forward(ctx, dt, lam_t, var_t, orders, per_series, jitter, want_chol):
        bsz, n = dt.shape
        d = sum((o + 1) // 2 for o in orders)
        c_orders = (ctypes.c_int * len(orders))(*orders)
        a_s = torch.empty((bsz, n, d, d), dtype=dt.dtype, device=dt.device)
        chol = torch.empty_like(a_s) if want_chol else None
        lam_c, var_c = lam_t.detach().contiguous(), var_t.detach().contiguous()
        _lib.call("mf_sde_matern_transitions", dt.dtype, bsz, n, len(orders), c_orders, _lib.ptr(lam_c), _lib.ptr(var_c),
                  int(per_series), _lib.ptr(dt.detach()), jitter, _lib.ptr(a_s), _lib.ptr(chol), None, _lib.stream_ptr(dt.device))
        ctx.save_for_backward(dt.detach(), lam_c, var_c)
        ctx.meta = (orders, per_series, jitter)
        if not want_chol:
            chol = a_s.new_zeros(())
            ctx.mark_non_differentiable(chol)
        return a_s, chol

    @staticmethod
    def backward(ctx, g_a, g_chol):
        dt, lam_c, var_c = ctx.saved_tensors
        orders, per_series, jitter = ctx.meta
        bsz, n = dt.shape
        c_orders = (ctypes.c_int * len(orders))(*orders)
        part = torch.empty((bsz, n, len(orders), 2), dtype=dt.dtype, device=dt.device)
        with torch.no_grad():
            ga = None if g_a is None else g_a.contiguous()
            gc = None if (g_chol is None or g_chol.dim() == 0) else g_chol.contiguous()
            _lib.call("mf_sde_matern_transitions_grad", dt.dtype, bsz, n, len(orders), c_orders, _lib.ptr(lam_c), _lib.ptr(var_c),
                      int(per_series), _lib.ptr(dt), jitter, _lib.ptr(ga), _lib.ptr(gc), _lib.ptr(part), _lib.stream_ptr(dt.device))
            g = torch.sum(part, dim=1)                                   # [B, ncomp, 2]
            if not per_series:
                g = torch.sum(g, dim=0)                                  # shared hyper-parameters: [ncomp, 2]
        return None, g[..., 0].contiguous(), g[..., 1].contiguous(), None, None, None, None


class _SdeTransitions(torch.autograd.Function):
    """``_MaternTransitions`` for generalised components: ``(A, chol Q)`` as a differentiable function of the stacked ``lam``, ``var``
    and ``omega`` (= 2π / period) - forward ``mf_sde_transitions_*``, backward ``mf_sde_transitions_grad_*`` (the same closed forms
    with three tangents), summed over the transitions here."""

    @staticmethod
    def forward(ctx, dt, lam_t, var_t, om_t, orders, oscs, per_series, jitter, want_chol):
        bsz, n = dt.shape
        d = sum((1 if o == 0 else (o + 1) // 2) * (2 if r else 1) for o, r in zip(orders, oscs))
        a_s = torch.empty((bsz, n, d, d), dtype=dt.dtype, device=dt.device)
        chol = torch.empty_like(a_s) if want_chol else None
        lam_c, var_c, om_c = lam_t.detach().contiguous(), var_t.detach().contiguous(), om_t.detach().contiguous()
        _lib.call("mf_sde_transitions", dt.dtype, bsz, n, len(orders), (ctypes.c_int * len(orders))(*orders),
                  (ctypes.c_int * len(orders))(*oscs), _lib.ptr(lam_c), _lib.ptr(var_c), _lib.ptr(om_c), int(per_series),
                  _lib.ptr(dt.detach()), jitter, _lib.ptr(a_s), _lib.ptr(chol), None, _lib.stream_ptr(dt.device))
        ctx.save_for_backward(dt.detach(), lam_c, var_c, om_c)
        ctx.meta = (orders, oscs, per_series, jitter)
        if not want_chol:
            chol = a_s.new_zeros(())
            ctx.mark_non_differentiable(chol)
        return a_s, chol

    @staticmethod
    def backward(ctx, g_a, g_chol):
        dt, lam_c, var_c, om_c = ctx.saved_tensors
        orders, oscs, per_series, jitter = ctx.meta
        bsz, n = dt.shape
        part = torch.empty((bsz, n, len(orders), 3), dtype=dt.dtype, device=dt.device)
        with torch.no_grad():
            ga = None if g_a is None else g_a.contiguous()
            gc = None if (g_chol is None or g_chol.dim() == 0) else g_chol.contiguous()
            _lib.call("mf_sde_transitions_grad", dt.dtype, bsz, n, len(orders), (ctypes.c_int * len(orders))(*orders),
                      (ctypes.c_int * len(orders))(*oscs), _lib.ptr(lam_c), _lib.ptr(var_c), _lib.ptr(om_c), int(per_series),
                      _lib.ptr(dt), jitter, _lib.ptr(ga), _lib.ptr(gc), _lib.ptr(part), _lib.stream_ptr(dt.device))
            g = torch.sum(part, dim=1)                                   # [B, ncomp, 3]
            if not per_series:
                g = torch.sum(g, dim=0)                                  # shared hyper-parameters: [ncomp, 3]
        return None, g[..., 0].contiguous(), g[..., 1].contiguous(), g[..., 2].contiguous(), None, None, None, None, None


def _general_transitions(c: "SDEKernel", time_deltas: torch.Tensor):
    """``(A, Q − jitter)`` of ONE generalised component in differentiable torch ops - the closed forms of ``mf_sde_transitions_*``
    (csrc/mf_sde.hip): the Matérn factor ``e^{−λΔt}(I + NΔt + N²Δt²/2)`` (order 0: ``[1]``), Kronecker-multiplied with the rotation
    ``R(ωΔt)`` when there is an oscillator; ``Q = P∞ − A P∞ Aᵀ``, symmetrised - and exactly zero for order 0."""
    x = time_deltas
    one, zero = torch.ones_like(x), torch.zeros_like(x)

    def hyper(h):                                       # [] or batch_shape -> broadcastable against batch_shape + [n]
        h = h.to(dtype=x.dtype, device=x.device)
        return h[..., None] if h.dim() > 0 else h

    def mat(rows):
        return torch.stack([torch.stack([e * one for e in row], dim=-1) for row in rows], dim=-2)

    lam, var = hyper(c._lambda), hyper(c._variance_t)
    if c.order == 0:
        a, p = mat([[one]]), mat([[var]])
    else:
        e = torch.exp(-lam * x)[..., None, None]
        l2 = lam * lam
        if c.order == 1:
            nil, p = mat([[zero]]), mat([[var]])
        elif c.order == 3:
            nil = mat([[lam, one], [-l2, -lam]])
            p = mat([[var, zero], [zero, var * l2]])
        else:
            nil = mat([[lam, one, zero], [zero, lam, one], [-l2 * lam, -3.0 * l2, -2.0 * lam]])
            l23 = l2 / 3.0
            p = mat([[var, zero, -var * l23], [zero, var * l23, zero], [-var * l23, zero, var * l2 * l2]])
        xm = x[..., None, None]
        a = torch.eye(nil.shape[-1], dtype=x.dtype, device=x.device) + nil * xm
        if c.order == 5:
            a = a + (nil @ nil) * (0.5 * xm ** 2)
        a = a * e
    if c._osc:
        th = hyper(c._omega) * x
        cos, sin = torch.cos(th), torch.sin(th)
        rot = mat([[cos, -sin], [sin, cos]])
        eye2 = torch.eye(2, dtype=x.dtype, device=x.device)
        a, p = (_kron(a, rot), _kron(p, eye2)) if c._osc == 1 else (_kron(rot, a), _kron(eye2, p))
    if c.order == 0:
        return a, torch.zeros_like(a)
    q = p - a @ p @ a.transpose(-1, -2)
    return a, 0.5 * (q + q.transpose(-1, -2))


class StationaryKernel(SDEKernel, abc.ABC):
    """Stationary SDE kernel: constant feedback matrix ``F`` and steady state covariance ``P∞`` (sde_kernel.py:353-497)."""

    @property
    @abc.abstractmethod
    def feedback_matrix(self) -> torch.Tensor:
        """``F``, ``[state_dim, state_dim]`` (leading batch dims if a hyper-parameter has them)."""

    @property
    @abc.abstractmethod
    def steady_state_covariance(self) -> torch.Tensor:
        """``P∞``."""

    def initial_mean(self, batch_shape) -> torch.Tensor:
        ref = self._components()[0]._variance_t
        return torch.zeros(tuple(batch_shape) + (self.state_dim,), dtype=ref.dtype, device=ref.device)

    def state_offsets(self, transition_times: torch.Tensor, time_deltas: torch.Tensor) -> torch.Tensor:
        """Zero: a stationary kernel's state has zero mean (sde_kernel.py:460-475 evaluates ``(I - A_k) 0``) - known without
        looking at the device, where the generic form has to test the mean (a host synchronisation per model build)."""
        return torch.zeros(tuple(time_deltas.shape) + (self.state_dim,), dtype=time_deltas.dtype, device=time_deltas.device)

    def initial_covariance(self, initial_time_point: torch.Tensor) -> torch.Tensor:
        """``P∞ + jitter`` (sde_kernel.py:402-419)."""
        assert initial_time_point.shape[-1] == 1
        p = self.steady_state_covariance
        batch = tuple(initial_time_point.shape[:-1])
        return p.expand(torch.broadcast_shapes(batch + p.shape[-2:], p.shape)) + self.jitter_matrix


class NonStationaryKernel(SDEKernel, abc.ABC):
    """SDE kernel ``dx = F(t) x dt + L(t) dβ`` whose feedback matrix and steady-state covariance depend on time
    (sde_kernel.py:499-537).  ``transition_times`` - ignored by a stationary kernel - decides what a transition is made of."""

    @abc.abstractmethod
    def feedback_matrices(self, time_points: torch.Tensor) -> torch.Tensor:
        """``F(t)``, ``batch_shape + [num_time_points, state_dim, state_dim]``."""

    @abc.abstractmethod
    def steady_state_covariances(self, time_points: torch.Tensor) -> torch.Tensor:
        """``P∞(t)``, ``batch_shape + [num_time_points, state_dim, state_dim]``."""

    @abc.abstractmethod
    def state_means(self, time_points: torch.Tensor) -> torch.Tensor:
        """``batch_shape + [num_time_points, state_dim]``."""


def _refuse_non_stationary_children(who: str, kernels) -> None:
    if any(isinstance(k, NonStationaryKernel) for k in kernels):
        raise NotImplementedError(f"{who} does not take a non-stationary child kernel (a sum of piecewise kernels is written as a "
                                  "PiecewiseKernel of Sums, with shared change points)")
    if any(isinstance(k, LatentExponentiallyGenerated) for k in kernels):
        raise NotImplementedError(f"{who} does not take a LatentExponentiallyGenerated child kernel: its dense feedback matrix is "
                                  "not a component of the closed-form generators")


# (tensor, version) pairs whose positivity has been read back from the device: the check of matern.py:52-56 is a host
# synchronisation, and a training loop builds the kernel objects anew around the SAME leaf tensors every step (six synchronisations
# per step at config 4's model).  The entry holds a WEAK reference (a cache must not keep hyper-parameter tensors of a million series
# alive): a dead reference, or a live one to another object under a recycled id, is a miss; an in-place update (an optimiser step)
# changes the version and is checked again.
_POSITIVE = {}


def _version_key(t: torch.Tensor):
    """``(data pointer, version counter)``: what the caches below compare.  The pointer catches ``set_()`` / ``.data = `` re-seating
    (invisible to the version counter); inference tensors track no version at all - ``None``: never cached."""
    if t.is_inference():
        return None
    return (t.data_ptr(), t._version)


def _known_positive(*tensors: torch.Tensor) -> bool:
    fresh = []
    for t in tensors:
        key = _version_key(t)
        hit = _POSITIVE.get(id(t)) if key is not None else None
        if hit is None or hit[0]() is not t or hit[1] != key:
            fresh.append(t)
    if not fresh:
        return True
    with torch.no_grad():
        bad = [(t.detach() <= 0).any() for t in fresh]
        if len({t.device for t in fresh}) == 1:
            ok = not bool(torch.stack(bad).any())           # one read-back for all of them
        else:
            ok = not any(bool(b) for b in bad)
    if ok:
        if len(_POSITIVE) > 256:
            _POSITIVE.clear()
        for t in fresh:
            key = _version_key(t)
            if key is not None:
                _POSITIVE[id(t)] = (weakref.ref(t), key)
    return ok


class _MaternBase(StationaryKernel):
    order = 0   # Matérn-order/2
    _osc = 0    # a component without an oscillator
    _omega = None

    def __init__(self, lengthscale: Hyper, variance: Hyper, output_dim: int = 1, jitter: float = 0.0, device=None,
                 dtype=torch.float64) -> None:
        super().__init__(output_dim, jitter)
        dev = device if device is not None else (lengthscale.device if isinstance(lengthscale, torch.Tensor) else "cpu")
        self._lengthscale_t = torch.as_tensor(lengthscale, dtype=dtype, device=dev)
        self._variance_t = torch.as_tensor(variance, dtype=dtype, device=dev)
        if not _known_positive(self._lengthscale_t, self._variance_t):
            raise ValueError("lengthscale and variance must be positive.")   # matern.py:52-56
        self._lambda_cached = None

    @property
    def state_dim(self) -> int:
        return (self.order + 1) // 2

    @property
    def lengthscale(self) -> torch.Tensor:
        return self._lengthscale_t

    @property
    def variance(self) -> torch.Tensor:
        return self._variance_t

    @property
    def _lambda(self) -> torch.Tensor:
        if torch.is_grad_enabled() and self._lengthscale_t.requires_grad:
            return math.sqrt(self.order) / self._lengthscale_t       # a node of its own per use: graphs built from it stay independent
        key = _version_key(self._lengthscale_t)                    # otherwise one division per kernel object, not one per use
        if key is None:                                            # (an inference tensor: no version to key a cache on)
            return math.sqrt(self.order) / self._lengthscale_t
        if self._lambda_cached is None or self._lambda_cached[0] != key:
            self._lambda_cached = (key, math.sqrt(self.order) / self._lengthscale_t.detach())
        return self._lambda_cached[1]

    def invalidate_cache(self) -> None:
        """Forget what was derived from the hyper-parameters (``√order/ℓ``, the positivity check).  The caches are keyed on the
        tensors' data pointer and version counter; a write THROUGH ``.data`` (``x.data.mul_()``) changes neither - call this
        after one (as ``KalmanFilter.invalidate_filter_cache`` / ``GaussianProcessRegression.invalidate_hyperparameter_cache``)."""
        self._lambda_cached = None
        for t in (self._lengthscale_t, self._variance_t):
            _POSITIVE.pop(id(t), None)

    def _components(self):
        return [self]

    def _leaves(self):
        return (self._lengthscale_t, self._variance_t)


class Matern12(_MaternBase):
    """Matérn-1/2 (exponential / Ornstein–Uhlenbeck) kernel (matern.py:27-127): ``F = −1/ℓ``, ``P∞ = σ²``."""
    order = 1

    @property
    def feedback_matrix(self) -> torch.Tensor:
        return (-1.0 / self._lengthscale_t)[..., None, None]

    @property
    def steady_state_covariance(self) -> torch.Tensor:
        return self._variance_t[..., None, None].clone()


class Matern32(_MaternBase):
    """Matérn-3/2 kernel (matern.py:237-373): ``F = [[0, 1], [−λ², −2λ]]``, ``P∞ = σ² diag(1, λ²)``, ``λ = √3/ℓ``."""
    order = 3

    @property
    def feedback_matrix(self) -> torch.Tensor:
        lam = self._lambda
        f = torch.zeros(tuple(lam.shape) + (2, 2), dtype=lam.dtype, device=lam.device)
        f[..., 0, 1] = 1.0
        f[..., 1, 0] = -lam ** 2
        f[..., 1, 1] = -2 * lam
        return f

    @property
    def steady_state_covariance(self) -> torch.Tensor:
        lam, var = self._lambda, self._variance_t
        p = torch.zeros(tuple(torch.broadcast_shapes(lam.shape, var.shape)) + (2, 2), dtype=lam.dtype, device=lam.device)
        p[..., 0, 0] = var
        p[..., 1, 1] = var * lam ** 2
        return p


class Matern52(_MaternBase):
    """Matérn-5/2 kernel (matern.py:376-518): ``F = [[0,1,0],[0,0,1],[−λ³,−3λ²,−3λ]]``, ``λ = √5/ℓ``."""
    order = 5

    @property
    def feedback_matrix(self) -> torch.Tensor:
        lam = self._lambda
        f = torch.zeros(tuple(lam.shape) + (3, 3), dtype=lam.dtype, device=lam.device)
        f[..., 0, 1] = 1.0
        f[..., 1, 2] = 1.0
        f[..., 2, 0] = -lam ** 3
        f[..., 2, 1] = -3 * lam ** 2
        f[..., 2, 2] = -3 * lam
        return f

    @property
    def steady_state_covariance(self) -> torch.Tensor:
        lam, var = self._lambda, self._variance_t
        l23 = lam ** 2 / 3.0
        p = torch.zeros(tuple(torch.broadcast_shapes(lam.shape, var.shape)) + (3, 3), dtype=lam.dtype, device=lam.device)
        p[..., 0, 0] = var
        p[..., 0, 2] = -var * l23
        p[..., 2, 0] = -var * l23
        p[..., 1, 1] = var * l23
        p[..., 2, 2] = var * lam ** 4
        return p


class Constant(StationaryKernel):
    """Constant kernel ``C(x, x') = σ²`` (constant.py:27-153): one state, ``F = [0]``, ``A_k = [1]``, ``P∞ = [σ²]`` - the order-0
    component.  ``Q_k = jitter·I`` exactly: the precision-form Kalman filter therefore needs ``jitter > 0`` on the kernel that
    builds the state space model (the ``Sum`` around it).  With ``jitter = 0`` the zero factor passes through as in the reference
    and the filter reports the non-positive pivot through ``MarkovflowAmdError``."""
    order = 0
    _osc = 0
    _omega = None

    def __init__(self, variance: Hyper, output_dim: int = 1, jitter: float = 0.0, device=None, dtype=torch.float64) -> None:
        super().__init__(output_dim, jitter)
        dev = device if device is not None else (variance.device if isinstance(variance, torch.Tensor) else "cpu")
        self._variance_t = torch.as_tensor(variance, dtype=dtype, device=dev)
        if not _known_positive(self._variance_t):
            raise ValueError("variance must be positive.")                   # constant.py:54-55

    @property
    def state_dim(self) -> int:
        return 1

    @property
    def variance(self) -> torch.Tensor:
        return self._variance_t

    @property
    def _lambda(self) -> torch.Tensor:
        return torch.zeros((), dtype=self._variance_t.dtype, device=self._variance_t.device)

    @property
    def feedback_matrix(self) -> torch.Tensor:
        return torch.zeros((1, 1), dtype=self._variance_t.dtype, device=self._variance_t.device)

    @property
    def steady_state_covariance(self) -> torch.Tensor:
        return self._variance_t[..., None, None].clone()

    def invalidate_cache(self) -> None:
        """Forget the positivity check of the variance (see ``_MaternBase.invalidate_cache``)."""
        for t in self._leaves():
            _POSITIVE.pop(id(t), None)

    def _components(self):
        return [self]

    def _leaves(self):
        return (self._variance_t,)


class HarmonicOscillator(Constant):
    """Periodic kernel ``C(x, x') = σ² cos(2π (x − x') / period)`` (periodic.py:27-203): two states, ``F = [[0, −ω], [ω, 0]]``,
    ``A_k = R(ωΔt_k) = [[cos, −sin], [sin, cos]]``, ``P∞ = σ² I``, ``ω = 2π / period`` - the order-0 component with an oscillator.
    ``Q_k = jitter·I`` exactly (a rotation adds no noise), so what ``Constant`` says about ``jitter`` holds here too."""
    _osc = 1

    def __init__(self, variance: Hyper, period: Hyper, output_dim: int = 1, jitter: float = 0.0, device=None,
                 dtype=torch.float64) -> None:
        dev = device if device is not None else next((x.device for x in (variance, period) if isinstance(x, torch.Tensor)), "cpu")
        super().__init__(variance, output_dim, jitter, device=dev, dtype=dtype)
        self._period_t = torch.as_tensor(period, dtype=dtype, device=dev)
        if not _known_positive(self._period_t):
            raise ValueError("period must be positive.")                     # periodic.py:84-85

    @property
    def state_dim(self) -> int:
        return 2

    @property
    def period(self) -> torch.Tensor:
        return self._period_t

    @property
    def _omega(self) -> torch.Tensor:
        return (2.0 * math.pi) / self._period_t

    @property
    def feedback_matrix(self) -> torch.Tensor:
        om = self._omega
        zero = torch.zeros_like(om)
        return torch.stack([torch.stack([zero, -om], dim=-1), torch.stack([om, zero], dim=-1)], dim=-2)

    @property
    def steady_state_covariance(self) -> torch.Tensor:
        var = self._variance_t
        return var[..., None, None] * torch.eye(2, dtype=var.dtype, device=var.device)

    def _leaves(self):
        return (self._variance_t, self._period_t)


class Product(StationaryKernel):
    """Product of kernels (sde_kernel.py:691-822): ``A_k``, ``P∞`` and the emission matrix are the Kronecker products of the
    children's, in the order of ``kernels`` (``kronecker_product`` of the reference).

    Supported: at most one Matérn factor, at most one ``HarmonicOscillator`` and any number of ``Constant`` factors (which only
    scale the variance) - a decaying oscillation ``Matern * HarmonicOscillator`` with ``σ² k_Matérn(r) cos(ωr)``, state dimension
    2, 4 or 6.  Anything else (Matérn × Matérn, two oscillators, a ``Sum`` or ``Product`` as a child) raises ``NotImplementedError``.
    The whole product is ONE generalised component of the HIP generator ``mf_sde_transitions_*``.  Without a Matérn factor it is of
    order 0 and ``Q_k = jitter·I`` exactly: see ``Constant`` on what that asks of ``jitter``.

    ``feedback_matrix`` is the Kronecker SUM ``F₁ ⊗ I + I ⊗ F₂``, for which ``A_k = exp(F Δt_k)`` holds as ``StationaryKernel``
    documents.  The reference returns the Kronecker PRODUCT of the children's feedback matrices (sde_kernel.py:783-793), for which
    that identity is false; nothing on the path consumes either."""

    def __init__(self, kernels: List[SDEKernel], jitter: float = 0.0):
        self._kernels = list(kernels)
        assert self._kernels, "There must be at least one child kernel."    # sde_kernel.py:745-749
        if not all(isinstance(k, SDEKernel) for k in self._kernels):
            raise TypeError("can only combine Kernel instances")
        assert len({k.output_dim for k in self._kernels}) == 1, "All kernels must have the same output dimension"
        _refuse_non_stationary_children("Product", self._kernels)
        matern = [k for k in self._kernels if isinstance(k, _MaternBase)]
        osc = [k for k in self._kernels if isinstance(k, HarmonicOscillator)]
        rest = [k for k in self._kernels if not isinstance(k, (_MaternBase, Constant))]
        if rest or len(matern) > 1 or len(osc) > 1:
            raise NotImplementedError(
                "Product supports at most one Matern12 / Matern32 / Matern52 factor, at most one HarmonicOscillator and any number "
                "of Constant factors; got " + " * ".join(type(k).__name__ for k in self._kernels))
        self._matern = matern[0] if matern else None
        self._oscillator = osc[0] if osc else None
        self.order = self._matern.order if matern else 0
        if not osc:
            self._osc = 0
        elif not matern or self._matern.state_dim == 1:
            self._osc = 1                                                    # (a 1 x 1 factor: both Kronecker orders coincide)
        else:
            self._osc = 1 if self._kernels.index(self._matern) < self._kernels.index(self._oscillator) else 2
        super().__init__(self._kernels[0].output_dim, jitter)

    @property
    def kernels(self) -> List[SDEKernel]:
        return self._kernels

    @property
    def state_dim(self) -> int:
        return math.prod(k.state_dim for k in self._kernels)

    @property
    def variance(self) -> torch.Tensor:
        """The product of the factors' variances."""
        return self._variance_t

    @property
    def _variance_t(self) -> torch.Tensor:
        out = self._kernels[0]._variance_t
        for k in self._kernels[1:]:
            out = out * k._variance_t
        return out

    @property
    def _lambda(self) -> torch.Tensor:
        if self._matern is not None:
            return self._matern._lambda
        ref = self._kernels[0]._variance_t
        return torch.zeros((), dtype=ref.dtype, device=ref.device)

    @property
    def _omega(self):
        return None if self._oscillator is None else self._oscillator._omega

    @property
    def feedback_matrix(self) -> torch.Tensor:
        out = None
        for k in self._kernels:
            f = k.feedback_matrix
            if out is None:
                out = f
                continue
            eye_l = torch.eye(out.shape[-1], dtype=f.dtype, device=f.device)
            eye_r = torch.eye(f.shape[-1], dtype=f.dtype, device=f.device)
            out = _kron(out, eye_r) + _kron(eye_l, f)
        return out

    @property
    def steady_state_covariance(self) -> torch.Tensor:
        out = None
        for k in self._kernels:
            p = k.steady_state_covariance
            out = p if out is None else _kron(out, p)
        return out

    def generate_emission_model(self, time_points: torch.Tensor) -> EmissionModel:
        """The Kronecker product of the children's emission matrices (sde_kernel.py:808-822); for the supported products that
        is the base class's ``[1, 0, …]``."""
        out = None
        for k in self._kernels:
            h = k.generate_emission_model(time_points).emission_matrix
            out = h if out is None else _kron(out, h)
        return EmissionModel(out.contiguous())

    def invalidate_cache(self) -> None:
        for k in self._kernels:
            k.invalidate_cache()

    def _components(self):
        return [self]

    def _leaves(self):
        return tuple(x for k in self._kernels for x in k._leaves())


class ConcatKernel(StationaryKernel, abc.ABC):
    """State = concatenation of the child states; ``A``, ``F``, ``P∞`` block diagonal (sde_kernel.py:540-658)."""

    def __init__(self, kernels: List[SDEKernel], jitter: float = 0.0):
        assert kernels, "There must be at least one child kernel."           # sde_kernel.py:566-571
        assert all(k.output_dim == kernels[0].output_dim for k in kernels), "All kernels must have the same output dimension"
        _refuse_non_stationary_children(type(self).__name__, kernels)
        self._kernels = list(kernels)
        super().__init__(self._kernels[0].output_dim, jitter)

    @property
    def kernels(self) -> List[SDEKernel]:
        return self._kernels

    @property
    def state_dim(self) -> int:
        return sum(k.state_dim for k in self._kernels)

    def _components(self):
        return [c for k in self._kernels for c in k._components()]

    def initial_mean(self, batch_shape) -> torch.Tensor:
        return torch.cat([k.initial_mean(batch_shape) for k in self._kernels], dim=-1)

    @property
    def feedback_matrix(self) -> torch.Tensor:
        return _block_diag([k.feedback_matrix for k in self._kernels])

    @property
    def steady_state_covariance(self) -> torch.Tensor:
        return _block_diag([k.steady_state_covariance for k in self._kernels])


class Sum(ConcatKernel):
    """Sum of kernels: ``H = [H₁, H₂, …]`` (sde_kernel.py:660-688)."""

    def generate_emission_model(self, time_points: torch.Tensor) -> EmissionModel:
        return EmissionModel(torch.cat([k.generate_emission_model(time_points).emission_matrix for k in self._kernels], dim=-1))


class IndependentMultiOutput(ConcatKernel):
    """Independent outputs, one child kernel each: ``H = H₁ ⊕ H₂ ⊕ …`` (sde_kernel.py:826-878)."""

    def __init__(self, kernels: List[SDEKernel], jitter: float = 0.0):
        super().__init__(kernels, jitter)
        self._output_dim = sum(k.output_dim for k in kernels)                # sde_kernel.py:843-845

    def generate_emission_model(self, time_points: torch.Tensor) -> EmissionModel:
        mats = [k.generate_emission_model(time_points).emission_matrix for k in self._kernels]
        lead = tuple(time_points.shape)
        out = torch.zeros(lead + (self.output_dim, self.state_dim), dtype=mats[0].dtype, device=mats[0].device)
        r = c = 0
        for m in mats:
            out[..., r:r + m.shape[-2], c:c + m.shape[-1]] = m
            r += m.shape[-2]
            c += m.shape[-1]
        return EmissionModel(out)


class FactorAnalysisKernel(ConcatKernel):
    """Observed processes mixed linearly from independent latent GPs (sde_kernel.py:881-941): ``f(t) = A(t) B g(t)`` with ``g`` the
    ``L = len(kernels)`` single-output children (the state is their concatenation, as ``IndependentMultiOutput``'s), ``A(t)`` a known,
    possibly time-dependent ``[output_dim, L]`` weight matrix (``weight_function``) and ``B`` the ``[L, L]`` ``loading_matrix``: the
    identity at construction, trainable unless ``trainable=False``.

    ``loading_matrix`` is a hyper-parameter of the EMISSION, not of the chain: it is not among the leaves of ``_components()``, so
    ``_needs_grad()`` keeps meaning "a hyper-parameter of the chain is under the tape", and ``SparseVariationalGaussianProcess``
    trains it on its fused route.  What caches a quantity that depends on it keys on ``_emission_leaves()`` as well."""

    def __init__(self, weight_function, kernels: List[SDEKernel], output_dim: int, trainable: bool = True, jitter: float = 0.0):
        """
        :param weight_function: time points ``batch + [num_data]`` -> weights ``batch + [num_data, output_dim, L]`` (a tensor of the
            time points' dtype and device).
        :param kernels: the ``L`` latent kernels, ``output_dim == 1`` each.
        :param output_dim: the number of observed processes.
        :param trainable: whether ``loading_matrix`` requires a gradient.
        """
        super().__init__(kernels, jitter)
        if any(k.output_dim != 1 for k in kernels):
            raise ValueError("FactorAnalysisKernel: every child kernel must have output_dim == 1 (one latent process each)")
        if not callable(weight_function):
            raise TypeError("FactorAnalysisKernel: weight_function must be callable")
        assert output_dim > 0, "The output dimension must be positive"
        self._latent_components = IndependentMultiOutput(kernels, jitter)
        self._output_dim = int(output_dim)
        self.latent_dim = self._latent_components.output_dim
        self._weight_function = weight_function
        ref = self._components()[0]._variance_t
        self._loading_matrix = torch.eye(self.latent_dim, dtype=ref.dtype, device=ref.device).requires_grad_(bool(trainable))

    @property
    def loading_matrix(self) -> torch.Tensor:
        """``B [L, L]``, a leaf tensor."""
        return self._loading_matrix

    @property
    def trainable_variables(self) -> Tuple[torch.Tensor, ...]:
        """``(loading_matrix,)`` when it is trainable (the children's hyper-parameters are plain tensors of their own)."""
        return (self._loading_matrix,) if self._loading_matrix.requires_grad else ()

    def _emission_leaves(self) -> Tuple[torch.Tensor, ...]:
        """The hyper-parameters of the emission that are not hyper-parameters of the chain."""
        return (self._loading_matrix,)

    def mixing_weights(self, time_points: torch.Tensor) -> torch.Tensor:
        """``W(t) = A(t) B``, ``time_points.shape + [output_dim, L]``, under the tape of ``loading_matrix`` and of whatever the weight
        function holds."""
        a = self._weight_function(time_points)
        expected = tuple(time_points.shape) + (self._output_dim, self.latent_dim)
        if not isinstance(a, torch.Tensor) or tuple(a.shape) != expected:
            got = tuple(a.shape) if isinstance(a, torch.Tensor) else type(a).__name__
            raise ValueError(f"FactorAnalysisKernel: weight_function returned {got}, expected a tensor of shape {expected} "
                             "(time_points.shape + (output_dim, latent_dim))")
        if a.dtype != time_points.dtype or a.device != time_points.device:
            raise ValueError(f"FactorAnalysisKernel: weight_function returned a tensor of shape {tuple(a.shape)} with "
                             f"{a.dtype} on {a.device}, expected the time points' {time_points.dtype} on {time_points.device}")
        # (L scaled copies summed, not ``a @ B``: the backward of that product onto ``B`` is a GEMM with an L x L result whose inner
        # dimension is every point and output of the batch, which the BLAS runs in ONE workgroup - 344 ms at B = 64, N = 10^4,
        # P = 5 on an MI355X, beside 0.4 ms for the data term; here it is L reductions)
        b = self._loading_matrix.to(dtype=a.dtype, device=a.device)
        return sum(a[..., l:l + 1] * b[l] for l in range(self.latent_dim))

    def latent_emission_model(self, time_points: torch.Tensor) -> EmissionModel:
        """The emission of the latent processes ``g``: ``IndependentMultiOutput``'s on the children, ``[.., N, L, state_dim]``."""
        return self._latent_components.generate_emission_model(time_points)

    def generate_emission_model(self, time_points: torch.Tensor) -> ComposedPairEmissionModel:
        """``H(t) = A(t) B (H_1 ⊕ H_2 ⊕ …)`` as a ``ComposedPairEmissionModel``."""
        return ComposedPairEmissionModel(EmissionModel(self.mixing_weights(time_points)), self.latent_emission_model(time_points))


def _refuse_factor_analysis(kernel, who: str) -> None:
    """``FactorAnalysisKernel`` mixes several latents into several observed series: the models written for ONE observed series per
    point refuse it."""
    if isinstance(kernel, FactorAnalysisKernel):
        raise NotImplementedError(f"{who} does not support a FactorAnalysisKernel (multi-output observations): use "
                                  "SparseVariationalGaussianProcess or GaussianProcessRegression")


ST_MAX_STATE_DIM = 64           # SparseSpatioTemporalKernel: Ms d_t, the range of the chain kernels and of mf_lik_st_expectations_*


class SparseSpatioTemporalKernel(IndependentMultiOutput):
    """``k((x, t), (x', t')) = k_s(x, x') k_t(t, t')`` with space marginalised to ``Ms`` inducing locations ``Z_s``
    (markovflow/models/spatio_temporal_variational.py:45-106): ``f(Z_s, .) = chol(K_s(Z_s, Z_s)) [h s_1(.), ..., h s_Ms(.)]`` with
    ``Ms`` independent copies ``s_i`` of ``kernel_time``'s state.  ``state_dim = Ms d_t`` (copy ``s`` in columns
    ``s d_t ... (s + 1) d_t - 1``), ``output_dim = Ms``.

    The chain's ``A``, ``chol Q`` and ``P_inf`` are ``I_Ms (x) `` the ``d_t x d_t`` blocks of ``kernel_time``, generated ONCE and placed
    on the block diagonal: the HIP generator never sees ``Ms`` component copies (it takes at most 16).  ``kernel_space`` is a
    ``spatial_kernels.SpatialKernel``; ``jitter`` is added to the diagonal of ``K_s(Z_s, Z_s)`` before its Cholesky."""

    def __init__(self, kernel_space, kernel_time: SDEKernel, inducing_space: torch.Tensor, jitter: float = 1e-6) -> None:
        from .spatial_kernels import SpatialKernel
        if not isinstance(kernel_space, SpatialKernel):
            raise TypeError("kernel_space must be a markovflow_amd.spatial_kernels.SpatialKernel")
        _refuse_non_stationary_children("SparseSpatioTemporalKernel", [kernel_time])
        _refuse_factor_analysis(kernel_time, "SparseSpatioTemporalKernel")
        if not isinstance(kernel_time, StationaryKernel) or kernel_time.output_dim != 1:
            raise TypeError("kernel_time must be a stationary markovflow_amd.kernels.SDEKernel with one output")
        if not isinstance(inducing_space, torch.Tensor) or inducing_space.dim() != 2 or inducing_space.shape[0] < 1:
            raise ValueError("inducing_space must be a tensor of shape [Ms, Dx] with Ms >= 1")
        if not jitter >= 0.0:
            raise ValueError("jitter must be a non-negative float number.")
        num_space = int(inducing_space.shape[0])
        if num_space * kernel_time.state_dim > ST_MAX_STATE_DIM:
            raise NotImplementedError(f"SparseSpatioTemporalKernel: Ms d_t = {num_space} x {kernel_time.state_dim} = "
                                      f"{num_space * kernel_time.state_dim} exceeds {ST_MAX_STATE_DIM}, the largest state dimension "
                                      "of the chain kernels")
        super().__init__([kernel_time] * num_space, kernel_time._jitter)
        self.kernel_space = kernel_space
        self.kernel_time = kernel_time
        self.inducing_space = inducing_space
        self.space_jitter = float(jitter)

    @property
    def num_inducing_space(self) -> int:
        return len(self._kernels)

    def _components(self):
        """ONE copy of ``kernel_time``'s components: the hyper-parameters behind the chain (for the caches and ``_needs_grad``)."""
        return self.kernel_time._components()

    def _replicate(self, block):
        return None if block is None else _kron(torch.eye(len(self._kernels), dtype=block.dtype, device=block.device), block)

    def _device_transitions(self, time_deltas: torch.Tensor, want_chol: bool, want_cov: bool, transition_times=None):
        """``I_Ms (x)`` the temporal kernel's ``(A, chol Q, Q)``: one generator call on ``d_t x d_t`` blocks."""
        return tuple(self._replicate(x) for x in self.kernel_time._device_transitions(time_deltas, want_chol, want_cov))

    def _torch_transitions(self, time_deltas: torch.Tensor, want_chol: bool, want_cov: bool):
        """The same replication of the temporal kernel's differentiable blocks: ``_components()`` is ONE copy's, so the inherited
        form would build ``d_t``-wide blocks against a ``state_dim``-wide jitter."""
        return tuple(self._replicate(x) for x in self.kernel_time._torch_transitions(time_deltas, want_chol, want_cov))

    def _initial_cholesky(self, batch, dtype, device):
        chol = self.kernel_time._initial_cholesky(batch, dtype, device)
        if chol is None:
            p0 = self.kernel_time.initial_covariance(torch.zeros(tuple(batch) + (1,), dtype=dtype, device=device))
            p0 = p0.to(dtype=dtype, device=device).expand(tuple(batch) + tuple(p0.shape[-2:])).contiguous()
            chol = _lib.checked_cholesky(p0, "SparseSpatioTemporalKernel (initial covariance)")
        return self._replicate(chol).contiguous()

    def space_cholesky(self, dtype=None, device=None) -> torch.Tensor:
        """``L = chol(K_s(Z_s, Z_s) + jitter I)``, ``[Ms, Ms]``; differentiable in the spatial hyper-parameters."""
        z = self.inducing_space if dtype is None else self.inducing_space.to(dtype=dtype, device=device)
        kzz = self.kernel_space.K(z)
        return torch.linalg.cholesky(kzz + self.space_jitter * torch.eye(kzz.shape[-1], dtype=kzz.dtype, device=kzz.device))

    def generate_emission_model(self, time_points: torch.Tensor) -> EmissionModel:
        """``chol(K_s(Z_s, Z_s)) (I_Ms (x) h)``, ``batch + [num_data, Ms, Ms d_t]`` (spatio_temporal_variational.py:72-85)."""
        h = super().generate_emission_model(time_points).emission_matrix
        return EmissionModel(self.space_cholesky(h.dtype, h.device) @ h)

    def space_weights(self, space_points: torch.Tensor) -> torch.Tensor:
        """``a = L^-1 K_s(Z_s, x)`` per point, ``[..., N, Ms]``: ``E[f(x, t) | s(t)] = a^T (I (x) h) s(t)``."""
        z = self.inducing_space.to(dtype=space_points.dtype, device=space_points.device)
        kzx = self.kernel_space.K(z, space_points)                                                  # [..., Ms, N]
        chol = self.space_cholesky(space_points.dtype, space_points.device)
        return torch.linalg.solve_triangular(chol, kzx, upper=False).transpose(-1, -2)

    def state_to_space_conditional_projection(self, inputs: torch.Tensor) -> torch.Tensor:
        """``P`` of ``E[f(x, t) | s(t)] = P s(t)`` for ``inputs [..., N, Dx + 1]`` (time in the last column),
        ``[..., N, 1, Ms d_t]`` (spatio_temporal_variational.py:87-106)."""
        space_points, time_points = inputs[..., :-1], inputs[..., -1]
        h = super().generate_emission_model(time_points).emission_matrix                            # [..., N, Ms, Ms d_t]
        return self.space_weights(space_points)[..., None, :] @ h


class _PiecewiseComponent:
    """Component ``j`` of a ``PiecewiseKernel``: the ``j``-th component of every segment's kernel, side by side.  It has what the
    models and caches walk (``order``, ``_osc``, ``_leaves()``, ``invalidate_cache()``) and is deliberately NOT a ``_MaternBase``: the
    fused Matérn routes of ``GaussianProcessRegression`` and ``SDEKernel._initial_cholesky`` would read ONE set of hyper-parameters
    off it.  ``_lambda`` / ``_variance_t`` / ``_omega`` carry the segments in a trailing dimension."""

    def __init__(self, per_segment) -> None:
        self._per_segment = list(per_segment)
        self.order, self._osc = per_segment[0].order, per_segment[0]._osc
        self.state_dim = per_segment[0].state_dim

    def _stack(self, tensors):
        shape = torch.broadcast_shapes(*[tuple(x.shape) for x in tensors])
        return torch.stack([x.expand(shape) for x in tensors], dim=-1)

    @property
    def _lambda(self) -> torch.Tensor:
        return self._stack([c._lambda for c in self._per_segment])

    @property
    def _variance_t(self) -> torch.Tensor:
        return self._stack([c._variance_t for c in self._per_segment])

    @property
    def _omega(self):
        return self._stack([c._omega for c in self._per_segment]) if self._osc else None

    def _leaves(self):
        return tuple(x for c in self._per_segment for x in c._leaves())

    def invalidate_cache(self) -> None:
        for c in self._per_segment:
            c.invalidate_cache()


def _structure(kernel):
    """The combinator tree of a kernel with the class of every node: what the segments of a ``PiecewiseKernel`` must share."""
    children = getattr(kernel, "kernels", None)
    return (type(kernel).__name__,) + (tuple(_structure(k) for k in children) if children is not None else ())


class _PiecewiseTransitions(torch.autograd.Function):
    """``_SdeTransitions`` for a ``PiecewiseKernel``: ``(A, chol Q)`` as a differentiable function of the stacked ``lam``, ``var``,
    ``omega`` (``[nseg, ncomp]`` or ``[B, nseg, ncomp]``) - forward ``mf_sde_piecewise_transitions_*``, backward
    ``mf_sde_piecewise_transitions_grad_*``, which also sums over the steps of every (series, segment) on the device, in a fixed
    order; only the sum over the series of shared hyper-parameters is left to torch."""

    @staticmethod
    def forward(ctx, t_start, dt, cp, lam_t, var_t, om_t, orders, oscs, per_series, jitter, want_chol):
        bsz, n = dt.shape
        d = sum((1 if o == 0 else (o + 1) // 2) * (2 if r else 1) for o, r in zip(orders, oscs))
        nseg = int(cp.shape[0]) + 1
        a_s = torch.empty((bsz, n, d, d), dtype=dt.dtype, device=dt.device)
        chol = torch.empty_like(a_s) if want_chol else None
        lam_c, var_c, om_c = lam_t.detach().contiguous(), var_t.detach().contiguous(), om_t.detach().contiguous()
        _lib.call("mf_sde_piecewise_transitions", dt.dtype, bsz, n, len(orders), (ctypes.c_int * len(orders))(*orders),
                  (ctypes.c_int * len(orders))(*oscs), nseg, _lib.ptr(cp if nseg > 1 else None), _lib.ptr(lam_c), _lib.ptr(var_c),
                  _lib.ptr(om_c), int(per_series), _lib.ptr(t_start), _lib.ptr(dt), jitter, _lib.ptr(a_s), _lib.ptr(chol), None, None,
                  _lib.stream_ptr(dt.device))
        ctx.save_for_backward(t_start, dt, cp, lam_c, var_c, om_c)
        ctx.meta = (orders, oscs, per_series, jitter)
        if not want_chol:
            chol = a_s.new_zeros(())
            ctx.mark_non_differentiable(chol)
        return a_s, chol

    @staticmethod
    def backward(ctx, g_a, g_chol):
        t_start, dt, cp, lam_c, var_c, om_c = ctx.saved_tensors
        orders, oscs, per_series, jitter = ctx.meta
        bsz, n = dt.shape
        nseg = int(cp.shape[0]) + 1
        out = torch.empty((bsz, nseg, len(orders), 3), dtype=dt.dtype, device=dt.device)
        with torch.no_grad():
            ga = None if g_a is None else g_a.contiguous()
            gc = None if (g_chol is None or g_chol.dim() == 0) else g_chol.contiguous()
            ws_bytes = int(_lib.load().mf_sde_piecewise_transitions_grad_workspace_bytes(bsz, n, len(orders), dt.element_size()))
            ws = _lib.workspace(ws_bytes, dt.device)
            _lib.call("mf_sde_piecewise_transitions_grad", dt.dtype, bsz, n, len(orders), (ctypes.c_int * len(orders))(*orders),
                      (ctypes.c_int * len(orders))(*oscs), nseg, _lib.ptr(cp if nseg > 1 else None), _lib.ptr(lam_c), _lib.ptr(var_c),
                      _lib.ptr(om_c), int(per_series), _lib.ptr(t_start), _lib.ptr(dt), jitter, _lib.ptr(ga), _lib.ptr(gc),
                      _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dt.device))
            g = out if per_series else torch.sum(out, dim=0)              # shared hyper-parameters: [nseg, ncomp, 3]
        return (None, None, None, g[..., 0].contiguous(), g[..., 1].contiguous(), g[..., 2].contiguous(), None, None, None, None,
                None)


class PiecewiseKernel(NonStationaryKernel):
    """Piecewise-stationary kernel (markovflow/kernels/piecewise_stationary.py:28-289): ``K`` sorted change points ``c_1 < … < c_K``
    split the time axis into ``K + 1`` segments ``(−∞, c_1), [c_1, c_2), …, [c_K, ∞)``, and on segment ``k`` the state follows the SDE
    of ``kernels[k]`` - a different lengthscale, variance or period on each side of a change point.  The state is shared: the
    segments' kernels have one signature (the same combinator structure and the same ``(order, oscillator)`` per component), e.g.
    all ``Matern32``, all ``Matern52 * HarmonicOscillator`` or all ``Constant + Matern12``.

    ``(A_k, chol Q_k)`` come from ONE launch of ``mf_sde_piecewise_transitions_*`` (csrc/mf_sde.hip), which looks the segment of
    every step up in the kernel; under a gradient on a HIP device the backward is ``mf_sde_piecewise_transitions_grad_*``.  CPU tensors
    under a gradient, ``Q`` under a gradient and gradients with respect to the times take a differentiable torch restatement.

    Limitations, all stated in DESIGN.md ("Piecewise-stationary kernels"):

    * *The crossing rule.*  A transition is generated ENTIRELY from the segment its start time lies in (a start time exactly on a
      change point belongs to the segment after it): ``Q_k = P∞(seg) − A_k P∞(seg) A_kᵀ + jitter`` with ``A_k`` of the same segment,
      also when ``t_k + Δt_k`` lies beyond the next change point.  This is the reference's behaviour; the chain is the exact
      marginal of the process only if no transition crosses a change point, i.e. if the change points are among the time points.
    * *Shared change points.*  ``change_points`` is ONE 1-D tensor for all series; it is sorted, finite and not trainable.  The
      children's hyper-parameters may carry ``batch_shape`` as elsewhere.
    * *GPR only.*  ``GaussianProcessRegression`` (likelihood, its backward, ``posterior.predict_f`` / ``predict_state``, sampling)
      supports it, through the materialised route generator → ``KalmanFilter``; every other model refuses a ``NonStationaryKernel``.
    * *Stationarity before the first point.*  Before the first conditioning point the process is taken to be stationary under the
      kernel active AT that point: ``initial_covariance(t0)`` is ``P∞`` of the segment holding each series' ``t0`` (the reference
      indexes ``[0]`` there, which takes the first batch entry), and a prediction before the first conditioning point - and the
      joint prior that posterior samples start from - uses that segment, whatever segment the new point itself lies in
      (``_lookup_times``).  ``change_points`` is read-only.

    As a child of ``Sum``, ``Product``, ``IndependentMultiOutput`` or ``SparseSpatioTemporalKernel`` it is refused: a sum of piecewise
    kernels is written as a piecewise kernel of sums."""

    def __init__(self, kernels: List[StationaryKernel], change_points: torch.Tensor, jitter: float = 0.0) -> None:
        self._kernels = list(kernels)
        assert self._kernels, "There must be at least one child kernel."                    # piecewise_stationary.py:64-72
        if any(isinstance(k, (IndependentMultiOutput, NonStationaryKernel)) for k in self._kernels):
            raise NotImplementedError("PiecewiseKernel segments are single-output stationary kernels: IndependentMultiOutput, "
                                      "SparseSpatioTemporalKernel and PiecewiseKernel children are not supported")
        _refuse_non_stationary_children("PiecewiseKernel", [k for k in self._kernels if isinstance(k, LatentExponentiallyGenerated)])
        if not all(isinstance(k, StationaryKernel) for k in self._kernels):
            raise TypeError("can only combine Kernel instances")
        assert len({k.output_dim for k in self._kernels}) == 1, "All kernels must have the same output dimension"
        assert len({k.state_dim for k in self._kernels}) == 1, "All kernels must have the same state dimension"
        if not all(isinstance(k, type(self._kernels[0])) for k in self._kernels):
            raise TypeError("can only combine kernels from the same class")
        comps = [k._components() for k in self._kernels]
        if len({_structure(k) for k in self._kernels}) != 1 or len({tuple((c.order, c._osc) for c in row) for row in comps}) != 1:
            raise TypeError("can only combine kernels of one signature: the same combinator structure and the same (order, "
                            "oscillator) of every component")
        if not isinstance(change_points, torch.Tensor) or change_points.dim() != 1:
            raise ValueError("change_points must be a 1-D tensor")
        assert len(self._kernels) == change_points.shape[0] + 1, "There must be one more kernel than change points"
        cp = change_points.detach()
        if cp.numel() and not (bool(torch.isfinite(cp).all()) and bool((cp[1:] >= cp[:-1]).all())):
            raise ValueError("change_points must be finite and sorted in ascending order")
        super().__init__(self._kernels[0].output_dim, jitter)
        self._change_points = cp.clone()
        self.num_change_points = int(cp.shape[0])
        self._state_dim = self._kernels[0].state_dim
        self._pieces = [_PiecewiseComponent([row[j] for row in comps]) for j in range(len(comps[0]))]
        # every segment under THIS kernel's jitter (a child's own jitter plays no part, as in the reference)
        self._segments = [Sum([k], jitter=jitter) for k in self._kernels]
        self._cp_cache = {}

    @property
    def kernels(self) -> List[StationaryKernel]:
        return self._kernels

    @property
    def state_dim(self) -> int:
        return self._state_dim

    def _components(self):
        return self._pieces

    def invalidate_cache(self) -> None:
        for k in self._kernels:
            k.invalidate_cache()

    @property
    def change_points(self) -> torch.Tensor:
        """The sorted change points (a copy of the constructor's argument; read-only: a kernel with other change points is
        another kernel)."""
        return self._change_points

    def _change_points_as(self, ref: torch.Tensor) -> torch.Tensor:
        """The change points in the dtype and on the device of ``ref`` (the comparison runs in that dtype).  The copies are keyed on
        the version counter too, so that an in-place write to ``change_points`` - which must keep them sorted - is not ignored."""
        key = (ref.dtype, str(ref.device), _version_key(self._change_points))
        if key not in self._cp_cache:
            self._cp_cache = {k: v for k, v in self._cp_cache.items() if k[2] == key[2]}
            self._cp_cache[key] = self._change_points.to(dtype=ref.dtype, device=ref.device).contiguous()
        return self._cp_cache[key]

    # -- the reference's methods ---------------------------------------------------------------------------------------------------
    def split_time_indices(self, time_points: torch.Tensor) -> torch.Tensor:
        """The segment of every time point, ``0 … num_change_points``, ``batch_shape + [num_time_points]``: the number of change
        points ``<= t`` (piecewise_stationary.py:126-143: ``searchsorted(..., "right") - 1`` on the ±∞-augmented array)."""
        return torch.searchsorted(self._change_points_as(time_points), time_points.detach().contiguous(), right=True)

    def _gather_segments(self, per_segment: List[torch.Tensor], time_points: torch.Tensor, trailing: int) -> torch.Tensor:
        batch = tuple(time_points.shape[:-1])
        tail = tuple(per_segment[0].shape[-trailing:])
        stacked = torch.stack([x.to(device=time_points.device).expand(batch + tail) for x in per_segment], dim=len(batch))
        idx = self.split_time_indices(time_points).reshape(tuple(time_points.shape) + (1,) * trailing)
        return torch.gather(stacked, len(batch), idx.expand(tuple(time_points.shape) + tail))

    def steady_state_covariances(self, time_points: torch.Tensor) -> torch.Tensor:
        """``P∞`` of the kernel active at every time point (piecewise_stationary.py:162-178)."""
        return self._gather_segments([k.steady_state_covariance for k in self._kernels], time_points, 2)

    def feedback_matrices(self, time_points: torch.Tensor) -> torch.Tensor:
        """``F`` of the kernel active at every time point (piecewise_stationary.py:230-246)."""
        return self._gather_segments([k.feedback_matrix for k in self._kernels], time_points, 2)

    def state_means(self, time_points: torch.Tensor) -> torch.Tensor:
        """Zero (piecewise_stationary.py:273-288: the stationary children have zero state means)."""
        ref = self._pieces[0]._variance_t
        return torch.zeros(tuple(time_points.shape) + (self.state_dim,), dtype=ref.dtype, device=time_points.device)

    def initial_mean(self, batch_shape) -> torch.Tensor:
        ref = self._pieces[0]._variance_t
        return torch.zeros(tuple(batch_shape) + (self.state_dim,), dtype=ref.dtype, device=ref.device)

    def initial_covariance(self, initial_time_point: torch.Tensor) -> torch.Tensor:
        """``P∞ + jitter`` of the segment holding each series' initial time point, ``batch_shape + [state_dim, state_dim]``."""
        assert initial_time_point.shape[-1] == 1
        p = self.steady_state_covariances(initial_time_point)[..., 0, :, :]
        return p + self.jitter_matrix.to(dtype=p.dtype, device=p.device)

    def state_offsets(self, transition_times: torch.Tensor, time_deltas: torch.Tensor) -> torch.Tensor:
        """Zero, as for every stationary child (piecewise_stationary.py:248-271)."""
        return torch.zeros(tuple(time_deltas.shape) + (self.state_dim,), dtype=time_deltas.dtype, device=time_deltas.device)

    def generate_emission_model(self, time_points: torch.Tensor) -> EmissionModel:
        """The children's shared emission model (piecewise_stationary.py:89-109, "assuming for now a shared emission model")."""
        return self._kernels[0].generate_emission_model(time_points)

    def _lookup_times(self, times, conditioning_time_points):
        """Before the first conditioning point the process is stationary under the kernel active AT that point: a time before it
        is looked up at it."""
        return torch.maximum(times, conditioning_time_points[..., :1].to(times.dtype))

    # -- transitions ---------------------------------------------------------------------------------------------------------------
    def _torch_transitions(self, time_deltas: torch.Tensor, want_chol: bool, want_cov: bool, transition_times=None):
        """The reference's algorithm in differentiable torch ops: every segment's closed forms on all steps, selected per step."""
        seg = self.split_time_indices(transition_times.to(time_deltas.dtype))
        out = None
        for k, kern in enumerate(self._segments):
            part = kern._torch_transitions(time_deltas, want_chol, want_cov)
            if out is None:
                out = list(part)
                continue
            here = (seg == k)[..., None, None]
            out = [None if x is None else torch.where(here, y, x) for x, y in zip(out, part)]
        return tuple(out)

    def _stacked_hyper(self, dtype, device, batch):
        """``lam``, ``var``, ``omega`` as ``[nseg, ncomp]`` or, when a hyper-parameter has a batch shape, ``[B, nseg, ncomp]``."""
        zero = torch.zeros((), dtype=dtype, device=device)
        rows = [k._components() for k in self._kernels]
        groups = [[[c._lambda.to(dtype=dtype, device=device) for c in row] for row in rows],
                  [[c._variance_t.to(dtype=dtype, device=device) for c in row] for row in rows],
                  [[zero if c._omega is None else c._omega.to(dtype=dtype, device=device) for c in row] for row in rows]]
        per_series = any(x.dim() > 0 for g in groups for row in g for x in row)
        if per_series:
            return per_series, [torch.stack([torch.stack([x.expand(batch).reshape(-1) for x in row], dim=-1) for row in g],
                                            dim=-2).contiguous() for g in groups]
        return per_series, [torch.stack([torch.stack(row) for row in g]).contiguous() for g in groups]

    def _device_transitions(self, time_deltas: torch.Tensor, want_chol: bool, want_cov: bool, transition_times=None):
        """``(A, chol Q, Q)`` through ``mf_sde_piecewise_transitions_*``; ``transition_times`` is required."""
        if transition_times is None:
            raise ValueError("PiecewiseKernel: the transitions depend on transition_times (the time every transition starts at)")
        if tuple(transition_times.shape) != tuple(time_deltas.shape):
            raise ValueError("transition_times and time_deltas must have one shape")
        batch = tuple(time_deltas.shape[:-1])
        n, d = time_deltas.shape[-1], self.state_dim
        needs_grad = self._needs_grad()
        times_grad = torch.is_grad_enabled() and (time_deltas.requires_grad or transition_times.requires_grad)
        if times_grad or (needs_grad and (want_cov or not time_deltas.is_cuda or time_deltas.numel() == 0)):
            return self._torch_transitions(time_deltas, want_chol, want_cov, transition_times)
        dt = time_deltas.detach().reshape(-1, n).contiguous()
        t_start = transition_times.detach().to(dt.dtype).reshape(-1, n).contiguous()
        bsz = dt.shape[0]
        cp = self._change_points_as(dt)
        per_series, (lam_t, var_t, om_t) = self._stacked_hyper(dt.dtype, dt.device, batch)
        comps = self._pieces
        orders, oscs = tuple(c.order for c in comps), tuple(c._osc for c in comps)
        shape = batch + (n, d, d)
        if needs_grad:
            a_s, chol = _PiecewiseTransitions.apply(t_start, dt, cp, lam_t, var_t, om_t, orders, oscs, bool(per_series),
                                                    float(self._jitter), bool(want_chol))
            return a_s.reshape(shape), (chol.reshape(shape) if want_chol else None), None
        a_s = torch.empty((bsz, n, d, d), dtype=dt.dtype, device=dt.device)
        chol = torch.empty_like(a_s) if want_chol else None
        cov = torch.empty_like(a_s) if want_cov else None
        _lib.call("mf_sde_piecewise_transitions", dt.dtype, bsz, n, len(comps), (ctypes.c_int * len(comps))(*orders),
                  (ctypes.c_int * len(comps))(*oscs), self.num_change_points + 1, _lib.ptr(cp if self.num_change_points else None),
                  _lib.ptr(lam_t), _lib.ptr(var_t), _lib.ptr(om_t), int(per_series), _lib.ptr(t_start), _lib.ptr(dt), self._jitter,
                  _lib.ptr(a_s), _lib.ptr(chol), _lib.ptr(cov), None, _lib.stream_ptr(dt.device))
        return (a_s.reshape(shape), None if chol is None else chol.reshape(shape), None if cov is None else cov.reshape(shape))


class _LegTransitions(torch.autograd.Function):
    """``(A [B,n,d,d], chol Q [B,n,d,d])`` of a ``LatentExponentiallyGenerated`` kernel as a differentiable function of its feedback
    matrix ``F`` (``[d,d]`` or ``[B,d,d]``) - forward ``mf_sde_leg_transitions_*``, backward ``mf_sde_leg_transitions_grad_*`` (the
    Cholesky adjoint and the Fréchet adjoint of the exponential per step, summed over the steps of a series on the device in a fixed
    order); only the sum over the series of a shared ``F`` is left to torch.  ``F`` is assembled from ``N`` and ``R`` by differentiable
    torch ops, which carry the gradient on."""

    @staticmethod
    def forward(ctx, dt, f_t, per_series, jitter, want_chol):
        bsz, n = dt.shape
        d = f_t.shape[-1]
        a_s = torch.empty((bsz, n, d, d), dtype=dt.dtype, device=dt.device)
        chol = torch.empty_like(a_s) if want_chol else None
        f_c = f_t.detach().contiguous()
        _lib.call("mf_sde_leg_transitions", dt.dtype, bsz, n, d, _lib.ptr(f_c), int(per_series), _lib.ptr(dt), jitter, _lib.ptr(a_s),
                  _lib.ptr(chol), None, _lib.stream_ptr(dt.device))
        ctx.save_for_backward(dt, f_c)
        ctx.meta = (per_series, jitter)
        if not want_chol:
            chol = a_s.new_zeros(())
            ctx.mark_non_differentiable(chol)
        return a_s, chol

    @staticmethod
    def backward(ctx, g_a, g_chol):
        dt, f_c = ctx.saved_tensors
        per_series, jitter = ctx.meta
        bsz, n = dt.shape
        d = f_c.shape[-1]
        out = torch.empty((bsz, d, d), dtype=dt.dtype, device=dt.device)
        with torch.no_grad():
            ga = None if g_a is None else g_a.contiguous()
            gc = None if (g_chol is None or g_chol.dim() == 0) else g_chol.contiguous()
            ws_bytes = int(_lib.load().mf_sde_leg_transitions_grad_workspace_bytes(bsz, n, d, dt.element_size()))
            ws = _lib.workspace(ws_bytes, dt.device)
            _lib.call("mf_sde_leg_transitions_grad", dt.dtype, bsz, n, d, _lib.ptr(f_c), int(per_series), _lib.ptr(dt), jitter,
                      _lib.ptr(ga), _lib.ptr(gc), _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dt.device))
            g = out if per_series else torch.sum(out, dim=0)              # a shared F: [d, d]
        return None, g, None, None, None


LEG_MAX_DEVICE_STATE_DIM = 16


class LatentExponentiallyGenerated(StationaryKernel):
    """The latent exponentially generated kernel of Loper et al. 2020 (markovflow/kernels/latent_exp_generated.py): a state of
    dimension ``d`` with a DENSE feedback matrix ``F = −½(N Nᵀ + R − Rᵀ)`` and steady-state covariance ``I``,

        ``A_k = expm(Δt_k F)``,  ``Q_k = I − A_k A_kᵀ + jitter·I``,

    ``N`` and ``R`` being ``[d, d]`` tensors (or ``batch_shape + [d, d]``: dynamics per series) that may require gradients.

    On a HIP device and for ``d <= 16`` the transitions come from ``mf_sde_leg_transitions_*`` (csrc/mf_leg.hip: scaling and squaring
    with ``expm − I`` carried through the squarings, so that ``Q_k`` keeps its relative accuracy at short gaps, where ``I − A Aᵀ``
    cancels), and under a gradient from ``_LegTransitions``, whose backward is ``mf_sde_leg_transitions_grad_*``.  CPU tensors, ``Q``
    under a gradient, gradients with respect to the times, ``d > 16`` and empty inputs take a torch restatement
    (``torch.linalg.matrix_exp``), which forms ``I − A Aᵀ`` as the reference does.

    ``output_dim=None`` reproduces the reference: ``output_dim = state_dim`` and every row of the emission matrix is ``[1, 0, …]``.
    ``output_dim=1`` is this project's extension: the scalar process that the one-output likelihood models need.

    Models: ``GaussianProcessRegression`` (the materialised route generator → ``KalmanFilter``) and, with ``output_dim=1``,
    ``SparseVariationalGaussianProcess`` are covered by tests; other models reach the kernel through the same public methods but
    are not.  As a child of ``Sum``, ``Product``, ``IndependentMultiOutput``, ``SparseSpatioTemporalKernel`` or ``PiecewiseKernel`` it
    is refused."""

    def __init__(self, N: torch.Tensor, R: torch.Tensor, jitter: float = 0.0, output_dim: Optional[int] = None) -> None:
        if not (isinstance(N, torch.Tensor) and isinstance(R, torch.Tensor)):
            raise TypeError("N and R must be tensors")
        if N.dim() < 2 or N.shape[-1] != N.shape[-2] or tuple(N.shape) != tuple(R.shape):
            raise ValueError("N and R must be square matrices of one shape, batch_shape + [state_dim, state_dim]")
        if N.dtype != R.dtype or N.device != R.device:
            raise ValueError("N and R must share dtype and device")
        self._state_dim = int(N.shape[-1])
        super().__init__(self._state_dim if output_dim is None else int(output_dim), jitter)
        self._N, self._R = N, R

    @property
    def state_dim(self) -> int:
        return self._state_dim

    @property
    def N(self) -> torch.Tensor:
        return self._N

    @property
    def R(self) -> torch.Tensor:
        return self._R

    @property
    def feedback_matrix(self) -> torch.Tensor:
        """``F = −½(N Nᵀ + R − Rᵀ)`` (latent_exp_generated.py ``feedback_matrix``), differentiable in ``N`` and ``R``."""
        n, r = self._N, self._R
        return -0.5 * (n @ n.transpose(-1, -2) + r - r.transpose(-1, -2))

    @property
    def steady_state_covariance(self) -> torch.Tensor:
        eye = torch.eye(self._state_dim, dtype=self._N.dtype, device=self._N.device)
        return eye.expand(tuple(self._N.shape)).clone()

    # -- what the rest of the package asks of a kernel ------------------------------------------------------------------------------
    def _components(self):
        return [self]

    def _leaves(self):
        return (self._N, self._R)

    def invalidate_cache(self) -> None:
        """Nothing is cached: ``F`` is assembled from ``N`` and ``R`` at every call."""

    @property
    def jitter_matrix(self) -> torch.Tensor:
        return self._jitter * torch.eye(self._state_dim, dtype=self._N.dtype, device=self._N.device)

    def initial_mean(self, batch_shape) -> torch.Tensor:
        return torch.zeros(tuple(batch_shape) + (self._state_dim,), dtype=self._N.dtype, device=self._N.device)

    def initial_covariance(self, initial_time_point: torch.Tensor) -> torch.Tensor:
        """``(1 + jitter)·I``."""
        assert initial_time_point.shape[-1] == 1
        batch = tuple(initial_time_point.shape[:-1])
        eye = torch.eye(self._state_dim, dtype=self._N.dtype, device=self._N.device)
        return ((1.0 + self._jitter) * eye).expand(batch + (self._state_dim, self._state_dim)).clone()

    def _needs_grad(self) -> bool:
        return torch.is_grad_enabled() and (self._N.requires_grad or self._R.requires_grad)

    def _initial_cholesky(self, batch, dtype, device):
        eye = torch.eye(self._state_dim, dtype=dtype, device=device)
        return (math.sqrt(1.0 + self._jitter) * eye).expand(tuple(batch) + (self._state_dim, self._state_dim)).contiguous()

    # -- transitions -----------------------------------------------------------------------------------------------------------------
    def _torch_transitions(self, time_deltas: torch.Tensor, want_chol: bool, want_cov: bool):
        """The reference's formulas in differentiable torch ops: ``A = matrix_exp(Δt F)``, ``Q = I − A Aᵀ + jitter·I`` (symmetrised),
        its Cholesky factor with an all-zero ``Q`` passed through as a zero factor."""
        f = self.feedback_matrix.to(dtype=time_deltas.dtype, device=time_deltas.device)
        f_b = f[..., None, :, :] if f.dim() > 2 else f
        a_s = torch.linalg.matrix_exp(f_b * time_deltas[..., None, None])
        if not (want_chol or want_cov):
            return a_s, None, None
        eye = torch.eye(self._state_dim, dtype=time_deltas.dtype, device=time_deltas.device)
        q = eye - a_s @ a_s.transpose(-1, -2)
        # (a skew F - N = 0 - has no process noise at all: exact zeros, as the device kernel gives, not the rounding of I − A Aᵀ)
        noisy = ~(f_b + f_b.transpose(-1, -2) == 0).all(dim=-1).all(dim=-1)[..., None, None]
        q_s = 0.5 * (q + q.transpose(-1, -2)) * noisy.to(q.dtype) + self._jitter * eye
        chol = None
        if want_chol:
            zero = (q_s == 0).all(dim=-1).all(dim=-1)[..., None, None]
            chol = torch.linalg.cholesky(torch.where(zero, eye, q_s)) * (~zero).to(q_s.dtype)
        return a_s, chol, (q_s if want_cov else None)

    def _device_transitions(self, time_deltas: torch.Tensor, want_chol: bool, want_cov: bool, transition_times=None):
        """``(A, chol Q, Q)`` for ``time_deltas`` of shape ``batch_shape + [n]``: ``mf_sde_leg_transitions_*``, under a gradient
        ``_LegTransitions``; the torch restatement where the class docstring says so."""
        batch = tuple(time_deltas.shape[:-1])
        n, d = time_deltas.shape[-1], self._state_dim
        needs_grad = self._needs_grad()
        times_grad = torch.is_grad_enabled() and time_deltas.requires_grad
        if (not time_deltas.is_cuda or time_deltas.numel() == 0 or d > LEG_MAX_DEVICE_STATE_DIM or times_grad
                or (needs_grad and want_cov)):
            return self._torch_transitions(time_deltas, want_chol, want_cov)
        dt = time_deltas.detach().reshape(-1, n).contiguous()
        bsz = dt.shape[0]
        f = self.feedback_matrix.to(dtype=dt.dtype, device=dt.device)
        per_series = f.dim() > 2
        f_t = f.expand(batch + (d, d)).reshape(-1, d, d) if per_series else f
        shape = batch + (n, d, d)
        if needs_grad:
            a_s, chol = _LegTransitions.apply(dt, f_t, bool(per_series), float(self._jitter), bool(want_chol))
            return a_s.reshape(shape), (chol.reshape(shape) if want_chol else None), None
        f_c = f_t.detach().contiguous()
        a_s = torch.empty((bsz, n, d, d), dtype=dt.dtype, device=dt.device)
        chol = torch.empty_like(a_s) if want_chol else None
        cov = torch.empty_like(a_s) if want_cov else None
        _lib.call("mf_sde_leg_transitions", dt.dtype, bsz, n, d, _lib.ptr(f_c), int(per_series), _lib.ptr(dt), self._jitter,
                  _lib.ptr(a_s), _lib.ptr(chol), _lib.ptr(cov), _lib.stream_ptr(dt.device))
        return (a_s.reshape(shape), None if chol is None else chol.reshape(shape), None if cov is None else cov.reshape(shape))
