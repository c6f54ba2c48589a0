"""
Likelihoods for the site-based models (``CVIGaussianProcess``): what ``markovflow/models/variational_cvi.py:321-420`` asks of
gpflow's likelihood classes - ``log_prob``, ``variational_expectations``, ``predict_log_density``, ``predict_mean_and_var`` - for

    * ``Gaussian(variance)``,
    * ``Bernoulli()``   with gpflow's probit link  ``p = 0.5 (1 + erf(f / sqrt 2)) (1 - 2e-3) + 1e-3``,  ``y in {0, 1}``,
    * ``Poisson()``     with the exp link and bin size 1,
    * ``StudentT(scale, df)``.

Tensors are ``batch + [N, 1]`` (one latent function, one output); ``variational_expectations`` and ``predict_log_density`` return
``batch + [N]`` as gpflow does.  On HIP tensors the expectations run in ONE kernel (``mf_lik_*``, csrc/mf_lik.hip: a lane per data
point, the Gauss-Hermite rule in the kernel arguments); CPU tensors take the torch statement of the same formulas below
(``torch_variational_expectations`` / ``torch_predict_log_density``), which is also what the kernel is timed against.

Gaussian and Poisson expectations are closed forms; Bernoulli and Student-t use an ``nq``-point Gauss-Hermite rule with
``f_i = mu + sqrt(2 var) x_i`` and ``w_i = weight_i / sqrt(pi)``:

    VE = sum w_i l(f_i),    dVE/dmu = sum w_i l'(f_i),    dVE/dvar = sum w_i l'(f_i) x_i / sqrt(2 var)

- the exact derivatives of the discretised sum (what the reference's tape through ``ndiagquad`` computes).  The domain is
``var > 0``: a point with a non-positive or NaN variance gets NaN.

The parameters (``variance``, ``scale``, ``df``) are plain Python floats and are NOT trainable.
"""
import ctypes
import math
from typing import Tuple

import numpy as np
import torch

from . import _lib

_JITTER = 1e-3          # gpflow's inv_probit
_MAX_POINTS = 32        # the rule travels in the kernel arguments


def _inv_probit(f: torch.Tensor) -> torch.Tensor:
    return 0.5 * (1.0 + torch.erf(f / math.sqrt(2.0))) * (1.0 - 2.0 * _JITTER) + _JITTER


class Likelihood:
    """Base class: the id and parameters the kernels take, the Gauss-Hermite rule, and the four methods.  Parameters are plain
    floats, not trainable."""

    _id = -1

    def __init__(self, num_gauss_hermite_points: int = 20) -> None:
        nq = int(num_gauss_hermite_points)
        if nq != num_gauss_hermite_points or not 1 <= nq <= _MAX_POINTS:
            raise ValueError(f"num_gauss_hermite_points must be an integer in 1..{_MAX_POINTS}, got {num_gauss_hermite_points}")
        self.num_gauss_hermite_points = nq
        self._nodes, self._weights = np.polynomial.hermite.hermgauss(nq)              # float64; weights sum to sqrt(pi)
        self._c_nodes = (ctypes.c_double * nq)(*self._nodes)
        self._c_weights = (ctypes.c_double * nq)(*self._weights)
        self._rule_tensors = {}        # (dtype, device) -> nodes, weights / sqrt(pi), log of those: the torch route's constants

    def _rule(self, ref: torch.Tensor):
        key = (ref.dtype, ref.device)
        if key not in self._rule_tensors:
            w = self._weights / math.sqrt(math.pi)
            self._rule_tensors[key] = tuple(torch.as_tensor(a, dtype=ref.dtype, device=ref.device) for a in (self._nodes, w, np.log(w)))
        return self._rule_tensors[key]

    # ---- what a subclass provides ------------------------------------------------------------------------------------------
    def _params(self) -> Tuple[float, ...]:
        return ()

    def _log_prob_and_grad(self, f: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``log p(y | f)`` and its derivative in ``f``, element-wise."""
        raise NotImplementedError

    def _closed_expectations(self, mu, var, y):
        """``(VE, dVE/dmu, dVE/dvar)`` in closed form, or None (quadrature)."""
        return None

    def predict_mean_and_var(self, fmu: torch.Tensor, fvar: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Mean and variance of ``y`` under ``f ~ N(fmu, fvar)`` (closed forms), shapes of ``fmu``."""
        raise NotImplementedError

    # ---- shared ----------------------------------------------------------------------------------------------------------------
    def _c_params(self):
        p = self._params()
        return (ctypes.c_double * len(p))(*p) if p else None

    def _check(self, what: str, fmu: torch.Tensor, **others: torch.Tensor):
        if fmu.dim() < 2 or fmu.shape[-1] != 1:
            raise ValueError(f"{type(self).__name__}.{what}: tensors must have shape batch + [N, 1], got {tuple(fmu.shape)}")
        for name, t in others.items():
            if tuple(t.shape) != tuple(fmu.shape):
                raise ValueError(f"{type(self).__name__}.{what}: {name} has shape {tuple(t.shape)}, expected {tuple(fmu.shape)}")
        if fmu.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {fmu.dtype}")
        _lib.same_dtype_device(fmu, f"{type(self).__name__}.{what}", **others)

    def log_prob(self, f: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``log p(y | f)``, ``batch + [N, 1] -> batch + [N]`` (element-wise torch on either device)."""
        self._check("log_prob", f, y=y)
        return self._log_prob_and_grad(f, y)[0][..., 0]

    def variational_expectations(self, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``E_{N(f | fmu, fvar)} log p(y | f)``, ``batch + [N]``.  Differentiable ONCE in ``fmu`` and ``fvar``: the backward
        multiplies the derivatives the forward computed alongside the value (no second-order support)."""
        self._check("variational_expectations", fmu, fvar=fvar, y=y)
        return _VariationalExpectations.apply(fmu, fvar, y, self)[..., 0]

    def predict_log_density(self, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``log int p(y | f) N(f | fmu, fvar) df``, ``batch + [N]`` (not differentiable)."""
        self._check("predict_log_density", fmu, fvar=fvar, y=y)
        with torch.no_grad():
            if not fmu.is_cuda:
                return torch_predict_log_density(self, fmu, fvar, y)[..., 0]
            mu, var, obs = fmu.contiguous(), fvar.contiguous(), y.contiguous()
            out = torch.empty_like(mu)
            _lib.call("mf_lik_predict_log_density", mu.dtype, mu.numel(), self._id, self._c_params(), self.num_gauss_hermite_points,
                      self._c_nodes, self._c_weights, _lib.ptr(mu), _lib.ptr(var), _lib.ptr(obs), _lib.ptr(out),
                      _lib.stream_ptr(mu.device))
            return out[..., 0]

    def _expectations(self, fmu, fvar, y):
        """``(VE, dVE/dmu, dVE/dvar)``, each of ``fmu``'s shape: the kernel on HIP tensors, torch on CPU tensors."""
        if not fmu.is_cuda:
            return torch_variational_expectations(self, fmu, fvar, y)
        mu, var, obs = fmu.contiguous(), fvar.contiguous(), y.contiguous()
        ve, g_mu, g_var = torch.empty_like(mu), torch.empty_like(mu), torch.empty_like(mu)
        _lib.call("mf_lik_variational_expectations", mu.dtype, mu.numel(), self._id, self._c_params(), self.num_gauss_hermite_points,
                  self._c_nodes, self._c_weights, _lib.ptr(mu), _lib.ptr(var), _lib.ptr(obs), _lib.ptr(ve), _lib.ptr(g_mu),
                  _lib.ptr(g_var), _lib.stream_ptr(mu.device))
        return ve, g_mu, g_var

    def cvi_site_update(self, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor, learning_rate: float, nat1: torch.Tensor,
                        nat2: torch.Tensor) -> None:
        """One CVI step on the sites, IN PLACE (variational_cvi.py:351-368): with ``g2 = dVE/dvar`` and ``g1 = dVE/dmu - 2 g2 fmu``
        (the gradient in the expectation parameters ``[mu, var + mu^2]``), ``nat <- (1 - lr) nat + lr g``.  ``nat1`` and ``nat2``
        hold one element per element of ``fmu`` (any shape) and must be contiguous.  HIP tensors: one launch of
        ``mf_lik_cvi_site_update_*``."""
        self._check("cvi_site_update", fmu, fvar=fvar, y=y)
        _lib.same_dtype_device(fmu, f"{type(self).__name__}.cvi_site_update", nat1=nat1, nat2=nat2)
        if nat1.numel() != fmu.numel() or nat2.numel() != fmu.numel() or not nat1.is_contiguous() or not nat2.is_contiguous():
            raise ValueError("cvi_site_update: nat1 and nat2 must be contiguous and hold one element per data point")
        if not 0.0 <= float(learning_rate) <= 1.0:
            raise ValueError(f"cvi_site_update: learning_rate must lie in [0, 1], got {learning_rate}")
        lr = float(learning_rate)
        with torch.no_grad():
            if not fmu.is_cuda:
                _, g_mu, g_var = torch_variational_expectations(self, fmu, fvar, y)
                nat1.mul_(1.0 - lr).add_(lr * (g_mu - 2.0 * g_var * fmu).reshape(nat1.shape))
                nat2.mul_(1.0 - lr).add_(lr * g_var.reshape(nat2.shape))
                return
            mu, var, obs = fmu.contiguous(), fvar.contiguous(), y.contiguous()
            _lib.call("mf_lik_cvi_site_update", mu.dtype, mu.numel(), self._id, self._c_params(), self.num_gauss_hermite_points,
                      self._c_nodes, self._c_weights, _lib.ptr(mu), _lib.ptr(var), _lib.ptr(obs), lr, _lib.ptr(nat1), _lib.ptr(nat2),
                      None, _lib.stream_ptr(mu.device))
            # the kernel wrote through raw pointers: tell torch, so that whatever keys a cache on (tensor, version) sees the write
            torch.autograd.graph.increment_version(nat1)
            torch.autograd.graph.increment_version(nat2)


class _VariationalExpectations(torch.autograd.Function):
    """Value ``batch + [N, 1]`` with the two derivatives computed in the same pass and saved for the backward."""

    @staticmethod
    def forward(ctx, fmu, fvar, y, lik):
        with torch.no_grad():
            ve, g_mu, g_var = lik._expectations(fmu.detach(), fvar.detach(), y.detach())
        ctx.save_for_backward(g_mu, g_var)
        return ve

    @staticmethod
    def backward(ctx, grad_out):
        if torch.is_grad_enabled():
            raise RuntimeError("Likelihood.variational_expectations is differentiable once: its backward uses the derivatives "
                               "computed in the forward and has no second-order support (create_graph=True)")
        g_mu, g_var = ctx.saved_tensors
        return grad_out * g_mu, grad_out * g_var, None, None


def torch_variational_expectations(lik: Likelihood, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor):
    """``(VE, dVE/dmu, dVE/dvar)`` as element-wise torch operations over ``[..., nq]`` temporaries, each of ``fmu``'s shape: the CPU
    route of ``Likelihood.variational_expectations``, and the composition ``mf_lik_*`` is measured against on the device."""
    ok = fvar > 0
    var = torch.where(ok, fvar, torch.ones_like(fvar))
    closed = lik._closed_expectations(fmu, var, y)
    if closed is None:
        x, w, _ = lik._rule(fmu)
        sd = torch.sqrt(2.0 * var)
        l, dl = lik._log_prob_and_grad(fmu[..., None] + sd[..., None] * x, y[..., None])
        closed = torch.sum(w * l, dim=-1), torch.sum(w * dl, dim=-1), torch.sum(w * dl * x, dim=-1) / sd
    nan = torch.full_like(fmu, float("nan"))
    return tuple(torch.where(ok, c, nan) for c in closed)


def torch_predict_log_density(lik: Likelihood, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``log int p(y | f) N(f | fmu, fvar) df`` in torch, ``fmu``'s shape (the CPU route of ``predict_log_density``)."""
    ok = fvar > 0
    var = torch.where(ok, fvar, torch.ones_like(fvar))
    if isinstance(lik, Gaussian):
        total = var + lik.variance
        out = -0.5 * (math.log(2 * math.pi) + torch.log(total)) - 0.5 * (y - fmu) ** 2 / total
    else:
        x, _, logw = lik._rule(fmu)
        l, _ = lik._log_prob_and_grad(fmu[..., None] + torch.sqrt(2.0 * var)[..., None] * x, y[..., None])
        out = torch.logsumexp(l + logw, dim=-1)
    return torch.where(ok, out, torch.full_like(fmu, float("nan")))


class Gaussian(Likelihood):
    """``p(y | f) = N(y | f, variance)``; ``variance`` is a plain float, not trainable."""

    _id = 0

    def __init__(self, variance: float = 1.0, num_gauss_hermite_points: int = 20) -> None:
        super().__init__(num_gauss_hermite_points)
        if not float(variance) > 0.0:
            raise ValueError(f"Gaussian: variance must be positive, got {variance}")
        self.variance = float(variance)

    def _params(self):
        return (self.variance,)

    def _log_prob_and_grad(self, f, y):
        r = y - f
        return -0.5 * (math.log(2 * math.pi) + math.log(self.variance)) - 0.5 * r * r / self.variance, r / self.variance

    def _closed_expectations(self, mu, var, y):
        r = y - mu
        ve = -0.5 * (math.log(2 * math.pi) + math.log(self.variance)) - 0.5 * (r * r + var) / self.variance
        return ve, r / self.variance, torch.full_like(mu, -0.5 / self.variance)

    def predict_mean_and_var(self, fmu, fvar):
        return fmu, fvar + self.variance


class Bernoulli(Likelihood):
    """``p(y = 1 | f) = inv_probit(f)`` (gpflow's probit link with its 1e-3 jitter), ``y in {0, 1}``.  No parameters."""

    _id = 1

    def _log_prob_and_grad(self, f, y):
        p = _inv_probit(f)
        dp = (1.0 - 2.0 * _JITTER) / math.sqrt(2 * math.pi) * torch.exp(-0.5 * f * f)
        return y * torch.log(p) + (1.0 - y) * torch.log1p(-p), dp * (y / p - (1.0 - y) / (1.0 - p))

    def predict_mean_and_var(self, fmu, fvar):
        p = _inv_probit(fmu / torch.sqrt(1.0 + fvar))
        return p, p - p * p


class Poisson(Likelihood):
    """``p(y | f) = Poisson(y | exp(f))`` (exp link, bin size 1).  No parameters."""

    _id = 2

    def _log_prob_and_grad(self, f, y):
        e = torch.exp(f)
        return y * f - e - torch.lgamma(y + 1.0), y - e

    def _closed_expectations(self, mu, var, y):
        e = torch.exp(mu + 0.5 * var)
        return y * mu - e - torch.lgamma(y + 1.0), y - e, -0.5 * e

    def predict_mean_and_var(self, fmu, fvar):
        m = torch.exp(fmu + 0.5 * fvar)
        return m, m + (torch.exp(fvar) - 1.0) * m * m


class StudentT(Likelihood):
    """``p(y | f) = StudentT(y | df, loc = f, scale)``; ``scale`` and ``df`` are plain floats, not trainable.  Not log-concave: a CVI
    step can drive a site precision negative, which the filter reports as a non-positive pivot."""

    _id = 3

    def __init__(self, scale: float = 1.0, df: float = 3.0, num_gauss_hermite_points: int = 20) -> None:
        super().__init__(num_gauss_hermite_points)
        if not float(scale) > 0.0 or not float(df) > 0.0:
            raise ValueError(f"StudentT: scale and df must be positive, got scale={scale}, df={df}")
        self.scale, self.df = float(scale), float(df)
        # the part of log p(y | f) that does not depend on f, for the kernel
        self._const = (math.lgamma(0.5 * (self.df + 1.0)) - math.lgamma(0.5 * self.df) - 0.5 * math.log(self.df * math.pi)
                       - math.log(self.scale))

    def _params(self):
        return (self.scale, self.df, self._const)

    def _log_prob_and_grad(self, f, y):
        r = y - f
        a = self.df * self.scale * self.scale
        return self._const - 0.5 * (self.df + 1.0) * torch.log1p(r * r / a), (self.df + 1.0) * r / (a + r * r)

    def predict_mean_and_var(self, fmu, fvar):
        if not self.df > 2.0:
            raise ValueError("StudentT.predict_mean_and_var: the variance is finite only for df > 2")
        return fmu, fvar + self.scale * self.scale * self.df / (self.df - 2.0)
