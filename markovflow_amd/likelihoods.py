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

Power expectation propagation (``PowerExpectationPropagation``) asks for the log of the expected ``alpha``-power density,

    I(mu, var; alpha) = log int p(y | f)^alpha N(f | mu, var) df,    g1 = dI/dmu,    g2 = d2I/dmu2

(``log_expected_density`` / ``grad_log_expected_density``) and for the site update built on it (``pep_site_update``).  Gaussian: closed
form, ``I = -(alpha / 2) log(2 pi s2) + log(2 pi s2 / alpha) / 2 + log N(y; mu, s2 / alpha + var)``.  The others use the rule: with
``v_i = alpha l(f_i) + log w_i`` and ``p_i = softmax_i v_i``,

    I = logsumexp_i v_i,    g1 = sum p_i alpha l'(f_i),    g2 = sum p_i (alpha l''(f_i) + alpha^2 l'(f_i)^2) - g1^2

- again the exact derivatives of the discretised sum (the reference's double tape); a node of weight exactly 0 contributes nothing.
DEVIATION from the reference: its generic ``PEPScalarLikelihood.log_expected_density`` ignores ``alpha`` and its ``PEPGaussian`` returns
``alpha log N(y; mu, s2 + var)``, which is not ``log int p^alpha q``; here the integral is computed.  At ``alpha = 1`` all three agree,
and ``I`` is ``predict_log_density``.

``MultiStageLikelihood`` (``markovflow/likelihoods/mutlistage_likelihood.py``; Seeger et al. 2016, intermittent demand) is the one
likelihood with more than one latent function: ``latent_dim = 3``, tensors ``batch + [N, 3]`` for the latents and ``batch + [N, 1]``
for the observations.  It is a decision tree over the three latents - ``y = 0`` with probability ``sigma(F0)``, else ``y = 1`` with
probability ``sigma(F1)``, else ``y - 2 ~ Poisson(exp(F2))`` - so its expectation is a sum of the Bernoulli and Poisson expectations
above over the latents the point's branch reads; on HIP tensors it is ONE launch of ``mf_lik_multistage_variational_expectations_*``.

The parameters (``variance``, ``scale``, ``df``) are plain Python floats and are NOT trainable.
"""
import ctypes
import math
from typing import Optional, Tuple

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
    latent_dim = 1          # latent functions per observation: models ask before they project (MultiStageLikelihood has 3)

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

    def _log_prob_second_derivative(self, f: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """The second derivative of ``log p(y | f)`` in ``f``, element-wise."""
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

    def _kernel_args(self):
        """What every ``mf_lik_*`` entry point takes behind its sizes: the id, the parameters and the Gauss-Hermite rule."""
        return self._id, self._c_params(), self.num_gauss_hermite_points, self._c_nodes, self._c_weights

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
            _lib.call("mf_lik_predict_log_density", mu.dtype, mu.numel(), *self._kernel_args(), _lib.ptr(mu), _lib.ptr(var),
                      _lib.ptr(obs), _lib.ptr(out), _lib.stream_ptr(mu.device))
            return out[..., 0]

    def _expectations(self, fmu, fvar, y):
        """``(VE, dVE/dmu, dVE/dvar)``, each of ``fmu``'s shape: the kernel on HIP tensors, torch on CPU tensors."""
        if not fmu.is_cuda:
            return torch_variational_expectations(self, fmu, fvar, y)
        mu, var, obs = fmu.contiguous(), fvar.contiguous(), y.contiguous()
        ve, g_mu, g_var = torch.empty_like(mu), torch.empty_like(mu), torch.empty_like(mu)
        _lib.call("mf_lik_variational_expectations", mu.dtype, mu.numel(), *self._kernel_args(), _lib.ptr(mu), _lib.ptr(var),
                  _lib.ptr(obs), _lib.ptr(ve), _lib.ptr(g_mu), _lib.ptr(g_var), _lib.stream_ptr(mu.device))
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
            _lib.call("mf_lik_cvi_site_update", mu.dtype, mu.numel(), *self._kernel_args(), _lib.ptr(mu), _lib.ptr(var),
                      _lib.ptr(obs), lr, _lib.ptr(nat1), _lib.ptr(nat2), None, _lib.stream_ptr(mu.device))
            # the kernel wrote through raw pointers: tell torch, so that whatever keys a cache on (tensor, version) sees the write
            torch.autograd.graph.increment_version(nat1)
            torch.autograd.graph.increment_version(nat2)

    # ---- power expectation propagation ---------------------------------------------------------------------------------------------
    @staticmethod
    def _check_alpha(what: str, alpha) -> float:
        if not 0.0 < float(alpha) <= 1.0:
            raise ValueError(f"{what}: alpha must lie in (0, 1], got {alpha}")
        return float(alpha)

    def _log_expected_density(self, fmu, fvar, y, alpha: float, want=(True, True, True)):
        """``(I, g1, g2)``, each of ``fmu``'s shape or None where not wanted: ONE launch of ``mf_lik_log_expected_density_*`` on HIP
        tensors, ``torch_log_expected_density`` on CPU tensors."""
        if not fmu.is_cuda:
            return tuple(o if w else None for o, w in zip(torch_log_expected_density(self, fmu, fvar, y, alpha), want))
        mu, var, obs = fmu.contiguous(), fvar.contiguous(), y.contiguous()
        outs = [torch.empty_like(mu) if w else None for w in want]
        _lib.call("mf_lik_log_expected_density", mu.dtype, mu.numel(), *self._kernel_args(), alpha, _lib.ptr(mu), _lib.ptr(var),
                  _lib.ptr(obs), *[_lib.ptr(o) for o in outs], _lib.stream_ptr(mu.device))
        return tuple(outs)

    def log_expected_density(self, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
        """``log int p(y | f)^alpha N(f | fmu, fvar) df``, ``batch + [N]`` (not differentiable).  Unlike the reference's, it IS the
        integral of the power (module docstring); at ``alpha = 1`` it is ``predict_log_density``."""
        self._check("log_expected_density", fmu, fvar=fvar, y=y)
        alpha = self._check_alpha("log_expected_density", alpha)
        with torch.no_grad():
            return self._log_expected_density(fmu, fvar, y, alpha, (True, False, False))[0][..., 0]

    def grad_log_expected_density(self, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor, alpha: float = 1.0):
        """``(I, (g1, g2))``: the value, ``batch + [N]``, with its first and second derivative in the mean, ``batch + [N, 1]`` each
        (the shapes of the reference's tape: the derivatives are taken with respect to ``fmu``).  Not differentiable further."""
        self._check("grad_log_expected_density", fmu, fvar=fvar, y=y)
        alpha = self._check_alpha("grad_log_expected_density", alpha)
        with torch.no_grad():
            led, g1, g2 = self._log_expected_density(fmu, fvar, y, alpha)
        return led[..., 0], (g1, g2)

    def pep_site_update(self, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor, alpha: float, learning_rate: float,
                        nat1: torch.Tensor, nat2: torch.Tensor, log_norm: torch.Tensor, update: Optional[torch.Tensor] = None) -> None:
        """One power-EP step on the sites ``exp(nat1 f + nat2 f^2 + log_norm)``, IN PLACE, from the posterior marginals ``fmu``,
        ``fvar`` of ``f`` (pep.py:179-215): cavity ``1 / v_c = 1 / fvar + 2 alpha nat2``, ``mu_c = v_c (fmu / fvar - alpha nat1)``;
        ``I, g1, g2`` at the cavity; ``den = 1 + v_c g2``, ``L2 = g2 / (2 den)``, ``L1 = (g1 - mu_c g2) / den``; normaliser
        ``I + G(mu_c, v_c) - G(fmu, fvar)``, ``G(mu, v) = (log v + mu^2 / v) / 2``; ``pep = (1 - alpha) old + (L1, L2, normaliser)``,
        ``new = (1 - lr) old + lr pep``.  ``nat1``, ``nat2`` and ``log_norm`` hold one element per element of ``fmu`` (any shape) and
        must be contiguous; ``update`` (bool or uint8, one element per point, None = every point) selects the points to update.
        DEVIATION from the reference: a point whose ``fvar``, ``1 / v_c`` or ``den`` is not positive, or whose new values are not
        finite, is SKIPPED - its three numbers stay as they were - where the reference would write NaN into the site.
        HIP tensors: one launch of ``mf_lik_pep_site_update_*``.  Returns None on either device: the cavity, which the kernel can
        write out and ``torch_pep_site_update`` returns, is ``PowerExpectationPropagation.compute_cavity``'s to report."""
        what = f"{type(self).__name__}.pep_site_update"
        self._check("pep_site_update", fmu, fvar=fvar, y=y)
        _lib.same_dtype_device(fmu, what, nat1=nat1, nat2=nat2, log_norm=log_norm)
        if any(t.numel() != fmu.numel() or not t.is_contiguous() for t in (nat1, nat2, log_norm)):
            raise ValueError("pep_site_update: nat1, nat2 and log_norm must be contiguous and hold one element per data point")
        alpha = self._check_alpha("pep_site_update", alpha)
        if not 0.0 <= float(learning_rate) <= 1.0:
            raise ValueError(f"pep_site_update: learning_rate must lie in [0, 1], got {learning_rate}")
        lr = float(learning_rate)
        if update is not None:
            if update.dtype not in (torch.bool, torch.uint8) or update.numel() != fmu.numel() or update.device != fmu.device:
                raise ValueError("pep_site_update: update must be a bool or uint8 tensor on the data's device with one element per "
                                 "data point")
            update = update.contiguous().view(torch.uint8)
        with torch.no_grad():
            if not fmu.is_cuda:
                torch_pep_site_update(self, fmu, fvar, y, alpha, lr, nat1, nat2, log_norm, update)
                return
            mu, var, obs = fmu.contiguous(), fvar.contiguous(), y.contiguous()
            _lib.call("mf_lik_pep_site_update", mu.dtype, mu.numel(), *self._kernel_args(), alpha, lr, _lib.ptr(mu), _lib.ptr(var),
                      _lib.ptr(obs), _lib.ptr(update), _lib.ptr(nat1), _lib.ptr(nat2), _lib.ptr(log_norm), None, None,
                      _lib.stream_ptr(mu.device))
            # the kernel wrote through raw pointers: tell torch (as cvi_site_update does)
            for t in (nat1, nat2, log_norm):
                torch.autograd.graph.increment_version(t)


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


def torch_log_expected_density(lik: Likelihood, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor, alpha: float = 1.0):
    """``(I, dI/dmu, d2I/dmu2)`` of ``I = log int p(y | f)^alpha N(f | fmu, fvar) df`` as element-wise torch operations over
    ``[..., nq]`` temporaries, each of ``fmu``'s shape: the CPU route of ``Likelihood.log_expected_density``, and (inside
    ``torch_pep_site_update``) the composition ``mf_lik_pep_site_update_*`` is measured against on the device."""
    ok = fvar > 0
    var = torch.where(ok, fvar, torch.ones_like(fvar))
    if isinstance(lik, Gaussian):
        sa = lik.variance / alpha
        iv = 1.0 / (sa + var)
        r = y - fmu
        led = (-0.5 * alpha * math.log(2 * math.pi * lik.variance) + 0.5 * (math.log(sa) + torch.log(iv)) - 0.5 * r * r * iv)
        outs = led, r * iv, -iv
    else:
        x, _, logw = lik._rule(fmu)
        f, yy = fmu[..., None] + torch.sqrt(2.0 * var)[..., None] * x, y[..., None]
        l, dl = lik._log_prob_and_grad(f, yy)
        a = alpha * dl
        b = alpha * lik._log_prob_second_derivative(f, yy) + a * a
        v = alpha * l + logw
        led = torch.logsumexp(v, dim=-1)
        pr = torch.exp(v - led[..., None])
        zero = torch.zeros_like(pr)
        g1 = torch.sum(torch.where(pr > 0, pr * a, zero), dim=-1)       # (a node of weight exactly 0 may carry an infinite l')
        outs = led, g1, torch.sum(torch.where(pr > 0, pr * b, zero), dim=-1) - g1 * g1
    nan = torch.full_like(fmu, float("nan"))
    return tuple(torch.where(ok, o, nan) for o in outs)


def torch_pep_site_update(lik: Likelihood, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor, alpha: float, learning_rate: float,
                          nat1: torch.Tensor, nat2: torch.Tensor, log_norm: torch.Tensor, update: Optional[torch.Tensor] = None):
    """``Likelihood.pep_site_update`` as a composition of element-wise torch operations, in place on ``nat1``, ``nat2``, ``log_norm``
    (one element per element of ``fmu``): its CPU route, and what ``mf_lik_pep_site_update_*`` fuses and is timed against.  Unlike
    the method, which returns None, it returns the cavity ``(mu_c, v_c)``, NaN where it does not exist - the counterpart of the
    kernel's optional ``cav_mu`` / ``cav_var`` outputs, for the tests that compare the two."""
    n1, n2, ln = (t.reshape(fmu.shape) for t in (nat1, nat2, log_norm))
    prec = 1.0 / fvar + 2.0 * alpha * n2
    cavity = (fvar > 0) & (prec > 0)
    nan, one = torch.full_like(fmu, float("nan")), torch.ones_like(fmu)
    vc = torch.where(cavity, 1.0 / prec, one)
    mc = torch.where(cavity, vc * (fmu / fvar - alpha * n1), one)
    led, g1, g2 = torch_log_expected_density(lik, mc, vc, y, alpha)
    if isinstance(lik, Gaussian):                  # closed form, free of the cancellation in 1 + v_c g2 (as the kernel)
        den = (lik.variance / alpha) / (lik.variance / alpha + vc)
    else:
        den = 1.0 + vc * g2
    l2 = 0.5 * g2 / den
    l1 = (g1 - mc * g2) / den
    norm = led + 0.5 * (torch.log(vc) + mc * mc / vc) - 0.5 * (torch.log(fvar) + fmu * fmu / fvar)
    lr = learning_rate
    new = [(1.0 - lr) * old + lr * ((1.0 - alpha) * old + step) for old, step in ((n1, l1), (n2, l2), (ln, norm))]
    ok = cavity & (den > 0) & torch.isfinite(new[0]) & torch.isfinite(new[1]) & torch.isfinite(new[2])
    if update is not None:
        ok = ok & (update.reshape(fmu.shape) != 0)
    for t, old, fresh in zip((nat1, nat2, log_norm), (n1, n2, ln), new):
        t.copy_(torch.where(ok, fresh, old).reshape(t.shape))
    return torch.where(cavity, mc, nan), torch.where(cavity, vc, nan)


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

    def _log_prob_second_derivative(self, f, y):
        return torch.full_like(f, -1.0 / self.variance)

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

    def _log_prob_second_derivative(self, f, y):
        # p'' = -f p':  l'' = -f l' - p'^2 (y / p^2 + (1 - y) / (1 - p)^2)
        p = _inv_probit(f)
        dp = (1.0 - 2.0 * _JITTER) / math.sqrt(2 * math.pi) * torch.exp(-0.5 * f * f)
        return -f * dp * (y / p - (1.0 - y) / (1.0 - p)) - dp * dp * (y / (p * p) + (1.0 - y) / ((1.0 - p) * (1.0 - p)))

    def predict_mean_and_var(self, fmu, fvar):
        p = _inv_probit(fmu / torch.sqrt(1.0 + fvar))
        return p, p - p * p


class Poisson(Likelihood):
    """``p(y | f) = Poisson(y | exp(f))`` (exp link, bin size 1).  No parameters."""

    _id = 2

    def _log_prob_and_grad(self, f, y):
        e = torch.exp(f)
        return y * f - e - torch.lgamma(y + 1.0), y - e

    def _log_prob_second_derivative(self, f, y):
        return -torch.exp(f) + 0.0 * y

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

    def _log_prob_second_derivative(self, f, y):
        r2 = (y - f) ** 2
        a = self.df * self.scale * self.scale
        return -(self.df + 1.0) * (a - r2) / ((a + r2) * (a + r2))

    def predict_mean_and_var(self, fmu, fvar):
        if not self.df > 2.0:
            raise ValueError("StudentT.predict_mean_and_var: the variance is finite only for df > 2")
        return fmu, fvar + self.scale * self.scale * self.df / (self.df - 2.0)


class MultiStageLikelihood(Likelihood):
    """The multi-stage likelihood for intermittent, bursty counts (``markovflow/likelihoods/mutlistage_likelihood.py``; Seeger,
    Salinas and Flunkert 2016): three latent functions ``F = [F0, F1, F2]`` and one observation column.  With ``sigma`` the probit
    link of ``Bernoulli`` (its 1e-3 jitter included) and the exp link with bin size 1 of ``Poisson``,

        log p(y | F) = [y == 0]  log sigma(F0)
                     + [y == 1] (log(1 - sigma(F0)) + log sigma(F1))
                     + [y >= 2] (log(1 - sigma(F0)) + log(1 - sigma(F1)) + log Poisson(y - 2 | exp(F2)))

    An observation that is none of ``0``, ``1``, ``>= 2`` (0.5, a negative number, NaN) contributes exactly 0, as the reference's
    three masks do; the comparisons are exact floating-point comparisons.  A latent that the point's branch does not read has
    derivative 0 and its variance is not examined; one that it reads with ``fvar <= 0`` or NaN makes the point's value and that
    latent's derivatives NaN.  The links are not arguments: the kernels hard-code them.  No parameters."""

    _id = 4
    latent_dim = 3

    def __init__(self, num_gauss_hermite_points: int = 20) -> None:
        super().__init__(num_gauss_hermite_points)
        self._bernoulli = Bernoulli(num_gauss_hermite_points)
        self._poisson = Poisson(num_gauss_hermite_points)

    def _check(self, what: str, fmu: torch.Tensor, y: torch.Tensor = None, **others: torch.Tensor):
        if fmu.dim() < 2 or fmu.shape[-1] != self.latent_dim:
            raise ValueError(f"{type(self).__name__}.{what}: the latents must have shape batch + [N, {self.latent_dim}], got "
                             f"{tuple(fmu.shape)}")
        for name, t in others.items():
            if tuple(t.shape) != tuple(fmu.shape):
                raise ValueError(f"{type(self).__name__}.{what}: {name} has shape {tuple(t.shape)}, expected {tuple(fmu.shape)}")
        if y is not None and tuple(y.shape) != tuple(fmu.shape[:-1]) + (1,):
            raise ValueError(f"{type(self).__name__}.{what}: y has shape {tuple(y.shape)}, expected {tuple(fmu.shape[:-1]) + (1,)}")
        if fmu.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {fmu.dtype}")
        _lib.same_dtype_device(fmu, f"{type(self).__name__}.{what}", y=y, **others)

    def log_prob(self, f: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``log p(y | F)``, ``batch + [N, 3]``, ``batch + [N, 1] -> batch + [N]`` (element-wise torch on either device)."""
        self._check("log_prob", f, y=y)
        obs = y[..., 0]
        is0, is1, is2 = obs == 0, obs == 1, obs >= 2
        zero, one = torch.zeros_like(obs), torch.ones_like(obs)
        yes0, no0 = (self._bernoulli._log_prob_and_grad(f[..., 0], t)[0] for t in (one, zero))
        yes1, no1 = (self._bernoulli._log_prob_and_grad(f[..., 1], t)[0] for t in (one, zero))
        count = self._poisson._log_prob_and_grad(f[..., 2], torch.where(is2, obs - 2.0, zero))[0]
        return torch.where(is0, yes0, zero) + torch.where(is1, no0 + yes1, zero) + torch.where(is2, no0 + no1 + count, zero)

    def variational_expectations(self, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``E_{prod_l N(F_l | fmu_l, fvar_l)} log p(y | F)``, ``batch + [N]``, from ``fmu``, ``fvar`` ``batch + [N, 3]`` and ``y``
        ``batch + [N, 1]``.  Differentiable ONCE in ``fmu`` and ``fvar``: the six derivatives per point are computed beside the value
        and saved (no second-order support)."""
        self._check("variational_expectations", fmu, y=y, fvar=fvar)
        return _MultiStageVariationalExpectations.apply(fmu, fvar, y, self)

    def _expectations(self, fmu, fvar, y):
        """``(VE [.., N], dVE/dmu [.., N, 3], dVE/dvar [.., N, 3])``: the kernel on HIP tensors, torch on CPU tensors."""
        if not fmu.is_cuda:
            return torch_multistage_variational_expectations(self, fmu, fvar, y)
        mu, var, obs = fmu.contiguous(), fvar.contiguous(), y.contiguous()
        ve, g_mu, g_var = torch.empty_like(obs[..., 0]), torch.empty_like(mu), torch.empty_like(mu)
        _lib.call("mf_lik_multistage_variational_expectations", mu.dtype, obs.numel(), self.num_gauss_hermite_points, self._c_nodes,
                  self._c_weights, _lib.ptr(mu), _lib.ptr(var), _lib.ptr(obs), _lib.ptr(ve), _lib.ptr(g_mu), _lib.ptr(g_var),
                  _lib.stream_ptr(mu.device))
        return ve, g_mu, g_var

    def predict_log_density(self, fmu, fvar, y):
        """Not available, as in the reference (mutlistage_likelihood.py:144-145)."""
        raise NotImplementedError("MultiStageLikelihood has no predictive density (the reference's raises too)")

    def predict_mean_and_var(self, fmu, fvar):
        """Not available, as in the reference (mutlistage_likelihood.py:147-148)."""
        raise NotImplementedError("MultiStageLikelihood has no predictive mean and variance (the reference's raises too)")

    def _one_latent_only(self, *args, **kwargs):
        raise NotImplementedError("MultiStageLikelihood has three latent functions: the site updates and the power-EP densities "
                                  "are written for one; use SparseVariationalGaussianProcess")

    cvi_site_update = log_expected_density = grad_log_expected_density = pep_site_update = _one_latent_only

    def sample_y(self, F_samples: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """Observations drawn from ``p(y | F)``, ``batch + [3] -> batch + [1]`` (mutlistage_likelihood.py:150-179): ``eta0 ~
        Bernoulli(sigma(F0))``; ``eta0 = 1`` gives 0, else ``eta1 ~ Bernoulli(sigma(F1)) = 1`` gives 1, else ``Poisson(exp(F2)) + 2``."""
        if F_samples.dim() < 1 or F_samples.shape[-1] != self.latent_dim:
            raise ValueError(f"MultiStageLikelihood.sample_y: F_samples must have shape batch + [3], got {tuple(F_samples.shape)}")
        if F_samples.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {F_samples.dtype}")
        eta0 = torch.bernoulli(_inv_probit(F_samples[..., 0]), generator=generator)
        eta1 = torch.bernoulli(_inv_probit(F_samples[..., 1]), generator=generator)
        count = torch.poisson(torch.exp(F_samples[..., 2]), generator=generator)
        return torch.where(eta0 == 1, torch.zeros_like(eta0), torch.where(eta1 == 1, torch.ones_like(eta0), count + 2.0))[..., None]


class _MultiStageVariationalExpectations(torch.autograd.Function):
    """Value ``batch + [N]`` with the ``2 latent_dim`` derivatives per point computed in the same pass and saved for the backward
    (``MultiStageLikelihood``, ``HeteroscedasticGaussian``)."""

    @staticmethod
    def forward(ctx, fmu, fvar, y, lik):
        with torch.no_grad():
            ve, g_mu, g_var = lik._expectations(fmu.detach(), fvar.detach(), y.detach())
        ctx.save_for_backward(g_mu, g_var)
        ctx.who = type(lik).__name__
        return ve

    @staticmethod
    def backward(ctx, grad_out):
        if torch.is_grad_enabled():
            raise RuntimeError(f"{ctx.who}.variational_expectations is differentiable once: its backward uses the "
                               "derivatives computed in the forward and has no second-order support (create_graph=True)")
        g_mu, g_var = ctx.saved_tensors
        return grad_out[..., None] * g_mu, grad_out[..., None] * g_var, None, None


def torch_multistage_variational_expectations(lik: MultiStageLikelihood, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor):
    """``(VE [.., N], dVE/dmu [.., N, 3], dVE/dvar [.., N, 3])`` of the multi-stage likelihood from ``torch_variational_expectations``
    of its Bernoulli and Poisson stages: the CPU route of ``MultiStageLikelihood.variational_expectations``, and the composition
    ``mf_lik_multistage_variational_expectations_*`` is measured against on the device.  The value is summed over the latents in
    ascending order, as the kernel sums it; a latent that the branch does not read is evaluated at variance 1 and masked out."""
    obs = y[..., 0]
    is0, is1, is2 = obs == 0, obs == 1, obs >= 2
    read = torch.stack([is0 | is1 | is2, is1 | is2, is2], dim=-1)
    var = torch.where(read, fvar, torch.ones_like(fvar))
    mu = torch.where(read, fmu, torch.zeros_like(fmu))
    target = torch.stack([is0, is1], dim=-1).to(fmu.dtype)                         # sigma(F0) for y = 0, sigma(F1) for y = 1
    stage = torch_variational_expectations(lik._bernoulli, mu[..., :2], var[..., :2], target)
    count = torch_variational_expectations(lik._poisson, mu[..., 2:], var[..., 2:], torch.where(is2, obs - 2.0, torch.zeros_like(obs))[..., None])
    ve, g_mu, g_var = (torch.where(read, torch.cat([s, c], dim=-1), torch.zeros_like(fmu)) for s, c in zip(stage, count))
    return (ve[..., 0] + ve[..., 1]) + ve[..., 2], g_mu, g_var


class HeteroscedasticGaussian(Likelihood):
    """A Gaussian whose mean AND log-variance are latent functions (the second half of the reference's stacked-kernels notebook):
    ``latent_dim = 2``, ``F = [F0, F1]``, ``y ~ N(F0, exp(F1))``; tensors ``batch + [N, 2]`` for the latents and ``batch + [N, 1]`` for
    the observations.  Everything is in closed form: with ``E = exp(-m1 + v1 / 2) ((m0 - y)^2 + v0)``,

        E_q log p(y | F) = -(log 2 pi + m1 + E) / 2

    with the derivatives ``-exp(-m1 + v1 / 2) (m0 - y)``, ``-exp(-m1 + v1 / 2) / 2`` (latent 0: mean, variance) and ``-(1 - E) / 2``,
    ``-E / 4`` (latent 1).  Both latents are read at every point: a variance that is ``<= 0`` or NaN makes the point's value and all
    four derivatives NaN.  No parameters; the quadrature rule is not used.  On stacked chains (``IndependentMultiOutputStack``) the
    SVGP data term of this likelihood is ONE call of ``mf_lik_stack_expectations_*``."""

    _id = 5
    latent_dim = 2

    _check = MultiStageLikelihood._check

    def log_prob(self, f: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``log N(y | F0, exp F1)``, ``batch + [N, 2]``, ``batch + [N, 1] -> batch + [N]``."""
        self._check("log_prob", f, y=y)
        r = y[..., 0] - f[..., 0]
        return -0.5 * (math.log(2.0 * math.pi) + f[..., 1] + r * r * torch.exp(-f[..., 1]))

    def variational_expectations(self, fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``E_{N(F0 | m0, v0) N(F1 | m1, v1)} log p(y | F)``, ``batch + [N]``.  Differentiable ONCE in ``fmu`` and ``fvar``: the four
        derivatives per point are computed beside the value and saved (no second-order support)."""
        self._check("variational_expectations", fmu, y=y, fvar=fvar)
        return _MultiStageVariationalExpectations.apply(fmu, fvar, y, self)

    def _expectations(self, fmu, fvar, y):
        """``(VE [.., N], dVE/dmu [.., N, 2], dVE/dvar [.., N, 2])`` in closed form: element-wise torch on either device."""
        m0, m1, v0, v1 = fmu[..., 0], fmu[..., 1], fvar[..., 0], fvar[..., 1]
        r = m0 - y[..., 0]
        e = torch.exp(0.5 * v1 - m1)
        big = e * (r * r + v0)
        ve = -0.5 * (math.log(2.0 * math.pi) + m1 + big)
        g_mu = torch.stack([-e * r, -0.5 * (1.0 - big)], dim=-1)
        g_var = torch.stack([-0.5 * e, -0.25 * big], dim=-1)
        bad = ~((v0 > 0) & (v1 > 0))
        nan = float("nan")
        return ve.masked_fill(bad, nan), g_mu.masked_fill(bad[..., None], nan), g_var.masked_fill(bad[..., None], nan)

    def predict_mean_and_var(self, fmu: torch.Tensor, fvar: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(m0, v0 + E exp F1) = (m0, v0 + exp(m1 + v1 / 2))``, ``batch + [N, 1]`` each."""
        self._check("predict_mean_and_var", fmu, fvar=fvar)
        return fmu[..., :1], fvar[..., :1] + torch.exp(fmu[..., 1:] + 0.5 * fvar[..., 1:])

    def predict_log_density(self, fmu, fvar, y):
        """Not available: the predictive density of a Gaussian with a log-normal variance has no closed form."""
        raise NotImplementedError("HeteroscedasticGaussian has no predictive density in closed form")

    def _one_latent_only(self, *args, **kwargs):
        raise NotImplementedError("HeteroscedasticGaussian has two latent functions: the site updates and the power-EP densities "
                                  "are written for one; use SparseVariationalGaussianProcess")

    cvi_site_update = log_expected_density = grad_log_expected_density = pep_site_update = _one_latent_only

    def sample_y(self, F_samples: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """Observations drawn from ``p(y | F)``, ``batch + [2] -> batch + [1]``."""
        if F_samples.dim() < 1 or F_samples.shape[-1] != self.latent_dim:
            raise ValueError(f"HeteroscedasticGaussian.sample_y: F_samples must have shape batch + [2], got {tuple(F_samples.shape)}")
        if F_samples.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {F_samples.dtype}")
        noise = torch.randn(F_samples.shape[:-1], dtype=F_samples.dtype, device=F_samples.device, generator=generator)
        return (F_samples[..., 0] + torch.exp(0.5 * F_samples[..., 1]) * noise)[..., None]


def torch_heteroscedastic_variational_expectations(fmu: torch.Tensor, fvar: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The statement of ``HeteroscedasticGaussian.variational_expectations`` in plain torch operations, ``batch + [N]``,
    differentiable by autograd to any order (no domain rule): what the closed-form derivatives are checked against."""
    r = fmu[..., 0] - y[..., 0]
    big = torch.exp(0.5 * fvar[..., 1] - fmu[..., 1]) * (r * r + fvar[..., 0])
    return -0.5 * (math.log(2.0 * math.pi) + fmu[..., 1] + big)
