"""
Cases, draws and yardsticks of the float32 checks of ``kl_divergence`` / ``marginals`` (tests/test_gpu_kl_float32.py,
tests/test_gpu_kl_from_moments.py, the float32 KL of tests/test_gpu_wave.py).

Rule (the idiom of tests/test_gpu_autograd_ops.py: FP32_LOOP_ERROR, FP32_FACTOR): a float32 kernel is compared with the closed form
in float64 on the float32-representable inputs it saw, and its error may be FP32_FACTOR x the error of the SAME closed form
evaluated in float32 on the CPU - the larger of 8 draws (DEFAULT_SEED + i), because one draw's max-norm rounding error moves by
half its size between seeds.  The yardsticks are committed in tests/helpers/kl_fp32_table.py; scripts/kl_fp32_yardsticks.py
prints that file (CPU only).

Which closed form measures which route (tests/helpers/kl_closed_forms.py):
    sweep      local form, sequential moment recursion        (one lane per series, d <= 9)
    scan, row  local form, Hillis-Steele scan of the moments  (few long chains: the scans in time; row form at 10 <= d <= 15)
    operators  operator form, sequential moments              (d > 32: the composition over the operator kernels)
    walk       operator form; the larger of the sequential and the scanned recursion (wave_kl_walk_kernel walks a chunk
               sequentially and composes the chunks' maps on long chains: its arithmetic lies between the two)
    from_moments      operator form on given (float32-rounded) moments
A yardstick is never taken below the float32 unit roundoff 2^-24: every figure compared is itself rounded to float32 once at the
scale of the metric's denominator, so no float32 evaluation is entitled to less (the CPU's can hit 0 by luck: d = 1, q2 = q1).
"""
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import kl_closed_forms as KC

DEFAULT_SEED = 71892305          # tests/conftest.py
SEEDS = 8
FP32_FACTOR = 4.0                # tests/test_gpu_autograd_ops.py: MFMA accumulation order and the scans' reassociation, nothing else
FP32_FLOOR = 2.0 ** -24

# route -> (d, T, B): the smallest shapes of the float64 tests (tests/test_gpu_gradients.py, tests/test_gpu_wave.py) that reach it
KL_CASES = {
    "sweep": [(1, 2, 2), (3, 40, 2), (9, 33, 1)],
    "scan": [(6, 70, 2), (5, 203, 3), (8, 90, 1), (9, 70, 1)],
    # (12, 9, 2): the float64 test's "tile engine value, re-evaluated backward" shape - the row kernels cover every shape at
    # 10 <= d <= 15 in this build (mf_row_operators_cover), so it runs the row form and its adjoint kernels like the long chains
    "row": [(12, 80, 2), (15, 70, 1), (12, 9, 2)],
    "walk": [(16, 9, 3), (17, 67, 2), (23, 130, 3), (32, 331, 1)],
    "operators": [(40, 20, 2)],
}
ADJOINT_ROUTES = ("sweep", "scan", "row")                      # where mf_ssm_kl_grad_* / mf_kf_loglik_grad_* run the backward
MARGINALS_CASES = [(1, 2, 2), (3, 40, 2), (9, 33, 1), (6, 70, 2), (5, 203, 3), (8, 90, 1), (9, 70, 1), (12, 100, 2), (15, 70, 1)]
FROM_MOMENTS_DIMS = (16, 17, 24, 31, 32)
FROM_MOMENTS_SHAPES = [(1, 1), (3, 2), (2, 9), (70, 5), (2, 130)]           # (B, T)
# the float32 KL of tests/test_gpu_wave.py::test_wave_marginals_and_covariance_blocks: (d, B, T)
WAVE_TEST_CASES = [(d, bsz, t) for d in (16, 27, 32) for bsz, t in [(1, 2), (70, 9), (3, 130), (70, 67), (1, 700), (5, 331)]]

GRAD_NAMES = tuple(f"q{i}.{k}" for i in (1, 2) for k in KC.CHAIN)


@pytest.fixture
def abi_calls(monkeypatch):
    """``(entry point, dtype, return code)`` of every call into the library, in order (``_lib.call`` goes through ``call_rc``): a
    test that can pass without its kernel having run proves nothing about the kernel."""
    seen, real = [], _lib.call_rc

    def spy(base, dtype, *args):
        rc = real(base, dtype, *args)
        seen.append((base, dtype, rc))
        return rc

    monkeypatch.setattr(_lib, "call_rc", spy)
    return seen


def ran(calls, dtype):
    """The entry points of ``dtype`` that returned 0."""
    return [name for name, dt, rc in calls if rc == 0 and dt == dtype]


def random_ssm(rng, batch, t, d):
    from test_gpu_kalman import random_ssm as draw            # the suite's generator (tests/test_gpu_kalman.py), well=True
    return draw(rng, batch, t, d, 1, well=True)


def rounded(x):
    """float32-representable float64 (a dict of arrays or one array)."""
    if isinstance(x, dict):
        return {k: rounded(v) for k, v in x.items()}
    return np.asarray(x).astype(np.float32).astype(np.float64)


def draw_kl(seed, d, t, bsz):
    """Two independent chains and per-series weights, all float32-representable."""
    rng = np.random.default_rng(seed)
    kw1 = rounded(random_ssm(rng, (bsz,), t, d))
    kw2 = rounded(random_ssm(rng, (bsz,), t, d))
    return kw1, kw2, rounded(rng.normal(size=bsz))


def draw_marginals(seed, d, t, bsz):
    rng = np.random.default_rng(seed)
    kw = rounded(random_ssm(rng, (bsz,), t, d))
    return kw, rounded(rng.normal(size=(bsz, t, d))), rounded(rng.normal(size=(bsz, t, d, d)))


def numpy_moments(kw):
    """``(means, covs, cross)`` of a chain by the explicit recursion in numpy float64."""
    tr = lambda x: np.swapaxes(x, -1, -2)                     # noqa: E731
    means, covs = [kw["mu0"]], [kw["chol_p0"] @ tr(kw["chol_p0"])]
    for k in range(kw["a_s"].shape[-3]):
        a, c = kw["a_s"][:, k], kw["chol_q"][:, k]
        means.append((a @ means[-1][..., None])[..., 0] + kw["b_s"][:, k])
        covs.append(a @ covs[-1] @ tr(a) + c @ tr(c))
    means, covs = np.stack(means, axis=1), np.stack(covs, axis=1)
    return means, covs, kw["a_s"] @ covs[:, :-1]


def draw_from_moments(seed, d, bsz, t, round_inputs):
    """Two chains and what mf_ssm_kl_from_moments reads of them: q1's covariances / cross-covariances and mu_2 - mu_1 by the
    explicit float64 recursion (rounded to float32 afterwards with ``round_inputs``: the kernel's inputs ARE these arrays)."""
    rng = np.random.default_rng(seed)
    kw1, kw2 = random_ssm(rng, (bsz,), t, d), random_ssm(rng, (bsz,), t, d)
    if round_inputs:
        kw1, kw2 = rounded(kw1), rounded(kw2)
    means_1, covs_1, cross_1 = numpy_moments(kw1)
    mean_diff = numpy_moments(kw2)[0] - means_1
    if round_inputs:
        covs_1, cross_1, mean_diff = rounded(covs_1), rounded(cross_1), rounded(mean_diff)
    return kw1, kw2, covs_1, cross_1, mean_diff


def from_moments_closed_form(kw1, kw2, covs_1, cross_1, mean_diff, dtype):
    cast = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=dtype)      # noqa: E731
    one = covs_1.shape[1] == 1
    return KC.kl_operator(cast(kw1["chol_p0"]), None if one else cast(kw1["chol_q"]), cast(kw2["chol_p0"]),
                          None if one else cast(kw2["a_s"]), None if one else cast(kw2["chol_q"]), cast(covs_1),
                          None if one else cast(cross_1), cast(mean_diff))


# ---- the closed form of a route, value and gradients ------------------------------------------------------------------------------
def _kl_forms(route):
    """The closed forms (as functions of two chains) whose float32 evaluation measures ``route``."""
    if route == "sweep":
        return [lambda q1, q2: KC.kl_local(q1, q2, scan=False)]
    if route in ("scan", "row"):
        return [lambda q1, q2: KC.kl_local(q1, q2, scan=True)]
    if route == "operators":
        return [lambda q1, q2: KC.kl_operator_from_chains(q1, q2, scan=False)]
    if route == "walk":
        return [lambda q1, q2: KC.kl_operator_from_chains(q1, q2, scan=False),
                lambda q1, q2: KC.kl_operator_from_chains(q1, q2, scan=True)]
    raise KeyError(route)


def kl_closed_form(form, kw1, kw2, weights, dtype, with_grads):
    """``(KL per series, the ten gradients of sum_s w_s KL_s or None)`` of one closed form in ``dtype``."""
    q1, q2 = KC.chain(kw1, dtype, with_grads), KC.chain(kw2, dtype, with_grads)
    value = form(q1, q2)
    grads = None
    if with_grads:
        torch.sum(value * torch.tensor(weights, dtype=dtype)).backward()
        grads = [torch.tril(t.grad) if i % 5 in (1, 4) else t.grad for i, t in enumerate(q1 + q2)]   # the factors are lower triangular
    return value.detach(), grads


@functools.lru_cache(maxsize=None)
def kl_reference(route, d, t, bsz, seed=DEFAULT_SEED):
    """The float64 reference of a case on its float32-representable draw: ``(kw1, kw2, weights, KL, gradients or None,
    KL(q1 || q1))`` - computed once, shared by the tests, never modified."""
    kw1, kw2, weights = draw_kl(seed, d, t, bsz)
    form = _kl_forms(route)[0]                                 # (in float64 every form is the same number)
    value, grads = kl_closed_form(form, kw1, kw2, weights, torch.float64, route in ADJOINT_ROUTES)
    same = kl_closed_form(form, kw1, kw1, weights, torch.float64, False)[0]
    return kw1, kw2, weights, value, grads, same


def kl_yardstick(route, d, t, bsz, seeds=SEEDS):
    """name -> the float32 closed form's error against the float64 one, the larger of ``seeds`` draws (and of the route's forms)."""
    worst = {}
    for i in range(seeds):
        kw1, kw2, weights, want, want_grads, want_same = kl_reference(route, d, t, bsz, DEFAULT_SEED + i)
        for form in _kl_forms(route):
            got, got_grads = kl_closed_form(form, kw1, kw2, weights, torch.float32, want_grads is not None)
            errs = {"kl": KC.value_error(got, want, t, d),
                    "kl_same": KC.value_error(kl_closed_form(form, kw1, kw1, weights, torch.float32, False)[0], want_same, t, d)}
            if want_grads is not None:
                errs.update({name: KC.tensor_error(g, w) for name, g, w in zip(GRAD_NAMES, got_grads, want_grads)})
            for name, e in errs.items():
                worst[name] = max(worst.get(name, FP32_FLOOR), e)
    return worst


MARGINALS_NAMES = ("means", "covs") + tuple("g." + k for k in KC.CHAIN)


def marginals_closed_form(kw, w_means, w_covs, dtype, scan):
    q = KC.chain(kw, dtype, True)
    means, covs = KC.moments(q, scan)
    cast = lambda x: torch.tensor(x, dtype=dtype)              # noqa: E731
    total = 0.0
    if w_means is not None:                                    # (None: that part of the functional is absent - a NULL gradient)
        total = total + torch.sum(cast(w_means) * means)
    if w_covs is not None:
        total = total + torch.sum(cast(w_covs) * covs)
    total.backward()
    grads = [torch.zeros_like(t) if t.grad is None else t.grad for t in q]       # (the means do not depend on the factors)
    return [means.detach(), covs.detach()] + [torch.tril(g) if i in (1, 4) else g for i, g in enumerate(grads)]


def marginals_scans(t):
    """Chains of at least 64 blocks with few series take the scans in time (tests/test_gpu_gradients.py)."""
    return t >= 64


@functools.lru_cache(maxsize=None)
def marginals_reference(d, t, bsz, seed=DEFAULT_SEED):
    kw, w_means, w_covs = draw_marginals(seed, d, t, bsz)
    return kw, w_means, w_covs, marginals_closed_form(kw, w_means, w_covs, torch.float64, False)


def marginals_yardstick(d, t, bsz, seeds=SEEDS):
    worst = {}
    for i in range(seeds):
        kw, w_means, w_covs, want = marginals_reference(d, t, bsz, DEFAULT_SEED + i)
        got = marginals_closed_form(kw, w_means, w_covs, torch.float32, marginals_scans(t))
        for name, g, w in zip(MARGINALS_NAMES, got, want):
            worst[name] = max(worst.get(name, FP32_FLOOR), KC.tensor_error(g, w))
    return worst


# mf_ssm_marginals_grad with g_means = NULL / g_covs = NULL: shapes on both sides of the scans in time, lane and row form (d >= 7)
MARGINALS_NULL_CASES = [(3, 40, 2), (9, 33, 1), (6, 70, 2), (12, 100, 2)]


def marginals_null_yardstick(d, t, bsz, seeds=SEEDS):
    """{"g_means": gradient name -> error, "g_covs": ...}: the functional without the named part."""
    worst = {"g_means": {}, "g_covs": {}}
    for i in range(seeds):
        kw, w_means, w_covs, _ = marginals_reference(d, t, bsz, DEFAULT_SEED + i)
        for absent, wm, wc in (("g_means", None, w_covs), ("g_covs", w_means, None)):
            want = marginals_closed_form(kw, wm, wc, torch.float64, False)[2:]
            got = marginals_closed_form(kw, wm, wc, torch.float32, marginals_scans(t))[2:]
            for name, g, w in zip(MARGINALS_NAMES[2:], got, want):
                worst[absent][name] = max(worst[absent].get(name, FP32_FLOOR), KC.tensor_error(g, w))
    return worst


def from_moments_yardstick(d, bsz, t, seeds=SEEDS):
    worst = FP32_FLOOR
    for i in range(seeds):
        args = draw_from_moments(DEFAULT_SEED + i, d, bsz, t, True)
        want = from_moments_closed_form(*args, torch.float64)
        worst = max(worst, KC.value_error(from_moments_closed_form(*args, torch.float32), want, t, d))
    return worst


def draw_wave_test(seed, d, bsz, t):
    """The two chains of test_wave_marginals_and_covariance_blocks, in the order that test draws them."""
    rng = np.random.default_rng(seed)
    return rounded(random_ssm(rng, (bsz,), t, d)), rounded(random_ssm(rng, (bsz,), t, d))


def wave_test_yardstick(d, bsz, t, seeds=SEEDS):
    worst = FP32_FLOOR
    for i in range(seeds):
        kw1, kw2 = draw_wave_test(DEFAULT_SEED + i, d, bsz, t)
        want = KC.kl_operator_from_chains(KC.chain(kw1), KC.chain(kw2))
        for scan in (False, True):
            got = KC.kl_operator_from_chains(KC.chain(kw1, torch.float32), KC.chain(kw2, torch.float32), scan=scan)
            worst = max(worst, KC.value_error(got, want, t, d))
    return worst
