"""
Cases, draws and yardsticks of the float32 checks of the backward of ``KalmanFilter.log_likelihood`` at d <= 15
(tests/test_gpu_loglik_grad_float32.py, the float32 tests of tests/test_gpu_grad_streamed.py and
tests/test_gpu_posterior_streamed.py).

The rule is that of tests/helpers/kl_fp32_cases.py, unchanged: a float32 kernel is compared with a float64 reference on the
float32-representable inputs it saw, and its error may be FP32_FACTOR x the error of the SAME arithmetic evaluated in float32 on the
CPU - the larger of SEEDS draws (DEFAULT_SEED + i), never below 2^-24; the metric is kl_closed_forms.tensor_error (max-norm over the
tensor / the reference's max-norm).  The yardsticks are committed in tests/helpers/loglik_fp32_table.py;
scripts/loglik_fp32_yardsticks.py prints that file (CPU only).  Nothing here is derived from a GPU's output.

Which arithmetic measures which kernels:
    LOCAL     mf_kf_loglik_grad_f32 (kf_grad_kernel, row_kf_grad_kernel, the tile route for m > 4): the local forms of Fisher's
              identity (tests/helpers/loglik_grad_closed_forms.py) in float32 against float64, both on the same float32-rounded
              EXACT smoothed moments - with the moments given the step is local in time, nothing of the smoother's conditioning
              enters.  Key (d, m, T, B, per_step).  The larger of two forms of the same numbers: Q^-1 (.) and C^-1 Psi C^-T by
              triangular solves, and by products with an explicitly inverted factor, which is how the kernels do it
              (tri_inv_lower in kf_grad_kernel, row_qinv in row_kf_grad_kernel): an inverse formed first rounds differently.
    STREAMED  mf_kf_loglik_grad_streamed_f32: the kernels' own step functions in float32, lane by lane on the CPU
              (tests/host_sim/post_sim.cpp: mf_grad_host_sim_f32), against torch autograd of the dense log-likelihood in float64.
              Key (d, m, T, B, chunks, per_step).  The rounding depends on the chunk length L, and the backward has no planning
              entry point that reports the L it chose (mf_kf_loglik_plan is the forward's): the yardstick is the larger over
              L in {ceil(T / chunks) if chunks > 0, 16, 64, T}.
    CHAIN     mf_kf_posterior_chain_f32 with a workspace: mf_post_host_sim_f32 against oracle.numpy_oracle.kf_posterior_ssm in
              float64, per output tensor, over the same set of L.  Key (d, m, T, B, chunks, per_step).

Draws: test_gpu_kalman.random_ssm(..., well=True); a shared precision (r r^T + I)^-1; per-step precisions uniform(0.5, 2) as in
tests/test_gpu_grad_streamed.py - for m > 1 that draw is made symmetric and its off-diagonal entries are scaled by 0.2 / (m - 1), so
that every block is diagonally dominant, hence positive definite (m = 1: the draw itself); weights uniform(0.5, 1.5).  Everything
is rounded to float32.
"""
import functools

import numpy as np
import torch

from helpers import kl_closed_forms as KC
from helpers import loglik_grad_closed_forms as LC
from helpers.kl_fp32_cases import DEFAULT_SEED, FP32_FACTOR, FP32_FLOOR, SEEDS, rounded  # noqa: F401  (one rule, one set of numbers)

KEYS = ("mu0", "chol_p0", "a_s", "b_s", "chol_q", "h", "y")
GRAD_NAMES = LC.NAMES                                     # mu0, cholP0, A, b, cholQ, H, y, Omega
STREAMED_NAMES = LC.NAMES[:7] + ("R^-1",)                 # Omega judged as the precision's gradient (precision_gradient below)
CHAIN_NAMES = ("mu0", "cholP0", "A", "b", "cholQ")

# ---- mf_kf_loglik_grad_f32 on given moments: (d, m, T, B), each with a shared and with per-step precisions ----------------------------
# launch edges: 64 lanes per block for the lane kernel (d <= 6), 4 rows per wavefront for the row kernel (7 <= d <= 15)
LOCAL_LANE_CASES = [(1, 1, 1, 3), (2, 2, 5, 1), (3, 4, 13, 5), (6, 1, 64, 1), (6, 3, 9, 2)]
LOCAL_ROW_CASES = [(7, 1, 1, 1), (7, 4, 5, 1), (9, 3, 13, 5), (10, 2, 3, 2), (12, 4, 7, 1), (15, 1, 2, 3), (15, 4, 33, 2)]
LOCAL_NULL_WEIGHT_CASES = [(6, 3, 9, 2), (9, 3, 13, 5)]  # one lane and one row case also with weights = NULL
LOCAL_TILE_CASES = [(3, 6, 12, 2), (9, 7, 20, 1), (12, 5, 9, 2)]        # m > 4 at d <= 15: big_kf_grad_f32
# through KalmanFilter.log_likelihood().backward() on the three-kernel route (T <= 64 or d > 6 keeps it off the streamed one)
API_CASES = [(4, 2, 30, 2), (6, 1, 64, 2), (8, 3, 70, 2), (9, 1, 130, 1), (12, 3, 70, 1), (15, 4, 66, 2)]

# ---- mf_kf_loglik_grad_streamed_f32: (d, m, T, B, chunks, per_step) ------------------------------------------------------------------
STREAMED_CASES = [(6, 1, 120, 3, 0, False), (6, 3, 70, 2, 5, False), (6, 1, 65, 3, 4, True), (4, 2, 90, 2, 3, False),
                  (1, 1, 90, 3, 5, False), (5, 3, 129, 2, 11, False), (2, 2, 90, 3, 4, False)]
STREAMED_FWD_CHUNKS = (None, 0, 9)
# the shapes test_streamed_backward_fp32_other_state_dimensions has always run: (d, m) at T = 90, B = 3 on 4 chunks
STREAMED_OTHER_DIMS = [(1, 1), (2, 2), (3, 1), (4, 3), (5, 1)]
STREAMED_OTHER_CASES = [(d, m, 90, 3, 4, False) for d, m in STREAMED_OTHER_DIMS]
STREAMED_API_CASE = (6, 2, 130, 2, 0, False)
STREAMED_NULL_CASE = (6, 3, 70, 2, 5, False)             # outputs skipped with NULL

# ---- mf_kf_posterior_chain_f32, streamed: tests/test_gpu_posterior_streamed.py::test_streamed_posterior_chain_fp32 -------------------
CHAIN_CASES = [(6, 1, 200, 3, 0, False), (4, 2, 100, 4, 5, False), (2, 1, 64, 5, 3, False)]


def local_keys():
    shapes = LOCAL_LANE_CASES + LOCAL_ROW_CASES + LOCAL_TILE_CASES
    return [s + (per_step,) for s in shapes for per_step in (False, True)] + [s + (False,) for s in API_CASES]


def streamed_keys():
    return STREAMED_CASES + [c for c in STREAMED_OTHER_CASES if c not in STREAMED_CASES] + [STREAMED_API_CASE]


def draw(seed, d, m, t, bsz, per_step):
    """``(chain and emission as a dict, R^-1 [m,m] or [B,T,m,m], weights [B])``, all float32-representable float64."""
    from test_gpu_kalman import random_ssm                   # the suite's generator (tests/test_gpu_kalman.py)
    rng = np.random.default_rng(seed)
    kw = random_ssm(rng, (bsz,), t, d, m, well=True)
    if per_step:
        r_inv = rng.uniform(0.5, 2.0, size=(bsz, t, m, m))
        if m > 1:
            eye = np.eye(m)
            r_inv = r_inv * eye + 0.5 * (r_inv + np.swapaxes(r_inv, -1, -2)) * (1.0 - eye) * (0.2 / (m - 1))
    else:
        r = rng.normal(size=(m, m))
        r_inv = np.linalg.inv(r @ r.T + np.eye(m))
        r_inv = 0.5 * (r_inv + r_inv.T)
    weights = rng.uniform(0.5, 1.5, size=bsz)
    return rounded(kw), rounded(r_inv), rounded(weights)


def errors(names, got, want):
    return {name: KC.tensor_error(g, w) for name, g, w in zip(names, got, want) if torch.as_tensor(w).numel() > 0}


def chunk_lengths(t, chunks):
    return sorted({16, 64, t} | ({-(-t // chunks)} if chunks > 0 else set()))


# ---- LOCAL ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def local_reference(d, m, t, bsz, per_step, seed=DEFAULT_SEED):
    """``(kw, R^-1, weights, exact moments rounded to float32, the eight tensors of the closed forms in float64 with these weights,
    the same with unit weights)`` - computed once, shared by the tests, never modified."""
    kw, r_inv, weights = draw(seed, d, m, t, bsz, per_step)
    moments = tuple(rounded(x) for x in LC.exact_moments(kw, r_inv))
    want = LC.local_gradients_numpy(kw, r_inv, moments, weights, torch.float64)
    return kw, r_inv, weights, moments, want, LC.local_gradients_numpy(kw, r_inv, moments, None, torch.float64)


def local_yardstick(d, m, t, bsz, per_step, seeds=SEEDS):
    worst = {}
    for i in range(seeds):
        kw, r_inv, weights, moments, want, _ = local_reference(d, m, t, bsz, per_step, DEFAULT_SEED + i)
        for explicit_inverse in (False, True):
            got = LC.local_gradients_numpy(kw, r_inv, moments, weights, torch.float32, explicit_inverse)
            for name, e in errors(GRAD_NAMES, got, want).items():
                worst[name] = max(worst.get(name, FP32_FLOOR), e)
    return worst


# ---- STREAMED --------------------------------------------------------------------------------------------------------------------------
def precision_gradient(omega, r_inv, weights, t, per_step):
    """d/dR^-1 from the kernel's Omega: -1/2 Omega from the quadratic forms + 1/2 w R from the log-determinant (the caller's)."""
    if per_step:
        return -0.5 * omega + 0.5 * weights[:, None, None, None] * np.linalg.inv(r_inv)
    return -0.5 * omega.sum(axis=(0, 1)) + 0.5 * weights.sum() * t * np.linalg.inv(r_inv)


def dense_autograd(kw, r_inv, weights, per_step):
    """The seven gradients and the (symmetrised) gradient of R^-1 of sum_s w_s log p(y_s) by torch autograd of the dense
    log-likelihood in float64."""
    from test_post_host_sim import _dense_log_likelihood
    leaves = [torch.tensor(kw[k], requires_grad=True) for k in KEYS]
    ri = torch.tensor(r_inv, requires_grad=True)
    total = 0.0
    for s in range(leaves[0].shape[0]):
        total = total + float(weights[s]) * _dense_log_likelihood(*[v[s] for v in leaves], ri[s] if per_step else ri)
    total.backward()
    g = [v.grad.numpy() for v in leaves]
    g[1], g[4] = np.tril(g[1]), np.tril(g[4])
    gr = ri.grad.numpy()
    return g + [0.5 * (gr + np.swapaxes(gr, -1, -2))]


@functools.lru_cache(maxsize=None)
def streamed_reference(d, m, t, bsz, per_step, seed=DEFAULT_SEED):
    """``(kw, R^-1, weights, the eight float64 references named STREAMED_NAMES)`` (chunks do not enter a reference)."""
    kw, r_inv, weights = draw(seed, d, m, t, bsz, per_step)
    return kw, r_inv, weights, dense_autograd(kw, r_inv, weights, per_step)


def streamed_errors(got, r_inv, weights, t, per_step, want):
    """``got``: the eight tensors of a streamed backward (numpy); Omega enters through the precision's gradient."""
    got = list(got[:7]) + [precision_gradient(got[7], r_inv, weights, t, per_step)]
    return errors(STREAMED_NAMES, got, want)


def streamed_yardstick(d, m, t, bsz, chunks, per_step, seeds=SEEDS):
    from test_post_host_sim import grad_host_sim
    worst = {}
    for i in range(seeds):
        kw, r_inv, weights, want = streamed_reference(d, m, t, bsz, per_step, DEFAULT_SEED + i)
        for length in chunk_lengths(t, chunks):
            rc, got = grad_host_sim(*(kw[k] for k in KEYS), r_inv, per_step, length, weights, dtype=np.float32)
            assert rc == 0
            for name, e in streamed_errors(got, r_inv, weights, t, per_step, want).items():
                worst[name] = max(worst.get(name, FP32_FLOOR), e)
    return worst


# ---- CHAIN -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_reference(d, m, t, bsz, per_step, seed=DEFAULT_SEED):
    from oracle import numpy_oracle as O
    kw, r_inv, _ = draw(seed, d, m, t, bsz, per_step)
    return kw, r_inv, O.kf_posterior_ssm(**kw, r_inv=r_inv)


def chain_yardstick(d, m, t, bsz, chunks, per_step, seeds=SEEDS):
    from test_post_host_sim import post_host_sim
    worst = {}
    for i in range(seeds):
        kw, r_inv, want = chain_reference(d, m, t, bsz, per_step, DEFAULT_SEED + i)
        for length in chunk_lengths(t, chunks):
            rc, got = post_host_sim(*(kw[k] for k in KEYS), r_inv, per_step, length, dtype=np.float32)
            assert rc == 0
            for name, e in errors(CHAIN_NAMES, got, want).items():
                worst[name] = max(worst.get(name, FP32_FLOOR), e)
    return worst


def report(what, errs, yard):
    """Print every figure, then assert: measured error <= FP32_FACTOR x the yardstick.  Returns the worst ratio."""
    for name, e in errs.items():
        print(f"  fp32 {what} {name}: error {e:.3g} (yardstick {yard[name]:.3g}, ratio {e / yard[name]:.2f})")
    worst = max(e / yard[name] for name, e in errs.items())
    print(f"  fp32 {what}: worst ratio {worst:.2f}")
    for name, e in errs.items():
        assert e <= FP32_FACTOR * yard[name], (what, name, e, yard[name])
    return worst
