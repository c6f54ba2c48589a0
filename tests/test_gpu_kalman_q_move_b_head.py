"""
The moved head carry of chol Q and b in the streaming log-likelihood kernel (csrc/mf_kf_lds.hpp with csrc/mf_head_carry.hpp) at
d = 6, m = 1 in fp64: chol Q's carried units - C[0][0], C[1][0], C[1][1] of a row that starts 32 ... 112 bytes into a 128-B line -
no longer wait in registers, the lane copies them from the tail slots to the row's head slots inside LDS a step ahead, as it does
for A, and the fetch of that row masks the head slots out; b's row image has a tail slot of its own, and a row of b that starts
112 bytes into a line takes b[0], b[1] from the fetch of the row before.  Which rows carry depends on BYTE addresses, so A, chol Q
and b each start 0, 16, ... 112 bytes into a 128-B aligned allocation, independently of each other, for series counts 1, 3 and 65
(idle lanes, wavefronts that straddle series), chains of 9, 67 and 319 blocks and partitions into chunks of 1, 2 and 3 steps
(the first, whole fetch of a chunk followed at once by carrying rows), of more than 8 steps (b's schedule has a period of 8) and
one chunk per series (the kernel variant without the spike).  Per-series values through the C ABI against the numpy oracle, fp64
rtol 1e-10 (fp32 5e-4): reference, helpers and tolerances of tests/test_gpu_kalman_a_head_move.py.  The carried entries of chol Q
and A jump from row to row as there, and b[0], b[1] are N(0, 2^2) per row: a stale, zeroed, lost or shifted unit is orders of
magnitude outside the tolerance.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from test_gpu_kalman_a_head_move import lively_a, reference
from test_gpu_kalman_head_carry import R_INV, constant, device, lively, per_series, shifted

pytestmark = pytest.mark.gpu


def chunk_counts(t):
    """Partitions of the t - 1 transitions: chunks of 1, 2 and 3 steps, of 10 steps where the chain has them, one chunk per series."""
    n = t - 1
    counts = {n, -(-n // 2), -(-n // 3), 1}
    if n > 10:
        counts.add(-(-n // 10))
    return sorted(counts)


@functools.lru_cache(maxsize=None)
def problem(bsz, t):
    """The chain and its reference, computed once per shape and left unchanged."""
    rng = np.random.default_rng(1000 * bsz + t)
    kw = lively_a(rng, bsz, t)
    kw["b_s"][..., :2] = 2.0 * rng.normal(size=kw["b_s"].shape[:-1] + (2,))
    return kw, reference(kw)


@pytest.mark.parametrize("k", range(8))
@pytest.mark.parametrize("t", [9, 67, 157 * 2 + 5])
@pytest.mark.parametrize("bsz", [1, 3, 65])
def test_shifted_bases_and_every_partition(bsz, t, k):
    """A 16 k bytes past a line, chol Q 16 (3 k + 1), b 16 (5 k + 2) (mod 128): each tensor meets every phase, in eight different
    combinations; chunks = 1 runs the kernel without the spike, every other count the one with it."""
    kw, ref = problem(bsz, t)
    dev = device(kw)
    dev[2] = shifted(kw["a_s"], torch.float64, (16 * k) % 128)
    dev[4] = shifted(kw["chol_q"], torch.float64, (16 * (3 * k + 1)) % 128)
    dev[3] = shifted(kw["b_s"], torch.float64, (16 * (5 * k + 2)) % 128)
    for chunks in chunk_counts(t):
        got = per_series(dev, R_INV, chunks) + constant(t, 1, R_INV)
        np.testing.assert_allclose(got, ref, rtol=1e-10, err_msg=f"chunks={chunks}")


@pytest.mark.parametrize("dtype,m", [(torch.float64, 2), (torch.float32, 1)])
def test_the_untouched_instantiations_still_agree_with_the_oracle(rng, dtype, m):
    """Two outputs and fp32 keep chol Q's register carry and b without a tail slot."""
    bsz, t = 3, 67
    kw = lively(rng, bsz, t, 6, m)
    if dtype == torch.float32:
        kw = {k: v.astype(np.float32).astype(np.float64) for k, v in kw.items()}
    r_inv = np.linalg.inv(0.5 * np.eye(m) + 0.1 * np.ones((m, m)))
    ref = O.kf_log_likelihood(**kw, r_inv=r_inv, per_series=True)
    dev = device(kw, dtype)
    dev[3] = shifted(kw["b_s"], dtype, 112)
    for chunks in chunk_counts(t):
        got = per_series(dev, r_inv, chunks, dtype=dtype) + constant(t, m, r_inv)
        np.testing.assert_allclose(got, ref, rtol=1e-10 if dtype == torch.float64 else 5e-4, err_msg=f"chunks={chunks}")
