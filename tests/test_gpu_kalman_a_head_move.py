"""
The moved head carry of A and the register path of H in the streaming log-likelihood kernel (csrc/mf_kf_lds.hpp with
csrc/mf_head_carry.hpp) at d = 6, m = 1 in fp64: a row of A that starts 64, 80, 96 or 112 bytes into a 128-B line takes all of its
part of that line - A[0][0..5] and A[1][0..1] at most - from the tail slots that the previous row's fetch filled; the lane copies
them to the row's head slots inside LDS a step ahead, so rows carry on consecutive steps out of one tail set; H no longer passes
through LDS, every lane loads its step's row straight into registers through a range-checked descriptor.  Which rows carry depends
on BYTE addresses, so everything that moves a phase is varied as in tests/test_gpu_kalman_a_head_carry.py (whose generator is
widened here) and tests/test_gpu_kalman_head_carry.py (whose helpers are used): chain lengths in all residues mod 4, EVERY number
of chunks from one per series to one step per chunk, A, chol Q, H and y on shifted bases, wavefronts that straddle series and that
are not full, the last rows of an allocation.  Per-series values through the C ABI against the numpy oracle, fp64 rtol 1e-10
(fp32 5e-4), as in those files.  Rows 0 and 1 of every A are scaled by their own factors from +-[0.5, 1.5], H is N(0, 1) per row
and y is N(0, 3^2): a stale, zeroed, lost or shifted unit is orders of magnitude outside the tolerance.
"""
import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from test_gpu_kalman import DEV, tt
from test_gpu_kalman_head_carry import KEYS, R_INV, constant, device, lively, per_series, shifted

pytestmark = pytest.mark.gpu


def lively_a(rng, bsz, t):
    """lively() (chol Q's carried entries jump as well: both carries run together) with rows 0 and 1 of each A - the entries that
    units 0 ... 3 hold - scaled per row, and a strongly varying y.  The chain stays well conditioned."""
    kw = lively(rng, bsz, t, 6, 1)
    rows = kw["a_s"].shape[:-2]
    for i in (0, 1):
        factor = rng.uniform(0.5, 1.5, size=rows) * rng.choice([-1.0, 1.0], size=rows)
        kw["a_s"][..., i, :] *= factor[..., None]
    kw["y"] = 3.0 * rng.normal(size=kw["y"].shape)
    return kw


def reference(kw):
    ref = O.kf_log_likelihood(**kw, r_inv=R_INV, per_series=True)
    assert np.all(np.isfinite(ref))
    return ref


def check(dev, ref, t, chunk_counts):
    for chunks in chunk_counts:
        got = per_series(dev, R_INV, chunks) + constant(t, 1, R_INV)
        np.testing.assert_allclose(got, ref, rtol=1e-10, err_msg=f"chunks={chunks}")


@pytest.mark.parametrize("t", [101, 102, 103, 104])
def test_every_residue_of_the_chain_length_and_every_partition(rng, t):
    """T - 1 in all four residues mod 4 (the phase of a series' first row), 70 series (wavefronts straddle series), every explicit
    number of chunks: chunks of 100 steps down to 3, 2 and 1, ragged and idle chunks, chunk starts in every residue mod 4, the
    step that opens a chunk (fetched whole) followed at once by a row that carries."""
    kw = lively_a(rng, 70, t)
    check(device(kw), reference(kw), t, range(1, t))


@pytest.mark.parametrize("shift", [16, 32, 48, 64, 80, 96, 112])
@pytest.mark.parametrize("t", [102, 104])
def test_bases_that_do_not_start_a_line(rng, t, shift):
    """A at 16 ... 112 bytes past a line (bases that are only 16-byte aligned carry at 80 and 112), chol Q and H at other such
    offsets, y at 8, 16 or 24 bytes past a line."""
    kw = lively_a(rng, 70, t)
    ref = reference(kw)
    dev = device(kw)
    dev[2] = shifted(kw["a_s"], torch.float64, shift)
    dev[4] = shifted(kw["chol_q"], torch.float64, (5 * shift + 32) % 128)
    dev[5] = shifted(kw["h"], torch.float64, (3 * shift + 16) % 128)
    dev[6] = shifted(kw["y"], torch.float64, 8 * (1 + (shift // 16) % 3))
    check(dev, ref, t, (1, 2, 4, 7, 33, 64))


@pytest.mark.parametrize("t", [100, 101, 102, 103])
def test_contiguous_slices_of_a_larger_allocation(rng, t):
    """A[1:], cholQ[1:], H[1:], y[1:] of tensors with one series more: the last series ends with its allocation, so the tail
    slots of its last row, the rows of H of its idle steps and its last group of y run past the end and must read as zeros that
    nothing uses."""
    kw = lively_a(rng, 71, t)
    ref = reference({k: v[1:] for k, v in kw.items()})
    full = {k: tt(kw[k]) for k in ("a_s", "chol_q", "h", "y")}
    dev = [tt(kw[k][1:]) for k in KEYS]
    dev[2], dev[4], dev[5], dev[6] = full["a_s"][1:], full["chol_q"][1:], full["h"][1:], full["y"][1:]
    assert dev[2].data_ptr() % 128 == (32 * (t - 1)) % 128 and all(dev[i].is_contiguous() for i in (2, 4, 5, 6))
    check(dev, ref, t, (1, 3, 4, 7, 64))


@pytest.mark.parametrize("t", [102, 103])
def test_h_and_y_end_where_their_range_ends(rng, t):
    """H and y directly followed by NaNs in the same buffer: the last series' row of H and group of y end where the descriptor's
    range ends, and nothing past it - the loads of idle steps, the second half of a y group - may reach a result."""
    kw = lively_a(rng, 70, t)
    ref = reference(kw)
    dev = device(kw)
    for i, key in ((5, "h"), (6, "y")):
        buf = torch.full((kw[key].size + 64,), float("nan"), dtype=torch.float64, device=DEV)
        buf[:kw[key].size].copy_(tt(kw[key]).reshape(-1))
        dev[i] = buf[:kw[key].size].view(kw[key].shape)
    check(dev, ref, t, (1, 3, 4, 7, 50, 64, t - 1))


@pytest.mark.parametrize("bsz,chunks", [(37, 5), (1, 3), (65, 1), (3, 43)])
def test_wavefronts_that_are_not_full(rng, bsz, chunks):
    """B x P = 185, 3, 65, 129: the last wavefront has idle lanes whose rows, H included, get the out-of-range offset."""
    t = 103
    kw = lively_a(rng, bsz, t)
    check(device(kw), reference(kw), t, (chunks,))


def test_long_chunks_and_the_automatic_partition(rng):
    """Chunks far longer than the period of the schedules and of the y groups, and the library's own choice of partition."""
    t = 1000
    kw = lively_a(rng, 130, t)
    check(device(kw), reference(kw), t, (0, 1, 5, 37))


@pytest.mark.parametrize("dtype,m", [(torch.float64, 2), (torch.float32, 1), (torch.float32, 2)])
def test_the_untouched_instantiations_still_agree_with_the_oracle(rng, dtype, m):
    """Two outputs and fp32 keep H in LDS and A without tail slots."""
    bsz, t = 70, 103
    kw = lively(rng, bsz, t, 6, m)
    if dtype == torch.float32:
        kw = {k: v.astype(np.float32).astype(np.float64) for k, v in kw.items()}
    r_inv = np.linalg.inv(0.5 * np.eye(m) + 0.1 * np.ones((m, m)))
    ref = O.kf_log_likelihood(**kw, r_inv=r_inv, per_series=True)
    dev = device(kw, dtype)
    for chunks in (1, 3, 4, 7, 64):
        got = per_series(dev, r_inv, chunks, dtype=dtype) + constant(t, m, r_inv)
        np.testing.assert_allclose(got, ref, rtol=1e-10 if dtype == torch.float64 else 5e-4, err_msg=f"chunks={chunks}")
