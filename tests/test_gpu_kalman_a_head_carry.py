"""
The head carry of A and the register path of y in the streaming log-likelihood kernel (csrc/mf_kf_lds.hpp with
csrc/mf_head_carry.hpp) at d = 6, m = 1 in fp64: a row of A that starts 96 (112) bytes into a 128-B line takes A[0][0..3]
(A[0][0..1]) from the tail slots that the previous row's fetch filled, its own fetch leaves that line alone, and a masked-out slot
keeps its data across the next fetch; y no longer passes through LDS, every lane loads its chunk's values in groups straight into
registers.  Which rows carry depends on BYTE addresses, and a chunk's first y is only 8-byte aligned, so everything that moves a
phase is varied as in tests/test_gpu_kalman_head_carry.py (whose helpers are used here): chain lengths in all residues mod 4,
partitions from one chunk to one step per chunk, A, chol Q and y on shifted bases, wavefronts that straddle series, the last row
and the last y group of an allocation.  Per-series values through the C ABI against the numpy oracle, fp64 rtol 1e-10.  Row 0 of
every A is scaled by its own factor from +-[0.5, 1.5] and y is N(0, 3^2): a stale, zeroed or shifted carry or y is orders of
magnitude outside the tolerance.
"""
import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from test_gpu_kalman import tt
from test_gpu_kalman_head_carry import KEYS, R_INV, constant, device, lively, per_series, shifted

pytestmark = pytest.mark.gpu


def lively_a(rng, bsz, t):
    """lively() (chol Q's carried entries jump as well: both carries run together) with row 0 of each A scaled per row and a
    strongly varying y.  The chain stays well conditioned: |A| entries ~ 0.2 x 1.5 at most."""
    kw = lively(rng, bsz, t, 6, 1)
    rows = kw["a_s"].shape[:-2]
    factor = rng.uniform(0.5, 1.5, size=rows) * rng.choice([-1.0, 1.0], size=rows)
    kw["a_s"][..., 0, :] *= factor[..., None]
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
    """T - 1 in all four residues mod 4 (the phase of a series' first row), 70 series (wavefronts straddle series); ragged and
    idle chunks, chunks of a single step, chunk starts in every residue mod 4 (y groups 8- but not 16- or 32-byte aligned)."""
    kw = lively_a(rng, 70, t)
    check(device(kw), reference(kw), t, (1, 2, 3, 4, 7, 13, 50, 64, t - 1))


@pytest.mark.parametrize("shift", [16, 32, 48, 64, 80, 96, 112])
@pytest.mark.parametrize("t", [102, 104])
def test_bases_that_do_not_start_a_line(rng, t, shift):
    """A at 16 ... 112 bytes past a line, chol Q at another such offset (a different one for every shift of A), y at 8, 16 or
    24 bytes past a line."""
    kw = lively_a(rng, 70, t)
    ref = reference(kw)
    dev = device(kw)
    dev[2] = shifted(kw["a_s"], torch.float64, shift)
    dev[4] = shifted(kw["chol_q"], torch.float64, (5 * shift + 32) % 128)
    dev[6] = shifted(kw["y"], torch.float64, 8 * (1 + (shift // 16) % 3))
    check(dev, ref, t, (1, 4, 7, 64))


@pytest.mark.parametrize("t", [100, 101, 102, 103])
def test_contiguous_slices_of_a_larger_allocation(rng, t):
    """A[1:], cholQ[1:], y[1:] of tensors with one series more: the last series ends with its allocation, so the tail slots of its
    last row and its last group of y run past the end and must read as zeros that nothing uses."""
    kw = lively_a(rng, 71, t)
    ref = reference({k: v[1:] for k, v in kw.items()})
    full_a, full_c, full_y = tt(kw["a_s"]), tt(kw["chol_q"]), tt(kw["y"])
    dev = [tt(kw[k][1:]) for k in KEYS]
    dev[2], dev[4], dev[6] = full_a[1:], full_c[1:], full_y[1:]
    assert dev[2].data_ptr() % 128 == (32 * (t - 1)) % 128 and dev[2].is_contiguous() and dev[6].is_contiguous()
    check(dev, ref, t, (1, 3, 4, 7, 64))


def test_long_chunks_and_the_automatic_partition(rng):
    """Chunks far longer than the period of the schedules and of the y groups, and the library's own choice of partition."""
    t = 1000
    kw = lively_a(rng, 130, t)
    check(device(kw), reference(kw), t, (0, 1, 5, 37))
