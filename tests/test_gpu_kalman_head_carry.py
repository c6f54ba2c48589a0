"""
The head carry of the streaming log-likelihood kernel (csrc/mf_kf_lds.hpp with csrc/mf_head_carry.hpp): at d = 6, m = 1 in fp64
the fetch of a chol Q row brings the next row's C[0][0], C[1][0], C[1][1] along whenever they sit in a 128-B line the two rows
share, the lane keeps them in registers across the step, and the next row's fetch leaves that line alone.  Which rows carry
depends on BYTE addresses (base of the tensor, series, chunk start, step), so everything that moves the phase is varied here:
chain lengths in all residues mod 4, time partitions from one chunk to one step per chunk, bases shifted by 16 ... 96 bytes,
wavefronts that straddle series, ragged and idle chunks, the last row of the tensor.  Per-series values through the C ABI with an
explicit chunk count (as `loglik_with_chunks` of tests/test_gpu_kalman.py) against the numpy oracle at that file's tolerances:
fp64 rtol 1e-10, fp32 rtol 5e-4.  The chol Q entries that can be carried change strongly from row to row, so a stale or zeroed
carry is orders of magnitude outside the tolerance.
"""
import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from oracle import numpy_oracle as O
from test_gpu_kalman import DEV, nn, random_ssm, tt

pytestmark = pytest.mark.gpu

KEYS = ("mu0", "chol_p0", "a_s", "b_s", "chol_q", "h", "y")


def lively(rng, bsz, t, d, m):
    """A well-conditioned chain whose C[0][0], C[1][0], C[1][1] jump from row to row (factors 0.5 ... 4, both signs off the
    diagonal): log C[0][0] and log C[1][1] enter the log-likelihood directly."""
    kw = random_ssm(rng, (bsz,), t, d, m, well=True)
    cq = kw["chol_q"]
    cq[..., 0, 0] = rng.uniform(0.5, 4.0, size=cq.shape[:-2])
    if d > 1:
        cq[..., 1, 1] = rng.uniform(0.5, 4.0, size=cq.shape[:-2])
        cq[..., 1, 0] = rng.uniform(-2.0, 2.0, size=cq.shape[:-2])
    return kw


def shifted(x, dtype, shift_bytes):
    """A contiguous device copy of x whose first byte lies shift_bytes past a 256-B aligned address."""
    esz = 8 if dtype == torch.float64 else 4
    assert shift_bytes % esz == 0
    pad = 256 // esz
    buf = torch.zeros(x.size + 2 * pad, dtype=dtype, device=DEV)
    skip = (-buf.data_ptr() % 256 + shift_bytes) // esz
    out = buf[skip:skip + x.size].view(x.shape)
    out.copy_(tt(x, dtype))
    assert out.data_ptr() % 256 == shift_bytes and out.is_contiguous()
    return out


def per_series(tensors, r_inv, chunks, dtype=torch.float64, per_step=False, expect_info=True):
    """mf_kf_loglik on device tensors (mu0, cholP0, A, b, cholQ, H, y) with an explicit number of time partitions."""
    mu0, cp0, a, b, cq, h, y = tensors
    bsz, t, m, d = h.shape
    lib = _lib.load()
    esz = 8 if dtype == torch.float64 else 4
    wsb = int(lib.mf_kf_loglik_workspace_bytes(bsz, t, d, esz, chunks))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
    out = torch.empty(bsz, dtype=dtype, device=DEV)
    info = _lib.new_info(torch.device(DEV))
    ri = tt(r_inv, dtype)
    _lib.call("mf_kf_loglik", dtype, bsz, t, d, m, _lib.ptr(mu0), _lib.ptr(cp0), _lib.ptr(a), _lib.ptr(b), _lib.ptr(cq),
              _lib.ptr(h), _lib.ptr(y), _lib.ptr(ri), int(per_step), 0.0, _lib.ptr(out), _lib.ptr(ws), wsb,
              _lib.ptr(info), chunks, None, None, _lib.stream_ptr(torch.device(DEV)))
    word = int(info.item())
    if expect_info:
        assert word == 0
        return nn(out)
    return nn(out), word


def device(kw, dtype=torch.float64):
    return [tt(kw[k], dtype) for k in KEYS]


def constant(t, m, r_inv):
    return -0.5 * np.log(2 * np.pi) * m * t + 0.5 * t * np.linalg.slogdet(r_inv)[1]


R_INV = np.array([[2.5]])


@pytest.mark.parametrize("t", [101, 102, 103, 104])
def test_every_residue_of_the_chain_length_and_every_partition(rng, t):
    """T - 1 in all four residues mod 4 (the phase of a series' first row), 70 series (wavefronts straddle series), partitions
    from one chunk per series to one step per chunk: ragged last chunks, idle lanes, chunks of a single step."""
    bsz = 70
    kw = lively(rng, bsz, t, 6, 1)
    ref = O.kf_log_likelihood(**kw, r_inv=R_INV, per_series=True)
    dev = device(kw)
    for chunks in (1, 3, 4, 7, 64, 2, 13, 50, t - 1):
        got = per_series(dev, R_INV, chunks) + constant(t, 1, R_INV)
        np.testing.assert_allclose(got, ref, rtol=1e-10, err_msg=f"chunks={chunks}")


@pytest.mark.parametrize("shift", [16, 32, 48, 64, 80, 96, 112])
@pytest.mark.parametrize("t", [102, 104])
def test_bases_that_do_not_start_a_line(rng, t, shift):
    """A and chol Q at 16 ... 112 bytes past a 128-B line (16-B aligned bases take the streaming kernel): each result exact."""
    bsz = 70
    kw = lively(rng, bsz, t, 6, 1)
    ref = O.kf_log_likelihood(**kw, r_inv=R_INV, per_series=True)
    dev = device(kw)
    dev[2] = shifted(kw["a_s"], torch.float64, (shift + 32) % 128)
    dev[4] = shifted(kw["chol_q"], torch.float64, shift)
    for chunks in (1, 4, 7, 64):
        got = per_series(dev, R_INV, chunks) + constant(t, 1, R_INV)
        np.testing.assert_allclose(got, ref, rtol=1e-10, err_msg=f"chunks={chunks}")


@pytest.mark.parametrize("t", [100, 101, 102, 103])
def test_contiguous_slices_of_a_larger_allocation(rng, t):
    """A[1:], cholQ[1:] of tensors with one series more: the slice starts (T - 1) x 288 B into the allocation, i.e. 32 x (T - 1)
    mod 128 bytes into a line (96, 0, 32 and 64 here).  The last series ends with the allocation: the tail of its last row is out
    of range."""
    bsz = 71
    kw = lively(rng, bsz, t, 6, 1)
    ref = O.kf_log_likelihood(**{k: v[1:] for k, v in kw.items()}, r_inv=R_INV, per_series=True)
    full_a, full_c = tt(kw["a_s"]), tt(kw["chol_q"])
    dev = [tt(kw[k][1:]) for k in KEYS]
    dev[2], dev[4] = full_a[1:], full_c[1:]
    assert dev[4].data_ptr() % 128 == (32 * (t - 1)) % 128 and dev[4].is_contiguous()
    for chunks in (1, 3, 4, 7, 64):
        got = per_series(dev, R_INV, chunks) + constant(t, 1, R_INV)
        np.testing.assert_allclose(got, ref, rtol=1e-10, err_msg=f"chunks={chunks}")


def test_long_chunks_and_the_automatic_partition(rng):
    """Chunks far longer than the period of the fetch schedule (4 steps), and the library's own choice of partition."""
    bsz, t = 130, 1000
    kw = lively(rng, bsz, t, 6, 1)
    ref = O.kf_log_likelihood(**kw, r_inv=R_INV, per_series=True)
    dev = device(kw)
    for chunks in (0, 1, 5, 37):
        got = per_series(dev, R_INV, chunks) + constant(t, 1, R_INV)
        np.testing.assert_allclose(got, ref, rtol=1e-10, err_msg=f"chunks={chunks}")


@pytest.mark.parametrize("entry,row", [((1, 1), 5), ((1, 1), 6), ((0, 0), 7), ((0, 0), 5), ((1, 1), 4)])
@pytest.mark.parametrize("chunks", [1, 3])
def test_non_positive_pivot_in_a_carried_entry(rng, entry, row, chunks):
    """A zero on the diagonal of chol Q in an entry that travels in registers (rows 5, 6, 7 of a series start 32, 64, 96 bytes
    into a line; row 4 starts a line and is fetched whole): the info word names series and block as in tests/test_gpu_errors.py."""
    bsz, t = 70, 41
    kw = lively(rng, bsz, t, 6, 1)
    series = 4                                        # (T - 1) x 288 B is a multiple of 128: every series starts a line
    kw["chol_q"][series, row, entry[0], entry[1]] = 0.0
    _, word = per_series(device(kw), R_INV, chunks, expect_info=False)
    lib = _lib.load()
    assert word >= 2
    flat = int(lib.mf_info_flat_index(word))
    assert flat // t == series and flat % t in (row, row + 1)


@pytest.mark.parametrize("dtype,d,m,per_step", [
    (torch.float32, 6, 1, False),      # fp32: 144-B rows, no tail slots
    (torch.float64, 5, 1, False),      # odd d: rows are not whole 16-B units
    (torch.float64, 6, 2, False),      # two outputs: the image has no room for tail slots
    (torch.float64, 6, 1, True),       # per-step precisions: likewise
    (torch.float64, 4, 1, False),      # rows are whole lines
    (torch.float32, 6, 2, False),
])
def test_the_other_instantiations_still_agree_with_the_oracle(rng, dtype, d, m, per_step):
    bsz, t = 70, 103
    kw = lively(rng, bsz, t, d, m)
    if dtype == torch.float32:
        kw = {k: v.astype(np.float32).astype(np.float64) for k, v in kw.items()}
    if per_step:
        prec = 0.5 + rng.random(size=(bsz, t, 1, 1))
        if dtype == torch.float32:
            prec = prec.astype(np.float32).astype(np.float64)
        ref = O.kf_log_likelihood(**kw, r_inv=prec, log_det_obs_precision=np.sum(np.log(prec), axis=(-1, -2, -3)), per_series=True)
        cst = -0.5 * np.log(2 * np.pi) * t + 0.5 * np.sum(np.log(prec), axis=(-1, -2, -3))
        r_inv = prec
    else:
        cov = 0.5 * np.eye(m) + 0.1 * np.ones((m, m))
        r_inv = np.linalg.inv(cov)
        ref = O.kf_log_likelihood(**kw, r_inv=r_inv, per_series=True)
        cst = constant(t, m, r_inv)
    dev = device(kw, dtype)
    for chunks in (1, 3, 4, 7, 64):
        got = per_series(dev, r_inv, chunks, dtype=dtype, per_step=per_step) + cst
        np.testing.assert_allclose(got, ref, rtol=1e-10 if dtype == torch.float64 else 5e-4, err_msg=f"chunks={chunks}")
