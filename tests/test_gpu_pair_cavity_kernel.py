"""GPU tests of ``mf_pair_cavity_*`` (csrc/mf_pair_cavity.hip) through the raw C ABI, against the dense-inverse statement of the cavity at
50 digits (tests/helpers/pair_cavity_exact.py).  Tolerance, per output of a launch: ``max |err| / (|reference| + 1)`` of the kernel is at
most 4 x the same figure of ``models.pair_cavity_torch`` - batched torch by explicit inverses, the arithmetic the kernel replaces - on CPU
tensors of the same dtype and the same (dtype-rounded) inputs.  Both figures are printed ("ERR ..."); measured maxima: CHANGELOG.md.
Shapes: every n = 2 ... 18, both dtypes, (B, S) = (1, 1) - one pair -, (3, 5) - 15 pairs: a partial workgroup at n = 2, full and ragged
ones above - and (2, 70) - 140 pairs: several workgroups of 16 ... 2 pairs with a ragged last one."""
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from markovflow_amd import models as MM
from helpers import pair_cavity_exact as X

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32]
NUMPY = {torch.float64: np.float64, torch.float32: np.float32}
GUARD, SENTINEL = 64, -77.25


def torch_route(case, dtype):
    return dict(zip(X.OUTPUTS, (t.numpy() for t in MM.pair_cavity_torch(*[torch.tensor(case[k], dtype=dtype) for k in X.KEYS]))))


@functools.lru_cache(maxsize=None)
def reference(shape, n, dtype):          # inputs, the 50-digit cavity and the torch route on them: once per case, shared
    case = X.draw(*shape, n, NUMPY[dtype])
    want = X.exact(case)
    assert all(np.isfinite(v).all() for v in want.values()), "the reference defines every pair"
    return case, want, torch_route(case, dtype)


def launch(dtype, case, n=None):         # one call: (rc, outputs as numpy arrays), the guard behind every output checked
    bsz, segs, size = case["pair_mean"].shape
    ins = [torch.tensor(case[k], dtype=dtype, device=DEV).contiguous() for k in X.KEYS]
    shapes = ((bsz, segs, size), (bsz, segs, size, size), (bsz, segs))
    bufs = [torch.full((int(np.prod(shape)) + GUARD,), SENTINEL, dtype=dtype, device=DEV) for shape in shapes]
    rc = _lib.call_rc("mf_pair_cavity", dtype, bsz, segs, size if n is None else n, *[_lib.ptr(t) for t in ins],
                      *[_lib.ptr(b[:-GUARD]) for b in bufs], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert all(bool(torch.all(b[-GUARD:] == SENTINEL)) for b in bufs), "a write past the end of an output"
    return rc, {k: b[:-GUARD].view(shape).cpu().numpy() for k, b, shape in zip(X.OUTPUTS, bufs, shapes)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (2, 70)])
@pytest.mark.parametrize("n", [2, 4, 6, 8, 10, 12, 14, 16, 18])
def test_every_pair_size_against_the_cavity_at_fifty_digits(n, shape, dtype):
    case, want, own = reference(shape, n, dtype)
    rc, out = launch(dtype, case)
    assert rc == 0
    assert np.array_equal(out["cav_cov"], out["cav_cov"].swapaxes(-1, -2)), "cav_cov is written symmetric"
    assert np.all(out["gamma"][case["beta"] == 0.0] == 0.0), "beta = 0: nothing is removed, gamma is 0"
    failures = X.within_four(f"n={n} {shape} {dtype}", out, own, want)
    assert not failures, "; ".join(failures)
    assert all(np.array_equal(out[k], again) for k, again in launch(dtype, case)[1].items()), "the same bits on every launch"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_pair_without_a_positive_definite_marginal_or_cavity_is_nan_alone(dtype):
    case = {k: v.copy() for k, v in reference((3, 5), 6, dtype)[0].items()}
    bad = [(0, 2), (1, 4)]
    q = np.linalg.qr(np.random.default_rng(5).normal(size=(6, 6)))[0]
    case["pair_cov"][0, 2] = (q * np.array([-1.0, 0.5, 1.0, 2.0, 3.0, 4.0])) @ q.T         # one negative eigenvalue
    case["pair_cov"][0, 2] = 0.5 * (case["pair_cov"][0, 2] + case["pair_cov"][0, 2].T)
    case["nat2"][1, 4], case["beta"][1, 4] = -4.0 * np.linalg.inv(case["pair_cov"][1, 4]), 1.0   # cavity precision -7 S^-1
    case = {k: v.astype(NUMPY[dtype]).astype(np.float64) for k, v in case.items()}
    want = X.exact(case, skip=bad)
    keep = np.isfinite(want["gamma"])
    assert int(keep.sum()) == 13 and all(np.isfinite(want[k][keep]).all() for k in X.OUTPUTS)
    rc, out = launch(dtype, case)
    assert rc == 0
    for k in X.OUTPUTS:
        assert all(np.isnan(out[k][at]).all() for at in bad) and np.isfinite(out[k][keep]).all(), f"{k}: NaN for those two pairs only"
    failures = X.within_four(f"not positive definite {dtype}", out, torch_route(case, dtype), want, keep)
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("n", [3, 20])
def test_an_odd_or_large_pair_size_is_rejected_and_nothing_is_written(n):
    rc, out = launch(torch.float64, reference((3, 5), 4, torch.float64)[0], n=n)
    assert rc < 0 and all(np.all(v == SENTINEL) for v in out.values())
