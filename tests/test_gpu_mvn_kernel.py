"""
GPU tests of ``mf_lik_sparse_mvn_expectations_*`` (csrc/mf_lik_mvn.hip) through the raw C ABI against tests/helpers/mvn_closed_forms.py.
Scheme, segment layouts (an empty segment, one point, exactly one tile, a tile plus a remainder, several tiles) and tolerances are
those of tests/test_gpu_factor_kernel.py: float64 within 64 eps of (magnitude + 1); float32 within 4 x the normalised error of the
helper's own numpy float32 evaluation, both against the float64 helper.  ``Lam`` is non-diagonal; guard bytes follow every buffer.
"""
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import mvn_closed_forms as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
K_F64 = 64.0
GUARD, SENTINEL = 64, -77.25
TILE = 64
LAYOUT = ((0, 1, 64, 130, 195), (195, 65, 130, 0, 0), (63, 65, 64, 195, 3))      # three series, N = 390 each
OUTS = ("quad_sum", "g_mean", "g_cov", "m_sum")
FN = "mf_lik_sparse_mvn_expectations"
CASES = [(2, 2), (3, 6), (4, 8), (2, 18), (4, 18)]


def spd(rng, shape, dim, ridge):
    a = rng.normal(size=shape + (dim, dim))
    return a @ np.swapaxes(a, -1, -2) / dim + ridge * np.eye(dim)


@functools.lru_cache(maxsize=None)
def reference(outs, two_d, f32):
    """Inputs (rounded to the dtype under test, symmetric after the rounding) and the float64 helper on them, per series."""
    rng = np.random.default_rng(100 * outs + two_d)
    dt = np.float32 if f32 else np.float64
    rnd = lambda a: np.asarray(a).astype(dt).astype(np.float64)          # noqa: E731
    sym = lambda a: np.tril(a) + np.swapaxes(np.tril(a, -1), -1, -2)     # noqa: E731
    bsz, segs, n = len(LAYOUT), len(LAYOUT[0]), int(np.sum(LAYOUT[0]))
    ref = dict(offsets=np.stack([np.concatenate([[0], np.cumsum(ln)]) for ln in LAYOUT]).astype(np.int64))
    ref["w"] = rnd(rng.uniform(-0.7, 0.7, size=(bsz, n, outs, two_d)))
    ref["c"] = sym(rnd(spd(rng, (bsz, n), outs, 0.05)))
    ref["y"] = rnd(rng.normal(size=(bsz, n, outs)))
    chol = np.tril(rng.uniform(-0.5, 0.5, size=(outs, outs)), -1) + np.diag(rng.uniform(0.6, 1.2, size=outs))
    ref["prec"] = sym(rnd(np.linalg.inv(chol @ chol.T)))                  # non-diagonal
    assert np.abs(ref["prec"][1, 0]) > 1e-3
    ref["pair_cov"] = sym(rnd(spd(rng, (bsz, segs), two_d, 0.1)))
    ref["pair_mean"] = rnd(rng.normal(size=(bsz, segs, two_d)))
    helper = lambda b, ty: MC.segment_expectations_mvn(ref["w"][b], ref["c"][b], ref["y"][b], ref["prec"], ref["offsets"][b],  # noqa: E731
                                                       ref["pair_mean"][b], ref["pair_cov"][b], ty)
    ref["want"] = [helper(b, np.float64) for b in range(bsz)]
    ref["want32"] = [helper(b, np.float32) for b in range(bsz)] if f32 else None
    return ref


def guarded(shape, dtype):
    buf = torch.full((int(np.prod(shape)) + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:-GUARD].view(shape)


def launch(dtype, ref, series=None, want=(True, True, True, True), two_d=None, outputs=None, null=None, short_ws=0):
    """One call on all the series of ``ref`` (or on ``series`` alone).  ``two_d`` / ``outputs``: what the call CLAIMS; ``null``: an input
    passed as NULL; ``short_ws``: bytes taken off the workspace size.  Returns ``(rc, outputs)`` after checking every guard region."""
    pick = (lambda a: a) if series is None else (lambda a: a[series:series + 1])
    bsz, n, outs_p, d2 = pick(ref["w"]).shape
    offsets = pick(ref["offsets"])
    segs = offsets.shape[1] - 1
    per = (np.diff(offsets, axis=1).reshape(-1) + TILE - 1) // TILE
    tiles, tile_seg, seg_tile = int(per.sum()), np.repeat(np.arange(per.size), per), np.concatenate([[0], np.cumsum(per)])
    tab = [torch.tensor(a, dtype=torch.int64, device=DEV).contiguous() for a in (offsets, tile_seg, seg_tile)]
    names = ("w", "c", "y", "prec", "pair_mean", "pair_cov")
    ins = [None if k == null else torch.tensor(ref[k] if k == "prec" else pick(ref[k]), dtype=dtype, device=DEV).contiguous() for k in names]
    shapes = ((bsz, segs), (bsz, segs, d2), (bsz, segs, d2, d2), (bsz, segs, outs_p, outs_p))
    outs = [guarded(s, dtype) if wanted else (None, None) for s, wanted in zip(shapes, want)]
    elem = torch.empty((), dtype=dtype).element_size()
    ws_bytes = int(_lib.load().mf_lik_sparse_mvn_expectations_workspace_bytes(tiles, d2, outs_p, elem))
    assert ws_bytes == tiles * (d2 * (d2 + 1) // 2 + d2 + outs_p * (outs_p + 1) // 2 + 1) * elem
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = _lib.call_rc(FN, dtype, bsz, n, segs, d2 if two_d is None else two_d, outs_p if outputs is None else outputs, _lib.ptr(tab[0]),
                      *[_lib.ptr(t) for t in ins], tiles, _lib.ptr(tab[1]), _lib.ptr(tab[2]), _lib.ptr(ws), ws_bytes - short_ws,
                      *[_lib.ptr(o[1]) for o in outs], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert all(b[0] is None or bool(torch.all(b[0][-GUARD:] == SENTINEL)) for b in outs), "a write past the end of an output"
    assert bool(torch.all(ws[ws_bytes:] == 0x5A)), "a write past the end of the workspace"
    return rc, [o[1] for o in outs]


def check(what, got, want, mag, dtype, got32=None):
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    scaled = np.abs(got - want) / (np.asarray(mag) + 1.0)
    if dtype == torch.float64:
        ratio = float(scaled.max() / EPS)
        print(f"RATIO f64 {what}: {ratio:.2f}")
        return None if ratio <= K_F64 else f"{what}: {ratio:.1f} eps (magnitude + 1)"
    own = float((np.abs(np.asarray(got32, dtype=np.float64) - want) / (np.asarray(mag) + 1.0)).max())
    print(f"ERR f32 {what}: kernel {scaled.max():.3e}  numpy float32 {own:.3e}")
    return None if scaled.max() <= 4.0 * own else f"{what}: kernel {scaled.max():.3e} against numpy float32 {own:.3e}"


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("outputs,two_d", CASES, ids=[f"P{p}-2d{d}" for p, d in CASES])
def test_batch_of_three_against_the_helper_and_each_series_alone_bit_for_bit(outputs, two_d, dtype):
    f32 = dtype == torch.float32
    ref = reference(outputs, two_d, f32)
    rc, outs = launch(dtype, ref)
    assert rc == 0
    failures = []
    for b in range(len(LAYOUT)):
        for key, got in zip(OUTS, outs):
            assert not bool(torch.any(got[b] == SENTINEL)), f"series {b} {key}: an element was not written"
            failures.append(check(f"P={outputs} 2d={two_d} series {b} {key}", got[b].cpu().numpy(), ref["want"][b][key],
                                  ref["want"][b]["mag_" + key], dtype, ref["want32"][b][key] if f32 else None))
    assert not [f for f in failures if f], "; ".join(f for f in failures if f)
    assert torch.equal(outs[2], outs[2].transpose(-1, -2)) and torch.equal(outs[3], outs[3].transpose(-1, -2)), "bitwise symmetric"
    for b, ln in enumerate(LAYOUT):
        for s, count in enumerate(ln):
            if count == 0:
                assert all(float(o[b, s].abs().max()) == 0.0 for o in outs), "an empty segment: exact zeros"
    for b in range(3):
        rc, one = launch(dtype, ref, series=b)
        assert rc == 0 and all(torch.equal(o[0], f[b]) for o, f in zip(one, outs)), "a series alone gives the bits it gives in a batch"
    rc, value = launch(dtype, ref, want=(True, False, False, False))
    assert rc == 0 and torch.equal(value[0], outs[0]), "value-only mode has the bits of the value beside the adjoints"


def test_refusals():
    ref = reference(3, 6, False)
    clean = lambda outs: all(bool(torch.all(o == SENTINEL)) for o in outs)          # noqa: E731
    for claim, want in ((dict(outputs=5), -101), (dict(two_d=7), -101), (dict(null="c"), -8), (dict(null="prec"), -10),
                        (dict(short_ws=1), -17)):
        rc, outs = launch(torch.float64, ref, **claim)
        assert rc == want and clean(outs), (claim, rc)
