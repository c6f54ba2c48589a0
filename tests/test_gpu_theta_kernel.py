"""
GPU tests of ``mf_lik_sparse_expectations_theta_*`` (csrc/mf_lik_theta.hip) through the raw C ABI against
tests/helpers/theta_closed_forms.py.  Layouts and tolerances are those of
tests/test_gpu_factor_kernel.py: float64 within 64 eps of (magnitude + 1); float32 within 4 x the normalised error of the helper's own
numpy float32 evaluation, both against the float64 helper.  Guard bytes follow every output and the workspace.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import theta_closed_forms as TC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
K_F64 = 64.0
GUARD, SENTINEL = 64, -77.25
TILE = 64
LAYOUT = ((0, 1, 64, 130, 195), (195, 65, 130, 0, 0), (63, 65, 64, 195, 3))      # three series, N = 390 each
OUTS = ("ve_sum", "g_mean", "g_cov", "g_theta")
FN = "mf_lik_sparse_expectations_theta"
DF, NQ = 3.0, 20
THETAS = (0.3, 1.1, 2.0)
NODES, WEIGHTS = (np.ctypeslib.as_ctypes(np.ascontiguousarray(a)) for a in np.polynomial.hermite.hermgauss(NQ))
PARAMS = (ctypes.c_double * 2)(DF, math.lgamma(0.5 * (DF + 1)) - math.lgamma(0.5 * DF) - 0.5 * math.log(DF * math.pi))


@functools.lru_cache(maxsize=None)
def reference(two_d, lik, f32, per_series):
    """Inputs (rounded to the dtype under test, symmetric after the rounding) and the float64 helper on them, per series."""
    rng = np.random.default_rng(100 * two_d + lik)
    dt = np.float32 if f32 else np.float64
    rnd = lambda a: np.asarray(a).astype(dt).astype(np.float64)          # noqa: E731
    bsz, segs, n = len(LAYOUT), len(LAYOUT[0]), int(np.sum(LAYOUT[0]))
    ref = dict(offsets=np.stack([np.concatenate([[0], np.cumsum(ln)]) for ln in LAYOUT]).astype(np.int64))
    ref["w"] = rnd(rng.uniform(-0.7, 0.7, size=(bsz, n, two_d)))
    ref["c"] = rnd(rng.uniform(0.05, 0.5, size=(bsz, n)))
    ref["y"] = rnd(rng.normal(size=(bsz, n)))
    a = rng.normal(size=(bsz, segs, two_d, two_d))
    cov = rnd(a @ np.swapaxes(a, -1, -2) / two_d + 0.1 * np.eye(two_d))          # SPD, ridge 0.1
    ref["pair_cov"] = np.tril(cov) + np.swapaxes(np.tril(cov, -1), -1, -2)
    ref["pair_mean"] = rnd(rng.normal(size=(bsz, segs, two_d)))
    ref["theta"] = rnd(THETAS if per_series else THETAS[:1])
    helper = lambda b, ty: TC.segment_expectations_theta(lik, ref["theta"][b if per_series else 0], ref["w"][b], ref["c"][b],  # noqa: E731
                                                         ref["y"][b], ref["offsets"][b], ref["pair_mean"][b], ref["pair_cov"][b], ty, DF, NQ)
    ref["want"] = [helper(b, np.float64) for b in range(bsz)]
    assert all(np.all(want["fvar"] > 0) for want in ref["want"]), "every point is inside the domain: no case is left out"
    ref["want32"] = [helper(b, np.float32) for b in range(bsz)] if f32 else None
    return ref


def guarded(shape, dtype):
    buf = torch.full((int(np.prod(shape)) + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:-GUARD].view(shape)


def launch(dtype, ref, lik, series=None, want=(True, True, True, True), two_d=None, null_theta=False, short_ws=0, theta=None):
    """One call on all the series of ``ref`` (or on ``series`` alone); ``lik`` / ``two_d``: what the call CLAIMS.  Checks the guards."""
    pick = (lambda a: a) if series is None else (lambda a: a[series:series + 1])
    bsz, n, d2 = pick(ref["w"]).shape
    offsets = pick(ref["offsets"])
    segs = offsets.shape[1] - 1
    per = (np.diff(offsets, axis=1).reshape(-1) + TILE - 1) // TILE
    tiles, tile_seg, seg_tile = int(per.sum()), np.repeat(np.arange(per.size), per), np.concatenate([[0], np.cumsum(per)])
    tab = [torch.tensor(a, dtype=torch.int64, device=DEV).contiguous() for a in (offsets, tile_seg, seg_tile)]
    ins = [torch.tensor(pick(ref[k]), dtype=dtype, device=DEV).contiguous() for k in ("w", "c", "y", "pair_mean", "pair_cov")]
    th = ref["theta"] if theta is None else np.asarray(theta)
    stride = int(th.size > 1)
    th = None if null_theta else torch.tensor(pick(th) if stride else th, dtype=dtype, device=DEV).contiguous()
    shapes = ((bsz, segs), (bsz, segs, d2), (bsz, segs, d2, d2), (bsz, segs))
    outs = [guarded(s, dtype) if wanted else (None, None) for s, wanted in zip(shapes, want)]
    elem = torch.empty((), dtype=dtype).element_size()
    ws_bytes = int(_lib.load().mf_lik_sparse_expectations_theta_workspace_bytes(tiles, d2, elem))
    assert ws_bytes == tiles * (d2 * (d2 + 1) // 2 + d2 + 2) * elem
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = _lib.call_rc(FN, dtype, bsz, n, segs, d2 if two_d is None else two_d, lik, PARAMS, NQ, NODES, WEIGHTS, _lib.ptr(th), stride,
                      _lib.ptr(tab[0]), *[_lib.ptr(t) for t in ins], tiles, _lib.ptr(tab[1]), _lib.ptr(tab[2]), _lib.ptr(ws),
                      ws_bytes - short_ws, *[_lib.ptr(o[1]) for o in outs], _lib.stream_ptr(DEV))
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
    print(f"ERR f32 {what}: kernel {scaled.max():.3e}  numpy float32 {own:.3e}  ratio {scaled.max() / max(own, 1e-300):.2f}")
    return None if scaled.max() <= 4.0 * own else f"{what}: kernel {scaled.max():.3e} against numpy float32 {own:.3e}"


@pytest.mark.parametrize("per_series", [False, True], ids=["shared", "per-series"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("lik", [0, 3], ids=["gaussian", "student-t"])
@pytest.mark.parametrize("two_d", [2, 10, 18])
def test_batch_of_three_against_the_helper_alone_and_output_by_output_bit_for_bit(two_d, lik, dtype, per_series):
    f32 = dtype == torch.float32
    ref = reference(two_d, lik, f32, per_series)
    rc, outs = launch(dtype, ref, lik)
    assert rc == 0
    failures = []
    for b in range(len(LAYOUT)):
        for key, got in zip(OUTS, outs):
            assert not bool(torch.any(got[b] == SENTINEL)), f"series {b} {key}: an element was not written"
            failures.append(check(f"lik={lik} 2d={two_d} series {b} {key}", got[b].cpu().numpy(), ref["want"][b][key],
                                  ref["want"][b]["mag_" + key], dtype, ref["want32"][b][key] if f32 else None))
    assert not [f for f in failures if f], "; ".join(f for f in failures if f)
    assert torch.equal(outs[2], outs[2].transpose(-1, -2)), "bitwise symmetric"
    for b, ln in enumerate(LAYOUT):
        for s, count in enumerate(ln):
            if count == 0:
                assert all(float(o[b, s].abs().max()) == 0.0 for o in outs), "an empty segment: exact zeros"
    for b in range(3):
        rc, one = launch(dtype, ref, lik, series=b)
        assert rc == 0 and all(torch.equal(o[0], f[b]) for o, f in zip(one, outs)), "a series alone gives the bits it gives in a batch"
    for want in ((False, False, False, True), (False, True, True, False), (True, False, False, False)):
        rc, some = launch(dtype, ref, lik, want=want)
        assert rc == 0 and all(o is None or torch.equal(o, f) for o, f in zip(some, outs)), f"{want}: the bits beside the others"


@pytest.mark.parametrize("bad", [0.0, -0.5, float("nan")], ids=["zero", "negative", "nan"])
@pytest.mark.parametrize("lik", [0, 3], ids=["gaussian", "student-t"])
def test_an_invalid_theta_poisons_its_own_series_only(lik, bad):
    ref = reference(10, lik, False, True)
    _, good = launch(torch.float64, ref, lik)
    rc, outs = launch(torch.float64, ref, lik, theta=(THETAS[0], bad, THETAS[2]))
    assert rc == 0
    for o, g in zip(outs, good):
        assert bool(torch.isnan(o[1]).all()), "all four outputs of every segment of the series, the empty ones included"
        assert torch.equal(o[0], g[0]) and torch.equal(o[2], g[2]), "the other series keep their bits"


def test_refusals():
    ref = reference(10, 0, False, True)
    clean = lambda outs: all(bool(torch.all(o == SENTINEL)) for o in outs)          # noqa: E731
    for lik, claim, want in ((1, {}, -101), (0, dict(two_d=5), -100), (0, dict(two_d=20), -100), (0, dict(null_theta=True), -10),
                             (3, dict(short_ws=1), -22)):
        rc, outs = launch(torch.float64, ref, lik, **claim)
        assert rc == want and clean(outs), (lik, claim, rc)
