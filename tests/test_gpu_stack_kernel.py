"""
GPU tests of ``mf_lik_stack_expectations_*`` (csrc/mf_lik_stack.hip) through the raw C ABI, against the numpy statement of its
formulas in tests/helpers/stack_closed_forms.py (``segment_expectations_stack``).  The scheme is that of
tests/test_gpu_multistage_kernel.py.

Tolerances.
  float64: ``|err| <= K eps (magnitude + 1)``, eps = 2^-52, K = 64, with the helper's magnitudes: sum_n |gv_k| |w_ki| |w_kj| for
    g_cov[k], sum_n |gm_k| |w_ki| for g_mean[k] and the sum of the expectations' own magnitudes for ve_sum.  check() prints every
    ratio ("RATIO f64 ...").  Measured maxima on an MI355X over all the cases of this file (81 figures): multi-stage ve_sum 2.07,
    g_mean 5.09, g_cov 4.82; heteroscedastic ve_sum 1.65, g_mean 1.31, g_cov 1.80.
  float32: the kernel's error, normalised by (magnitude + 1) and maximised over an output of one series, against 4 x the same figure
    of the helper evaluated in numpy float32 on the same (float32-rounded) inputs; the helper projects and sums in the kernel's order
    (points ascending, the latents of a point ascending, tiles of 64 points, then the tiles), and both errors are taken against the
    float64 helper.  Measured per series on an MI355X over the 81 figures: multi-stage ve_sum at most 1.07 x, g_mean 0.53 x,
    g_cov 0.66 x; heteroscedastic ve_sum 1.54 x, g_mean 1.91 x, g_cov 1.25 x; the largest normalised error 7.6e-07.

Every series has N = 390 points in S = 5 segments whose lengths are drawn from {0, 1, 3, 63, 64, 65, 130, 195}: a tile is 64 points, so
segments of one, two, three and four tiles are combined, both sides of a tile boundary are met and segments are empty.  The
multi-stage observations cycle through (0, 1, 2, 5, 0, 1, 9, 0.5): every branch of the likelihood and the one that contributes
nothing; the heteroscedastic ones are drawn from a normal, and the rows of ``w`` of the log-variance latent are scaled so that
``|mu_1| <= 3`` (the helper's float32 evaluation is asserted finite on these inputs).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import stack_closed_forms as ST

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
K_F64 = 64.0
DTYPES = [torch.float64, torch.float32]
GUARD, SENTINEL = 64, -77.25
TILE = 64
LAYOUT = ((0, 1, 64, 130, 195), (195, 65, 130, 0, 0), (63, 65, 64, 195, 3))      # three series, N = 390 each
OUTS = ("ve_sum", "g_mean", "g_cov")
FN = "mf_lik_stack_expectations"
Y_CYCLE = (0.0, 1.0, 2.0, 5.0, 0.0, 1.0, 9.0, 0.5)
CASES = [(3, 4, 20), (3, 4, 32), (2, 5, 20)]           # (K, lik, nq)


@functools.lru_cache(maxsize=None)
def c_rule(nq):
    x, w = np.polynomial.hermite.hermgauss(nq)
    return (ctypes.c_double * nq)(*x), (ctypes.c_double * nq)(*w)


def tile_table(offsets):
    """``(num_tiles, tile_seg, seg_tile)`` of ``offsets [B, S + 1]``, in plain numpy."""
    per = (np.diff(offsets, axis=1).reshape(-1) + TILE - 1) // TILE
    return int(per.sum()), np.repeat(np.arange(per.size), per).astype(np.int64), np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def reference(lat, lik, nq, two_d, f32, layout=LAYOUT):
    """Inputs (rounded to the dtype under test) and the float64 helper on them, per series - computed once per case and shared,
    read-only.  S_pair is a random SPD matrix and c > 0: every s2 > 0 by construction."""
    rng = np.random.default_rng(lik * 1000 + two_d * 100 + nq)
    dt = np.float32 if f32 else np.float64
    rnd = lambda a: np.asarray(a).astype(dt).astype(np.float64)          # noqa: E731
    bsz, segs, n = len(layout), len(layout[0]), int(np.sum(layout[0]))
    assert all(int(np.sum(ln)) == n for ln in layout)
    ref = dict(offsets=np.stack([np.concatenate([[0], np.cumsum(ln)]) for ln in layout]).astype(np.int64))
    w = rng.uniform(-0.7, 0.7, size=(bsz, lat, n, two_d))
    a = rng.normal(size=(bsz, lat, segs, two_d, two_d))
    ref["pair_cov"] = rnd(a @ np.swapaxes(a, -1, -2) / two_d + 0.1 * np.eye(two_d))
    ref["pair_mean"] = rnd(rng.normal(size=(bsz, lat, segs, two_d)))
    if lik == ST.HETERO:                                                 # |mu_1| <= 0.7 scale sum_i |m_i| <= 3
        reach = 0.7 * np.abs(ref["pair_mean"][:, 1]).sum(axis=-1).max(axis=-1)
        w[:, 1] *= np.minimum(1.0, 3.0 / reach)[:, None, None]
        ref["y"] = rnd(rng.normal(scale=1.5, size=(bsz, n)))
    else:
        ref["y"] = rnd(np.resize(np.asarray(Y_CYCLE), (bsz, n)))
    ref["w"] = rnd(w)
    ref["c"] = rnd(rng.uniform(0.05, 0.5, size=(bsz, lat, n)))
    ref["want"] = [helper(ref, b, lik, nq, np.float64) for b in range(bsz)]
    if f32:
        ref["want32"] = [helper(ref, b, lik, nq, np.float32) for b in range(bsz)]
        assert all(np.all(np.isfinite(v)) for low in ref["want32"] for v in low.values()), "the float32 helper stays finite"
    freeze(ref)
    return ref


def helper(ref, b, lik, nq, dtype):
    return ST.segment_expectations_stack(ref["w"][b], ref["c"][b], ref["y"][b], ref["offsets"][b], ref["pair_mean"][b],
                                         ref["pair_cov"][b], lik, nq, dtype)


def freeze(ref):
    for v in ref.values():
        for a in (v if isinstance(v, list) else [v]):
            for x in (a.values() if isinstance(a, dict) else [a]):
                x.setflags(write=False)


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def guarded(shape, dtype):
    """A sentinel-filled buffer of ``shape`` followed by a sentinel-filled guard region."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def launch(lik, nq, dtype, ref, series=None, want=(True, True, True), table=None, two_d=None, latent_dim=None):
    """One call on all the series of ``ref`` (or on ``series`` alone).  ``table``: a (corrupt) tile table in place of the right one;
    ``two_d`` / ``latent_dim`` / ``lik``: what the call CLAIMS (the buffers keep their shapes).  Returns ``(rc, [ve_sum, g_mean,
    g_cov])`` as tensors (None where not asked for) after checking every guard region."""
    pick = (lambda a: a) if series is None else (lambda a: a[series:series + 1])
    bsz, lat, n, d2 = pick(ref["w"]).shape
    offsets = pick(ref["offsets"])
    segs = offsets.shape[1] - 1
    tiles, tile_seg, seg_tile = tile_table(offsets)
    if table is not None:
        tile_seg, seg_tile = table
    tab = [torch.tensor(a, dtype=torch.int64, device=DEV).contiguous() for a in (offsets, tile_seg, seg_tile)]
    ins = [dev(pick(ref[k]), dtype) for k in ("w", "c", "y", "pair_mean", "pair_cov")]
    shapes = ((bsz, segs), (bsz, lat, segs, d2), (bsz, lat, segs, d2, d2))
    outs = [guarded(s, dtype) if w else (None, None) for s, w in zip(shapes, want)]
    ws_bytes = int(_lib.load().mf_lik_stack_expectations_workspace_bytes(tiles, d2, lat, ins[0].element_size()))
    assert ws_bytes == tiles * (lat * (d2 * (d2 + 1) // 2 + d2) + 1) * ins[0].element_size()
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    nodes, weights = c_rule(nq)
    rc = _lib.call_rc(FN, dtype, bsz, lat if latent_dim is None else latent_dim, n, segs, d2 if two_d is None else two_d, lik, None, nq,
                      nodes, weights, _lib.ptr(tab[0]), *[_lib.ptr(t) for t in ins], tiles, _lib.ptr(tab[1]), _lib.ptr(tab[2]),
                      _lib.ptr(ws), ws_bytes, *[_lib.ptr(o[1]) for o in outs], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert all(b[0] is None or bool(torch.all(b[0][-GUARD:] == SENTINEL)) for b in outs), "a write past the end of an output"
    assert bool(torch.all(ws[ws_bytes:] == 0x5A)), "a write past the end of the workspace"
    return rc, [o[1] for o in outs]


def check(what, got, want, mag, dtype, got32=None):
    """float64: the K eps bound; float32: 4 x the normalised error of the numpy float32 evaluation.  Prints the figure, returns the
    failure as text or None."""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    scaled = np.abs(got - want) / (np.asarray(mag) + 1.0)
    if dtype == torch.float64:
        ratio = float(scaled.max() / EPS)
        print(f"RATIO f64 {what}: {ratio:.2f}")
        if ratio > K_F64:
            return f"{what}: {ratio:.1f} eps (magnitude + 1) at {np.unravel_index(int(scaled.argmax()), scaled.shape)}"
    else:
        own = float((np.abs(np.asarray(got32, dtype=np.float64) - want) / (np.asarray(mag) + 1.0)).max())
        print(f"ERR f32 {what}: kernel {scaled.max():.3e}  numpy float32 {own:.3e}  ({scaled.max() / own if own else float(scaled.max() > 0):.2f} x)")
        if scaled.max() > 4.0 * own:
            return f"{what}: kernel {scaled.max():.3e} against numpy float32 {own:.3e}"
    return None


def check_against_helper(tag, ref, dtype, outs, series=None):
    """Every series and every output on its own; every figure is printed before the first failure is raised."""
    f32 = dtype == torch.float32
    rows = list(range(len(ref["want"]))) if series is None else [series]
    failures = []
    for i, b in enumerate(rows):
        want = ref["want"][b]
        own = ref["want32"][b] if f32 else {}
        for key, got in zip(OUTS, outs):
            if got is not None:
                assert not bool(torch.any(got[i] == SENTINEL)), f"{tag} series {b} {key}: an element was not written"
                failures.append(check(f"{tag} series {b} {key}", got[i].cpu().numpy(), want[key], want["mag_" + key], dtype, own.get(key)))
    failures = [f for f in failures if f]
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lat,lik,nq", CASES)
@pytest.mark.parametrize("two_d", [2, 6, 18])
def test_batch_of_three_against_the_helper_and_each_series_alone_bit_for_bit(two_d, lat, lik, nq, dtype):
    ref = reference(lat, lik, nq, two_d, dtype == torch.float32)
    rc, outs = launch(lik, nq, dtype, ref)
    assert rc == 0
    check_against_helper(f"K={lat} lik={lik} 2d={two_d} nq={nq}", ref, dtype, outs)
    g_cov = outs[2]
    assert torch.equal(g_cov, g_cov.transpose(-1, -2)), "g_cov is symmetric: both triangles are written from one sum"
    for b, ln in enumerate(LAYOUT):
        for s, count in enumerate(ln):
            if count == 0:
                assert float(outs[0][b, s].abs()) == 0.0 and all(float(o[b, :, s].abs().max()) == 0.0 for o in outs[1:]), \
                    "an empty segment: exact zeros"
    rc, again = launch(lik, nq, dtype, ref)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(again, outs)), "two launches on the same inputs return the same bits"
    for b in range(3):
        rc, one = launch(lik, nq, dtype, ref, series=b)
        assert rc == 0
        assert all(torch.equal(o[0], f[b]) for o, f in zip(one, outs)), "a series alone gives the bits it gives in a batch"
    rc, value = launch(lik, nq, dtype, ref, want=(True, False, False))
    assert rc == 0 and value[1] is None and value[2] is None
    assert torch.equal(value[0], outs[0]), "value-only mode has the bits of the value beside the gradients"
    rc, grads = launch(lik, nq, dtype, ref, want=(False, True, True))
    assert rc == 0 and grads[0] is None and torch.equal(grads[1], outs[1]) and torch.equal(grads[2], outs[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_bad_variance_on_a_read_latent_poisons_its_segment_on_every_chain_and_on_an_unread_one_changes_nothing(dtype):
    lat, lik, nq, two_d, f32 = 3, 4, 20, 6, dtype == torch.float32
    ref = dict(reference(lat, lik, nq, two_d, f32))
    rc, clean = launch(lik, nq, dtype, ref)
    assert rc == 0
    y, off = ref["y"], ref["offsets"]

    def point(b, s, value, skip=0):
        """The first point of segment ``s`` of series ``b``, ``skip`` points in, that observes ``value``."""
        ks = [k for k in range(off[b, s] + skip, off[b, s + 1]) if y[b, k] == value]
        assert ks, (b, s, value)
        return ks[0]

    # latents that are not read: 1 and 2 of a y == 0 point (in the second tile of its segment), 2 of two y == 1 points, all three of a
    # y == 0.5 point
    c = ref["c"].copy()
    k0, k1, k2, k3 = point(0, 3, 0.0, skip=64), point(1, 0, 1.0), point(2, 0, 0.5), point(1, 2, 1.0)
    for (b, k, l), v in zip(((0, k0, 1), (0, k0, 2), (1, k1, 2), (2, k2, 0), (2, k2, 1), (2, k2, 2), (1, k3, 2)),
                            (-1e6, 0.0, float("nan"), -1e6, 0.0, float("nan"), -3.0)):
        c[b, l, k] = v
    ref["c"] = c
    rc, outs = launch(lik, nq, dtype, ref)
    assert rc == 0
    assert all(torch.equal(o, f) for o, f in zip(outs, clean)), "the variance of a latent that is not read is not examined"
    # latents that are read.  series 0: latent 1 of a y == 9 point in the second tile of segment 3; series 2: latent 0 of a y == 0
    # point of segment 0 (NaN) and latent 1 of a y == 1 point of the last segment
    c = c.copy()
    for b, k, l, v in ((0, point(0, 3, 9.0, skip=64), 1, -1e6), (2, point(2, 0, 0.0), 0, float("nan")), (2, point(2, 4, 1.0), 1, -1e6)):
        c[b, l, k] = v
    ref["c"] = c
    rc, outs = launch(lik, nq, dtype, ref)
    assert rc == 0
    poisoned = {(0, 3), (2, 0), (2, 4)}
    for b in range(3):
        for s in range(5):
            for o, f in zip(outs, clean):
                got, was = (o[b, s], f[b, s]) if o.dim() == 2 else (o[b, :, s], f[b, :, s])
                if (b, s) in poisoned:
                    assert bool(torch.isnan(got).all()), "every output of its segment is NaN, on all K chains"
                else:
                    assert torch.equal(got, was), "every other segment keeps its bits"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_heteroscedastic_likelihood_reads_both_latents_at_every_point(dtype):
    lat, lik, nq, two_d, f32 = 2, 5, 20, 6, dtype == torch.float32
    ref = dict(reference(lat, lik, nq, two_d, f32))
    rc, clean = launch(lik, nq, dtype, ref)
    assert rc == 0
    off = ref["offsets"]
    c = ref["c"].copy()
    # (the log-variance latent in the second tile of a segment, the mean latent with NaN, the log-variance latent of a short segment)
    c[0, 1, off[0, 3] + 70], c[2, 0, off[2, 0] + 5], c[2, 1, off[2, 4]] = -1e6, float("nan"), -1e3
    ref["c"] = c
    rc, outs = launch(lik, nq, dtype, ref)
    assert rc == 0
    poisoned = {(0, 3), (2, 0), (2, 4)}
    for b in range(3):
        for s in range(5):
            for o, f in zip(outs, clean):
                got, was = (o[b, s], f[b, s]) if o.dim() == 2 else (o[b, :, s], f[b, :, s])
                if (b, s) in poisoned:
                    assert bool(torch.isnan(got).all()), "every output of its segment is NaN, on both chains"
                else:
                    assert torch.equal(got, was), "every other segment keeps its bits"


def test_a_signature_that_is_not_instantiated_returns_minus_101_and_writes_nothing():
    dtype = torch.float64
    ref = reference(3, 4, 20, 6, False)
    for claim in (dict(latent_dim=4), dict(two_d=20), dict(two_d=3), dict(two_d=0), dict(latent_dim=2), dict(latent_dim=1),
                  dict(lik=5), dict(lik=1), dict(lik=0), dict(lik=6)):
        rc, outs = launch(claim.pop("lik", 4), 20, dtype, ref, **claim)
        assert rc == -101, claim
        assert all(bool(torch.all(o == SENTINEL)) for o in outs), "nothing is written"
    rc, outs = launch(4, 20, dtype, reference(2, 5, 20, 6, False))                      # (K, lik) = (2, 4)
    assert rc == -101 and all(bool(torch.all(o == SENTINEL)) for o in outs)
    nodes, weights = c_rule(20)
    with pytest.raises(NotImplementedError, match="not instantiated"):
        _lib.call(FN, dtype, 1, 4, 0, 1, 4, 4, None, 20, nodes, weights, *([None] * 6), 0, None, None, None, 0, None, None, None,
                  _lib.stream_ptr(DEV))
    # the leading argument checks, N = 0 and B = 0
    call = lambda *a: _lib.call_rc(FN, dtype, *a, _lib.stream_ptr(DEV))          # noqa: E731
    tail = [*([None] * 6), 0, None, None, None, 0, None, None, None]
    assert call(-1, 3, 0, 1, 6, 4, None, 20, nodes, weights, *tail) == -1 and call(1, 3, -1, 1, 6, 4, None, 20, nodes, weights, *tail) == -3
    assert call(1, 3, 0, 0, 6, 4, None, 20, nodes, weights, *tail) == -4 and call(1, 3, 0, 1, 6, 4, None, 0, nodes, weights, *tail) == -8
    assert call(1, 3, 0, 1, 6, 4, None, 33, nodes, weights, *tail) == -8 and call(1, 3, 0, 1, 6, 4, None, 20, None, weights, *tail) == -9
    assert call(1, 3, 0, 1, 6, 4, None, 20, nodes, None, *tail) == -10 and call(0, 3, 5, 1, 6, 4, None, 20, nodes, weights, *tail) == 0
    out = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((2, 5), (2, 3, 5, 6), (2, 3, 5, 6, 6))]
    assert call(2, 3, 0, 5, 6, 4, None, 20, nodes, weights, *([None] * 6), 0, None, None, None, 0, *[_lib.ptr(o) for o in out]) == 0
    torch.cuda.synchronize()
    assert all(float(o.abs().max()) == 0.0 for o in out), "N = 0: every output is zero"
    assert call(2, 3, 0, 5, 6, 4, None, 20, nodes, weights, *([None] * 6), 3, None, None, None, 0, *[_lib.ptr(o) for o in out]) == -17
    assert call(2, 3, 0, 5, 6, 4, None, 20, nodes, weights, *([None] * 6), 0, None, None, None, 0, _lib.ptr(out[0]), None, _lib.ptr(out[2])) == -23
    assert call(2, 3, 0, 5, 6, 4, None, 20, nodes, weights, *([None] * 6), 0, None, None, None, 0, _lib.ptr(out[0]), _lib.ptr(out[1]), None) == -24


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lat,lik", [(3, 4), (2, 5)])
def test_a_corrupt_tile_table_gives_wrong_numbers_at_most(lat, lik, dtype):
    ref = reference(lat, lik, 20, 18, dtype == torch.float32)
    tiles, tile_seg, seg_tile = tile_table(ref["offsets"])
    rng = np.random.default_rng(5)
    wild = np.array([-1, -2 ** 40, 15, 2 ** 40, 2 ** 62, 14, 7, -7], dtype=np.int64)
    for seg_table, tile_first in ((np.resize(wild, tiles), seg_tile), (tile_seg, np.resize(wild, seg_tile.size)),
                                  (rng.permutation(tile_seg), seg_tile[::-1].copy()),
                                  (np.zeros(tiles, dtype=np.int64), np.zeros(seg_tile.size, dtype=np.int64))):
        rc, outs = launch(lik, 20, dtype, ref, table=(seg_table, tile_first))          # (launch checks every guard region)
        assert rc == 0 and all(o is not None for o in outs)
