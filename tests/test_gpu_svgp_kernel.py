"""
GPU tests of ``mf_lik_sparse_expectations_*`` (csrc/mf_lik.hip) through the raw C ABI, against the numpy statement of its formulas
in tests/helpers/svgp_closed_forms.py (``segment_expectations``).

Tolerances, in the scheme of tests/test_gpu_sparse_cvi_kernel.py.
  float64: ``|err| <= K eps (magnitude + 1)``, eps = 2^-52, K = 64, with the helper's magnitudes: sum_k |gv| |w_i| |w_j| for g_cov,
    sum_k |gm| |w_i| for g_mean and the sum of the expectations' own magnitudes for ve_sum.  check() prints every ratio
    ("RATIO f64 ...").  Measured maxima on an MI355X over all the cases of this file: ve_sum 1.78, g_mean 5.23, g_cov 5.83.
  float32: the kernel's error, normalised by (magnitude + 1) and maximised over an output of one series, against 4 x the same figure
    of the helper evaluated in numpy float32 on the same (float32-rounded) inputs; the helper projects and sums in the kernel's order
    (tiles of 64 points in ascending order, then the tiles), and both errors are taken against the float64 helper.  Measured per
    series on an MI355X: g_mean at most 3.44 x, g_cov 2.30 x, the largest normalised error 1.8e-6 (in several Poisson
    cases g_mean and g_cov are the helper's very bits).
    ve_sum is the exception: its maximum is taken over the three series of a launch together.  Per series it has five segment sums,
    up to two of them empty, and the kernel's expf / lgammaf are good to an ulp or two where numpy's float32 exp and gammaln are
    computed in double and rounded once.  In two of the float32 launches the kernel's ve_sum error of one series is 1.4 - 1.8 eps32
    (magnitude + 1) while the helper lands within 0.35 eps32, and the ratio is 4.83 x (Poisson, 2d = 6, series 0:
    1.69e-7 against 3.49e-8) and 5.26 x (Poisson, nq = 32, series 1: 2.18e-7 against 4.14e-8); over the launch those are 2.17 x and
    1.51 x, and the worst launch is 3.23 x (Bernoulli, nq = 32).

Every series has N = 390 points in S = 5 segments whose lengths are drawn from {0, 1, 3, 63, 64, 65, 130, 195}: a tile is 64 points, so
segments of one, two, three and four tiles are combined, both sides of a tile boundary are met and segments are empty.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import likelihood_closed_forms as L
from helpers import svgp_closed_forms as SV

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
K_F64 = 64.0
NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
DTYPES = [torch.float64, torch.float32]
GUARD, SENTINEL = 64, -77.25
TILE = 64
LAYOUT = ((0, 1, 64, 130, 195), (195, 65, 130, 0, 0), (63, 65, 64, 195, 3))      # three series, N = 390 each
OUTS = ("ve_sum", "g_mean", "g_cov")
FN = "mf_lik_sparse_expectations"


def host_array(values):
    return (ctypes.c_double * len(values))(*values) if len(values) else None


def c_params(name):
    params = L.LIKELIHOODS[name][1]
    if name == L.STUDENTT:
        scale, df = params
        from scipy import special
        const = special.gammaln(0.5 * (df + 1)) - special.gammaln(0.5 * df) - 0.5 * np.log(df * np.pi) - np.log(scale)
        return host_array((scale, df, float(const)))
    return host_array(params)


@functools.lru_cache(maxsize=None)
def c_rule(nq):
    x, w = np.polynomial.hermite.hermgauss(nq)
    return host_array(tuple(x)), host_array(tuple(w))


def tile_table(offsets):
    """``(num_tiles, tile_seg, seg_tile)`` of ``offsets [B, S + 1]``, in plain numpy."""
    per = (np.diff(offsets, axis=1).reshape(-1) + TILE - 1) // TILE
    return int(per.sum()), np.repeat(np.arange(per.size), per).astype(np.int64), np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def reference(name, nq, two_d, f32, layout=LAYOUT):
    """Inputs (rounded to the dtype under test) and the float64 helper on them, per series - computed once per case and shared,
    read-only.  S_pair is a random SPD matrix and c > 0: fvar > 0 by construction."""
    rng = np.random.default_rng(two_d * 100 + nq)
    dt = np.float32 if f32 else np.float64
    rnd = lambda a: np.asarray(a).astype(dt).astype(np.float64)          # noqa: E731
    bsz, segs, n = len(layout), len(layout[0]), int(np.sum(layout[0]))
    assert all(int(np.sum(ln)) == n for ln in layout)
    ref = dict(offsets=np.stack([np.concatenate([[0], np.cumsum(ln)]) for ln in layout]).astype(np.int64))
    ref["w"] = rnd(rng.uniform(-0.7, 0.7, size=(bsz, n, two_d)))
    ref["c"] = rnd(rng.uniform(0.05, 0.5, size=(bsz, n)))
    a = rng.normal(size=(bsz, segs, two_d, two_d))
    ref["pair_cov"] = rnd(a @ a.transpose(0, 1, 3, 2) / two_d + 0.1 * np.eye(two_d))
    ref["pair_mean"] = rnd(rng.normal(size=(bsz, segs, two_d)))
    ref["y"] = rnd(np.resize(np.asarray(L.OBSERVED[name]), (bsz, n)))
    per = lambda b, dtype: SV.segment_expectations(L.LIKELIHOODS[name], ref["w"][b], ref["c"][b], ref["y"][b], ref["offsets"][b],   # noqa: E731
                                                   ref["pair_mean"][b], ref["pair_cov"][b], nq, dtype)
    ref["want"] = [per(b, np.float64) for b in range(bsz)]
    if f32:
        ref["want32"] = [per(b, np.float32) for b in range(bsz)]
    for v in ref.values():
        for a in (v if isinstance(v, list) else [v]):
            for x in (a.values() if isinstance(a, dict) else [a]):
                x.setflags(write=False)
    return ref


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def guarded(shape, dtype):
    """A sentinel-filled buffer of ``shape`` followed by a sentinel-filled guard region."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def launch(name, nq, dtype, ref, series=None, want=(True, True, True)):
    """One call on all the series of ``ref`` (or on ``series`` alone).  Returns ``(rc, [ve_sum, g_mean, g_cov])`` as tensors (None where
    not asked for) after checking every guard region."""
    pick = (lambda a: a) if series is None else (lambda a: a[series:series + 1])
    bsz, n, two_d = pick(ref["w"]).shape
    offsets = pick(ref["offsets"])
    segs = offsets.shape[1] - 1
    tiles, tile_seg, seg_tile = tile_table(offsets)
    table = [torch.tensor(a, dtype=torch.int64, device=DEV).contiguous() for a in (offsets, tile_seg, seg_tile)]
    ins = [dev(pick(ref[k]), dtype) for k in ("w", "c", "y", "pair_mean", "pair_cov")]
    shapes = ((bsz, segs), (bsz, segs, two_d), (bsz, segs, two_d, two_d))
    outs = [guarded(s, dtype) if w else (None, None) for s, w in zip(shapes, want)]
    ws_bytes = int(_lib.load().mf_lik_sparse_expectations_workspace_bytes(tiles, two_d, ins[0].element_size()))
    assert ws_bytes == tiles * (two_d * (two_d + 1) // 2 + two_d + 1) * ins[0].element_size()
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    nodes, weights = c_rule(nq)
    rc = _lib.call_rc(FN, dtype, bsz, n, segs, two_d, L.IDS[name], c_params(name), nq, nodes, weights, _lib.ptr(table[0]),
                      *[_lib.ptr(t) for t in ins], tiles, _lib.ptr(table[1]), _lib.ptr(table[2]), _lib.ptr(ws), ws_bytes,
                      *[_lib.ptr(o[1]) for o in outs], _lib.stream_ptr(DEV))
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
    """Every series and every output on its own, as tests/test_gpu_sparse_cvi_kernel.py does; every figure is printed before the
    first failure is raised.  The one exception is ``ve_sum`` in float32, whose maximum is taken over the launch's series together
    (its per-series figures are still printed): see the module docstring."""
    f32 = dtype == torch.float32
    rows = list(range(len(ref["want"]))) if series is None else [series]
    failures = []
    for i, b in enumerate(rows):
        want = ref["want"][b]
        own = ref["want32"][b] if f32 else {}
        for key, got in zip(OUTS, outs):
            if got is not None:
                assert not bool(torch.any(got[i] == SENTINEL)), f"{tag} series {b} {key}: an element was not written"
                failed = check(f"{tag} series {b} {key}", got[i].cpu().numpy(), want[key], want["mag_" + key], dtype, own.get(key))
                if not (f32 and key == "ve_sum"):
                    failures.append(failed)
    if f32 and outs[0] is not None:
        gather = lambda src, k: np.stack([src[b][k] for b in rows])          # noqa: E731
        failures.append(check(f"{tag} launch ve_sum", outs[0].cpu().numpy(), gather(ref["want"], "ve_sum"),
                              gather(ref["want"], "mag_ve_sum"), dtype, gather(ref["want32"], "ve_sum")))
    failures = [f for f in failures if f]
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("two_d", [2, 4, 6, 8, 10, 12, 14, 16, 18])
@pytest.mark.parametrize("name", NAMES)
def test_batch_of_three_against_the_helper_and_each_series_alone_bit_for_bit(name, two_d, dtype):
    ref = reference(name, 20, two_d, dtype == torch.float32)
    rc, outs = launch(name, 20, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} 2d={two_d}", ref, dtype, outs)
    g_cov = outs[2]
    assert torch.equal(g_cov, g_cov.transpose(-1, -2)), "g_cov is symmetric: both triangles are written from one sum"
    # empty segments: exact zeros
    for b, ln in enumerate(LAYOUT):
        for s, count in enumerate(ln):
            if count == 0:
                assert all(float(o[b, s].abs().max()) == 0.0 for o in outs)
    rc, again = launch(name, 20, dtype, ref)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(again, outs)), "two launches on the same inputs return the same bits"
    for b in range(3):
        rc, one = launch(name, 20, dtype, ref, series=b)
        assert rc == 0
        assert all(torch.equal(o[0], f[b]) for o, f in zip(one, outs)), "a series alone gives the bits it gives in a batch"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nq", [1, 32])
@pytest.mark.parametrize("name", NAMES)
def test_quadrature_rules_of_one_and_of_thirty_two_nodes(name, nq, dtype):
    ref = reference(name, nq, 6, dtype == torch.float32)
    rc, outs = launch(name, nq, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} nq={nq}", ref, dtype, outs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("two_d", [6, 18])
def test_value_only_mode_and_gradients_without_the_value_return_the_same_bits(two_d, dtype):
    ref = reference(L.BERNOULLI, 20, two_d, dtype == torch.float32)
    rc, full = launch(L.BERNOULLI, 20, dtype, ref)
    assert rc == 0
    rc, value = launch(L.BERNOULLI, 20, dtype, ref, want=(True, False, False))
    assert rc == 0 and value[1] is None and value[2] is None and torch.equal(value[0], full[0])
    rc, grads = launch(L.BERNOULLI, 20, dtype, ref, want=(False, True, True))
    assert rc == 0 and grads[0] is None and torch.equal(grads[1], full[1]) and torch.equal(grads[2], full[2])


def test_no_points_writes_zeros_and_no_series_launches_nothing():
    dtype = torch.float64
    ref = dict(reference(L.BERNOULLI, 20, 4, False))
    ref.update(w=ref["w"][:2, :0], c=ref["c"][:2, :0], y=ref["y"][:2, :0], offsets=np.zeros((2, 6), dtype=np.int64),
               **{k: ref[k][:2] for k in ("pair_mean", "pair_cov")})
    rc, outs = launch(L.BERNOULLI, 20, dtype, ref)
    assert rc == 0
    assert all(float(o.abs().max()) == 0.0 for o in outs), "N = 0: every output is zero"
    nodes, weights = c_rule(20)
    s = _lib.stream_ptr(DEV)
    # N = 0 needs no input, no table and no workspace
    out = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((2, 5), (2, 5, 4), (2, 5, 4, 4))]
    assert _lib.call_rc(FN, dtype, 2, 0, 5, 4, 1, None, 20, nodes, weights, *([None] * 6), 0, None, None, None, 0,
                        *[_lib.ptr(o) for o in out], s) == 0
    assert all(float(o.abs().max()) == 0.0 for o in out)
    assert _lib.call_rc(FN, dtype, 0, 5, 3, 4, 1, None, 20, nodes, weights, *([None] * 6), 0, None, None, None, 0, None, None, None, s) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_a_bad_variance_poisons_its_own_segment_and_leaves_the_others_bit_identical(name, dtype):
    ref = dict(reference(name, 20, 6, dtype == torch.float32))
    rc, clean = launch(name, 20, dtype, ref)
    assert rc == 0
    c = ref["c"].copy()
    # series 0: point 70 of the 130 of segment 3 (its second tile); series 2: a NaN in segment 0 and a point of the last segment
    bad = [(0, 65 + 70, -1e6), (2, 5, float("nan")), (2, 63 + 65 + 64 + 195 + 1, -1e6)]
    for b, k, v in bad:
        c[b, k] = v
    ref["c"] = c
    rc, outs = launch(name, 20, dtype, ref)
    assert rc == 0
    poisoned = {(0, 3), (2, 0), (2, 4)}
    for b in range(3):
        for s in range(5):
            for o, f in zip(outs, clean):
                if (b, s) in poisoned:
                    assert bool(torch.isnan(o[b, s]).all()), "every output of its segment is NaN"
                else:
                    assert torch.equal(o[b, s], f[b, s]), "every other segment keeps its bits"


def test_bad_arguments_return_their_codes_and_launch_nothing():
    dtype = torch.float64
    ref = reference(L.STUDENTT, 20, 4, False)
    tiles, tile_seg, seg_tile = tile_table(ref["offsets"])
    table = [torch.tensor(a, dtype=torch.int64, device=DEV) for a in (ref["offsets"], tile_seg, seg_tile)]
    ins = [dev(ref[k], dtype) for k in ("w", "c", "y", "pair_mean", "pair_cov")]
    io = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((3, 5), (3, 5, 4), (3, 5, 4, 4))]
    ws_bytes = tiles * 15 * 8
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    nodes, weights = c_rule(20)
    par, s = c_params(L.STUDENTT), _lib.stream_ptr(DEV)
    p = [_lib.ptr(table[0])] + [_lib.ptr(t) for t in ins]
    tb, o = [_lib.ptr(table[1]), _lib.ptr(table[2]), _lib.ptr(ws)], [_lib.ptr(t) for t in io]

    def call(bsz=3, n=390, segs=5, two_d=4, lik=3, params=par, nq=20, nd=nodes, wt=weights, ptrs=p, nt=tiles, tab=tb, nbytes=ws_bytes,
             outs=o):
        return _lib.call_rc(FN, dtype, bsz, n, segs, two_d, lik, params, nq, nd, wt, *ptrs, nt, *tab, nbytes, *outs, s)

    assert call(bsz=-1) == -1 and call(n=-1) == -2 and call(segs=0) == -3
    for two_d in (0, 1, 3, 5, 20, -2):
        assert call(two_d=two_d) == -100
    assert call(lik=7) == -5 and call(params=None) == -6 and call(nq=0) == -7 and call(nq=33) == -7
    assert call(nd=None) == -8 and call(wt=None) == -9
    for i in range(6):
        assert call(ptrs=p[:i] + [None] + p[i + 1:]) == -(10 + i)
    assert call(nt=-1) == -16 and call(nt=2 ** 31) == -16 and call(n=0) == -16          # tiles without points
    for i in range(3):
        assert call(tab=tb[:i] + [None] + tb[i + 1:]) == -(17 + i)
    assert call(nbytes=ws_bytes - 1) == -20 and call(nbytes=0) == -20
    assert call(outs=[o[0], None, o[2]]) == -22 and call(outs=[o[0], o[1], None]) == -23
    assert call(outs=[None] * 3) == 0                                   # nothing asked for
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in io)
    assert int(_lib.load().mf_lik_sparse_expectations_workspace_bytes(0, 4, 8)) == 0
    assert int(_lib.load().mf_lik_sparse_expectations_workspace_bytes(7, 5, 8)) == 0
    with pytest.raises(NotImplementedError):
        _lib.call(FN, dtype, 3, 390, 5, 20, 3, par, 20, nodes, weights, *p, tiles, *tb, ws_bytes, *o, s)
    with pytest.raises(ValueError, match="invalid argument #7"):
        _lib.call(FN, dtype, 3, 390, 5, 4, 3, par, 40, nodes, weights, *p, tiles, *tb, ws_bytes, *o, s)
