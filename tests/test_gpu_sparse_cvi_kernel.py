"""
GPU tests of ``mf_lik_sparse_cvi_site_update_*`` (csrc/mf_lik.hip) through the raw C ABI, against the numpy statement of its
formulas in tests/helpers/sparse_cvi_closed_forms.py (``segment_update``).

Tolerances, in the scheme of tests/test_gpu_likelihoods.py.
  float64: ``|err| <= K eps (magnitude + 1)``, eps = 2^-52, K = 64, with the helper's magnitudes: for the sites
    |nat| + sum_k |g| |w_i| |w_j| and |nat| + sum_k |g1| |w_i| (|g| the helper's sums of absolute quadrature terms), for the per-point
    outputs sum |w_i| |m_i|, |c| + sum |w_i| |S_ij| |w_j| and the expectation's own magnitude.  check() prints every ratio
    ("RATIO f64 ...").  Measured maxima on an MI355X over all the cases of this file: nat1 1.44, nat2 4.40, fmu 1.19,
    fvar 3.10, ve 16.85 (ve inherits fvar's rounding through dVE/dvar).
  float32: the kernel's error, normalised by (magnitude + 1) and maximised over the outputs, against 4 x the same figure of the helper
    evaluated in numpy float32 on the same (float32-rounded) inputs; both errors are taken against the float64 helper.  Measured: at
    most 3.5 x (ve; nat1 3.3 x, nat2 2.6 x), the largest normalised error 4.7e-6.

Every series has N = 195 points in S = 5 segments whose lengths are drawn from {0, 1, 63, 64, 65, 130} (tiles are 64 points: both
sides of a tile, an empty segment, a multi-tile segment); further layouts put all the points into one segment, or have no points.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import likelihood_closed_forms as L
from helpers import sparse_cvi_closed_forms as SC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
K_F64 = 64.0
NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
DTYPES = [torch.float64, torch.float32]
GUARD, SENTINEL = 64, -77.25
LAYOUT = ((0, 1, 64, 130, 0), (65, 130, 0, 0, 0), (63, 1, 1, 65, 65))      # three series, N = 195 each
ONE_SEGMENT = ((0, 195, 0),)
OUTS = ("fmu", "fvar", "ve")
FN = "mf_lik_sparse_cvi_site_update"


def np_dtype(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


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


@functools.lru_cache(maxsize=None)
def reference(name, nq, two_d, f32, layout=LAYOUT, lr=0.25):
    """Inputs (rounded to the dtype under test) and the float64 helper on them, per series - computed once per case and shared,
    read-only.  S_pair is a random SPD matrix and c > 0: fvar > 0 by construction."""
    rng = np.random.default_rng(two_d * 100 + nq)
    dt = np.float32 if f32 else np.float64
    rnd = lambda a: np.asarray(a).astype(dt).astype(np.float64)          # noqa: E731
    bsz, segs, n = len(layout), len(layout[0]), int(np.sum(layout[0]))
    ref = dict(offsets=np.stack([np.concatenate([[0], np.cumsum(ln)]) for ln in layout]).astype(np.int64))
    ref["w"] = rnd(rng.uniform(-0.7, 0.7, size=(bsz, n, two_d)))
    ref["c"] = rnd(rng.uniform(0.05, 0.5, size=(bsz, n)))
    a = rng.normal(size=(bsz, segs, two_d, two_d))
    ref["pair_cov"] = rnd(a @ a.transpose(0, 1, 3, 2) / two_d + 0.1 * np.eye(two_d))
    ref["pair_mean"] = rnd(rng.normal(size=(bsz, segs, two_d)))
    ref["y"] = rnd(np.resize(np.asarray(L.OBSERVED[name]), (bsz, n)))
    ref["nat1"] = rnd(rng.normal(size=(bsz, segs, two_d)))
    ref["nat2"] = rnd(-0.5 - rng.random(size=(bsz, segs, two_d, two_d)))
    per = lambda b, dtype: SC.segment_update(L.LIKELIHOODS[name], ref["w"][b], ref["c"][b], ref["y"][b], ref["offsets"][b],   # noqa: E731
                                             ref["pair_mean"][b], ref["pair_cov"][b], lr, ref["nat1"][b], ref["nat2"][b], nq, dtype)
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


def guarded(values, dtype):
    """A buffer holding ``values`` (or, given a shape, the sentinel) followed by a sentinel-filled guard region."""
    shape = values if isinstance(values, tuple) else np.asarray(values).shape
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    if not isinstance(values, tuple):
        buf[:n] = dev(values, dtype).reshape(-1)
    return buf, buf[:n].view(shape)


def guard_intact(buf):
    return bool(torch.all(buf[-GUARD:] == SENTINEL))


def launch(name, nq, dtype, ref, series=None, lr=0.25, update=True, want=(True, True, True)):
    """One launch on all the series of ``ref`` (or on ``series`` alone).  Returns ``(rc, nat1, nat2, [fmu, fvar, ve])`` as tensors
    (None where not asked for) after checking every guard region."""
    pick = (lambda a: a) if series is None else (lambda a: a[series:series + 1])
    bsz, n, two_d = pick(ref["w"]).shape
    segs = ref["offsets"].shape[1] - 1
    seg = torch.tensor(pick(ref["offsets"]), dtype=torch.int64, device=DEV).contiguous()
    ins = [dev(pick(ref[k]), dtype) for k in ("w", "c", "y", "pair_mean", "pair_cov")]
    nat = [guarded(pick(ref[k]), dtype) if update else (None, None) for k in ("nat1", "nat2")]
    outs = [guarded((bsz, n), dtype) if w else (None, None) for w in want]
    nodes, weights = c_rule(nq)
    rc = _lib.call_rc(FN, dtype, bsz, n, segs, two_d, L.IDS[name], c_params(name), nq, nodes, weights, _lib.ptr(seg),
                      *[_lib.ptr(t) for t in ins], lr, _lib.ptr(nat[0][1]), _lib.ptr(nat[1][1]), *[_lib.ptr(o[1]) for o in outs],
                      _lib.stream_ptr(DEV))
    assert all(b[0] is None or guard_intact(b[0]) for b in nat + outs), "a write past the end of an output"
    return rc, nat[0][1], nat[1][1], [o[1] for o in outs]


def check(what, got, want, mag, dtype, got32=None):
    """float64: the K eps bound; float32: 4 x the normalised error of the numpy float32 evaluation.  Prints the figure first."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    scaled = np.abs(got - want) / (np.asarray(mag) + 1.0)
    if dtype == torch.float64:
        ratio = float(scaled.max() / EPS)
        print(f"RATIO f64 {what}: {ratio:.2f}")
        assert ratio <= K_F64, f"{what}: {ratio:.1f} eps (magnitude + 1) at {np.unravel_index(int(scaled.argmax()), scaled.shape)}"
    else:
        own = float((np.abs(np.asarray(got32, dtype=np.float64) - want) / (np.asarray(mag) + 1.0)).max())
        print(f"ERR f32 {what}: kernel {scaled.max():.3e}  numpy float32 {own:.3e}")
        assert scaled.max() <= 4.0 * own, f"{what}: kernel {scaled.max():.3e} against numpy float32 {own:.3e}"


def check_against_helper(tag, ref, dtype, nat1, nat2, outs, series=None):
    f32 = dtype == torch.float32
    for i, b in enumerate(range(len(ref["want"])) if series is None else [series]):
        want = ref["want"][b]
        own = ref["want32"][b] if f32 else {}
        for key, got in (("nat1", nat1), ("nat2", nat2)) + tuple(zip(OUTS, outs)):
            if got is not None:
                check(f"{tag} series {b} {key}", got[i].cpu().numpy(), want[key], want["mag_" + key], dtype, own.get(key))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("two_d", [2, 4, 6, 8, 10, 12, 14, 16, 18])
@pytest.mark.parametrize("name", NAMES)
def test_batch_of_three_against_the_helper_and_each_series_alone_bit_for_bit(name, two_d, dtype):
    ref = reference(name, 20, two_d, dtype == torch.float32)
    rc, nat1, nat2, outs = launch(name, 20, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} 2d={two_d}", ref, dtype, nat1, nat2, outs)
    again = launch(name, 20, dtype, ref)
    assert torch.equal(again[1], nat1) and torch.equal(again[2], nat2), "two launches on the same inputs return the same bits"
    assert all(torch.equal(a, b) for a, b in zip(again[3], outs))
    for b in range(3):
        rc, one1, one2, one_outs = launch(name, 20, dtype, ref, series=b)
        assert rc == 0
        assert torch.equal(one1[0], nat1[b]) and torch.equal(one2[0], nat2[b]), "a series alone gives the bits it gives in a batch"
        assert all(torch.equal(o[0], f[b]) for o, f in zip(one_outs, outs))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nq", [1, 32])
@pytest.mark.parametrize("name", NAMES)
def test_quadrature_rules_of_one_and_of_thirty_two_nodes_on_single_series(name, nq, dtype):
    ref = reference(name, nq, 6, dtype == torch.float32)
    for b in range(3):
        rc, nat1, nat2, outs = launch(name, nq, dtype, ref, series=b)
        assert rc == 0
        check_against_helper(f"{name} nq={nq} B=1", ref, dtype, nat1, nat2, outs, series=b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_all_points_in_one_segment_with_unit_learning_rate(name, dtype):
    """195 points = three full tiles and one of three points behind one accumulator; lr = 1 forgets the old sites, and the two empty
    segments become exactly zero."""
    ref = reference(name, 20, 12, dtype == torch.float32, layout=ONE_SEGMENT, lr=1.0)
    rc, nat1, nat2, outs = launch(name, 20, dtype, ref, lr=1.0)
    assert rc == 0
    check_against_helper(f"{name} one segment", ref, dtype, nat1, nat2, outs)
    assert float(nat1[0, 0].abs().max()) == 0.0 and float(nat2[0, 2].abs().max()) == 0.0


def test_no_points_decays_the_sites_and_no_series_launches_nothing():
    dtype = torch.float64
    ref = dict(reference(L.BERNOULLI, 20, 4, False))
    ref.update(w=ref["w"][:2, :0], c=ref["c"][:2, :0], y=ref["y"][:2, :0], offsets=np.zeros((2, 6), dtype=np.int64),
               **{k: ref[k][:2] for k in ("pair_mean", "pair_cov", "nat1", "nat2")})
    rc, nat1, nat2, _ = launch(L.BERNOULLI, 20, dtype, ref, lr=0.25)
    assert rc == 0
    np.testing.assert_array_equal(nat1.cpu().numpy(), 0.75 * ref["nat1"])
    np.testing.assert_array_equal(nat2.cpu().numpy(), 0.75 * ref["nat2"])
    nodes, weights = c_rule(20)
    s = _lib.stream_ptr(DEV)
    assert _lib.call_rc(FN, dtype, 0, 5, 3, 4, 1, None, 20, nodes, weights, *([None] * 6), 0.5, *([None] * 5), s) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_projection_only_mode_and_null_combinations_of_the_optional_outputs(dtype):
    ref = reference(L.BERNOULLI, 20, 6, dtype == torch.float32)
    rc, nat1, nat2, full = launch(L.BERNOULLI, 20, dtype, ref)
    assert rc == 0
    for mask in range(8):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        rc, n1, n2, got = launch(L.BERNOULLI, 20, dtype, ref, update=False, want=want)
        assert rc == 0 and n1 is None and n2 is None
        for g, f, w in zip(got, full, want):
            assert (g is None) == (not w) and (g is None or torch.equal(g, f)), "projection only: the update's own per-point outputs"
        rc, n1, n2, got = launch(L.BERNOULLI, 20, dtype, ref, update=True, want=want)
        assert rc == 0 and torch.equal(n1, nat1) and torch.equal(n2, nat2)
        assert all(g is None or torch.equal(g, f) for g, f in zip(got, full))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_a_bad_variance_poisons_its_own_segment_and_leaves_the_others_bit_identical(name, dtype):
    ref = dict(reference(name, 20, 6, dtype == torch.float32))
    clean = launch(name, 20, dtype, ref)
    c = ref["c"].copy()
    # series 0: point 70 of segment 3 (its second tile); series 2: the single point of segment 1 and a point of segment 4
    bad = [(0, 65 + 70, -1e6), (2, 63, float("nan")), (2, 63 + 1 + 1 + 65 + 5, -1e6)]
    for b, k, v in bad:
        c[b, k] = v
    ref["c"] = c
    rc, nat1, nat2, outs = launch(name, 20, dtype, ref)
    assert rc == 0
    poisoned = {(0, 3), (2, 1), (2, 4)}
    for b in range(3):
        for s in range(5):
            if (b, s) in poisoned:
                assert bool(torch.isnan(nat1[b, s]).all()) and bool(torch.isnan(nat2[b, s]).all()), "its segment's sites are NaN"
            else:
                assert torch.equal(nat1[b, s], clean[1][b, s]) and torch.equal(nat2[b, s], clean[2][b, s])
    good = torch.ones((3, 195), dtype=torch.bool, device=DEV)
    for b, k, _ in bad:
        good[b, k] = False
    for o, f in zip(outs, clean[3]):
        assert bool(torch.isnan(o[~good]).all()), "a point outside the domain comes out NaN"
        assert torch.equal(o[good], f[good]), "every other point keeps its bits"


def test_bad_arguments_return_their_codes_and_launch_nothing():
    dtype = torch.float64
    ref = reference(L.STUDENTT, 20, 4, False)
    seg = torch.tensor(ref["offsets"], dtype=torch.int64, device=DEV)
    ins = [dev(ref[k], dtype) for k in ("w", "c", "y", "pair_mean", "pair_cov")]
    io = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((3, 5, 4), (3, 5, 4, 4), (3, 195), (3, 195), (3, 195))]
    nodes, weights = c_rule(20)
    par, s = c_params(L.STUDENTT), _lib.stream_ptr(DEV)
    p, o = [_lib.ptr(seg)] + [_lib.ptr(t) for t in ins], [_lib.ptr(t) for t in io]

    def call(bsz=3, n=195, segs=5, two_d=4, lik=3, params=par, nq=20, nd=nodes, wt=weights, ptrs=p, lr=0.5, outs=o):
        return _lib.call_rc(FN, dtype, bsz, n, segs, two_d, lik, params, nq, nd, wt, *ptrs, lr, *outs, s)

    assert call(bsz=-1) == -1 and call(n=-1) == -2 and call(segs=0) == -3
    for two_d in (0, 1, 3, 5, 20, -2):
        assert call(two_d=two_d) == -100
    assert call(lik=7) == -5 and call(params=None) == -6 and call(nq=0) == -7 and call(nq=33) == -7
    assert call(nd=None) == -8 and call(wt=None) == -9
    for i in range(6):
        assert call(ptrs=p[:i] + [None] + p[i + 1:]) == -(10 + i)
    assert call(lr=1.5) == -16 and call(lr=-0.1) == -16 and call(lr=float("nan")) == -16
    assert call(outs=[None] + o[1:]) == -17 and call(outs=o[:1] + [None] + o[2:]) == -18
    assert call(outs=[None] * 5) == 0                                   # nothing asked for
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in io)
    with pytest.raises(NotImplementedError):
        _lib.call(FN, dtype, 3, 195, 5, 20, 3, par, 20, nodes, weights, *p, 0.5, *o, s)
    with pytest.raises(ValueError, match="invalid argument #7"):
        _lib.call(FN, dtype, 3, 195, 5, 4, 3, par, 40, nodes, weights, *p, 0.5, *o, s)
