"""
GPU tests of ``mf_lik_sparse_pep_site_update_*`` (csrc/mf_lik.hip) through the raw C ABI, against the numpy statement of its two
passes in tests/helpers/sparse_pep_closed_forms.py (``segment_pep_update``).

Tolerances, in the scheme of tests/test_gpu_svgp_kernel.py.
  float64: ``|err| <= K eps (magnitude + 1)``, eps = 2^-52, K = 64, with the helper's magnitudes.  ``fmu`` and ``fvar`` are checked
    first, against the helper's projection; everything behind them is checked against the helper evaluated AT the kernel's own
    ``(fmu, fvar)`` (the helper's ``at=``), so that the sensitivity of I, g1, g2 to a rounding of the projection - third derivatives -
    does not have to be bounded.  check() prints every ratio ("RATIO f64 ...").
  float32: the kernel's error, normalised by (magnitude + 1) and maximised over an output of one LAUNCH, against 4 x the same figure
    of the helper evaluated in numpy float32 on the same (float32-rounded) inputs; both errors are taken against the float64 helper.
    The maximum runs over the launch and not over a series because a series has four segment sums, some of them empty, and numpy's
    float32 exp / erf / lgamma are computed in double and rounded once where the kernel's are good to an ulp or two: over so few
    numbers the helper's own error can be a fraction of an ulp (tests/test_gpu_svgp_kernel.py meets the same with ``ve_sum``).  For
    the same reason the one-point shape (1, 1, 2) is run on sixteen draws and judged on their maxima.
  Inputs are ``sparse_pep_closed_forms.random_case``: fvar below about 0.4, where 1 + fvar g2 >= 0.1 for all four likelihoods; the
  reference asserts that the helper defines every point, in both dtypes.

Measured maxima on an MI355X over all the cases of this file: CHANGELOG.md.

The main layout is (B, N, S) = (3, 130, 4) with the segment lengths 0, 1, 63, 64, 65 and 129: a tile is 64 points, so segments of one,
two and three tiles are combined, both sides of a tile boundary are met and segments are empty.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import likelihood_closed_forms as L
from helpers import sparse_cvi_closed_forms as SC
from helpers import sparse_pep_closed_forms as SP

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
K_F64 = 64.0
NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
DTYPES = [torch.float64, torch.float32]
GUARD, SENTINEL = 64, -77.25
TILE = 64
LAYOUT = ((0, 1, 65, 64), (63, 2, 0, 65), (129, 0, 1, 0))      # three series, N = 130 each
SITES = ("nat1", "nat2", "log_norm")
POINTS = ("fmu", "fvar", "led")
FN = "mf_lik_sparse_pep_site_update"
M52_M52 = [dict(order=5, ls=1.0, var=1.0, period=None, osc=0), dict(order=5, ls=3.0, var=0.5, period=None, osc=0)]


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
def c_rule(nq=20):
    x, w = np.polynomial.hermite.hermgauss(nq)
    return host_array(tuple(x)), host_array(tuple(w))


def tile_table(offsets):
    """``(num_tiles, tile_seg, seg_tile)`` of ``offsets [B, S + 1]``, in plain numpy."""
    per = (np.diff(offsets, axis=1).reshape(-1) + TILE - 1) // TILE
    return int(per.sum()), np.repeat(np.arange(per.size), per).astype(np.int64), np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


def helper(name, ref, b, alpha, lr, dtype=np.float64, at=None):
    return SP.segment_pep_update(L.LIKELIHOODS[name], ref["w"][b], ref["c"][b], ref["y"][b], ref["offsets"][b], ref["cav_mean"][b],
                                 ref["cav_cov"][b], alpha, lr, ref["nat1"][b], ref["nat2"][b], ref["log_norm"][b], ref["seg_const"][b],
                                 20, dtype, at)


def freeze(ref):
    for v in ref.values():
        for a in (v if isinstance(v, list) else [v]):
            for x in (a.values() if isinstance(a, dict) else [a]):
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)
    return ref


def finish(name, ref, f32, alpha, lr):
    """Round the inputs to the dtype under test and add the float64 helper (and the numpy float32 one) per series."""
    dt = np.float32 if f32 else np.float64
    for k in ("w", "c", "y", "cav_mean", "cav_cov", "nat1", "nat2", "log_norm", "seg_const"):
        ref[k] = np.asarray(ref[k]).astype(dt).astype(np.float64)
    bsz = ref["w"].shape[0]
    ref["want"] = [helper(name, ref, b, alpha, lr) for b in range(bsz)]
    assert not any(w["skipped"].any() for w in ref["want"]) and all(np.isfinite(w["led"]).all() for w in ref["want"])
    if f32:
        ref["want32"] = [helper(name, ref, b, alpha, lr, np.float32) for b in range(bsz)]
        assert not any(w["skipped"].any() for w in ref["want32"])
    return freeze(ref)


@functools.lru_cache(maxsize=None)
def reference(name, two_d, f32, alpha=0.5, lr=0.5, layout=LAYOUT, seed=0):
    """Inputs and the helper on them - computed once per case and shared, read-only."""
    return finish(name, SP.random_case(name, two_d, layout, seed), f32, alpha, lr)


@functools.lru_cache(maxsize=None)
def matern_reference(f32, alpha, lr):
    """2d = 12 with the projections of Sum(Matern52, Matern52), the kernel of the benchmarks: 130 points on [0, 6.5] per series, three
    inducing points, the cavity a shrunk prior pair marginal (fvar up to about 1.3), Bernoulli observations."""
    rng = np.random.default_rng(12)
    ref = SP.random_case(L.BERNOULLI, 12, ((40, 30, 45, 15), (0, 66, 0, 64)))
    z = [np.array([2.0, 3.5, 5.75]), np.array([-1.0, 3.3, 3.4])]
    pinf = SC._transition(M52_M52, 1.0)[2]
    for b, ln in enumerate(((40, 30, 45, 15), (0, 66, 0, 64))):
        edges = np.concatenate([[0.0], z[b], [6.5]])
        x = np.sort(np.concatenate([rng.uniform(max(lo, 0.0) + 1e-3, hi, size=k) for lo, hi, k in zip(edges[:-1], edges[1:], ln) if k]))
        idx, ref["w"][b], ref["c"][b] = SC.conditional_projections(M52_M52, x, z[b])
        assert np.array_equal(SC.offsets_of(idx, 4), ref["offsets"][b])
        kuu = SC.dense_state_prior(M52_M52, z[b])
        ref["cav_cov"][b] = 0.25 * SC.pair_marginals(np.zeros(kuu.shape[0]), kuu, pinf, 6)[1]
    return finish(L.BERNOULLI, ref, f32, alpha, lr)


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def guarded(shape, dtype, fill=None):
    """A buffer of ``shape`` (sentinel-filled, or a copy of ``fill``) followed by a sentinel-filled guard region."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    if fill is not None:
        buf[:n] = dev(fill, dtype).reshape(-1)
    return buf, buf[:n].view(shape)


def launch(name, dtype, ref, alpha=0.5, lr=0.5, series=None, update=True, outputs=True, table=None, const=True):
    """One call on all the series of ``ref`` (or on ``series`` alone).  Returns ``(rc, dict)`` with the three site tensors (update
    mode), ``led_sum`` and the per-point outputs as tensors, after checking every guard region."""
    pick = (lambda a: a) if series is None else (lambda a: a[series:series + 1])
    bsz, n, two_d = pick(ref["w"]).shape
    offsets = pick(ref["offsets"])
    segs = offsets.shape[1] - 1
    tiles, tile_seg, seg_tile = tile_table(offsets) if table is None else table
    tab = [torch.tensor(a, dtype=torch.int64, device=DEV).contiguous() for a in (offsets, tile_seg, seg_tile)]
    ins = [dev(pick(ref[k]), dtype) for k in ("w", "c", "y", "cav_mean", "cav_cov")]
    seg_const = dev(pick(ref["seg_const"]), dtype) if const else None
    bufs = {}
    if update:
        for k, shape in zip(SITES, ((bsz, segs, two_d), (bsz, segs, two_d, two_d), (bsz, segs))):
            bufs[k] = guarded(shape, dtype, pick(ref[k]))
    if outputs:
        bufs["led_sum"] = guarded((bsz, segs), dtype)
        for k in POINTS:
            bufs[k] = guarded((bsz, n), dtype)
    ws_bytes = int(_lib.load().mf_lik_sparse_expectations_workspace_bytes(tiles, two_d, ins[0].element_size()))
    assert ws_bytes == max(tiles, 0) * (two_d * (two_d + 1) // 2 + two_d + 1) * ins[0].element_size()
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    nodes, weights = c_rule()
    p = lambda k: _lib.ptr(bufs[k][1]) if k in bufs else None          # noqa: E731
    rc = _lib.call_rc(FN, dtype, bsz, n, segs, two_d, L.IDS[name], c_params(name), 20, nodes, weights, alpha, lr, _lib.ptr(tab[0]),
                      *[_lib.ptr(t) for t in ins], _lib.ptr(seg_const), tiles, _lib.ptr(tab[1]), _lib.ptr(tab[2]), _lib.ptr(ws), ws_bytes,
                      *[p(k) for k in SITES], p("led_sum"), *[p(k) for k in POINTS], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert all(bool(torch.all(b[0][-GUARD:] == SENTINEL)) for b in bufs.values()), "a write past the end of an output"
    assert bool(torch.all(ws[ws_bytes:] == 0x5A)), "a write past the end of the workspace"
    return rc, {k: b[1] for k, b in bufs.items()}


def check(what, got, want, mag):
    """float64: the K eps bound.  Prints the figure, returns the failure as text or None."""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    scaled = np.abs(got - want) / (np.asarray(mag) + 1.0)
    ratio = (float(scaled.max()) if scaled.size else 0.0) / EPS
    print(f"RATIO f64 {what}: {ratio:.2f}")
    if ratio > K_F64:
        return f"{what}: {ratio:.1f} eps (magnitude + 1) at {np.unravel_index(int(scaled.argmax()), scaled.shape)}"
    return None


def float32_errors(ref, out, rows):
    """Per output of a float32 launch: the kernel's and the numpy float32 helper's largest error normalised by (magnitude + 1), both
    against the float64 helper."""
    stack = lambda src, field: np.stack([np.asarray(src[b][field], dtype=np.float64) for b in rows])          # noqa: E731
    errs = {}
    for k in [k for k in SITES + ("led_sum",) + POINTS if k in out]:
        got = out[k].cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(got)), f"{k}: non-finite result"
        want, mag = stack(ref["want"], k), stack(ref["want"], "mag_" + k) + 1.0
        errs[k] = (float((np.abs(got - want) / mag).max()), float((np.abs(stack(ref["want32"], k) - want) / mag).max()))
    return errs


def check_float32(tag, errs):
    """4 x the numpy float32 evaluation's figure; prints every figure, returns the failures as text."""
    failures = []
    for k, (top, own) in errs.items():
        print(f"ERR f32 {tag} {k}: kernel {top:.3e}  numpy float32 {own:.3e}  ({top / own if own else float(top > 0):.2f} x)")
        if top > 4.0 * own:
            failures.append(f"{tag} {k}: kernel {top:.3e} against numpy float32 {own:.3e}")
    return failures


def check_against_helper(tag, name, ref, dtype, out, alpha, lr):
    """Every output of the launch; every figure is printed before the first failure is raised."""
    rows = list(range(len(ref["want"])))
    keys = [k for k in SITES + ("led_sum",) + POINTS if k in out]
    for k in ("led_sum",) + POINTS:
        if k in out:
            assert not bool(torch.any(out[k] == SENTINEL)), f"{tag} {k}: an element was not written"
    failures = []
    if dtype == torch.float32:
        failures = check_float32(tag, float32_errors(ref, out, rows))
    else:
        got = {k: out[k].cpu().numpy().astype(np.float64) for k in keys}
        for b in rows:
            want = ref["want"][b]
            for k in ("fmu", "fvar"):
                failures.append(check(f"{tag} series {b} {k}", got[k][b], want[k], want["mag_" + k]))
            at = helper(name, ref, b, alpha, lr, at=(got["fmu"][b], got["fvar"][b]))
            for k in keys:
                if k not in ("fmu", "fvar"):
                    failures.append(check(f"{tag} series {b} {k}", got[k][b], at[k], at["mag_" + k]))
    failures = [f for f in failures if f]
    assert not failures, "; ".join(failures)


def same_bits(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) for k in (keys or a.keys()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("two_d", [2, 10, 16, 18])
@pytest.mark.parametrize("name", NAMES)
def test_batch_of_three_against_the_helper_each_series_alone_and_evaluation_only_bit_for_bit(name, two_d, dtype):
    ref = reference(name, two_d, dtype == torch.float32)
    rc, out = launch(name, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} 2d={two_d}", name, ref, dtype, out, 0.5, 0.5)
    assert torch.equal(out["nat2"], out["nat2"].transpose(-1, -2)), "nat2 stays symmetric: both triangles are written from one sum"
    rc, again = launch(name, dtype, ref)
    assert rc == 0 and same_bits(again, out), "two launches on the same inputs return the same bits"
    for b in range(3):
        rc, one = launch(name, dtype, ref, series=b)
        assert rc == 0
        assert all(torch.equal(one[k][0], out[k][b]) for k in out), "a series alone gives the bits it gives in a batch"
    rc, value = launch(name, dtype, ref, update=False)
    assert rc == 0 and not any(k in value for k in SITES)
    assert same_bits(value, out, ("led_sum",) + POINTS), "evaluation only: the bits it has beside the update"
    rc, quiet = launch(name, dtype, ref, outputs=False)
    assert rc == 0 and same_bits(quiet, out, SITES), "the update without the optional outputs: the same bits"
    # empty segments: sum 0, the sites decay by 1 - lr alpha (log_norm: plus lr seg_const)
    for b, ln in enumerate(LAYOUT):
        for s, count in enumerate(ln):
            if count == 0:
                assert float(out["led_sum"][b, s]) == 0.0
                np.testing.assert_allclose(out["nat1"][b, s].cpu().numpy(), 0.75 * ref["nat1"][b, s], rtol=1e-6)
                np.testing.assert_allclose(float(out["log_norm"][b, s]), 0.75 * ref["log_norm"][b, s] + 0.5 * ref["seg_const"][b, s],
                                           rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lr", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_powers_and_rates_at_pairs_of_twelve_with_the_sum_of_two_matern52(alpha, lr, dtype):
    ref = matern_reference(dtype == torch.float32, alpha, lr)
    rc, out = launch(L.BERNOULLI, dtype, ref, alpha, lr)
    assert rc == 0
    check_against_helper(f"m52+m52 alpha={alpha} lr={lr}", L.BERNOULLI, ref, dtype, out, alpha, lr)
    if lr == 0.0:
        for k in SITES:
            assert torch.equal(out[k], dev(ref[k], dtype)), "lr = 0 leaves the sites as they are, bit for bit"
    rc, plain = launch(L.BERNOULLI, dtype, ref, alpha, lr, const=False)
    assert rc == 0 and same_bits(plain, out, ("nat1", "nat2", "led_sum") + POINTS), "seg_const enters log_norm only"
    if lr > 0.0:
        assert not torch.equal(plain["log_norm"], out["log_norm"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_two_series_of_two_hundred_points_in_one_segment(name, dtype):
    ref = reference(name, 4, dtype == torch.float32, 1.0, 1.0, ((200,), (200,)))
    rc, out = launch(name, dtype, ref, 1.0, 1.0)
    assert rc == 0
    check_against_helper(f"{name} (2, 200, 1)", name, ref, dtype, out, 1.0, 1.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_one_point_in_two_segments(name, dtype):
    """(B, N, S) = (1, 1, 2), sixteen draws.  float64: every launch on its own.  float32: a launch has one point and two segment
    numbers, so the helper's own error is a sample of one or two roundings and can be a small fraction of an ulp by chance (measured:
    2.7e-9 = 0.04 ulp for a log_norm whose kernel value is off by 0.3 ulp); the 4 x criterion is therefore applied to the maxima over
    the sixteen launches, per output - the same rule over a set large enough to hold it."""
    f32 = dtype == torch.float32
    worst = {}
    for seed in range(16):
        ref = reference(name, 4, f32, 1.0, 1.0, ((1, 0),), seed)
        rc, out = launch(name, dtype, ref, 1.0, 1.0)
        assert rc == 0
        if f32:
            for k, (top, own) in float32_errors(ref, out, [0]).items():
                worst[k] = (max(worst.get(k, (0.0, 0.0))[0], top), max(worst.get(k, (0.0, 0.0))[1], own))
        else:
            check_against_helper(f"{name} (1, 1, 2) draw {seed}", name, ref, dtype, out, 1.0, 1.0)
    failures = check_float32(f"{name} (1, 1, 2) x 16", worst)
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_an_undefined_point_and_a_missing_cavity_skip_their_own_segments_only(name, dtype):
    ref = dict(reference(name, 10, dtype == torch.float32))
    rc, clean = launch(name, dtype, ref)
    assert rc == 0
    c, cav_cov, cav_mean = ref["c"].copy(), ref["cav_cov"].copy(), ref["cav_mean"].copy()
    c[0, 1 + 65 + 3] = -1e6                   # series 0: one point of the 64 of segment 3
    c[2, 100] = float("nan")                  # series 2: one point among the 129 of segment 0, in its second tile
    cav_cov[1, 0] = float("nan")              # series 1, segment 0: a cavity that does not exist (not positive definite: NaN inputs)
    cav_mean[1, 0] = float("nan")
    ref.update(c=c, cav_cov=cav_cov, cav_mean=cav_mean)
    rc, out = launch(name, dtype, ref)
    assert rc == 0
    skipped = {(0, 3), (2, 0), (1, 0)}
    for b in range(3):
        for s in range(4):
            if (b, s) in skipped:
                for k in SITES:
                    assert torch.equal(out[k][b, s], dev(ref[k][b, s], dtype)), "its segment is untouched, bit for bit"
                assert bool(torch.isnan(out["led_sum"][b, s]))
            else:
                assert all(torch.equal(out[k][b, s], clean[k][b, s]) for k in SITES + ("led_sum",)), "every other segment keeps its bits"
    assert bool(torch.isnan(out["fvar"][0, 69])) and bool(torch.isnan(out["fmu"][2, 100])) and bool(torch.isnan(out["led"][1, :63]).all())
    untouched = torch.ones(3, 130, dtype=torch.bool, device=DEV)
    untouched[0, 69] = untouched[2, 100] = False
    untouched[1, :63] = False
    assert all(torch.equal(out[k][untouched], clean[k][untouched]) for k in POINTS)


def test_a_wrong_tile_table_is_clamped():
    """Tiles that name segments which do not exist and first-tile numbers that disagree with the offsets: wrong numbers, the return
    code 0 and no write outside the buffers (launch() checks the guard regions)."""
    dtype = torch.float64
    ref = reference(L.BERNOULLI, 4, False)
    tiles, tile_seg, seg_tile = tile_table(ref["offsets"])
    wild = tile_seg.copy()
    wild[0], wild[1], wild[-1] = -5, 10 ** 12, 12
    rc, _ = launch(L.BERNOULLI, dtype, ref, table=(tiles, wild, seg_tile))
    assert rc == 0
    shifted = seg_tile.copy()
    shifted[1:-1] += 3
    shifted[2] = -7
    shifted[-1] = 10 ** 9
    rc, _ = launch(L.BERNOULLI, dtype, ref, table=(tiles, tile_seg, shifted))
    assert rc == 0


def test_no_points_decays_the_sites_and_no_series_launches_nothing():
    dtype = torch.float64
    ref = dict(reference(L.BERNOULLI, 4, False))
    ref.update(w=ref["w"][:2, :0], c=ref["c"][:2, :0], y=ref["y"][:2, :0], offsets=np.zeros((2, 5), dtype=np.int64),
               **{k: ref[k][:2] for k in ("cav_mean", "cav_cov", "nat1", "nat2", "log_norm", "seg_const")})
    rc, out = launch(L.BERNOULLI, dtype, ref)
    assert rc == 0
    assert float(out["led_sum"].abs().max()) == 0.0
    np.testing.assert_allclose(out["nat1"].cpu().numpy(), 0.75 * ref["nat1"], rtol=1e-15)
    np.testing.assert_allclose(out["nat2"].cpu().numpy(), 0.75 * ref["nat2"], rtol=1e-15)
    np.testing.assert_allclose(out["log_norm"].cpu().numpy(), 0.75 * ref["log_norm"] + 0.5 * ref["seg_const"], rtol=1e-14, atol=1e-15)
    nodes, weights = c_rule()
    s = _lib.stream_ptr(DEV)
    # N = 0 needs no input, no table and no workspace
    led_sum = torch.full((2, 4), SENTINEL, dtype=dtype, device=DEV)
    assert _lib.call_rc(FN, dtype, 2, 0, 4, 4, 1, None, 20, nodes, weights, 0.5, 0.5, *([None] * 7), 0, None, None, None, 0, None, None,
                        None, _lib.ptr(led_sum), None, None, None, s) == 0
    torch.cuda.synchronize()
    assert float(led_sum.abs().max()) == 0.0
    assert _lib.call_rc(FN, dtype, 0, 5, 3, 4, 1, None, 20, nodes, weights, 0.5, 0.5, *([None] * 7), 0, None, None, None, 0,
                        *([None] * 7), s) == 0


def test_bad_arguments_return_their_codes_and_launch_nothing():
    dtype = torch.float64
    ref = reference(L.STUDENTT, 4, False)
    tiles, tile_seg, seg_tile = tile_table(ref["offsets"])
    table = [torch.tensor(a, dtype=torch.int64, device=DEV) for a in (ref["offsets"], tile_seg, seg_tile)]
    ins = [dev(ref[k], dtype) for k in ("w", "c", "y", "cav_mean", "cav_cov")]
    io = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((3, 4, 4), (3, 4, 4, 4), (3, 4), (3, 4), (3, 130), (3, 130),
                                                                             (3, 130))]
    ws_bytes = tiles * 15 * 8
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    nodes, weights = c_rule()
    par, s = c_params(L.STUDENTT), _lib.stream_ptr(DEV)
    p = [_lib.ptr(table[0])] + [_lib.ptr(t) for t in ins]
    tb, o = [_lib.ptr(table[1]), _lib.ptr(table[2]), _lib.ptr(ws)], [_lib.ptr(t) for t in io]

    def call(bsz=3, n=130, segs=4, two_d=4, lik=3, params=par, nq=20, nd=nodes, wt=weights, alpha=0.5, lr=0.5, ptrs=p, nt=tiles, tab=tb,
             nbytes=ws_bytes, outs=o):
        return _lib.call_rc(FN, dtype, bsz, n, segs, two_d, lik, params, nq, nd, wt, alpha, lr, *ptrs, None, nt, *tab, nbytes, *outs, s)

    assert call(bsz=-1) == -1 and call(n=-1) == -2 and call(segs=0) == -3
    for two_d in (0, 1, 3, 5, 20, -2):
        assert call(two_d=two_d) == -100
    assert call(lik=7) == -5 and call(params=None) == -6 and call(nq=0) == -7 and call(nq=33) == -7
    assert call(nd=None) == -8 and call(wt=None) == -9
    assert call(alpha=0.0) == -10 and call(alpha=1.5) == -10 and call(alpha=float("nan")) == -10
    assert call(lr=-0.5) == -11 and call(lr=1.5) == -11 and call(lr=float("nan")) == -11
    for i in range(6):
        assert call(ptrs=p[:i] + [None] + p[i + 1:]) == -(12 + i)
    assert call(nt=-1) == -19 and call(nt=2 ** 31) == -19 and call(n=0) == -19          # tiles without points
    for i in range(3):
        assert call(tab=tb[:i] + [None] + tb[i + 1:]) == -(20 + i)
    assert call(nbytes=ws_bytes - 1) == -23 and call(nbytes=0) == -23
    for i in range(3):
        assert call(outs=o[:i] + [None] + o[i + 1:]) == -(24 + i)
    assert call(outs=[None, None, o[2]] + o[3:]) == -24 and call(outs=[o[0], None, None] + o[3:]) == -25
    assert call(outs=[None] * 7) == 0                                   # nothing asked for
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in io)
    with pytest.raises(NotImplementedError):
        _lib.call(FN, dtype, 3, 130, 4, 20, 3, par, 20, nodes, weights, 0.5, 0.5, *p, None, tiles, *tb, ws_bytes, *o, s)
    with pytest.raises(ValueError, match="invalid argument #10"):
        _lib.call(FN, dtype, 3, 130, 4, 4, 3, par, 20, nodes, weights, 2.0, 0.5, *p, None, tiles, *tb, ws_bytes, *o, s)
