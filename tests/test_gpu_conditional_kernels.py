"""
GPU tests of the two lane-per-point kernels behind every prediction (csrc/mf_kernels.hpp), through the raw C ABI:
``mf_sde_conditional_statistics_*`` (``sde_cond_stats_kernel``) and ``mf_sde_conditional_predict_*`` (``sde_predict_kernel``), at every
state dimension d = 1..9 in float64 and float32, against the numpy statement of their formulas in
tests/helpers/conditional_closed_forms.py (which tests/test_conditional_closed_forms_host.py pins on direct Gaussian conditioning and
on long double: the float64 helper is within 1.1 eps (magnitude + 1) of long double on these inputs).

Inputs are random and well conditioned on purpose (``A = 0.7 randn / sqrt(d)``, ``Q = W W^T / d + I / 2``; the moments of the fused kernel
differ from series to series), so that the bound measures the kernel's arithmetic and not a condition number.  Every output buffer is
pre-filled with a sentinel and followed by a guard of 64 elements: the guard must stay untouched and no sentinel may survive inside.

Tolerances, in the scheme of tests/test_gpu_likelihoods.py and tests/test_gpu_sparse_cvi_kernel.py.
  float64: ``|err| <= K eps (magnitude + 1)`` against the float64 helper, eps = 2^-52, K = 64, the magnitude being the helper's: the
    same expression with every factor replaced by its absolute value.  check() prints every ratio ("RATIO f64 ...").
    Measured maxima on an MI355X over all the cases of this file: statistics D 0.98, E 1.83, T 0.96; predict mean
    1.66, cov 1.21.
  float32: the kernel's worst error over a launch, normalised by (magnitude + 1), per output, against 4 x the same figure of the helper
    evaluated in numpy float32 on the same (float32-rounded) inputs; both errors are taken against the float64 helper ("RATIO f32
    ...": the multiple).  Measured: statistics D 2.39 x, E 1.52 x, T 2.36 x; predict mean 2.37 x, cov 2.22 x.
    A maximum over one or a few lanes is a lottery (the numpy evaluation of a single d = 1 point is often exact): the 4 x comparison
    is made on launches of 64 lanes and more, and a smaller launch must return, bit for bit, what the same points return inside the
    large one - a lane's result depends on nothing but its own inputs - besides staying within K eps32 (magnitude + 1).
  Symmetry: ``T`` of the statistics kernel is written by ``store_sym`` and must be exactly symmetric; the fused kernel's covariance
    is assembled entry by entry and must be symmetric to K eps (magnitude + 1) with the eps of its own format.
"""
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import conditional_closed_forms as CC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS, EPS32 = 2.0 ** -52, 2.0 ** -23
K_F64 = 64.0
F32_FACTOR = 4.0
F32_MIN_LANES = 64                   # the float32 comparison is a maximum over at least this many lanes (module docstring)
GUARD, SENTINEL = 64, -77.25
DIMS = list(range(1, 10))
DTYPES = [torch.float64, torch.float32]
SIZES = (1, 63, 64, 65, 193)
LAYOUTS = ((3, 7, 43), (2, 5, 64), (5, 3, 13), (2, 1, 70))          # (B, N, Np); (1, 1, 1) is cut out of (2, 1, 70)
STATS, PREDICT = "mf_sde_conditional_statistics", "mf_sde_conditional_predict"
COV_KEYS = ("covs", "sub", "p0")

dims = pytest.mark.parametrize("d", DIMS, ids=[f"d{d}" for d in DIMS])
dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])


def rounded(a, f32):
    return np.asarray(a).astype(np.float32 if f32 else np.float64).astype(np.float64)


def freeze(obj):
    if isinstance(obj, np.ndarray):
        obj.setflags(write=False)
    elif isinstance(obj, dict):
        for v in obj.values():
            freeze(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            freeze(v)
    return obj


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def guarded(shape, dtype):
    """A sentinel-filled output of ``shape`` followed by a sentinel-filled guard region: ``(whole buffer, output view)``."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def written_inside_and_nowhere_else(*bufs):
    for buf, out in bufs:
        if buf is not None:
            assert bool(torch.all(buf[-GUARD:] == SENTINEL)), "a write past the end of an output"
            assert not bool(torch.any(out == SENTINEL)), "an element of an output was never written"


def check(what, got, want, mag, dtype, got32=None, keep=None):
    """float64: the K eps bound; float32: 4 x the normalised error of the numpy float32 evaluation (launches of >= 64 lanes).  Prints
    the figure first.  ``keep``: a mask over the leading (lane) axis."""
    got, want, mag = np.asarray(got, dtype=np.float64), np.asarray(want), np.asarray(mag)
    if keep is not None:
        got, want, mag = got[keep], want[keep], mag[keep]
        got32 = None if got32 is None else np.asarray(got32)[keep]
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    scaled = np.abs(got - want) / (mag + 1.0)
    if dtype == torch.float64:
        ratio = float(scaled.max() / EPS)
        print(f"RATIO f64 {what}: {ratio:.2f}")
        assert ratio <= K_F64, f"{what}: {ratio:.1f} eps (magnitude + 1) at {np.unravel_index(int(scaled.argmax()), scaled.shape)}"
    elif got32 is not None and got.shape[0] >= F32_MIN_LANES:
        own = float((np.abs(np.asarray(got32, dtype=np.float64) - want) / (mag + 1.0)).max())
        multiple = float(scaled.max()) / own if own > 0 else (0.0 if scaled.max() == 0 else float("inf"))
        print(f"RATIO f32 {what}: {multiple:.2f} x (kernel {scaled.max():.3e}, numpy float32 {own:.3e})")
        assert scaled.max() <= F32_FACTOR * own, f"{what}: kernel {scaled.max():.3e} against numpy float32 {own:.3e}"
    else:
        # a few float32 lanes: no statistics to compare with; they are compared bit for bit with a large launch by the caller, and
        # must at least be float32-accurate in the plain K eps sense
        assert float(scaled.max()) <= K_F64 * EPS32, f"{what}: {scaled.max() / EPS32:.1f} eps32 (magnitude + 1)"


# ---- conditional statistics --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stats_reference(d, f32, variant="generic", n=193):
    """Inputs (rounded to the dtype under test) and the helper on them - computed once per case and shared, read-only."""
    rng = np.random.default_rng(1000 + d)
    a_mt, q_mt, a_tp, q_tp = CC.draw_statistics_inputs(rng, n, d)
    eye, zero = np.broadcast_to(np.eye(d), (n, d, d)).copy(), np.zeros((n, d, d))
    want = None
    if variant == "training":                            # the new point IS the next training point
        a_tp, q_tp = eye, zero
        want = (zero, eye, zero)                         # D = 0, E = I, T = 0 exactly
    elif variant == "far_before":                        # the previous neighbour is the stationary prior at -APPROX_INF
        a_mt, q_mt = zero, CC._spd(rng, (n,), d)
    elif variant == "far_after":                         # the next neighbour is the stationary prior at +APPROX_INF
        a_tp, q_tp = zero, CC._spd(rng, (n,), d)
    elif variant == "pivot":                             # one point whose Q_tp + A_tp Q_mt A_tp^T is not positive definite
        q_tp[77] = -np.eye(d)
    ins = tuple(rounded(x, f32) for x in (a_mt, q_mt, a_tp, q_tp))
    helper, mags = CC.statistics(*ins)
    ref = dict(ins=ins, want=helper if want is None else want, mags=mags)
    if f32:
        ref["want32"] = CC.statistics(*ins, dtype=np.float32)[0]
    return freeze(ref)


def launch_stats(ref, d, dtype, n, info=None):
    ins = [dev(x[:n], dtype) for x in ref["ins"]]
    proj, cov = guarded((n, d, 2 * d), dtype), guarded((n, d, d), dtype)
    rc = _lib.call_rc(STATS, dtype, n, d, *[_lib.ptr(x) for x in ins], _lib.ptr(proj[1]), _lib.ptr(cov[1]), info, _lib.stream_ptr(DEV))
    assert rc == 0
    written_inside_and_nowhere_else(proj, cov)
    return proj[1], cov[1]


def check_stats(tag, ref, d, dtype, proj, cov, keep=None):
    n = proj.shape[0]
    got = (proj[..., :d].cpu().numpy(), proj[..., d:].cpu().numpy(), cov.cpu().numpy())
    own = ref.get("want32", (None,) * 3)
    for name, g, w, m, o in zip("DET", got, ref["want"], ref["mags"], own):
        check(f"statistics {name} | d={d} n={n} {tag}", g, w[:n], m[:n], dtype, None if o is None else o[:n], keep)
    assert torch.equal(cov, cov.transpose(-1, -2)), "T is written by store_sym: exactly symmetric"


@dtypes
@dims
def test_statistics_at_one_lane_and_around_one_and_three_wavefronts(d, dtype):
    ref = stats_reference(d, dtype == torch.float32)
    full = launch_stats(ref, d, dtype, SIZES[-1])
    check_stats("generic", ref, d, dtype, *full)
    for n in SIZES[:-1]:
        proj, cov = launch_stats(ref, d, dtype, n)
        check_stats("generic", ref, d, dtype, proj, cov)
        assert torch.equal(proj, full[0][:n]) and torch.equal(cov, full[1][:n]), "a point's result does not depend on the launch"


@dtypes
@dims
def test_statistics_of_a_new_point_on_a_training_point(d, dtype):
    """A_tp = I, Q_tp = 0: x_t = x_+, so E = I, D = 0 and T = 0 - each to the rounding of the generic expression that produced it."""
    ref = stats_reference(d, dtype == torch.float32, "training")
    check_stats("training point", ref, d, dtype, *launch_stats(ref, d, dtype, 193))


@dtypes
@dims
@pytest.mark.parametrize("variant", ["far_before", "far_after"])
def test_statistics_next_to_the_stationary_prior(variant, d, dtype):
    """The neighbours at -/+ APPROX_INF: A_mt = 0, Q_mt = Pinf (D = 0), and the mirror A_tp = 0, Q_tp = Pinf (E = 0, D = A_mt,
    T = Q_mt)."""
    ref = stats_reference(d, dtype == torch.float32, variant)
    proj, cov = launch_stats(ref, d, dtype, 193)
    check_stats(variant, ref, d, dtype, proj, cov)
    if variant == "far_before":
        assert float(proj[..., :d].abs().max()) == 0.0, "D = A_mt - E A_tp A_mt with A_mt = 0"
    else:
        assert float(proj[..., d:].abs().max()) == 0.0, "E = (A_tp Q_mt)^T S^-1 with A_tp = 0"
        assert torch.equal(proj[..., :d], dev(ref["ins"][0], dtype)) and torch.equal(cov, dev(ref["ins"][1], dtype))


# ---- the fused prediction ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def predict_reference(layout, d, f32, pivot=False):
    bsz, n, n_new = layout
    case = CC.draw_predict_inputs(np.random.default_rng(2000 + 10 * d + n), bsz, n, n_new, d)
    if pivot:
        case["q_tp"][1, 12] = -np.eye(d)
    for k in CC.PREDICT_KEYS:
        if case[k] is not None:
            case[k] = rounded(case[k], f32)
    if n_new > n:
        assert all(set(case["idx"][b]) == set(range(n + 1)) for b in range(bsz)), "every series meets every insertion index"
        assert not any(np.array_equal(case["idx"][b], np.sort(case["idx"][b])) for b in range(bsz)), "not in lane order"
    per = [CC.predict_series(case, b) for b in range(bsz)]
    ref = dict(case=case, layout=layout, d=d)
    ref["want"] = tuple(np.stack([p[0][i] for p in per]) for i in range(2))
    ref["mags"] = tuple(np.stack([p[1][i] for p in per]) for i in range(2))
    if f32:
        ref["want32"] = tuple(np.stack([CC.predict_series(case, b, dtype=np.float32)[0][i] for b in range(bsz)]) for i in range(2))
    return freeze(ref)


def launch_predict(case, dtype, with_cov=True, info=None):
    """One launch on all the series of ``case``.  Without ``with_cov`` no covariance input is passed at all."""
    (bsz, n_new), (_, n, d) = case["idx"].shape, case["means"].shape
    idx = torch.tensor(np.asarray(case["idx"]), dtype=torch.int64, device=DEV).contiguous()
    ins = [None if case[k] is None or (k in COV_KEYS and not with_cov) else dev(case[k], dtype) for k in CC.PREDICT_KEYS]
    mean = guarded((bsz, n_new, d), dtype)
    cov = guarded((bsz, n_new, d, d), dtype) if with_cov else (None, None)
    rc = _lib.call_rc(PREDICT, dtype, bsz, n, n_new, d, _lib.ptr(idx), *[_lib.ptr(x) for x in ins], _lib.ptr(mean[1]), _lib.ptr(cov[1]),
                      info, _lib.stream_ptr(DEV))
    assert rc == 0
    written_inside_and_nowhere_else(mean, cov)
    return mean[1], cov[1]


def check_predict(tag, ref, dtype, mean, cov, keep=None, want=None, mags=None, own=None):
    want, mags = ref["want"] if want is None else want, ref["mags"] if mags is None else mags
    own = ref.get("want32", (None, None)) if own is None else own
    d = ref["d"]
    lanes = lambda a, tail: None if a is None else np.asarray(a).reshape((-1,) + (d,) * tail)     # noqa: E731
    check(f"predict mean | d={d} {tag}", lanes(mean.cpu().numpy(), 1), lanes(want[0], 1), lanes(mags[0], 1), dtype, lanes(own[0], 1), keep)
    if cov is None:
        return
    got = lanes(cov.cpu().numpy(), 2)
    check(f"predict cov | d={d} {tag}", got, lanes(want[1], 2), lanes(mags[1], 2), dtype, lanes(own[1], 2), keep)
    skew = np.abs(got - np.swapaxes(got, -1, -2)) / (lanes(mags[1], 2) + 1.0)
    if keep is not None:
        skew = skew[keep]
    assert float(skew.max()) <= K_F64 * (EPS if dtype == torch.float64 else EPS32), "the covariance is symmetric to within the bound"


@dtypes
@dims
@pytest.mark.parametrize("layout", LAYOUTS, ids=["x".join(map(str, lay)) for lay in LAYOUTS])
def test_predict_mean_and_full_covariance_on_every_layout(layout, d, dtype):
    """(3, 7, 43): 129 lanes, series 0 -> 1 and 1 -> 2 change inside a wavefront, three blocks.  (2, 5, 64): a series per block.
    (5, 3, 13): five series in two blocks.  (2, 1, 70): N = 1 - no subsequent covariances, every index 0 or 1."""
    ref = predict_reference(layout, d, dtype == torch.float32)
    assert (ref["case"]["sub"] is None) == (layout[1] == 1)
    mean, cov = launch_predict(ref["case"], dtype)
    check_predict("x".join(map(str, layout)), ref, dtype, mean, cov)


@dtypes
@dims
def test_predict_of_one_point_of_one_series_of_one_training_point(d, dtype):
    """(B, N, Np) = (1, 1, 1), once before and once after the only training point: lanes of series 0 of the (2, 1, 70) layout, launched
    alone - the bound, and the bits of the large launch."""
    ref = predict_reference((2, 1, 70), d, dtype == torch.float32)
    full_mean, full_cov = launch_predict(ref["case"], dtype)
    for index in (0, 1):
        p = int(np.flatnonzero(ref["case"]["idx"][0] == index)[0])
        one = {k: None if v is None else (v[:1] if k in ("means", "covs", "m0", "p0") else v[:1, p:p + 1]) for k, v in ref["case"].items()}
        assert one["idx"].shape == (1, 1) and one["sub"] is None
        mean, cov = launch_predict(one, dtype)
        cut = lambda pair: tuple(x[:1, p:p + 1] for x in pair)                                          # noqa: E731
        check_predict(f"1x1x1 index {index}", ref, dtype, mean, cov, want=cut(ref["want"]), mags=cut(ref["mags"]),
                      own=cut(ref["want32"]) if "want32" in ref else None)
        assert torch.equal(mean[0, 0], full_mean[0, p]) and torch.equal(cov[0, 0], full_cov[0, p])


@dtypes
@dims
@pytest.mark.parametrize("layout", [(3, 7, 43), (2, 1, 70)], ids=["3x7x43", "2x1x70"])
def test_predict_means_only_takes_no_covariance_input_and_returns_the_same_bits(layout, d, dtype):
    ref = predict_reference(layout, d, dtype == torch.float32)
    mean, _ = launch_predict(ref["case"], dtype)
    only, none = launch_predict(ref["case"], dtype, with_cov=False)
    assert none is None and torch.equal(only, mean)


# ---- degenerate sizes, argument checks, the pivot report ---------------------------------------------------------------------------
@dtypes
@dims
def test_no_series_no_new_points_and_no_points_return_zero_and_write_nothing(d, dtype):
    ref = predict_reference((3, 7, 43), d, dtype == torch.float32)
    case = ref["case"]
    idx = torch.tensor(np.asarray(case["idx"]), dtype=torch.int64, device=DEV)
    tensors = [dev(case[k], dtype) for k in CC.PREDICT_KEYS]
    ins = [_lib.ptr(t) for t in tensors]
    outs = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((3, 43, d), (3, 43, d, d))]
    s = _lib.stream_ptr(DEV)
    for bsz, n_new in ((0, 43), (3, 0), (0, 0)):
        assert _lib.call_rc(PREDICT, dtype, bsz, 7, n_new, d, _lib.ptr(idx), *ins, *[_lib.ptr(o) for o in outs], None, s) == 0
    assert _lib.call_rc(PREDICT, dtype, 0, 7, 43, d, *([None] * 12), None, s) == 0, "sizes are looked at before pointers"
    st = stats_reference(d, dtype == torch.float32)
    st_tensors = [dev(x, dtype) for x in st["ins"]]
    st_ins = [_lib.ptr(t) for t in st_tensors]
    st_outs = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((193, d, 2 * d), (193, d, d))]
    assert _lib.call_rc(STATS, dtype, 0, d, *st_ins, *[_lib.ptr(o) for o in st_outs], None, s) == 0
    assert _lib.call_rc(STATS, dtype, 0, d, *([None] * 6), None, s) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in outs + st_outs)


def test_bad_arguments_return_their_codes_and_launch_nothing():
    dtype, d = torch.float64, 3
    ref = predict_reference((3, 7, 43), d, False)
    case = ref["case"]
    idx = _lib.ptr(torch.tensor(np.asarray(case["idx"]), dtype=torch.int64, device=DEV))
    tensors = [dev(case[k], dtype) for k in CC.PREDICT_KEYS]             # kept alive to the end of the test
    p = [_lib.ptr(t) for t in tensors]
    io = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((3, 43, d), (3, 43, d, d), (193, d, 2 * d), (193, d, d))]
    o = [_lib.ptr(t) for t in io]
    s = _lib.stream_ptr(DEV)

    def predict(bsz=3, n=7, n_new=43, dim=d, index=idx, ptrs=p, mean=o[0], cov=o[1]):
        return _lib.call_rc(PREDICT, dtype, bsz, n, n_new, dim, index, *ptrs, mean, cov, None, s)

    without = lambda ptrs, i: ptrs[:i] + [None] + ptrs[i + 1:]                                      # noqa: E731
    assert predict(bsz=-1) == -1 and predict(n=0) == -2 and predict(n=-3) == -2 and predict(n_new=-1) == -3
    assert predict(dim=0) == -4 and predict(dim=-1) == -4 and predict(index=None) == -5
    for i in range(4):                                                   # A_mt, Q_mt, A_tp, Q_tp
        assert predict(ptrs=without(p, i)) == -6
    assert predict(ptrs=without(p, 4)) == -10                            # means
    for i in (5, 6, 8):                                                  # covs, subsequent_covs (N > 1), prior_cov - with a covariance output
        assert predict(ptrs=without(p, i)) == -11
    assert predict(ptrs=without(p, 7)) == -13 and predict(mean=None) == -15
    assert predict(dim=10) == -100 and predict(dim=33) == -100

    st_tensors = [dev(x, dtype) for x in stats_reference(d, False)["ins"]]
    q = [_lib.ptr(t) for t in st_tensors]

    def stats(n=193, dim=d, ptrs=q, proj=o[2], cov=o[3]):
        return _lib.call_rc(STATS, dtype, n, dim, *ptrs, proj, cov, None, s)

    assert stats(n=-1) == -1 and stats(dim=0) == -2 and stats(dim=-2) == -2
    for i in range(4):
        assert stats(ptrs=without(q, i)) == -3
    assert stats(proj=None) == -7 and stats(cov=None) == -8
    assert stats(dim=10) == -100 and stats(dim=33) == -100
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in io), "the checks return before anything is launched"
    with pytest.raises(NotImplementedError):
        _lib.call(STATS, dtype, 193, 10, *q, o[2], o[3], None, s)
    with pytest.raises(NotImplementedError):
        _lib.call(PREDICT, dtype, 3, 7, 43, 10, idx, *p, o[0], o[1], None, s)
    with pytest.raises(ValueError, match="invalid argument #11"):
        _lib.call(PREDICT, dtype, 3, 7, 43, d, idx, *without(p, 5), o[0], o[1], None, s)


def expect_pivot_report(info, what):
    """The library's ordinary report of a non-positive pivot: the `info` word of the stream, mirrored and raised."""
    with pytest.raises(_lib.MarkovflowAmdError):
        _lib.raise_on_info(info, what, DEV)
        _lib.check_errors()
    _lib.check_errors()                                                  # reported once, then clean again


@dtypes
@pytest.mark.parametrize("d", [2, 9], ids=["d2", "d9"])
def test_statistics_report_a_non_positive_pivot_and_leave_the_other_points_alone(d, dtype):
    ref = stats_reference(d, dtype == torch.float32, "pivot", 130)
    a_mt, q_mt, a_tp, q_tp = ref["ins"]
    assert np.linalg.eigvalsh(q_tp[77] + a_tp[77] @ q_mt[77] @ a_tp[77].T).min() < 0, "the case is what it claims to be"
    _lib.check_errors()                                                  # start clean
    proj, cov = launch_stats(ref, d, dtype, 130, info=_lib.pivot_info(DEV))
    expect_pivot_report(_lib.pivot_info(DEV), "test: conditional statistics")
    keep = np.arange(130) != 77
    got = (proj[..., :d].cpu().numpy(), proj[..., d:].cpu().numpy(), cov.cpu().numpy())
    for name, g, w, m, o in zip("DET", got, ref["want"], ref["mags"], ref.get("want32", (None,) * 3)):
        check(f"statistics {name} | d={d} n=130 one bad pivot", g, w, m, dtype, o, keep)
    clean = stats_reference(d, dtype == torch.float32, "generic", 130)
    assert all(np.array_equal(x[keep], y[keep]) for x, y in zip(ref["ins"], clean["ins"]))
    ok_proj, ok_cov = launch_stats(clean, d, dtype, 130, info=_lib.pivot_info(DEV))
    sel = torch.tensor(keep, device=DEV)
    assert torch.equal(ok_proj[sel], proj[sel]) and torch.equal(ok_cov[sel], cov[sel]), "the other lanes keep their bits"
    _lib.check_errors()                                                  # ... and a clean launch raises nothing


@dtypes
@pytest.mark.parametrize("d", [2, 9], ids=["d2", "d9"])
def test_predict_reports_a_non_positive_pivot_and_leaves_the_other_points_alone(d, dtype):
    layout = (2, 5, 65)                                                  # 130 lanes
    ref = predict_reference(layout, d, dtype == torch.float32, True)
    case = ref["case"]
    bad = case["q_tp"][1, 12] + case["a_tp"][1, 12] @ case["q_mt"][1, 12] @ case["a_tp"][1, 12].T
    assert np.linalg.eigvalsh(bad).min() < 0, "the case is what it claims to be"
    _lib.check_errors()
    mean, cov = launch_predict(case, dtype, info=_lib.pivot_info(DEV))
    expect_pivot_report(_lib.pivot_info(DEV), "test: conditional predict")
    keep = np.arange(130) != 65 + 12
    check_predict("2x5x65 one bad pivot", ref, dtype, mean, cov, keep=keep)
    clean = predict_reference(layout, d, dtype == torch.float32)
    ok_mean, ok_cov = launch_predict(clean["case"], dtype, info=_lib.pivot_info(DEV))
    sel = torch.tensor(keep, device=DEV)
    assert torch.equal(ok_mean.reshape(130, d)[sel], mean.reshape(130, d)[sel])
    assert torch.equal(ok_cov.reshape(130, d, d)[sel], cov.reshape(130, d, d)[sel]), "the other lanes keep their bits"
    _lib.check_errors()
