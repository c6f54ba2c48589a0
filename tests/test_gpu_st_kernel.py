"""
GPU tests of ``mf_lik_st_expectations_*`` (csrc/mf_st.hip) through the raw C ABI, with a guard region behind every output, against
the numpy statement of its formulas in tests/helpers/st_closed_forms.py (``st_expectations``).

Shapes.  ``T = ST_EXPECT_TILE = 256``; every series has N = 2 T + 67 = 579 points in five segments of lengths 0, 1, T, T + 1 and 65
(in three orders for the three series): an empty segment, a segment of one point, a full row, a row plus one point, and a group of
64 plus one point - a partial group and a partial row both occur.  ``(Ms, d_t)`` runs over (1,1), (1,3), (2,1), (5,3), (21,3), (32,2)
and (64,1): pair dimensions 2, 6, 4, 30, 126, 128, 128 - one and several slabs, a partial slab, slabs of 32 and of 16 rows, the
padding of W to a multiple of 16.

Accuracy, the project's rule for a kernel whose error is compared with a composition's (CHANGELOG, "limit 4 x"): the YARDSTICK of an
output is the error of ``st_expected_log_likelihood_torch`` (values, and its autograd gradients) evaluated in the dtype under test
against the helper one precision up - float64 for float32, numpy.longdouble for float64 - on the inputs of the case and seven more
draws of the same kind, normalised element by element by eps x the output's magnitude (``mag_*`` of the helper), maximised over the
elements, the series and those 8 seeds and floored at 1.
scripts/st_yardsticks.py measures it on the CPU and records it in tests/golden/st_yardsticks.json, per (Ms, d_t), dtype, likelihood
and output.  The kernel's normalised error, against the same helper one precision up, may be at most 4 x the yardstick.
``check_against_helper`` prints every ratio (``RATIO ...``).  Measured worst ratios kernel / yardstick on an MI355X over every case
of this file (allowed: 4), float64 / float32: ve_sum 0.93 / 1.05, g_mean 1.59 / 1.43, g_cov 1.19 / 1.71, g_a 1.82 / 1.95, g_wt
2.47 / 2.63, g_c 2.35 / 2.06, fmu 1.91 / 1.72, fvar 1.18 / 1.34.  The yardsticks themselves lie between 1 and 74.9 eps x magnitude
at 20 nodes (the largest: ``g_c`` of the Bernoulli likelihood in float32); with one node ``gv`` is zero and the Student-t ``gm`` is
ill-conditioned in ``fmu``, and the yardsticks of ``g_a`` and ``g_wt`` reach 513 and 1135 (every rule has its own entry: ``.../nq1``).
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from markovflow_amd import _lib, models
from helpers import likelihood_closed_forms as L
from helpers import st_closed_forms as ST

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = models.ST_EXPECT_TILE
GUARD, SENTINEL = 64, -77.25
LAYOUT = ((0, 1, T, T + 1, 65), (T + 1, 65, 0, T, 1), (65, T, 1, 0, T + 1))      # three series, N = 2 T + 67 each
SIZES = [(1, 1), (1, 3), (2, 1), (5, 3), (21, 3), (32, 2), (64, 1)]
ALL_LIKS = {(5, 3), (32, 2)}
NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
DTYPES = [torch.float64, torch.float32]
SEG_OUTS, POINT_OUTS, PROJ_OUTS = ("ve_sum", "g_mean", "g_cov"), ("g_a", "g_wt", "g_c"), ("fmu", "fvar")
OUTS = SEG_OUTS + POINT_OUTS + PROJ_OUTS
FN = "mf_lik_st_expectations"
EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}
YARD_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "st_yardsticks.json")
CASES = [(ms, dt, name) for ms, dt in SIZES for name in (NAMES if (ms, dt) in ALL_LIKS else NAMES[:2])]


OTHER_NQ = (1, 32)


def case_seed(ms, dt, nq):
    return 1000 * ms + 10 * dt + nq


def yard_key(ms, dt, dtype, name, nq=20):
    return f"{ms}x{dt}/{'f32' if dtype == torch.float32 else 'f64'}/{name}" + ("" if nq == 20 else f"/nq{nq}")


@functools.lru_cache(maxsize=None)
def yardsticks():
    with open(YARD_FILE) as f:
        return json.load(f)


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
    per = (np.diff(offsets, axis=1).reshape(-1) + T - 1) // T
    return int(per.sum()), np.repeat(np.arange(per.size), per).astype(np.int64), np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


def draw_inputs(ms, dt, name, f32, layout, seed):
    """Inputs rounded to the dtype under test.  |W| <= 0.7 / sqrt(Ms d_t) keeps fvar of order one at every size; pair_cov is a
    random SPD matrix and c > 0, so fvar > 0 by construction."""
    rng = np.random.default_rng(seed)
    ty = np.float32 if f32 else np.float64
    rnd = lambda v: np.asarray(v).astype(ty).astype(np.float64)          # noqa: E731
    bsz, segs, n, pair = len(layout), len(layout[0]), int(np.sum(layout[0])), 2 * ms * dt
    ref = dict(offsets=np.stack([np.concatenate([[0], np.cumsum(ln)]) for ln in layout]).astype(np.int64))
    ref["a"] = rnd(rng.uniform(-1.0, 1.0, size=(bsz, n, ms)) / np.sqrt(ms))
    ref["wt"] = rnd(rng.uniform(-0.7, 0.7, size=(bsz, n, 2 * dt)) / np.sqrt(dt))
    ref["c"] = rnd(rng.uniform(0.05, 0.5, size=(bsz, n)))
    root = rng.normal(size=(bsz, segs, pair, pair))
    ref["pair_cov"] = rnd(root @ root.transpose(0, 1, 3, 2) / pair + 0.1 * np.eye(pair))
    ref["pair_mean"] = rnd(rng.normal(size=(bsz, segs, pair)))
    ref["y"] = rnd(np.resize(np.asarray(L.OBSERVED[name]), (bsz, n)))
    return ref


@functools.lru_cache(maxsize=None)
def reference(ms, dt, name, nq, f32, layout=LAYOUT, skew=False):
    """The inputs and the helper one precision up on them, per series - computed once per case and shared, read-only."""
    ref = draw_inputs(ms, dt, name, f32, layout, case_seed(ms, dt, nq))
    if skew:                                       # a non-symmetric pair_cov with the same symmetric part
        rng = np.random.default_rng(5)
        anti = rng.normal(size=ref["pair_cov"].shape)
        ty = np.float32 if f32 else np.float64
        ref["pair_cov"] = (ref["pair_cov"] + 0.25 * (anti - anti.transpose(0, 1, 3, 2))).astype(ty).astype(np.float64)
    up = np.float64 if f32 else np.longdouble
    ref["want"] = [ST.st_expectations(L.LIKELIHOODS[name], ref["a"][b], ref["wt"][b], ref["c"][b], ref["y"][b], ref["offsets"][b],
                                      ref["pair_mean"][b], ref["pair_cov"][b], nq, up) for b in range(len(layout))]
    for v in ref.values():
        for item in (v if isinstance(v, list) else [v]):
            for x in (item.values() if isinstance(item, dict) else [item]):
                x.setflags(write=False)
    return ref


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def guarded(shape, dtype):
    """A sentinel-filled buffer of ``shape`` followed by a sentinel-filled guard region."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def launch(name, nq, dtype, ref, series=None, want=OUTS, with_y=True):
    """One call on all the series of ``ref`` (or on ``series`` alone).  Returns ``(rc, {output: tensor})`` after checking every guard
    region."""
    pick = (lambda v: v) if series is None else (lambda v: v[series:series + 1])
    bsz, n, ms = pick(ref["a"]).shape
    two_dt = ref["wt"].shape[-1]
    pair = ms * two_dt
    offsets = pick(ref["offsets"])
    segs = offsets.shape[1] - 1
    tiles, tile_seg, seg_tile = tile_table(offsets)
    table = [torch.tensor(v, dtype=torch.int64, device=DEV).contiguous() for v in (offsets, tile_seg, seg_tile)]
    ins = [dev(pick(ref[k]), dtype) for k in ("a", "wt", "c", "y", "pair_mean", "pair_cov")]
    if not with_y:
        ins[3] = None
    shapes = dict(ve_sum=(bsz, segs), g_mean=(bsz, segs, pair), g_cov=(bsz, segs, pair, pair), g_a=(bsz, n, ms), g_wt=(bsz, n, two_dt),
                  g_c=(bsz, n), fmu=(bsz, n), fvar=(bsz, n))
    outs = {k: guarded(shapes[k], dtype) if k in want else (None, None) for k in OUTS}
    esize = ins[0].element_size()
    ws_bytes = int(_lib.load().mf_lik_st_expectations_workspace_bytes(tiles, ms, two_dt, esize))
    assert ws_bytes == tiles * (pair * (pair + 1) // 2 + pair + 1) * esize
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    nodes, weights = c_rule(nq)
    rc = _lib.call_rc(FN, dtype, bsz, n, segs, ms, two_dt, L.IDS[name], c_params(name), nq, nodes, weights, _lib.ptr(table[0]),
                      *[_lib.ptr(t) for t in ins], tiles, _lib.ptr(table[1]), _lib.ptr(table[2]), _lib.ptr(ws), ws_bytes,
                      *[_lib.ptr(outs[k][1]) for k in OUTS], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert all(b[0] is None or bool(torch.all(b[0][-GUARD:] == SENTINEL)) for b in outs.values()), "a write past the end of an output"
    assert bool(torch.all(ws[ws_bytes:] == 0x5A)), "a write past the end of the workspace"
    return rc, {k: v[1] for k, v in outs.items()}


def check_against_helper(tag, ms, dt, name, ref, dtype, outs, series=None, nq=20):
    """Every series and every output: the normalised error against 4 x the recorded yardstick.  Every figure is printed before the
    first failure is raised."""
    key = yard_key(ms, dt, dtype, name, nq)
    yard = yardsticks()[key]
    rows = list(range(len(ref["want"]))) if series is None else [series]
    failures = []
    for i, b in enumerate(rows):
        want = ref["want"][b]
        for out, got in outs.items():
            if got is None:
                continue
            assert not bool(torch.any(got[i] == SENTINEL)), f"{tag} series {b} {out}: an element was not written"
            got_np = got[i].cpu().numpy().astype(np.float64)
            assert np.all(np.isfinite(got_np)), f"{tag} series {b} {out}: non-finite result"
            err = np.abs(got_np - want[out].astype(np.float64) if want[out].dtype != np.longdouble
                         else (got_np.astype(np.longdouble) - want[out]).astype(np.float64))
            mag = np.asarray(want["mag_" + out])
            scaled = np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), np.where(err > 0, np.inf, 0.0)) / EPS[dtype]
            worst = float(scaled.max()) if scaled.size else 0.0
            print(f"RATIO {key} series {b} {out}: {worst:.2f} eps mag, yardstick {yard[out]:.2f}, {worst / yard[out]:.2f} x")
            if worst > 4.0 * yard[out]:
                failures.append(f"{tag} series {b} {out}: {worst:.2f} eps mag against a yardstick of {yard[out]:.2f}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ms,dt,name", CASES)
def test_batch_of_three_against_the_helper_each_series_alone_and_a_repeat_bit_for_bit(ms, dt, name, dtype):
    ref = reference(ms, dt, name, 20, dtype == torch.float32)
    rc, outs = launch(name, 20, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} {ms}x{dt}", ms, dt, name, ref, dtype, outs)
    assert torch.equal(outs["g_cov"], outs["g_cov"].transpose(-1, -2)), "g_cov is symmetric: both triangles come from one sum"
    for b, ln in enumerate(LAYOUT):                # empty segments: exact zeros
        for s, count in enumerate(ln):
            if count == 0:
                assert all(float(outs[k][b, s].abs().max()) == 0.0 for k in SEG_OUTS)
    rc, again = launch(name, 20, dtype, ref)
    assert rc == 0 and all(torch.equal(again[k], outs[k]) for k in OUTS), "two launches on the same inputs return the same bits"
    for b in range(3):
        rc, one = launch(name, 20, dtype, ref, series=b)
        assert rc == 0
        assert all(torch.equal(one[k][0], outs[k][b]) for k in OUTS), "a series alone gives the bits it gives in a batch"


# the five independent switches of the ABI; every non-empty subset of them, 31 in all
SWITCHES = (("ve_sum",), ("g_mean", "g_cov"), POINT_OUTS, ("fmu",), ("fvar",))
COMBOS = [sum((SWITCHES[i] for i in range(5) if mask >> i & 1), ()) for mask in range(1, 32)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ms,dt", [(5, 3), (32, 2)])
def test_every_output_combination_has_the_bits_of_the_full_call(ms, dt, dtype):
    ref = reference(ms, dt, L.BERNOULLI, 20, dtype == torch.float32)
    rc, full = launch(L.BERNOULLI, 20, dtype, ref)
    assert rc == 0 and len(COMBOS) == 31 and len(set(COMBOS)) == 31
    for want in COMBOS:
        rc, part = launch(L.BERNOULLI, 20, dtype, ref, want=want)
        assert rc == 0
        for k in OUTS:
            assert (part[k] is None) == (k not in want)
            if k in want:
                assert torch.equal(part[k], full[k]), f"{k} in the call for {want} differs from {k} in the full call"
    rc, proj = launch(L.BERNOULLI, 20, dtype, ref, want=PROJ_OUTS, with_y=False)
    assert rc == 0 and all(torch.equal(proj[k], full[k]) for k in PROJ_OUTS), "projection only: y may be NULL"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nq", [1, 20, 32])
def test_quadrature_sizes(nq, dtype):
    ref = reference(5, 3, L.STUDENTT, nq, dtype == torch.float32)
    rc, outs = launch(L.STUDENTT, nq, dtype, ref)
    assert rc == 0
    check_against_helper(f"student-t nq={nq}", 5, 3, L.STUDENTT, ref, dtype, outs, nq=nq)      # (a yardstick per rule)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ms,dt", [(5, 3), (32, 2)])
def test_a_non_symmetric_pair_cov_is_honoured(ms, dt, dtype):
    ref = reference(ms, dt, L.GAUSSIAN, 20, dtype == torch.float32, skew=True)
    rc, outs = launch(L.GAUSSIAN, 20, dtype, ref)
    assert rc == 0
    check_against_helper(f"skew {ms}x{dt}", ms, dt, L.GAUSSIAN, ref, dtype, outs)
    plain = reference(ms, dt, L.GAUSSIAN, 20, dtype == torch.float32)
    assert not np.array_equal(plain["pair_cov"], ref["pair_cov"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_negative_variance_poisons_its_own_point_and_segment_only(dtype):
    ms, dt = 5, 3
    base = reference(ms, dt, L.BERNOULLI, 20, dtype == torch.float32)
    rc, clean = launch(L.BERNOULLI, 20, dtype, base)
    assert rc == 0
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    series, seg = 1, 3                             # a full row of series 1; its point 7
    point = int(base["offsets"][series, seg]) + 7
    bad["c"][series, point] = -1e6
    rc, outs = launch(L.BERNOULLI, 20, dtype, bad)
    assert rc == 0
    for k in SEG_OUTS:
        assert bool(torch.isnan(outs[k][series, seg]).all()), f"{k} of the poisoned segment is NaN"
        mask = torch.ones(outs[k].shape[:2], dtype=torch.bool, device=DEV)
        mask[series, seg] = False
        assert torch.equal(outs[k][mask], clean[k][mask]), f"{k} of every other segment keeps its bits"
    for k in POINT_OUTS + PROJ_OUTS:
        assert bool(torch.isnan(outs[k][series, point]).all()), f"{k} of the poisoned point is NaN"
        mask = torch.ones(outs[k].shape[:2], dtype=torch.bool, device=DEV)
        mask[series, point] = False
        assert torch.equal(outs[k][mask], clean[k][mask]), f"{k} of every other point keeps its bits"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_no_points_and_no_series(dtype):
    ms, dt, pair = 2, 1, 4
    empty = dict(offsets=np.zeros((2, 4), dtype=np.int64), a=np.zeros((2, 0, ms)), wt=np.zeros((2, 0, 2 * dt)), c=np.zeros((2, 0)),
                 y=np.zeros((2, 0)), pair_mean=np.ones((2, 3, pair)), pair_cov=np.ones((2, 3, pair, pair)))
    rc, outs = launch(L.GAUSSIAN, 20, dtype, empty)
    assert rc == 0 and all(float(outs[k].abs().max()) == 0.0 for k in SEG_OUTS), "N = 0: every segment gets zeros"
    lib = _lib.load()
    assert int(lib.mf_lik_st_expectations_workspace_bytes(0, ms, 2 * dt, 8)) == 0
    nodes, weights = c_rule(20)
    buf = torch.full((8,), SENTINEL, dtype=dtype, device=DEV)
    rc = _lib.call_rc(FN, dtype, 0, 5, 3, ms, 2 * dt, 0, c_params(L.GAUSSIAN), 20, nodes, weights, *([None] * 7), 0, None, None, None, 0,
                      _lib.ptr(buf), *([None] * 7), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.all(buf == SENTINEL)), "B = 0: nothing is launched"


def test_every_bad_argument_is_refused_and_nothing_is_written():
    dtype = torch.float64
    ref = reference(2, 1, L.GAUSSIAN, 20, False)
    bsz, n, ms = ref["a"].shape
    two_dt, segs = 2, ref["offsets"].shape[1] - 1
    pair = ms * two_dt
    tiles, tile_seg, seg_tile = tile_table(ref["offsets"])
    table = [torch.tensor(v, dtype=torch.int64, device=DEV) for v in (ref["offsets"], tile_seg, seg_tile)]
    ins = [dev(ref[k], dtype) for k in ("a", "wt", "c", "y", "pair_mean", "pair_cov")]
    shapes = [(bsz, segs), (bsz, segs, pair), (bsz, segs, pair, pair), (bsz, n, ms), (bsz, n, two_dt), (bsz, n), (bsz, n), (bsz, n)]
    outs = [torch.full(s, SENTINEL, dtype=dtype, device=DEV) for s in shapes]
    ws_bytes = int(_lib.load().mf_lik_st_expectations_workspace_bytes(tiles, ms, two_dt, 8))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    nodes, weights = c_rule(20)
    good = [bsz, n, segs, ms, two_dt, 0, c_params(L.GAUSSIAN), 20, nodes, weights, _lib.ptr(table[0]), *[_lib.ptr(t) for t in ins], tiles,
            _lib.ptr(table[1]), _lib.ptr(table[2]), _lib.ptr(ws), ws_bytes, *[_lib.ptr(o) for o in outs], _lib.stream_ptr(DEV)]
    zero_weights = host_array((0.0,) * 20)
    bad = [(1, -1, -1), (2, -1, -2), (3, 0, -3), (4, 0, -100), (4, 65, -100), (5, 3, -100), (5, 0, -100), (5, 130, -100), (6, 4, -6),
           (7, None, -7), (7, host_array((-1.0,)), -7), (8, 0, -8), (8, 33, -8), (9, None, -9), (10, None, -10), (10, zero_weights, -10),
           (11, None, -11), (12, None, -12), (13, None, -13), (14, None, -14), (15, None, -15), (16, None, -16), (17, None, -17),
           (18, -1, -18), (18, 2 ** 31, -18), (19, None, -19), (20, None, -20), (21, None, -21), (22, ws_bytes - 1, -22), (24, None, -24),
           (25, None, -25), (26, None, -26), (27, None, -27), (28, None, -28)]
    for position, value, code in bad:
        args = list(good)
        args[position - 1] = value
        assert _lib.call_rc(FN, dtype, *args) == code, f"argument {position} = {value!r}"
    args = list(good)
    args[3], args[4] = 33, 4                       # Ms d_t = 66
    assert _lib.call_rc(FN, dtype, *args) == -100
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in outs), "an error return launches nothing"
    assert _lib.call_rc(FN, dtype, *good) == 0
    torch.cuda.synchronize()
    assert not any(bool(torch.any(o == SENTINEL)) for o in outs)
