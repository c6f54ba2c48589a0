"""
GPU tests of ``mf_lik_st_cvi_site_update_*`` (csrc/mf_st.hip) through the raw C ABI, with a guard region behind ``nat1``, ``nat2``,
every optional output and the workspace, against the literal numpy statement of the reference's update in
tests/helpers/st_cvi_closed_forms.py.

Shapes: those of tests/test_gpu_st_kernel.py - its ``LAYOUT``, three series of 579 points in segments of 0, 1, 256, 257 and 65
points in three orders, and its inputs - at ``(Ms, d_t)`` = (1,1), (5,3), (21,3), (32,2) and (64,1): pair dimensions 2, 30, 126, 128,
128, one and several slabs, a partial slab, the padding of W, both slab heights.  Gaussian and Bernoulli everywhere, all four
likelihoods at (5,3).  Two starts: zero sites at ``lr = 1`` (the sites become the site sums) and random symmetric sites at
``lr = 0.3`` (rounded to the dtype under test).

Accuracy, the project's rule (CHANGELOG, "limit 4 x"): the YARDSTICK of an output is the error of ``st_cvi_site_update_torch`` in the
dtype under test against the helper one precision up - float64 for float32, numpy.longdouble for float64 - on the inputs of the case
and seven more draws, normalised element by element by eps x the output's magnitude (``mag_*`` of the helper), maximised over the
elements, the series and those 8 seeds and floored at 1.  scripts/st_cvi_yardsticks.py measures it on the CPU and records it in
tests/golden/st_cvi_yardsticks.json per (Ms, d_t), dtype, likelihood, start and output.  The kernel's normalised error, against the
same helper, may be at most 4 x the yardstick; ``check_against_helper`` prints every ratio (``RATIO ...``).
Measured worst ratios kernel / yardstick on an MI355X over every case of this file (allowed: 4), float64 / float32:
nat1 1.43 / 1.51, nat2 1.27 / 1.71, ve_sum 0.93 / 1.05.  The yardsticks lie between 1 and 1.9 eps x magnitude for ``nat1`` (its magnitude counts
``|gm| + 2 |gv| |fmu|`` per point), 1.3 and 11.2 for ``nat2`` (the largest: the Gaussian likelihood at (64,1) in float32) and 3.6 and 6.3
for ``ve_sum``.

The exact statements - bits of ``mf_lik_st_expectations_*`` from zero sites, symmetry, ``lr = 0``, empty segments, repeats, a series
alone, the output combinations, the poisoned point - would each catch a wrong index that a tolerance lets through.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import likelihood_closed_forms as L
from helpers import st_cvi_closed_forms as STC
import test_gpu_st_kernel as K

pytestmark = pytest.mark.gpu
DEV = K.DEV
GUARD, SENTINEL = K.GUARD, K.SENTINEL
LAYOUT = K.LAYOUT
SIZES = [(1, 1), (5, 3), (21, 3), (32, 2), (64, 1)]
ALL_LIKS = {(5, 3)}
NAMES = K.NAMES
DTYPES = K.DTYPES
CASES = [(ms, dt, name) for ms, dt in SIZES for name in (NAMES if (ms, dt) in ALL_LIKS else NAMES[:2])]
FN = "mf_lik_st_cvi_site_update"
OPT_OUTS = ("ve_sum", "fmu", "fvar")
CHECKED = ("nat1", "nat2", "ve_sum")
STARTS = ("zero", "sym")
YARD_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "st_cvi_yardsticks.json")


def learning_rate(start, f32):
    """1 from zero sites, 0.3 - as the dtype under test holds it - from the random ones."""
    return 1.0 if start == "zero" else (float(np.float32(0.3)) if f32 else 0.3)


def yard_key(ms, dt, dtype, name, start):
    return f"{ms}x{dt}/{'f32' if dtype == torch.float32 else 'f64'}/{name}/{start}"


@functools.lru_cache(maxsize=None)
def yardsticks():
    with open(YARD_FILE) as f:
        return json.load(f)


def draw_sites(ms, dt, f32, layout, seed, start):
    """The old sites ``(nat1 [B, S, n], nat2 [B, S, n, n])`` rounded to the dtype under test: zeros, or random with a symmetric
    ``nat2``."""
    bsz, segs, pair = len(layout), len(layout[0]), 2 * ms * dt
    if start == "zero":
        return np.zeros((bsz, segs, pair)), np.zeros((bsz, segs, pair, pair))
    rng = np.random.default_rng(seed + 500009)
    ty = np.float32 if f32 else np.float64
    nat1 = rng.normal(size=(bsz, segs, pair)).astype(ty)
    root = rng.normal(size=(bsz, segs, pair, pair)).astype(ty)
    nat2 = ty(-0.5) * (root + root.transpose(0, 1, 3, 2))          # (formed in the dtype: an addition commutes, so symmetric bit for bit)
    return nat1.astype(np.float64), nat2.astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(ms, dt, name, f32, layout=LAYOUT):
    """The inputs of tests/test_gpu_st_kernel.py's case, both starts and the helper one precision up on them, per series - computed
    once per case and shared, read-only."""
    seed = K.case_seed(ms, dt, 20)
    ref = K.draw_inputs(ms, dt, name, f32, layout, seed)
    up = np.float64 if f32 else np.longdouble
    sums = [STC.st_cvi_site_sums(L.LIKELIHOODS[name], ref["a"][b], ref["wt"][b], ref["c"][b], ref["y"][b], ref["offsets"][b],
                                 ref["pair_mean"][b], ref["pair_cov"][b], 20, up) for b in range(len(layout))]
    ref["sites"], ref["want"] = {}, {}
    for start in STARTS:
        nat1, nat2 = draw_sites(ms, dt, f32, layout, seed, start)
        ref["sites"][start] = (nat1, nat2)
        ref["want"][start] = [{**{k: v for k, v in sums[b].items() if "theta" not in k},
                               **STC.blend(sums[b], learning_rate(start, f32), nat1[b], nat2[b], up)} for b in range(len(layout))]
    return ref


def launch(name, dtype, ref, lr, sites, series=None, want=OPT_OUTS, nq=20):
    """One call on all the series of ``ref`` (or on ``series`` alone) from a copy of ``sites``.  Returns ``(rc, {name: tensor})``
    with the new sites and the optional outputs, after checking every guard region."""
    pick = (lambda v: v) if series is None else (lambda v: v[series:series + 1])
    bsz, n, ms = pick(ref["a"]).shape
    two_dt = ref["wt"].shape[-1]
    pair = ms * two_dt
    offsets = pick(ref["offsets"])
    segs = offsets.shape[1] - 1
    tiles, tile_seg, seg_tile = K.tile_table(offsets)
    table = [torch.tensor(v, dtype=torch.int64, device=DEV).contiguous() for v in (offsets, tile_seg, seg_tile)]
    ins = [K.dev(pick(ref[k]), dtype) for k in ("a", "wt", "c", "y", "pair_mean", "pair_cov")]
    bufs = {}
    for key, value in zip(("nat1", "nat2"), sites):
        bufs[key] = K.guarded(pick(value).shape, dtype)
        bufs[key][1].copy_(K.dev(pick(value), dtype))
    shapes = dict(ve_sum=(bsz, segs), fmu=(bsz, n), fvar=(bsz, n))
    for key in OPT_OUTS:
        bufs[key] = K.guarded(shapes[key], dtype) if key in want else (None, None)
    esize = ins[0].element_size()
    ws_bytes = int(_lib.load().mf_lik_st_cvi_site_update_workspace_bytes(tiles, ms, two_dt, esize))
    assert ws_bytes == tiles * (pair * (pair + 1) // 2 + pair + 1) * esize
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    nodes, weights = K.c_rule(nq)
    rc = _lib.call_rc(FN, dtype, bsz, n, segs, ms, two_dt, L.IDS[name], K.c_params(name), nq, nodes, weights, _lib.ptr(table[0]),
                      *[_lib.ptr(t) for t in ins], tiles, _lib.ptr(table[1]), _lib.ptr(table[2]), _lib.ptr(ws), ws_bytes, lr,
                      _lib.ptr(bufs["nat1"][1]), _lib.ptr(bufs["nat2"][1]), *[_lib.ptr(bufs[k][1]) for k in OPT_OUTS],
                      _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert all(b[0] is None or bool(torch.all(b[0][-GUARD:] == SENTINEL)) for b in bufs.values()), "a write past the end of an output"
    assert bool(torch.all(ws[ws_bytes:] == 0x5A)), "a write past the end of the workspace"
    return rc, {k: v[1] for k, v in bufs.items()}


def check_against_helper(tag, key, want_all, dtype, outs, series=None):
    """Every series, ``nat1``, ``nat2`` and ``ve_sum``: the normalised error against 4 x the recorded yardstick.  Every figure is
    printed before the first failure is raised."""
    yard = yardsticks()[key]
    rows = list(range(len(want_all))) if series is None else [series]
    failures = []
    for i, b in enumerate(rows):
        want = want_all[b]
        for out in CHECKED:
            got = outs[out]
            got_np = got[i].cpu().numpy().astype(np.float64)
            assert np.all(np.isfinite(got_np)), f"{tag} series {b} {out}: non-finite result"
            err = np.abs(got_np - want[out].astype(np.float64) if want[out].dtype != np.longdouble
                         else (got_np.astype(np.longdouble) - want[out]).astype(np.float64))
            mag = np.asarray(want["mag_" + out])
            scaled = np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), np.where(err > 0, np.inf, 0.0)) / K.EPS[dtype]
            worst = float(scaled.max()) if scaled.size else 0.0
            print(f"RATIO {key} series {b} {out}: {worst:.2f} eps mag, yardstick {yard[out]:.2f}, {worst / yard[out]:.2f} x")
            if worst > 4.0 * yard[out]:
                failures.append(f"{tag} series {b} {out}: {worst:.2f} eps mag against a yardstick of {yard[out]:.2f}")
    assert not failures, "; ".join(failures)


def one_minus_times(sites, lr, dtype):
    """``(1 - lr) nat`` as the kernel forms it: ``1 - lr`` once in the dtype, one multiplication."""
    one_minus = torch.tensor(1.0, dtype=dtype, device=DEV) - torch.tensor(lr, dtype=dtype, device=DEV)
    return [one_minus * K.dev(v, dtype) for v in sites]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ms,dt,name", CASES)
def test_both_starts_against_the_helper_and_the_exact_statements(ms, dt, name, dtype):
    f32 = dtype == torch.float32
    ref = reference(ms, dt, name, f32)
    # ---- zero sites, lr = 1: the sites are the site sums, with the bits mf_lik_st_expectations_* gives on the same inputs
    rc, zero = launch(name, dtype, ref, 1.0, ref["sites"]["zero"])
    assert rc == 0
    check_against_helper(f"{name} {ms}x{dt} zero", yard_key(ms, dt, dtype, name, "zero"), ref["want"]["zero"], dtype, zero)
    rc, expect = K.launch(name, 20, dtype, ref, want=("ve_sum", "g_mean", "g_cov", "fmu", "fvar"))
    assert rc == 0
    assert torch.equal(zero["nat2"], expect["g_cov"]), "from zero sites at lr = 1, nat2 has the bits of g_cov"
    assert all(torch.equal(zero[k], expect[k]) for k in OPT_OUTS), "ve_sum, fmu and fvar have the bits of mf_lik_st_expectations_*"
    assert torch.equal(zero["nat2"], zero["nat2"].transpose(-1, -2)), "nat2 is symmetric bit for bit"
    # ---- random symmetric sites, lr = 0.3
    lr, sites = learning_rate("sym", f32), ref["sites"]["sym"]
    rc, sym = launch(name, dtype, ref, lr, sites)
    assert rc == 0
    check_against_helper(f"{name} {ms}x{dt} sym", yard_key(ms, dt, dtype, name, "sym"), ref["want"]["sym"], dtype, sym)
    assert torch.equal(sym["nat2"], sym["nat2"].transpose(-1, -2)), "a symmetric nat2 stays symmetric bit for bit"
    assert all(torch.equal(sym[k], zero[k]) for k in OPT_OUTS), "the optional outputs do not depend on the sites"
    decayed = one_minus_times(sites, lr, dtype)
    for b, ln in enumerate(LAYOUT):
        for s, count in enumerate(ln):
            if count == 0:
                assert torch.equal(sym["nat1"][b, s], decayed[0][b, s]) and torch.equal(sym["nat2"][b, s], decayed[1][b, s]), \
                    "an empty segment: exactly (1 - lr) nat"
                assert float(sym["ve_sum"][b, s]) == 0.0
    rc, again = launch(name, dtype, ref, lr, sites)
    assert rc == 0 and all(torch.equal(again[k], sym[k]) for k in sym), "two launches from the same start return the same bits"
    for b in range(3):
        rc, one = launch(name, dtype, ref, lr, sites, series=b)
        assert rc == 0
        assert all(torch.equal(one[k][0], sym[k][b]) for k in sym), "a series alone gives the bits it gives in a batch"
    # ---- lr = 0: finite sites keep their bits
    rc, kept = launch(name, dtype, ref, 0.0, sites)
    assert rc == 0 and torch.equal(kept["nat1"], K.dev(sites[0], dtype)) and torch.equal(kept["nat2"], K.dev(sites[1], dtype))


# every subset of the three optional outputs, 8 in all
COMBOS = [tuple(k for i, k in enumerate(OPT_OUTS) if mask >> i & 1) for mask in range(8)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ms,dt", [(5, 3), (32, 2)])
def test_every_output_combination_leaves_the_bits_of_the_sites_unchanged(ms, dt, dtype):
    f32 = dtype == torch.float32
    ref = reference(ms, dt, L.BERNOULLI, f32)
    lr, sites = learning_rate("sym", f32), ref["sites"]["sym"]
    rc, full = launch(L.BERNOULLI, dtype, ref, lr, sites)
    assert rc == 0 and len(set(COMBOS)) == 8
    for want in COMBOS:
        rc, part = launch(L.BERNOULLI, dtype, ref, lr, sites, want=want)
        assert rc == 0
        assert torch.equal(part["nat1"], full["nat1"]) and torch.equal(part["nat2"], full["nat2"]), f"the sites of the call for {want}"
        for k in OPT_OUTS:
            assert (part[k] is None) == (k not in want)
            if k in want:
                assert torch.equal(part[k], full[k]), f"{k} in the call for {want} differs from {k} in the full call"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_negative_variance_poisons_its_own_segment_only(dtype):
    ms, dt = 5, 3
    f32 = dtype == torch.float32
    base = reference(ms, dt, L.BERNOULLI, f32)
    lr, sites = learning_rate("sym", f32), base["sites"]["sym"]
    rc, clean = launch(L.BERNOULLI, dtype, base, lr, sites)
    assert rc == 0
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    series, seg = 1, 3                             # a full row of series 1; its point 7
    assert LAYOUT[series][seg] == K.T
    point = int(base["offsets"][series, seg]) + 7
    bad["c"][series, point] = -1e6
    rc, outs = launch(L.BERNOULLI, dtype, bad, lr, sites)
    assert rc == 0
    for k in CHECKED:
        assert bool(torch.isnan(outs[k][series, seg]).all()), f"{k} of the poisoned segment is NaN"
        mask = torch.ones(outs[k].shape[:2], dtype=torch.bool, device=DEV)
        mask[series, seg] = False
        assert torch.equal(outs[k][mask], clean[k][mask]), f"{k} of every other segment and series keeps its bits"
    for k in ("fmu", "fvar"):
        assert bool(torch.isnan(outs[k][series, point]))
        mask = torch.ones(outs[k].shape[:2], dtype=torch.bool, device=DEV)
        mask[series, point] = False
        assert torch.equal(outs[k][mask], clean[k][mask]), f"{k} of every other point keeps its bits"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_no_points_and_no_series(dtype):
    ms, dt, pair = 2, 1, 4
    f32 = dtype == torch.float32
    empty = dict(offsets=np.zeros((2, 4), dtype=np.int64), a=np.zeros((2, 0, ms)), wt=np.zeros((2, 0, 2 * dt)), c=np.zeros((2, 0)),
                 y=np.zeros((2, 0)), pair_mean=np.ones((2, 3, pair)), pair_cov=np.ones((2, 3, pair, pair)))
    lr = learning_rate("sym", f32)
    sites = draw_sites(ms, dt, f32, ((0, 0, 0), (0, 0, 0)), 3, "sym")
    rc, outs = launch(L.GAUSSIAN, dtype, empty, lr, sites)
    decayed = one_minus_times(sites, lr, dtype)
    assert rc == 0 and torch.equal(outs["nat1"], decayed[0]) and torch.equal(outs["nat2"], decayed[1]), "N = 0: every site decays"
    assert float(outs["ve_sum"].abs().max()) == 0.0
    assert int(_lib.load().mf_lik_st_cvi_site_update_workspace_bytes(0, ms, 2 * dt, 8)) == 0
    nodes, weights = K.c_rule(20)
    buf1, buf2 = (torch.full((8,), SENTINEL, dtype=dtype, device=DEV) for _ in range(2))
    rc = _lib.call_rc(FN, dtype, 0, 5, 3, ms, 2 * dt, 0, K.c_params(L.GAUSSIAN), 20, nodes, weights, *([None] * 7), 0, None, None, None, 0,
                      0.5, _lib.ptr(buf1), _lib.ptr(buf2), None, None, None, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.all(buf1 == SENTINEL)) and bool(torch.all(buf2 == SENTINEL)), "B = 0: nothing is launched"


def test_every_bad_argument_is_refused_and_the_sites_are_untouched():
    dtype = torch.float64
    ref = reference(1, 1, L.GAUSSIAN, False)
    bsz, n, ms = ref["a"].shape
    two_dt, segs = 2, ref["offsets"].shape[1] - 1
    pair = ms * two_dt
    tiles, tile_seg, seg_tile = K.tile_table(ref["offsets"])
    table = [torch.tensor(v, dtype=torch.int64, device=DEV) for v in (ref["offsets"], tile_seg, seg_tile)]
    ins = [K.dev(ref[k], dtype) for k in ("a", "wt", "c", "y", "pair_mean", "pair_cov")]
    shapes = [(bsz, segs, pair), (bsz, segs, pair, pair), (bsz, segs), (bsz, n), (bsz, n)]
    outs = [torch.full(s, SENTINEL, dtype=dtype, device=DEV) for s in shapes]
    ws_bytes = int(_lib.load().mf_lik_st_cvi_site_update_workspace_bytes(tiles, ms, two_dt, 8))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    nodes, weights = K.c_rule(20)
    good = [bsz, n, segs, ms, two_dt, 0, K.c_params(L.GAUSSIAN), 20, nodes, weights, _lib.ptr(table[0]), *[_lib.ptr(t) for t in ins], tiles,
            _lib.ptr(table[1]), _lib.ptr(table[2]), _lib.ptr(ws), ws_bytes, 0.5, *[_lib.ptr(o) for o in outs], _lib.stream_ptr(DEV)]
    zero_weights = K.host_array((0.0,) * 20)
    bad = [(1, -1, -1), (2, -1, -2), (3, 0, -3), (4, 0, -100), (4, 65, -100), (5, 3, -100), (5, 0, -100), (5, 130, -100), (6, 4, -6),
           (7, None, -7), (7, K.host_array((-1.0,)), -7), (8, 0, -8), (8, 33, -8), (9, None, -9), (10, None, -10),
           (10, zero_weights, -10), (11, None, -11), (12, None, -12), (13, None, -13), (14, None, -14), (15, None, -15), (16, None, -16),
           (17, None, -17), (18, -1, -18), (18, 2 ** 31, -18), (19, None, -19), (20, None, -20), (21, None, -21), (22, ws_bytes - 1, -22),
           (23, -0.1, -23), (23, 1.5, -23), (23, float("nan"), -23), (24, None, -24), (25, None, -25)]
    for position, value, code in bad:
        args = list(good)
        args[position - 1] = value
        assert _lib.call_rc(FN, dtype, *args) == code, f"argument {position} = {value!r}"
    args = list(good)
    args[3], args[4] = 33, 4                       # Ms d_t = 66
    assert _lib.call_rc(FN, dtype, *args) == -100
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in outs), "an error return launches nothing: nat1 and nat2 are untouched"
    assert _lib.call_rc(FN, dtype, *good) == 0
    torch.cuda.synchronize()
    assert not any(bool(torch.any(o == SENTINEL)) for o in outs)
