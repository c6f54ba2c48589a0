"""
GPU tests of ``mf_lik_iw_log_weights_*`` (csrc/mf_lik.hip) through the raw C ABI, against the numpy statement of its formulas in
tests/helpers/iwvi_closed_forms.py (``iw_log_weights``).

Tolerances, in the scheme of tests/test_gpu_svgp_kernel.py.
  float64: ``|err| <= K eps (magnitude + 1)``, eps = 2^-52, K = 64, with the helper's magnitudes: with
    fmag_n = sum_i |h_i s_i| + sum_i |w_i| (|prior_i| + |u_i|), sum_n (|l_n| + |l'_n| fmag_n) for log_lik and
    sum_n (|l'_n| + |l''_n| fmag_n) |w_n,.| for g_u.  check() prints every ratio ("RATIO f64 ...").
  float32: the kernel's error, normalised by (magnitude + 1) and maximised over an output of one series, against 4 x the same figure
    of the helper evaluated in numpy float32 on the same (float32-rounded) inputs; the helper sums in the kernel's order (the points
    of a tile of 64 ascending, then the tiles, then the two segments of g_u), and both errors are taken against the float64 helper.
  Measured maxima on an MI355X over all the cases of this file.  float64: log_lik 1.58, g_u 1.25 (of the 64 allowed).  float32, per
    series: log_lik at most 2.99 x the helper's figure (Poisson, K = 1, the emission row of a sum kernel, series 1: 8.2e-8 against
    2.7e-8), g_u 3.15 x (Student-t, 2d = 14, series 2: 3.3e-8 against 1.0e-8); the largest normalised errors are 2.9e-7 and 3.9e-7.
    The per-launch maximum that tests/test_gpu_svgp_kernel.py needs for its float32 value sum is not needed here.

Every series has N = 390 points in S = 5 segments (M = 4 inducing points) whose lengths are drawn from {0, 1, 3, 63, 64, 65, 130, 195}:
a tile is 64 points, so segments of one, two, three and four tiles are combined, both sides of a tile boundary are met, segments are
empty and so are the first and the last one.  K = 5 samples (one chunk of 8), K = 1 for a sample alone and K = 9 for a chunk and one.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import iwvi_closed_forms as IW
from helpers import likelihood_closed_forms as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
K_F64 = 64.0
NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
DTYPES = [torch.float64, torch.float32]
GUARD, SENTINEL = 64, -77.25
TILE = 64
CHUNK = 8                       # samples per block of pass 1
LAYOUT = ((0, 1, 64, 130, 195), (195, 65, 130, 0, 0), (63, 65, 64, 195, 3))      # three series, N = 390 each
OUTS = ("log_lik", "g_u")
FN = "mf_lik_iw_log_weights"
SUM_PATTERN = (1.0, 0.0, 0.0, 1.0)          # the emission row of Matern52 + Matern12


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


def tile_table(offsets):
    """``(num_tiles, tile_seg, seg_tile)`` of ``offsets [B, S + 1]``, in plain numpy."""
    per = (np.diff(offsets, axis=1).reshape(-1) + TILE - 1) // TILE
    return int(per.sum()), np.repeat(np.arange(per.size), per).astype(np.int64), np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


def freeze(ref):
    for v in ref.values():
        for a in (v if isinstance(v, list) else [v]):
            for x in (a.values() if isinstance(a, dict) else [a]):
                x.setflags(write=False)
    return ref


def evaluate(name, ref, f32, final=False):
    """The float64 helper per series (and the float32 one) on the inputs of ``ref``; ``final``: the mode without ``u_post``."""
    lik = L.LIKELIHOODS[name]
    per = lambda b, dtype: IW.iw_log_weights(lik, ref["h"], None if final else ref["w"][b], ref["y"][b], ref["offsets"][b],     # noqa: E731
                                            ref["states"][:, b], None if final else ref["u_post"][:, b], dtype)
    ref["want"] = [per(b, np.float64) for b in range(ref["y"].shape[0])]
    if f32:
        ref["want32"] = [per(b, np.float32) for b in range(ref["y"].shape[0])]
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, two_d, f32, k=5, h=None, layout=LAYOUT):
    """Inputs (rounded to the dtype under test) and the helper on them, per series - computed once per case and shared, read-only."""
    ref = IW.random_case(name, two_d, layout, k, seed=two_d * 100 + k, f32=f32, h=h)
    return freeze(evaluate(name, ref, f32))


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def guarded(shape, dtype):
    """A sentinel-filled buffer of ``shape`` followed by a sentinel-filled guard region."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def launch(name, dtype, ref, series=None, sample=None, want=(True, True), final=False):
    """One call on all the series and samples of ``ref`` (or on ``series`` / ``sample`` alone).  ``final``: without ``u_post`` and
    ``w``.  Returns ``(rc, [log_lik, g_u])`` as tensors (None where not asked for) after checking every guard region."""
    pick = (lambda a: a) if series is None else (lambda a: a[series:series + 1])
    pick_k = (lambda a: pick(a.swapaxes(0, 1)).swapaxes(0, 1)) if sample is None else \
        (lambda a: pick(a[sample:sample + 1].swapaxes(0, 1)).swapaxes(0, 1))
    states = pick_k(ref["states"])
    k, bsz, _, d = states.shape
    offsets = pick(ref["offsets"])
    segs, n = offsets.shape[1] - 1, pick(ref["y"]).shape[1]
    tiles, tile_seg, seg_tile = tile_table(offsets)
    table = [torch.tensor(a, dtype=torch.int64, device=DEV).contiguous() for a in (offsets, tile_seg, seg_tile)]
    w = None if final else dev(pick(ref["w"]), dtype)
    u_post = None if final else dev(pick_k(ref["u_post"]), dtype)
    ins = [w, dev(pick(ref["y"]), dtype), dev(ref["h"], dtype), dev(states, dtype), u_post]
    shapes = ((k, bsz, segs), (k, bsz, segs - 1, d))
    outs = [guarded(s, dtype) if wanted else (None, None) for s, wanted in zip(shapes, want)]
    ws_bytes = int(_lib.load().mf_lik_iw_log_weights_workspace_bytes(tiles, k, 2 * d, ins[1].element_size()))
    assert ws_bytes == tiles * k * (2 * d + 1) * ins[1].element_size()
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = _lib.call_rc(FN, dtype, bsz, n, segs, 2 * d, k, L.IDS[name], c_params(name), _lib.ptr(table[0]),
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
        ratio = float(scaled.max() / EPS) if scaled.size else 0.0
        print(f"RATIO f64 {what}: {ratio:.2f}")
        if ratio > K_F64:
            return f"{what}: {ratio:.1f} eps (magnitude + 1) at {np.unravel_index(int(scaled.argmax()), scaled.shape)}"
    else:
        own = float((np.abs(np.asarray(got32, dtype=np.float64) - want) / (np.asarray(mag) + 1.0)).max())
        print(f"ERR f32 {what}: kernel {scaled.max():.3e}  numpy float32 {own:.3e}  ({scaled.max() / own if own else float(scaled.max() > 0):.2f} x)")
        if scaled.max() > 4.0 * own:
            return f"{what}: kernel {scaled.max():.3e} against numpy float32 {own:.3e}"
    return None


def check_against_helper(tag, ref, dtype, outs):
    """Every series and every output on its own; every figure is printed before the first failure is raised."""
    f32 = dtype == torch.float32
    failures = []
    for b in range(len(ref["want"])):
        want = ref["want"][b]
        own = ref["want32"][b] if f32 else {}
        for key, got in zip(OUTS, outs):
            if got is not None:
                assert not bool(torch.any(got[:, b] == SENTINEL)), f"{tag} series {b} {key}: an element was not written"
                failures.append(check(f"{tag} series {b} {key}", got[:, b].cpu().numpy(), want[key], want["mag_" + key], dtype,
                                      own.get(key)))
    failures = [f for f in failures if f]
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("two_d", [2, 4, 6, 8, 10, 12, 14, 16, 18])
@pytest.mark.parametrize("name", NAMES)
def test_batch_of_three_against_the_helper_and_every_series_and_sample_alone_bit_for_bit(name, two_d, dtype):
    ref = reference(name, two_d, dtype == torch.float32)
    rc, outs = launch(name, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} 2d={two_d}", ref, dtype, outs)
    log_lik, g_u = outs
    # empty segments: exact zeros; an inducing point between two empty segments gets a zero adjoint
    for b, ln in enumerate(LAYOUT):
        for s, count in enumerate(ln):
            if count == 0:
                assert float(log_lik[:, b, s].abs().max()) == 0.0
                if s + 1 < len(ln) and ln[s + 1] == 0:
                    assert float(g_u[:, b, s].abs().max()) == 0.0
    rc, again = launch(name, dtype, ref)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(again, outs)), "two launches on the same inputs return the same bits"
    for b in range(3):
        rc, one = launch(name, dtype, ref, series=b)
        assert rc == 0
        assert all(torch.equal(o[:, 0], f[:, b]) for o, f in zip(one, outs)), "a series alone gives the bits it gives in a batch"
    for k in range(5):
        rc, one = launch(name, dtype, ref, sample=k)
        assert rc == 0
        assert all(torch.equal(o[0], f[k]) for o, f in zip(one, outs)), "a sample alone gives the bits it gives among K"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", [L.BERNOULLI, L.POISSON])
def test_one_sample_more_than_a_chunk(name, dtype):
    ref = reference(name, 6, dtype == torch.float32, k=CHUNK + 1)
    rc, outs = launch(name, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} K={CHUNK + 1}", ref, dtype, outs)
    for k in (0, CHUNK - 1, CHUNK):
        rc, one = launch(name, dtype, ref, sample=k)
        assert rc == 0 and all(torch.equal(o[0], f[k]) for o, f in zip(one, outs)), "the sample of the second chunk too"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_a_single_sample_and_the_emission_row_of_a_sum_kernel(name, dtype):
    ref = reference(name, 8, dtype == torch.float32, k=1, h=SUM_PATTERN)
    rc, outs = launch(name, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} K=1 h=sum", ref, dtype, outs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("two_d", [6, 18])
def test_value_only_and_adjoint_only_calls_return_the_same_bits(two_d, dtype):
    ref = reference(L.BERNOULLI, two_d, dtype == torch.float32)
    rc, full = launch(L.BERNOULLI, dtype, ref)
    assert rc == 0
    rc, value = launch(L.BERNOULLI, dtype, ref, want=(True, False))
    assert rc == 0 and value[1] is None and torch.equal(value[0], full[0])
    rc, grad = launch(L.BERNOULLI, dtype, ref, want=(False, True))
    assert rc == 0 and grad[0] is None and torch.equal(grad[1], full[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_final_samples_equal_the_corrected_mode_with_a_vanishing_correction(name, dtype):
    """Without ``u_post`` the states are final; fed with ``u_post`` = the prior at the inducing rows (every delta is 0) the corrected
    mode returns the same bits in ``log_lik``."""
    f32 = dtype == torch.float32
    base = reference(name, 6, f32)
    same = dict(base)
    same["u_post"] = base["prior_z"]
    rc, corrected = launch(name, dtype, same, want=(True, False))
    assert rc == 0
    final = dict(base)
    rows = np.stack([IW.rows_of(base["offsets"][b])[1] for b in range(3)])
    final["states"] = np.stack([base["states"][:, b, rows[b]] for b in range(3)], axis=1)
    rc, outs = launch(name, dtype, final, want=(True, False), final=True)
    assert rc == 0 and torch.equal(outs[0], corrected[0])
    check_against_helper(f"{name} final", evaluate(name, final, f32, final=True), dtype, outs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_a_nan_in_the_prior_draw_poisons_its_own_sample_and_segment_only(name, dtype):
    ref = dict(reference(name, 6, dtype == torch.float32))
    rc, clean = launch(name, dtype, ref)
    assert rc == 0
    states = ref["states"].copy()
    # sample 2, series 0: point 70 of the 130 of segment 3 (its second tile), at row n + s
    states[2, 0, (65 + 70) + 3, 0] = float("nan")
    ref["states"] = states
    rc, outs = launch(name, dtype, ref)
    assert rc == 0
    for k in range(5):
        for b in range(3):
            for s in range(5):
                if (k, b, s) == (2, 0, 3):
                    assert bool(torch.isnan(outs[0][k, b, s]))
                else:
                    assert torch.equal(outs[0][k, b, s], clean[0][k, b, s]), "every other value keeps its bits"
            for m in range(4):
                if (k, b) == (2, 0) and m in (2, 3):
                    assert bool(torch.isnan(outs[1][k, b, m]).all()), "the adjoints of the segment's two inducing points"
                else:
                    assert torch.equal(outs[1][k, b, m], clean[1][k, b, m]), "every other adjoint keeps its bits"


def test_no_points_writes_zeros_and_no_series_or_samples_launch_nothing():
    dtype = torch.float64
    s = _lib.stream_ptr(DEV)
    # N = 0 needs no input, no table and no workspace
    out = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((3, 2, 5), (3, 2, 4, 2))]
    one = torch.zeros(8, dtype=dtype, device=DEV)
    assert _lib.call_rc(FN, dtype, 2, 0, 5, 4, 3, 1, None, *([None] * 5), _lib.ptr(one), 0, None, None, None, 0,
                        *[_lib.ptr(o) for o in out], s) == 0
    torch.cuda.synchronize()
    assert all(float(o.abs().max()) == 0.0 for o in out), "N = 0: every output is zero"
    value = torch.full((3, 2, 5), SENTINEL, dtype=dtype, device=DEV)
    assert _lib.call_rc(FN, dtype, 2, 0, 5, 4, 3, 1, None, *([None] * 6), 0, None, None, None, 0, _lib.ptr(value), None, s) == 0
    torch.cuda.synchronize()
    assert float(value.abs().max()) == 0.0
    out = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((3, 2, 5), (3, 2, 4, 2))]
    assert _lib.call_rc(FN, dtype, 0, 0, 5, 4, 3, 1, None, *([None] * 5), _lib.ptr(one), 0, None, None, None, 0, *[_lib.ptr(o) for o in out], s) == 0
    assert _lib.call_rc(FN, dtype, 2, 0, 5, 4, 0, 1, None, *([None] * 5), _lib.ptr(one), 0, None, None, None, 0, *[_lib.ptr(o) for o in out], s) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in out), "B = 0 or K = 0: nothing is written"


def test_bad_arguments_return_their_codes_and_launch_nothing():
    dtype = torch.float64
    ref = reference(L.STUDENTT, 4, False)
    tiles, tile_seg, seg_tile = tile_table(ref["offsets"])
    table = [torch.tensor(a, dtype=torch.int64, device=DEV) for a in (ref["offsets"], tile_seg, seg_tile)]
    ins = [dev(ref[k], dtype) for k in ("w", "y", "h", "states", "u_post")]
    io = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((5, 3, 5), (5, 3, 4, 2))]
    ws_bytes = tiles * 5 * 5 * 8
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    par, s = c_params(L.STUDENTT), _lib.stream_ptr(DEV)
    p = [_lib.ptr(table[0])] + [_lib.ptr(t) for t in ins]
    tb, o = [_lib.ptr(table[1]), _lib.ptr(table[2]), _lib.ptr(ws)], [_lib.ptr(t) for t in io]

    def call(bsz=3, n=390, segs=5, two_d=4, k=5, lik=3, params=par, ptrs=p, nt=tiles, tab=tb, nbytes=ws_bytes, outs=o):
        return _lib.call_rc(FN, dtype, bsz, n, segs, two_d, k, lik, params, *ptrs, nt, *tab, nbytes, *outs, s)

    assert call(bsz=-1) == -1 and call(n=-1) == -2 and call(segs=0) == -3
    for two_d in (0, 1, 3, 5, 20, -2):
        assert call(two_d=two_d) == -100
    assert call(k=-1) == -5 and call(lik=7) == -6 and call(params=None) == -7
    for i in range(5):
        assert call(ptrs=p[:i] + [None] + p[i + 1:]) == -(8 + i)
    assert call(ptrs=p[:5] + [None]) == -20, "the adjoint needs u_post"
    assert call(nt=-1) == -14 and call(nt=2 ** 31) == -14 and call(n=0) == -14          # tiles without points
    for i in range(3):
        assert call(tab=tb[:i] + [None] + tb[i + 1:]) == -(15 + i)
    assert call(nbytes=ws_bytes - 1) == -18 and call(nbytes=0) == -18
    assert call(outs=[None, None]) == 0                                 # nothing asked for
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in io)
    assert int(_lib.load().mf_lik_iw_log_weights_workspace_bytes(0, 5, 4, 8)) == 0
    assert int(_lib.load().mf_lik_iw_log_weights_workspace_bytes(7, 5, 5, 8)) == 0
    with pytest.raises(NotImplementedError):
        _lib.call(FN, dtype, 3, 390, 5, 20, 5, 3, par, *p, tiles, *tb, ws_bytes, *o, s)
    with pytest.raises(ValueError, match="invalid argument #6"):
        _lib.call(FN, dtype, 3, 390, 5, 4, 5, 9, par, *p, tiles, *tb, ws_bytes, *o, s)
