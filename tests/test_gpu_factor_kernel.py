"""
GPU tests of ``mf_lik_sparse_factor_expectations_*`` (csrc/mf_lik_factor.hip) through the raw C ABI, against the numpy statement of
its formulas in tests/helpers/factor_closed_forms.py (``segment_expectations_factor``).  The scheme and the constants are those of
tests/test_gpu_multistage_kernel.py.

Tolerances.
  float64: ``|err| <= K eps (magnitude + 1)``, eps = 2^-52, K = 64, with the helper's magnitudes: the sums of the absolute values of
    the terms of every output (``mag_ve_sum``, ``mag_g_mean``, ``mag_g_cov``, ``mag_g_w``).  check() prints every ratio
    ("RATIO f64 ...").
  float32: the kernel's error, normalised by (magnitude + 1) and maximised over an output of one series, against 4 x the same figure
    of the helper evaluated in numpy float32 on the same (float32-rounded) inputs in the kernel's order of summation; both errors
    are taken against the float64 helper.  check() prints every figure ("ERR f32 ...").
  Measured maxima on an MI355X over all the cases of this file (2026-10-21).  float64 ratios, of the 64 allowed: ve_sum 1.98,
    g_mean 1.16, g_cov 1.66, g_w 36.0 - the last in the Bernoulli case (series 0 ... 2: 20.4, 36.0, 22.7), where the link's
    ``1 + erf`` cancels in the tails and the device's erf and scipy's differ by an ulp, as in tests/test_gpu_multistage_kernel.py's
    element-wise figures; every other likelihood stays below 2.3.  float32, of the 4 x allowed: ve_sum 3.25 x, g_mean 2.44 x,
    g_cov 1.95 x, g_w 1.80 x; the largest normalised float32 error 9.3e-06.

Every series has N = 390 points in S = 5 segments whose lengths are drawn from {0, 1, 3, 63, 64, 65, 130, 195}: a tile is 64 points, so
segments of one, two, three and four tiles are combined, both sides of a tile boundary are met and segments are empty.

The inputs keep the yardstick inside its domain by construction (``reference`` asserts it on the CPU): S_pair is a random SPD matrix
plus 0.1 I, Cg = c c^T / L + 0.05 I, wg is uniform in +-0.7 and W in +-1 (+-0.5 for the Poisson case), so every s2_p > 0 and every
Poisson mean mu_p + s2_p / 2 < 6, where the float32 exp cannot dominate.

The cases (L, 2d, P), with C = 4 the kernel's output chunk: (2, 4, 1) the smallest; (2, 10, 5) the factor-analysis notebook's;
(3, 18, C) a full chunk, (3, 6, C + 1) one past it, (4, 8, 2 C + 1) several chunks with a remainder; (4, 18, 5) the largest
instantiated 2d at L = 4.  N = 0 writes zeros through pass 2 alone (the sum over no points), B = 0 launches nothing.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import factor_closed_forms as FC
from helpers import likelihood_closed_forms as L


pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
K_F64 = 64.0
DTYPES = [torch.float64, torch.float32]
GUARD, SENTINEL = 64, -77.25
TILE = 64
CHUNK = 4                                        # FACTOR_CHUNK of csrc/mf_lik_factor.hip
LAYOUT = ((0, 1, 64, 130, 195), (195, 65, 130, 0, 0), (63, 65, 64, 195, 3))      # three series, N = 390 each
OUTS = ("ve_sum", "g_mean", "g_cov", "g_w")
FN = "mf_lik_sparse_factor_expectations"
NQ = 20
CASES = [(2, 4, 1), (2, 10, 5), (3, 18, CHUNK), (3, 6, CHUNK + 1), (4, 8, 2 * CHUNK + 1), (4, 18, 5)]
RUNS = [(L.GAUSSIAN,) + case for case in CASES] + [(name, 2, 10, 5) for name in (L.BERNOULLI, L.POISSON, L.STUDENTT)]


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
def reference(name, lat, two_d, outs, f32, layout=LAYOUT):
    """Inputs (rounded to the dtype under test) and the float64 helper on them, per series - computed once per case and shared,
    read-only."""
    rng = np.random.default_rng(1000 * lat + 10 * two_d + outs + 7 * L.IDS[name])
    dt = np.float32 if f32 else np.float64
    rnd = lambda a: np.asarray(a).astype(dt).astype(np.float64)          # noqa: E731
    bsz, segs, n = len(layout), len(layout[0]), int(np.sum(layout[0]))
    assert all(int(np.sum(ln)) == n for ln in layout)
    ref = dict(offsets=np.stack([np.concatenate([[0], np.cumsum(ln)]) for ln in layout]).astype(np.int64))
    ref["wg"] = rnd(rng.uniform(-0.7, 0.7, size=(bsz, n, lat, two_d)))
    c = rnd(rng.normal(size=(bsz, n, lat, lat)))
    cg = rnd(c @ c.transpose(0, 1, 3, 2) / lat + 0.05 * np.eye(lat))
    ref["cg"] = np.tril(cg) + np.tril(cg, -1).transpose(0, 1, 3, 2)        # (symmetric after the rounding too)
    ref["mix"] = rnd(rng.uniform(-1.0, 1.0, size=(bsz, n, outs, lat)) * (0.5 if name == L.POISSON else 1.0))
    a = rng.normal(size=(bsz, segs, two_d, two_d))
    cov = rnd(a @ a.transpose(0, 1, 3, 2) / two_d + 0.1 * np.eye(two_d))
    ref["pair_cov"] = np.tril(cov) + np.tril(cov, -1).transpose(0, 1, 3, 2)
    ref["pair_mean"] = rnd(rng.normal(size=(bsz, segs, two_d)))
    if name == L.BERNOULLI:
        y = rng.integers(0, 2, size=(bsz, n, outs))
    elif name == L.POISSON:
        y = rng.integers(0, 10, size=(bsz, n, outs))
    else:
        y = rng.normal(size=(bsz, n, outs))
    ref["y"] = rnd(y)
    seg = [np.repeat(np.arange(segs), ln) for ln in layout]
    for b in range(bsz):                          # the domain, by construction
        mu_g = np.einsum("kli,ki->kl", ref["wg"][b], ref["pair_mean"][b][seg[b]])
        sig = ref["cg"][b] + np.einsum("kli,kij,kqj->klq", ref["wg"][b], ref["pair_cov"][b][seg[b]], ref["wg"][b])
        mu, s2 = np.einsum("kpl,kl->kp", ref["mix"][b], mu_g), np.einsum("kpl,klq,kpq->kp", ref["mix"][b], sig, ref["mix"][b])
        assert np.all(s2 > 0) and (name != L.POISSON or np.all(mu + 0.5 * s2 < 6.0))
    ref["want"] = [helper(name, ref, b, np.float64) for b in range(bsz)]
    if f32:
        ref["want32"] = [helper(name, ref, b, np.float32) for b in range(bsz)]
    freeze(ref)
    return ref


def helper(name, ref, b, dtype):
    return FC.segment_expectations_factor(L.LIKELIHOODS[name], ref["wg"][b], ref["cg"][b], ref["mix"][b], ref["y"][b], ref["offsets"][b],
                                          ref["pair_mean"][b], ref["pair_cov"][b], NQ, dtype)


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


def launch(name, dtype, ref, series=None, want=(True, True, True, True), two_d=None, latent_dim=None, outputs=None):
    """One call on all the series of ``ref`` (or on ``series`` alone).  ``two_d`` / ``latent_dim`` / ``outputs``: what the call
    CLAIMS (the buffers keep their shapes).  Returns ``(rc, [ve_sum, g_mean, g_cov, g_w])`` as tensors (None where not asked for)
    after checking every guard region."""
    pick = (lambda a: a) if series is None else (lambda a: a[series:series + 1])
    bsz, n, lat, d2 = pick(ref["wg"]).shape
    outs_p = ref["mix"].shape[2]
    offsets = pick(ref["offsets"])
    segs = offsets.shape[1] - 1
    tiles, tile_seg, seg_tile = tile_table(offsets)
    tab = [torch.tensor(a, dtype=torch.int64, device=DEV).contiguous() for a in (offsets, tile_seg, seg_tile)]
    ins = [dev(pick(ref[k]), dtype) for k in ("wg", "cg", "mix", "y", "pair_mean", "pair_cov")]
    shapes = ((bsz, segs), (bsz, segs, d2), (bsz, segs, d2, d2), (bsz, n, outs_p, lat))
    outs = [guarded(s, dtype) if w else (None, None) for s, w in zip(shapes, want)]
    ws_bytes = int(_lib.load().mf_lik_sparse_factor_expectations_workspace_bytes(tiles, d2, ins[0].element_size()))
    assert ws_bytes == tiles * (d2 * (d2 + 1) // 2 + d2 + 1) * ins[0].element_size()
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    nodes, weights = c_rule(NQ)
    rc = _lib.call_rc(FN, dtype, bsz, n, segs, d2 if two_d is None else two_d, lat if latent_dim is None else latent_dim,
                      outs_p if outputs is None else outputs, L.IDS[name], c_params(name), NQ, nodes, weights, _lib.ptr(tab[0]),
                      *[_lib.ptr(t) for t in ins], tiles, _lib.ptr(tab[1]), _lib.ptr(tab[2]), _lib.ptr(ws), ws_bytes,
                      *[_lib.ptr(o[1]) for o in outs], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert all(b[0] is None or bool(torch.all(b[0][-GUARD:] == SENTINEL)) for b in outs), "a write past the end of an output"
    assert bool(torch.all(ws[ws_bytes:] == 0x5A)), "a write past the end of the workspace"
    return rc, [o[1] for o in outs]


def check(what, got, want, mag, dtype, got32=None):
    """float64: the K eps bound; float32: 4 x the normalised error of the numpy float32 evaluation.  Prints the figure, returns the
    failure as text or None."""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    if got.size == 0:
        return None
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
@pytest.mark.parametrize("name,lat,two_d,outputs", RUNS, ids=[f"{r[0]}-L{r[1]}-2d{r[2]}-P{r[3]}" for r in RUNS])
def test_batch_of_three_against_the_helper_and_each_series_alone_bit_for_bit(name, lat, two_d, outputs, dtype):
    ref = reference(name, lat, two_d, outputs, dtype == torch.float32)
    rc, outs = launch(name, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} L={lat} 2d={two_d} P={outputs}", ref, dtype, outs)
    g_cov = outs[2]
    assert torch.equal(g_cov, g_cov.transpose(-1, -2)), "g_cov is symmetric: both triangles are written from one sum"
    for b, ln in enumerate(LAYOUT):
        for s, count in enumerate(ln):
            if count == 0:
                assert all(float(o[b, s].abs().max()) == 0.0 for o in outs[:3]), "an empty segment: exact zeros"
    rc, again = launch(name, dtype, ref)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(again, outs)), "two launches on the same inputs return the same bits"
    for b in range(3):
        rc, one = launch(name, dtype, ref, series=b)
        assert rc == 0
        assert all(torch.equal(o[0], f[b]) for o, f in zip(one, outs)), "a series alone gives the bits it gives in a batch"
    rc, value = launch(name, dtype, ref, want=(True, False, False, False))
    assert rc == 0 and value[1] is None and value[2] is None and value[3] is None
    assert torch.equal(value[0], outs[0]), "value-only mode has the bits of the value beside the gradients"
    rc, pair = launch(name, dtype, ref, want=(True, True, True, False))
    assert rc == 0 and pair[3] is None and all(torch.equal(a, b) for a, b in zip(pair[:3], outs[:3])), "g_w NULL: the pair adjoints keep their bits"
    rc, only_w = launch(name, dtype, ref, want=(False, False, False, True))
    assert rc == 0 and only_w[0] is None and torch.equal(only_w[3], outs[3]), "g_w on its own has the same bits"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_an_output_outside_the_domain_poisons_its_own_segment_and_its_own_row_of_g_w(dtype):
    name, f32 = L.GAUSSIAN, dtype == torch.float32
    ref = dict(reference(name, 2, 10, 5, f32))
    rc, clean = launch(name, dtype, ref)
    assert rc == 0
    off = ref["offsets"]
    # W_p = 0 gives s2_p = 0 exactly: output 3 of a point in the second tile of segment 3 of series 0, and - NaN - output 0 of the
    # first point of series 2
    mix = ref["mix"].copy()
    k0, k2 = int(off[0, 3]) + 70, int(off[2, 0])
    mix[0, k0, 3, :] = 0.0
    mix[2, k2, 0, 1] = float("nan")
    ref["mix"] = mix
    rc, outs = launch(name, dtype, ref)
    assert rc == 0
    poisoned = {(0, 3), (2, 0)}
    for b in range(3):
        for s in range(5):
            for o, f in zip(outs[:3], clean[:3]):
                if (b, s) in poisoned:
                    assert bool(torch.isnan(o[b, s]).all()), "every output of its segment is NaN"
                else:
                    assert torch.equal(o[b, s], f[b, s]), "every other segment keeps its bits"
    g_w, g_w_clean = outs[3], clean[3]
    assert bool(torch.isnan(g_w[0, k0, 3]).all()) and bool(torch.isnan(g_w[2, k2, 0]).all()), "the output's own row of g_w is NaN"
    keep = torch.ones(g_w.shape[:3], dtype=torch.bool, device=DEV)
    keep[0, k0, 3] = keep[2, k2, 0] = False
    assert torch.equal(g_w[keep], g_w_clean[keep]), "every other row of g_w keeps its bits"


def test_argument_checks_and_signatures_that_are_not_instantiated():
    dtype, name = torch.float64, L.GAUSSIAN
    ref = reference(name, 2, 10, 5, False)
    for claim in (dict(latent_dim=5), dict(latent_dim=1), dict(two_d=9), dict(two_d=11), dict(two_d=2), dict(two_d=20),
                  dict(latent_dim=4, two_d=6), dict(latent_dim=3, two_d=4), dict(outputs=1025)):
        rc, outs = launch(name, dtype, ref, **claim)
        assert rc == -101, claim
        assert all(bool(torch.all(o == SENTINEL)) for o in outs), "nothing is written"
    rc, outs = launch(name, dtype, ref, outputs=0)
    assert rc == -6 and all(bool(torch.all(o == SENTINEL)) for o in outs)
    nodes, weights = c_rule(NQ)
    par = c_params(name)
    call = lambda *a: _lib.call_rc(FN, dtype, *a, _lib.stream_ptr(DEV))          # noqa: E731
    head = (2, 130, 5, 10, 2, 5, 0, par, NQ, nodes, weights)
    offsets = np.array([[0, 1, 64, 100, 130, 130], [0, 0, 65, 65, 129, 130]], dtype=np.int64)
    tiles, tile_seg, seg_tile = tile_table(offsets)
    tab = [torch.tensor(a, dtype=torch.int64, device=DEV) for a in (offsets, tile_seg, seg_tile)]
    ins = [torch.zeros(shape, dtype=dtype, device=DEV) for shape in ((2, 130, 2, 10), (2, 130, 2, 2), (2, 130, 5, 2), (2, 130, 5), (2, 5, 10),
                                                                      (2, 5, 10, 10))]
    ws_bytes = int(_lib.load().mf_lik_sparse_factor_expectations_workspace_bytes(tiles, 10, 8))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    out = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((2, 5), (2, 5, 10), (2, 5, 10, 10), (2, 130, 5, 2))]
    full = [_lib.ptr(tab[0]), *[_lib.ptr(t) for t in ins], tiles, _lib.ptr(tab[1]), _lib.ptr(tab[2]), _lib.ptr(ws), ws_bytes,
            *[_lib.ptr(o) for o in out]]
    for pos in (12, 13, 14, 15, 16, 17, 18, 20, 21, 22):                  # a NULL input, table or workspace
        args = list(full)
        args[pos - 12] = None
        assert call(*head, *args) == -pos, pos
    args = list(full)
    args[23 - 12] = ws_bytes - 1
    assert call(*head, *args) == -23, "a workspace that is too small"
    args = list(full)
    args[19 - 12] = -1
    assert call(*head, *args) == -19
    args = list(full)
    args[25 - 12] = None
    assert call(*head, *args) == -25, "g_cov without g_mean"
    args = list(full)
    args[26 - 12] = None
    assert call(*head, *args) == -26, "g_mean without g_cov"
    for pos, value, want in ((0, -1, -1), (1, -1, -2), (2, 0, -3), (6, 7, -7), (7, None, -8), (8, 0, -9), (8, 33, -9), (9, None, -10),
                             (10, None, -11)):
        args = list(head)
        args[pos] = value
        assert call(*args, *full) == want, (pos, value)
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in out), "nothing is launched on an error"
    assert call(*head, *full[:12], None, None, None, None) == 0, "every output NULL: nothing to do"
    # B = 0 launches nothing; N = 0 writes the sums over no points
    assert call(0, 130, 5, 10, 2, 5, 0, par, NQ, nodes, weights, *full) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in out), "B = 0: nothing is written"
    empty = [*([None] * 7), 0, None, None, None, 0, *[_lib.ptr(o) for o in out[:3]], None]
    assert call(2, 0, 5, 10, 2, 5, 0, par, NQ, nodes, weights, *empty) == 0
    torch.cuda.synchronize()
    assert all(float(o.abs().max()) == 0.0 for o in out[:3]), "N = 0: every sum is zero"
    with pytest.raises(NotImplementedError, match="not instantiated"):
        _lib.call(FN, dtype, 1, 0, 1, 10, 5, 5, 0, par, NQ, nodes, weights, *([None] * 7), 0, None, None, None, 0, None, None, None, None,
                  _lib.stream_ptr(DEV))
