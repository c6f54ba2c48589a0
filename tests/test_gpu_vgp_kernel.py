"""
GPU tests of ``mf_lik_dense_expectations_*`` and ``mf_lik_dense_expectations_adjoint_*`` (csrc/mf_lik.hip) through the raw C ABI,
against the numpy statement of their formulas in tests/helpers/vgp_closed_forms.py.

Tolerances, in the scheme of tests/test_gpu_svgp_kernel.py.
  float64: ``|err| <= K eps (magnitude + 1)``, eps = 2^-52, K = 64, with the helper's magnitudes: the expectations' own for g_mu and
    g_var, their sum over the series for ve_sum.  check() prints every ratio ("RATIO f64 ...").
  float32: the kernel's error, normalised by (magnitude + 1) and maximised over an output of one series, against 4 x the same figure
    of the helper evaluated in numpy float32 on the same (float32-rounded) inputs; the helper projects and sums in the kernel's order
    (include/markovflow_amd.h), and both errors are taken against the float64 helper.
  adjoint: every element is a product of three factors, (weight (g_var h_i)) h_j or (weight g_mu) h_i with one factor fewer: three
    roundings at the most, each of relative size eps / 2, so ``|err| <= 3 eps |product|`` holds with room (eps = 2^-52 or 2^-23; the
    reference product is formed in float64 from the inputs as rounded to the dtype under test).
Measured maxima on an MI355X over all the cases of this file.  float64: ve_sum 2.85, g_mu 50.1 (Bernoulli, d = 12, N = 65: the
  probit's 1 + erf cancels in the tail, and the helper's magnitude counts the terms of the quadrature, not that cancellation), g_var
  23.9.  Adjoint: float64 the helper's very bits (plain products), float32 at most 0.94 (g_means) and 1.37 (g_covs) eps |product|.
  float32, the three-series launches, per series: g_mu at most 3.52 x, g_var 2.51 x, the largest normalised error 1.5e-5 (Bernoulli).
  Two exceptions, both of the kind tests/test_gpu_svgp_kernel.py documents for its ve_sum, and for its cause: the figure is a maximum
  over few samples, the kernel's expf / erff / lgammaf are good to an ulp or two where numpy's float32 functions are computed in double
  and rounded once, and now and then the helper lands within a small fraction of an ulp of the float64 value.
  * ve_sum is ONE number per series, so its maximum is taken over the series of a launch together (the per-series figures are still
    printed).  Per series, 5 of the 34 three-series launches and 18 of the 24 launches of 32 series hold a series above 4 x - up to
    41 x (Bernoulli, nq = 32: 3.6e-7 against the helper's 2.5e-7 over the launch, 1.46 x) and 361 x (Gaussian, d = 5, N = 1, where the
    launch's figures are the same bits) - while over the launch the worst is 3.60 x (Poisson, nq = 1: 7.8e-8 against 2.2e-8) among the
    three-series launches and 2.46 x among those of 32 series.  (The kernel adds a tile's points and a series' tiles in a double
    accumulator; with a float accumulator two launches at d = 5, Poisson and Student-t, measured 4.59 x and 4.09 x over the launch.)
  * the launches of 32 series at N = 1, 64, 65 judge g_mu and g_var over the launch as well.  At N = 1 a series IS one sample: per
    series up to 64 x (g_mu) and 49 x (g_var) in 10 and 6 of the 24 launches.  At N = 64 and 65 the per-series figure is the largest
    of 512 maxima (32 series x 16 launches) over 64 or 65 points: at most 3.21 x in this run except Bernoulli, d = 5, N = 65 at 4.82 x (with h drawn from
    [-0.7, 0.7] instead, two Bernoulli launches at N = 64 measured 4.05 x and 4.23 x).  Over the launch: g_mu at most 2.06 x, g_var 2.65 x.

The main shape is three series of N = 195 points: three full tiles of 64 and a remainder of 3, both sides of a tile boundary; single
launches at N = 1, 64 and 65 cover one lane, exactly one tile and one point beyond it.  ``covs`` is a random SPD matrix and ``h`` a
random row, not [1, 0, ...]; one case adds a strictly upper-triangular part to ``covs``, which pins the full-matrix definition of fvar.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import likelihood_closed_forms as L
from helpers import vgp_closed_forms as VG

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
EPS32 = 2.0 ** -23
K_F64 = 64.0
NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
DTYPES = [torch.float64, torch.float32]
DIMS = [1, 2, 5, 6, 9, 12]
GUARD, SENTINEL = 64, -77.25
TILE = 64
OUTS = ("ve_sum", "g_mu", "g_var")
FN, ADJ = "mf_lik_dense_expectations", "mf_lik_dense_expectations_adjoint"
VE = ("ve_sum",)           # float32: judged over the launch, see the module docstring


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
def reference(name, nq, d, f32, n=195, bsz=3, upper=0.0):
    """Inputs (rounded to the dtype under test) and the float64 helper on them, per series - computed once per case and shared,
    read-only.  covs is a random SPD matrix (plus ``upper`` times a random strictly upper-triangular one): fvar > 0, asserted."""
    rng = np.random.default_rng(d * 100 + nq + n)
    dt = np.float32 if f32 else np.float64
    rnd = lambda a: np.asarray(a).astype(dt).astype(np.float64)          # noqa: E731
    # |h_i| in [0.2, 0.7] with a random sign: with d = 1, fvar = h^2 P, and an h next to 0 would leave the domain's interior
    ref = dict(h=rnd(rng.uniform(0.2, 0.7, size=(bsz, n, d)) * rng.choice([-1.0, 1.0], size=(bsz, n, d))))
    a = rng.normal(size=(bsz, n, d, d))
    covs = a @ a.transpose(0, 1, 3, 2) / d + 0.1 * np.eye(d)
    if upper:
        covs = covs + upper * np.triu(rng.uniform(-1.0, 1.0, size=(bsz, n, d, d)), k=1)
    ref["covs"] = rnd(covs)
    ref["means"] = rnd(rng.normal(size=(bsz, n, d)))
    ref["y"] = rnd(np.resize(np.asarray(L.OBSERVED[name]), (bsz, n)))
    per = lambda b, dtype: VG.dense_expectations(L.LIKELIHOODS[name], ref["h"][b], ref["means"][b], ref["covs"][b], ref["y"][b], nq,   # noqa: E731
                                                 dtype)
    ref["want"] = [per(b, np.float64) for b in range(bsz)]
    assert all(w["fvar"].min() > 1e-4 for w in ref["want"] if n), "the case keeps every point inside the domain"
    if f32:
        ref["want32"] = [per(b, np.float32) for b in range(bsz)]
    for v in ref.values():
        for a in (v if isinstance(v, list) else [v]):
            for x in (a.values() if isinstance(a, dict) else [a]):
                if isinstance(x, np.ndarray):
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
    """One call on all the series of ``ref`` (or on ``series`` alone).  Returns ``(rc, [ve_sum, g_mu, g_var])`` as tensors (None where
    not asked for) after checking every guard region."""
    pick = (lambda a: a) if series is None else (lambda a: a[series:series + 1])
    bsz, n, d = pick(ref["h"]).shape
    ins = [dev(pick(ref[k]), dtype) for k in ("h", "means", "covs", "y")]
    shapes = ((bsz,), (bsz, n), (bsz, n))
    outs = [guarded(s, dtype) if w else (None, None) for s, w in zip(shapes, want)]
    ws_bytes = int(_lib.load().mf_lik_dense_expectations_workspace_bytes(bsz, n, ins[0].element_size()))
    assert ws_bytes == bsz * ((n + TILE - 1) // TILE) * ins[0].element_size()
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    nodes, weights = c_rule(nq)
    rc = _lib.call_rc(FN, dtype, bsz, n, d, L.IDS[name], c_params(name), nq, nodes, weights, *[_lib.ptr(t) for t in ins], _lib.ptr(ws),
                      ws_bytes, *[_lib.ptr(o[1]) for o in outs], _lib.stream_ptr(DEV))
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


def check_against_helper(tag, ref, dtype, outs, over_launch=()):
    """Every series and every output on its own; every figure is printed before the first failure is raised.  In float32 the outputs
    named in ``over_launch`` are judged by their maximum over the launch's series together (their per-series figures are still
    printed): see the module docstring."""
    f32 = dtype == torch.float32
    rows = list(range(len(ref["want"])))
    failures = []
    for b in rows:
        want = ref["want"][b]
        own = ref["want32"][b] if f32 else {}
        for key, got in zip(OUTS, outs):
            if got is not None:
                assert not bool(torch.any(got[b] == SENTINEL)), f"{tag} series {b} {key}: an element was not written"
                failed = check(f"{tag} series {b} {key}", got[b].cpu().numpy(), want[key], want["mag_" + key], dtype, own.get(key))
                if not (f32 and key in over_launch):
                    failures.append(failed)
    gather = lambda src, k: np.stack([np.asarray(src[b][k]) for b in rows])          # noqa: E731
    for key, got in zip(OUTS, outs):
        if f32 and got is not None and key in over_launch:
            failures.append(check(f"{tag} launch {key}", got.cpu().numpy(), gather(ref["want"], key), gather(ref["want"], "mag_" + key),
                                  dtype, gather(ref["want32"], key)))
    failures = [f for f in failures if f]
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", NAMES)
def test_batch_of_three_against_the_helper_and_each_series_alone_bit_for_bit(name, d, dtype):
    ref = reference(name, 20, d, dtype == torch.float32)
    rc, outs = launch(name, 20, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} d={d}", ref, dtype, outs, over_launch=VE)
    rc, again = launch(name, 20, dtype, ref)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(again, outs)), "two launches on the same inputs return the same bits"
    for b in range(3):
        rc, one = launch(name, 20, dtype, ref, series=b)
        assert rc == 0
        assert all(torch.equal(o[0], f[b]) for o, f in zip(one, outs)), "a series alone gives the bits it gives in a batch"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("d", [5, 12])
@pytest.mark.parametrize("name", NAMES)
def test_one_point_one_full_tile_and_one_point_beyond_it(name, d, n, dtype):
    ref = reference(name, 20, d, dtype == torch.float32, n=n, bsz=32)
    rc, outs = launch(name, 20, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} d={d} N={n}", ref, dtype, outs, over_launch=OUTS)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nq", [1, 32])
@pytest.mark.parametrize("name", NAMES)
def test_quadrature_rules_of_one_and_of_thirty_two_nodes(name, nq, dtype):
    ref = reference(name, nq, 6, dtype == torch.float32)
    rc, outs = launch(name, nq, dtype, ref)
    assert rc == 0
    check_against_helper(f"{name} nq={nq}", ref, dtype, outs, over_launch=VE)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("d", [5, 12])
def test_a_covariance_that_is_not_symmetric_is_read_in_full(d, dtype):
    ref = reference(L.STUDENTT, 20, d, dtype == torch.float32, upper=0.02)
    covs = ref["covs"]
    assert float(np.abs(covs - covs.transpose(0, 1, 3, 2)).max()) > 1e-3
    # the case can tell the definitions apart: the lower triangle mirrored moves fvar by far more than the bound
    mirrored = np.tril(covs) + np.tril(covs, -1).transpose(0, 1, 3, 2)
    moved = np.einsum("bki,bkij,bkj->bk", ref["h"], covs - mirrored, ref["h"])
    assert float(np.abs(moved).max()) > 1e-3
    rc, outs = launch(L.STUDENTT, 20, dtype, ref)
    assert rc == 0
    check_against_helper(f"upper-triangular part d={d}", ref, dtype, outs, over_launch=VE)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("d", [6, 12])
def test_value_only_mode_and_gradients_without_the_value_return_the_same_bits(d, dtype):
    ref = reference(L.BERNOULLI, 20, d, dtype == torch.float32)
    rc, full = launch(L.BERNOULLI, 20, dtype, ref)
    assert rc == 0
    rc, value = launch(L.BERNOULLI, 20, dtype, ref, want=(True, False, False))
    assert rc == 0 and value[1] is None and value[2] is None and torch.equal(value[0], full[0])
    rc, grads = launch(L.BERNOULLI, 20, dtype, ref, want=(False, True, True))
    assert rc == 0 and grads[0] is None and torch.equal(grads[1], full[1]) and torch.equal(grads[2], full[2])


def test_no_points_writes_zeros_and_no_series_launches_nothing():
    dtype = torch.float64
    nodes, weights = c_rule(20)
    s = _lib.stream_ptr(DEV)
    # N = 0 needs no input and no workspace
    out = torch.full((2,), SENTINEL, dtype=dtype, device=DEV)
    assert _lib.call_rc(FN, dtype, 2, 0, 4, 1, None, 20, nodes, weights, None, None, None, None, None, 0, _lib.ptr(out), None, None, s) == 0
    assert float(out.abs().max()) == 0.0, "N = 0: the sums are zero"
    assert _lib.call_rc(FN, dtype, 0, 5, 4, 1, None, 20, nodes, weights, None, None, None, None, None, 0, None, None, None, s) == 0
    assert int(_lib.load().mf_lik_dense_expectations_workspace_bytes(0, 5, 8)) == 0
    assert int(_lib.load().mf_lik_dense_expectations_workspace_bytes(2, 0, 8)) == 0
    assert _lib.call_rc(ADJ, dtype, 0, 5, 4, None, None, None, None, None, None, s) == 0
    assert _lib.call_rc(ADJ, dtype, 2, 0, 4, None, None, None, None, None, None, s) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_a_bad_covariance_poisons_its_own_point_and_series_and_leaves_the_rest_bit_identical(name, dtype):
    ref = dict(reference(name, 20, 6, dtype == torch.float32))
    rc, clean = launch(name, 20, dtype, ref)
    assert rc == 0
    covs = ref["covs"].copy()
    b_bad, k_bad = 1, 70                      # the second tile of the second series
    covs[b_bad, k_bad] = -np.eye(6)
    ref["covs"] = covs
    rc, outs = launch(name, 20, dtype, ref)
    assert rc == 0
    ve_sum, g_mu, g_var = outs
    assert bool(torch.isnan(ve_sum[b_bad])) and bool(torch.isnan(g_mu[b_bad, k_bad])) and bool(torch.isnan(g_var[b_bad, k_bad]))
    keep = torch.ones((3, 195), dtype=torch.bool, device=DEV)
    keep[b_bad, k_bad] = False
    assert torch.equal(g_mu[keep], clean[1][keep]) and torch.equal(g_var[keep], clean[2][keep]), "every other point keeps its bits"
    assert torch.equal(ve_sum[[0, 2]], clean[0][[0, 2]]), "every other series keeps its bits"


def test_bad_arguments_return_their_codes_and_launch_nothing():
    dtype = torch.float64
    ref = reference(L.STUDENTT, 20, 4, False)
    ins = [dev(ref[k], dtype) for k in ("h", "means", "covs", "y")]
    io = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((3,), (3, 195), (3, 195))]
    ws_bytes = 3 * 4 * 8
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    nodes, weights = c_rule(20)
    par, s = c_params(L.STUDENTT), _lib.stream_ptr(DEV)
    p, o = [_lib.ptr(t) for t in ins], [_lib.ptr(t) for t in io]

    def call(bsz=3, n=195, d=4, lik=3, params=par, nq=20, nd=nodes, wt=weights, ptrs=p, wsp=_lib.ptr(ws), nbytes=ws_bytes, outs=o):
        return _lib.call_rc(FN, dtype, bsz, n, d, lik, params, nq, nd, wt, *ptrs, wsp, nbytes, *outs, s)

    assert call(bsz=-1) == -1 and call(n=-1) == -2
    for d in (0, 13, -1, 64):
        assert call(d=d) == -100
    assert call(lik=7) == -4 and call(params=None) == -5 and call(nq=0) == -6 and call(nq=33) == -6
    assert call(nd=None) == -7 and call(wt=None) == -8
    for i in range(4):
        assert call(ptrs=p[:i] + [None] + p[i + 1:]) == -(9 + i)
    assert call(wsp=None) == -13
    assert call(nbytes=ws_bytes - 1) == -14 and call(nbytes=0) == -14
    assert call(outs=[o[0], None, o[2]]) == -16 and call(outs=[o[0], o[1], None]) == -17
    assert call(outs=[None] * 3) == 0                                   # nothing asked for
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in io)
    assert call(wsp=None, nbytes=0, outs=[None, o[1], o[2]]) == 0       # the gradients alone need no workspace
    with pytest.raises(NotImplementedError):
        _lib.call(FN, dtype, 3, 195, 13, 3, par, 20, nodes, weights, *p, _lib.ptr(ws), ws_bytes, *o, s)
    with pytest.raises(ValueError, match="invalid argument #6"):
        _lib.call(FN, dtype, 3, 195, 4, 3, par, 40, nodes, weights, *p, _lib.ptr(ws), ws_bytes, *o, s)
    # the adjoint entry
    g = [torch.full(shape, SENTINEL, dtype=dtype, device=DEV) for shape in ((3, 195, 4), (3, 195, 4, 4))]
    a = [p[0], o[1], o[2], None, _lib.ptr(g[0]), _lib.ptr(g[1])]
    adj = lambda bsz=3, n=195, d=4, args=a: _lib.call_rc(ADJ, dtype, bsz, n, d, *args, s)      # noqa: E731
    assert adj(bsz=-1) == -1 and adj(n=-1) == -2 and adj(d=0) == -100 and adj(d=13) == -100
    assert adj(args=[None] + a[1:]) == -4 and adj(args=[a[0], None] + a[2:]) == -5 and adj(args=a[:2] + [None] + a[3:]) == -6
    assert adj(args=a[:4] + [None, None]) == 0                          # nothing asked for
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in g)


# ---- the adjoint entry -------------------------------------------------------------------------------------------------------------
def launch_adjoint(dtype, h, g_mu, g_var, weight, want=(True, True)):
    bsz, n, d = h.shape
    ins = [dev(a, dtype) for a in (h, g_mu, g_var)]
    wt = None if weight is None else dev(weight, dtype)
    outs = [guarded(s, dtype) if w else (None, None) for s, w in zip(((bsz, n, d), (bsz, n, d, d)), want)]
    rc = _lib.call_rc(ADJ, dtype, bsz, n, d, *[_lib.ptr(t) for t in ins], _lib.ptr(wt), *[_lib.ptr(o[1]) for o in outs],
                      _lib.stream_ptr(DEV))
    assert all(b[0] is None or bool(torch.all(b[0][-GUARD:] == SENTINEL)) for b in outs), "a write past the end of an output"
    assert all(b[1] is None or not bool(torch.any(b[1] == SENTINEL)) for b in outs), "an element was not written"
    return rc, [o[1] for o in outs]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("d", DIMS)
def test_adjoint_expansion_against_the_helpers_products(d, dtype):
    f32 = dtype == torch.float32
    rng = np.random.default_rng(40 + d)
    rnd = lambda a: np.asarray(a).astype(np.float32 if f32 else np.float64).astype(np.float64)          # noqa: E731
    bsz, n = 3, 195
    h, g_mu, g_var = rnd(rng.uniform(-0.7, 0.7, size=(bsz, n, d))), rnd(rng.normal(size=(bsz, n))), rnd(rng.normal(size=(bsz, n)))
    weight = rnd(rng.uniform(0.5, 2.0, size=bsz) * np.array([1.0, -1.0, 1.0]))
    rc, outs = launch_adjoint(dtype, h, g_mu, g_var, weight)
    assert rc == 0
    eps = EPS32 if f32 else EPS
    for b in range(bsz):
        want = VG.dense_adjoint(h[b], g_mu[b], g_var[b], weight[b])
        for key, got in zip(("g_means", "g_covs"), outs):
            err = np.abs(got[b].cpu().numpy().astype(np.float64) - want[key])
            mag = want["mag_" + key]
            ratio = float((err[mag > 0] / (eps * mag[mag > 0])).max())
            print(f"RATIO adjoint {'f32' if f32 else 'f64'} d={d} series {b} {key}: {ratio:.2f} eps |product|")
            assert np.all(err <= 3.0 * eps * mag), f"{key}: {ratio:.2f} eps |product|"
    # weight = NULL is a vector of ones, bit for bit; either output alone has the bits it has beside the other
    rc, plain = launch_adjoint(dtype, h, g_mu, g_var, None)
    rc1, ones = launch_adjoint(dtype, h, g_mu, g_var, np.ones(bsz))
    assert rc == 0 and rc1 == 0 and all(torch.equal(a, b) for a, b in zip(plain, ones))
    rc, only_means = launch_adjoint(dtype, h, g_mu, g_var, weight, want=(True, False))
    rc1, only_covs = launch_adjoint(dtype, h, g_mu, g_var, weight, want=(False, True))
    assert rc == 0 and rc1 == 0 and torch.equal(only_means[0], outs[0]) and torch.equal(only_covs[1], outs[1])
