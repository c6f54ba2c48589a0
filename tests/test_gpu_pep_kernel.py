"""
GPU tests of the power-EP kernels (csrc/mf_lik.hip: ``mf_lik_log_expected_density_*``, ``mf_lik_pep_site_update_*``) through the raw
C ABI and through markovflow_amd/likelihoods.py, against the numpy / scipy reference of tests/helpers/pep_closed_forms.py.  Layout
and tolerance scheme are those of tests/test_gpu_likelihoods.py.

Tolerances.
  float64: ``|err| <= K eps (magnitude + 1)``, eps = 2^-52, with the helper's magnitudes (its module docstring): the softmax-weighted
    sums of the absolute terms for I, g1, g2, and a running error bound through the scalar algebra for the cavity and the site update.
    The site update is compared at the KERNEL'S OWN cavity (its ``cav_mu`` / ``cav_var`` outputs, which are checked first): the
    helper then evaluates steps 2-5 at exactly the numbers the kernel used.
  float32: the kernel's error, normalised by (magnitude + 1) and maximised over the grid, against 4 x the same figure of the helper
    evaluated in numpy float32 on the same (float32-rounded) inputs; both errors are taken against the float64 helper.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import likelihoods as ML
from helpers import likelihood_closed_forms as L
from helpers import pep_closed_forms as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
# tests/test_gpu_likelihoods.py's K.  check() prints every ratio ("RATIO f64 ..."); a ratio above 64 wants an explanation, not a
# larger K.  Measured on an MI355X, the largest over all cases: I 25.88 (Poisson, nq = 32), g1 8.64, g2 2.66, cav_mu 0.22,
# cav_var 0.00, nat1 0.76, nat2 1.83, log_norm 2.15; I against mf_lik_predict_log_density 0.81; kernel against torch 0.69.
# float32, kernel error over the numpy float32 helper's (bound 4): I 2.73, g1 2.60, g2 2.03, cavity 1.00, nat1 3.31, nat2 3.00,
# log_norm 2.78; kernel against torch (bound 8) 5.32.
K_F64 = 64.0
NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
NQS = [1, 20, 32]
SIZES = [1, 255, 256, 257, 1000]
ALPHAS = [1.0, 0.5]
RATES = [1.0, 0.3]
DTYPES = [torch.float64, torch.float32]
GUARD, SENTINEL = 64, -77.25
LED, PEP = "mf_lik_log_expected_density", "mf_lik_pep_site_update"


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


def build_likelihood(name, nq=20):
    params = L.LIKELIHOODS[name][1]
    return {L.GAUSSIAN: lambda: mfa.Gaussian(params[0], nq), L.BERNOULLI: lambda: mfa.Bernoulli(nq), L.POISSON: lambda: mfa.Poisson(nq),
            L.STUDENTT: lambda: mfa.StudentT(*params, nq)}[name]()


@functools.lru_cache(maxsize=None)
def c_rule(nq):
    x, w = np.polynomial.hermite.hermgauss(nq)
    return host_array(tuple(x)), host_array(tuple(w))


def frozen(ref):
    for v in ref.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, nq, alpha, f32, n=256):
    """The grid as cavities (rounded to the dtype under test, n points of the grid repeated) and the float64 helper on them -
    computed once per case and shared, read-only."""
    spec = L.LIKELIHOODS[name]
    dt = np.float32 if f32 else np.float64
    mu, var, y = (np.resize(a, n).astype(dt).astype(np.float64) for a in L.value_grid(name))
    vals, mags = P.log_expected_density(spec, mu, var, y, alpha, nq)
    ref = dict(mu=mu, var=var, y=y, vals=vals, mags=mags)
    if alpha == 1.0:
        ref["pld_mag"] = L.predict_log_density_magnitude(spec, mu, var, y, nq)
    if f32:
        ref["vals32"] = P.log_expected_density(spec, mu, var, y, alpha, nq, dtype=np.float32)[0]
    return frozen(ref)


@functools.lru_cache(maxsize=None)
def site_reference(name, nq, alpha, f32, n=256):
    """The grid as posterior marginals, with sites whose cavity exists and whose den is at least 0.1 (found with the float64
    helper on the rounded inputs: 1 / v_c = (1 + c) / s, and a tighter cavity brings den towards 1)."""
    spec = L.LIKELIHOODS[name]
    dt = np.float32 if f32 else np.float64
    rnd = lambda a: np.asarray(a).astype(dt).astype(np.float64)                                 # noqa: E731
    m, s, y = (rnd(np.resize(a, n)) for a in L.value_grid(name))
    rng = np.random.default_rng(7)
    nat1, log_norm = rnd(0.3 * rng.normal(size=n) / np.sqrt(s)), rnd(rng.normal(size=n))
    nat2 = np.full(n, np.nan)
    for c in (-0.3, 0.5, 3.0, 30.0, 300.0, 3000.0):
        trial = np.where(np.isnan(nat2), rnd(c / (2 * alpha * s)), nat2)
        r = P.pep_site_update(spec, m, s, y, alpha, 1.0, nat1, trial, log_norm, nq)
        nat2 = np.where(np.isnan(nat2) & (r["den"] >= 0.1) & ~r["skipped"], trial, nat2)
    assert not np.isnan(nat2).any(), "no site with den >= 0.1 found for some grid point"
    return frozen(dict(m=m, s=s, y=y, nat1=nat1, nat2=nat2, log_norm=log_norm))


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def guarded(n, dtype, fill=None):
    """An output of n elements followed by a sentinel-filled guard region."""
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    if fill is not None:
        buf[:n] = dev(fill, dtype)
    return buf, buf[:n]


def guard_intact(buf, n):
    return bool(torch.all(buf[n:] == SENTINEL))


def bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def check(what, got, want, mag, dtype, got32=None):
    """float64: the K eps bound; float32: 4 x the normalised error of the numpy float32 evaluation.  Prints the figure first."""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    scaled = np.abs(got - want) / (np.asarray(mag) + 1.0)
    if dtype == torch.float64:
        ratio = float(scaled.max() / EPS)
        print(f"RATIO f64 {what}: {ratio:.2f}")
        assert ratio <= K_F64, f"{what}: {ratio:.1f} eps (magnitude + 1) at point {int(scaled.argmax())}"
    else:
        own = float((np.abs(np.asarray(got32, dtype=np.float64) - want) / (np.asarray(mag) + 1.0)).max())
        print(f"ERR f32 {what}: kernel {scaled.max():.3e}  numpy float32 {own:.3e}")
        assert scaled.max() <= 4.0 * own, f"{what}: kernel {scaled.max():.3e} against numpy float32 {own:.3e}"


def raw_led(name, nq, dtype, alpha, mu, var, y, want=(True, True, True)):
    n = mu.numel()
    bufs = [guarded(n, dtype) if w else (None, None) for w in want]
    nodes, weights = c_rule(nq)
    rc = _lib.call_rc(LED, dtype, n, L.IDS[name], c_params(name), nq, nodes, weights, alpha, _lib.ptr(mu), _lib.ptr(var), _lib.ptr(y),
                      *[_lib.ptr(b[1]) for b in bufs], _lib.stream_ptr(DEV))
    assert rc == 0
    assert all(b[0] is None or guard_intact(b[0], n) for b in bufs)
    return [b[1] for b in bufs]


def raw_pep(name, nq, dtype, alpha, lr, m, s, y, sites, update=None, want=(True, True)):
    """In place on guarded copies of ``sites`` = (nat1, nat2, log_norm) as numpy arrays; returns (nat1, nat2, log_norm, cav_mu,
    cav_var) as device tensors (None where not wanted)."""
    n = m.numel()
    bufs = [guarded(n, dtype, a) for a in sites] + [guarded(n, dtype) if w else (None, None) for w in want]
    nodes, weights = c_rule(nq)
    rc = _lib.call_rc(PEP, dtype, n, L.IDS[name], c_params(name), nq, nodes, weights, alpha, lr, _lib.ptr(m), _lib.ptr(s), _lib.ptr(y),
                      _lib.ptr(update), *[_lib.ptr(b[1]) for b in bufs], _lib.stream_ptr(DEV))
    assert rc == 0
    assert all(b[0] is None or guard_intact(b[0], n) for b in bufs)
    return [b[1] for b in bufs]


def check_site_update(tag, name, nq, dtype, alpha, lr, n=256):
    """The kernel's cavity against the helper's; then the three site numbers against the helper at the kernel's cavity."""
    f32 = dtype == torch.float32
    spec, ref = L.LIKELIHOODS[name], site_reference(name, nq, alpha, f32, n)
    args = [ref[k] for k in ("m", "s", "y")]
    sites = [ref[k] for k in ("nat1", "nat2", "log_norm")]
    got = [t.cpu().numpy() for t in raw_pep(name, nq, dtype, alpha, lr, *(dev(a, dtype) for a in args), sites)]
    own = P.pep_site_update(spec, *args, alpha, lr, *sites, nq)
    own32 = P.cavity(ref["m"], ref["s"], ref["nat1"], ref["nat2"], alpha, np.float32) if f32 else (None, None)
    check(f"{tag} cav_mu", got[3], own["cav_mu"], own["cav_mags"][0], dtype, own32[0])
    check(f"{tag} cav_var", got[4], own["cav_var"], own["cav_mags"][1], dtype, own32[1])
    at = (got[3].astype(np.float64), got[4].astype(np.float64))
    want = P.pep_site_update(spec, *args, alpha, lr, *sites, nq, at_cavity=at)
    assert not want["skipped"].any()
    want32 = P.pep_site_update(spec, *args, alpha, lr, *sites, nq, at_cavity=at, dtype=np.float32) if f32 else {}
    for i, key in enumerate(("nat1", "nat2", "log_norm")):
        check(f"{tag} lr={lr} {key}", got[i], want[key], want["mags"][i], dtype, want32.get(key))
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("name", NAMES)
def test_both_entry_points_through_the_raw_abi(name, nq, alpha, dtype):
    f32 = dtype == torch.float32
    ref = reference(name, nq, alpha, f32)
    mu, var, y = (dev(ref[k], dtype) for k in ("mu", "var", "y"))
    tag = f"{name} nq={nq} alpha={alpha}"
    got = raw_led(name, nq, dtype, alpha, mu, var, y)
    for i, out in enumerate(("I", "g1", "g2")):
        check(f"{tag} {out}", got[i].cpu().numpy(), ref["vals"][i], ref["mags"][i], dtype, ref["vals32"][i] if f32 else None)
    if alpha == 1.0:
        # (b) at alpha = 1, I is the predictive log density: kernel against kernel, each within the bound of the same reference
        buf, pld = guarded(mu.numel(), dtype)
        nodes, weights = c_rule(nq)
        rc = _lib.call_rc("mf_lik_predict_log_density", dtype, mu.numel(), L.IDS[name], c_params(name), nq, nodes, weights, _lib.ptr(mu),
                          _lib.ptr(var), _lib.ptr(y), _lib.ptr(pld), _lib.stream_ptr(DEV))
        assert rc == 0 and guard_intact(buf, mu.numel())
        diff = float(((got[0] - pld).abs().double().cpu().numpy() / (ref["pld_mag"] + 1.0)).max())
        if f32:
            own = float((np.abs(ref["vals32"][0].astype(np.float64) - ref["vals"][0]) / (ref["pld_mag"] + 1.0)).max())
            print(f"ERR f32 {tag} I against mf_lik_predict_log_density: {diff:.3e}  numpy float32 {own:.3e}")
            assert diff <= 8.0 * own
        else:
            print(f"RATIO f64 {tag} I against mf_lik_predict_log_density: {diff / EPS:.2f}")
            assert diff <= K_F64 * EPS
    for lr in RATES:
        check_site_update(tag, name, nq, dtype, alpha, lr)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_block_with_guards(n, dtype):
    """One lane per point, 256 per block: sizes on both sides of a block, a single point and several blocks; every output and every
    site array is followed by a guard region that must stay as it was (raw_* assert it).  N = 1 is compared bit for bit with the
    first point of the N = 257 launch, whose accuracy the N = 257 case checks (a float32 yardstick made of one number may be exact by
    luck), and in float64 against the reference as well."""
    f32 = dtype == torch.float32
    for name in NAMES:
        if n == 1:
            ref, sref = reference(name, 20, 0.5, f32, 257), site_reference(name, 20, 0.5, f32, 257)
            big = raw_led(name, 20, dtype, 0.5, *(dev(ref[k], dtype) for k in ("mu", "var", "y")))
            one = raw_led(name, 20, dtype, 0.5, *(dev(ref[k][:1], dtype) for k in ("mu", "var", "y")))
            assert all(torch.equal(bits(o), bits(b[:1])) for o, b in zip(one, big))
            if not f32:                 # float64: the K eps bound on the single point as well
                for i, out in enumerate(("I", "g1", "g2")):
                    check(f"{name} N=1 {out}", one[i].cpu().numpy(), ref["vals"][i][:1], ref["mags"][i][:1], dtype)
            sites = [sref[k] for k in ("nat1", "nat2", "log_norm")]
            big = raw_pep(name, 20, dtype, 0.5, 0.3, *(dev(sref[k], dtype) for k in ("m", "s", "y")), sites)
            one = raw_pep(name, 20, dtype, 0.5, 0.3, *(dev(sref[k][:1], dtype) for k in ("m", "s", "y")), [a[:1] for a in sites])
            assert all(torch.equal(bits(o), bits(b[:1])) for o, b in zip(one, big))
            if not f32:
                spec, args = L.LIKELIHOODS[name], [sref[k][:1] for k in ("m", "s", "y")]
                got = [t.cpu().numpy() for t in one]
                own = P.pep_site_update(spec, *args, 0.5, 0.3, *[a[:1] for a in sites], 20)
                check(f"{name} N=1 cav_mu", got[3], own["cav_mu"], own["cav_mags"][0], dtype)
                check(f"{name} N=1 cav_var", got[4], own["cav_var"], own["cav_mags"][1], dtype)
                want = P.pep_site_update(spec, *args, 0.5, 0.3, *[a[:1] for a in sites], 20, at_cavity=(got[3], got[4]))
                assert not want["skipped"].any()
                for i, key in enumerate(("nat1", "nat2", "log_norm")):
                    check(f"{name} N=1 {key}", got[i], want[key], want["mags"][i], dtype)
            continue
        ref = reference(name, 20, 0.5, f32, n)
        mu, var, y = (dev(ref[k], dtype) for k in ("mu", "var", "y"))
        got = raw_led(name, 20, dtype, 0.5, mu, var, y)
        for i, out in enumerate(("I", "g1", "g2")):
            check(f"{name} N={n} {out}", got[i].cpu().numpy(), ref["vals"][i], ref["mags"][i], dtype, ref["vals32"][i] if f32 else None)
        check_site_update(f"{name} N={n}", name, 20, dtype, 0.5, 0.3, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_poisson_where_every_unshifted_term_underflows(dtype):
    """(a) y = 0, mu = 8, var = 1e-2: sum_i exp(alpha l_i) w_i is 0.0 in float64; the shifted sum gives I = -1421.145... at alpha = 1
    and -725.42... at alpha = 0.5.  The point rides at the end of the Poisson grid, so that the float32 yardstick is a maximum over
    257 points."""
    f32 = dtype == torch.float32
    spec = L.LIKELIHOODS[L.POISSON]
    grid = L.value_grid(L.POISSON)
    mu, var, y = (np.append(a, v).astype(np_dtype(dtype)).astype(np.float64) for a, v in zip(grid, (8.0, 1e-2, 0.0)))
    for alpha, value in ((1.0, -1421.145), (0.5, -725.42)):
        vals, mags = P.log_expected_density(spec, mu, var, y, alpha)
        vals32 = P.log_expected_density(spec, mu, var, y, alpha, dtype=np.float32)[0] if f32 else (None,) * 3
        got = raw_led(L.POISSON, 20, dtype, alpha, *(dev(a, dtype) for a in (mu, var, y)))
        for i, out in enumerate(("I", "g1", "g2")):
            check(f"poisson underflow alpha={alpha} {out}", got[i].cpu().numpy(), vals[i], mags[i], dtype, vals32[i])
        last = float(got[0][-1])
        assert np.isfinite(last) and abs(last - value) < (0.05 if f32 else 1e-2), last
        assert abs(vals[0][-1] - value) < 1e-2


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_null_combinations_of_the_optional_outputs(dtype):
    """(c)"""
    f32 = dtype == torch.float32
    ref = reference(L.BERNOULLI, 20, 0.5, f32, 257)
    mu, var, y = (dev(ref[k], dtype) for k in ("mu", "var", "y"))
    full = raw_led(L.BERNOULLI, 20, dtype, 0.5, mu, var, y)
    for mask in range(8):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        got = raw_led(L.BERNOULLI, 20, dtype, 0.5, mu, var, y, want)
        for g, f, w in zip(got, full, want):
            assert (g is None) == (not w) and (g is None or torch.equal(g, f))
    sref = site_reference(L.BERNOULLI, 20, 0.5, f32, 257)
    args = [dev(sref[k], dtype) for k in ("m", "s", "y")]
    sites = [sref[k] for k in ("nat1", "nat2", "log_norm")]
    both = raw_pep(L.BERNOULLI, 20, dtype, 0.5, 0.3, *args, sites)
    for want in ((False, False), (True, False), (False, True)):
        got = raw_pep(L.BERNOULLI, 20, dtype, 0.5, 0.3, *args, sites, want=want)
        assert all(torch.equal(g, b) for g, b in zip(got[:3], both[:3]))
        assert all((g is None) == (not w) and (g is None or torch.equal(g, b)) for g, b, w in zip(got[3:], both[3:], want))
    ones = torch.ones(257, dtype=torch.uint8, device=DEV)
    flagged = raw_pep(L.BERNOULLI, 20, dtype, 0.5, 0.3, *args, sites, update=ones)
    assert all(torch.equal(g, b) for g, b in zip(flagged, both)), "update = all ones is update = NULL"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_skipped_sites_stay_bit_identical_and_their_neighbours_are_updated(name, dtype):
    """(d) in ONE launch: a cavity precision that is zero and one that is negative, fvar = 0 and fvar < 0, NaN in fmu, in fvar, in y
    and in each of the three site numbers, and update = 0.  Those sites keep their bits (NaN payloads included), every other site
    is what the launch without the bad points gives, and the cavity goes out for every point - NaN exactly where it does not exist."""
    f32 = dtype == torch.float32
    n, alpha, lr = 257, 0.5, 0.3
    ref = site_reference(name, 20, alpha, f32, n)
    m, s, y, nat1, nat2, log_norm = (ref[k].copy() for k in ("m", "s", "y", "nat1", "nat2", "log_norm"))
    clean = raw_pep(name, 20, dtype, alpha, lr, *(dev(a, dtype) for a in (m, s, y)), (nat1, nat2, log_norm))
    nan = float("nan")
    s[3] = 2.0 ** -3
    nat2[3] = -(2.0 ** 3)                         # 1 / s + 2 alpha n2 = 8 + 2 x 0.5 x (-8) = 0, exactly
    nat2[64] = -1.0e3 / s[64]                     # negative cavity precision
    s[65] = 0.0
    s[100] = -1.0
    m[101] = nan
    s[102] = nan
    y[255] = nan
    nat1[256] = nan
    nat2[200] = nan
    log_norm[201] = nan
    update = np.ones(n, dtype=np.uint8)
    update[[0, 128]] = 0
    no_cavity = [3, 64, 65, 100, 102, 200]        # (a NaN mean or nat1 leaves the cavity VARIANCE defined)
    skipped = sorted(no_cavity + [101, 256, 255, 201, 0, 128])
    before = [dev(a, dtype) for a in (nat1, nat2, log_norm)]
    got = raw_pep(name, 20, dtype, alpha, lr, *(dev(a, dtype) for a in (m, s, y)), (nat1, nat2, log_norm), update=dev(update, torch.uint8))
    good = torch.ones(n, dtype=torch.bool, device=DEV)
    good[skipped] = False
    for g, b, c in zip(got[:3], before, clean[:3]):
        assert torch.equal(bits(g)[~good], bits(b)[~good]), "a skipped site must keep its bits"
        assert torch.equal(g[good], c[good]), "its neighbours are updated as without the bad points"
        assert not bool(torch.any(bits(g)[good] == bits(b)[good])), "every other site moved"
    for g, c, undefined in zip(got[3:], clean[3:], (no_cavity + [101, 256], no_cavity)):
        assert bool(torch.isnan(g[undefined]).all()), "no cavity: NaN"
        exists = torch.ones(n, dtype=torch.bool, device=DEV)
        exists[undefined] = False
        assert torch.equal(g[exists], c[exists]), "the cavity is written for every point, updated or not"


def test_empty_input_and_bad_arguments_launch_nothing():
    """(e)"""
    dtype = torch.float64
    ref = site_reference(L.STUDENTT, 20, 0.5, False, 65)
    ins = [dev(ref[k], dtype) for k in ("m", "s", "y")]
    outs = [torch.full((65,), SENTINEL, dtype=dtype, device=DEV) for _ in range(5)]
    nodes, weights = c_rule(20)
    p, o, s = [_lib.ptr(t) for t in ins], [_lib.ptr(t) for t in outs], _lib.stream_ptr(DEV)
    led = lambda *a: _lib.call_rc(LED, dtype, *a)      # noqa: E731
    pep = lambda *a: _lib.call_rc(PEP, dtype, *a)      # noqa: E731
    par = c_params(L.STUDENTT)
    assert led(0, 3, par, 20, nodes, weights, 0.5, *p, *o[:3], s) == 0
    assert pep(0, 3, par, 20, nodes, weights, 0.5, 0.5, *p, None, *o, s) == 0
    assert led(65, 7, par, 20, nodes, weights, 0.5, *p, *o[:3], s) == -2
    assert led(65, 3, None, 20, nodes, weights, 0.5, *p, *o[:3], s) == -3
    assert led(65, 3, par, 33, nodes, weights, 0.5, *p, *o[:3], s) == -4
    assert led(65, 3, par, 20, nodes, weights, 0.0, *p, *o[:3], s) == -7
    assert led(65, 3, par, 20, nodes, weights, 1.25, *p, *o[:3], s) == -7
    assert led(65, 3, par, 20, nodes, weights, 0.5, None, p[1], p[2], *o[:3], s) == -8
    assert led(65, 3, par, 20, nodes, weights, 0.5, p[0], None, p[2], *o[:3], s) == -9
    assert led(65, 3, par, 20, nodes, weights, 0.5, p[0], p[1], None, *o[:3], s) == -10
    assert led(65, 3, par, 20, nodes, weights, 0.5, *p, None, None, None, s) == 0          # nothing asked for
    assert pep(65, 7, par, 20, nodes, weights, 0.5, 0.5, *p, None, *o, s) == -2
    assert pep(65, 3, par, 0, nodes, weights, 0.5, 0.5, *p, None, *o, s) == -4
    assert pep(65, 3, par, 20, nodes, weights, float("nan"), 0.5, *p, None, *o, s) == -7
    assert pep(65, 3, par, 20, nodes, weights, 0.5, 2.0, *p, None, *o, s) == -8
    assert pep(65, 3, par, 20, nodes, weights, 0.5, -0.5, *p, None, *o, s) == -8
    assert pep(65, 3, par, 20, nodes, weights, 0.5, 0.5, None, p[1], p[2], None, *o, s) == -9
    assert pep(65, 3, par, 20, nodes, weights, 0.5, 0.5, p[0], None, p[2], None, *o, s) == -10
    assert pep(65, 3, par, 20, nodes, weights, 0.5, 0.5, p[0], p[1], None, None, *o, s) == -11
    assert pep(65, 3, par, 20, nodes, weights, 0.5, 0.5, *p, None, None, o[1], o[2], o[3], o[4], s) == -13
    assert pep(65, 3, par, 20, nodes, weights, 0.5, 0.5, *p, None, o[0], None, o[2], o[3], o[4], s) == -14
    assert pep(65, 3, par, 20, nodes, weights, 0.5, 0.5, *p, None, o[0], o[1], None, o[3], o[4], s) == -15
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in outs)
    with pytest.raises(ValueError, match="invalid argument #7"):
        _lib.call(LED, dtype, 65, 3, par, 20, nodes, weights, 2.0, *p, *o[:3], s)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_against_the_torch_composition_and_through_the_classes(name, dtype, monkeypatch):
    """(f) ``torch_pep_site_update`` on the same device tensors: two evaluations of the same formulas in the same precision, each
    within the bound of the helper; their difference is held to the same K in float64 (float32: 8 x the numpy float32 figure - the
    torch route has no double combination of the Poisson constant, measured 5.32).  Then the
    Likelihood methods on HIP tensors: the raw ABI's numbers, the documented shapes, one launch each, version counters moved."""
    f32 = dtype == torch.float32
    alpha, lr, n = 0.5, 0.3, 256
    spec, lik = L.LIKELIHOODS[name], build_likelihood(name)
    ref = site_reference(name, 20, alpha, f32, n)
    m, s, y = (dev(ref[k], dtype).reshape(4, 64, 1) for k in ("m", "s", "y"))
    sites = [ref[k] for k in ("nat1", "nat2", "log_norm")]
    raw = raw_pep(name, 20, dtype, alpha, lr, m.reshape(-1), s.reshape(-1), y.reshape(-1), sites)
    t1, t2, tn = dev(sites[0], dtype).reshape(4, 64, 1), dev(sites[1], dtype).reshape(4, 64, 1, 1), dev(sites[2], dtype).reshape(4, 64, 1)
    cav = ML.torch_pep_site_update(lik, m, s, y, alpha, lr, t1, t2, tn)
    at = (raw[3].double().cpu().numpy(), raw[4].double().cpu().numpy())
    want = P.pep_site_update(spec, ref["m"], ref["s"], ref["y"], alpha, lr, *sites, at_cavity=at)
    want32 = P.pep_site_update(spec, ref["m"], ref["s"], ref["y"], alpha, lr, *sites, at_cavity=at, dtype=np.float32) if f32 else {}
    for got, mine, key, mag in zip((t1, t2, tn), raw[:3], ("nat1", "nat2", "log_norm"), want["mags"]):
        scaled = (got.reshape(-1) - mine).abs().double().cpu().numpy() / (mag + 1.0)
        if f32:
            own = float((np.abs(want32[key].astype(np.float64) - want[key]) / (mag + 1.0)).max())
            print(f"ERR f32 {name} kernel against torch {key}: {scaled.max():.3e}  numpy float32 {own:.3e}")
            assert scaled.max() <= 8.0 * own
        else:
            print(f"RATIO f64 {name} kernel against torch {key}: {scaled.max() / EPS:.2f}")
            assert scaled.max() <= K_F64 * EPS
    assert bool(torch.isfinite(cav[0]).all()) and tuple(cav[0].shape) == (4, 64, 1)
    seen = []
    real = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real(base, *a))[1])

    def no_torch(*a, **k):
        raise AssertionError("the torch route must not run on HIP tensors")

    monkeypatch.setattr(ML, "torch_log_expected_density", no_torch)
    monkeypatch.setattr(ML, "torch_pep_site_update", no_torch)
    u1, u2, un = dev(sites[0], dtype).reshape(4, 64, 1), dev(sites[1], dtype).reshape(4, 64, 1, 1), dev(sites[2], dtype).reshape(4, 64, 1)
    versions = [t._version for t in (u1, u2, un)]
    lik.pep_site_update(m, s, y, alpha, lr, u1, u2, un)
    assert all(t._version > v for t, v in zip((u1, u2, un), versions)), "an in-place write torch has to know about"
    assert all(torch.equal(u.reshape(-1), r) for u, r in zip((u1, u2, un), raw[:3]))
    flags = torch.zeros(4, 64, 1, dtype=torch.bool, device=DEV)
    flags[:, ::2] = True
    v1, v2, vn = dev(sites[0], dtype).reshape(4, 64, 1), dev(sites[1], dtype).reshape(4, 64, 1, 1), dev(sites[2], dtype).reshape(4, 64, 1)
    lik.pep_site_update(m, s, y, alpha, lr, v1, v2, vn, update=flags)
    assert torch.equal(v1[:, ::2], u1[:, ::2]) and torch.equal(v1[:, 1::2], dev(sites[0], dtype).reshape(4, 64, 1)[:, 1::2])
    cref = reference(name, 20, alpha, f32)
    mu, var, obs = (dev(cref[k], dtype).reshape(4, 64, 1) for k in ("mu", "var", "y"))
    led = raw_led(name, 20, dtype, alpha, mu.reshape(-1), var.reshape(-1), obs.reshape(-1))
    value = lik.log_expected_density(mu, var, obs, alpha)
    assert tuple(value.shape) == (4, 64) and torch.equal(value.reshape(-1), led[0])
    obj, (g1, g2) = lik.grad_log_expected_density(mu, var, obs, alpha)
    assert tuple(obj.shape) == (4, 64) and tuple(g1.shape) == tuple(g2.shape) == (4, 64, 1)
    assert torch.equal(obj.reshape(-1), led[0]) and torch.equal(g1.reshape(-1), led[1]) and torch.equal(g2.reshape(-1), led[2])
    assert seen == [PEP, PEP, LED, LED, LED]
