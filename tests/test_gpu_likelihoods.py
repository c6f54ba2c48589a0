"""
GPU tests of the likelihood kernels (csrc/mf_lik.hip) through the raw C ABI and through markovflow_amd/likelihoods.py, against the
numpy / scipy reference of tests/helpers/likelihood_closed_forms.py.

Tolerances.
  float64: ``|err| <= K eps (magnitude + 1)``, eps = 2^-52, with the helper's magnitudes, the sums of the absolute terms:
    sum w_i |l(f_i)| for a value, sum w_i |l'(f_i)| and sum w_i |l'(f_i)| |x_i| / sqrt(2 var) for the derivatives.  K_F64 below and what has been
    measured on an MI355X are next to each other.
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
from helpers import likelihood_closed_forms as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
# The issue's starting K.  Measured on an MI355X on scales this file still uses: ve 2.58, predict_log_density 23.67 (Poisson,
# nq = 32).  The derivative and site-update ratios on the sums above are printed by check() ("RATIO f64 ..."): K becomes 4 x the
# largest once they are recorded; a ratio above 64 wants an explanation, not a larger K.
K_F64 = 64.0
NAMES = [L.GAUSSIAN, L.BERNOULLI, L.POISSON, L.STUDENTT]
NQS = [1, 7, 20, 32]
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
DTYPES = [torch.float64, torch.float32]
GUARD, SENTINEL = 64, -77.25


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
def reference(name, nq, f32, n=256):
    """Inputs (rounded to the dtype under test, n points of the grid repeated) and the float64 helper on them - computed once
    per case and shared, read-only."""
    spec = L.LIKELIHOODS[name]
    dt = np.float32 if f32 else np.float64
    mu, var, y = (np.resize(a, n).astype(dt).astype(np.float64) for a in L.value_grid(name))
    vals, mags = L.expectations(spec, mu, var, y, nq)
    ref = dict(mu=mu, var=var, y=y, vals=vals, mags=mags, pld=L.predict_log_density(spec, mu, var, y, nq),
               pld_mag=L.predict_log_density_magnitude(spec, mu, var, y, nq))
    if f32:
        ref["vals32"] = L.expectations(spec, mu, var, y, nq, dtype=np.float32)[0]
        ref["pld32"] = L.predict_log_density(spec, mu, var, y, nq, dtype=np.float32)
    for v in ref.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return ref


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV).contiguous()


def guarded(n, dtype):
    """An output of n elements followed by a sentinel-filled guard region."""
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n]


def guard_intact(buf, n):
    return bool(torch.all(buf[n:] == SENTINEL))


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


def raw_ve(name, nq, dtype, mu, var, y, want=(True, True, True)):
    n = mu.numel()
    bufs = [guarded(n, dtype) if w else (None, None) for w in want]
    nodes, weights = c_rule(nq)
    rc = _lib.call_rc("mf_lik_variational_expectations", dtype, n, L.IDS[name], c_params(name), nq, nodes, weights, _lib.ptr(mu),
                      _lib.ptr(var), _lib.ptr(y), *[_lib.ptr(b[1]) for b in bufs], _lib.stream_ptr(DEV))
    assert rc == 0
    assert all(b[0] is None or guard_intact(b[0], n) for b in bufs)
    return [None if b[1] is None else b[1] for b in bufs]


def raw_site(name, nq, dtype, mu, var, y, lr, nat1, nat2, want_ve=True):
    n = mu.numel()
    ve_buf, ve = guarded(n, dtype) if want_ve else (None, None)
    nodes, weights = c_rule(nq)
    rc = _lib.call_rc("mf_lik_cvi_site_update", dtype, n, L.IDS[name], c_params(name), nq, nodes, weights, _lib.ptr(mu),
                      _lib.ptr(var), _lib.ptr(y), lr, _lib.ptr(nat1), _lib.ptr(nat2), _lib.ptr(ve), _lib.stream_ptr(DEV))
    assert rc == 0 and (ve_buf is None or guard_intact(ve_buf, n))
    return ve


def raw_pld(name, nq, dtype, mu, var, y):
    n = mu.numel()
    buf, out = guarded(n, dtype)
    nodes, weights = c_rule(nq)
    rc = _lib.call_rc("mf_lik_predict_log_density", dtype, n, L.IDS[name], c_params(name), nq, nodes, weights, _lib.ptr(mu),
                      _lib.ptr(var), _lib.ptr(y), _lib.ptr(out), _lib.stream_ptr(DEV))
    assert rc == 0 and guard_intact(buf, n)
    return out


def site_reference(ref, lr, nat1_0, nat2_0, vals):
    _, g_mu, g_var = (np.asarray(v, dtype=np.float64) for v in vals)
    return (1 - lr) * nat1_0 + lr * (g_mu - 2 * g_var * ref["mu"]), (1 - lr) * nat2_0 + lr * g_var


def site_magnitudes(ref, nat1_0, nat2_0):
    return np.abs(nat1_0) + ref["mags"][1] + 2 * ref["mags"][2] * np.abs(ref["mu"]), np.abs(nat2_0) + ref["mags"][2]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("name", NAMES)
def test_three_entry_points_through_the_raw_abi(name, nq, dtype):
    f32 = dtype == torch.float32
    ref = reference(name, nq, f32)
    mu, var, y = (dev(ref[k], dtype) for k in ("mu", "var", "y"))
    tag = f"{name} nq={nq}"
    got = raw_ve(name, nq, dtype, mu, var, y)
    for i, out in enumerate(("ve", "g_mu", "g_var")):
        check(f"{tag} {out}", got[i].cpu().numpy(), ref["vals"][i], ref["mags"][i], dtype, ref["vals32"][i] if f32 else None)
    pld = raw_pld(name, nq, dtype, mu, var, y)
    check(f"{tag} predict_log_density", pld.cpu().numpy(), ref["pld"], ref["pld_mag"], dtype, ref.get("pld32"))
    rng = np.random.default_rng(5)
    nat1_0 = rng.normal(size=mu.numel()).astype(np_dtype(dtype)).astype(np.float64)
    nat2_0 = (-0.5 - rng.random(mu.numel())).astype(np_dtype(dtype)).astype(np.float64)
    for lr in (0.1, 1.0):
        nat1, nat2 = dev(nat1_0, dtype), dev(nat2_0, dtype)
        ve = raw_site(name, nq, dtype, mu, var, y, lr, nat1, nat2)
        assert torch.equal(ve, got[0]), "the site update's optional value is the expectation kernel's"
        want = site_reference(ref, lr, nat1_0, nat2_0, ref["vals"])
        mags = site_magnitudes(ref, nat1_0, nat2_0)
        own = (None, None)
        if f32:
            lr32, g32 = np.float32(lr), [np.asarray(v, dtype=np.float32) for v in ref["vals32"]]
            m32, one = ref["mu"].astype(np.float32), np.float32(1)
            own = ((one - lr32) * nat1_0.astype(np.float32) + lr32 * (g32[1] - np.float32(2) * g32[2] * m32),
                   (one - lr32) * nat2_0.astype(np.float32) + lr32 * g32[2])
        check(f"{tag} lr={lr} nat1", nat1.cpu().numpy(), want[0], mags[0], dtype, own[0])
        check(f"{tag} lr={lr} nat2", nat2.cpu().numpy(), want[1], mags[1], dtype, own[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_wavefront_and_the_block_with_guards(n, dtype):
    """One lane per point, 256 per block: sizes on both sides of a wavefront (64) and of a block (256), several blocks (1000);
    every output is followed by a guard region that must stay as it was (raw_* assert it)."""
    f32 = dtype == torch.float32
    for name in NAMES:
        ref = reference(name, 20, f32, n)
        mu, var, y = (dev(ref[k], dtype) for k in ("mu", "var", "y"))
        got = raw_ve(name, 20, dtype, mu, var, y)
        for i, out in enumerate(("ve", "g_mu", "g_var")):
            check(f"{name} N={n} {out}", got[i].cpu().numpy(), ref["vals"][i], ref["mags"][i], dtype, ref["vals32"][i] if f32 else None)
        pld = raw_pld(name, 20, dtype, mu, var, y)
        check(f"{name} N={n} predict_log_density", pld.cpu().numpy(), ref["pld"], ref["pld_mag"], dtype, ref.get("pld32"))
        nat1_buf, nat1 = guarded(n, dtype)
        nat2_buf, nat2 = guarded(n, dtype)
        nat1.fill_(0.25)
        nat2.fill_(-0.75)
        raw_site(name, 20, dtype, mu, var, y, 0.5, nat1, nat2, want_ve=False)
        assert guard_intact(nat1_buf, n) and guard_intact(nat2_buf, n)
        # against the kernel's OWN derivatives: g1 = g_mu - 2 g_var mu, then (1 - lr) nat + lr g - at most five roundings of the
        # terms' magnitudes (product, difference, two products, sum), bounded by 8 ulp of the sum of the absolute terms
        own = [g.double().cpu().numpy() for g in got]
        want = site_reference(ref, 0.5, 0.25, -0.75, own)
        ulp = 2.0 ** -23 if f32 else EPS
        scale1 = 0.125 + 0.5 * (np.abs(own[1]) + 2 * np.abs(own[2] * ref["mu"]))
        scale2 = 0.375 + 0.5 * np.abs(own[2])
        assert np.all(np.abs(nat1.double().cpu().numpy() - want[0]) <= 8 * ulp * scale1)
        assert np.all(np.abs(nat2.double().cpu().numpy() - want[1]) <= 8 * ulp * scale2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_null_combinations_of_the_optional_outputs(dtype):
    ref = reference(L.BERNOULLI, 20, dtype == torch.float32, 257)
    mu, var, y = (dev(ref[k], dtype) for k in ("mu", "var", "y"))
    full = raw_ve(L.BERNOULLI, 20, dtype, mu, var, y)
    for mask in range(8):
        want = tuple(bool(mask >> i & 1) for i in range(3))
        got = raw_ve(L.BERNOULLI, 20, dtype, mu, var, y, want)
        for g, f, w in zip(got, full, want):
            assert (g is None) == (not w) and (g is None or torch.equal(g, f))
    nat = [dev(np.linspace(-1, 1, 257), dtype) for _ in range(4)]
    assert raw_site(L.BERNOULLI, 20, dtype, mu, var, y, 0.3, nat[0], nat[1], want_ve=False) is None
    ve = raw_site(L.BERNOULLI, 20, dtype, mu, var, y, 0.3, nat[2], nat[3], want_ve=True)
    assert torch.equal(ve, full[0]) and torch.equal(nat[0], nat[2]) and torch.equal(nat[1], nat[3])


def test_empty_input_and_bad_arguments_launch_nothing():
    dtype = torch.float64
    ref = reference(L.STUDENTT, 20, False, 65)
    mu, var, y = (dev(ref[k], dtype) for k in ("mu", "var", "y"))
    outs = [torch.full((65,), SENTINEL, dtype=dtype, device=DEV) for _ in range(3)]
    nodes, weights = c_rule(20)
    p = [_lib.ptr(t) for t in (mu, var, y)]
    o = [_lib.ptr(t) for t in outs]
    s = _lib.stream_ptr(DEV)
    ve = lambda *a: _lib.call_rc("mf_lik_variational_expectations", dtype, *a)      # noqa: E731
    site = lambda *a: _lib.call_rc("mf_lik_cvi_site_update", dtype, *a)             # noqa: E731
    pld = lambda *a: _lib.call_rc("mf_lik_predict_log_density", dtype, *a)          # noqa: E731
    par = c_params(L.STUDENTT)
    assert ve(0, 3, par, 20, nodes, weights, *p, *o, s) == 0
    assert site(0, 3, par, 20, nodes, weights, *p, 0.5, o[0], o[1], o[2], s) == 0
    assert pld(0, 3, par, 20, nodes, weights, *p, o[0], s) == 0
    assert ve(65, 7, par, 20, nodes, weights, *p, *o, s) == -2
    assert ve(65, 3, None, 20, nodes, weights, *p, *o, s) == -3
    assert ve(65, 3, par, 33, nodes, weights, *p, *o, s) == -4
    assert ve(65, 3, par, 0, nodes, weights, *p, *o, s) == -4
    assert ve(65, 3, par, 20, nodes, weights, p[0], None, p[2], *o, s) == -8
    assert ve(65, 3, par, 20, nodes, weights, p[0], p[1], None, *o, s) == -9
    assert site(65, 3, par, 20, nodes, weights, *p, 2.0, o[0], o[1], o[2], s) == -10
    assert site(65, 3, par, 20, nodes, weights, *p, 0.5, None, o[1], o[2], s) == -11
    assert site(65, 3, par, 20, nodes, weights, *p, 0.5, o[0], None, o[2], s) == -12
    assert pld(65, 3, par, 20, nodes, weights, *p, None, s) == -10
    assert ve(65, 3, par, 20, nodes, weights, *p, None, None, None, s) == 0          # nothing asked for
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == SENTINEL)) for t in outs)
    with pytest.raises(ValueError, match="invalid argument #4"):
        _lib.call("mf_lik_predict_log_density", dtype, 65, 3, par, 40, nodes, weights, *p, o[0], s)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_a_bad_variance_gives_nan_in_its_own_point_and_leaves_the_neighbours_bit_identical(name, dtype):
    ref = reference(name, 20, dtype == torch.float32, 257)
    mu, var, y = (dev(ref[k], dtype) for k in ("mu", "var", "y"))
    nat0 = dev(np.linspace(-2, -1, 257), dtype)

    def everything(v):
        nat1, nat2 = nat0.clone(), nat0.clone()
        ve = raw_site(name, 20, dtype, mu, v, y, 0.5, nat1, nat2)
        return raw_ve(name, 20, dtype, mu, v, y) + [raw_pld(name, 20, dtype, mu, v, y), ve, nat1, nat2]

    clean = everything(var)
    bad = torch.tensor([0, 63, 64, 100, 256], device=DEV)
    dirty_var = var.clone()
    dirty_var[bad] = torch.tensor([0.0, float("nan"), -1.0, 0.0, float("nan")], dtype=dtype, device=DEV)
    dirty = everything(dirty_var)
    good = torch.ones(257, dtype=torch.bool, device=DEV)
    good[bad] = False
    for c, d in zip(clean, dirty):
        assert bool(torch.isnan(d[bad]).all()), "a point outside the domain must come out NaN"
        assert torch.equal(c[good], d[good]), "its neighbours must not change by a bit"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_classes_run_the_kernels(name, dtype, monkeypatch):
    """The Likelihood classes on HIP tensors: the same numbers as the raw ABI, gpflow's shapes, gradients through backward(), and
    no launch other than the mf_lik kernels'."""
    params = L.LIKELIHOODS[name][1]
    lik = {L.GAUSSIAN: lambda: mfa.Gaussian(params[0]), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson,
           L.STUDENTT: lambda: mfa.StudentT(*params)}[name]()
    ref = reference(name, 20, dtype == torch.float32)
    mu, var, y = (dev(ref[k], dtype).reshape(4, 64, 1) for k in ("mu", "var", "y"))
    raw = raw_ve(name, 20, dtype, mu.reshape(-1), var.reshape(-1), y.reshape(-1))
    raw_density = raw_pld(name, 20, dtype, mu.reshape(-1), var.reshape(-1), y.reshape(-1))
    seen = []
    real = _lib.call_rc
    monkeypatch.setattr(_lib, "call_rc", lambda base, *a: (seen.append(base), real(base, *a))[1])
    fmu, fvar = mu.clone().requires_grad_(True), var.clone().requires_grad_(True)
    out = lik.variational_expectations(fmu, fvar, y)
    assert tuple(out.shape) == (4, 64) and torch.equal(out.detach().reshape(-1), raw[0])
    weights = torch.linspace(0.5, 1.5, 256, dtype=dtype, device=DEV).reshape(4, 64)
    (out * weights).sum().backward()
    assert torch.equal(fmu.grad.reshape(-1), weights.reshape(-1) * raw[1])
    assert torch.equal(fvar.grad.reshape(-1), weights.reshape(-1) * raw[2])
    density = lik.predict_log_density(mu, var, y)
    assert tuple(density.shape) == (4, 64) and torch.equal(density.reshape(-1), raw_density)
    nat1, nat2 = torch.zeros_like(mu), torch.full_like(mu, -0.5)[..., None]
    v1, v2 = nat1._version, nat2._version
    lik.cvi_site_update(mu, var, y, 1.0, nat1, nat2)
    assert nat1._version > v1 and nat2._version > v2, "an in-place write torch has to know about"
    assert torch.equal(nat2.reshape(-1), raw[2])
    assert seen == ["mf_lik_variational_expectations", "mf_lik_predict_log_density", "mf_lik_cvi_site_update"]
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(lik.variational_expectations(fmu, fvar, y).sum(), fmu, create_graph=True)
    mean, variance = lik.predict_mean_and_var(mu, var)
    assert mean.is_cuda and tuple(mean.shape) == tuple(variance.shape) == (4, 64, 1)
