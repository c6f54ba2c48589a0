"""
GPU tests of ``mf_mean_response_*`` and ``mf_mean_response_grad_*`` (csrc/mf_sde.hip) through the raw C ABI, with a guard region behind
every output and workspace, against the long double reference of tests/helpers/mean_function_closed_forms.py (direct sums over the
actions, not the recurrence).

``(B, K, N)`` = (3, 5, 37): a partial last wavefront and wavefronts that straddle series; (2, 1, 130): a single action and more than one
block per series; (2, 70, 130) with one time point per bin first: more bins than lanes, and the first block of 64 points of every
series holds 64 distinct bins, so the reverse mode writes and reads the last record slot of a block (asserted from the bins);
(1, 1, 1).  Every case with N >= 8 holds points before the first action (bitwise zero), points exactly on an action time (bitwise
equal to a run with that action's right-hand side zeroed), one point 1e3 lengthscales behind the last action and, for K >= 2, a
duplicated action time; the (3, 5, 37) cases run a second time with shuffled time points.

Tolerances are measured per case and series (``mean_function_closed_forms.allowed``): the yardstick - the recurrence in numpy in the
working dtype - against the reference, as errors scaled by the summed magnitudes of the terms; the kernel is allowed 8 x the
yardstick's largest scaled error with a floor of 8 d eps.  Every test prints its largest ratio.
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import mean_function_closed_forms as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 64, -77.25
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
SHAPES = [(3, 5, 37), (2, 1, 130), (2, 70, 130), (1, 1, 1)]
TWO_PI = 2.0 * np.pi

# name -> (components (order, osc, lam, omega), output map, outputs m, whether `a` is exercised)
SIGNATURES = {
    "m12": ([(1, 0, 1.0 / 0.8, 0.0)], [0], 1, True),
    "m32": ([(3, 0, np.sqrt(3.0) / 1.1, 0.0)], [0], 1, True),
    "m52": ([(5, 0, np.sqrt(5.0) / 1.4, 0.0)], [0], 1, True),
    "m32+m52": ([(3, 0, np.sqrt(3.0) / 0.9, 0.0), (5, 0, np.sqrt(5.0) / 1.6, 0.0)], [0, 0], 1, True),
    "imo_m12_m52": ([(1, 0, 1.0 / 0.7, 0.0), (5, 0, np.sqrt(5.0) / 1.2, 0.0)], [0, 1], 2, True),
    "m32xosc": ([(3, 1, np.sqrt(3.0) / 1.3, TWO_PI / 2.5)], [0], 1, True),
    "oscxm32": ([(3, 2, np.sqrt(3.0) / 1.3, TWO_PI / 2.5)], [0], 1, True),
    "constxosc": ([(0, 1, 0.0, TWO_PI / 3.0)], [0], 1, True),
    "const+m32": ([(0, 0, 0.0, 0.0), (3, 0, np.sqrt(3.0) / 1.1, 0.0)], [0, 0], 1, False),     # (impulse only: F is singular)
}


def tt(x, dtype):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def guards_intact(*bufs):
    return all(b is None or bool(torch.all(b[-GUARD:] == SENTINEL)) for b in bufs)


def need_reference(dtype):
    if dtype == torch.float64 and not MC.longdouble_ok():
        pytest.skip("numpy.longdouble is no wider than a double here: no reference for the float64 accuracy")


def ints(xs):
    return (ctypes.c_int * len(xs))(*xs)


def series_comps(comps, b, per_series):
    """The components of series ``b``: with per-series hyper-parameters every series has its own ``lam`` and ``omega``."""
    scale = 1.0 + 0.25 * b if per_series else 1.0
    return [(o, r, lam * scale, om / scale) for o, r, lam, om in comps]


@functools.lru_cache(maxsize=None)
def make_case(name, shape, per_series, dtype_name, shuffled):
    """Inputs rounded to the working dtype (the kernel's input IS the rounded value) and the long double reference, computed once
    and shared by the forward and the reverse test."""
    comps, out_map, m, with_a = SIGNATURES[name]
    bsz, num, n = shape
    npd = np.dtype(dtype_name).type
    d, nc = MC.state_dim(comps), len(comps)
    rng = np.random.default_rng(zlib.crc32(repr((name, shape, per_series, dtype_name)).encode()))
    longest = max([np.sqrt(o) / lam for o, _, lam, _ in comps if o > 0] + [1.0])
    tau = np.sort(rng.uniform(0.0, 6.0, size=(bsz, num)), axis=-1).astype(npd)
    if num >= 2:                                                                  # a duplicated action time; with one point per bin
        dup = num // 2 if num < 64 else num - 1                                   # it lies behind the 64 bins of the first block
        tau[:, dup] = tau[:, dup - 1]
    t = np.zeros((bsz, n), dtype=npd)
    on_action = []                                                                # (series, point, action) of the points ON an action
    for b in range(bsz):
        pts = []
        if num >= 64:                                                             # one point per bin, consecutive points in consecutive bins
            edges = np.concatenate([tau[b].astype(np.float64), [tau[b, -1] + 0.5]])
            pts += [0.5 * (edges[k] + edges[k + 1]) for k in range(num)]
        if n >= 8:
            pts += [float(tau[b, 0]) - 0.3, float(tau[b, 0]) - 1e3, float(tau[b, 0])]
            on_action.append((b, len(pts) - 1, 0))
            q = num - 1
            pts.append(float(tau[b, q]))
            on_action.append((b, len(pts) - 1, q))
            pts.append(float(tau[b, -1]) + 1e3 * longest)
        while len(pts) < n:
            pts.append(rng.uniform(float(tau[b, 0]) - 0.5, float(tau[b, -1]) + 3.0) if n > 1 else float(tau[b, -1]) + 0.7)
        t[b] = np.asarray(pts[:n]).astype(npd)
    if shuffled:
        perm = rng.permutation(n)
        t = t[:, perm]
        inv = np.argsort(perm)
        on_action = [(b, int(inv[p]), q) for b, p, q in on_action]
    r = rng.standard_normal((bsz, num, d)).astype(npd)
    a = rng.standard_normal((bsz, num, d)).astype(npd) if with_a else None
    g = rng.standard_normal((bsz, n, m)).astype(npd)
    lam = np.array([[c[2] for c in series_comps(comps, b, per_series)] for b in range(bsz)]).astype(npd)
    om = np.array([[c[3] for c in series_comps(comps, b, per_series)] for b in range(bsz)]).astype(npd)
    h = MC.emission(comps, out_map, m)
    ref = []
    for b in range(bsz):
        cb = [(o, osc, float(lam[b, i]), float(om[b, i])) for i, (o, osc, _, _) in enumerate(comps)]     # (the rounded values)
        ref.append((cb,) + MC.linear_map(cb, tau[b], t[b]))
    return dict(comps=comps, out_map=out_map, m=m, d=d, nc=nc, tau=tau, t=t, r=r, a=a, g=g, h=h, ref=ref, on_action=on_action,
                lam=lam if per_series else lam[0], om=om if per_series else om[0])


def run_forward(case, dtype, per_series, r, a, want_state=True):
    bsz, num = case["tau"].shape
    n, d, m, nc = case["t"].shape[1], case["d"], case["m"], case["nc"]
    (f_buf, f), (c_buf, coef) = guarded((bsz, n, m), dtype), guarded((bsz, num, d), dtype)
    s_buf, state = guarded((bsz, n, d), dtype) if want_state else (None, None)
    orders, oscs = [c[0] for c in case["comps"]], [c[1] for c in case["comps"]]
    held = [tt(case["lam"], dtype), tt(case["om"], dtype), tt(case["tau"], dtype), tt(r, dtype), None if a is None else tt(a, dtype),
            tt(case["t"], dtype)]
    rc = _lib.call_rc("mf_mean_response", dtype, bsz, num, n, nc, ints(orders), ints(oscs), _lib.ptr(held[0]), _lib.ptr(held[1]),
                      int(per_series), _lib.ptr(held[2]), _lib.ptr(held[3]), _lib.ptr(held[4]), _lib.ptr(held[5]), m,
                      ints(case["out_map"]), _lib.ptr(f), _lib.ptr(state), _lib.ptr(coef), _lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(f_buf, s_buf, c_buf)
    return f.cpu().numpy(), None if state is None else state.cpu().numpy()


def run_reverse(case, dtype, per_series, g, want_a=True):
    bsz, num = case["tau"].shape
    n, d, m, nc = case["t"].shape[1], case["d"], case["m"], case["nc"]
    r_buf, g_r = guarded((bsz, num, d), dtype)
    a_buf, g_a = guarded((bsz, num, d), dtype) if want_a else (None, None)
    ws_bytes = int(_lib.load().mf_mean_response_grad_workspace_bytes(bsz, n, nc, d, np.dtype(NP[dtype]).itemsize))
    assert ws_bytes > 0
    ws_buf = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    orders, oscs = [c[0] for c in case["comps"]], [c[1] for c in case["comps"]]
    held = [tt(case["lam"], dtype), tt(case["om"], dtype), tt(case["tau"], dtype), tt(case["t"], dtype), tt(g, dtype)]
    rc = _lib.call_rc("mf_mean_response_grad", dtype, bsz, num, n, nc, ints(orders), ints(oscs), _lib.ptr(held[0]), _lib.ptr(held[1]),
                      int(per_series), _lib.ptr(held[2]), _lib.ptr(held[3]), m, ints(case["out_map"]), _lib.ptr(held[4]), _lib.ptr(g_r),
                      _lib.ptr(g_a), _lib.ptr(ws_buf), ws_bytes, _lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(r_buf, a_buf) and bool(torch.all(ws_buf[ws_bytes:] == 0x5A))
    return g_r.cpu().numpy(), None if g_a is None else g_a.cpu().numpy()


def project(case, state, npd):
    """``H state`` summed in the order of the components, in the working dtype."""
    out = np.zeros(state.shape[:-1] + (case["m"],), dtype=npd)
    for off, o in zip(MC.offsets(case["comps"]), case["out_map"]):
        out[..., o] = out[..., o] + state[..., off]
    return out


CASES = [(s, False) for s in SHAPES] + [((3, 5, 37), True)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("per_series", [False, True], ids=["shared", "per_series"])
@pytest.mark.parametrize("shape,shuffled", CASES, ids=lambda v: "shuffled" if v is True else "" if v is False else "B%dK%dN%d" % v)
@pytest.mark.parametrize("name", list(SIGNATURES))
def test_forward(name, shape, shuffled, per_series, dtype):
    need_reference(dtype)
    npd = NP[dtype]
    case = make_case(name, shape, per_series, np.dtype(npd).name, shuffled)
    d, h = case["d"], case["h"]
    worst = 0.0
    for a in ([case["a"], None] if case["a"] is not None else [None]):
        f, state = run_forward(case, dtype, per_series, case["r"], a)
        f_only, _ = run_forward(case, dtype, per_series, case["r"], a, want_state=False)
        assert np.array_equal(f, f_only)
        assert np.array_equal(project(case, state, npd), f)                        # H state IS f
        for b, (cb, m_r, m_a) in enumerate(case["ref"]):
            before = MC.bins(case["tau"][b], case["t"][b]) < 0
            assert not np.any(state[b][before]) and not np.any(f[b][before])       # exact zeros before the first action
            ref = np.einsum("nikj,kj->ni", m_r, case["r"][b].astype(MC.LD))
            if a is not None:
                ref = ref + np.einsum("nikj,kj->ni", m_a, a[b].astype(MC.LD))
            mag = MC.forward_magnitude(m_r, m_a, case["r"][b], None if a is None else a[b])
            yard = MC.recurrence(cb, case["tau"][b], case["r"][b], None if a is None else a[b], case["t"][b], npd)
            bound = MC.allowed(MC.scaled_error(yard, ref, mag, npd), d, npd)
            err = MC.scaled_error(state[b], ref, mag, npd)
            assert np.all(np.isfinite(state[b])) and err.max() <= bound, (b, err.max(), bound)
            worst = max(worst, err.max() / bound)
            bound_f = MC.allowed(MC.scaled_error(yard.astype(MC.LD) @ h.T, ref @ h.T, mag @ h.T, npd), d, npd)
            err_f = MC.scaled_error(f[b], ref @ h.T, mag @ h.T, npd)
            assert err_f.max() <= bound_f, (b, err_f.max(), bound_f)
            worst = max(worst, err_f.max() / bound_f)
        # a point exactly ON an action time does not see that action: bitwise the value with the action's sources zeroed
        for b, p, q in case["on_action"]:
            r0 = case["r"].copy()
            r0[b, q] = 0
            a0 = None
            if a is not None:
                a0 = a.copy()
                a0[b, q] = 0
            f0, s0 = run_forward(case, dtype, per_series, r0, a0)
            assert np.array_equal(f0[b, p], f[b, p]) and np.array_equal(s0[b, p], state[b, p])
    print(f"mean_response forward {name} {shape} largest error / allowed: {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("per_series", [False, True], ids=["shared", "per_series"])
@pytest.mark.parametrize("shape,shuffled", CASES, ids=lambda v: "shuffled" if v is True else "" if v is False else "B%dK%dN%d" % v)
@pytest.mark.parametrize("name", list(SIGNATURES))
def test_reverse(name, shape, shuffled, per_series, dtype):
    need_reference(dtype)
    npd = NP[dtype]
    case = make_case(name, shape, per_series, np.dtype(npd).name, shuffled)
    d, h = case["d"], case["h"]
    if shape[1] >= 64:      # every series' first block of 64 points fills all 64 record slots
        for b in range(shape[0]):
            first = MC.bins(case["tau"][b], case["t"][b])[:64]
            assert first.min() >= 0 and len(set(first.tolist())) == 64
    g_r, g_a = run_reverse(case, dtype, per_series, case["g"])
    again_r, again_a = run_reverse(case, dtype, per_series, case["g"])
    assert np.array_equal(g_r, again_r) and np.array_equal(g_a, again_a)           # deterministic: bit for bit
    only_r, none = run_reverse(case, dtype, per_series, case["g"], want_a=False)   # a NULL g_a is accepted
    assert none is None and np.array_equal(only_r, g_r)
    worst = 0.0
    for b, (cb, m_r, m_a) in enumerate(case["ref"]):
        g_state = case["g"][b].astype(MC.LD) @ h
        yard_r, yard_a = MC.reverse_recurrence(cb, case["tau"][b], case["t"][b], g_state.astype(npd), npd)
        for got, yard, mat in ((g_r[b], yard_r, m_r), (g_a[b], yard_a, m_a)):
            ref = np.einsum("nikj,ni->kj", mat, g_state)
            mag = MC.reverse_magnitude(mat, g_state)
            bound = MC.allowed(MC.scaled_error(yard, ref, mag, npd), d, npd)
            err = MC.scaled_error(got, ref, mag, npd)
            assert np.all(np.isfinite(got)) and err.max() <= bound, (b, err.max(), bound)
            worst = max(worst, err.max() / bound)
    print(f"mean_response reverse {name} {shape} largest error / allowed: {worst:.3f}")


def test_argument_checks():
    """The negative position of the offending argument, before any launch."""
    dtype = torch.float64
    x, f_out, c_out = (torch.zeros(8, dtype=dtype, device=DEV) for _ in range(3))
    p, pf, pc, stream = _lib.ptr(x), _lib.ptr(f_out), _lib.ptr(c_out), _lib.stream_ptr(torch.device(DEV))

    def fwd(bsz=1, num=1, n=1, nc=1, orders=(3,), oscs=(0,), lam=p, om=None, tau=p, r=p, t=p, m=1, out=(0,), f=pf, coef=pc):
        return _lib.call_rc("mf_mean_response", dtype, bsz, num, n, nc, ints(orders), ints(oscs), lam, om, 0, tau, r, None, t, m,
                            ints(out), f, None, coef, stream)

    assert fwd() == 0
    assert fwd(bsz=-1) == -1 and fwd(num=0) == -2 and fwd(n=-1) == -3 and fwd(nc=17, orders=(1,) * 17, oscs=(0,) * 17, out=(0,) * 17) == -4
    assert fwd(orders=(2,)) == -5 and fwd(oscs=(3,)) == -6 and fwd(lam=None) == -7 and fwd(oscs=(1,)) == -8
    assert fwd(tau=None) == -10 and fwd(r=None) == -11 and fwd(t=None) == -13 and fwd(m=2) == -14 and fwd(out=(1,)) == -15
    assert fwd(f=None) == -16 and fwd(coef=None) == -18
    assert fwd(bsz=0) == 0 and fwd(n=0) == 0
    lib = _lib.load()
    assert lib.mf_mean_response_grad_workspace_bytes(2, 130, 2, 5, 8) == 2 * 3 * (64 * 7 * 8 + 64 * 4 + 4)
    assert lib.mf_mean_response_grad_workspace_bytes(2, 130, 2, 5, 2) == 0
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    rc = _lib.call_rc("mf_mean_response_grad", dtype, 1, 1, 1, 1, ints((3,)), ints((0,)), p, None, 0, p, p, 1, ints((0,)), p, pf, None,
                      _lib.ptr(ws), 64, stream)
    assert rc == -18                                                               # (a workspace that is too small)
    torch.cuda.synchronize()
