"""
GPU tests of the kernel -> state space model generators (csrc/mf_sde.hip) and their reverse modes at EVERY time gap, in float32 and
float64, through the raw C ABI, against an exact reference (tests/helpers/generator_exact.py: mpmath at 80 digits) under bounds that
come from the CPU alone (tests/helpers/generator_fp_cases.py has the rule and the metrics, tests/helpers/generator_fp_table.py the
committed yardsticks): per step and tensor, error <= FP32_FACTOR x yardstick.

Shape: B = 3 series of n = 45 steps - 135 (series, step) pairs: two full 64-lane blocks and a tail of 7, one block straddling a
series boundary - with the 13 gaps of the grid (0, 2^-24 .. 2^-1, 3, 40, 1e10) tiled along n in a shuffled order that is rotated
from series to series.  Hyper-parameters and weights are the yardsticks' own draws (series b: draw b; shared: draw 0; a kind that
occurs twice in a signature: the next draw), the weights of step k scaled by 2^((k mod 3) - 1), which is exact, so that no two
steps of a series carry the same incoming gradient.  The entries of the incoming gradients that the kernels must not read (outside
the diagonal blocks, above the diagonal of g_cholQ) hold 3 and 5.

Every test prints its largest error-to-yardstick ratio per tensor and the gap it occurred at (``-s``).  Measured on an MI355X: 1.00
for every generator entry point in both precisions (the kernels reproduce the CPU evaluation of their statements up to the nudged
exp / sin / cos), 0.70 / 0.58 for the piecewise sums, 0.49 / 0.63 for the fused / materialised GPR log-likelihood.

That the assertions can fail was checked on the CPU with the numpy evaluation standing in for the kernels: the rotation transposed
puts A at about 5e15 x (float64) and 7e6 x (float32) its yardstick, a Dual square root whose tangent is off by 1e-3 puts the
gradients at about 5e12 x and 6e3 - 9e3 x; exp, sin and cos three ulp off stay within the factor (2 - 3.5 x).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from markovflow_amd import _lib
from helpers import generator_exact as E
from helpers import generator_fp_cases as C
from helpers import generator_fp_table as TABLE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 64, -77.25
B, N = 3, 45
TORCH = {"f32": torch.float32, "f64": torch.float64}
DT_NAMES = ["f64", "f32"]
SHARING = [False, True]
_ORDER = np.random.default_rng(C.DEFAULT_SEED).permutation(len(C.GAPS))
GAP_IDX = np.array([[_ORDER[(k + 4 * b) % len(C.GAPS)] for k in range(N)] for b in range(B)])
DT = np.array(C.GAPS)[GAP_IDX]
POW2 = 2.0 ** ((np.arange(N) % 3) - 1)

SIGNATURES = {
    "m12": [(1, 0)], "m32": [(3, 0)], "m52": [(5, 0)], "m52_m32_m12": [(5, 0), (3, 0), (1, 0)],
    "const": [(0, 0)],
    "m12xho_osc1": [(1, 1)], "m32xho_osc1": [(3, 1)], "m52xho_osc1": [(5, 1)],
    "m12xho_osc2": [(1, 2)], "m32xho_osc2": [(3, 2)], "m52xho_osc2": [(5, 2)],
    "mixed16": [(5, 1), (3, 2), (3, 1), (1, 0), (0, 0)],
}
MATERN_ONLY = ["m12", "m32", "m52", "m52_m32_m12"]
PIECEWISE = ["m32", "m52xho_osc1", "mixed16"]
CHANGE_POINTS = [1.0, 2.0, 3.0]


def tt(x, dt_name):
    return torch.tensor(np.ascontiguousarray(x), dtype=TORCH[dt_name], device=DEV)


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def guarded(shape, dt_name):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=TORCH[dt_name], device=DEV)
    return buf, buf[:n].view(shape)


def guards_intact(*bufs):
    return all(bool(torch.all(b[-GUARD:] == SENTINEL)) for b in bufs)


def stream():
    return _lib.stream_ptr(torch.device(DEV))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
class Case:
    """One signature's inputs: ``draw_idx`` [B, N, ncomp] (the yardstick draw behind every (series, step, component)), the
    hyper-parameter arrays ``lam`` / ``var`` / ``omega`` ([ncomp] or [B, ncomp]; piecewise: [nseg, ncomp] or [B, nseg, ncomp]),
    the incoming gradients ``g_a`` / ``g_c`` [B, N, d, d] and, piecewise, start times and segments."""

    def __init__(self, sig, per_series, dt_name, nseg=None, empty=0):
        """``nseg``: segments that get steps (None: not piecewise); ``empty``: further segments behind them that get none and
        carry the hyper-parameters of segment 0."""
        self.comps, self.per_series, self.dt_name, self.nseg = SIGNATURES[sig], per_series, dt_name, nseg
        self.total = (nseg or 1) + empty
        self.change_points = CHANGE_POINTS[:self.total - 1]
        self.sizes = [E.size(o, r) for o, r in self.comps]
        self.offs = [int(x) for x in np.cumsum([0] + self.sizes[:-1])]
        self.d, self.ncomp = sum(self.sizes), len(self.comps)
        occurrence = [self.comps[:c].count(kind) for c, kind in enumerate(self.comps)]
        segs = nseg or 1
        self.seg = np.zeros((B, N), dtype=np.int64)
        self.t_start = None
        if nseg:
            # starts spread over the segments; the step of gap 1e10 starts at -1e10 (segment 0)
            self.seg = (np.arange(N)[None, :] + np.arange(B)[:, None]) % nseg
            self.t_start = np.where(DT == 1e10, -1e10, 0.25 + self.seg.astype(np.float64))
            self.seg = np.where(DT == 1e10, 0, self.seg)
        # draw of (series, segment, component)
        table = np.array([[[((b if per_series else 0) + s + occurrence[c]) % 3 for c in range(self.ncomp)] for s in range(segs)]
                          for b in range(B)])
        self.draw_idx = table[np.arange(B)[:, None], self.seg]                       # [B, N, ncomp]

        def hyper(name):
            a = np.array([[[C.draw(int(table[b, s if s < segs else 0, c]), dt_name, *self.comps[c])[name] for c in range(self.ncomp)]
                           for s in range(self.total)] for b in range(B)])
            a = a if nseg else a[:, 0]
            return a if per_series else a[0]
        self.lam, self.var, self.omega = hyper("lam"), hyper("var"), hyper("omega")
        self.g_a, self.g_c = np.full((B, N, self.d, self.d), 3.0), np.full((B, N, self.d, self.d), 5.0)
        for b in range(B):
            for k in range(N):
                for c, (off, size) in enumerate(zip(self.offs, self.sizes)):
                    dr = C.draw(int(self.draw_idx[b, k, c]), dt_name, *self.comps[c])
                    sl = slice(off, off + size)
                    self.g_a[b, k, sl, sl] = dr["w_a"] * POW2[k]
                    self.g_c[b, k, sl, sl] = np.where(np.tri(size, dtype=bool), dr["w_c"] * POW2[k], 5.0)

    def exact(self, b, k, c):
        return C.exact_step(self.dt_name, *self.comps[c], int(self.draw_idx[b, k, c]), float(DT[b, k]))

    def yard(self, b, k, c):
        return TABLE.GENERATOR[(self.dt_name,) + self.comps[c] + (float(DT[b, k]),)]

    def block_mask(self):
        mask = np.zeros((self.d, self.d), dtype=bool)
        for off, size in zip(self.offs, self.sizes):
            mask[off:off + size, off:off + size] = True
        return mask


# ---- the entry points --------------------------------------------------------------------------------------------------------------------
def forward(entry, case, jitter, dt=DT):
    """{"A", "cholQ", "Q"}: device tensors [B, N, d, d] of mf_sde_matern_transitions / mf_sde_transitions /
    mf_sde_piecewise_transitions."""
    dn = case.dt_name
    bufs = [guarded((B, N, case.d, case.d), dn) for _ in range(3)]
    lam, var, om, dt_d = tt(case.lam, dn), tt(case.var, dn), tt(case.omega, dn), tt(dt, dn)
    orders, osc = ints([o for o, _ in case.comps]), ints([r for _, r in case.comps])
    outs = [_lib.ptr(v) for _, v in bufs]
    if entry == "mf_sde_matern_transitions":
        _lib.call(entry, TORCH[dn], B, N, case.ncomp, orders, _lib.ptr(lam), _lib.ptr(var), int(case.per_series), _lib.ptr(dt_d),
                  jitter, *outs, stream())
    elif entry == "mf_sde_transitions":
        _lib.call(entry, TORCH[dn], B, N, case.ncomp, orders, osc, _lib.ptr(lam), _lib.ptr(var), _lib.ptr(om), int(case.per_series),
                  _lib.ptr(dt_d), jitter, *outs, stream())
    else:
        nseg = case.total
        cp = tt(case.change_points, dn) if nseg > 1 else None
        ts = tt(case.t_start if case.t_start is not None else np.zeros((B, N)), dn)
        shape = (B, nseg, case.ncomp) if case.per_series else (nseg, case.ncomp)
        lam, var, om = (x.reshape(shape).contiguous() for x in (lam, var, om))
        seg_buf = torch.full((B * N + GUARD,), -77, dtype=torch.int32, device=DEV)
        _lib.call(entry, TORCH[dn], B, N, case.ncomp, orders, osc, nseg, _lib.ptr(cp), _lib.ptr(lam), _lib.ptr(var), _lib.ptr(om),
                  int(case.per_series), _lib.ptr(ts), _lib.ptr(dt_d), jitter, *outs, _lib.ptr(seg_buf[:B * N]), stream())
        torch.cuda.synchronize()
        assert bool(torch.all(seg_buf[-GUARD:] == -77))
        np.testing.assert_array_equal(seg_buf[:B * N].view(B, N).cpu().numpy(), case.seg)
    torch.cuda.synchronize()
    assert guards_intact(*[b for b, _ in bufs]), "a write past the end of an output"
    return dict(zip(("A", "cholQ", "Q"), [v for _, v in bufs]))


def nn(x):
    return x.cpu().numpy().astype(np.float64)


def same_bits(x, y):
    """torch.equal on the bit patterns: chol Q at jitter 0 holds NaN where Q lost positive definiteness."""
    as_int = torch.int64 if x.dtype == torch.float64 else torch.int32
    return torch.equal(x.view(as_int), y.view(as_int))


class Worst:
    """The largest error-to-yardstick ratio per tensor, where it occurred, and every miss of the bound."""

    def __init__(self, what):
        self.what, self.ratio, self.misses = what, {}, []

    def add(self, name, err, yard, where):
        ratio = err / yard
        if ratio > self.ratio.get(name, (-1.0, None))[0]:
            self.ratio[name] = (ratio, where)
        if not err <= C.FP32_FACTOR * yard:
            self.misses.append((name, where, err, yard))

    def finish(self):
        for name, (ratio, where) in self.ratio.items():
            print(f"  RATIO {self.what} {name}: {ratio:.3g} at gap {where[0]:.3g} "
                  f"(series {where[1]}, step {where[2]}, component {where[3]})")
        assert not self.misses, (self.what, self.misses[:8], len(self.misses))


def check_forward(what, case, a=None, q0=None, q=None, low=None):
    worst = Worst(f"{what} {case.dt_name}")
    mask = case.block_mask()
    for x in (a, q0, q, low):
        if x is not None:
            assert np.all(x[..., ~mask] == 0), "entries outside the diagonal blocks must be exact zeros"
    for x in (q0, q):
        if x is not None:
            assert np.array_equal(x, np.swapaxes(x, -1, -2)), "Q must be exactly symmetric"
    if low is not None:
        assert np.all(np.triu(low, 1) == 0), "the upper triangle of chol Q must be exactly zero"
    for b in range(B):
        for k in range(N):
            for c, (off, size) in enumerate(zip(case.offs, case.sizes)):
                sl = slice(off, off + size)
                got = [None if x is None else x[b, k, sl, sl] for x in (a, q0, q, low)]
                for name, err in C.forward_errors(case.exact(b, k, c), *got).items():
                    worst.add(name, err, case.yard(b, k, c)[name], (float(DT[b, k]), b, k, c))
    worst.finish()


def check_long_and_zero_gaps(case, at_jitter, at_zero):
    """dt = 1e10: nothing is NaN, A is within the bound of 0 (a constant factor's A stays 1).  dt = 0 at jitter 0: A = I, Q = 0 and
    chol Q = 0 exactly."""
    for x in at_jitter.values():
        assert np.all(np.isfinite(x))
    long_gap, zero_gap = DT == 1e10, DT == 0.0
    assert long_gap.any() and zero_gap.any()
    a = at_jitter["A"][long_gap]
    for c, (off, size) in enumerate(zip(case.offs, case.sizes)):
        order, osc = case.comps[c]
        if order:
            yard = TABLE.GENERATOR[(case.dt_name, order, osc, 1e10)]["A"]
            assert np.max(np.abs(a[:, off:off + size, off:off + size])) <= C.FP32_FACTOR * yard
    assert np.all(at_zero["A"][zero_gap] == np.eye(case.d))
    assert np.all(at_zero["Q"][zero_gap] == 0) and np.all(at_zero["cholQ"][zero_gap] == 0)


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("per_series", SHARING, ids=["shared", "per-series"])
@pytest.mark.parametrize("sig", sorted(SIGNATURES))
def test_forward_at_every_gap(sig, per_series, dt_name):
    """mf_sde_transitions (and, for Matern-only signatures, mf_sde_matern_transitions): A, Q at jitter 0 and at the jitter, chol Q at
    the jitter, per step; the exact values at dt = 0; the bit-identity the header promises between the entry points."""
    case = Case(sig, per_series, dt_name)
    jit = C.JITTER[dt_name]
    entries = ["mf_sde_transitions"] + (["mf_sde_matern_transitions"] if sig in MATERN_ONLY else [])
    results = {}
    for entry in entries:
        at_jitter, at_zero = forward(entry, case, jit), forward(entry, case, 0.0)
        results[entry] = (at_jitter, at_zero)
        hj, h0 = {k: nn(v) for k, v in at_jitter.items()}, {k: nn(v) for k, v in at_zero.items()}
        check_forward(entry, case, a=hj["A"], q0=h0["Q"], q=hj["Q"], low=hj["cholQ"])
        assert np.array_equal(hj["A"], h0["A"])
        check_long_and_zero_gaps(case, hj, h0)
    single = forward("mf_sde_piecewise_transitions", case, jit)
    for k in ("A", "cholQ", "Q"):
        assert torch.equal(single[k], results["mf_sde_transitions"][0][k]), f"nseg = 1 must give mf_sde_transitions bit for bit ({k})"
        if len(entries) == 2:
            general, matern = (results[e] for e in entries)
            assert torch.equal(general[0][k], matern[0][k]), f"without an oscillator the two generators must agree bit for bit ({k})"
            assert same_bits(general[1][k], matern[1][k]), f"... and at jitter 0 ({k})"


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("per_series", SHARING, ids=["shared", "per-series"])
@pytest.mark.parametrize("sig", PIECEWISE)
def test_piecewise_forward_at_every_gap(sig, per_series, dt_name):
    """nseg = 3, starts spread over the segments, the step of gap 1e10 out of -1e10: the reference of every step is the exact
    component with ITS segment's hyper-parameters."""
    case = Case(sig, per_series, dt_name, nseg=3)
    assert set(case.seg.ravel()) == {0, 1, 2}
    at_jitter = {k: nn(v) for k, v in forward("mf_sde_piecewise_transitions", case, C.JITTER[dt_name]).items()}
    at_zero = {k: nn(v) for k, v in forward("mf_sde_piecewise_transitions", case, 0.0).items()}
    check_forward("mf_sde_piecewise_transitions", case, a=at_jitter["A"], q0=at_zero["Q"], q=at_jitter["Q"], low=at_jitter["cholQ"])
    check_long_and_zero_gaps(case, at_jitter, at_zero)


# ---- reverse -----------------------------------------------------------------------------------------------------------------------------
def packed_record(case):
    """The packed incoming gradients of mf_sde_matern_transitions_grad_packed: per transition the K x K blocks of g_A of every
    component, padded to 16 bytes, then the lower triangles (row-major) of the blocks of g_cholQ, padded to 16 bytes."""
    per = 16 // (8 if case.dt_name == "f64" else 4)
    ra, rc = sum(s * s for s in case.sizes), sum(s * (s + 1) // 2 for s in case.sizes)
    pa, pc = -(-ra // per) * per, -(-rc // per) * per
    rec = np.full((B, N, pa + pc), 7.0)
    ia, ic = 0, pa
    for off, size in zip(case.offs, case.sizes):
        rec[..., ia:ia + size * size] = case.g_a[..., off:off + size, off:off + size].reshape(B, N, -1)
        ia += size * size
        for i in range(size):
            rec[..., ic:ic + i + 1] = case.g_c[..., off + i, off:off + i + 1]
            ic += i + 1
    return rec


def reverse(entry, case, jitter, g_a, g_c, dt=DT):
    """out of a reverse mode as a device tensor: [B, N, ncomp, 2] (Matern), [B, N, ncomp, 3] (general), [B, nseg, ncomp, 3]."""
    dn = case.dt_name
    lam, var, om, dt_d = tt(case.lam, dn), tt(case.var, dn), tt(case.omega, dn), tt(dt, dn)
    orders, osc = ints([o for o, _ in case.comps]), ints([r for _, r in case.comps])
    ga_d, gc_d = (None if g is None else tt(g, dn) for g in (g_a, g_c))
    if entry == "mf_sde_matern_transitions_grad":
        buf, out = guarded((B, N, case.ncomp, 2), dn)
        _lib.call(entry, TORCH[dn], B, N, case.ncomp, orders, _lib.ptr(lam), _lib.ptr(var), int(case.per_series), _lib.ptr(dt_d),
                  jitter, _lib.ptr(ga_d), _lib.ptr(gc_d), _lib.ptr(out), stream())
    elif entry == "mf_sde_matern_transitions_grad_packed":
        buf, out = guarded((B, N, case.ncomp, 2), dn)
        _lib.call(entry, TORCH[dn], B, N, case.ncomp, orders, _lib.ptr(lam), _lib.ptr(var), int(case.per_series), _lib.ptr(dt_d),
                  jitter, _lib.ptr(ga_d), _lib.ptr(out), stream())
    elif entry == "mf_sde_transitions_grad":
        buf, out = guarded((B, N, case.ncomp, 3), dn)
        _lib.call(entry, TORCH[dn], B, N, case.ncomp, orders, osc, _lib.ptr(lam), _lib.ptr(var), _lib.ptr(om), int(case.per_series),
                  _lib.ptr(dt_d), jitter, _lib.ptr(ga_d), _lib.ptr(gc_d), _lib.ptr(out), stream())
    else:
        nseg = case.total
        buf, out = guarded((B, nseg, case.ncomp, 3), dn)
        cp, ts = tt(case.change_points, dn), tt(case.t_start, dn)
        shape = (B, nseg, case.ncomp) if case.per_series else (nseg, case.ncomp)
        lam, var, om = (x.reshape(shape).contiguous() for x in (lam, var, om))
        ws_bytes = int(_lib.load().mf_sde_piecewise_transitions_grad_workspace_bytes(B, N, case.ncomp, 8 if dn == "f64" else 4))
        ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
        _lib.call(entry, TORCH[dn], B, N, case.ncomp, orders, osc, nseg, _lib.ptr(cp), _lib.ptr(lam), _lib.ptr(var), _lib.ptr(om),
                  int(case.per_series), _lib.ptr(ts), _lib.ptr(dt_d), jitter, _lib.ptr(ga_d), _lib.ptr(gc_d), _lib.ptr(out), _lib.ptr(ws),
                  ws_bytes, stream())
        torch.cuda.synchronize()
        assert bool(torch.all(ws[-GUARD:] == 0x5A)), "a write past the end of the workspace"
    torch.cuda.synchronize()
    assert guards_intact(buf), "a write past the end of the output"
    return out.clone()


def check_per_step(what, case, which, out):
    """out [B, N, ncomp, 2 or 3] of a per-step reverse mode against mp.diff, slot by slot."""
    worst = Worst(f"{what} {case.dt_name}")
    slots = out.shape[-1]
    for b in range(B):
        for k in range(N):
            for c, (order, osc) in enumerate(case.comps):
                got = np.zeros(3)
                got[:slots] = out[b, k, c] / POW2[k]
                for name, err in C.grad_errors(case.exact(b, k, c), which, got).items():
                    if slots == 2 and name.endswith("omega"):
                        continue
                    worst.add(name, err, case.yard(b, k, c)[name], (float(DT[b, k]), b, k, c))
    worst.finish()


def check_structural_zeros(case, out):
    for c, (order, osc) in enumerate(case.comps):
        if order == 0:
            assert np.all(out[..., c, 0] == 0), "d/dlam of an order-0 component must be an exact zero"
        if not osc and out.shape[-1] == 3:
            assert np.all(out[..., c, 2] == 0), "d/domega without an oscillator must be an exact zero"


def check_zero_gap_contributes_nothing(entry, case, packed=False):
    """jitter 0: a step of dt = 0 has Q = 0, the factor passes through as zero and A = I does not depend on anything."""
    g_a = packed_record(case) if packed else case.g_a
    out = nn(reverse(entry, case, 0.0, g_a, None if packed else case.g_c))
    assert (DT == 0.0).any() and np.all(out[DT == 0.0] == 0)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("per_series", SHARING, ids=["shared", "per-series"])
@pytest.mark.parametrize("sig", MATERN_ONLY)
def test_matern_reverse_at_every_gap(sig, per_series, dt_name):
    """mf_sde_matern_transitions_grad with both, with one and with the other incoming gradient, and _grad_packed fed the packed
    record of the same gradients."""
    case = Case(sig, per_series, dt_name)
    jit = C.JITTER[dt_name]
    entry = "mf_sde_matern_transitions_grad"
    both = reverse(entry, case, jit, case.g_a, case.g_c)
    check_per_step(entry, case, "g", nn(both))
    check_per_step(entry + " (g_A alone)", case, "gA", nn(reverse(entry, case, jit, case.g_a, None)))
    check_per_step(entry + " (g_cholQ alone)", case, "gC", nn(reverse(entry, case, jit, None, case.g_c)))
    assert torch.equal(both, reverse(entry, case, jit, case.g_a, case.g_c)), "two calls must agree bit for bit"
    packed = reverse(entry + "_packed", case, jit, packed_record(case), None)
    check_per_step(entry + "_packed", case, "g", nn(packed))
    assert torch.equal(packed, both), "the packed record holds the same numbers: the same result, bit for bit"
    check_zero_gap_contributes_nothing(entry, case)
    check_zero_gap_contributes_nothing(entry + "_packed", case, packed=True)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("per_series", SHARING, ids=["shared", "per-series"])
@pytest.mark.parametrize("sig", sorted(SIGNATURES))
def test_general_reverse_at_every_gap(sig, per_series, dt_name):
    case = Case(sig, per_series, dt_name)
    jit = C.JITTER[dt_name]
    entry = "mf_sde_transitions_grad"
    both = reverse(entry, case, jit, case.g_a, case.g_c)
    check_structural_zeros(case, nn(both))
    check_per_step(entry, case, "g", nn(both))
    check_per_step(entry + " (g_A alone)", case, "gA", nn(reverse(entry, case, jit, case.g_a, None)))
    only_c = nn(reverse(entry, case, jit, None, case.g_c))
    check_structural_zeros(case, only_c)
    check_per_step(entry + " (g_cholQ alone)", case, "gC", only_c)
    assert torch.equal(both, reverse(entry, case, jit, case.g_a, case.g_c)), "two calls must agree bit for bit"
    check_zero_gap_contributes_nothing(entry, case)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("per_series", SHARING, ids=["shared", "per-series"])
@pytest.mark.parametrize("sig", PIECEWISE)
def test_piecewise_reverse_at_every_gap(sig, per_series, dt_name):
    """out [B, nseg, ncomp, 3]: the exact per-step terms are summed per (series, segment) in mpmath; the bound of a sum is the sum of
    its steps' bounds (FP32_FACTOR x yardstick x S of the step)."""
    import mpmath as mp
    case = Case(sig, per_series, dt_name, nseg=3, empty=1)          # change points 1, 2, 3: segment 3 gets no step
    jit = C.JITTER[dt_name]
    entry = "mf_sde_piecewise_transitions_grad"
    outs = {which: reverse(entry, case, jit, g_a, g_c)
            for which, (g_a, g_c) in {"g": (case.g_a, case.g_c), "gA": (case.g_a, None), "gC": (None, case.g_c)}.items()}
    again = reverse(entry, case, jit, case.g_a, case.g_c)
    all_zero_gaps = nn(reverse(entry, case, 0.0, case.g_a, case.g_c, dt=np.zeros((B, N))))
    assert torch.equal(outs["g"], again), "two calls must agree bit for bit"
    assert np.all(all_zero_gaps == 0), "steps of dt = 0 at jitter 0 contribute exact zeros"
    worst = Worst(f"{entry} {dt_name}")
    for which, out in outs.items():
        out = nn(out)
        check_structural_zeros(case, out)
        assert np.all(out[:, 3] == 0), "a segment without a step must get exact zeros"
        for b in range(B):
            for s in range(3):
                steps = np.flatnonzero(case.seg[b] == s)
                for c in range(case.ncomp):
                    with mp.workdps(E.DPS):
                        total, allowed = [mp.mpf(0)] * 3, np.zeros(3)
                        for k in steps:
                            ex, yard = case.exact(b, k, c), case.yard(b, k, c)
                            for j, p in enumerate(C.PARAMS):
                                total[j] += ex[which + "_mp"][j] * mp.mpf(float(POW2[k]))
                                if f"{which}_{p}" in yard:
                                    allowed[j] += yard[f"{which}_{p}"] * ex[which][1][j] * POW2[k]
                    err = E.error(out[b, s, c], total)
                    for j, p in enumerate(C.PARAMS):
                        if f"{which}_{p}" not in C.GRAD_NAMES:
                            continue
                        if allowed[j] == 0:
                            assert err[j] == 0, (which, p, b, s, c, err[j])
                            continue
                        worst.add(f"{which}_{p}", err[j], allowed[j], (float("nan"), b, s, c))
    worst.finish()


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("per_series", SHARING, ids=["shared", "per-series"])
@pytest.mark.parametrize("sig", MATERN_ONLY)
def test_prior_factor_reverse(sig, per_series, dt_name):
    """mf_sde_matern_prior_chol_grad on 67 series (a full block and a tail): d/d(lam, var) of <g, tril chol(Pinf + jitter I)>."""
    comps = SIGNATURES[sig]
    bsz = 67
    sizes = [E.size(o, 0) for o, _ in comps]
    offs = [int(x) for x in np.cumsum([0] + sizes[:-1])]
    d = sum(sizes)
    idx = np.array([[((b if per_series else 0) + c) % 3 for c in range(len(comps))] for b in range(bsz)])
    scale = 2.0 ** ((np.arange(bsz) % 3) - 1)
    g = np.full((bsz, d, d), 5.0)
    for b in range(bsz):
        for c, (off, size) in enumerate(zip(offs, sizes)):
            w_c = C.draw(int(idx[b, c]), dt_name, comps[c][0], 0)["w_c"]
            g[b, off:off + size, off:off + size] = np.where(np.tri(size, dtype=bool), w_c * scale[b], 5.0)

    def hyper(name):
        a = np.array([[C.draw(int(idx[b, c]), dt_name, comps[c][0], 0)[name] for c in range(len(comps))] for b in range(bsz)])
        return a if per_series else a[0]
    lam, var, g_d = tt(hyper("lam"), dt_name), tt(hyper("var"), dt_name), tt(g, dt_name)
    outs = []
    for _ in range(2):
        buf, out = guarded((bsz, len(comps), 2), dt_name)
        _lib.call("mf_sde_matern_prior_chol_grad", TORCH[dt_name], bsz, len(comps), ints([o for o, _ in comps]), _lib.ptr(lam),
                  _lib.ptr(var), int(per_series), C.JITTER[dt_name], _lib.ptr(g_d), _lib.ptr(out), stream())
        torch.cuda.synchronize()
        assert guards_intact(buf)
        outs.append(out.clone())
    assert torch.equal(*outs), "two calls must agree bit for bit"
    got = nn(outs[0])
    worst = Worst(f"mf_sde_matern_prior_chol_grad {dt_name}")
    for b in range(bsz):
        for c, (order, _) in enumerate(comps):
            errs = C.prior_errors(C.exact_prior(dt_name, order, int(idx[b, c])), got[b, c] / scale[b])
            for name, err in errs.items():
                worst.add(name, err, TABLE.PRIOR[(dt_name, order)][name], (float("nan"), b, 0, c))
    worst.finish()


# ---- the fused GPR log-likelihood, float64 ---------------------------------------------------------------------------------------------
def gpr_const(g):
    n = len(g["t"])
    return -0.5 * n * g["m"] * math.log(2.0 * math.pi) + 0.5 * n * g["m"] * math.log(1.0 / g["noise"])


def fused_loglik(sig, i, chunks):
    kind, orders = sig
    g = C.gpr_draw(i, sig)
    n, d = len(g["t"]), sum(E.matern_size(o) for o in orders)
    lam, var, t, y = tt(g["lam"], "f64"), tt(g["var"], "f64"), tt(g["t"][None], "f64"), tt(g["y"][None], "f64")
    y1, rinv = y[..., 0].contiguous(), tt(np.eye(g["m"]) / g["noise"], "f64")          # (named: an input must outlive the launch)
    rinv1 = rinv.reshape(-1)[:1].contiguous()
    lib = _lib.load()
    wsb = int(lib.mf_kf_loglik_workspace_bytes(1, n, d, 8, chunks))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    buf, out = guarded((1,), "f64")
    info = _lib.new_info(torch.device(DEV))
    head = (1, n, len(orders), ints(list(orders)), _lib.ptr(lam), _lib.ptr(var), 0, _lib.ptr(t))
    tail = (C.JITTER["f64"], gpr_const(g), _lib.ptr(out), _lib.ptr(ws), wsb, _lib.ptr(info), chunks, None, None, stream())
    if kind == "multi":
        _lib.call("mf_gpr_matern_multi_loglik", torch.float64, *head, _lib.ptr(y), g["m"], _lib.ptr(rinv), *tail)
    else:
        _lib.call("mf_gpr_matern_loglik", torch.float64, *head, _lib.ptr(y1), _lib.ptr(rinv1), *tail)
    torch.cuda.synchronize()
    assert guards_intact(buf) and int(info.item()) == 0
    return float(out.item())


def materialised_loglik(sig, i, chunks):
    """mf_sde_matern_transitions + mf_kf_loglik on the same inputs (chol P0 = numpy's Cholesky of Pinf + jitter I)."""
    kind, orders = sig
    g = C.gpr_draw(i, sig)
    mu0, chol_p0, _, b_s, _, h, y, r_inv = C.gpr_materialised(i, sig)
    n, d, m = len(g["t"]), len(mu0), g["m"]
    lam, var, dt = tt(g["lam"], "f64"), tt(g["var"], "f64"), tt(g["gaps"][None], "f64")
    a_s, chol_q = (torch.empty((1, n - 1, d, d), dtype=torch.float64, device=DEV) for _ in range(2))
    _lib.call("mf_sde_matern_transitions", torch.float64, 1, n - 1, len(orders), ints(list(orders)), _lib.ptr(lam), _lib.ptr(var), 0,
              _lib.ptr(dt), C.JITTER["f64"], _lib.ptr(a_s), _lib.ptr(chol_q), None, stream())
    lib = _lib.load()
    wsb = int(lib.mf_kf_loglik_workspace_bytes(1, n, d, 8, chunks))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    info = _lib.new_info(torch.device(DEV))
    ins = [tt(x[None], "f64") for x in (mu0, chol_p0)] + [a_s, tt(b_s[None], "f64"), chol_q, tt(h[None], "f64"), tt(y[None], "f64"),
                                                           tt(r_inv, "f64")]
    _lib.call("mf_kf_loglik", torch.float64, 1, n, d, m, *[_lib.ptr(x) for x in ins], 0, gpr_const(g), _lib.ptr(out), _lib.ptr(ws), wsb,
              _lib.ptr(info), chunks, None, None, stream())
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    return float(out.item())


@pytest.mark.parametrize("chunks", C.GPR_CHUNKS)
@pytest.mark.parametrize("sig", C.GPR_SIGNATURES, ids=lambda s: s[0] + "-" + "".join(str(o) for o in s[1]))
def test_fused_gpr_loglik_against_the_exact_log_density(sig, chunks):
    """The register route ((5), (3,3), (5,5)), the row route ((5,5,5), d = 9; single- and multi-output) and the materialised route,
    each against the exact Gaussian log density of the chain (mpmath), time gaps 2^-24 .. 40, jitter 1e-10.  Float32 is out of
    scope: no same-precision CPU evaluation of the filter exists to measure it against."""
    yard = TABLE.GPR[sig]
    for route, fn in (("fused", fused_loglik), ("materialised", materialised_loglik)):
        worst = Worst(f"gpr {route} {sig} chunks={chunks} f64")
        for i in range(3):
            value = fn(sig, i, chunks)
            worst.add("loglik", C.gpr_error(value, i, sig), yard, (float("nan"), i, 0, 0))
        worst.finish()
