"""PiecewiseKernel: the fused generator (``mf_sde_piecewise_transitions``) and its reverse mode (``mf_sde_piecewise_transitions_grad``)
against the reference's algorithm restated with the stationary entry points - ``searchsorted``, per segment a mask, a gather of the
segment's steps, ONE ``mf_sde_transitions`` (``_grad``) call with the segment's hyper-parameters, and a scatter back (the sum over
the steps for the reverse mode) - markovflow/kernels/piecewise_stationary.py:180-204.

Matern32 (d = 2) and Matern52 x HarmonicOscillator (d = 6), B = 64 series of T = 4096 time points (4095 transitions), K in {1, 15}
change points evenly spread over the series' span of 400 time units (K + 1 segments of equal length, gaps of 0.05 ... 0.15), shared
hyper-parameters, float64 and float32.
Both sides write (A, chol Q) into preallocated [B, T-1, d, d] tensors; the reverse mode takes dense g_A, g_cholQ and ends at the
[nseg, ncomp, 3] gradient.  The restated side needs the number of steps per segment on the host (one ``nonzero`` per segment: the
``dynamic_partition`` of the reference); its indices are computed inside the timed region, as the fused side's lookup is.

The variants alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the medians
(and minima) of the per-call window times are printed, then one JSON line.  Before timing, the two sides are compared.
Usage: python3 scripts/bench_piecewise.py [--rounds R] [--window K]"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from markovflow_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--window", type=int, default=10)
args = ap.parse_args()
dev = torch.device("cuda:0")
rounds, window = args.rounds, args.window
BSZ, T, JITTER, SPAN = 64, 4096, 1e-6, 400.0
KERNELS = {"Matern32": ((3,), (0,), 2), "Matern52xHO": ((5,), (1,), 6)}


def timed(fn):
    """Per-call time of a window of calls between two device events, in ms."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(window):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / window


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts)}


def alternate(*fns):
    out = [[] for _ in fns]
    for _ in range(2):                                  # warm-up windows
        for fn in fns:
            timed(fn)
    for _ in range(rounds):                             # alternating, one process
        for ts, fn in zip(out, fns):
            ts.append(timed(fn))
    return [stats(ts) for ts in out]


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def case(name, num_cp, dtype):
    orders, oscs, d = KERNELS[name]
    nseg, n, ncomp = num_cp + 1, T - 1, len(orders)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    gaps = 0.5 + torch.rand(BSZ, T, dtype=torch.float64, device=dev, generator=g)
    t = torch.cumsum(gaps, dim=-1)
    t = ((t - t[:, :1]) / (t[:, -1:] - t[:, :1]) * SPAN).to(dtype)               # every series spans [0, SPAN]: gaps of 0.05 ... 0.15
    cp = (torch.arange(1, nseg, dtype=torch.float64, device=dev) * (SPAN / nseg)).to(dtype)
    t_start, dt = t[:, :-1].contiguous(), (t[:, 1:] - t[:, :-1]).contiguous()
    ls = 0.3 + 0.1 * torch.arange(nseg, dtype=torch.float64, device=dev)
    lam = (math.sqrt(orders[0]) / ls).to(dtype).reshape(nseg, ncomp).contiguous()
    var = (0.5 + 0.05 * torch.arange(nseg, dtype=torch.float64, device=dev)).to(dtype).reshape(nseg, ncomp).contiguous()
    om = (2.0 * math.pi / (0.7 + 0.1 * torch.arange(nseg, dtype=torch.float64, device=dev))).to(dtype).reshape(nseg, ncomp).contiguous()
    c_orders, c_oscs, stream = ints(orders), ints(oscs), _lib.stream_ptr(dev)
    a_f, c_f = (torch.empty((BSZ, n, d, d), dtype=dtype, device=dev) for _ in range(2))
    a_r, c_r = (torch.empty((BSZ, n, d, d), dtype=dtype, device=dev) for _ in range(2))
    g_a = torch.randn((BSZ, n, d, d), dtype=dtype, device=dev, generator=g)
    g_c = torch.tril(torch.randn((BSZ, n, d, d), dtype=dtype, device=dev, generator=g))
    out_f = torch.empty((BSZ, nseg, ncomp, 3), dtype=dtype, device=dev)
    ws_bytes = int(_lib.load().mf_sde_piecewise_transitions_grad_workspace_bytes(BSZ, n, ncomp, dt.element_size()))
    ws = _lib.workspace(ws_bytes, dev)
    cp_ptr = _lib.ptr(cp) if num_cp else None

    def fused_forward():
        _lib.call("mf_sde_piecewise_transitions", dtype, BSZ, n, ncomp, c_orders, c_oscs, nseg, cp_ptr, _lib.ptr(lam), _lib.ptr(var),
                  _lib.ptr(om), 0, _lib.ptr(t_start), _lib.ptr(dt), JITTER, _lib.ptr(a_f), _lib.ptr(c_f), None, None, stream)

    def fused_backward():
        _lib.call("mf_sde_piecewise_transitions_grad", dtype, BSZ, n, ncomp, c_orders, c_oscs, nseg, cp_ptr, _lib.ptr(lam), _lib.ptr(var),
                  _lib.ptr(om), 0, _lib.ptr(t_start), _lib.ptr(dt), JITTER, _lib.ptr(g_a), _lib.ptr(g_c), _lib.ptr(out_f), _lib.ptr(ws),
                  ws_bytes, stream)
        return torch.sum(out_f, dim=0)

    def partition():
        seg = torch.searchsorted(cp, t_start, right=True).reshape(-1)
        return [torch.nonzero(seg == k)[:, 0] for k in range(nseg)]

    def restated_forward():
        dt_flat, a_flat, c_flat = dt.reshape(-1), a_r.view(-1, d, d), c_r.view(-1, d, d)
        for k, idx in enumerate(partition()):
            nk = int(idx.shape[0])
            if nk == 0:
                continue
            dt_k = dt_flat[idx]
            a_k, c_k = (torch.empty((nk, d, d), dtype=dtype, device=dev) for _ in range(2))
            _lib.call("mf_sde_transitions", dtype, 1, nk, ncomp, c_orders, c_oscs, _lib.ptr(lam[k]), _lib.ptr(var[k]), _lib.ptr(om[k]), 0,
                      _lib.ptr(dt_k), JITTER, _lib.ptr(a_k), _lib.ptr(c_k), None, stream)
            a_flat.index_copy_(0, idx, a_k)
            c_flat.index_copy_(0, idx, c_k)

    def restated_backward():
        dt_flat, ga_flat, gc_flat = dt.reshape(-1), g_a.view(-1, d, d), g_c.view(-1, d, d)
        rows = []
        for k, idx in enumerate(partition()):
            nk = int(idx.shape[0])
            if nk == 0:
                rows.append(torch.zeros((ncomp, 3), dtype=dtype, device=dev))
                continue
            dt_k, ga_k, gc_k = dt_flat[idx], ga_flat[idx], gc_flat[idx]
            part = torch.empty((1, nk, ncomp, 3), dtype=dtype, device=dev)
            _lib.call("mf_sde_transitions_grad", dtype, 1, nk, ncomp, c_orders, c_oscs, _lib.ptr(lam[k]), _lib.ptr(var[k]), _lib.ptr(om[k]),
                      0, _lib.ptr(dt_k), JITTER, _lib.ptr(ga_k), _lib.ptr(gc_k), _lib.ptr(part), stream)
            rows.append(torch.sum(part, dim=(0, 1)))
        return torch.stack(rows)

    # the two sides must agree before their times are compared
    fused_forward()
    restated_forward()
    torch.cuda.synchronize()
    fwd_diff = max(float((a_f - a_r).abs().max()), float((c_f - c_r).abs().max()))
    g_f, g_r = fused_backward(), restated_backward()
    bwd_rel = float((g_f - g_r).abs().max() / g_r.abs().max())
    assert fwd_diff <= (1e-12 if dtype == torch.float64 else 1e-5) * max(1.0, float(a_r.abs().max()), float(c_r.abs().max())), fwd_diff
    assert bwd_rel <= (1e-10 if dtype == torch.float64 else 1e-3), bwd_rel
    t_ff, t_rf = alternate(fused_forward, restated_forward)
    t_fb, t_rb = alternate(fused_backward, restated_backward)
    res = {"kernel": name, "d": d, "B": BSZ, "T": T, "K": num_cp, "dtype": str(dtype).replace("torch.", ""),
           "forward_fused_ms": t_ff, "forward_restated_ms": t_rf, "backward_fused_ms": t_fb, "backward_restated_ms": t_rb,
           "forward_max_abs_diff": fwd_diff, "backward_max_rel_diff": bwd_rel,
           "forward_output_GBps": 2 * BSZ * n * d * d * dt.element_size() / t_ff["median"] / 1e6}
    print(f"{name:12s} K={num_cp:2d} {res['dtype']:8s} forward fused {t_ff['median']:.3f} ms (min {t_ff['min']:.3f}), restated "
          f"{t_rf['median']:.3f} ms (min {t_rf['min']:.3f});  backward fused {t_fb['median']:.3f} ms (min {t_fb['min']:.3f}), restated "
          f"{t_rb['median']:.3f} ms (min {t_rb['min']:.3f})", flush=True)
    return res


results = [case(name, k, dtype) for name in KERNELS for k in (1, 15) for dtype in (torch.float64, torch.float32)]
print(json.dumps({"cases": results, "rounds": rounds, "window": window}))
