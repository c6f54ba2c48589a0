"""LatentExponentiallyGenerated: the fused generator (``mf_sde_leg_transitions``) and its reverse mode (``mf_sde_leg_transitions_grad``,
through ``kernels._LegTransitions``) against the torch restatement (``torch.linalg.matrix_exp``, ``I − A Aᵀ``, a batched Cholesky and
their autograd: ``LatentExponentiallyGenerated._torch_transitions``).

B = 64 series of T = 4096 time points (4095 transitions, gaps of 0.05 ... 0.15), d in {2, 6, 12}, a shared feedback matrix, float64
and float32.  Forward: ``(A, chol Q)``; backward: forward plus the gradient of ``<g_A, A> + <g_C, chol Q>`` onto ``N`` and ``R``.

The variants alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the
medians (and minima) of the per-call window times are printed, then one JSON line.  Before timing, the two sides are compared.
Usage: python3 scripts/bench_leg.py [--rounds R] [--window K]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from markovflow_amd import kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--window", type=int, default=4)
args = ap.parse_args()
dev = torch.device("cuda:0")
rounds, window = args.rounds, args.window
BSZ, T, JITTER = 64, 4096, 1e-6


def timed(fn):
    """Per-call time of a window of calls between two device events, in ms."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(window):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / window


def alternate(*fns):
    out = [[] for _ in fns]
    for _ in range(2):                                  # warm-up windows
        for fn in fns:
            timed(fn)
    for _ in range(rounds):                             # alternating, one process
        for ts, fn in zip(out, fns):
            ts.append(timed(fn))
    return [{"median": statistics.median(ts), "min": min(ts)} for ts in out]


results = []
for dtype in (torch.float64, torch.float32):
    for d in (2, 6, 12):
        gen = torch.Generator().manual_seed(d)
        n_mat = (torch.eye(d, dtype=torch.float64) + 0.3 * torch.randn((d, d), generator=gen, dtype=torch.float64)).to(dev, dtype)
        r_mat = torch.randn((d, d), generator=gen, dtype=torch.float64).to(dev, dtype)
        dt = (0.05 + 0.1 * torch.rand((BSZ, T - 1), generator=gen, dtype=torch.float64)).to(dev, dtype)
        g_a = torch.randn((BSZ, T - 1, d, d), generator=gen, dtype=torch.float64).to(dev, dtype)
        g_c = torch.randn((BSZ, T - 1, d, d), generator=gen, dtype=torch.float64).to(dev, dtype).tril()

        def forward(route, n_t=n_mat, r_t=r_mat):
            kern = K.LatentExponentiallyGenerated(n_t, r_t, jitter=JITTER)
            if route == "torch":
                return kern._torch_transitions(dt, True, False)[:2]
            return kern._device_transitions(dt, True, False)[:2]

        def backward(route):
            n_t, r_t = n_mat.clone().requires_grad_(True), r_mat.clone().requires_grad_(True)
            a_s, chol = forward(route, n_t, r_t)
            ((g_a * a_s).sum() + (g_c * chol).sum()).backward()
            return n_t.grad, r_t.grad

        with torch.no_grad():
            ref, got = forward("torch"), forward("hip")
        (gn_t, gr_t), (gn_h, gr_h) = backward("torch"), backward("hip")
        check = {"A": float((ref[0] - got[0]).abs().max()), "chol": float((ref[1] - got[1]).abs().max()),
                 "gN": float(((gn_t - gn_h).abs().max() / gn_t.abs().max())), "gR": float(((gr_t - gr_h).abs().max() / gr_t.abs().max()))}
        with torch.no_grad():
            f_hip, f_torch = alternate(lambda: forward("hip"), lambda: forward("torch"))
        b_hip, b_torch = alternate(lambda: backward("hip"), lambda: backward("torch"))
        row = {"dtype": str(dtype).split(".")[-1], "d": d, "forward_hip_ms": f_hip, "forward_torch_ms": f_torch,
               "forward_backward_hip_ms": b_hip, "forward_backward_torch_ms": b_torch, "agreement": check}
        results.append(row)
        print(f"{row['dtype']} d={d:2d}  forward: HIP {f_hip['median']:.3f} ms, torch {f_torch['median']:.3f} ms ({f_torch['median'] / f_hip['median']:.1f}x)"
              f"   forward+backward: HIP {b_hip['median']:.3f} ms, torch {b_torch['median']:.3f} ms ({b_torch['median'] / b_hip['median']:.1f}x)"
              f"   max |dA| {check['A']:.1e} |dchol| {check['chol']:.1e} rel gN {check['gN']:.1e} gR {check['gR']:.1e}", flush=True)
print(json.dumps({"bench": "leg", "B": BSZ, "T": T, "rounds": rounds, "window": window, "results": results}))
