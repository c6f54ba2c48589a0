"""ImpulseMeanFunction: the fused route (``mf_mean_response``: a coefficient scan and one evaluation kernel that builds every block of
``exp(F dt)`` in registers) against the composition the reference uses, made of operations that existed before the fused kernels:
``state_transitions`` on the action gaps, ``LowerTriangularBlockTriDiagonal.solve`` for the coefficients, ``state_transitions`` on
the data (a materialised ``[B, N, d, d]``), two gathers, a matmul and the projection.

Shapes ``(B, K, N)`` in {(1, 8, 1 << 20), (64, 8, 16384), (64, 256, 16384), (1024, 4, 1024)}, a Matern-3/2 kernel (d = 2) and
``Matern32 + Matern52`` (d = 5), float64 and float32.

The two sides alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the
medians (and minima) of the per-call window times are printed, then one JSON line.  Before timing, the two sides are compared.
Usage: python3 scripts/bench_mean_function.py [--rounds R] [--window K]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import markovflow_amd as mfa  # noqa: E402
from markovflow_amd.kernels import to_delta_time  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--window", type=int, default=8)
args = ap.parse_args()
dev = torch.device("cuda:0")
rounds, window = args.rounds, args.window
SHAPES = [(1, 8, 1 << 20), (64, 8, 16384), (64, 256, 16384), (1024, 4, 1024)]


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


def composition(kernel, tau, u, t):
    """The reference's evaluation (mean_function.py:195-258) on this package's operators."""
    k, d = tau.shape[-1], u.shape[-1]
    eye = torch.eye(d, dtype=u.dtype, device=u.device).expand(tuple(tau.shape) + (d, d)).contiguous()
    a_s = -kernel.state_transitions(tau[..., :-1], to_delta_time(tau)) if k > 1 else None
    coef = mfa.LowerTriangularBlockTriDiagonal(eye, a_s).solve(u)
    coef = torch.cat([torch.zeros_like(coef[..., :1, :]), coef], dim=-2)
    idx = torch.searchsorted(tau, t)
    start = torch.cat([tau[..., :1], tau], dim=-1)
    delta = (t - torch.gather(start, -1, idx)).clamp(min=0.0)         # (the reference's dummy first bin: a zero coefficient)
    c_k = torch.gather(coef, -2, idx[..., None].expand(tuple(idx.shape) + (d,)))
    state = torch.matmul(kernel.state_transitions(t, delta), c_k[..., None])[..., 0]
    return kernel.generate_emission_model(t).project_state_to_f(state)


results = []
for dtype in (torch.float64, torch.float32):
    for name in ("Matern32", "Matern32+Matern52"):
        for bsz, num, n in SHAPES:
            gen = torch.Generator().manual_seed(bsz + num)
            if name == "Matern32":
                kernel = mfa.Matern32(0.9, 1.0, device=dev, dtype=dtype)
            else:
                kernel = mfa.Sum([mfa.Matern32(0.9, 1.0, device=dev, dtype=dtype), mfa.Matern52(1.6, 1.3, device=dev, dtype=dtype)])
            d = kernel.state_dim
            tau = torch.sort(10.0 * torch.rand((bsz, num), generator=gen, dtype=torch.float64), dim=-1)[0].to(dev, dtype)
            u = torch.randn((bsz, num, d), generator=gen, dtype=torch.float64).to(dev, dtype)
            t = torch.sort(-1.0 + 13.0 * torch.rand((bsz, n), generator=gen, dtype=torch.float64), dim=-1)[0].to(dev, dtype)
            mean = mfa.ImpulseMeanFunction(tau, u, kernel)
            with torch.no_grad():
                got, ref = mean(t), composition(kernel, tau, u, t)
                diff = float((got - ref).abs().max() / ref.abs().max())
                fused, comp = alternate(lambda: mean(t), lambda: composition(kernel, tau, u, t))
            row = {"dtype": str(dtype).replace("torch.", ""), "kernel": name, "B": bsz, "K": num, "N": n, "max_rel_diff": diff,
                   "fused_ms": fused, "composition_ms": comp, "ratio_median": comp["median"] / fused["median"]}
            results.append(row)
            print(f"{row['dtype']:8s} {name:18s} B={bsz:5d} K={num:4d} N={n:8d}  fused {fused['median']:8.4f} ms (min {fused['min']:8.4f})  "
                  f"composition {comp['median']:8.4f} ms (min {comp['min']:8.4f})  x{row['ratio_median']:.2f}  diff {diff:.1e}", flush=True)
print(json.dumps({"bench": "mean_function", "rounds": rounds, "window": window, "results": results}))
