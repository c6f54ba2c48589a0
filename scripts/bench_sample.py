"""StateSpaceModel.sample outside the tape: the fused sampler (``mf_ssm_sample``, csrc/mf_sample.hip) against the composed route
(``_sample_composed``: two concatenated copies of the chain, a batched ``chol Q eps``, an add, ``mf_ssm_marginal_means``) on the same eps,
at two shapes and both dtypes:

  partitioned   S = 16 samples of B = 64 series, T = 10 100 steps, d = 6 (the prior draw of scripts/bench_iwvi.py),
  sweep         S = 60 000 samples of B = 1 series, T = 11 steps, d = 6 (scripts/bench_sampling.py's kind of shape).

The two variants alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the
medians (and minima) of the per-call window times are printed, then one JSON line with the bytes the algorithm needs by shapes and
the rate they give over the median.  eps is drawn once per shape, outside the timed region, and both routes read it; before timing
their outputs are compared at the timed shape.  Kernel times come from a ``rocprofv3 --kernel-trace --stats`` run of this script.
Usage: python3 scripts/bench_sample.py [--rounds R] [--window W] [--small]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import markovflow_amd as mfa  # noqa: E402
from markovflow_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--window", type=int, default=3)
ap.add_argument("--small", action="store_true", help="a hundredth of the work: a rehearsal of the script, not a measurement")
args = ap.parse_args()
dev = torch.device("cuda:0")
SHAPES = {"partitioned": (16, 64, 10100, 6), "sweep": (60000, 1, 11, 6)}
if args.small:
    SHAPES = {"partitioned": (16, 8, 1010, 6), "sweep": (600, 1, 11, 6)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.window):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.window


def alternate(variants):
    for _ in range(2):
        for fn in variants.values():
            timed(fn)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    return {name: {"median": statistics.median(ts), "min": min(ts)} for name, ts in times.items()}


def chain(bsz, t, dtype):
    """The Sum(Matern52, Matern52) chain of scripts/bench_iwvi.py on ``bsz`` grids of ``t`` points with exponential gaps."""
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    x = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, t, dtype=torch.float64, device=dev).exponential_(1.0, generator=g), dim=-1)
    kern = mfa.Sum([mfa.Matern52(1.0, 1.0, jitter=1e-9, device=dev), mfa.Matern52(3.0, 0.5, jitter=1e-9, device=dev)], jitter=1e-9)
    ssm = kern.state_space_model(x)
    leaves = (ssm.initial_mean, ssm.cholesky_initial_covariance, ssm.state_transitions, ssm.state_offsets, ssm.cholesky_process_covariances)
    return mfa.StateSpaceModel(*[v.to(dtype) for v in leaves])


def fused(ssm, eps, out, ws, ws_bytes):
    mu0, cp0, a_f, b_f, cq = ssm._flat_params()
    s, bsz, t, d = out.shape
    _lib.call("mf_ssm_sample", out.dtype, bsz, s, t, d, _lib.ptr(mu0), _lib.ptr(cp0), _lib.ptr(a_f), _lib.ptr(b_f), _lib.ptr(cq),
              _lib.ptr(eps), _lib.ptr(out), _lib.ptr(ws), ws_bytes, 0, _lib.stream_ptr(dev))
    return out


res = {"rounds": args.rounds, "window": args.window, "cases": {}}
with torch.no_grad():
    for name, (s, bsz, t, d) in SHAPES.items():
        for dtype in (torch.float64, torch.float32):
            ssm = chain(bsz, t, dtype)
            assert ssm.state_dim == d
            eps = torch.randn((s, bsz, t, d, 1), dtype=dtype, device=dev)
            out = torch.empty((s, bsz, t, d), dtype=dtype, device=dev)
            size = out.element_size()
            ws_bytes = int(_lib.load().mf_ssm_sample_workspace_bytes(bsz, s, t, d, size, 0))
            ws = _lib.workspace(ws_bytes, dev)
            want = ssm._sample_composed(eps)
            got = fused(ssm, eps, out, ws, ws_bytes)
            diff = float((got - want).abs().max() / want.abs().max())
            # two recursions in the working dtype against each other, relative to the largest state: a few thousand eps at the most
            assert diff < (1e-12 if dtype == torch.float64 else 1e-4), diff
            del want
            chain_bytes = (bsz * (t - 1) * (2 * d * d + d) + bsz * (d * d + d)) * size
            draw_bytes = s * bsz * t * d * size
            passes = 2 if ws_bytes else 1
            needed = passes * (draw_bytes + chain_bytes) + draw_bytes              # eps and the chain per pass, the draw once
            r = alternate({"fused_ms": lambda: fused(ssm, eps, out, ws, ws_bytes), "composed_ms": lambda: ssm._sample_composed(eps)})
            r.update(shape={"S": s, "B": bsz, "T": t, "d": d}, regime="partitioned" if ws_bytes else "sweep", rel_diff=diff,
                     bytes_needed=needed, fused_gb_per_s=needed / (r["fused_ms"]["median"] * 1e-3) / 1e9)
            key = f"{name}_{'f64' if dtype == torch.float64 else 'f32'}"
            res["cases"][key] = r
            print(f"{key:18s} fused {r['fused_ms']['median']:8.3f} ms (min {r['fused_ms']['min']:8.3f})   composed "
                  f"{r['composed_ms']['median']:8.3f} ms (min {r['composed_ms']['min']:8.3f})   {needed / 1e9:.3f} GB by shapes, "
                  f"{r['fused_gb_per_s']:.0f} GB/s   rel diff {diff:.1e}")
            del ssm, eps, out, ws
            torch.cuda.empty_cache()
print(json.dumps(res))
