"""StateSpaceModel.log_pdf: the fused route (``mf_ssm_log_pdf`` / ``mf_ssm_log_pdf_grad``, csrc/mf_logpdf.hip) against the composition
(``_log_pdf_composed``: a batched ``A x``, two ``solve_triangular`` calls, a ``cat`` and a ``sum``, differentiated by autograd) on the same
states, forward and forward plus backward with the states and the five leaves under the tape, at two shapes and both dtypes:

  iwvi    S = 16 samples of B = 64 series, T = 100 steps, d = 6 (the density ratio of scripts/bench_iwvi.py),
  large   S = 64 samples of B = 64 series, T = 2 000 steps, d = 6.

The variants alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the
medians (and minima) of the per-call window times are printed, then one JSON line with the bytes the algorithm needs by shapes.  Before
timing, value and gradients of the two routes are compared at the timed shape.  The times are whole-call medians (host included).
Usage: python3 scripts/bench_log_pdf.py [--rounds R] [--window W] [--small]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import markovflow_amd as mfa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--window", type=int, default=5)
ap.add_argument("--small", action="store_true", help="a fraction of the work: a rehearsal of the script, not a measurement")
args = ap.parse_args()
dev = torch.device("cuda:0")
SHAPES = {"iwvi": (16, 64, 100, 6), "large": (64, 64, 2000, 6)}
if args.small:
    SHAPES = {"iwvi": (16, 8, 100, 6), "large": (64, 4, 200, 6)}


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
    """The Sum(Matern52, Matern52) chain of scripts/bench_iwvi.py on ``bsz`` grids of ``t`` points with exponential gaps, as leaves."""
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    x = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, t, dtype=torch.float64, device=dev).exponential_(1.0, generator=g), dim=-1)
    kern = mfa.Sum([mfa.Matern52(1.0, 1.0, jitter=1e-9, device=dev), mfa.Matern52(3.0, 0.5, jitter=1e-9, device=dev)], jitter=1e-9)
    ssm = kern.state_space_model(x)
    leaves = (ssm.initial_mean, ssm.cholesky_initial_covariance, ssm.state_transitions, ssm.state_offsets, ssm.cholesky_process_covariances)
    return mfa.StateSpaceModel(*[v.to(dtype).requires_grad_(True) for v in leaves])


res = {"rounds": args.rounds, "window": args.window, "cases": {}}
for name, (s, bsz, t, d) in SHAPES.items():
    for dtype in (torch.float64, torch.float32):
        ssm = chain(bsz, t, dtype)
        assert ssm.state_dim == d
        with torch.no_grad():
            states = ssm.sample((s,))
        states.requires_grad_(True)
        leaves = [states, ssm.initial_mean, ssm.cholesky_initial_covariance, ssm.state_transitions, ssm.state_offsets,
                  ssm.cholesky_process_covariances]
        cot = torch.randn((s, bsz), dtype=dtype, device=dev)

        def fwd(route):
            with torch.no_grad():
                return route(states)

        def fwd_bwd(route):
            return torch.autograd.grad(route(states), leaves, cot)

        # chol Q of short gaps is inverted: in float64 the two routes agree to 1e-8 of the largest entry; in float32 each is held
        # against the composition in float64 on the same (rounded) inputs, and the fused error may be 4 x the composition's
        ref = mfa.StateSpaceModel(*[v.detach().double().requires_grad_(True) for v in leaves[1:]])
        x64 = states.detach().double().requires_grad_(True)
        want = [ref._log_pdf_composed(x64)]
        want += torch.autograd.grad(want[0], [x64, ref.initial_mean, ref.cholesky_initial_covariance, ref.state_transitions,
                                              ref.state_offsets, ref.cholesky_process_covariances], cot.double())

        def errors(route):
            outs = [fwd(route)] + list(fwd_bwd(route))
            return [float((a.double() - (torch.tril(b) if i in (3, 6) else b).detach()).abs().max() / b.detach().abs().max())
                    for i, (a, b) in enumerate(zip(outs, want))]

        diffs, base = errors(ssm.log_pdf), errors(ssm._log_pdf_composed)
        if dtype == torch.float64:
            assert max(diffs) < 1e-8, diffs
        else:
            assert all(a <= 4 * b + 1e-6 for a, b in zip(diffs, base)), (diffs, base)
        del ref, x64, want
        size = states.element_size()
        chain_bytes = (bsz * (t - 1) * (2 * d * d + d) + bsz * (d * d + d)) * size
        state_bytes = s * bsz * t * d * size
        r = alternate({"fused_fwd_ms": lambda: fwd(ssm.log_pdf), "composed_fwd_ms": lambda: fwd(ssm._log_pdf_composed),
                       "fused_fwd_bwd_ms": lambda: fwd_bwd(ssm.log_pdf), "composed_fwd_bwd_ms": lambda: fwd_bwd(ssm._log_pdf_composed)})
        r.update(shape={"S": s, "B": bsz, "T": t, "d": d}, rel_diffs=diffs, fwd_bytes=state_bytes + chain_bytes,
                 bwd_bytes=2 * (state_bytes + chain_bytes))
        key = f"{name}_{'f64' if dtype == torch.float64 else 'f32'}"
        res["cases"][key] = r
        print(f"{key:10s} " + "   ".join(f"{k[:-3]} {v['median']:8.3f} (min {v['min']:8.3f})" for k, v in r.items() if k.endswith("_ms"))
              + f" ms   largest rel diff {max(diffs):.1e}")
        del ssm, states, leaves, cot
        torch.cuda.empty_cache()
print(json.dumps(res))
