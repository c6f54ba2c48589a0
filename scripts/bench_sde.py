"""Non-linear SDEs: the fused kernels of csrc/mf_nlsde.hip against the torch routes of ``markovflow_amd.sde``.

* ``euler_maruyama`` (ONE launch for all steps) against ``euler_maruyama_torch`` (about five launches per step) at ``B = 65536``,
  ``T = 1000``, ``D = 1`` and ``D = 4``, double well, with the achieved bytes per second against the ``2 B T D`` elements the kernel must
  move (the noise in, the path out); the draw of the noise (``torch.randn``) is timed on its own.
* ``linearize_sde`` and the drift difference with its four derivatives (forward and backward) against their torch compositions over
  ``[B, N, nq]`` temporaries at ``B = 64``, ``N = 10^4``, ``nq = 20``.

The two sides alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the
medians (and minima) of the per-call window times are printed, then one JSON line.  Before timing, the two sides are compared.
Usage: python3 scripts/bench_sde.py [--rounds R] [--window K] [--paths B] [--steps T]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from markovflow_amd import sde as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=int, default=4)
ap.add_argument("--paths", type=int, default=65536)
ap.add_argument("--steps", type=int, default=1000)
args = ap.parse_args()
dev = torch.device("cuda:0")
rounds, window = args.rounds, args.window


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


def rel_diff(a, b):
    return float((a - b).abs().max() / b.abs().max())


results = []
for dtype in (torch.float64, torch.float32):
    name = str(dtype).replace("torch.", "")
    for d in (1, 4):
        bsz, tn = args.paths, args.steps
        q = 0.5 * torch.eye(d, dtype=torch.float64) + 0.1
        sde = S.DoubleWellSDE(q)
        gen = torch.Generator(device=dev).manual_seed(d)
        x0 = torch.randn((bsz, d), generator=gen, dtype=dtype, device=dev).clamp(-1.5, 1.5)
        grid = torch.linspace(0.0, 1.0, tn, dtype=torch.float64).to(dev, dtype)
        noise = torch.randn((bsz, tn - 1, d), generator=gen, dtype=dtype, device=dev)
        with torch.no_grad():
            diff = rel_diff(S.euler_maruyama(sde, x0, grid, noise=noise), S.euler_maruyama_torch(sde, x0, grid, noise))
            fused, comp, draw = alternate(lambda: S.euler_maruyama(sde, x0, grid, noise=noise),
                                          lambda: S.euler_maruyama_torch(sde, x0, grid, noise),
                                          lambda: torch.randn((bsz, tn - 1, d), generator=gen, dtype=dtype, device=dev))
        moved = 2.0 * bsz * tn * d * x0.element_size()
        row = {"what": "euler_maruyama", "dtype": name, "B": bsz, "T": tn, "D": d, "max_rel_diff": diff, "fused_ms": fused,
               "torch_ms": comp, "noise_draw_ms": draw, "ratio_median": comp["median"] / fused["median"],
               "fused_GB_per_s": moved / (fused["median"] * 1e-3) / 1e9}
        results.append(row)
        print(f"{name:8s} euler_maruyama B={bsz} T={tn} D={d}  fused {fused['median']:9.4f} ms (min {fused['min']:9.4f}, "
              f"{row['fused_GB_per_s']:7.1f} GB/s)  torch {comp['median']:9.3f} ms (min {comp['min']:9.3f})  x{row['ratio_median']:.1f}  "
              f"noise draw {draw['median']:8.4f} ms  diff {diff:.1e}", flush=True)
        del noise
    bsz, n, nq = 64, 10000, 20
    gen = torch.Generator().manual_seed(5)
    mean = (3.0 * torch.rand((bsz, n, 1), generator=gen, dtype=torch.float64) - 1.5).to(dev, dtype)
    cov = (0.05 + 0.5 * torch.rand((bsz, n, 1, 1), generator=gen, dtype=torch.float64)).to(dev, dtype)
    a_d = torch.randn((bsz, n, 1, 1), generator=gen, dtype=torch.float64).to(dev, dtype)
    b_d = torch.randn((bsz, n, 1), generator=gen, dtype=torch.float64).to(dev, dtype)
    times = torch.linspace(0.0, 10.0, n + 1, dtype=torch.float64).to(dev, dtype)
    sde = S.DoubleWellSDE([[0.5]], num_gauss_hermite_points=nq)
    first = (mean[:, 0], cov[:, 0])
    with torch.no_grad():
        ssm = S.linearize_sde(sde, times, (mean, cov), first)
        ref = S.linearize_torch(sde, times, mean[..., 0], cov[..., 0, 0])
        diff = max(rel_diff(ssm.state_transitions[..., 0, 0], ref[0]), rel_diff(ssm.state_offsets[..., 0], ref[1]))
        fused, comp = alternate(lambda: S.linearize_sde(sde, times, (mean, cov), first),
                                lambda: S.linearize_torch(sde, times, mean[..., 0], cov[..., 0, 0]))
    row = {"what": "linearize_sde", "dtype": name, "B": bsz, "N": n, "nq": nq, "max_rel_diff": diff, "fused_ms": fused, "torch_ms": comp,
           "ratio_median": comp["median"] / fused["median"]}
    results.append(row)
    print(f"{name:8s} linearize_sde B={bsz} N={n} nq={nq}  fused {fused['median']:8.4f} ms (min {fused['min']:8.4f})  "
          f"torch {comp['median']:8.4f} ms (min {comp['min']:8.4f})  x{row['ratio_median']:.2f}  diff {diff:.1e}", flush=True)

    leaves = [t.clone().requires_grad_(True) for t in (mean, cov, a_d, b_d)]

    def fused_step():
        for t in leaves:
            t.grad = None
        S.squared_drift_difference_along_Gaussian_path(sde, S.LinearDrift(leaves[2], leaves[3]), (leaves[0], leaves[1]), 0.01, nq).sum().backward()

    def torch_step():
        for t in leaves:
            t.grad = None
        S.squared_drift_difference_torch(sde, leaves[0][..., 0], leaves[1][..., 0, 0], leaves[2][..., 0, 0], leaves[3][..., 0], 0.01,
                                         nq).sum().backward()

    fused_step()
    g_fused = [t.grad.clone() for t in leaves]
    torch_step()
    diff = max(rel_diff(a, t.grad) for a, t in zip(g_fused, leaves))
    fused, comp = alternate(fused_step, torch_step)
    row = {"what": "drift_difference_value_and_grad", "dtype": name, "B": bsz, "N": n, "nq": nq, "max_rel_diff": diff, "fused_ms": fused,
           "torch_ms": comp, "ratio_median": comp["median"] / fused["median"]}
    results.append(row)
    print(f"{name:8s} drift difference + backward B={bsz} N={n} nq={nq}  fused {fused['median']:8.4f} ms (min {fused['min']:8.4f})  "
          f"torch {comp['median']:8.4f} ms (min {comp['min']:8.4f})  x{row['ratio_median']:.2f}  diff {diff:.1e}", flush=True)
print(json.dumps({"bench": "sde", "rounds": rounds, "window": window, "results": results}))
