"""SpatioTemporalSparseCVI's site update at the shapes of scripts/bench_st.py - one series of N = 10^5 points, Ms = 32 spatial inducing
points, temporal Matern32 (D = Ms d_t = 64, pairs of dimension 128), Mt = 100 inducing times, Bernoulli likelihood, 20 Gauss-Hermite
nodes, in float64 and float32 - on three routes, on the same tensors:

  (1) the fused call, ``mf_lik_st_cvi_site_update``,
  (2) the composition from ``mf_lik_st_expectations``'s outputs: ``theta_1 = g_mean - 2 g_cov m``, ``theta_2 = g_cov`` and the blend
      in torch,
  (3) ``models.st_cvi_site_update_torch``,

  (a) as functions on random positive definite pair marginals at Ms = 32 in both dtypes, and
  (b) as ``update_sites()`` of a model - the pair marginals of ``dist_q`` from the sites, then the route - at the largest model the
      chain operators carry in the dtype: Ms = 32 (D = 64) in float32, Ms = 16 (D = 32) in float64 (``--model-space`` overrides
      both), beside ``dist_q`` and its pair marginals on their own.

The variants alternate inside one process in windows of ``--window`` calls between two device events, every window from the same
sites; after warm-up windows the medians (and minima) of the per-call window times are printed, then one JSON line.  Before timing,
the three routes are compared on the same inputs.
Usage: python3 scripts/bench_st_cvi.py [--points N] [--space Ms] [--model-space Ms] [--inducing Mt] [--rounds R] [--window W]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import markovflow_amd as mfa  # noqa: E402
from markovflow_amd import models as MM  # noqa: E402
from markovflow_amd import spatial_kernels as SK  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=100000)
ap.add_argument("--space", type=int, default=32)
ap.add_argument("--model-space", type=int, default=None)
ap.add_argument("--inducing", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
n, ms, mt, rounds, window = args.points, args.space, args.inducing, args.rounds, args.window
lik = mfa.Bernoulli()
LR = 0.1


def timed(fn, reset):
    """Per-call time of a window of calls between two device events, in ms; ``reset`` runs before the first event."""
    reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(window):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / window


def alternate(variants, reset):
    """Two warm-up windows, then ``rounds`` alternating windows of every variant: ``{name: {median, min}}``."""
    for _ in range(2):
        for fn in variants.values():
            timed(fn, reset)
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, reset))
    return {name: {"median": statistics.median(ts), "min": min(ts)} for name, ts in times.items()}


def build(dtype, num_space):
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    rand = lambda *shape: torch.rand(*shape, dtype=dtype, device=dev, generator=g)          # noqa: E731
    times = torch.sort(100.0 * rand(n)).values
    inputs = torch.cat([2.0 * rand(n, 2) - 1.0, times[:, None]], dim=-1).contiguous()
    obs = (rand(n, 1) < 0.5).to(dtype)
    z_space = (2.0 * rand(num_space, 2) - 1.0).contiguous()
    z_time = ((torch.arange(mt, dtype=dtype, device=dev) + 0.5) * (100.0 / mt)).contiguous()
    model = mfa.SpatioTemporalSparseCVI(z_space, z_time, SK.Matern32(1.0, 0.7, device=dev, dtype=dtype),
                                        mfa.Matern32(5.0, 1.0, jitter=1e-6, device=dev, dtype=dtype), lik, learning_rate=LR)
    return model, (inputs, obs), g


def composed_from_expectations(a, wt, c, y, offsets, tiles, pair_mean, pair_cov, nat1, nat2):
    """Route (2): one call of ``mf_lik_st_expectations_*`` for ``g_mean`` and ``g_cov``, the mat-vec and the blend in torch."""
    _, g_mean, g_cov = MM._st_expectations_launch(lik, a, wt, c, y, offsets, tiles, pair_mean, pair_cov, want_grads=True)[:3]
    theta1 = g_mean - 2.0 * (g_cov @ pair_mean[..., None])[..., 0]
    nat1.mul_(1.0 - LR).add_(LR * theta1)
    nat2.mul_(1.0 - LR).add_(LR * g_cov)


def measure(dtype):
    # ---- (a) the three routes as functions, on random pair marginals
    model, (inputs, obs), g = build(dtype, ms)
    order, a, wt, c, indices, offsets, tiles = model._projections(inputs)
    assert order is None
    y = obs[..., 0].contiguous()
    pair = 2 * model.kernel.state_dim
    root = torch.randn(mt + 1, pair, pair, dtype=dtype, device=dev, generator=g)
    pair_cov = (root @ root.transpose(-1, -2) / pair + 0.1 * torch.eye(pair, dtype=dtype, device=dev)).contiguous()
    pair_mean = torch.randn(mt + 1, pair, dtype=dtype, device=dev, generator=g)
    site = torch.randn(mt + 1, pair, pair, dtype=dtype, device=dev, generator=g)
    start = torch.randn(mt + 1, pair, dtype=dtype, device=dev, generator=g), (-0.5 * (site + site.transpose(-1, -2))).contiguous()
    nat1, nat2 = start[0].clone(), start[1].clone()

    def reset():
        nat1.copy_(start[0])
        nat2.copy_(start[1])

    routes = {
        "fused_ms": lambda: MM.st_cvi_site_update_hip(lik, a, wt, c, y, offsets, pair_mean, pair_cov, LR, nat1, nat2, tiles=tiles),
        "from_expectations_ms": lambda: composed_from_expectations(a, wt, c, y, offsets, tiles, pair_mean, pair_cov, nat1, nat2),
        "torch_ms": lambda: MM.st_cvi_site_update_torch(lik, a, wt, c, y, indices, pair_mean, pair_cov, LR, nat1, nat2),
    }
    got = {}
    for name, fn in routes.items():
        reset()
        fn()
        got[name] = (nat1.clone(), nat2.clone())
    rel = {name: [float((p - q).abs().max() / q.abs().max()) for p, q in zip(got[name], got["torch_ms"])] for name in list(routes)[:2]}
    assert max(max(v) for v in rel.values()) < (1e-9 if dtype == torch.float64 else 2e-3), rel
    res = {"dtype": str(dtype).split(".")[-1], "rel_diff_to_torch": rel}
    res["function"] = alternate(routes, reset)

    # ---- (b) update_sites() of the largest model the chain operators carry in this dtype
    model, xy, _ = build(dtype, args.model_space or (ms if dtype == torch.float32 else min(ms, 16)))
    model.update_sites(xy)                       # (a dist_q that is not the prior)
    start_b = model.nat1.clone(), model.nat2.clone()
    _, a_b, wt_b, c_b, _, offsets_b, tiles_b = model._projections(xy[0])
    y_b = xy[1][..., 0].contiguous()

    def reset_b():
        model.nat1.copy_(start_b[0])
        model.nat2.copy_(start_b[1])

    def from_expectations_step():
        with torch.no_grad():
            pm, pc = model._pair_marginals()
            composed_from_expectations(a_b, wt_b, c_b, y_b, offsets_b, tiles_b, pm, pc, model.nat1, model.nat2)

    def torch_step():
        model._fused = lambda inputs_: False
        try:
            model.update_sites(xy)
        finally:
            del model._fused

    def pair_marginals():
        with torch.no_grad():
            model._pair_marginals()

    res["model_D"] = model.kernel.state_dim
    res["step"] = alternate({"fused_update_sites_ms": lambda: model.update_sites(xy), "from_expectations_update_sites_ms": from_expectations_step,
                             "torch_update_sites_ms": torch_step, "dist_q_and_pair_marginals_ms": pair_marginals}, reset_b)
    for group in ("function", "step"):
        for key, val in res[group].items():
            print(f"{res['dtype']:8s} {key:36s} median {val['median']:9.3f} ms   min {val['min']:9.3f} ms")
    f = res["function"]
    print(f"{res['dtype']:8s} fused / from expectations: {f['fused_ms']['median'] / f['from_expectations_ms']['median']:.3f},  "
          f"fused / torch: {f['fused_ms']['median'] / f['torch_ms']['median']:.4f}")
    return res


out = {"shape": {"N": n, "Ms": ms, "Mt": mt, "D": 2 * ms, "likelihood": "Bernoulli", "nodes": lik.num_gauss_hermite_points,
                 "learning_rate": LR}, "rounds": rounds, "window": window, "runs": [measure(torch.float64), measure(torch.float32)]}
print(json.dumps(out))          # (one line: what CHANGELOG.md quotes)
