"""SparseCVIGaussianProcess at the shape scripts/bench_cvi.py uses for the dense-site model - B = 64 series, N = 10^4 points,
Sum(Matern52, Matern52) (d = 6, pairs of 2d = 12), fp64, Bernoulli likelihood, 20 Gauss-Hermite points - with M = 100 inducing
points per series:

  * one ``update_sites()`` (posterior chain on the M inducing points, its pair marginals, the cached per-point projections and ONE
    ``mf_lik_sparse_cvi_site_update`` launch),
  * the site kernel alone against the torch composition of the same update (``models.sparse_cvi_site_update_torch``: gathers,
    the expectations, ``back_project_nats`` to [B, N, 2d, 2d] and ``index_add_``) on the same device tensors, and
  * the site kernel alone on the long-segment layout M = 1 (two segments per series, about N / 2 points each) at the same N.

The variants alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the
medians (and minima) of the per-call window times are printed, then one JSON line.  Before timing, kernel and composition are
compared on the same inputs.  The kernel's achieved bytes/s counts the bytes it must move: (2d + 2) values in per point, the pair
marginals in, the sites in and out.
Usage: python3 scripts/bench_sparse_cvi.py [--batch B] [--points N] [--inducing M] [--rounds R] [--window K]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import markovflow_amd as mfa  # noqa: E402
from markovflow_amd import models as MM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--points", type=int, default=10000)
ap.add_argument("--inducing", type=int, default=100)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--window", type=int, default=10)
args = ap.parse_args()
dev = torch.device("cuda:0")
bsz, n, rounds, window = args.batch, args.points, args.rounds, args.window
f64 = torch.float64
g = torch.Generator(device=dev)
g.manual_seed(3)
x = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, n, dtype=f64, device=dev).exponential_(1.0, generator=g), dim=-1)
y = (torch.rand(bsz, n, 1, dtype=f64, device=dev, generator=g) < 0.5).to(f64)
lik = mfa.Bernoulli()
lr = 0.1


def build(m):
    kern = mfa.Sum([mfa.Matern52(1.0, 1.0, jitter=1e-9, device=dev), mfa.Matern52(3.0, 0.5, jitter=1e-9, device=dev)], jitter=1e-9)
    frac = (torch.arange(m, dtype=f64, device=dev) + 0.5) / m
    z = (x[:, :1] + frac * (x[:, -1:] - x[:, :1])).contiguous()                    # evenly spaced over every series' span
    return mfa.SparseCVIGaussianProcess(kern, z, lik, learning_rate=lr)


def timed(fn):
    """Per-call time of a window of calls between two device events, in ms."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(window):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / window


def site_inputs(model):
    """The tensors one site update reads, after three warm-up steps (code objects, allocator, sites away from zero)."""
    for _ in range(3):
        model.update_sites((x, y))
    w, c, indices, offsets = model._projections(x)
    pair_mean, pair_cov = model._pair_marginals(model.dist_q)
    return w, c, indices, offsets, pair_mean.contiguous(), pair_cov.contiguous()


def kernel_bytes(m, two_d=12, esz=8):
    sites = bsz * (m + 1) * (two_d + two_d * two_d)
    return esz * (bsz * n * (two_d + 2) + 3 * sites) + 8 * bsz * (m + 2)


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts)}


with torch.no_grad():
    model = build(args.inducing)
    w, c, indices, offsets, pair_mean, pair_cov = site_inputs(model)
    yy = y[..., 0]
    a1, a2 = model.nat1.clone(), model.nat2.clone()
    b1, b2 = a1.clone(), a2.clone()
    kernel = lambda: MM.sparse_cvi_site_update_hip(lik, w, c, yy, offsets, pair_mean, pair_cov, lr, a1, a2)               # noqa: E731
    composed = lambda: MM.sparse_cvi_site_update_torch(lik, w, c, yy, indices, pair_mean, pair_cov, lr, b1, b2)           # noqa: E731
    # same inputs, both variants: the results must agree before their times are compared (index_add_ sums in another order)
    kernel()
    composed()
    err = max(float((a1 - b1).abs().max()), float((a2 - b2).abs().max()))
    scale = max(float(b1.abs().max()), float(b2.abs().max()))
    assert err <= 1e-10 * scale, (err, scale)
    t_kernel, t_torch, t_update, t_long = [], [], [], []
    for _ in range(2):                                  # warm-up windows
        timed(kernel)
        timed(composed)
    for _ in range(rounds):                             # alternating, one process
        t_kernel.append(timed(kernel))
        t_torch.append(timed(composed))
    update = lambda: model.update_sites((x, y))          # noqa: E731
    timed(update)
    for _ in range(rounds):
        t_update.append(timed(update))
    float(model.classic_elbo((x, y)))                   # the sites stayed in the domain (a failure would raise here)
    # the long-segment layout: one inducing point in the middle of every series
    long_model = build(1)
    lw, lc, _, loffsets, lpm, lpc = site_inputs(long_model)
    l1, l2 = long_model.nat1.clone(), long_model.nat2.clone()
    long_kernel = lambda: MM.sparse_cvi_site_update_hip(lik, lw, lc, yy, loffsets, lpm, lpc, lr, l1, l2)                 # noqa: E731
    for _ in range(2):
        timed(long_kernel)
    for _ in range(rounds):
        t_long.append(timed(long_kernel))

res = {
    "shape": {"B": bsz, "N": n, "M": args.inducing, "d": 6, "dtype": "float64", "likelihood": "Bernoulli",
              "nq": lik.num_gauss_hermite_points},
    "update_sites_ms": stats(t_update),
    "site_kernel_ms": stats(t_kernel),
    "torch_composition_ms": stats(t_torch),
    "site_kernel_bytes": kernel_bytes(args.inducing),
    "site_kernel_GBps": kernel_bytes(args.inducing) / statistics.median(t_kernel) / 1e6,
    "site_kernel_ns_per_point": statistics.median(t_kernel) * 1e6 / (bsz * n),
    "long_segment_M1_site_kernel_ms": stats(t_long),
    "long_segment_M1_ns_per_point": statistics.median(t_long) * 1e6 / (bsz * n),
    "kernel_vs_torch_max_abs_diff": err,
    "rounds": rounds,
    "window": window,
}
for label, key in (("update_sites()", "update_sites_ms"), ("mf_lik_sparse_cvi_site_update", "site_kernel_ms"),
                   ("torch composition", "torch_composition_ms"), ("site kernel, M = 1", "long_segment_M1_site_kernel_ms")):
    print(f"{label:32s} median {res[key]['median']:.3f} ms   min {res[key]['min']:.3f} ms")
print(f"site kernel: {res['site_kernel_GBps']:.1f} GB/s over {res['site_kernel_bytes'] / 1e6:.1f} MB it must move; "
      f"{res['site_kernel_ns_per_point']:.3f} ns per point balanced, {res['long_segment_M1_ns_per_point']:.3f} ns per point at M = 1")
print(json.dumps(res))
