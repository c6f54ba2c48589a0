"""SparsePowerExpectationPropagation at the shape scripts/bench_sparse_cvi.py and scripts/bench_pep.py use - B = 64 series, N = 10^4
points, Sum(Matern52, Matern52) (d = 6, pairs of 2d = 12), fp64, Bernoulli likelihood, 20 Gauss-Hermite points, alpha = lr = 1/2 -
with M = 100 inducing points per series and with M = 2 (three long segments per series):

  * one ``update_sites()`` (posterior chain on the M inducing points, its pair marginals, the batched pair cavity, the cached
    per-point projections and ONE ``mf_lik_sparse_pep_site_update`` call of two launches),
  * the kernel pair alone against the torch composition of the same step (``models.sparse_pep_site_update_torch``) on the same device
    tensors,
  * the kernel pair against ``mf_lik_sparse_expectations`` (value and adjoints: SVGP's pair, the same front end and workspace row) at
    the same shape in the same process, and
  * ``PowerExpectationPropagation.update_sites()`` - one site per data point, a full smoother pass - at the same N.

The variants alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the
medians (and minima) of the per-call window times are printed, then one JSON line.  Before timing, kernel pair and composition are
compared on the same inputs.
Usage: python3 scripts/bench_sparse_pep.py [--batch B] [--points N] [--rounds R] [--window K] [--no-dense]"""
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
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--window", type=int, default=10)
ap.add_argument("--no-dense", action="store_true", help="skip PowerExpectationPropagation.update_sites()")
args = ap.parse_args()
dev = torch.device("cuda:0")
bsz, n, rounds, window = args.batch, args.points, args.rounds, args.window
f64 = torch.float64
g = torch.Generator(device=dev)
g.manual_seed(3)
x = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, n, dtype=f64, device=dev).exponential_(1.0, generator=g), dim=-1)
y = (torch.rand(bsz, n, 1, dtype=f64, device=dev, generator=g) < 0.5).to(f64)
lik = mfa.Bernoulli()
alpha = lr = 0.5


def kernel_sum():
    return mfa.Sum([mfa.Matern52(1.0, 1.0, jitter=1e-9, device=dev), mfa.Matern52(3.0, 0.5, jitter=1e-9, device=dev)], jitter=1e-9)


def build(m):
    frac = (torch.arange(m, dtype=f64, device=dev) + 0.5) / m
    z = (x[:, :1] + frac * (x[:, -1:] - x[:, :1])).contiguous()                    # evenly spaced over every series' span
    return mfa.SparsePowerExpectationPropagation(kernel_sum(), z, lik, learning_rate=lr, alpha=alpha)


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


def measure(m):
    """The four timings at M = m inducing points (ms per call) and the agreement of kernel pair and composition."""
    model = build(m)
    for _ in range(3):                                   # code objects, allocator, sites away from zero
        model.update_sites((x, y))
    w, c, indices, offsets, tiles = model._projections(x)
    cav_mean, cav_cov, seg_const = (t.contiguous() for t in model._cavity(x, model.dist_q))
    pair_mean, pair_cov = (t.contiguous() for t in model._pair_marginals(model.dist_q))
    assert bool(torch.isfinite(cav_cov).all()), "every cavity exists"
    yy = y[..., 0]
    a = [t.clone() for t in (model.nat1, model.nat2, model.log_norm)]
    b = [t.clone() for t in a]
    pair = lambda: MM.sparse_pep_site_update_hip(lik, w, c, yy, offsets, cav_mean, cav_cov, alpha, lr, *a, seg_const=seg_const,     # noqa: E731
                                                 tiles=tiles)
    composed = lambda: MM.sparse_pep_site_update_torch(lik, w, c, yy, indices, cav_mean, cav_cov, alpha, lr, *b,                   # noqa: E731
                                                       seg_const=seg_const)
    svgp = lambda: MM._sparse_expectations_launch(lik, w, c, yy, offsets, tiles, pair_mean, pair_cov, True)                        # noqa: E731
    # same inputs, both variants: the results must agree before their times are compared (index_add_ sums in another order)
    pair()
    composed()
    err = max(float((s - t).abs().max()) for s, t in zip(a, b))
    scale = max(float(t.abs().max()) for t in b)
    assert err <= 1e-10 * scale, (err, scale)
    t_pair, t_torch, t_svgp, t_update = [], [], [], []
    for _ in range(2):                                  # warm-up windows
        timed(pair)
        timed(composed)
        timed(svgp)
    for _ in range(rounds):                             # alternating, one process
        t_pair.append(timed(pair))
        t_torch.append(timed(composed))
        t_svgp.append(timed(svgp))
    update = lambda: model.update_sites((x, y))          # noqa: E731
    timed(update)
    for _ in range(rounds):
        t_update.append(timed(update))
    assert bool(torch.isfinite(model.energy((x, y))).all())          # the sites stayed in the domain
    return {"update_sites_ms": stats(t_update), "kernel_pair_ms": stats(t_pair), "torch_composition_ms": stats(t_torch),
            "svgp_pair_ms": stats(t_svgp), "kernel_pair_ns_per_point": statistics.median(t_pair) * 1e6 / (bsz * n),
            "svgp_pair_ns_per_point": statistics.median(t_svgp) * 1e6 / (bsz * n), "num_tiles": tiles[0],
            "kernel_vs_torch_max_abs_diff": err}


with torch.no_grad():
    res = {"shape": {"B": bsz, "N": n, "d": 6, "dtype": "float64", "likelihood": "Bernoulli", "nq": lik.num_gauss_hermite_points,
                     "alpha": alpha, "lr": lr}, "rounds": rounds, "window": window}
    for m in (100, 2):
        res[f"M{m}"] = measure(m)
    if not args.no_dense:
        dense = mfa.PowerExpectationPropagation((x, y), kernel_sum(), lik, learning_rate=lr, alpha=alpha)
        step = lambda: dense.update_sites()                  # noqa: E731
        for _ in range(2):
            timed(step)
        res["dense_pep_update_sites_ms"] = stats([timed(step) for _ in range(rounds)])

for m in (100, 2):
    r = res[f"M{m}"]
    for label, key in (("update_sites()", "update_sites_ms"), ("mf_lik_sparse_pep_site_update", "kernel_pair_ms"),
                       ("torch composition", "torch_composition_ms"), ("mf_lik_sparse_expectations", "svgp_pair_ms")):
        print(f"M = {m:3d}  {label:32s} median {r[key]['median']:.3f} ms   min {r[key]['min']:.3f} ms")
    print(f"M = {m:3d}  kernel pair {r['kernel_pair_ns_per_point']:.3f} ns per point, SVGP pair {r['svgp_pair_ns_per_point']:.3f} ns per point, "
          f"{r['num_tiles']} tiles")
if "dense_pep_update_sites_ms" in res:
    print(f"PowerExpectationPropagation.update_sites()  median {res['dense_pep_update_sites_ms']['median']:.3f} ms")
print(json.dumps(res))
