"""SparseVariationalGaussianProcess with MultiStageLikelihood: the multi-latent data term fused (``mf_lik_sparse_multi_expectations``)
against composed (``models.sparse_multi_expected_log_likelihood_torch``) and against the single-latent pair.
IndependentMultiOutput([Matern32] * 3) (d = 6, pairs of 2d = 12, L = 3 latents), 20 Gauss-Hermite points, B = 64 series, N = 10^4
points, M = 100 inducing points, observations drawn with ``sample_y``.

Timed:
  * ``elbo`` forward + backward onto the leaves of ``dist_q``, fused and composed on the same model and tensors (float64: the model);
  * per dtype (float64, then float32 on the same tensors cast down), alternating in one process:
      - the kernel pair alone, value and adjoints;
      - ``sparse_multi_expected_log_likelihood_torch`` forward + backward onto the pair marginals, the composition it replaces;
      - ``mf_lik_sparse_expectations`` (Bernoulli, one latent) at the same N, tile table and 2d = 12: row 0 of ``w`` and ``c``.

The variants alternate in windows of ``--window`` calls between two device events; after warm-up windows the medians (and minima) of
the per-call window times are printed, then one JSON line.  Before timing, fused and composed results are compared.  The pair's
achieved bytes/s counts the bytes it must move: L (2d + 1) + 1 values in per point, the pair marginals in, the workspace written and
read, the three outputs.
Usage: python3 scripts/bench_multistage.py [--rounds R] [--window K] [--batch B] [--points N] [--inducing M]"""
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
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--window", type=int, default=10)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--points", type=int, default=10000)
ap.add_argument("--inducing", type=int, default=100)
args = ap.parse_args()
dev = torch.device("cuda:0")
bsz, n, m = args.batch, args.points, args.inducing
rounds, window = args.rounds, args.window
f64 = torch.float64
two_d, latents = 12, 3
g = torch.Generator(device=dev)
g.manual_seed(3)
x = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, n, dtype=f64, device=dev).exponential_(1.0, generator=g), dim=-1)
lik = mfa.MultiStageLikelihood()
span = x[:, -1:] - x[:, :1]
phase = (x - x[:, :1]) / span
latent = torch.stack([0.8 * torch.sin(9.0 * phase) - 0.2, torch.cos(6.0 * phase), 0.9 + 0.6 * torch.sin(4.0 * phase + 1.0)], dim=-1)
y = lik.sample_y(latent, generator=g)
kern = mfa.IndependentMultiOutput([mfa.Matern32(ls, var, jitter=1e-9, device=dev) for ls, var in ((1.0, 1.0), (3.0, 0.7), (0.5, 1.3))],
                                  jitter=1e-9)
frac = (torch.arange(m, dtype=f64, device=dev) + 0.5) / m
z = (x[:, :1] + frac * span).contiguous()                                      # evenly spaced over every series' span


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


model = mfa.SparseVariationalGaussianProcess(kern, lik, z)
for _ in range(2):                                      # a q away from the prior
    mfa.SSMNaturalGradient(gamma=0.05, momentum=False).minimize(lambda: model.loss((x, y)), model.dist_q)
leaves = model.trainable_variables


def step(fused):
    model._fused = (lambda t: True) if fused else (lambda t: False)
    return torch.autograd.grad(model.elbo((x, y)), leaves)


def elbo_of(fused):
    model._fused = (lambda t: True) if fused else (lambda t: False)
    with torch.no_grad():
        return float(model.elbo((x, y)))


# same model, both routes: the results must agree before their times are compared
v_fused, v_composed = elbo_of(True), elbo_of(False)
g_fused, g_composed = step(True), step(False)
assert abs(v_fused - v_composed) <= 1e-9 * abs(v_composed), (v_fused, v_composed)
grad_err = max(float((a - b).abs().max()) for a, b in zip(g_fused, g_composed))
grad_scale = max(float(b.abs().max()) for b in g_composed)
assert grad_err <= 1e-8 * grad_scale, (grad_err, grad_scale)
t_fused, t_composed = alternate(lambda: step(True), lambda: step(False))
del model._fused
print(f"{'elbo fwd + bwd, fused':44s} median {t_fused['median']:.3f} ms   min {t_fused['min']:.3f} ms", flush=True)
print(f"{'elbo fwd + bwd, composed':44s} median {t_composed['median']:.3f} ms   min {t_composed['min']:.3f} ms", flush=True)

with torch.no_grad():
    _, w64, c64, indices, offsets, tiles = model._projections(x)
    pm64, pc64 = (t.contiguous() for t in model._pair_marginals())
bern = mfa.Bernoulli()
row = two_d * (two_d + 1) // 2 + two_d + 1
segs = bsz * (m + 1)
res = {"shape": {"B": bsz, "N": n, "M": m, "d": 6, "latents": latents, "likelihood": "MultiStageLikelihood",
                 "nq": lik.num_gauss_hermite_points, "tiles": tiles[0]},
       "elbo_fwd_bwd_fused_ms": t_fused, "elbo_fwd_bwd_composed_ms": t_composed,
       "fused_vs_composed_elbo_rel_diff": abs(v_fused - v_composed) / abs(v_composed),
       "fused_vs_composed_grad_max_abs_diff": grad_err, "rounds": rounds, "window": window}
for dtype, name, tol in ((torch.float64, "float64", 1e-10), (torch.float32, "float32", 1e-3)):
    w, c, pair_mean, pair_cov = (t.to(dtype).contiguous() for t in (w64, c64, pm64, pc64))
    yy = y[..., 0].to(dtype).contiguous()
    w1, c1, y1 = w[..., 0, :].contiguous(), c[..., 0].contiguous(), (yy == 0).to(dtype)      # latent 0 as a Bernoulli problem

    def pair():
        with torch.no_grad():
            return MM._sparse_multi_expectations_launch(lik, w, c, yy, offsets, tiles, pair_mean, pair_cov, True)

    def single():
        with torch.no_grad():
            return MM._sparse_expectations_launch(bern, w1, c1, y1, offsets, tiles, pair_mean, pair_cov, True)

    def composed():
        pm, pc = pair_mean.clone().requires_grad_(True), pair_cov.clone().requires_grad_(True)
        value = MM.sparse_multi_expected_log_likelihood_torch(lik, w, c, yy, indices, pm, pc)
        return (value,) + torch.autograd.grad(value.sum(), (pm, pc))

    for a, b, what in zip(pair(), composed(), ("ve_sum", "g_mean", "g_cov")):
        err, scale = float((a - b.detach()).abs().max()), float(b.detach().abs().max())
        assert err <= tol * scale, (name, what, err, scale)
    t_pair, t_torch, t_single = alternate(pair, composed, single)
    esz = w.element_size()
    pair_bytes = esz * (bsz * n * (latents * (two_d + 1) + 1) + segs * (two_d + two_d * two_d) + 2 * tiles[0] * row
                        + segs * (1 + two_d + two_d * two_d)) + 8 * (bsz * (m + 2) + tiles[0] + segs + 1)
    for label, t in (("mf_lik_sparse_multi_expectations", t_pair), ("torch composition, fwd + bwd", t_torch),
                     ("mf_lik_sparse_expectations (one latent)", t_single)):
        print(f"{name} {label:36s} median {t['median']:.3f} ms   min {t['min']:.3f} ms", flush=True)
    print(f"{name} pair: {pair_bytes / t_pair['median'] / 1e6:.1f} GB/s over {pair_bytes / 1e6:.1f} MB it must move; "
          f"{t_pair['median'] * 1e6 / (bsz * n):.3f} ns per point, {t_pair['median'] / t_single['median']:.2f} x the single-latent pair, "
          f"{t_torch['median'] / t_pair['median']:.1f} x faster than the composition", flush=True)
    res[name] = {"kernel_pair_ms": t_pair, "torch_composition_ms": t_torch, "single_latent_pair_ms": t_single,
                 "kernel_pair_bytes": pair_bytes, "kernel_pair_GBps": pair_bytes / t_pair["median"] / 1e6,
                 "kernel_pair_ns_per_point": t_pair["median"] * 1e6 / (bsz * n),
                 "multi_over_single": t_pair["median"] / t_single["median"],
                 "composition_over_pair": t_torch["median"] / t_pair["median"]}
print(json.dumps(res))
