"""SparseVariationalGaussianProcess: the ELBO's data term fused (``mf_lik_sparse_expectations``) against composed
(``models.sparse_expected_log_likelihood_torch``), and one ``SSMNaturalGradient.minimize``.  Sum(Matern52, Matern52) (d = 6, pairs
of 2d = 12), fp64, Bernoulli likelihood, 20 Gauss-Hermite points, at one of three shapes:

  a   B = 64 series, N = 10^4 points, M = 100 inducing points      (balanced: about 100 points per segment)
  b   B = 1,         N = 10^5,        M = 1000                     (one long series)
  c   B = 64,        N = 10^4,        M = 2                        (long segments: about 3300 points each)

Timed, per shape:
  * ``elbo`` forward + backward onto the leaves of ``dist_q``, fused and composed on the same model and tensors;
  * the kernel pair alone (value and adjoints), next to ``mf_lik_sparse_cvi_site_update`` (lr = 1, zeroed sites) on the same tensors -
    the one-wavefront-per-segment layout the two-pass layout is measured against;
  * one ``SSMNaturalGradient.minimize`` with and without momentum.

The variants alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the medians
(and minima) of the per-call window times are printed, then one JSON line.  Before timing, the fused and composed ELBO and gradients
are compared.  The kernel pair's achieved bytes/s counts the bytes it must move: (2d + 2) values in per point, the pair marginals
in, the workspace written and read, the three outputs.
Usage: python3 scripts/bench_svgp.py [--shape a|b|c] [--rounds R] [--window K]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import markovflow_amd as mfa  # noqa: E402
from markovflow_amd import models as MM  # noqa: E402

SHAPES = {"a": (64, 10000, 100), "b": (1, 100000, 1000), "c": (64, 10000, 2)}
ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=sorted(SHAPES), default="a")
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--window", type=int, default=10)
args = ap.parse_args()
dev = torch.device("cuda:0")
bsz, n, m = SHAPES[args.shape]
rounds, window = args.rounds, args.window
f64 = torch.float64
two_d = 12
g = torch.Generator(device=dev)
g.manual_seed(3)
x = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, n, dtype=f64, device=dev).exponential_(1.0, generator=g), dim=-1)
y = (torch.rand(bsz, n, 1, dtype=f64, device=dev, generator=g) < 0.5).to(f64)
lik = mfa.Bernoulli()
kern = mfa.Sum([mfa.Matern52(1.0, 1.0, jitter=1e-9, device=dev), mfa.Matern52(3.0, 0.5, jitter=1e-9, device=dev)], jitter=1e-9)
frac = (torch.arange(m, dtype=f64, device=dev) + 0.5) / m
z = (x[:, :1] + frac * (x[:, -1:] - x[:, :1])).contiguous()                    # evenly spaced over every series' span


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
    mfa.SSMNaturalGradient(gamma=0.1, momentum=False).minimize(lambda: model.loss((x, y)), model.dist_q)
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

with torch.no_grad():
    _, w, c, _, offsets, tiles = model._projections(x)
    pair_mean, pair_cov = (t.contiguous() for t in model._pair_marginals())
    yy = y[..., 0].contiguous()
    nat1 = torch.zeros(bsz, m + 1, two_d, dtype=f64, device=dev)
    nat2 = torch.zeros(bsz, m + 1, two_d, two_d, dtype=f64, device=dev)

    def pair():
        return MM._sparse_expectations_launch(lik, w, c, yy, offsets, tiles, pair_mean, pair_cov, True)

    def site():
        return MM.sparse_cvi_site_update_hip(lik, w, c, yy, offsets, pair_mean, pair_cov, 1.0, nat1, nat2)

    # the two kernels sum the same terms: g_cov is nat2 at lr = 1 from zeroed sites
    site()
    cov_err = float((pair()[2] - nat2).abs().max())
    assert cov_err <= 1e-10 * float(nat2.abs().max()), cov_err
    t_pair, t_site = alternate(pair, site)

for label, t in (("elbo fwd + bwd, fused", t_fused), ("elbo fwd + bwd, composed", t_composed),
                 ("mf_lik_sparse_expectations", t_pair), ("mf_lik_sparse_cvi_site_update", t_site)):
    print(f"{label:32s} median {t['median']:.3f} ms   min {t['min']:.3f} ms", flush=True)

plain, heavy = mfa.SSMNaturalGradient(gamma=0.05, momentum=False), mfa.SSMNaturalGradient(gamma=0.05, momentum=True)
t_plain, t_heavy = alternate(lambda: plain.minimize(lambda: model.loss((x, y)), model.dist_q),
                             lambda: heavy.minimize(lambda: model.loss((x, y)), model.dist_q))
final = elbo_of(True)                                   # q stayed in the domain (a failure would raise or give NaN here)
del model._fused
assert final == final, "the ELBO after the timed natural-gradient steps is NaN"

esz, row = 8, two_d * (two_d + 1) // 2 + two_d + 1
segs = bsz * (m + 1)
pair_bytes = esz * (bsz * n * (two_d + 2) + segs * (two_d + two_d * two_d) + 2 * tiles[0] * row + segs * (1 + two_d + two_d * two_d)) \
    + 8 * (bsz * (m + 2) + tiles[0] + segs + 1)
res = {
    "shape": {"name": args.shape, "B": bsz, "N": n, "M": m, "d": 6, "dtype": "float64", "likelihood": "Bernoulli",
              "nq": lik.num_gauss_hermite_points, "tiles": tiles[0]},
    "elbo_fwd_bwd_fused_ms": t_fused,
    "elbo_fwd_bwd_composed_ms": t_composed,
    "kernel_pair_ms": t_pair,
    "kernel_pair_bytes": pair_bytes,
    "kernel_pair_GBps": pair_bytes / t_pair["median"] / 1e6,
    "kernel_pair_ns_per_point": t_pair["median"] * 1e6 / (bsz * n),
    "site_kernel_ms": t_site,
    "site_kernel_ns_per_point": t_site["median"] * 1e6 / (bsz * n),
    "natgrad_minimize_ms": t_plain,
    "natgrad_minimize_momentum_ms": t_heavy,
    "fused_vs_composed_elbo_rel_diff": abs(v_fused - v_composed) / abs(v_composed),
    "fused_vs_composed_grad_max_abs_diff": grad_err,
    "rounds": rounds,
    "window": window,
}
for label, key in (("natgrad minimize", "natgrad_minimize_ms"), ("natgrad minimize, momentum", "natgrad_minimize_momentum_ms")):
    print(f"{label:32s} median {res[key]['median']:.3f} ms   min {res[key]['min']:.3f} ms")
print(f"kernel pair: {res['kernel_pair_GBps']:.1f} GB/s over {pair_bytes / 1e6:.1f} MB it must move; "
      f"{res['kernel_pair_ns_per_point']:.3f} ns per point against {res['site_kernel_ns_per_point']:.3f} of the site kernel")
print(json.dumps(res))
