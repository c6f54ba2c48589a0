"""PowerExpectationPropagation at the shape scripts/bench_cvi.py uses - B = 64 series, T = 10^4 points, Sum(Matern52, Matern52) (d = 6),
fp64, Bernoulli likelihood, 20 Gauss-Hermite points:

  * one ``update_sites()`` (filter route's posterior chain, marginals, projection, ONE ``mf_lik_pep_site_update`` launch),
  * the site-update kernel alone against the SAME update written as torch element-wise operations on the same device tensors
    (``likelihoods.torch_pep_site_update``: cavity, log-sum-exp with two derivatives over [B, T, 20] temporaries, correction,
    normaliser, step and the skip mask), and
  * ``mf_lik_cvi_site_update`` on the same marginals (N = B T points), for the ratio of the two site kernels.

The three variants of the second and third measurement alternate inside one process; medians and minima of device-event times over
the rounds are printed, then one JSON line.  Before timing, kernel and torch composition are compared on the same inputs, against
the bound of tests/test_gpu_pep_kernel.py's comparison of the two, K eps (magnitude + 1) with K = 64; the magnitudes need the test
helper, and a magnitude is at least |value|, so the stricter |difference| <= 64 eps (|value| + 1) is asserted.
Usage: python3 scripts/bench_pep.py [B] [T] [rounds]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import markovflow_amd as mfa  # noqa: E402
from markovflow_amd import likelihoods as ML  # noqa: E402

dev = torch.device("cuda:0")
bsz = int(sys.argv[1]) if len(sys.argv) > 1 else 64
tn = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 30
f64 = torch.float64
g = torch.Generator(device=dev)
g.manual_seed(3)
t_pts = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, tn, dtype=f64, device=dev).exponential_(1.0, generator=g), dim=-1)
y = (torch.rand(bsz, tn, 1, dtype=f64, device=dev, generator=g) < 0.5).to(f64)
kern = mfa.Sum([mfa.Matern52(1.0, 1.0, jitter=1e-9, device=dev), mfa.Matern52(3.0, 0.5, jitter=1e-9, device=dev)], jitter=1e-9)
lik = mfa.Bernoulli()
lr, alpha, cvi_lr = 0.5, 0.5, 0.1
model = mfa.PowerExpectationPropagation((t_pts, y), kern, lik, learning_rate=lr, alpha=alpha)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


with torch.no_grad():
    for _ in range(3):                                  # warm-up: code objects, allocator, and sites away from their start
        model.update_sites()
    fmu, fvar = model._project(model.posterior_kalman.posterior_state_space_model())
    fmu, fvar = fmu.contiguous(), fvar.contiguous()
    start = [model.sites.nat1.clone(), model.sites.nat2.clone(), model.sites.log_norm.clone()]
    # same inputs, both variants: the results must agree before their times are compared
    a = [s.clone() for s in start]
    b = [s.clone() for s in start]
    lik.pep_site_update(fmu, fvar, y, alpha, lr, *a)
    ML.torch_pep_site_update(lik, fmu, fvar, y, alpha, lr, *b)
    moved = float((a[0] - start[0]).abs().max())
    assert moved > 0.0, "the update moved nothing"
    eps = 2.0 ** -52
    err = max(float(((p - q).abs() / (q.abs() + 1.0)).max()) for p, q in zip(a, b))
    assert err <= 64.0 * eps, err
    c1, c2 = start[0].clone(), start[1].clone()
    t_kernel, t_torch, t_cvi, t_update = [], [], [], []

    def reset(sites):
        for s, s0 in zip(sites, start):                 # every timed call starts from the same sites: no drift towards a skip
            s.copy_(s0)

    for _ in range(3):
        lik.pep_site_update(fmu, fvar, y, alpha, lr, *a)
        ML.torch_pep_site_update(lik, fmu, fvar, y, alpha, lr, *b)
        lik.cvi_site_update(fmu, fvar, y, cvi_lr, c1, c2)
    for _ in range(rounds):                             # alternating, one process
        reset(a)
        reset(b)
        c1.copy_(start[0])
        c2.copy_(start[1])
        t_kernel.append(timed(lambda: lik.pep_site_update(fmu, fvar, y, alpha, lr, *a)))
        t_torch.append(timed(lambda: ML.torch_pep_site_update(lik, fmu, fvar, y, alpha, lr, *b)))
        t_cvi.append(timed(lambda: lik.cvi_site_update(fmu, fvar, y, cvi_lr, c1, c2)))
    for _ in range(max(rounds // 3, 5)):
        t_update.append(timed(model.update_sites))
    float(model.elbo())                                 # the sites stayed in the domain (a failure would raise here)
    energy = model.energy()
    assert bool(torch.isfinite(energy).all())


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts)}


res = {
    "shape": {"B": bsz, "T": tn, "d": 6, "dtype": "float64", "likelihood": "Bernoulli", "nq": lik.num_gauss_hermite_points,
              "alpha": alpha, "learning_rate": lr},
    "update_sites_ms": stats(t_update),
    "pep_site_kernel_ms": stats(t_kernel),
    "torch_composition_ms": stats(t_torch),
    "cvi_site_kernel_ms": stats(t_cvi),
    "pep_over_cvi_kernel": statistics.median(t_kernel) / statistics.median(t_cvi),
    "torch_over_kernel": statistics.median(t_torch) / statistics.median(t_kernel),
    "kernel_vs_torch_max_scaled_diff_eps": err / eps,
    "rounds": rounds,
}
for label, key in (("update_sites()", "update_sites_ms"), ("mf_lik_pep_site_update", "pep_site_kernel_ms"),
                   ("torch composition", "torch_composition_ms"), ("mf_lik_cvi_site_update", "cvi_site_kernel_ms")):
    print(f"{label:26s}median {res[key]['median']:.3f} ms   min {res[key]['min']:.3f} ms")
print(json.dumps(res))
