"""CVIGaussianProcess at the shape scripts/prof_cvi.py uses - B = 64 series, T = 10^4 points, Sum(Matern52, Matern52) (d = 6), fp64,
Bernoulli likelihood, 20 Gauss-Hermite points:

  * one ``update_sites()`` (filter route's posterior chain, marginals, projection, ONE ``mf_lik_cvi_site_update`` launch), and
  * the site-update kernel alone against the SAME update written as torch element-wise operations on the same device tensors
    (``likelihoods.torch_variational_expectations`` + the two in-place axpy's: about forty launches over [B, T, 20] temporaries).

The two variants of the second measurement alternate inside one process; medians and minima of device-event times over the rounds
are printed, then one JSON line.  Before timing, the two variants are compared on the same inputs.
Usage: python3 scripts/bench_cvi.py [B] [T] [rounds]"""
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
lr = 0.1
model = mfa.CVIGaussianProcess((t_pts, y), kern, lik, learning_rate=lr)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def torch_site_update(fmu, fvar, obs, nat1, nat2):
    _, g_mu, g_var = ML.torch_variational_expectations(lik, fmu, fvar, obs)
    nat1.mul_(1.0 - lr).add_(lr * (g_mu - 2.0 * g_var * fmu))
    nat2.mul_(1.0 - lr).add_(lr * g_var.reshape(nat2.shape))


with torch.no_grad():
    for _ in range(3):                                  # warm-up: code objects, allocator, and sites away from their start
        model.update_sites()
    fmu, fvar = model._project(model.posterior_kalman.posterior_state_space_model())
    fmu, fvar = fmu.contiguous(), fvar.contiguous()
    # same inputs, both variants: the results must agree before their times are compared
    a1, a2 = model.sites.nat1.clone(), model.sites.nat2.clone()
    b1, b2 = a1.clone(), a2.clone()
    lik.cvi_site_update(fmu, fvar, y, lr, a1, a2)
    torch_site_update(fmu, fvar, y, b1, b2)
    err = max(float((a1 - b1).abs().max()), float((a2 - b2).abs().max()))
    scale = max(float(b1.abs().max()), float(b2.abs().max()))
    assert err <= 1e-12 * scale, (err, scale)
    n1, n2 = a1, a2
    t_kernel, t_torch, t_update = [], [], []
    for _ in range(3):
        lik.cvi_site_update(fmu, fvar, y, lr, n1, n2)
        torch_site_update(fmu, fvar, y, b1, b2)
    for _ in range(rounds):                             # alternating, one process
        t_kernel.append(timed(lambda: lik.cvi_site_update(fmu, fvar, y, lr, n1, n2)))
        t_torch.append(timed(lambda: torch_site_update(fmu, fvar, y, b1, b2)))
    for _ in range(max(rounds // 3, 5)):
        t_update.append(timed(model.update_sites))
    float(model.elbo())                                 # the sites stayed in the domain (a failure would raise here)

res = {
    "shape": {"B": bsz, "T": tn, "d": 6, "dtype": "float64", "likelihood": "Bernoulli", "nq": lik.num_gauss_hermite_points},
    "update_sites_ms": {"median": statistics.median(t_update), "min": min(t_update)},
    "site_kernel_ms": {"median": statistics.median(t_kernel), "min": min(t_kernel)},
    "torch_composition_ms": {"median": statistics.median(t_torch), "min": min(t_torch)},
    "kernel_vs_torch_max_abs_diff": err,
    "rounds": rounds,
}
print(f"update_sites()            median {res['update_sites_ms']['median']:.3f} ms   min {res['update_sites_ms']['min']:.3f} ms")
print(f"mf_lik_cvi_site_update    median {res['site_kernel_ms']['median']:.3f} ms   min {res['site_kernel_ms']['min']:.3f} ms")
print(f"torch composition         median {res['torch_composition_ms']['median']:.3f} ms   min {res['torch_composition_ms']['min']:.3f} ms")
print(json.dumps(res))
