"""VariationalGaussianProcess at the shape the sibling scripts use - B = 64 series, N = 10^4 points, Sum(Matern52, Matern52) (d = 6),
fp64, Bernoulli likelihood, 20 Gauss-Hermite nodes:

  (a) the kernel pair ``mf_lik_dense_expectations`` + ``mf_lik_dense_expectations_adjoint`` (value, two derivatives per point, their
      expansion onto the marginals) against ``models.dense_expected_log_likelihood_torch`` forward plus backward on the same marginals,
      and each kernel on its own,
  (b) ``elbo()`` plus ``backward()`` per step on the fused route and on the composed route (``_fused`` patched), and its other parts on
      their own: ``dist_q.marginals`` forward plus backward, the KL term forward plus backward,
  (c) ``CVIGaussianProcess.update_sites()`` at the same N and ``SparseVariationalGaussianProcess.elbo()`` plus ``backward()`` with
      ``--inducing`` inducing points on the same data, for context.

The variants alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the
medians (and minima) of the per-call window times are printed, then one JSON line.  Before timing, kernel pair and composition are
compared on the same inputs.  Achieved bytes per second are the kernels' MINIMAL traffic over their time: the expectations kernel reads
d^2 + 2 d + 1 values per point (covs, means, h, y) and writes 2; the adjoint reads d + 2 and writes d^2 + d.
Usage: python3 scripts/bench_vgp.py [--batch B] [--points N] [--inducing M] [--rounds R] [--window W]"""
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
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--window", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
bsz, n, m, rounds, window = args.batch, args.points, args.inducing, args.rounds, args.window
f64 = torch.float64
g = torch.Generator(device=dev)
g.manual_seed(3)
x = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, n, dtype=f64, device=dev).exponential_(1.0, generator=g), dim=-1)
y = (torch.rand(bsz, n, 1, dtype=f64, device=dev, generator=g) < 0.5).to(f64)
frac = (torch.arange(m, dtype=f64, device=dev) + 0.5) / m
z = (x[:, :1] + frac * (x[:, -1:] - x[:, :1])).contiguous()                    # evenly spaced over every series' span
lik = mfa.Bernoulli()


def kernel_sum():
    return mfa.Sum([mfa.Matern52(1.0, 1.0, jitter=1e-9, device=dev), mfa.Matern52(3.0, 0.5, jitter=1e-9, device=dev)], jitter=1e-9)


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


def alternate(variants):
    """Two warm-up windows, then ``rounds`` alternating windows of every variant: ``{name: stats}``."""
    for _ in range(2):
        for fn in variants.values():
            timed(fn)
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    return {name: stats(ts) for name, ts in times.items()}


xy = (x, y)
model = mfa.VariationalGaussianProcess(xy, kernel_sum(), lik)
cvi = mfa.CVIGaussianProcess(xy, kernel_sum(), lik, learning_rate=0.5)
svgp = mfa.SparseVariationalGaussianProcess(kernel_sum(), lik, z)
d = model.kernel.state_dim
h, yy = model._h, model._y
with torch.no_grad():
    means, covs = (t.contiguous() for t in model.dist_q.marginals)
weight = torch.ones(bsz, dtype=f64, device=dev)

# (a) the same inputs, both variants: the results must agree before their times are compared
m_leaf, p_leaf = means.clone().requires_grad_(True), covs.clone().requires_grad_(True)
fused_value = MM.dense_expected_log_likelihood(lik, h, yy, m_leaf, p_leaf)
fused_grads = torch.autograd.grad(fused_value.sum(), (m_leaf, p_leaf))
torch_value = MM.dense_expected_log_likelihood_torch(lik, h, yy, m_leaf, p_leaf)
torch_grads = torch.autograd.grad(torch_value.sum(), (m_leaf, p_leaf))
err_v = float((fused_value.detach() - torch_value.detach()).abs().max() / torch_value.detach().abs().max())
err_g = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(fused_grads, torch_grads))
assert err_v < 1e-12 and err_g < 1e-10, (err_v, err_g)
del fused_grads, torch_grads, fused_value, torch_value

lib = MM._lib.load()
ws_bytes = int(lib.mf_lik_dense_expectations_workspace_bytes(bsz, n, 8))
ws = MM._lib.workspace(ws_bytes, dev)
ve_sum = torch.empty(bsz, dtype=f64, device=dev)
g_mu, g_var = torch.empty(bsz, n, dtype=f64, device=dev), torch.empty(bsz, n, dtype=f64, device=dev)
g_means, g_covs = torch.empty_like(means), torch.empty_like(covs)
ptr, stream = MM._lib.ptr, MM._lib.stream_ptr(dev)


def expectations():
    MM._lib.call("mf_lik_dense_expectations", f64, bsz, n, d, *lik._kernel_args(), ptr(h), ptr(means), ptr(covs), ptr(yy), ptr(ws),
                 ws_bytes, ptr(ve_sum), ptr(g_mu), ptr(g_var), stream)


def adjoint():
    MM._lib.call("mf_lik_dense_expectations_adjoint", f64, bsz, n, d, ptr(h), ptr(g_mu), ptr(g_var), ptr(weight), ptr(g_means),
                 ptr(g_covs), stream)


def pair():
    expectations()
    adjoint()


def composed():
    m_leaf.grad = p_leaf.grad = None
    MM.dense_expected_log_likelihood_torch(lik, h, yy, m_leaf, p_leaf).sum().backward()


def step_of(mod, *data):
    def step():
        for leaf_ in mod.trainable_variables:
            leaf_.grad = None
        mod.elbo(*data).backward()
    return step


fused_step, svgp_step = step_of(model), step_of(svgp, xy)


def composed_step():
    model._fused = lambda: False
    try:
        fused_step()
    finally:
        del model._fused


def marginals_fwd_bwd():
    for leaf_ in model.trainable_variables:
        leaf_.grad = None
    mm, cc = model.dist_q.marginals
    torch.autograd.backward((mm, cc), (g_means, g_covs))


def kl_fwd_bwd():
    for leaf_ in model.trainable_variables:
        leaf_.grad = None
    model.dist_q.kl_divergence(model.dist_p).sum().backward()


with torch.no_grad():
    expectations()
res = {"shape": {"B": bsz, "N": n, "M": m, "d": d, "dtype": "float64", "likelihood": "Bernoulli", "nodes": lik.num_gauss_hermite_points},
       "rounds": rounds, "window": window, "kernel_vs_torch_rel_diff": {"value": err_v, "adjoint": err_g}}
res["kernel"] = alternate({"kernel_pair_ms": pair, "expectations_ms": expectations, "adjoint_ms": adjoint, "torch_composition_ms": composed})
res["step"] = alternate({"fused_elbo_backward_ms": fused_step, "composed_elbo_backward_ms": composed_step,
                         "marginals_fwd_bwd_ms": marginals_fwd_bwd, "kl_fwd_bwd_ms": kl_fwd_bwd, "cvi_update_sites_ms": cvi.update_sites,
                         "svgp_elbo_backward_ms": svgp_step})
points = bsz * n
res["expectations_min_bytes"] = points * (d * d + 2 * d + 1 + 2) * 8
res["adjoint_min_bytes"] = points * (d + 2 + d * d + d) * 8
res["expectations_gb_per_s"] = res["expectations_min_bytes"] / (res["kernel"]["expectations_ms"]["median"] * 1e-3) / 1e9
res["adjoint_gb_per_s"] = res["adjoint_min_bytes"] / (res["kernel"]["adjoint_ms"]["median"] * 1e-3) / 1e9
step = res["step"]
res["data_term_share_of_fused_step"] = res["kernel"]["kernel_pair_ms"]["median"] / step["fused_elbo_backward_ms"]["median"]
for group in ("kernel", "step"):
    for key, val in res[group].items():
        print(f"{key:28s} median {val['median']:9.3f} ms   min {val['min']:9.3f} ms")
print(f"expectations: {res['expectations_gb_per_s']:.0f} GB/s of its minimal traffic; adjoint: {res['adjoint_gb_per_s']:.0f} GB/s; the kernel "
      f"pair is {100 * res['data_term_share_of_fused_step']:.0f} % of a fused elbo() + backward()")
print(json.dumps(res))
