"""SpatioTemporalSparseVariational at the shape of BASELINE config 5's chain - one series of N = 10^5 points, Ms = 32 spatial inducing
points, temporal Matern32 (D = Ms d_t = 64, pairs of dimension 128), Mt = 100 inducing times, Bernoulli likelihood, 20 Gauss-Hermite
nodes, in float64 and float32:

  (a) ``mf_lik_st_expectations`` (value, the adjoints onto the pair marginals, the per-point adjoints: one call) against
      ``models.st_expected_log_likelihood_torch`` forward plus backward on the same inputs, the value-only call, and the kernel's
      achieved FMA rate against 4 N (2D)^2 flops with its minimal traffic,
  (b) ``elbo()`` plus ``backward()`` per step on the fused route and on the composed route (``_fused`` patched), and its other parts
      on their own: the pair marginals forward plus backward, the KL term forward plus backward - at the largest model the chain
      operators carry in the dtype: the marginals, their adjoint and the KL reach state dimension 64 in float32 and 32 in float64,
      so (b) runs at Ms = 32 (D = 64) in float32 and at Ms = 16 (D = 32) in float64 (``--model-space`` overrides both), and (a)
      takes its pair marginals from a random positive definite draw.

The variants alternate inside one process in windows of ``--window`` calls between two device events; after warm-up windows the
medians (and minima) of the per-call window times are printed, then one JSON line.  Before timing, kernel and composition are
compared on the same inputs.
Usage: python3 scripts/bench_st.py [--points N] [--space Ms] [--model-space Ms] [--inducing Mt] [--rounds R] [--window W]"""
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


def timed(fn):
    """Per-call time of a window of calls between two device events, in ms."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(window):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / window


def alternate(variants):
    """Two warm-up windows, then ``rounds`` alternating windows of every variant: ``{name: {median, min}}``."""
    for _ in range(2):
        for fn in variants.values():
            timed(fn)
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
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
    model = mfa.SpatioTemporalSparseVariational(z_space, z_time, SK.Matern32(1.0, 0.7, device=dev, dtype=dtype),
                                                mfa.Matern32(5.0, 1.0, jitter=1e-6, device=dev, dtype=dtype), lik)
    return model, (inputs, obs), g


def measure(dtype):
    model, (inputs, obs), g = build(dtype, ms)
    order, a, wt, c, indices, offsets, tiles = model._projections(inputs)
    assert order is None
    y = obs[..., 0].contiguous()
    pair = 2 * model.kernel.state_dim
    root = torch.randn(mt + 1, pair, pair, dtype=dtype, device=dev, generator=g)
    pair_cov = (root @ root.transpose(-1, -2) / pair + 0.1 * torch.eye(pair, dtype=dtype, device=dev)).contiguous()
    pair_mean = torch.randn(mt + 1, pair, dtype=dtype, device=dev, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (pair_mean, pair_cov, a, wt, c)]

    def fused():
        for leaf in leaves:
            leaf.grad = None
        MM.st_expected_log_likelihood(lik, leaves[2], leaves[3], leaves[4], y, offsets, leaves[0], leaves[1], tiles=tiles).sum().backward()

    def composed():
        for leaf in leaves:
            leaf.grad = None
        MM.st_expected_log_likelihood_torch(lik, leaves[2], leaves[3], leaves[4], y, indices, leaves[0], leaves[1]).sum().backward()

    def grads_of(fn):
        fn()
        return [leaf.grad.clone() for leaf in leaves]

    rel = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(grads_of(fused), grads_of(composed))]
    assert max(rel) < (1e-9 if dtype == torch.float64 else 2e-3), rel
    # (b): the largest model the chain operators carry in this dtype
    model, xy, _ = build(dtype, args.model_space or (ms if dtype == torch.float32 else min(ms, 16)))

    def launch(value=False, grads=False, point=False):
        return lambda: MM._st_expectations_launch(lik, a, wt, c, y, offsets, tiles, pair_mean, pair_cov, value, grads, point)

    def step():
        for leaf in model.trainable_variables:
            leaf.grad = None
        model.elbo(xy).backward()

    def composed_step():
        model._fused = lambda inputs_: False
        try:
            step()
        finally:
            del model._fused

    _, a_b, wt_b, c_b, _, offsets_b, tiles_b = model._projections(xy[0])
    y_b = xy[1][..., 0].contiguous()
    with torch.no_grad():
        pm_b, pc_b = (t.contiguous() for t in model._pair_marginals())
    g_pm, g_pc = torch.ones_like(pm_b), torch.ones_like(pc_b)

    def data_term():
        MM._st_expectations_launch(lik, a_b, wt_b, c_b, y_b, offsets_b, tiles_b, pm_b, pc_b, True, True, False)

    def marginals_fwd_bwd():
        for leaf in model.trainable_variables:
            leaf.grad = None
        torch.autograd.backward(model._pair_marginals(), (g_pm, g_pc))

    def kl_fwd_bwd():
        for leaf in model.trainable_variables:
            leaf.grad = None
        model.dist_q.kl_divergence(model.dist_p).sum().backward()

    res = {"dtype": str(dtype).split(".")[-1], "kernel_vs_torch_rel_diff": rel, "model_D": model.kernel.state_dim}
    res["kernel"] = alternate({"kernel_all_outputs_ms": launch(True, True, True), "kernel_value_and_pair_adjoints_ms": launch(True, True),
                               "kernel_value_only_ms": launch(True), "fused_fwd_bwd_ms": fused, "torch_composition_fwd_bwd_ms": composed})
    res["step"] = alternate({"fused_elbo_backward_ms": step, "composed_elbo_backward_ms": composed_step, "data_term_kernel_ms": data_term,
                             "pair_marginals_fwd_bwd_ms": marginals_fwd_bwd, "kl_fwd_bwd_ms": kl_fwd_bwd})
    esize = a.element_size()
    rows = tiles[0]
    res["flops"] = 4 * n * pair * pair
    res["tflops"] = res["flops"] / (res["kernel"]["kernel_all_outputs_ms"]["median"] * 1e-3) / 1e12
    # inputs once, the pair covariance once per group of 64 points and both ways, the workspace written and read, the outputs
    groups = (n + 63) // 64 + (mt + 1)
    res["bytes"] = esize * (n * (2 * (ms + wt.shape[-1]) + 3) + groups * 2 * pair * pair + 2 * rows * (pair * (pair + 1) // 2 + pair + 1)
                            + (mt + 1) * (pair * pair + pair + 1))
    res["gb_per_s"] = res["bytes"] / (res["kernel"]["kernel_all_outputs_ms"]["median"] * 1e-3) / 1e9
    res["data_term_share_of_fused_step"] = res["step"]["data_term_kernel_ms"]["median"] / res["step"]["fused_elbo_backward_ms"]["median"]
    for group in ("kernel", "step"):
        for key, val in res[group].items():
            print(f"{res['dtype']:8s} {key:36s} median {val['median']:9.3f} ms   min {val['min']:9.3f} ms")
    print(f"{res['dtype']:8s} kernel: {res['tflops']:.2f} TFLOP/s of 4 N (2D)^2, {res['gb_per_s']:.0f} GB/s of its traffic; the data term is "
          f"{100 * res['data_term_share_of_fused_step']:.0f} % of a fused elbo() + backward()")
    return res


out = {"shape": {"N": n, "Ms": ms, "Mt": mt, "D": 2 * ms, "likelihood": "Bernoulli", "nodes": lik.num_gauss_hermite_points},
       "rounds": rounds, "window": window, "runs": [measure(torch.float64), measure(torch.float32)]}
print(json.dumps(out))          # (one line: what CHANGELOG.md quotes)
