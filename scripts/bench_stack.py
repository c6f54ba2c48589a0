"""SparseVariationalGaussianProcess with MultiStageLikelihood on STACKED chains (``IndependentMultiOutputStack``): the stacked data
term (``mf_lik_stack_expectations``) against its torch composition, against the concatenated data term
(``mf_lik_sparse_multi_expectations`` on ``IndependentMultiOutput``) and the two models' training steps against each other.
20 Gauss-Hermite points, B = 64 series, N = 10^4 points, M = 100 inducing points, observations drawn with ``sample_y``.

Timed, alternating in one process:
  (a) per dtype: ``mf_lik_stack_expectations`` at K = 3, three Matern-3/2 (2d = 4), value and adjoints, against
      ``sparse_stack_expected_log_likelihood_torch`` forward + backward onto the pair marginals;
  (b) per dtype, in the same alternation: ``mf_lik_sparse_multi_expectations`` on ``IndependentMultiOutput([Matern32] * 3)`` (2d = 12),
      the same data and hyper-parameters;
  (c) float64: ``elbo`` forward + backward onto the leaves of ``dist_q`` of the stacked model against the concatenated model;
  (d) float64: the same step of the stacked model at three Matern-5/2 (2d = 6) and at three sums of three Matern-5/2 (2d = 18 per
      latent, 54 concatenated: a model the concatenated route cannot fuse).

The variants alternate in windows of ``--window`` calls between two device events; after warm-up windows the medians (and minima) of
the per-call window times are printed, then one JSON line.  Before timing, the stacked kernel is compared with its composition, and
the stacked ELBO at the prior with the concatenated one.
Usage: python3 scripts/bench_stack.py [--rounds R] [--window K] [--batch B] [--points N] [--inducing M]"""
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
latents = 3
g = torch.Generator(device=dev)
g.manual_seed(3)
x = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, n, dtype=f64, device=dev).exponential_(1.0, generator=g), dim=-1)
lik = mfa.MultiStageLikelihood()
span = x[:, -1:] - x[:, :1]
phase = (x - x[:, :1]) / span
latent = torch.stack([0.8 * torch.sin(9.0 * phase) - 0.2, torch.cos(6.0 * phase), 0.9 + 0.6 * torch.sin(4.0 * phase + 1.0)], dim=-1)
y = lik.sample_y(latent, generator=g)
HYPER = ((1.0, 1.0), (3.0, 0.7), (0.5, 1.3))
frac = (torch.arange(m, dtype=f64, device=dev) + 0.5) / m
z = (x[:, :1] + frac * span).contiguous()                                      # evenly spaced over every series' span
xs = x[:, None, :].expand(bsz, latents, n).contiguous()                        # the stacked layout: the same times on every chain
zs = z[:, None, :].expand(bsz, latents, m).contiguous()


def children(cls, repeat=1):
    one = lambda ls, var: cls(ls, var / repeat, jitter=1e-9, device=dev)      # noqa: E731
    return [one(ls, var) if repeat == 1 else mfa.Sum([one(ls * (1.0 + 0.3 * r), var) for r in range(repeat)]) for ls, var in HYPER]


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


def show(label, t):
    print(f"{label:58s} median {t['median']:.3f} ms   min {t['min']:.3f} ms", flush=True)


stacked = mfa.SparseVariationalGaussianProcess(mfa.IndependentMultiOutputStack(children(mfa.Matern32), jitter=1e-9), lik, zs)
concat = mfa.SparseVariationalGaussianProcess(mfa.IndependentMultiOutput(children(mfa.Matern32), jitter=1e-9), lik, z)
with torch.no_grad():
    v_stacked, v_concat = float(stacked.elbo((xs, y))), float(concat.elbo((x, y)))
assert abs(v_stacked - v_concat) <= 1e-9 * abs(v_concat), (v_stacked, v_concat)          # at the prior the two models are one
for model, xy in ((stacked, (xs, y)), (concat, (x, y))):                                # a q away from the prior
    for _ in range(2):
        mfa.SSMNaturalGradient(gamma=0.05, momentum=False).minimize(lambda: model.loss(xy), model.dist_q)


def step_of(model, xy):
    leaves = model.trainable_variables
    return lambda: torch.autograd.grad(model.elbo(xy), leaves)


res = {"shape": {"B": bsz, "N": n, "M": m, "latents": latents, "likelihood": "MultiStageLikelihood", "nq": lik.num_gauss_hermite_points},
       "rounds": rounds, "window": window, "stacked_vs_concatenated_elbo_at_prior_rel_diff": abs(v_stacked - v_concat) / abs(v_concat)}

# (a) and (b): the kernels alone
with torch.no_grad():
    _, ws64, cs64, indices_s, offsets_s, tiles_s, shared = stacked._projections(xs)
    pms64, pcs64 = (t.contiguous() for t in stacked._pair_marginals())
    _, wc64, cc64, _, offsets_c, tiles_c = concat._projections(x)
    pmc64, pcc64 = (t.contiguous() for t in concat._pair_marginals())
assert shared and tiles_s[0] == tiles_c[0]
offsets0 = offsets_s[..., 0, :].contiguous()
res["shape"]["tiles"] = tiles_s[0]
for dtype, name, tol in ((torch.float64, "float64", 1e-10), (torch.float32, "float32", 1e-3)):
    ws, cs, pms, pcs, wc, cc, pmc, pcc = (t.to(dtype).contiguous() for t in (ws64, cs64, pms64, pcs64, wc64, cc64, pmc64, pcc64))
    yy = y[..., 0].to(dtype).contiguous()

    def stack_pair():
        with torch.no_grad():
            return MM.segmented_ops._sparse_stack_expectations_launch(lik, ws, cs, yy, offsets0, tiles_s, pms, pcs, True)

    def concat_pair():
        with torch.no_grad():
            return MM._sparse_multi_expectations_launch(lik, wc, cc, yy, offsets_c, tiles_c, pmc, pcc, True)

    def composed():
        pm, pc = pms.clone().requires_grad_(True), pcs.clone().requires_grad_(True)
        value = MM.sparse_stack_expected_log_likelihood_torch(lik, ws, cs, yy, indices_s, pm, pc)
        return (value,) + torch.autograd.grad(value.sum(), (pm, pc))

    for a, b, what in zip(stack_pair(), composed(), ("ve_sum", "g_mean", "g_cov")):
        err, scale = float((a - b.detach()).abs().max()), float(b.detach().abs().max())
        assert err <= tol * scale, (name, what, err, scale)
    t_stack, t_torch, t_concat = alternate(stack_pair, composed, concat_pair)
    show(f"{name} mf_lik_stack_expectations (K = 3, 2d = 4)", t_stack)
    show(f"{name} torch composition, fwd + bwd", t_torch)
    show(f"{name} mf_lik_sparse_multi_expectations (2d = 12)", t_concat)
    print(f"{name}: stacked / concatenated {t_stack['median'] / t_concat['median']:.2f}, "
          f"{t_torch['median'] / t_stack['median']:.1f} x faster than the composition", flush=True)
    res[name] = {"stack_kernel_ms": t_stack, "torch_composition_ms": t_torch, "concatenated_kernel_ms": t_concat,
                 "stack_over_concatenated": t_stack["median"] / t_concat["median"],
                 "composition_over_stack": t_torch["median"] / t_stack["median"]}

# (c): the training step of the two models
t_s, t_c = alternate(step_of(stacked, (xs, y)), step_of(concat, (x, y)))
show("elbo fwd + bwd, stacked (3 x Matern32, 2d = 4)", t_s)
show("elbo fwd + bwd, concatenated (2d = 12)", t_c)
res["elbo_fwd_bwd_stacked_ms"], res["elbo_fwd_bwd_concatenated_ms"] = t_s, t_c
res["elbo_stacked_over_concatenated"] = t_s["median"] / t_c["median"]
del stacked, concat, ws64, cs64, wc64, cc64

# (d): larger latents
for label, key, kids in (("3 x Matern52, 2d = 6", "elbo_fwd_bwd_stacked_m52_ms", children(mfa.Matern52)),
                         ("3 x Sum of 3 Matern52, 2d = 18", "elbo_fwd_bwd_stacked_2d18_ms", children(mfa.Matern52, repeat=3))):
    model = mfa.SparseVariationalGaussianProcess(mfa.IndependentMultiOutputStack(kids, jitter=1e-9), lik, zs)
    mfa.SSMNaturalGradient(gamma=0.05, momentum=False).minimize(lambda: model.loss((xs, y)), model.dist_q)
    (t_d,) = alternate(step_of(model, (xs, y)))
    show(f"elbo fwd + bwd, stacked ({label})", t_d)
    res[key] = t_d
    del model
print(json.dumps(res))
