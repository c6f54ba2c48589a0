"""SparseVariationalGaussianProcess with a FactorAnalysisKernel: the multi-output data term fused
(``mf_lik_sparse_factor_expectations``) against composed (``models.sparse_factor_expected_log_likelihood_torch``) and beside the
single-latent pair.  FactorAnalysisKernel([Matern52, Matern32]) (d = 5, pairs of 2d = 10, L = 2 latents), A(t) = phase(t) (x) A0 with
a trainable loading matrix, P = 5 and P = 32 observed series, Gaussian and Poisson likelihoods, B = 64 series, N = 10^4 points,
M = 100 inducing points.

Timed, per P and likelihood:
  * ``elbo`` forward + backward onto the leaves of ``dist_q`` AND the loading matrix, fused and composed on the same model and tensors
    (float64: the model);
  * per dtype (float64, then float32 on the same tensors cast down), alternating in one process:
      - the kernel pair alone: value, pair adjoints and g_w;
      - ``sparse_factor_expected_log_likelihood_torch`` forward + backward onto the pair marginals and the mixing weights, the
        composition it replaces, on the same device;
      - ``mf_lik_sparse_expectations`` (one latent, one output, the same likelihood) at the same N, tile table and 2d = 10: row 0 of
        ``wg`` and entry (0, 0) of ``cg``.

Expectation, recorded before the first run: per point the work is L projections of the pair plus P likelihood evaluations, so at
P = 5 the Gaussian case should sit near the single-latent pair's time at the same 2d.  No speed-up is fixed in advance.

The variants alternate in windows of ``--window`` calls between two device events; after warm-up windows the medians (and minima) of
the per-call window times are printed, then one JSON line.  Before timing, fused and composed results are compared.
Usage: python3 scripts/bench_factor_analysis.py [--rounds R] [--window K] [--batch B] [--points N] [--inducing M] [--outputs 5,32]"""
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
ap.add_argument("--outputs", type=str, default="5,32")
args = ap.parse_args()
dev = torch.device("cuda:0")
bsz, n, m = args.batch, args.points, args.inducing
rounds, window = args.rounds, args.window
f64 = torch.float64
two_d, latents = 10, 2
g = torch.Generator(device=dev)
g.manual_seed(3)
x = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, n, dtype=f64, device=dev).exponential_(1.0, generator=g), dim=-1)
span = x[:, -1:] - x[:, :1]
x0 = x[:, :1].contiguous()
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


res = {"shape": {"B": bsz, "N": n, "M": m, "d": 5, "latents": latents, "two_d": two_d}, "rounds": rounds, "window": window, "cases": {}}
for outputs in [int(p) for p in args.outputs.split(",")]:
    a0 = 0.4 * torch.randn(outputs, latents, dtype=f64, device=dev, generator=g)

    def weights(t, a0=a0):
        """A(t) = (0.5 + phase(t)) (x) A0: the notebook's weight function on the series' own span."""
        a = a0.to(t.dtype)
        return (0.5 + (t - x0.to(t.dtype)) / span.to(t.dtype))[..., None, None] * a

    latent = torch.stack([torch.sin(9.0 * (x - x0) / span), 0.8 * torch.cos(6.0 * (x - x0) / span)], dim=-1)
    f = (weights(x) @ latent[..., None])[..., 0]                                 # [B, N, P]
    for lik_name, lik in (("gaussian", mfa.Gaussian(0.3)), ("poisson", mfa.Poisson())):
        if lik_name == "gaussian":
            y = f + 0.3 ** 0.5 * torch.randn(f.shape, dtype=f64, device=dev, generator=g)
        else:
            y = torch.poisson(torch.exp(f), generator=g)
        kern = mfa.FactorAnalysisKernel(weights, [mfa.Matern52(1.0, 1.0, jitter=1e-9, device=dev), mfa.Matern32(3.0, 0.7, jitter=1e-9, device=dev)],
                                        output_dim=outputs, jitter=1e-9)
        model = mfa.SparseVariationalGaussianProcess(kern, lik, z)
        for _ in range(2):                              # a q away from the prior
            mfa.SSMNaturalGradient(gamma=0.05, momentum=False).minimize(lambda: model.loss((x, y)), model.dist_q)
        leaves = tuple(model.trainable_variables) + (kern.loading_matrix,)

        def step(fused):
            if fused:
                model.__dict__.pop("_fused", None)
            else:
                model._fused = lambda t: False
            return torch.autograd.grad(model.elbo((x, y)), leaves)

        def elbo_of(fused):
            if fused:
                model.__dict__.pop("_fused", None)
            else:
                model._fused = lambda t: False
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
        model.__dict__.pop("_fused", None)
        tag = f"P={outputs} {lik_name}"
        print(f"{tag} {'elbo fwd + bwd, fused':40s} median {t_fused['median']:.3f} ms   min {t_fused['min']:.3f} ms", flush=True)
        print(f"{tag} {'elbo fwd + bwd, composed':40s} median {t_composed['median']:.3f} ms   min {t_composed['min']:.3f} ms", flush=True)
        case = {"elbo_fwd_bwd_fused_ms": t_fused, "elbo_fwd_bwd_composed_ms": t_composed,
                "fused_vs_composed_elbo_rel_diff": abs(v_fused - v_composed) / abs(v_composed),
                "fused_vs_composed_grad_max_abs_diff": grad_err}
        with torch.no_grad():
            _, wg64, cg64, indices, offsets, tiles = model._projections(x)
            pm64, pc64 = (t.contiguous() for t in model._pair_marginals())
            mix64 = kern.mixing_weights(x).contiguous()
        case["tiles"] = tiles[0]
        for dtype, name, tol in ((torch.float64, "float64", 1e-10), (torch.float32, "float32", 1e-3)):
            wg, cg, mix, pair_mean, pair_cov, yy = (t.to(dtype).contiguous() for t in (wg64, cg64, mix64, pm64, pc64, y))
            w1, c1, y1 = wg[..., 0, :].contiguous(), cg[..., 0, 0].contiguous(), yy[..., 0].contiguous()

            def pair():
                with torch.no_grad():
                    return MM._sparse_factor_expectations_launch(lik, wg, cg, mix, yy, offsets, tiles, pair_mean, pair_cov, True, True)

            def single():
                with torch.no_grad():
                    return MM._sparse_expectations_launch(lik, w1, c1, y1, offsets, tiles, pair_mean, pair_cov, True)

            def composed():
                pm, pc, mx = (t.clone().requires_grad_(True) for t in (pair_mean, pair_cov, mix))
                value = MM.sparse_factor_expected_log_likelihood_torch(lik, wg, cg, mx, yy, indices, pm, pc)
                return (value,) + torch.autograd.grad(value.sum(), (pm, pc, mx))

            for a, b, what in zip(pair(), composed(), ("ve_sum", "g_mean", "g_cov", "g_w")):
                err, scale = float((a - b.detach()).abs().max()), float(b.detach().abs().max())
                assert err <= tol * scale, (tag, name, what, err, scale)
            t_pair, t_torch, t_single = alternate(pair, composed, single)
            for label, t in (("mf_lik_sparse_factor_expectations", t_pair), ("torch composition, fwd + bwd", t_torch),
                             ("mf_lik_sparse_expectations (one latent)", t_single)):
                print(f"{tag} {name} {label:40s} median {t['median']:.3f} ms   min {t['min']:.3f} ms", flush=True)
            print(f"{tag} {name} pair: {t_pair['median'] * 1e6 / (bsz * n):.3f} ns per point, {t_pair['median'] / t_single['median']:.2f} x "
                  f"the single-latent pair, {t_torch['median'] / t_pair['median']:.1f} x faster than the composition", flush=True)
            case[name] = {"kernel_pair_ms": t_pair, "torch_composition_ms": t_torch, "single_latent_pair_ms": t_single,
                          "kernel_pair_ns_per_point": t_pair["median"] * 1e6 / (bsz * n),
                          "factor_over_single": t_pair["median"] / t_single["median"],
                          "composition_over_pair": t_torch["median"] / t_pair["median"]}
        res["cases"][tag] = case
        del model, wg64, cg64, mix64
print(json.dumps(res))
