"""SparseVariationalGaussianProcess under a MultivariateGaussian likelihood: the correlated-noise data term fused
(``mf_lik_sparse_mvn_expectations``) against composed (``models.sparse_mvn_expected_log_likelihood_torch``) and beside the factor
pair.  B = 64 series, N = 10^4 points, M = 100 inducing points; P = 2 on IndependentMultiOutput([Matern52, Matern32]) (2d = 10) and
P = 4 on IndependentMultiOutput([Matern52, Matern32, Matern32, Matern12]) (2d = 16); a non-diagonal trainable Cholesky factor.

Timed, per P:
  * ``elbo`` forward + backward onto the leaves of ``dist_q`` AND the Cholesky factor, fused and composed on the same model (float64);
  * per dtype (float64, then float32 on the same tensors cast down), alternating in one process:
      - the kernel pair alone: value, pair adjoints and m_sum;
      - ``sparse_mvn_expected_log_likelihood_torch`` forward + backward onto the pair marginals and the factor, on the same device;
      - ``mf_lik_sparse_factor_expectations`` (Gaussian, L = P latents mixed by the identity: the same projections, P scalar
        likelihoods instead of one joint one) at the same N, tile table and 2d.

Expectation, recorded before the first run: the pair does the factor pair's projection and reduction without its
chunked walk over the outputs, so it should sit at or a little below the factor pair's time at L = P.  No speed-up is fixed in advance.

The variants alternate in windows of ``--window`` calls between two device events; after warm-up windows the medians (and minima) of
the per-call window times are printed, then one JSON line.  Before timing, fused and composed results are compared.
Usage: python3 scripts/bench_mvn.py [--rounds R] [--window K] [--batch B] [--points N] [--inducing M]"""
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
g = torch.Generator(device=dev)
g.manual_seed(3)
x = torch.cumsum(0.05 + 0.05 * torch.empty(bsz, n, dtype=f64, device=dev).exponential_(1.0, generator=g), dim=-1)
span = x[:, -1:] - x[:, :1]
z = (x[:, :1] + (torch.arange(m, dtype=f64, device=dev) + 0.5) / m * span).contiguous()
phase = (x - x[:, :1]) / span


def timed(fn):
    """Per-call time of a window of calls between two device events, in ms."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(window):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / window


def alternate(*fns):
    out = [[] for _ in fns]
    for _ in range(2):                                  # warm-up windows
        for fn in fns:
            timed(fn)
    for _ in range(rounds):                             # alternating, one process
        for ts, fn in zip(out, fns):
            ts.append(timed(fn))
    return [{"median": statistics.median(ts), "min": min(ts)} for ts in out]


def matern(order, ls, var):
    return {5: mfa.Matern52, 3: mfa.Matern32, 1: mfa.Matern12}[order](ls, var, jitter=1e-9, device=dev)


CASES = {2: [(5, 1.0, 1.0), (3, 3.0, 0.7)], 4: [(5, 1.0, 1.0), (3, 3.0, 0.7), (3, 0.8, 1.2), (1, 2.0, 0.9)]}
res = {"shape": {"B": bsz, "N": n, "M": m}, "rounds": rounds, "window": window, "cases": {}}
for outputs, children in CASES.items():
    kern = mfa.IndependentMultiOutput([matern(*c) for c in children])
    two_d = 2 * kern.state_dim
    chol = (0.5 * torch.eye(outputs, dtype=f64, device=dev) + torch.tril(0.2 * torch.randn(outputs, outputs, dtype=f64, device=dev, generator=g), -1))
    latent = torch.stack([torch.sin((5.0 + 2.0 * p) * phase + p) for p in range(outputs)], dim=-1)
    y = latent + (torch.randn(latent.shape, dtype=f64, device=dev, generator=g)[..., None, :] @ chol.T)[..., 0, :]
    leaf = chol.clone().requires_grad_(True)
    lik = mfa.MultivariateGaussian(leaf)
    model = mfa.SparseVariationalGaussianProcess(kern, lik, z)
    for _ in range(2):                                  # a q away from the prior
        mfa.SSMNaturalGradient(gamma=0.05, momentum=False).minimize(lambda: model.loss((x, y)), model.dist_q)
    leaves = tuple(model.trainable_variables) + (leaf,)

    def step(fused):
        if fused:
            model.__dict__.pop("_fused", None)
        else:
            model._fused = lambda t: False
        value = model.elbo((x, y))
        return (value.detach(),) + torch.autograd.grad(value, leaves)

    # same model, both routes: the results must agree before their times are compared
    r_fused, r_composed = step(True), step(False)
    elbo_rel = abs(float(r_fused[0]) - float(r_composed[0])) / abs(float(r_composed[0]))
    grad_err = max(float((a - b).abs().max()) for a, b in zip(r_fused[1:], r_composed[1:]))
    grad_scale = max(float(b.abs().max()) for b in r_composed[1:])
    assert elbo_rel <= 1e-9 and grad_err <= 1e-8 * grad_scale, (elbo_rel, grad_err, grad_scale)
    t_fused, t_composed = alternate(lambda: step(True), lambda: step(False))
    model.__dict__.pop("_fused", None)
    tag = f"P={outputs} 2d={two_d}"
    print(f"{tag} {'elbo fwd + bwd, fused':40s} median {t_fused['median']:.3f} ms   min {t_fused['min']:.3f} ms", flush=True)
    print(f"{tag} {'elbo fwd + bwd, composed':40s} median {t_composed['median']:.3f} ms   min {t_composed['min']:.3f} ms", flush=True)
    case = {"elbo_fwd_bwd_fused_ms": t_fused, "elbo_fwd_bwd_composed_ms": t_composed, "fused_vs_composed_elbo_rel_diff": elbo_rel,
            "fused_vs_composed_grad_max_abs_diff": grad_err}
    with torch.no_grad():
        _, w64, c64, indices, offsets, tiles = model._projections(x)
        pm64, pc64 = (t.contiguous() for t in model._pair_marginals())
    case["tiles"] = tiles[0]
    gauss = mfa.Gaussian(0.3)
    for dtype, name, tol in ((torch.float64, "float64", 1e-10), (torch.float32, "float32", 1e-3)):
        w, c, pair_mean, pair_cov, yy = (t.to(dtype).contiguous() for t in (w64, c64, pm64, pc64, y))
        lik_t = mfa.MultivariateGaussian(chol.to(dtype))
        prec = lik_t.precision(w).contiguous()
        mix = torch.eye(outputs, dtype=dtype, device=dev).expand(bsz, n, outputs, outputs).contiguous()

        def pair():
            with torch.no_grad():
                return MM._sparse_mvn_expectations_launch(lik_t, w, c, yy, prec, offsets, tiles, pair_mean, pair_cov, True, True)

        def factor():
            with torch.no_grad():
                return MM._sparse_factor_expectations_launch(gauss, w, c, mix, yy, offsets, tiles, pair_mean, pair_cov, True, False)

        def composed():
            pm, pc, lf = (t.clone().requires_grad_(True) for t in (pair_mean, pair_cov, chol.to(dtype)))
            value = MM.sparse_mvn_expected_log_likelihood_torch(mfa.MultivariateGaussian(lf), w, c, yy, indices, pm, pc)
            return (value,) + torch.autograd.grad(value.sum(), (pm, pc, lf))

        counts = (offsets[..., 1:] - offsets[..., :-1]).to(dtype)
        quad_sum, g_mean, g_cov, _ = pair()
        value, r_mean, r_cov, _ = composed()
        for a, b, what in ((-0.5 * (quad_sum + counts * lik_t.log_normaliser(w)), value, "ve_sum"), (g_mean, r_mean, "g_mean"),
                           (g_cov, r_cov, "g_cov")):
            err, scale = float((a - b.detach()).abs().max()), float(b.detach().abs().max())
            assert err <= tol * scale, (tag, name, what, err, scale)
        t_pair, t_torch, t_factor = alternate(pair, composed, factor)
        for label, t in (("mf_lik_sparse_mvn_expectations", t_pair), ("torch composition, fwd + bwd", t_torch),
                         ("mf_lik_sparse_factor_expectations (L = P)", t_factor)):
            print(f"{tag} {name} {label:42s} median {t['median']:.3f} ms   min {t['min']:.3f} ms", flush=True)
        print(f"{tag} {name} pair: {t_pair['median'] * 1e6 / (bsz * n):.3f} ns per point, {t_pair['median'] / t_factor['median']:.2f} x "
              f"the factor pair, {t_torch['median'] / t_pair['median']:.1f} x faster than the composition", flush=True)
        case[name] = {"kernel_pair_ms": t_pair, "torch_composition_ms": t_torch, "factor_pair_ms": t_factor,
                      "kernel_pair_ns_per_point": t_pair["median"] * 1e6 / (bsz * n),
                      "mvn_over_factor": t_pair["median"] / t_factor["median"],
                      "composition_over_pair": t_torch["median"] / t_pair["median"]}
    res["cases"][tag] = case
    del model, w64, c64
print(json.dumps(res))
