"""SparseVariationalGaussianProcess with a trainable likelihood parameter: the kernel pair that reads the parameter from device memory
and returns the adjoint onto it (``mf_lik_sparse_expectations_theta``) against the pair that takes it as a host double
(``mf_lik_sparse_expectations``) on the same tensors.  B = 64 series, N = 10^4 points, M = 100 inducing points,
Sum([Matern52, Matern32, Matern12]) (2d = 12); Gaussian with a variance per series and Student-t (df = 3) with a scale per series.

Timed, per likelihood:
  * ``elbo`` forward + backward onto the leaves of ``dist_q`` AND the likelihood's leaf, fused and composed on the same model (float64);
  * per dtype (float64, then float32 on the same tensors cast down), alternating in one process: the theta pair with all four outputs,
    and the float pair (value and pair adjoints, the parameter one host double for all series) at the same tile table.

Expectation, recorded before the first run: the theta pair adds one LDS row, one accumulator entry and 8 bytes per
workspace row to the float pair and no traffic besides, so it should cost about what the float pair costs (ratio about 1.0).

The variants alternate in windows of ``--window`` calls between two device events; after warm-up windows the medians (and minima) of
the per-call window times are printed, then one JSON line.  Before timing, the two pairs and the two routes are compared.
Usage: python3 scripts/bench_theta.py [--rounds R] [--window K] [--batch B] [--points N] [--inducing M]"""
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
y = (torch.sin(7.0 * (x - x[:, :1]) / span) + 0.3 * torch.randn(bsz, n, dtype=f64, device=dev, generator=g))[..., None]


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


def kernel():
    return mfa.Sum([mfa.Matern52(1.0, 1.0, jitter=1e-9, device=dev), mfa.Matern32(3.0, 0.7, jitter=1e-9, device=dev),
                    mfa.Matern12(2.0, 0.5, jitter=1e-9, device=dev)])


start = torch.linspace(0.3, 0.6, bsz, dtype=f64, device=dev)          # one value per series
CASES = {"gaussian": (lambda t: mfa.Gaussian(variance=t)), "student-t": (lambda t: mfa.StudentT(scale=t, df=3.0))}
res = {"shape": {"B": bsz, "N": n, "M": m}, "rounds": rounds, "window": window, "cases": {}}
for tag, make in CASES.items():
    lik = make(start)
    model = mfa.SparseVariationalGaussianProcess(kernel(), lik, z)
    for _ in range(2):                                  # a q away from the prior
        mfa.SSMNaturalGradient(gamma=0.05, momentum=False).minimize(lambda: model.loss((x, y)), model.dist_q)
    leaves = tuple(model.trainable_variables) + lik.trainable_variables

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
    print(f"{tag} {'elbo fwd + bwd, fused':40s} median {t_fused['median']:.3f} ms   min {t_fused['min']:.3f} ms", flush=True)
    print(f"{tag} {'elbo fwd + bwd, composed':40s} median {t_composed['median']:.3f} ms   min {t_composed['min']:.3f} ms", flush=True)
    case = {"elbo_fwd_bwd_fused_ms": t_fused, "elbo_fwd_bwd_composed_ms": t_composed, "fused_vs_composed_elbo_rel_diff": elbo_rel,
            "fused_vs_composed_grad_max_abs_diff": grad_err, "composed_over_fused": t_composed["median"] / t_fused["median"]}
    with torch.no_grad():
        order, w64, c64, _, offsets, tiles = model._projections(x)
        pm64, pc64 = (t.contiguous() for t in model._pair_marginals())
        y64 = y[..., 0] if order is None else torch.gather(y[..., 0], -1, order)
    case["tiles"], case["two_d"] = tiles[0], w64.shape[-1]
    shared = make(0.45)                                 # the float form: one host double for all series
    for dtype, name, tol in ((torch.float64, "float64", 1e-10), (torch.float32, "float32", 1e-3)):
        w, c, pair_mean, pair_cov, yy = (t.to(dtype).contiguous() for t in (w64, c64, pm64, pc64, y64))
        th, th_shared = start.to(dtype), torch.tensor(0.45, dtype=dtype, device=dev)

        def theta_pair(theta=th):
            with torch.no_grad():
                return MM._sparse_theta_expectations_launch(lik, theta, w, c, yy, offsets, tiles, pair_mean, pair_cov, True, True)

        def float_pair():
            with torch.no_grad():
                return MM._sparse_expectations_launch(shared, w, c, yy, offsets, tiles, pair_mean, pair_cov, True)

        for a, b, what in zip(theta_pair(th_shared), float_pair(), ("ve_sum", "g_mean", "g_cov")):      # the same numbers at one value
            err, scale = float((a - b).abs().max()), float(b.abs().max())
            assert err <= tol * scale, (tag, name, what, err, scale)
        t_theta, t_float = alternate(theta_pair, float_pair)
        for label, t in (("mf_lik_sparse_expectations_theta", t_theta), ("mf_lik_sparse_expectations", t_float)):
            print(f"{tag} {name} {label:36s} median {t['median']:.3f} ms   min {t['min']:.3f} ms", flush=True)
        print(f"{tag} {name} theta pair: {t_theta['median'] * 1e6 / (bsz * n):.3f} ns per point, {t_theta['median'] / t_float['median']:.3f} x "
              "the float pair", flush=True)
        case[name] = {"theta_pair_ms": t_theta, "float_pair_ms": t_float, "theta_pair_ns_per_point": t_theta["median"] * 1e6 / (bsz * n),
                      "theta_over_float": t_theta["median"] / t_float["median"]}
    res["cases"][tag] = case
    del model, w64, c64
print(json.dumps(res))
