"""The accuracy yardsticks of tests/test_gpu_st_kernel.py, measured on the CPU: the error of ``st_expected_log_likelihood_torch`` (value
and autograd gradients) and of the torch route of ``st_point_marginals`` in the dtype under test against
tests/helpers/st_closed_forms.py one precision up (float64 for float32, numpy.longdouble for float64), on inputs drawn as the test
draws them, normalised element by element by eps x the output's magnitude, maximised over the elements, the series and 8 seeds (the test's own
inputs and seven more draws), floored at 1.

    python scripts/st_yardsticks.py            # prints every figure and rewrites tests/golden/st_yardsticks.json
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import markovflow_amd as mfa                                  # noqa: E402
from markovflow_amd import models                             # noqa: E402
from helpers import likelihood_closed_forms as L              # noqa: E402
from helpers import st_closed_forms as ST                     # noqa: E402
import test_gpu_st_kernel as K                                # noqa: E402

SEEDS = 8
LIKS = {L.GAUSSIAN: lambda: mfa.Gaussian(0.7), L.BERNOULLI: mfa.Bernoulli, L.POISSON: mfa.Poisson,
        L.STUDENTT: lambda: mfa.StudentT(1.3, 3.5)}


def torch_outputs(name, ref, dtype, nq):
    """Every output of the kernel from the torch composition, on all the series of ``ref`` at once."""
    t = lambda k, grad=False: torch.tensor(ref[k], dtype=dtype).requires_grad_(grad)        # noqa: E731
    a, wt, c, pm, pc = (t(k, True) for k in ("a", "wt", "c", "pair_mean", "pair_cov"))
    offsets = torch.tensor(ref["offsets"])
    indices = models._segments_of(offsets, a.shape[-2])
    lik = LIKS[name]() if name in (L.GAUSSIAN, L.POISSON) else (mfa.StudentT(1.3, 3.5, nq) if name == L.STUDENTT else mfa.Bernoulli(nq))
    ve = models.st_expected_log_likelihood_torch(lik, a, wt, c, t("y"), indices, pm, pc)
    grads = torch.autograd.grad(ve.sum(), (pm, pc, a, wt, c))
    fmu, fvar = models.st_point_marginals(a.detach(), wt.detach(), c.detach(), offsets, pm.detach(), pc.detach())
    names = ("ve_sum", "g_mean", "g_cov", "g_a", "g_wt", "g_c", "fmu", "fvar")
    return dict(zip(names, [x.detach().numpy() for x in (ve,) + grads + (fmu, fvar)]))


def main():
    table = {}
    cases = [(ms, dt, name, 20) for ms, dt, name in K.CASES] + [(5, 3, L.STUDENTT, nq) for nq in K.OTHER_NQ]
    for ms, dt, name, nq in cases:
        for dtype, tag, up in ((torch.float64, "f64", np.longdouble), (torch.float32, "f32", np.float64)):
            worst = {k: 1.0 for k in K.OUTS}
            # the test's own inputs and seven more draws of the same kind
            for seed in [K.case_seed(ms, dt, nq)] + [7919 * s + 100 * ms + dt for s in range(1, SEEDS)]:
                ref = K.draw_inputs(ms, dt, name, dtype == torch.float32, K.LAYOUT, seed)
                got = torch_outputs(name, ref, dtype, nq)
                for b in range(len(K.LAYOUT)):
                    want = ST.st_expectations(L.LIKELIHOODS[name], ref["a"][b], ref["wt"][b], ref["c"][b], ref["y"][b],
                                              ref["offsets"][b], ref["pair_mean"][b], ref["pair_cov"][b], nq, up)
                    for k in K.OUTS:
                        err = np.abs((got[k][b].astype(up) - want[k]).astype(np.float64))
                        mag = np.asarray(want["mag_" + k])
                        scaled = np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), 0.0) / K.EPS[dtype]
                        worst[k] = max(worst[k], float(scaled.max()))
            key = K.yard_key(ms, dt, dtype, name, nq)
            table[key] = {k: round(v, 3) for k, v in worst.items()}
            print(key, table[key], flush=True)
    with open(K.YARD_FILE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
