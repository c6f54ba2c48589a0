"""The accuracy yardsticks of tests/test_gpu_st_cvi_kernel.py, measured on the CPU: the error of ``st_cvi_site_update_torch`` in the
dtype under test against tests/helpers/st_cvi_closed_forms.py one precision up (float64 for float32, numpy.longdouble for float64),
on inputs drawn as the test draws them, from zero sites at ``lr = 1`` and from random symmetric sites at ``lr = 0.3``, for ``nat1``,
``nat2`` and ``ve_sum``, normalised element by element by eps x the output's magnitude, maximised over the elements, the series and
8 seeds (the test's own inputs and seven more draws), floored at 1.

    python scripts/st_cvi_yardsticks.py [--jobs J]   # prints every figure and rewrites tests/golden/st_cvi_yardsticks.json
"""
import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from markovflow_amd import models                             # noqa: E402
from helpers import likelihood_closed_forms as L              # noqa: E402
from helpers import st_cvi_closed_forms as STC                # noqa: E402
import st_yardsticks as Y                                     # noqa: E402
import test_gpu_st_cvi_kernel as C                            # noqa: E402

K = C.K
SEEDS = Y.SEEDS


def torch_outputs(name, ref, dtype, lr, sites):
    """``nat1``, ``nat2`` and ``ve_sum`` of the torch composition, on all the series of ``ref`` at once."""
    t = lambda v: torch.tensor(v, dtype=dtype)        # noqa: E731
    indices = models._segments_of(torch.tensor(ref["offsets"]), ref["a"].shape[-2])
    nat1, nat2 = t(sites[0]), t(sites[1])
    ve_sum, _, _ = models.st_cvi_site_update_torch(Y.LIKS[name](), *[t(ref[k]) for k in ("a", "wt", "c", "y")], indices,
                                                   t(ref["pair_mean"]), t(ref["pair_cov"]), lr, nat1, nat2)
    return dict(nat1=nat1.numpy(), nat2=nat2.numpy(), ve_sum=ve_sum.numpy())


def measure(case):
    ms, dt, name = case
    torch.set_num_threads(1)
    rows = {}
    for dtype, up in ((torch.float64, np.longdouble), (torch.float32, np.float64)):
        f32 = dtype == torch.float32
        worst = {start: {k: 1.0 for k in C.CHECKED} for start in C.STARTS}
        # the test's own inputs and seven more draws of the same kind
        for seed in [K.case_seed(ms, dt, 20)] + [7919 * s + 100 * ms + dt for s in range(1, SEEDS)]:
            ref = K.draw_inputs(ms, dt, name, f32, C.LAYOUT, seed)
            sums = [STC.st_cvi_site_sums(L.LIKELIHOODS[name], ref["a"][b], ref["wt"][b], ref["c"][b], ref["y"][b], ref["offsets"][b],
                                         ref["pair_mean"][b], ref["pair_cov"][b], 20, up) for b in range(len(C.LAYOUT))]
            for start in C.STARTS:
                lr, sites = C.learning_rate(start, f32), C.draw_sites(ms, dt, f32, C.LAYOUT, seed, start)
                got = torch_outputs(name, ref, dtype, lr, sites)
                for b in range(len(C.LAYOUT)):
                    want = {**sums[b], **STC.blend(sums[b], lr, sites[0][b], sites[1][b], up)}
                    for k in C.CHECKED:
                        err = np.abs((got[k][b].astype(up) - want[k]).astype(np.float64))
                        mag = np.asarray(want["mag_" + k])
                        scaled = np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), 0.0) / K.EPS[dtype]
                        worst[start][k] = max(worst[start][k], float(scaled.max()))
        for start in C.STARTS:
            rows[C.yard_key(ms, dt, dtype, name, start)] = {k: round(v, 3) for k, v in worst[start].items()}
    return rows


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--jobs", type=int, default=4)
    table = {}
    with ProcessPoolExecutor(max_workers=parser.parse_args().jobs) as pool:
        for rows in pool.map(measure, C.CASES):
            for key, row in rows.items():
                table[key] = row
                print(key, row, flush=True)
    with open(C.YARD_FILE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
