#!/usr/bin/env python3
"""Print tests/helpers/kl_fp32_table.py: the float32 yardsticks of the KL / marginals tests (tests/helpers/kl_fp32_cases.py has the
rule).  CPU only, a minute or so:   python scripts/kl_fp32_yardsticks.py > tests/helpers/kl_fp32_table.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from helpers import kl_fp32_cases as C  # noqa: E402


def fmt(x):
    return f"{x:.2e}"


def main():
    torch.set_num_threads(1)           # one summation order, whatever the machine
    out = ['"""Float32 yardsticks of the KL / marginals tests: the error of the closed forms of tests/helpers/kl_closed_forms.py evaluated in',
           "float32 on the CPU against their float64 evaluation, the larger of 8 draws, never below 2^-24 (rule and metric:",
           'tests/helpers/kl_fp32_cases.py).  Generated: python scripts/kl_fp32_yardsticks.py > tests/helpers/kl_fp32_table.py"""',
           "", "# (route, d, T, B) -> the value for q1 != q2 (kl) and q2 = q1 (kl_same); with an adjoint kernel: the ten gradients of sum_s w_s KL_s",
           "KL = {"]
    for route, shapes in C.KL_CASES.items():
        for shape in shapes:
            y = C.kl_yardstick(route, *shape)
            out.append(f"    {(route,) + shape!r}: {{" + ", ".join(f'"{k}": {fmt(v)}' for k, v in y.items()) + "},")
    out += ["}", "", "# (d, T, B) -> marginal means, covariances and the five gradients of a random linear functional of them", "MARGINALS = {"]
    for shape in C.MARGINALS_CASES:
        y = C.marginals_yardstick(*shape)
        out.append(f"    {shape!r}: {{" + ", ".join(f'"{k}": {fmt(v)}' for k, v in y.items()) + "},")
    out += ["}", "", "# (d, T, B) -> the five gradients with one of the incoming gradients absent (mf_ssm_marginals_grad: g_means / g_covs = NULL)",
            "MARGINALS_NULL = {"]
    for shape in C.MARGINALS_NULL_CASES:
        y = C.marginals_null_yardstick(*shape)
        out.append(f"    {shape!r}: {{" + ", ".join(f'"{a}": {{' + ", ".join(f'"{k}": {fmt(v)}' for k, v in row.items()) + "}" for a, row in y.items()) + "},")
    out += ["}", "", "# (d, B, T) -> mf_ssm_kl_from_moments_f32: the operator form on float32-rounded moments", "FROM_MOMENTS = {"]
    for d in C.FROM_MOMENTS_DIMS:
        out.append("    " + " ".join(f"{(d, bsz, t)!r}: {fmt(C.from_moments_yardstick(d, bsz, t))}," for bsz, t in C.FROM_MOMENTS_SHAPES))
    out += ["}", "", "# (d, B, T) -> the float32 KL of tests/test_gpu_wave.py::test_wave_marginals_and_covariance_blocks (route: walk)", "WAVE_TEST = {"]
    for i in range(0, len(C.WAVE_TEST_CASES), 6):
        out.append("    " + " ".join(f"{case!r}: {fmt(C.wave_test_yardstick(*case))}," for case in C.WAVE_TEST_CASES[i:i + 6]))
    out.append("}")
    print("\n".join(out))


if __name__ == "__main__":
    main()
