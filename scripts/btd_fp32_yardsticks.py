#!/usr/bin/env python3
"""Print tests/helpers/btd_fp32_table.py: the float32 yardsticks of the block-tridiagonal operator tests
(tests/helpers/btd_fp32_cases.py has the rule).  CPU only, a few minutes:
    python scripts/btd_fp32_yardsticks.py > tests/helpers/btd_fp32_table.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from helpers import btd_fp32_cases as C  # noqa: E402


def row(key, y):
    return f"    {key!r}: {{" + ", ".join(f'"{k}": {v:.2e}' for k, v in y.items()) + "},"


def main():
    torch.set_num_threads(1)           # one summation order, whatever the machine
    out = ['"""Float32 yardsticks of the block-tridiagonal operator tests: the error of the closed forms of',
           "tests/helpers/btd_fp32_closed_forms.py evaluated in float32 on the CPU against the sequential form in float64, the larger of 8",
           "draws and of the sequential / partitioned forms the route can evaluate, never below 2^-24 (rule, draws and plans:",
           "tests/helpers/btd_fp32_cases.py).  One kernel needed a form beyond those two: bigop_matvec_kernel (csrc/mf_bigops_impl.hpp,",
           "dense_mult at d >= 10) keeps ONE running sum per output row over up to 3 d terms, where numpy's product leaves the order to",
           "its BLAS (several partial sums): with numpy's product alone as the yardstick L x missed at (64, 12, 1); the kernel's",
           "arithmetic read off its source is the textbook dot product - so dense_mult is measured by the larger of numpy's product and",
           "btd_fp32_closed_forms.matvec_running_sum, on every route.",
           'Generated: python scripts/btd_fp32_yardsticks.py > tests/helpers/btd_fp32_table.py"""',
           "", "# (route, d, T, B) -> cholesky, symmetric dense_mult, upper_diagonal_lower without / with eta (matrix draw); solve, dense_mult,",
           "# abs_log_det, blocks of the inverse (factor draw)", "BTD = {"]
    for case in C.CASES:
        out.append(row(case, C.yardstick(*case)))
    out += ["}", "", "# (route, d, T, B) -> the same matrix without a sub-diagonal", "NO_SUB = {"]
    for case in C.NO_SUB_CASES:
        out.append(row(case, C.no_sub_yardstick(*case)))
    out += ["}", "", "# (route, d, T, B) -> mf_btd_logdet_quad_f32", "LOGDET_QUAD = {"]
    for case in C.LOGDET_QUAD_CASES:
        out.append(f"    {case!r}: {C.logdet_quad_yardstick(*case):.2e},")
    out.append("}")
    print("\n".join(out))


if __name__ == "__main__":
    main()
