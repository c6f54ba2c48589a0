#!/usr/bin/env python3
"""Print tests/helpers/generator_fp_table.py: the float32 and float64 yardsticks of the generator checks at every time gap
(tests/helpers/generator_fp_cases.py has the rule, the metrics and the assumption about the device's exp / sin / cos).  CPU only
(numpy and mpmath), a few minutes; fails when a squared pivot of the CPU evaluation falls below 0.9 jitter for any draw, gap or
component kind:   python scripts/generator_fp_yardsticks.py > tests/helpers/generator_fp_table.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from helpers import generator_fp_cases as C  # noqa: E402


def row(key, yard):
    return f"    {key!r}: {{" + ", ".join(f'"{k}": {v:.2e}' for k, v in yard.items()) + "},"


def main():
    out = ['"""Yardsticks of the generator checks at every time gap: the error of the arithmetic of csrc/mf_sde.hip evaluated in the dtype',
           f"on the CPU against mpmath at 80 digits, per step and tensor, the larger of {C.SEEDS} draws and of exp / sin / cos moved by",
           f"{C.ULP_NUDGE} ulp, never below 2^-24 (f32) / 2^-53 (f64) (rule and metrics: tests/helpers/generator_fp_cases.py).",
           'Generated: python scripts/generator_fp_yardsticks.py > tests/helpers/generator_fp_table.py"""',
           "", "# (dtype, order, osc, gap) -> {tensor: yardstick}; Q0: Q at jitter 0, everything else at the jitter of the dtype",
           "GENERATOR = {"]
    out += [row(key, C.yardstick(*key)) for key in C.keys()]
    out += ["}", "", "# (dtype, order) -> the gradient of chol(Pinf + jitter I) (mf_sde_matern_prior_chol_grad)", "PRIOR = {"]
    out += [row((dt_name, order), C.prior_yardstick(dt_name, order)) for dt_name in C.DTYPES for order in C.PRIOR_ORDERS]
    out += ["}", "", "# (outputs, signature) -> the float64 log-likelihood of oracle.numpy_oracle on the float64 closed forms against the",
            "# exact Gaussian log density of the chain, relative to |value|", "GPR = {"]
    out += [f"    {sig!r}: {C.gpr_yardstick(sig):.2e}," for sig in C.GPR_SIGNATURES]
    out.append("}")
    print("\n".join(out))


if __name__ == "__main__":
    main()
