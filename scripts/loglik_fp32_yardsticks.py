#!/usr/bin/env python3
"""Print tests/helpers/loglik_fp32_table.py: the float32 yardsticks of the log-likelihood gradient tests at d <= 15
(tests/helpers/loglik_fp32_cases.py has the rule).  CPU only; builds tests/host_sim/libmf_post_sim.so with hipcc when it is stale
(a minute), then a few minutes:   python scripts/loglik_fp32_yardsticks.py > tests/helpers/loglik_fp32_table.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from helpers import loglik_fp32_cases as C  # noqa: E402


def row(key, yard):
    return f"    {key!r}: {{" + ", ".join(f'"{k}": {v:.2e}' for k, v in yard.items()) + "},"


def main():
    torch.set_num_threads(1)           # one summation order, whatever the machine
    out = ['"""Float32 yardsticks of the log-likelihood gradient tests at d <= 15: the error of the kernels\' arithmetic evaluated in float32 on',
           "the CPU against a float64 reference, per tensor, the larger of 8 draws, never below 2^-24 (rule, metric and what measures",
           "what: tests/helpers/loglik_fp32_cases.py).",
           'Generated: python scripts/loglik_fp32_yardsticks.py > tests/helpers/loglik_fp32_table.py"""',
           "", "# (d, m, T, B, per_step) -> the local forms of Fisher's identity in float32 on float32-rounded exact moments", "LOCAL = {"]
    out += [row(key, C.local_yardstick(*key)) for key in C.local_keys()]
    out += ["}", "", "# (d, m, T, B, chunks, per_step) -> mf_grad_host_sim_f32 against dense autograd, the larger over the chunk lengths",
            "STREAMED = {"]
    out += [row(key, C.streamed_yardstick(*key)) for key in C.streamed_keys()]
    out += ["}", "", "# (d, m, T, B, chunks, per_step) -> mf_post_host_sim_f32 against the numpy oracle, the larger over the chunk lengths",
            "CHAIN = {"]
    out += [row(key, C.chain_yardstick(*key)) for key in C.CHAIN_CASES]
    out.append("}")
    print("\n".join(out))


if __name__ == "__main__":
    main()
