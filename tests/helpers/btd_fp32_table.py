"""Float32 yardsticks of the block-tridiagonal operator tests: the error of the closed forms of
tests/helpers/btd_fp32_closed_forms.py evaluated in float32 on the CPU against the sequential form in float64, the larger of 8
draws and of the sequential / partitioned forms the route can evaluate, never below 2^-24 (rule, draws and plans:
tests/helpers/btd_fp32_cases.py).  One kernel needed a form beyond those two: bigop_matvec_kernel (csrc/mf_bigops_impl.hpp,
dense_mult at d >= 10) keeps ONE running sum per output row over up to 3 d terms, where numpy's product leaves the order to
its BLAS (several partial sums): with numpy's product alone as the yardstick L x missed at (64, 12, 1); the kernel's
arithmetic read off its source is the textbook dot product - so dense_mult is measured by the larger of numpy's product and
btd_fp32_closed_forms.matvec_running_sum, on every route.
Generated: python scripts/btd_fp32_yardsticks.py > tests/helpers/btd_fp32_table.py"""

# (route, d, T, B) -> cholesky, symmetric dense_mult, upper_diagonal_lower without / with eta (matrix draw); solve, dense_mult,
# abs_log_det, blocks of the inverse (factor draw)
BTD = {
    ('sweep', 1, 1, 3): {"chol.diag": 5.96e-08, "sym.mult": 5.96e-08, "mult": 5.96e-08, "mult_t": 5.96e-08, "solve": 5.96e-08, "solve_t": 5.96e-08, "logdet": 5.96e-08, "inv.diag": 6.83e-08},
    ('sweep', 3, 4, 3): {"chol.diag": 6.04e-08, "sym.mult": 1.18e-07, "chol.sub": 1.64e-07, "udl.u_t": 1.17e-07, "udl.chol_d": 5.96e-08, "eta.u_t": 1.17e-07, "eta.chol_d": 5.96e-08, "eta.m_post": 1.74e-07, "eta.chol_dinv": 8.12e-08, "mult": 8.79e-08, "mult_t": 1.02e-07, "solve": 8.23e-08, "solve_t": 1.22e-07, "logdet": 1.04e-07, "inv.diag": 1.51e-07, "inv.sub": 2.12e-07},
    ('sweep', 6, 63, 2): {"chol.diag": 6.90e-08, "sym.mult": 2.24e-07, "chol.sub": 1.52e-07, "udl.u_t": 3.28e-07, "udl.chol_d": 7.95e-08, "eta.u_t": 3.28e-07, "eta.chol_d": 7.95e-08, "eta.m_post": 1.77e-07, "eta.chol_dinv": 1.83e-07, "mult": 1.65e-07, "mult_t": 1.76e-07, "solve": 1.52e-07, "solve_t": 1.95e-07, "logdet": 6.14e-08, "inv.diag": 1.77e-07, "inv.sub": 2.20e-07},
    ('sweep', 9, 17, 2): {"chol.diag": 6.43e-08, "sym.mult": 3.49e-07, "chol.sub": 2.09e-07, "udl.u_t": 3.28e-07, "udl.chol_d": 1.44e-07, "eta.u_t": 3.28e-07, "eta.chol_d": 1.44e-07, "eta.m_post": 5.07e-07, "eta.chol_dinv": 3.67e-07, "mult": 1.55e-07, "mult_t": 1.66e-07, "solve": 1.60e-07, "solve_t": 1.82e-07, "logdet": 1.03e-07, "inv.diag": 2.27e-07, "inv.sub": 3.02e-07},
    ('sweep', 2, 64, 4096): {"chol.diag": 5.96e-08, "sym.mult": 1.66e-07, "chol.sub": 1.37e-07, "udl.u_t": 1.98e-07, "udl.chol_d": 6.42e-08, "eta.u_t": 1.98e-07, "eta.chol_d": 6.42e-08, "eta.m_post": 2.71e-07, "eta.chol_dinv": 1.82e-07, "mult": 1.20e-07, "mult_t": 1.64e-07, "solve": 2.16e-07, "solve_t": 1.22e-07, "logdet": 1.84e-07, "inv.diag": 1.99e-07, "inv.sub": 1.45e-07},
    ('lane_par', 1, 64, 1): {"chol.diag": 5.96e-08, "sym.mult": 1.10e-07, "chol.sub": 5.96e-08, "udl.u_t": 1.43e-07, "udl.chol_d": 5.96e-08, "eta.u_t": 1.43e-07, "eta.chol_d": 5.96e-08, "eta.m_post": 1.64e-07, "eta.chol_dinv": 8.31e-08, "mult": 6.00e-08, "mult_t": 1.02e-07, "solve": 6.30e-08, "solve_t": 6.63e-08, "logdet": 6.92e-08, "inv.diag": 1.40e-07, "inv.sub": 1.80e-07},
    ('lane_par', 3, 70, 2): {"chol.diag": 7.35e-08, "sym.mult": 1.33e-07, "chol.sub": 1.21e-07, "udl.u_t": 2.47e-07, "udl.chol_d": 5.96e-08, "eta.u_t": 2.47e-07, "eta.chol_d": 5.96e-08, "eta.m_post": 1.98e-07, "eta.chol_dinv": 1.37e-07, "mult": 1.09e-07, "mult_t": 1.26e-07, "solve": 8.92e-08, "solve_t": 1.08e-07, "logdet": 5.96e-08, "inv.diag": 1.32e-07, "inv.sub": 1.74e-07},
    ('lane_par', 4, 209, 1): {"chol.diag": 5.98e-08, "sym.mult": 2.33e-07, "chol.sub": 1.36e-07, "udl.u_t": 2.16e-07, "udl.chol_d": 6.71e-08, "eta.u_t": 2.16e-07, "eta.chol_d": 6.71e-08, "eta.m_post": 2.13e-07, "eta.chol_dinv": 1.18e-07, "mult": 1.57e-07, "mult_t": 1.14e-07, "solve": 1.11e-07, "solve_t": 9.81e-08, "logdet": 7.26e-08, "inv.diag": 1.21e-07, "inv.sub": 1.87e-07},
    ('lane_par', 2, 777, 3): {"chol.diag": 6.14e-08, "sym.mult": 1.28e-07, "chol.sub": 1.04e-07, "udl.u_t": 1.48e-07, "udl.chol_d": 8.52e-08, "eta.u_t": 1.48e-07, "eta.chol_d": 8.52e-08, "eta.m_post": 1.95e-07, "eta.chol_dinv": 1.59e-07, "mult": 1.11e-07, "mult_t": 9.18e-08, "solve": 9.84e-08, "solve_t": 8.77e-08, "logdet": 7.10e-08, "inv.diag": 1.34e-07, "inv.sub": 1.50e-07},
    ('row_par', 5, 65, 1): {"chol.diag": 5.96e-08, "sym.mult": 2.94e-07, "chol.sub": 1.44e-07, "udl.u_t": 1.90e-07, "udl.chol_d": 6.08e-08, "eta.u_t": 1.90e-07, "eta.chol_d": 6.08e-08, "eta.m_post": 1.89e-07, "eta.chol_dinv": 1.26e-07, "mult": 1.31e-07, "mult_t": 1.68e-07, "solve": 1.05e-07, "solve_t": 1.16e-07, "logdet": 8.33e-08, "inv.diag": 1.27e-07, "inv.sub": 1.99e-07},
    ('row_par', 6, 64, 1): {"chol.diag": 6.64e-08, "sym.mult": 1.71e-07, "chol.sub": 1.65e-07, "udl.u_t": 2.13e-07, "udl.chol_d": 6.92e-08, "eta.u_t": 2.13e-07, "eta.chol_d": 6.92e-08, "eta.m_post": 2.37e-07, "eta.chol_dinv": 1.68e-07, "mult": 1.47e-07, "mult_t": 1.74e-07, "solve": 1.35e-07, "solve_t": 1.84e-07, "logdet": 5.96e-08, "inv.diag": 1.62e-07, "inv.sub": 2.94e-07},
    ('row_par', 7, 70, 2): {"chol.diag": 7.17e-08, "sym.mult": 2.00e-07, "chol.sub": 1.68e-07, "udl.u_t": 2.23e-07, "udl.chol_d": 8.31e-08, "eta.u_t": 2.23e-07, "eta.chol_d": 8.31e-08, "eta.m_post": 2.87e-07, "eta.chol_dinv": 1.47e-07, "mult": 1.50e-07, "mult_t": 1.70e-07, "solve": 2.02e-07, "solve_t": 1.64e-07, "logdet": 1.20e-07, "inv.diag": 1.67e-07, "inv.sub": 1.86e-07},
    ('row_par', 9, 209, 1): {"chol.diag": 6.44e-08, "sym.mult": 3.69e-07, "chol.sub": 2.17e-07, "udl.u_t": 3.01e-07, "udl.chol_d": 1.05e-07, "eta.u_t": 3.01e-07, "eta.chol_d": 1.05e-07, "eta.m_post": 3.56e-07, "eta.chol_dinv": 1.76e-07, "mult": 2.06e-07, "mult_t": 2.11e-07, "solve": 2.50e-07, "solve_t": 2.32e-07, "logdet": 5.96e-08, "inv.diag": 1.97e-07, "inv.sub": 2.81e-07},
    ('row', 10, 2, 3): {"chol.diag": 5.96e-08, "sym.mult": 1.96e-07, "chol.sub": 1.98e-07, "udl.u_t": 1.79e-07, "udl.chol_d": 8.72e-08, "eta.u_t": 1.79e-07, "eta.chol_d": 8.72e-08, "eta.m_post": 4.44e-07, "eta.chol_dinv": 1.46e-07, "mult": 1.32e-07, "mult_t": 1.59e-07, "solve": 1.23e-07, "solve_t": 1.65e-07, "logdet": 1.36e-07, "inv.diag": 1.42e-07, "inv.sub": 2.53e-07},
    ('row', 15, 15, 1): {"chol.diag": 1.08e-07, "sym.mult": 2.66e-07, "chol.sub": 3.98e-07, "udl.u_t": 5.74e-07, "udl.chol_d": 1.37e-07, "eta.u_t": 5.74e-07, "eta.chol_d": 1.37e-07, "eta.m_post": 1.05e-06, "eta.chol_dinv": 3.63e-07, "mult": 2.07e-07, "mult_t": 2.62e-07, "solve": 2.67e-07, "solve_t": 2.18e-07, "logdet": 6.81e-08, "inv.diag": 2.15e-07, "inv.sub": 2.97e-07},
    ('row', 12, 80, 2): {"chol.diag": 7.45e-08, "sym.mult": 2.99e-07, "chol.sub": 3.29e-07, "udl.u_t": 3.98e-07, "udl.chol_d": 1.27e-07, "eta.u_t": 3.98e-07, "eta.chol_d": 1.27e-07, "eta.m_post": 1.19e-06, "eta.chol_dinv": 2.19e-07, "mult": 2.97e-07, "mult_t": 3.54e-07, "solve": 2.85e-07, "solve_t": 2.70e-07, "logdet": 1.11e-07, "inv.diag": 2.54e-07, "inv.sub": 3.01e-07},
    ('row', 15, 70, 1): {"chol.diag": 9.63e-08, "sym.mult": 2.76e-07, "chol.sub": 4.78e-07, "udl.u_t": 6.49e-07, "udl.chol_d": 1.49e-07, "eta.u_t": 6.49e-07, "eta.chol_d": 1.53e-07, "eta.m_post": 1.63e-06, "eta.chol_dinv": 9.52e-07, "mult": 2.45e-07, "mult_t": 2.76e-07, "solve": 2.95e-07, "solve_t": 3.10e-07, "logdet": 8.31e-08, "inv.diag": 3.73e-07, "inv.sub": 4.46e-07},
    ('tile', 12, 1, 2): {"chol.diag": 5.96e-08, "sym.mult": 1.80e-07, "mult": 9.19e-08, "mult_t": 1.09e-07, "solve": 2.87e-07, "solve_t": 1.55e-07, "logdet": 7.98e-08, "inv.diag": 1.76e-07},
    ('wave', 16, 9, 3): {"chol.diag": 6.97e-08, "sym.mult": 2.60e-07, "chol.sub": 2.52e-07, "udl.u_t": 3.25e-07, "udl.chol_d": 1.08e-07, "eta.u_t": 3.25e-07, "eta.chol_d": 1.08e-07, "eta.m_post": 8.95e-07, "eta.chol_dinv": 2.65e-07, "mult": 2.01e-07, "mult_t": 2.51e-07, "solve": 2.29e-07, "solve_t": 2.42e-07, "logdet": 1.03e-07, "inv.diag": 3.65e-07, "inv.sub": 4.52e-07},
    ('wave', 21, 67, 2): {"chol.diag": 7.38e-08, "sym.mult": 3.66e-07, "chol.sub": 3.24e-07, "udl.u_t": 4.20e-07, "udl.chol_d": 1.02e-07, "eta.u_t": 4.20e-07, "eta.chol_d": 1.02e-07, "eta.m_post": 8.20e-07, "eta.chol_dinv": 3.66e-07, "mult": 2.66e-07, "mult_t": 3.22e-07, "solve": 2.64e-07, "solve_t": 3.06e-07, "logdet": 8.16e-08, "inv.diag": 2.95e-07, "inv.sub": 4.95e-07},
    ('wave', 32, 130, 1): {"chol.diag": 7.02e-08, "sym.mult": 5.17e-07, "chol.sub": 4.27e-07, "udl.u_t": 4.27e-07, "udl.chol_d": 1.35e-07, "eta.u_t": 4.27e-07, "eta.chol_d": 1.35e-07, "eta.m_post": 6.59e-07, "eta.chol_dinv": 2.65e-07, "mult": 3.52e-07, "mult_t": 4.39e-07, "solve": 3.37e-07, "solve_t": 3.39e-07, "logdet": 1.11e-07, "inv.diag": 3.79e-07, "inv.sub": 4.08e-07},
    ('panel', 33, 5, 2): {"chol.diag": 6.60e-08, "sym.mult": 3.52e-07, "chol.sub": 4.03e-07, "udl.u_t": 5.41e-07, "udl.chol_d": 9.28e-08, "eta.u_t": 5.41e-07, "eta.chol_d": 9.28e-08, "eta.m_post": 4.96e-07, "eta.chol_dinv": 3.43e-07, "mult": 2.51e-07, "mult_t": 3.74e-07, "solve": 2.86e-07, "solve_t": 2.68e-07, "logdet": 1.09e-07, "inv.diag": 3.28e-07, "inv.sub": 3.14e-07},
    ('panel', 48, 20, 1): {"chol.diag": 5.96e-08, "sym.mult": 7.10e-07, "chol.sub": 4.99e-07, "udl.u_t": 5.41e-07, "udl.chol_d": 9.27e-08, "eta.u_t": 5.41e-07, "eta.chol_d": 9.27e-08, "eta.m_post": 8.85e-07, "eta.chol_dinv": 2.60e-07, "mult": 4.90e-07, "mult_t": 5.82e-07, "solve": 3.14e-07, "solve_t": 3.16e-07, "logdet": 9.88e-08, "inv.diag": 3.59e-07, "inv.sub": 5.05e-07},
    ('panel', 64, 12, 1): {"chol.diag": 6.40e-08, "sym.mult": 7.44e-07, "chol.sub": 5.38e-07, "udl.u_t": 5.54e-07, "udl.chol_d": 9.94e-08, "eta.u_t": 5.54e-07, "eta.chol_d": 9.94e-08, "eta.m_post": 7.15e-07, "eta.chol_dinv": 3.55e-07, "mult": 7.47e-07, "mult_t": 5.11e-07, "solve": 4.00e-07, "solve_t": 3.67e-07, "logdet": 6.21e-08, "inv.diag": 3.94e-07, "inv.sub": 5.90e-07},
}

# (route, d, T, B) -> the same matrix without a sub-diagonal
NO_SUB = {
    ('sweep', 3, 4, 3): {"chol.diag": 5.96e-08, "sym.mult": 7.04e-08},
    ('lane_par', 3, 70, 2): {"chol.diag": 5.96e-08, "sym.mult": 9.29e-08},
    ('row_par', 7, 70, 2): {"chol.diag": 5.96e-08, "sym.mult": 8.07e-08},
    ('row', 12, 80, 2): {"chol.diag": 5.96e-08, "sym.mult": 1.53e-07},
    ('tile', 12, 1, 2): {"chol.diag": 5.96e-08, "sym.mult": 1.80e-07},
    ('wave', 21, 67, 2): {"chol.diag": 5.96e-08, "sym.mult": 2.61e-07},
    ('panel', 33, 5, 2): {"chol.diag": 5.96e-08, "sym.mult": 2.32e-07},
}

# (route, d, T, B) -> mf_btd_logdet_quad_f32
LOGDET_QUAD = {
    ('sweep', 1, 1, 3): 1.46e-07,
    ('sweep', 3, 4, 3): 1.75e-07,
    ('sweep', 6, 63, 2): 1.58e-07,
    ('sweep', 9, 17, 2): 1.90e-07,
    ('sweep', 2, 64, 4096): 2.39e-07,
    ('lane_par', 1, 64, 1): 1.02e-07,
    ('lane_par', 3, 70, 2): 1.55e-07,
    ('lane_par', 4, 209, 1): 1.33e-07,
    ('lane_par', 2, 777, 3): 1.55e-07,
    ('row_par', 5, 65, 1): 1.08e-07,
    ('row_par', 6, 64, 1): 1.50e-07,
    ('row_par', 7, 70, 2): 1.80e-07,
    ('row_par', 9, 209, 1): 9.52e-08,
}
