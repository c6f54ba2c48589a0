"""Float32 yardsticks of the KL / marginals tests: the error of the closed forms of tests/helpers/kl_closed_forms.py evaluated in
float32 on the CPU against their float64 evaluation, the larger of 8 draws, never below 2^-24 (rule and metric:
tests/helpers/kl_fp32_cases.py).  Generated: python scripts/kl_fp32_yardsticks.py > tests/helpers/kl_fp32_table.py"""

# (route, d, T, B) -> the value for q1 != q2 (kl) and q2 = q1 (kl_same); with an adjoint kernel: the ten gradients of sum_s w_s KL_s
KL = {
    ('sweep', 1, 2, 2): {"kl": 1.86e-07, "kl_same": 5.96e-08, "q1.mu0": 1.57e-07, "q1.chol_p0": 1.88e-07, "q1.a_s": 9.66e-08, "q1.b_s": 1.25e-07, "q1.chol_q": 1.35e-06, "q2.mu0": 9.11e-08, "q2.chol_p0": 2.58e-07, "q2.a_s": 9.66e-08, "q2.b_s": 1.25e-07, "q2.chol_q": 4.52e-07},
    ('sweep', 3, 40, 2): {"kl": 1.88e-07, "kl_same": 5.96e-08, "q1.mu0": 1.53e-07, "q1.chol_p0": 1.62e-07, "q1.a_s": 1.59e-07, "q1.b_s": 1.49e-07, "q1.chol_q": 1.62e-07, "q2.mu0": 9.59e-08, "q2.chol_p0": 1.72e-07, "q2.a_s": 2.62e-07, "q2.b_s": 1.54e-07, "q2.chol_q": 2.18e-07},
    ('sweep', 9, 33, 1): {"kl": 1.42e-07, "kl_same": 5.96e-08, "q1.mu0": 1.36e-07, "q1.chol_p0": 1.88e-07, "q1.a_s": 2.39e-07, "q1.b_s": 1.68e-07, "q1.chol_q": 1.86e-07, "q2.mu0": 1.41e-07, "q2.chol_p0": 2.45e-07, "q2.a_s": 1.85e-07, "q2.b_s": 1.56e-07, "q2.chol_q": 1.98e-07},
    ('scan', 6, 70, 2): {"kl": 2.32e-07, "kl_same": 5.96e-08, "q1.mu0": 1.76e-07, "q1.chol_p0": 2.22e-07, "q1.a_s": 2.76e-07, "q1.b_s": 1.82e-07, "q1.chol_q": 1.63e-07, "q2.mu0": 1.31e-07, "q2.chol_p0": 2.72e-07, "q2.a_s": 2.02e-07, "q2.b_s": 1.42e-07, "q2.chol_q": 1.68e-07},
    ('scan', 5, 203, 3): {"kl": 2.59e-07, "kl_same": 5.96e-08, "q1.mu0": 1.42e-07, "q1.chol_p0": 2.19e-07, "q1.a_s": 1.84e-07, "q1.b_s": 1.58e-07, "q1.chol_q": 2.50e-07, "q2.mu0": 1.36e-07, "q2.chol_p0": 1.74e-07, "q2.a_s": 2.04e-07, "q2.b_s": 1.35e-07, "q2.chol_q": 2.61e-07},
    ('scan', 8, 90, 1): {"kl": 1.89e-07, "kl_same": 5.96e-08, "q1.mu0": 1.26e-07, "q1.chol_p0": 1.32e-07, "q1.a_s": 1.65e-07, "q1.b_s": 1.79e-07, "q1.chol_q": 2.12e-07, "q2.mu0": 1.88e-07, "q2.chol_p0": 2.63e-07, "q2.a_s": 2.06e-07, "q2.b_s": 1.97e-07, "q2.chol_q": 2.22e-07},
    ('scan', 9, 70, 1): {"kl": 1.40e-07, "kl_same": 5.96e-08, "q1.mu0": 1.52e-07, "q1.chol_p0": 2.29e-07, "q1.a_s": 1.47e-07, "q1.b_s": 1.53e-07, "q1.chol_q": 2.44e-07, "q2.mu0": 1.59e-07, "q2.chol_p0": 1.75e-07, "q2.a_s": 1.54e-07, "q2.b_s": 1.60e-07, "q2.chol_q": 1.79e-07},
    ('row', 12, 80, 2): {"kl": 1.07e-07, "kl_same": 5.96e-08, "q1.mu0": 1.32e-07, "q1.chol_p0": 2.40e-07, "q1.a_s": 1.67e-07, "q1.b_s": 2.14e-07, "q1.chol_q": 2.33e-07, "q2.mu0": 1.58e-07, "q2.chol_p0": 1.56e-07, "q2.a_s": 2.52e-07, "q2.b_s": 2.11e-07, "q2.chol_q": 1.81e-07},
    ('row', 15, 70, 1): {"kl": 7.52e-08, "kl_same": 5.96e-08, "q1.mu0": 1.51e-07, "q1.chol_p0": 3.67e-07, "q1.a_s": 2.28e-07, "q1.b_s": 2.14e-07, "q1.chol_q": 2.22e-07, "q2.mu0": 1.98e-07, "q2.chol_p0": 2.31e-07, "q2.a_s": 2.76e-07, "q2.b_s": 1.74e-07, "q2.chol_q": 1.92e-07},
    ('row', 12, 9, 2): {"kl": 1.42e-07, "kl_same": 5.96e-08, "q1.mu0": 1.23e-07, "q1.chol_p0": 2.71e-07, "q1.a_s": 1.74e-07, "q1.b_s": 2.80e-07, "q1.chol_q": 2.67e-07, "q2.mu0": 1.68e-07, "q2.chol_p0": 2.71e-07, "q2.a_s": 2.05e-07, "q2.b_s": 1.43e-07, "q2.chol_q": 1.60e-07},
    ('walk', 16, 9, 3): {"kl": 1.71e-07, "kl_same": 1.26e-07},
    ('walk', 17, 67, 2): {"kl": 1.15e-07, "kl_same": 6.03e-08},
    ('walk', 23, 130, 3): {"kl": 1.15e-07, "kl_same": 8.55e-08},
    ('walk', 32, 331, 1): {"kl": 1.49e-07, "kl_same": 5.96e-08},
    ('operators', 40, 20, 2): {"kl": 1.54e-07, "kl_same": 1.53e-07},
}

# (d, T, B) -> marginal means, covariances and the five gradients of a random linear functional of them
MARGINALS = {
    (1, 2, 2): {"means": 5.96e-08, "covs": 5.96e-08, "g.mu0": 9.22e-08, "g.chol_p0": 5.96e-08, "g.a_s": 1.15e-07, "g.b_s": 5.96e-08, "g.chol_q": 5.96e-08},
    (3, 40, 2): {"means": 7.14e-08, "covs": 9.94e-08, "g.mu0": 6.70e-08, "g.chol_p0": 8.78e-08, "g.a_s": 1.22e-07, "g.b_s": 7.78e-08, "g.chol_q": 1.10e-07},
    (9, 33, 1): {"means": 5.96e-08, "covs": 8.89e-08, "g.mu0": 8.11e-08, "g.chol_p0": 1.30e-07, "g.a_s": 1.39e-07, "g.b_s": 7.98e-08, "g.chol_q": 1.23e-07},
    (6, 70, 2): {"means": 1.51e-07, "covs": 1.18e-07, "g.mu0": 1.59e-07, "g.chol_p0": 1.25e-07, "g.a_s": 1.94e-07, "g.b_s": 1.46e-07, "g.chol_q": 1.67e-07},
    (5, 203, 3): {"means": 1.25e-07, "covs": 1.70e-07, "g.mu0": 9.86e-08, "g.chol_p0": 1.40e-07, "g.a_s": 2.28e-07, "g.b_s": 1.26e-07, "g.chol_q": 1.32e-07},
    (8, 90, 1): {"means": 7.61e-08, "covs": 1.43e-07, "g.mu0": 1.15e-07, "g.chol_p0": 1.24e-07, "g.a_s": 1.47e-07, "g.b_s": 1.30e-07, "g.chol_q": 1.45e-07},
    (9, 70, 1): {"means": 9.59e-08, "covs": 1.63e-07, "g.mu0": 1.82e-07, "g.chol_p0": 1.78e-07, "g.a_s": 1.61e-07, "g.b_s": 1.18e-07, "g.chol_q": 1.58e-07},
    (12, 100, 2): {"means": 1.09e-07, "covs": 1.62e-07, "g.mu0": 1.50e-07, "g.chol_p0": 1.61e-07, "g.a_s": 1.73e-07, "g.b_s": 1.28e-07, "g.chol_q": 1.77e-07},
    (15, 70, 1): {"means": 8.78e-08, "covs": 1.86e-07, "g.mu0": 1.21e-07, "g.chol_p0": 1.99e-07, "g.a_s": 1.77e-07, "g.b_s": 1.21e-07, "g.chol_q": 1.68e-07},
}

# (d, T, B) -> the five gradients with one of the incoming gradients absent (mf_ssm_marginals_grad: g_means / g_covs = NULL)
MARGINALS_NULL = {
    (3, 40, 2): {"g_means": {"g.mu0": 5.96e-08, "g.chol_p0": 8.78e-08, "g.a_s": 1.46e-07, "g.b_s": 5.96e-08, "g.chol_q": 1.10e-07}, "g_covs": {"g.mu0": 6.70e-08, "g.chol_p0": 5.96e-08, "g.a_s": 1.21e-07, "g.b_s": 7.78e-08, "g.chol_q": 5.96e-08}},
    (9, 33, 1): {"g_means": {"g.mu0": 5.96e-08, "g.chol_p0": 1.30e-07, "g.a_s": 1.36e-07, "g.b_s": 5.96e-08, "g.chol_q": 1.23e-07}, "g_covs": {"g.mu0": 8.11e-08, "g.chol_p0": 5.96e-08, "g.a_s": 9.55e-08, "g.b_s": 7.98e-08, "g.chol_q": 5.96e-08}},
    (6, 70, 2): {"g_means": {"g.mu0": 5.96e-08, "g.chol_p0": 1.25e-07, "g.a_s": 1.54e-07, "g.b_s": 5.96e-08, "g.chol_q": 1.67e-07}, "g_covs": {"g.mu0": 1.59e-07, "g.chol_p0": 5.96e-08, "g.a_s": 1.62e-07, "g.b_s": 1.46e-07, "g.chol_q": 5.96e-08}},
    (12, 100, 2): {"g_means": {"g.mu0": 5.96e-08, "g.chol_p0": 1.61e-07, "g.a_s": 1.69e-07, "g.b_s": 5.96e-08, "g.chol_q": 1.77e-07}, "g_covs": {"g.mu0": 1.50e-07, "g.chol_p0": 5.96e-08, "g.a_s": 1.65e-07, "g.b_s": 1.28e-07, "g.chol_q": 5.96e-08}},
}

# (d, B, T) -> mf_ssm_kl_from_moments_f32: the operator form on float32-rounded moments
FROM_MOMENTS = {
    (16, 1, 1): 2.50e-07, (16, 3, 2): 1.63e-07, (16, 2, 9): 1.29e-07, (16, 70, 5): 1.89e-07, (16, 2, 130): 1.08e-07,
    (17, 1, 1): 1.54e-07, (17, 3, 2): 1.32e-07, (17, 2, 9): 1.13e-07, (17, 70, 5): 1.91e-07, (17, 2, 130): 1.41e-07,
    (24, 1, 1): 2.39e-07, (24, 3, 2): 1.31e-07, (24, 2, 9): 9.50e-08, (24, 70, 5): 1.61e-07, (24, 2, 130): 1.28e-07,
    (31, 1, 1): 3.85e-07, (31, 3, 2): 1.97e-07, (31, 2, 9): 1.35e-07, (31, 70, 5): 1.78e-07, (31, 2, 130): 1.11e-07,
    (32, 1, 1): 1.54e-07, (32, 3, 2): 1.99e-07, (32, 2, 9): 1.15e-07, (32, 70, 5): 1.87e-07, (32, 2, 130): 8.43e-08,
}

# (d, B, T) -> the float32 KL of tests/test_gpu_wave.py::test_wave_marginals_and_covariance_blocks (route: walk)
WAVE_TEST = {
    (16, 1, 2): 1.37e-07, (16, 70, 9): 1.72e-07, (16, 3, 130): 1.16e-07, (16, 70, 67): 1.42e-07, (16, 1, 700): 9.50e-08, (16, 5, 331): 1.24e-07,
    (27, 1, 2): 1.38e-07, (27, 70, 9): 2.13e-07, (27, 3, 130): 1.07e-07, (27, 70, 67): 1.68e-07, (27, 1, 700): 7.17e-08, (27, 5, 331): 1.34e-07,
    (32, 1, 2): 7.07e-08, (32, 70, 9): 2.23e-07, (32, 3, 130): 1.52e-07, (32, 70, 67): 1.66e-07, (32, 1, 700): 6.37e-08, (32, 5, 331): 1.57e-07,
}
