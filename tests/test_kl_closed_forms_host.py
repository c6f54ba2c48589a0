"""
CPU checks of the references the float32 KL / marginals tests rest on (tests/helpers/kl_closed_forms.py), in float64: both
formulations of KL(q1 || q2) against the numpy restatement of the reference (oracle.numpy_oracle.ssm_kl_divergence,
markovflow/state_space_model.py:528-593), the two variants of the moment recursion against each other, on the shapes the GPU tests
use; and that the committed yardstick table has an entry for every case.
"""
import numpy as np
import pytest
import torch

from oracle import numpy_oracle as O
from helpers import kl_closed_forms as KC
from helpers import kl_fp32_cases as C
from helpers import kl_fp32_table as TABLE

KL_SHAPES = sorted({shape for shapes in C.KL_CASES.values() for shape in shapes})


@pytest.mark.parametrize("d,t,bsz", KL_SHAPES)
def test_both_forms_match_the_oracle(d, t, bsz):
    kw1, kw2, _ = C.draw_kl(C.DEFAULT_SEED, d, t, bsz)
    want = O.ssm_kl_divergence(tuple(kw1[k] for k in KC.CHAIN), tuple(kw2[k] for k in KC.CHAIN))
    q1, q2 = KC.chain(kw1), KC.chain(kw2)
    for scan in (False, True):
        np.testing.assert_allclose(KC.kl_local(q1, q2, scan=scan).numpy(), want, rtol=1e-10)
        np.testing.assert_allclose(KC.kl_operator_from_chains(q1, q2, scan=scan).numpy(), want, rtol=1e-10)
    assert float(KC.kl_local(q1, q1).abs().max()) < 1e-12 * t * d
    assert float(KC.kl_operator_from_chains(q1, q1).abs().max()) < 1e-12 * t * d


@pytest.mark.parametrize("d", C.FROM_MOMENTS_DIMS)
@pytest.mark.parametrize("bsz,t", C.FROM_MOMENTS_SHAPES)
def test_operator_form_from_given_moments_matches_the_oracle(d, bsz, t):
    """The inputs of mf_ssm_kl_from_moments (T = 1: no transitions at all), unrounded."""
    kw1, kw2, covs_1, cross_1, mean_diff = C.draw_from_moments(C.DEFAULT_SEED, d, bsz, t, False)
    want = O.ssm_kl_divergence(tuple(kw1[k] for k in KC.CHAIN), tuple(kw2[k] for k in KC.CHAIN))
    got = C.from_moments_closed_form(kw1, kw2, covs_1, cross_1, mean_diff, torch.float64)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-10)


@pytest.mark.parametrize("d,t,bsz", sorted(set(C.MARGINALS_CASES) | set(KL_SHAPES)))
def test_moment_recursion_variants_agree(d, t, bsz):
    kw = C.draw_marginals(C.DEFAULT_SEED, d, t, bsz)[0]
    q = KC.chain(kw)
    means, covs = KC.moments_sequential(q)
    means_s, covs_s = KC.moments_scan(q)
    want_m, want_c, want_x = C.numpy_moments(kw)
    np.testing.assert_allclose(means.numpy(), want_m, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(covs.numpy(), want_c, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(means_s.numpy(), want_m, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(covs_s.numpy(), want_c, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(KC.cross_covariances(q, covs).numpy(), want_x, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(want_m, O.ssm_marginal_means(kw["mu0"], kw["a_s"], kw["b_s"]), rtol=1e-12, atol=1e-13)


def test_gradients_of_both_recursion_variants_agree():
    """What autograd makes of the two variants is the same adjoint (the yardstick differentiates whichever the kernel evaluates)."""
    d, t, bsz = 5, 70, 2
    kw1, kw2, weights = C.draw_kl(C.DEFAULT_SEED, d, t, bsz)
    seq = C.kl_closed_form(lambda a, b: KC.kl_local(a, b, scan=False), kw1, kw2, weights, torch.float64, True)[1]
    scan = C.kl_closed_form(lambda a, b: KC.kl_local(a, b, scan=True), kw1, kw2, weights, torch.float64, True)[1]
    for name, g, w in zip(C.GRAD_NAMES, scan, seq):
        assert KC.tensor_error(g, w) < 1e-11, name
    kw, w_m, w_c = C.draw_marginals(C.DEFAULT_SEED, d, t, bsz)
    for name, g, w in zip(C.MARGINALS_NAMES, C.marginals_closed_form(kw, w_m, w_c, torch.float64, True),
                          C.marginals_closed_form(kw, w_m, w_c, torch.float64, False)):
        assert KC.tensor_error(g, w) < 1e-11, name


def test_the_committed_table_covers_every_case_and_is_what_the_script_measures():
    for route, shapes in C.KL_CASES.items():
        for shape in shapes:
            names = {"kl", "kl_same"} | (set(C.GRAD_NAMES) if route in C.ADJOINT_ROUTES else set())
            assert set(TABLE.KL[(route,) + shape]) == names
    assert set(TABLE.MARGINALS) == set(C.MARGINALS_CASES) and all(set(v) == set(C.MARGINALS_NAMES) for v in TABLE.MARGINALS.values())
    assert set(TABLE.FROM_MOMENTS) == {(d, b, t) for d in C.FROM_MOMENTS_DIMS for b, t in C.FROM_MOMENTS_SHAPES}
    assert set(TABLE.WAVE_TEST) == set(C.WAVE_TEST_CASES)
    every = [v for row in list(TABLE.KL.values()) + list(TABLE.MARGINALS.values()) for v in row.values()]
    every += list(TABLE.FROM_MOMENTS.values()) + list(TABLE.WAVE_TEST.values())
    # float32 has 24 bits: no yardstick below one rounding, none that would let half the digits go
    assert min(every) >= 0.99 * C.FP32_FLOOR and max(every) < 1e-5
    # one cheap entry re-measured (BLAS builds may differ in the last place of a sum: a factor of three, not equality)
    again = C.kl_yardstick("sweep", 3, 40, 2)
    for name, v in TABLE.KL[("sweep", 3, 40, 2)].items():
        assert v / 3.0 <= again[name] <= 3.0 * v, name
