"""
GPU parity tests of the wave kernels (csrc/mf_wave.hpp: one wavefront per (series, chunk), every matrix a register tile in the
accumulator layout of the 16x16x4 matrix-core instruction, 16 <= d <= 32, at most four outputs) - level 0 of
KalmanFilter.log_likelihood (/root/reference/markovflow/kalman_filter.py:184-255) between the row kernels (d <= 15) and the tile
engine.  Through the C ABI with explicit time partitions (first chunk without a spike, later chunks with one, ragged last chunks,
more than one reduction level) and through the classes; fp64 against the numpy oracle at the tolerance of the register kernels
(rtol 1e-9), fp32 on fp32-rounded inputs (rtol 3e-4, as tests/test_gpu_kalman_large_d.py).  The reference's largest tested state
dimension (d = 30, T = 1001: tests/unit/test_ssm_gaussian_transformations.py:40-46) is a case; the C oracle checks every series
at the shape VERDICT r04 names (B = 512, T = 1000).
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from oracle import c_oracle
from oracle import numpy_oracle as O
from test_gpu_kalman import DEV, build_kf, loglik_with_chunks, nn, random_ssm, tt

pytestmark = pytest.mark.gpu
F32 = torch.float32


def rounded(kw):
    return {k: v.astype(np.float32).astype(np.float64) for k, v in kw.items()}


def _r_inv(rng, m):
    a = rng.normal(size=(m, m))
    return a @ a.T + np.eye(m)


def _const(m, t, r_inv):
    return -0.5 * np.log(2 * np.pi) * m * t + 0.5 * t * np.linalg.slogdet(r_inv)[1]


@pytest.mark.parametrize("d,m,t,bsz,chunks", [
    (16, 1, 40, 3, 1), (16, 1, 41, 3, 2), (16, 1, 64, 2, 5), (16, 2, 33, 2, 3), (16, 4, 20, 2, 4), (16, 1, 2, 3, 1),
    (17, 1, 30, 2, 1), (17, 1, 31, 2, 3), (24, 1, 50, 2, 4), (24, 3, 27, 2, 2), (30, 1, 45, 2, 3), (32, 1, 40, 2, 1),
    (32, 1, 37, 2, 4), (32, 4, 25, 2, 3), (20, 1, 300, 1, 70), (16, 1, 200, 2, 0), (32, 2, 90, 3, 0),
])
def test_wave_log_likelihood_fp64_against_the_oracle(rng, d, m, t, bsz, chunks):
    kw = random_ssm(rng, (bsz,), t, d, m, well=True)
    r_inv = _r_inv(rng, m)
    ref = O.kf_log_likelihood(**kw, r_inv=r_inv, per_series=True)
    got = loglik_with_chunks(kw, r_inv, chunks) + _const(m, t, r_inv)
    np.testing.assert_allclose(got, ref, rtol=1e-9)


@pytest.mark.parametrize("d,m,t,bsz,chunks", [(16, 1, 40, 3, 2), (16, 3, 33, 2, 3), (24, 1, 50, 2, 4), (32, 2, 40, 2, 3),
                                              (30, 1, 120, 2, 0), (17, 4, 30, 2, 1)])
def test_wave_log_likelihood_fp32_against_the_oracle(rng, d, m, t, bsz, chunks):
    kw = rounded(random_ssm(rng, (bsz,), t, d, m, well=True))
    r_inv = _r_inv(rng, m).astype(np.float32).astype(np.float64)
    ref = O.kf_log_likelihood(**kw, r_inv=r_inv, per_series=True)
    got = loglik_with_chunks(kw, r_inv, chunks, dtype=F32) + _const(m, t, r_inv)
    np.testing.assert_allclose(got, ref, rtol=3e-4)


@pytest.mark.parametrize("d", [16, 24, 32])
def test_wave_time_partition_invariance(rng, d):
    """log|M| and r^T M^-1 r do not depend on the elimination order: any partition gives the same scalar (to rounding)."""
    t = 281
    kw = random_ssm(rng, (2,), t, d, 1, well=True)
    r_inv = np.array([[2.0]])
    base = loglik_with_chunks(kw, r_inv, 1)
    for chunks in (2, 3, 7, 16, 70):
        np.testing.assert_allclose(loglik_with_chunks(kw, r_inv, chunks), base, rtol=1e-10)


def test_wave_per_step_precisions_through_the_sites_filter(rng):
    """KalmanFilterWithSites (kalman_filter.py:437-497): per-step observation precisions, d = 24."""
    d, t = 24, 60
    kw = random_ssm(rng, (), t, d, 1, well=True)
    prec = 0.5 + rng.random(size=(t, 1, 1))
    ssm = mfa.StateSpaceModel(*(tt(kw[k]) for k in ("mu0", "chol_p0", "a_s", "b_s", "chol_q")))
    sites = mfa.UnivariateGaussianSitesNat(nat1=tt(kw["y"] * prec[..., 0]), nat2=tt(-0.5 * prec))
    kf = mfa.KalmanFilterWithSites(ssm, mfa.EmissionModel(tt(kw["h"])), sites)
    ref = O.kf_log_likelihood(**kw, r_inv=prec, log_det_obs_precision=np.sum(np.log(prec)))
    np.testing.assert_allclose(float(kf.log_likelihood().cpu()), ref, rtol=1e-9)


def test_wave_reference_largest_tested_shape_d30_T1001(rng):
    """d = 30, T = 1001: the largest chain the reference's own tests build
    (/root/reference/tests/unit/test_ssm_gaussian_transformations.py:40-46), through the classes, batch of 3."""
    d, t = 30, 1001
    kw = random_ssm(rng, (3,), t, d, 1, well=True)
    kf = build_kf(kw, np.array([[0.6]]))
    ref = O.kf_log_likelihood(**kw, r_inv=np.array([[1.0 / 0.36]]))
    np.testing.assert_allclose(float(kf.log_likelihood().cpu()), ref, rtol=1e-9)


def test_wave_not_positive_definite_is_reported(rng):
    kw = random_ssm(rng, (2,), 30, 16, 1, well=True)
    kw["chol_q"][1, 11] = 0.0
    kf = build_kf(kw, np.array([[0.7]]))
    _lib.check_errors()
    with pytest.raises(mfa.MarkovflowAmdError, match="log_likelihood"):
        float(kf.log_likelihood())
    _lib.check_errors()


@pytest.mark.parametrize("d", [16, 32])
def test_wave_every_series_against_the_c_oracle_at_the_verdict_shape(rng, d):
    """B = 512, T = 1000, fp64: every series against the C restatement (OpenMP over the batch)."""
    bsz, t, m = 512, 1000, 1
    kw = random_ssm(rng, (bsz,), t, d, m, well=True)
    r_inv = np.array([[1.7]])
    ref = c_oracle.kf_loglik(kw["mu0"], kw["chol_p0"], kw["a_s"], kw["b_s"], kw["chol_q"], kw["h"], kw["y"], r_inv, generic=True)
    got = loglik_with_chunks(kw, r_inv, 0) + _const(m, t, r_inv)            # (the C oracle returns the complete per-series value)
    np.testing.assert_allclose(got, ref, rtol=1e-9)


# ---- precision assembly on register tiles (wave_ssm_precision_kernel): StateSpaceModel.precision, BaseKalmanFilter._k_inv_post --------
@pytest.mark.parametrize("dtype,d,m,t,bsz", [(torch.float64, 16, 1, 9, 3), (torch.float64, 16, 3, 2, 2), (torch.float64, 17, 1, 12, 2),
                                             (torch.float64, 24, 2, 30, 2), (torch.float64, 32, 4, 17, 2), (torch.float64, 30, 1, 40, 1),
                                             (torch.float32, 16, 1, 20, 2), (torch.float32, 32, 2, 11, 2)])
def test_wave_precision_prior_and_posterior(rng, dtype, d, m, t, bsz):
    """`ssm.precision` (state_space_model.py:431-483) and `kf._k_inv_post` (kalman_filter.py:86-101) for 16 <= d <= 32 against the
    numpy oracle, block by block; the information vector through the posterior's initial mean / offsets is covered by
    tests/test_gpu_large_d_ops.py::test_large_d_posterior_marginals_and_kl."""
    kw = random_ssm(rng, (bsz,), t, d, m, well=True)
    if dtype == F32:
        kw = rounded(kw)
    tol = dict(rtol=1e-9, atol=1e-10) if dtype == torch.float64 else dict(rtol=2e-4, atol=2e-4)
    cov = 0.5 * np.eye(m) + 0.1 * np.ones((m, m))
    chol_r = np.linalg.cholesky(cov)
    if dtype == F32:
        chol_r = chol_r.astype(np.float32).astype(np.float64)
    kf = build_kf(kw, chol_r, dtype=dtype)
    prec = kf.prior_ssm.precision
    want_d, want_s = O.ssm_precision(kw["chol_p0"], kw["a_s"], kw["chol_q"])
    np.testing.assert_allclose(nn(prec.block_diagonal), want_d, **tol)
    np.testing.assert_allclose(nn(prec.block_sub_diagonal), want_s, **tol)
    post = kf._k_inv_post
    want_d, want_s = O.kf_posterior_precision(kw["chol_p0"], kw["a_s"], kw["chol_q"], kw["h"], np.linalg.inv(chol_r @ chol_r.T))
    np.testing.assert_allclose(nn(post.block_diagonal), want_d, **tol)
    np.testing.assert_allclose(nn(post.block_sub_diagonal), want_s, **tol)


# ---- LowerTriangularBlockTriDiagonal.solve on the wave solve kernel (csrc/mf_wave_ops.hpp) -----------------------------------------
@pytest.mark.parametrize("dtype,d", [(torch.float64, 16), (torch.float64, 17), (torch.float64, 24), (torch.float64, 31),
                                     (torch.float64, 32), (torch.float32, 16), (torch.float32, 21), (torch.float32, 32)])
@pytest.mark.parametrize("bl,lead,n,has_sub", [(1, (), 1, False), (3, (), 2, True), (5, (2,), 37, True), (2, (3,), 11, False),
                                               # long enough for the time partition (composed maps on the register tiles, then the
                                               # walk per chunk): even and ragged last chunks
                                               (9, (), 200, True), (4, (), 300, True), (3, (), 131, True)])
def test_wave_solve_both_orientations(rng, dtype, d, bl, lead, n, has_sub):
    """block_tri_diag.py:339-351: L z = r and L^T z = r, right-hand sides with leading dimensions broadcast over the factor
    (series r uses factor r % Bl), ragged wavefronts (Br not a multiple of the 4 or 2 series a wavefront walks), a block-diagonal
    factor (no coupling), one block."""
    from test_gpu_large_d_ops import TOL, scaled_spd_btd
    diag, sub = scaled_spd_btd(rng, (bl,), n, d, has_sub)
    ld, ls = O.btd_cholesky(diag, sub)
    if dtype == torch.float32:
        ld = ld.astype(np.float32).astype(np.float64)
        ls = None if ls is None else ls.astype(np.float32).astype(np.float64)
    rhs = rng.normal(size=lead + (bl, n, d))
    exact = mfa.LowerTriangularBlockTriDiagonal(tt(np.tril(ld), dtype), tt(ls, dtype))
    r = tt(rhs, dtype)
    tol = TOL[dtype]
    np.testing.assert_allclose(nn(exact.solve(r)), O.btd_solve(ld, ls, rhs), **tol)
    np.testing.assert_allclose(nn(exact.solve(r, transpose_left=True)), O.btd_solve(ld, ls, rhs, transpose_left=True), **tol)


def test_wave_solve_round_trip_at_the_operator_bench_shape(rng):
    """B = 512, T = 1000, d = 16 and 32: L (L^-1 r) = r and L^T (L^-T r) = r through dense_mult - a size-independent property at
    the shape scripts/bench_bigops.py times."""
    from test_gpu_large_d_ops import scaled_spd_btd
    for d, bsz in ((16, 512), (32, 130)):
        diag, sub = scaled_spd_btd(rng, (bsz,), 1000, d, True)
        ld, ls = tt(np.tril(diag), torch.float64), tt(sub, torch.float64)      # any lower factor with a safe diagonal will do
        low = mfa.LowerTriangularBlockTriDiagonal(ld, ls)
        r = torch.randn(bsz, 1000, d, dtype=torch.float64, device=DEV)
        z = low.solve(r)
        torch.testing.assert_close(low.dense_mult(z), r, rtol=1e-9, atol=1e-9)
        zt = low.solve(r, transpose_left=True)
        torch.testing.assert_close(low.dense_mult(zt, transpose_left=True), r, rtol=1e-9, atol=1e-9)


# ---- cholesky / upper_diagonal_lower / block_diagonal_of_inverse, one wavefront per series (csrc/mf_wave_ops.hpp) ------------------
@pytest.mark.parametrize("dtype,d", [(torch.float64, 16), (torch.float64, 17), (torch.float64, 24), (torch.float64, 31),
                                     (torch.float64, 32), (torch.float32, 16), (torch.float32, 21), (torch.float32, 32)])
@pytest.mark.parametrize("bsz,n,has_sub", [(1, 1, False), (3, 2, True), (2, 37, True), (70, 9, True), (2, 5, False),
                                           # long enough for the time partition of the Cholesky factorisation (chunks of >= 16 blocks)
                                           (3, 100, True), (70, 67, True), (1, 500, True)])
def test_wave_factorisations_against_the_oracle(rng, dtype, d, bsz, n, has_sub):
    """block_tri_diag.py:423-436 (cholesky), :438-545 (upper_diagonal_lower), :318-337 (block diagonal and sub-diagonal of the
    inverse): every block of every series against the oracle's serial recursions; one block, a block-diagonal matrix, more series
    than one wavefront round would need."""
    from test_gpu_large_d_ops import TOL, scaled_spd_btd
    diag, sub = scaled_spd_btd(rng, (bsz,), n, d, has_sub)
    if dtype == torch.float32:
        diag = diag.astype(np.float32).astype(np.float64)
        sub = None if sub is None else sub.astype(np.float32).astype(np.float64)
    tol = TOL[dtype]
    # the strict upper triangle of the diagonal blocks must not be read (block_tri_diag.py:423-436 factors the lower band)
    junk = np.triu(rng.normal(size=diag.shape), 1)
    sym = mfa.SymmetricBlockTriDiagonal(tt(np.tril(diag) + junk, dtype), tt(sub, dtype))
    chol = sym.cholesky
    ld, ls = O.btd_cholesky(diag, sub)
    np.testing.assert_allclose(nn(chol.block_diagonal), np.tril(ld), **tol)
    if has_sub:
        np.testing.assert_allclose(nn(chol.block_sub_diagonal), ls, **tol)
    exact = mfa.LowerTriangularBlockTriDiagonal(tt(np.tril(ld), dtype), tt(ls, dtype))
    inv_d, inv_s = O.btd_block_diagonal_of_inverse(ld, ls, return_sub=True) if has_sub else (O.btd_block_diagonal_of_inverse(ld, ls), None)
    if has_sub:
        got_d, got_s = exact._diag_and_sub_of_inverse(want_sub=True)
        np.testing.assert_allclose(nn(got_s), inv_s, **tol)
    else:
        got_d = exact.block_diagonal_of_inverse()
    np.testing.assert_allclose(nn(got_d), inv_d, **tol)
    if has_sub:
        sym2 = mfa.SymmetricBlockTriDiagonal(tt(diag, dtype), tt(sub, dtype))
        u_t, chol_d = sym2.upper_diagonal_lower()
        want_u, want_c = O.btd_upper_diagonal_lower(diag, sub)
        np.testing.assert_allclose(nn(u_t.block_sub_diagonal), want_u, **tol)
        np.testing.assert_allclose(nn(chol_d.block_diagonal), np.tril(want_c), **tol)


def test_wave_cholesky_reports_a_matrix_that_is_not_positive_definite(rng):
    from test_gpu_large_d_ops import scaled_spd_btd
    diag, sub = scaled_spd_btd(rng, (70,), 6, 20, True)
    diag[33, 4, 17, 17] = -1.0
    with pytest.raises(mfa.MarkovflowAmdError):
        c = mfa.SymmetricBlockTriDiagonal(tt(diag, torch.float64), tt(sub, torch.float64)).cholesky
        _ = c.block_diagonal
        mfa.check_errors()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("d,m,bsz,t", [(16, 1, 70, 12), (24, 2, 3, 40), (32, 1, 2, 25),
                                       # chains long enough for the time partition of the sweep (chunks of >= 16 blocks: up-sweep with
                                       # a spike, boundary pass, emit - csrc/mf_wave_ops.hpp), ragged last chunks
                                       (16, 1, 3, 100), (17, 3, 70, 67), (32, 2, 2, 131), (16, 4, 1, 700)])
def test_wave_posterior_chain_against_the_oracle(rng, dtype, d, m, bsz, t):
    """kalman_filter.py:159-174: the posterior state space model through precision -> upper_diagonal_lower with the information
    vector riding along (means, Cholesky factors of the conditional covariances)."""
    kw = random_ssm(rng, (bsz,), t, d, m, well=True)
    if dtype == torch.float32:
        kw = rounded(kw)
    chol_r = (0.6 * np.eye(m)).astype(np.float32).astype(np.float64)
    r_inv = np.linalg.inv(chol_r @ chol_r.T)
    kf = build_kf(kw, chol_r, dtype=dtype)
    post = kf.posterior_state_space_model()
    want = O.kf_posterior_ssm(**kw, r_inv=r_inv)
    got = (post.initial_mean, post.cholesky_initial_covariance, post.state_transitions, post.state_offsets,
           post.cholesky_process_covariances)
    tol = dict(rtol=1e-7, atol=1e-9) if dtype == torch.float64 else dict(rtol=5e-3, atol=5e-4)
    for g, w in zip(got, want):
        np.testing.assert_allclose(nn(g), w, **tol)


# ---- marginals / covariance blocks / KL on the register tiles (csrc/mf_wave_ops.hpp: wave_marginals_kernel) ------------------------
@pytest.mark.parametrize("dtype,d", [(torch.float64, 16), (torch.float64, 23), (torch.float64, 32), (torch.float32, 16),
                                     (torch.float32, 27), (torch.float32, 32)])
@pytest.mark.parametrize("bsz,t", [(1, 2), (70, 9), (3, 130), (70, 67), (1, 700), (5, 331)])
def test_wave_marginals_and_covariance_blocks(rng, dtype, d, bsz, t):
    """state_space_model.py:232-262,326-341 / gauss_markov.py:107-117: means, covariances and Cov(x_{k+1}, x_k) of every series
    against the explicit forward recursion; the KL divergence to a second chain (state_space_model.py:528-593) against the oracle."""
    from test_gpu_large_d_ops import TOL
    kw = random_ssm(rng, (bsz,), t, d, 1, well=True)
    kw2 = random_ssm(rng, (bsz,), t, d, 1, well=True)
    if dtype == torch.float32:
        kw, kw2 = rounded(kw), rounded(kw2)
    names = ("mu0", "chol_p0", "a_s", "b_s", "chol_q")
    ssm = mfa.StateSpaceModel(*(tt(kw[k], dtype) for k in names))
    means, covs = ssm.marginals
    covs2, sub = ssm.covariance_blocks()
    em = O.ssm_marginal_means(kw["mu0"], kw["a_s"], kw["b_s"])
    ec = [kw["chol_p0"] @ np.swapaxes(kw["chol_p0"], -1, -2)]
    for k in range(t - 1):
        a, c = kw["a_s"][:, k], kw["chol_q"][:, k]
        ec.append(a @ ec[-1] @ np.swapaxes(a, -1, -2) + c @ np.swapaxes(c, -1, -2))
    ec = np.stack(ec, axis=1)
    tol = TOL[dtype]
    np.testing.assert_allclose(nn(means), em, **tol)
    # the means alone: from 129 transitions on the chunk maps on the register tiles, then the walk per chunk (mf_wave_ops.hpp)
    np.testing.assert_allclose(nn(ssm.marginal_means), em, **tol)
    np.testing.assert_allclose(nn(covs), ec, **tol)
    np.testing.assert_allclose(nn(covs2), ec, **tol)
    np.testing.assert_allclose(nn(sub), O.ssm_subsequent_covariances(kw["a_s"], ec), **tol)
    other = mfa.StateSpaceModel(*(tt(kw2[k], dtype) for k in names))
    if dtype == torch.float64:
        want = O.ssm_kl_divergence(tuple(kw[k] for k in names), tuple(kw2[k] for k in names))
        np.testing.assert_allclose(nn(ssm.kl_divergence(other)), want, rtol=1e-8)
    else:
        # float32 (wave_kl_walk_kernel<float, ...>): against the operator form in float64 on the float32-representable chains,
        # within FP32_FACTOR x the same form evaluated in float32 (rule, metric and table: tests/helpers/kl_fp32_cases.py)
        from helpers import kl_closed_forms as KC
        from helpers import kl_fp32_cases as C
        from helpers import kl_fp32_table as TABLE
        want = KC.kl_operator_from_chains(KC.chain(kw), KC.chain(kw2))
        err, yard = KC.value_error(ssm.kl_divergence(other), want, t, d), TABLE.WAVE_TEST[(d, bsz, t)]
        print(f"  fp32 kl walk d={d} B={bsz} T={t}: error {err:.3g} (closed form in float32 {yard:.3g}, ratio {err / yard:.2f})")
        assert err <= C.FP32_FACTOR * yard
