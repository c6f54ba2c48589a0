"""
The models, one module per family, and the functional layer their fused launches go through.  Every model has a zero mean
function; every name below is importable from ``markovflow_amd.models``.

``GaussianProcessRegression`` (``gpr.py``): GP regression as a Kalman filter on the kernel's state space model; for Matérn
components the kernel -> state space model step is fused into the sweep, ``mf_gpr_matern_loglik_*`` and its ``_grad`` /
``posterior_chain`` siblings.

``CVIGaussianProcess`` (``sites.py``): one univariate Gaussian site per data point, updated by conjugate-computation VI;
``mf_lik_cvi_site_update_*``.

``PowerExpectationPropagation`` (``sites.py``): the same sites updated by power EP, with the EP energy; ``mf_lik_pep_site_update_*``.

``SparseCVIGaussianProcess`` (``sparse.py``): ``M + 1`` sites on the pairs of neighbouring inducing states, CVI;
``mf_lik_sparse_cvi_site_update_*``.

``SparsePowerExpectationPropagation`` (``sparse.py``): the same sites with a normaliser each, power EP;
``mf_lik_sparse_pep_site_update_*``.

``SparseVariationalGaussianProcess`` (``sparse.py``): SVGP, ``q`` a trainable chain on the inducing points;
``mf_lik_sparse_expectations_*``; on the stacked chains of an ``IndependentMultiOutputStack`` with a multi-latent likelihood,
``mf_lik_stack_expectations_*``.

``ImportanceWeightedVI`` (``sparse.py``): SVGP with the importance-weighted bound, proposals by Matheron's rule;
``mf_lik_iw_log_weights_*``.

``VariationalGaussianProcess`` (``variational.py``): ``q`` a trainable chain on the states at the data points;
``mf_lik_dense_expectations_*`` and ``mf_lik_dense_expectations_adjoint_*``.

``SpatioTemporalSparseVariational`` (``spatio_temporal.py``): SVGP for a product kernel ``k_s(x, x') k_t(t, t')``;
``mf_lik_st_expectations_*``.

``SpatioTemporalSparseCVI`` (``spatio_temporal.py``): its site-based variant; ``mf_lik_st_cvi_site_update_*``.

``segmented_ops.py`` holds the fused ops on pairs of inducing states as functions (``*_hip`` wrapper, ``*_torch`` reference route,
autograd ``Function``), ``_common.py`` the shared checks and the one launch path of the fused entry points.
"""
from .. import _lib  # noqa: F401  (with ``KalmanFilter`` and the private names below: what scripts/ and tests/ reach through here)
from ..kalman_filter import KalmanFilter  # noqa: F401
from ._common import back_project_nats, gradient_correction, gradient_transformation_mean_var_to_expectation
from .gpr import GaussianProcessRegression
from .segmented_ops import (IW_SAMPLE_CHUNK, SPARSE_EXPECT_TILE, SPARSE_FACTOR_LATENTS, SPARSE_FACTOR_MAX_OUTPUTS, SPARSE_SITE_MAX_TWO_D,
                            _iw_log_weights_launch, _segments_of, _sparse_expectations_launch, _sparse_factor_expectations_launch,
                            _sparse_multi_expectations_launch, iw_log_likelihood, iw_log_likelihood_torch, iw_merged_time_points,
                            pair_cavity, sparse_cvi_site_update_hip, sparse_cvi_site_update_torch, sparse_expectation_tiles,
                            sparse_expected_log_likelihood, sparse_expected_log_likelihood_torch,
                            sparse_factor_expected_log_likelihood, sparse_factor_expected_log_likelihood_torch,
                            sparse_factor_site_projections, sparse_multi_expected_log_likelihood,
                            sparse_multi_expected_log_likelihood_torch, sparse_multi_output_expected_log_likelihood_torch,
                            sparse_multi_site_projections, sparse_pep_site_update_hip, sparse_pep_site_update_torch,
                            sparse_site_projections, sparse_stack_expected_log_likelihood,
                            sparse_stack_expected_log_likelihood_torch)
from .sites import CVIGaussianProcess, PowerExpectationPropagation
from .sparse import (ImportanceWeightedVI, SparseCVIGaussianProcess, SparsePowerExpectationPropagation,
                     SparseVariationalGaussianProcess, _SparseSitesGaussianProcess)
from .spatio_temporal import (ST_EXPECT_TILE, SpatioTemporalSparseCVI, SpatioTemporalSparseVariational, _st_expectations_launch,
                              st_cvi_site_update_hip, st_cvi_site_update_torch, st_expected_log_likelihood,
                              st_expected_log_likelihood_torch, st_point_marginals)
from .variational import (DENSE_EXPECT_MAX_D, DENSE_EXPECT_TILE, VariationalGaussianProcess, dense_expected_log_likelihood,
                          dense_expected_log_likelihood_torch)
