"""
markovflow_amd - MI355X-native Kalman filter / block-tridiagonal precision operator.

Drop-in for the hot path of secondmind-labs/markovflow (``kalman_filter.py``, ``block_tri_diag.py``,
``state_space_model.py``, ``gauss_markov.py``, ``emission_model.py``): same class and method names,
torch HIP tensors in place of TensorFlow tensors, hand-written gfx950 kernels underneath.
"""
from .block_tri_diag import BlockTriDiagonal, LowerTriangularBlockTriDiagonal, SymmetricBlockTriDiagonal
from .emission_model import ComposedPairEmissionModel, EmissionModel, StackEmissionModel
from .gauss_markov import GaussMarkovDistribution, check_compatible
from .kalman_filter import (
    BaseKalmanFilter,
    GaussianSites,
    KalmanFilter,
    KalmanFilterWithSites,
    KalmanFilterWithSparseSites,
    UnivariateGaussianSitesNat,
)
from .state_space_model import StateSpaceModel, state_space_model_from_covariances
from . import conditionals, distributed, kernels, likelihoods, mean_function, models, sde, spatial_kernels, ssm_gaussian_transformations, ssm_natgrad
from .kernels import (Constant, FactorAnalysisKernel, HarmonicOscillator, IndependentMultiOutput, IndependentMultiOutputStack, LatentExponentiallyGenerated, Matern12, Matern32, Matern52, NonStationaryKernel,
                      PiecewiseKernel, Product, SDEKernel, SparseSpatioTemporalKernel, StackKernel, StationaryKernel, Sum)
from .likelihoods import Bernoulli, Gaussian, HeteroscedasticGaussian, Likelihood, MultiStageLikelihood, Poisson, StudentT
from .mean_function import ImpulseMeanFunction, LinearMeanFunction, MeanFunction, StepMeanFunction, ZeroMeanFunction
from .models import (CVIGaussianProcess, GaussianProcessRegression, ImportanceWeightedVI, PowerExpectationPropagation,
                     SparseCVIGaussianProcess, SparsePowerExpectationPropagation, SparseVariationalGaussianProcess,
                     SpatioTemporalSparseCVI, SpatioTemporalSparseVariational, VariationalGaussianProcess)
from .sde import (SDE, DoubleWellSDE, LinearDrift, OrnsteinUhlenbeckSDE, euler_maruyama, linearize_sde,
                  squared_drift_difference_along_Gaussian_path)
from .ssm_natgrad import SSMNaturalGradient
from .posterior import AnalyticPosteriorProcess, ConditionalProcess, ImportanceWeightedPosteriorProcess
from ._lib import MarkovflowAmdError, check_errors, errors_as_nan, set_synchronous_checks

__all__ = [
    "BlockTriDiagonal", "LowerTriangularBlockTriDiagonal", "SymmetricBlockTriDiagonal", "EmissionModel",
    "GaussMarkovDistribution", "check_compatible", "BaseKalmanFilter", "GaussianSites", "KalmanFilter",
    "KalmanFilterWithSites", "KalmanFilterWithSparseSites", "UnivariateGaussianSitesNat", "StateSpaceModel",
    "state_space_model_from_covariances", "conditionals", "distributed", "kernels", "models", "ssm_gaussian_transformations", "SDEKernel", "StationaryKernel", "Matern12", "Matern32",
    "Matern52", "Sum", "IndependentMultiOutput", "FactorAnalysisKernel", "ComposedPairEmissionModel", "Constant", "HarmonicOscillator", "Product", "GaussianProcessRegression", "AnalyticPosteriorProcess", "ConditionalProcess",
    "MarkovflowAmdError", "check_errors", "errors_as_nan", "set_synchronous_checks",
    "likelihoods", "Likelihood", "Gaussian", "Bernoulli", "Poisson", "StudentT", "MultiStageLikelihood", "HeteroscedasticGaussian", "StackKernel", "IndependentMultiOutputStack", "StackEmissionModel", "CVIGaussianProcess", "PowerExpectationPropagation",
    "SparseCVIGaussianProcess", "SparseVariationalGaussianProcess", "SSMNaturalGradient", "ssm_natgrad",
    "SparsePowerExpectationPropagation", "ImportanceWeightedVI", "ImportanceWeightedPosteriorProcess",
    "VariationalGaussianProcess", "spatial_kernels", "SparseSpatioTemporalKernel", "SpatioTemporalSparseVariational", "SpatioTemporalSparseCVI",
    "NonStationaryKernel", "PiecewiseKernel", "LatentExponentiallyGenerated",
    "mean_function", "MeanFunction", "ZeroMeanFunction", "LinearMeanFunction", "ImpulseMeanFunction", "StepMeanFunction",
    "sde", "SDE", "OrnsteinUhlenbeckSDE", "DoubleWellSDE", "LinearDrift", "euler_maruyama", "linearize_sde",
    "squared_drift_difference_along_Gaussian_path",
]
