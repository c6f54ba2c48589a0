"""
Emission model ``f_k = H_k x_k`` - mirror of ``markovflow/emission_model.py:25-153`` (reference).
The projections are tiny batched products; inside ``KalmanFilter.log_likelihood`` they are fused
into the HIP kernel and never materialised.
"""
from typing import Tuple

import torch


class EmissionModel:
    """Linear projection of states to outputs (emission_model.py:25-153)."""

    def __init__(self, emission_matrix: torch.Tensor) -> None:
        """:param emission_matrix: ``batch_dim + [num_data, output_dim, state_dim]``."""
        if emission_matrix.dim() < 3:
            raise ValueError(
                f"Emission Matrix must be at least 3D but has shape {tuple(emission_matrix.shape)}"
            )  # emission_model.py:46-49
        self._H = emission_matrix

    @property
    def batch_shape(self) -> torch.Size:
        return self._H.shape[:-3]

    @property
    def num_data(self) -> int:
        return self._H.shape[-3]

    @property
    def output_dim(self) -> int:
        return self._H.shape[-2]

    @property
    def state_dim(self) -> int:
        return self._H.shape[-1]

    @property
    def emission_matrix(self) -> torch.Tensor:
        return self._H

    def project_state_marginals_to_f(
        self, means: torch.Tensor, covariances: torch.Tensor, full_output_cov: bool = False
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.project_state_to_f(means), self.project_state_covariance_to_f(covariances, full_output_cov)

    def project_state_to_f(self, state: torch.Tensor) -> torch.Tensor:
        """``H x`` (emission_model.py:115-128)."""
        if state.shape[-1] != self.state_dim or state.shape[-2] != self.num_data:
            raise ValueError(f"state has shape {tuple(state.shape)}, expected [..., {self.num_data}, {self.state_dim}]")
        return torch.matmul(self._H, state[..., None])[..., 0]

    def project_state_covariance_to_f(self, covariance: torch.Tensor, full_output_cov: bool = False) -> torch.Tensor:
        """``H S Hᵀ`` or its diagonal (emission_model.py:130-153)."""
        if tuple(covariance.shape[-3:]) != (self.num_data, self.state_dim, self.state_dim):
            raise ValueError(f"covariance has shape {tuple(covariance.shape)}")
        hs = torch.matmul(self._H, covariance)
        if full_output_cov:
            return torch.matmul(hs, self._H.transpose(-1, -2))
        return torch.sum(self._H * hs, dim=-1)


class ComposedPairEmissionModel(EmissionModel):
    """Emission through an intermediate space (emission_model.py:157-266): ``g_k = H_inner x_k`` (``inner_dim`` latent functions) and
    ``f_k = H_outer,k g_k``, so the emission matrix is ``H_outer @ H_inner``.  The ``_f`` methods are ``EmissionModel``'s on the
    product; the ``_g`` methods project onto the intermediate space with the inner model.  Plain batched products: CPU or HIP
    tensors, differentiable by autograd."""

    def __init__(self, outer_emission_model: EmissionModel, inner_emission_model: EmissionModel) -> None:
        """:param outer_emission_model: ``batch + [num_data, output_dim, inner_dim]``;
        :param inner_emission_model: ``batch + [num_data, inner_dim, state_dim]``."""
        outer, inner = outer_emission_model.emission_matrix, inner_emission_model.emission_matrix
        if outer.shape[-1] != inner.shape[-2] or outer.shape[-3] != inner.shape[-3]:
            raise ValueError(f"the outer emission matrix {tuple(outer.shape)} does not compose with the inner one {tuple(inner.shape)}")
        super().__init__(torch.matmul(outer, inner))
        self._inner_emission_model = inner_emission_model

    @property
    def state_dim(self) -> int:
        return self._inner_emission_model.state_dim

    @property
    def inner_dim(self) -> int:
        """The dimension of the intermediate space ``g``."""
        return self._inner_emission_model.output_dim

    @property
    def inner_emission_matrix(self) -> torch.Tensor:
        """``batch + [num_data, inner_dim, state_dim]``."""
        return self._inner_emission_model.emission_matrix

    def project_state_marginals_to_g(
        self, means: torch.Tensor, covariances: torch.Tensor, full_output_cov: bool = True
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._inner_emission_model.project_state_marginals_to_f(means, covariances, full_output_cov)

    def project_state_to_g(self, state: torch.Tensor) -> torch.Tensor:
        """``H_inner x``."""
        return self._inner_emission_model.project_state_to_f(state)

    def project_state_covariance_to_g(self, covariance: torch.Tensor, full_output_cov: bool = True) -> torch.Tensor:
        """``H_inner S H_innerᵀ`` (the default) or its diagonal."""
        return self._inner_emission_model.project_state_covariance_to_f(covariance, full_output_cov)


class StackEmissionModel(EmissionModel):
    """Emission of ``K`` parallel, independent chains, one per output (emission_model.py:270-378): the emission matrix is
    ``lead + [K, num_data, 1, state_dim]`` - ``K = output_dim`` is the LAST batch dimension, as a ``StackKernel``'s chains carry it -
    and the projections move ``K`` from the batch to the last dimension of the result: ``f_k = H_k x_k`` per chain.  Plain batched
    products: CPU or HIP tensors, differentiable by autograd."""

    def __init__(self, emission_matrix: torch.Tensor) -> None:
        """:param emission_matrix: ``lead + [K, num_data, 1, state_dim]``."""
        if emission_matrix.dim() < 4:
            raise ValueError(f"Emission Matrix must be at least 4D but has shape {tuple(emission_matrix.shape)}")  # emission_model.py:307-310
        if emission_matrix.shape[-2] != 1:
            raise ValueError("StackEmissionModel: every chain has ONE output (emission matrix lead + [K, num_data, 1, state_dim]), got "
                             f"{tuple(emission_matrix.shape)}")
        super().__init__(emission_matrix)

    @property
    def output_dim(self) -> int:
        """``K``, the last batch dimension."""
        return self._H.shape[-4]

    def project_state_to_f(self, state: torch.Tensor) -> torch.Tensor:
        """``lead + [K, num_data, state_dim] -> lead + [num_data, K]`` (emission_model.py:325-344)."""
        if tuple(state.shape[-3:]) != (self.output_dim, self.num_data, self.state_dim):
            raise ValueError(f"state has shape {tuple(state.shape)}, expected [..., {self.output_dim}, {self.num_data}, {self.state_dim}]")
        return torch.sum(self._H[..., 0, :] * state, dim=-1).transpose(-1, -2)

    def project_state_covariance_to_f(self, covariance: torch.Tensor, full_output_cov: bool = False) -> torch.Tensor:
        """``lead + [K, num_data, state_dim, state_dim] -> lead + [num_data, K]``: ``H_k S_k H_k^T`` per chain; ``full_output_cov``:
        the same numbers on the diagonal of ``lead + [num_data, K, K]`` - the chains are independent (emission_model.py:346-378)."""
        if tuple(covariance.shape[-4:]) != (self.output_dim, self.num_data, self.state_dim, self.state_dim):
            raise ValueError(f"covariance has shape {tuple(covariance.shape)}, expected [..., {self.output_dim}, {self.num_data}, "
                             f"{self.state_dim}, {self.state_dim}]")
        h = self._H[..., 0, :]
        var = torch.sum(h * torch.sum(covariance * h[..., None, :], dim=-1), dim=-1).transpose(-1, -2)
        return torch.diag_embed(var) if full_output_cov else var
