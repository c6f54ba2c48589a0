"""
GPU test of the launch path of the fused ops (``_launch`` in markovflow_amd/models/_common.py) on NON-CONTIGUOUS inputs.  The
wrappers make a contiguous copy of such an input and hand the kernel a raw pointer; a pointer keeps no tensor alive, so a copy that is
dropped before the launch goes back to the caching allocator, which hands the same block to the next copy of that size - ``c`` and
``y`` have equal size, and a small ``pair_mean`` and ``pair_cov`` share a size class - and the kernel then reads one tensor's data for
both.  Nothing faults; the numbers are wrong.

Every function runs twice on the same values: once with every floating-point input a strided view (every second element of a buffer
twice as wide, the gaps filled with 1e30), once with contiguous clones held by the test.  Outputs, gradients and updated sites must
be ``torch.equal``.  The shape is the smallest at which two same-sized copies can land in one cached block: ``B = 2`` series of
``N = 5`` points in ``S = 3`` segments, one of them empty, ``2d = 2``, a Gaussian likelihood.  (``h`` of ``iw_log_likelihood`` has
``d = 1`` element and is contiguous whatever its stride.)
"""
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import models as MM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, N, S, TWO_D, K = 2, 5, 3, 2, 2
D, M = TWO_D // 2, S - 1
ALPHA, LR = 0.5, 0.7


def strided(t: torch.Tensor) -> torch.Tensor:
    """The values of ``t`` as a view of every second element of a buffer twice as wide."""
    big = torch.full(tuple(t.shape[:-1]) + (2 * t.shape[-1],), 1e30, dtype=t.dtype, device=t.device)
    big[..., ::2] = t
    view = big[..., ::2]
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


@pytest.fixture(params=[torch.float64, torch.float32], ids=["f64", "f32"])
def values(request):
    """Contiguous inputs of every function under test, on the device."""
    gen = torch.Generator().manual_seed(20)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)

    def spd(*lead):
        a = rnd(*lead, TWO_D, TWO_D)
        return a @ a.transpose(-1, -2) + torch.eye(TWO_D, dtype=torch.float64)

    sym = rnd(B, S, TWO_D, TWO_D)
    vals = dict(w=rnd(B, N, TWO_D), c=0.5 + rnd(B, N) ** 2, y=rnd(B, N), pair_mean=rnd(B, S, TWO_D), pair_cov=spd(B, S),
                cav_mean=rnd(B, S, TWO_D), cav_cov=spd(B, S), seg_const=rnd(B, S), nat1=rnd(B, S, TWO_D),
                nat2=-0.05 * (sym + sym.transpose(-1, -2)), log_norm=rnd(B, S), states=rnd(K, B, N + M, D), u_post=rnd(K, B, M, D),
                h=torch.ones(D, dtype=torch.float64))
    vals = {name: t.to(dtype=request.param, device=DEV).contiguous() for name, t in vals.items()}
    vals["offsets"] = torch.tensor([[0, 2, 2, 5]] * B, dtype=torch.int64, device=DEV)
    return vals


def as_given(vals, names, views: bool):
    """The named inputs as strided views, or as contiguous clones."""
    return [strided(vals[n]) if views else vals[n].clone() for n in names]


def sites(vals, names):
    """Fresh contiguous site tensors: the wrappers update them in place and require them contiguous."""
    return [vals[n].clone() for n in names]


def run_both(call):
    """``call(views)`` for views True and False; every tensor of the first result must equal its partner in the second."""
    got, want = call(True), call(False)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(b).all(), f"result {i} of the contiguous call is not finite"
        assert torch.equal(a, b), f"result {i}: strided inputs give {a}, contiguous clones give {b}"


def test_sparse_expected_log_likelihood(values):
    lik = mfa.Gaussian(0.3)

    def call(views):
        w, c, y, pair_mean, pair_cov = as_given(values, ("w", "c", "y", "pair_mean", "pair_cov"), views)
        pair_mean.requires_grad_()
        pair_cov.requires_grad_()
        out = MM.sparse_expected_log_likelihood(lik, w, c, y, values["offsets"], pair_mean, pair_cov)
        weights = torch.arange(1, B * S + 1, dtype=out.dtype, device=DEV).reshape(B, S)
        g_mean, g_cov = torch.autograd.grad(torch.sum(weights * out), (pair_mean, pair_cov))
        return out.detach(), g_mean.contiguous(), g_cov.contiguous()

    run_both(call)


def test_sparse_cvi_site_update_hip(values):
    lik = mfa.Gaussian(0.3)

    def call(views):
        w, c, y, pair_mean, pair_cov = as_given(values, ("w", "c", "y", "pair_mean", "pair_cov"), views)
        nat1, nat2 = sites(values, ("nat1", "nat2"))
        outs = MM.sparse_cvi_site_update_hip(lik, w, c, y, values["offsets"], pair_mean, pair_cov, LR, nat1, nat2, want_outputs=True)
        return tuple(outs) + (nat1, nat2)

    run_both(call)


def test_sparse_pep_site_update_hip(values):
    lik = mfa.Gaussian(0.3)

    def call(views):
        w, c, y, cav_mean, cav_cov, seg_const = as_given(values, ("w", "c", "y", "cav_mean", "cav_cov", "seg_const"), views)
        nat1, nat2, log_norm = sites(values, ("nat1", "nat2", "log_norm"))
        outs = MM.sparse_pep_site_update_hip(lik, w, c, y, values["offsets"], cav_mean, cav_cov, ALPHA, LR, nat1, nat2, log_norm,
                                             seg_const=seg_const, want_led_sum=True, want_outputs=True)
        return tuple(outs) + (nat1, nat2, log_norm)

    run_both(call)


def test_iw_log_likelihood(values):
    lik = mfa.Gaussian(0.3)

    def call(views):
        w, y, states, u_post = as_given(values, ("w", "y", "states", "u_post"), views)
        u_post.requires_grad_()
        out = MM.iw_log_likelihood(lik, values["h"], w, y, values["offsets"], states, u_post)
        weights = torch.arange(1, K * B + 1, dtype=out.dtype, device=DEV).reshape(K, B)
        (g_u,) = torch.autograd.grad(torch.sum(weights * out), (u_post,))
        return out.detach(), g_u.contiguous()

    run_both(call)
