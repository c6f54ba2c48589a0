"""
Reverse mode through the block-tridiagonal OPERATORS on the GPU: the autograd Functions of
markovflow_amd/_autograd_ops.py over the HIP kernels, against torch's reverse mode through the dense matrices, and the chain the
reference's CVI models differentiate - ``dist_p.precision -> naturals_to_ssm_params -> kl_divergence``
(/root/reference/markovflow/models/variational_cvi.py:105-136,402; the operators' gradients there come from banded_matrices,
block_tri_diag.py:22-31) - against central differences of the same (forward-only, oracle-checked) kernels.  fp64.
"""
import collections

import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _autograd_ops as ag
from markovflow_amd import _lib
from markovflow_amd import ssm_gaussian_transformations as G
from test_autograd_ops import (adjoint_case, blocks_of, dense_cholesky_blocks, dense_inverse_blocks, dense_of, random_factor,
                               random_spd, spd_blocks_of_factor)
from test_gpu_kalman import DEV, nn, random_ssm, tt

pytestmark = pytest.mark.gpu
F64 = torch.float64


def dev(x):
    return None if x is None else x.to(DEV)


@pytest.mark.parametrize("batch,n,d", [((), 7, 3), ((2,), 70, 6), ((3,), 5, 2), ((), 40, 9)])
def test_cholesky_solve_inverse_blocks_and_products_vs_dense_autograd(batch, n, d):
    rng = np.random.default_rng(5)
    (diag, sub), _ = random_spd(rng, batch, n, d)
    rhs = torch.tensor(rng.normal(size=(2,) + batch + (n, d)), dtype=F64)
    w1, w2, w3, w4 = (torch.tensor(rng.normal(size=s), dtype=F64, device=DEV) for s in
                      (batch + (n, d, d), batch + (n - 1, d, d), (2,) + batch + (n, d), (2,) + batch + (n, d)))

    def loss(dg, sb, r, native):
        if native:
            sym = mfa.SymmetricBlockTriDiagonal(dg, sb)
            chol = sym.cholesky
            inv_d, inv_s = chol._diag_and_sub_of_inverse(want_sub=True)
            x, xt = chol.solve(r), chol.solve(r, transpose_left=True)
            prod = sym.dense_mult(r) + chol.dense_mult(r) + chol.dense_mult(r, transpose_left=True)
            logdet = chol.abs_log_det()
        else:
            full = dense_of(0.5 * (dg + dg.transpose(-1, -2)), sb, True)
            cf = torch.linalg.cholesky(full)
            inv_d, inv_s = blocks_of(torch.linalg.inv(full), n, d)
            flat = r.reshape(r.shape[:-2] + (n * d, 1))
            x = torch.linalg.solve_triangular(cf, flat, upper=False).reshape(r.shape)
            xt = torch.linalg.solve_triangular(cf.transpose(-1, -2), flat, upper=True).reshape(r.shape)
            prod = ((full + cf + cf.transpose(-1, -2)) @ flat).reshape(r.shape)
            logdet = torch.sum(torch.log(torch.diagonal(cf, dim1=-2, dim2=-1)), dim=-1)
        return (torch.sum(inv_d * w1) + torch.sum(inv_s * w2) + torch.sum(x * w3) + torch.sum(xt * w4) + torch.sum(prod * w3)
                + torch.sum(logdet))

    grads = []
    for native in (True, False):
        dg, sb, r = (dev(t).clone().requires_grad_(True) for t in (diag, sub, rhs))
        val = loss(dg, sb, r, native)
        val.backward()
        grads.append((float(val.detach()), dg.grad, sb.grad, r.grad))
    assert grads[0][0] == pytest.approx(grads[1][0], rel=1e-9)
    for g1, g2 in zip(grads[0][1:], grads[1][1:]):
        scale = float(g2.abs().max())
        assert float((g1 - g2).abs().max()) <= 1e-8 * scale


def test_precision_is_differentiable(rng):
    kw = random_ssm(rng, (2,), 12, 3, 1, well=True)
    leaves = [tt(kw[k]).requires_grad_(True) for k in ("mu0", "chol_p0", "a_s", "b_s", "chol_q")]
    ssm = mfa.StateSpaceModel(*leaves)
    prec = ssm.precision
    plain = mfa.StateSpaceModel(*(x.detach() for x in leaves)).precision
    np.testing.assert_allclose(nn(prec.block_diagonal), nn(plain.block_diagonal), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(nn(prec.block_sub_diagonal), nn(plain.block_sub_diagonal), rtol=1e-10, atol=1e-12)
    (prec.block_diagonal.sum() + 2 * prec.block_sub_diagonal.sum()).backward()
    assert all(x.grad is not None and bool(torch.isfinite(x.grad).all()) for x in (leaves[1], leaves[2], leaves[4]))


def _cvi_kl(lengthscale, variance, t_pts, nat1, nat2):
    """KL(q || p) with p the Matern-3/2 prior and q = prior x Gaussian sites, built the way variational_cvi.py:105-136 builds it."""
    kern = mfa.Matern32(lengthscale, variance, jitter=1e-9)
    dist_p = kern.state_space_model(t_pts)
    prec = dist_p.precision
    h = kern.generate_emission_model(t_pts).emission_matrix                        # [.., T, 1, d]
    theta_lin = (h.transpose(-1, -2) @ nat1[..., None])[..., 0]
    theta_diag = -0.5 * prec.block_diagonal + h.transpose(-1, -2) @ nat2 @ h
    theta_sub = -prec.block_sub_diagonal
    a_s, offsets, chol_p0, chol_q, mu0 = G.naturals_to_ssm_params(theta_lin, theta_diag, theta_sub)
    dist_q = mfa.StateSpaceModel(mu0, chol_p0, a_s, offsets, chol_q)
    return torch.sum(dist_q.kl_divergence(dist_p))


def test_cvi_shaped_gradient_through_precision_and_naturals(rng):
    """d KL / d lengthscale, d KL / d variance and d KL / d sites through the whole chain against central differences."""
    bsz, n = 2, 60
    t_pts = torch.cumsum(0.05 + 0.1 * torch.rand(bsz, n, dtype=F64, device=DEV), dim=-1)
    nat1 = tt(rng.normal(size=(bsz, n, 1)))
    nat2 = tt(-0.5 * rng.uniform(0.5, 2.0, size=(bsz, n, 1, 1)))
    ls0 = tt(np.array([0.7, 1.3]))
    var0 = tt(np.array([1.2, 0.8]))
    ls, var = ls0.clone().requires_grad_(True), var0.clone().requires_grad_(True)
    n1, n2 = nat1.clone().requires_grad_(True), nat2.clone().requires_grad_(True)
    kl = _cvi_kl(ls, var, t_pts, n1, n2)
    kl.backward()
    with torch.no_grad():
        for which, base, grad in (("lengthscale", ls0, ls.grad), ("variance", var0, var.grad)):
            for i in range(bsz):
                hstep = 1e-6
                up, dn = base.clone(), base.clone()
                up[i] += hstep; dn[i] -= hstep
                args_up = (up, var0) if which == "lengthscale" else (ls0, up)
                args_dn = (dn, var0) if which == "lengthscale" else (ls0, dn)
                fd = (float(_cvi_kl(*args_up, t_pts, nat1, nat2)) - float(_cvi_kl(*args_dn, t_pts, nat1, nat2))) / (2 * hstep)
                assert float(grad[i]) == pytest.approx(fd, rel=2e-5, abs=1e-7), which
        d1 = tt(rng.normal(size=nat1.shape))
        hstep = 1e-6
        fd = (float(_cvi_kl(ls0, var0, t_pts, nat1 + hstep * d1, nat2)) - float(_cvi_kl(ls0, var0, t_pts, nat1 - hstep * d1, nat2))) / (2 * hstep)
        assert float(torch.sum(n1.grad * d1)) == pytest.approx(fd, rel=2e-5, abs=1e-7)
        assert bool(torch.isfinite(n2.grad).all())


# ---- the HIP adjoints of cholesky / block_diagonal_of_inverse (mf_btd_cholesky_grad_*, mf_btd_diag_of_inverse_grad_*) -------------
CHOL_GRAD, INV_GRAD = "mf_btd_cholesky_grad", "mf_btd_diag_of_inverse_grad"


@pytest.fixture
def abi_calls(monkeypatch):
    """Counts the entry points that go through ``_lib.call`` (``_autograd_ops`` reaches the adjoint kernels as ``_lib.call``): a
    parity test that can pass without the kernel having run proves nothing about the kernel."""
    counts = collections.Counter()
    real = _lib.call

    def spy(base, *args, **kwargs):
        counts[base] += 1
        return real(base, *args, **kwargs)

    monkeypatch.setattr(_lib, "call", spy)
    return counts


class Ctx:
    pass


@pytest.mark.parametrize("batch,n,d,with_sub,which", [
    ((3,), 300, 6, True, "both"), ((2,), 1000, 4, True, "both"), ((4100,), 12, 4, True, "both"), ((2, 3), 40, 2, True, "both"),
    ((5,), 64, 9, True, "both"), ((3,), 50, 7, True, "both"), ((2,), 30, 5, False, "both"), ((3,), 1, 3, False, "both"),
    ((2,), 2, 6, True, "both"), ((2,), 200, 6, True, "diag"), ((2,), 200, 6, True, "sub"), ((1,), 3000, 1, True, "both"),
    # 10 <= d <= 32 (round 6, csrc/mf_adj.hip, register MFMA tiles): chains shorter than 32 blocks - one wavefront per series walks
    # the recurrence - and longer ones - local terms + congruence scans, parallel in time (ragged chunk partitions, one of the two
    # incoming gradients missing) - incl. the reference's largest tested operator shape, d = 30, T = 1001
    # (tests/unit/test_ssm_gaussian_transformations.py:40-46)
    ((3,), 40, 12, True, "both"), ((2,), 25, 16, True, "both"), ((2,), 30, 24, True, "diag"), ((2,), 30, 24, True, "sub"),
    ((1,), 12, 32, True, "both"), ((2,), 9, 17, False, "both"), ((3,), 1, 20, False, "both"), ((1,), 1001, 30, True, "both"),
    ((2,), 77, 16, True, "both"), ((3,), 100, 20, True, "diag"), ((2,), 64, 32, True, "sub"), ((5,), 33, 10, True, "both"),
    ((2,), 130, 24, True, "both"), ((70,), 45, 15, True, "both"),
    # one incoming gradient missing (NULL) in the sequential kernels (n < 32) of both tile counts and in the scans at d <= 16
    ((2,), 12, 16, True, "diag"), ((2,), 12, 10, True, "sub"), ((2,), 5, 31, True, "sub"), ((2,), 31, 17, True, "diag"),
    ((1,), 40, 15, True, "diag"), ((2,), 33, 16, True, "sub"), ((3,), 40, 12, False, "diag"), ((2,), 1, 32, False, "diag"),
])
def test_hip_operator_adjoints_against_the_torch_recursions(batch, n, d, with_sub, which, abi_calls):
    """The kernels against the block-by-block torch recursions (which tests/test_autograd_ops.py pins on dense autograd): few long
    series (recursion parallel in time), many short ones (a lane per series), no coupling, a single block, only one of the two
    output gradients given (a NULL pointer at the C ABI: through ``loss.backward()`` autograd hands zeros instead).  ``backward`` is
    called directly, with the tape OFF as under ``loss.backward()`` - with the tape on it takes the torch route (create_graph)."""
    rng = np.random.default_rng(11)
    # (d >= 10: G_k = W_k L_k^-1 has to stay a contraction for the recurrences to be evaluable over a thousand blocks at all - in any
    # implementation: the couplings and the strict lower triangles are scaled with the state dimension, random_factor)
    ldiag, lsub = (x.to(DEV) for x in random_factor(rng, batch, n, d, scaled=d >= 10))
    if not with_sub or n == 1:
        lsub = None
    g1 = torch.tensor(rng.normal(size=tuple(ldiag.shape)), dtype=F64, device=DEV) if which in ("both", "diag") else None
    g2 = (torch.tensor(rng.normal(size=tuple(lsub.shape)), dtype=F64, device=DEV)
          if (lsub is not None and which in ("both", "sub")) else None)
    assert ag._hip_grad_ws(ldiag) is not None
    # cholesky: gradients w.r.t. the factor's blocks -> gradients w.r.t. the matrix' blocks
    ctx = Ctx()
    ctx.has_sub = lsub is not None
    ctx.saved_tensors = (ldiag, lsub if lsub is not None else ldiag.new_zeros(0))
    with torch.no_grad():
        _, gd, gs = ag.BtdCholesky.backward(ctx, g1, g2)
    assert (abi_calls[CHOL_GRAD], abi_calls[INV_GRAD]) == (1, 0), "the cholesky adjoint kernel has to take this call"
    want_d, want_s = ag._cholesky_backward_torch(ldiag, lsub, g1, g2)
    scale = float(want_d.abs().max())
    assert float((gd - want_d).abs().max()) <= 1e-9 * scale
    if lsub is not None:
        assert float((gs - want_s).abs().max()) <= 1e-9 * max(float(want_s.abs().max()), scale)
    # block_diagonal_of_inverse: gradients w.r.t. the blocks of the inverse -> gradients w.r.t. the factor's blocks
    chol = mfa.LowerTriangularBlockTriDiagonal(ldiag, lsub)
    odiag, _ = chol._diag_and_sub_of_inverse(want_sub=lsub is not None)
    ctx = Ctx()
    ctx.has_sub, ctx.want_sub = lsub is not None, lsub is not None
    ctx.saved_tensors = (ldiag, lsub if lsub is not None else ldiag.new_zeros(0), odiag.contiguous())
    with torch.no_grad():
        _, gl, gw, _ = ag.BtdInverseBlocks.backward(ctx, g1, g2)
    assert (abi_calls[CHOL_GRAD], abi_calls[INV_GRAD]) == (1, 1), "the inverse blocks' adjoint kernel has to take this call"
    want_l, want_w = ag._inverse_blocks_backward_torch(ldiag, lsub, g1, g2)
    if want_l is None:
        want_l = torch.zeros_like(ldiag)
    scale = max(float(want_l.abs().max()), 1e-30)
    assert float((gl - want_l).abs().max()) <= 1e-9 * scale
    if lsub is not None:
        if want_w is None:
            want_w = torch.zeros_like(lsub)
        assert float((gw - want_w).abs().max()) <= 1e-9 * max(float(want_w.abs().max()), scale)


def test_hip_operator_adjoints_fp32(abi_calls):
    rng = np.random.default_rng(12)
    ldiag, lsub = (x.to(device=DEV, dtype=torch.float32) for x in random_factor(rng, (3,), 120, 5))
    g1 = torch.tensor(rng.normal(size=tuple(ldiag.shape)), dtype=torch.float32, device=DEV)
    g2 = torch.tensor(rng.normal(size=tuple(lsub.shape)), dtype=torch.float32, device=DEV)
    ctx = Ctx()
    ctx.has_sub = True
    ctx.saved_tensors = (ldiag, lsub)
    with torch.no_grad():
        _, gd, gs = ag.BtdCholesky.backward(ctx, g1, g2)
    assert abi_calls[CHOL_GRAD] == 1
    want_d, want_s = ag._cholesky_backward_torch(ldiag.double(), lsub.double(), g1.double(), g2.double())
    assert float((gd.double() - want_d).abs().max()) <= 2e-4 * float(want_d.abs().max())
    assert float((gs.double() - want_s).abs().max()) <= 2e-4 * float(want_s.abs().max())


@pytest.mark.parametrize("d,n,bsz", [(40, 50, 2), (64, 130, 1), (33, 9, 3)])
def test_operator_adjoints_beyond_the_kernels_take_the_scan_forms(d, n, bsz):
    """d > 32 (fp32 operators on the panel / tile engine): no adjoint kernel; a GPU tensor takes the scan forms of
    markovflow_amd/_autograd_ops.py (local terms + a Hillis-Steele congruence scan, no Python loop over the blocks) - checked
    against the block loops in float32 arithmetic on the same device."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    f32 = torch.float32
    ld = torch.tril((4.0 / d) * 0.3 * torch.randn(bsz, n, d, d, dtype=f32, device=DEV, generator=gen), -1) + torch.diag_embed(
        1 + torch.rand(bsz, n, d, dtype=f32, device=DEV, generator=gen))
    ls = (2.0 / d) * 0.3 * torch.randn(bsz, n - 1, d, d, dtype=f32, device=DEV, generator=gen)
    assert ag._hip_grad_ws(ld) is None and ag._scan_pays(ld)
    dg = ld @ ld.transpose(-1, -2)
    dg[:, 1:] += ls @ ls.transpose(-1, -2)
    sb = ls @ ld[:, :-1].transpose(-1, -2)
    dg.requires_grad_(True); sb.requires_grad_(True)
    w = torch.randn(bsz, n, d, d, dtype=f32, device=DEV, generator=gen)
    inv_d, inv_s = mfa.SymmetricBlockTriDiagonal(dg, sb).cholesky._diag_and_sub_of_inverse(want_sub=True)
    (torch.sum(inv_d * w) + torch.sum(inv_s)).backward()
    got_d, got_s = dg.grad.clone(), sb.grad.clone()
    # the same chain with the block loops
    chol = mfa.SymmetricBlockTriDiagonal(dg.detach(), sb.detach()).cholesky
    cd, cs = chol.block_diagonal, chol.block_sub_diagonal
    gl, gw = ag._inverse_blocks_backward_torch(cd, cs, w, torch.ones_like(sb))
    want_d, want_s = ag._cholesky_backward_torch(cd, cs, gl, gw)
    scale = float(want_d.abs().max())
    assert float((got_d - want_d).abs().max()) <= 2e-3 * scale
    assert float((got_s - want_s).abs().max()) <= 2e-3 * max(float(want_s.abs().max()), scale)



# ---- 10 <= d <= 32: the register-tile adjoints (csrc/mf_adj.hip) through the public API and a real loss.backward() ----------------
# Every case asserts the ROUTE (abi_calls: the adjoint entry point was called exactly once) and compares with plain fp64 that is not
# the code under test: torch reverse mode through the dense n d x n d matrix where that fits (n d <= 2500), else the block loops of
# _autograd_ops.py, which tests/test_autograd_ops.py pins on dense autograd at these d.  The cases follow the branches of mf_adj.hip /
# mf_api.hip: the row tables' hand-over (10 <= d <= 15), one tile (d <= 16) or four (d > 16), identity padding (d = 10 ... 15, 17 ... 31),
# the sequential kernel (n < 32) or local terms + scan (n >= 32: ragged chunk partitions at n = 77, 130, 1001), one wavefront per
# series / per block with few series and with more than there are compute units, a block-diagonal factor.
DENSE_LIMIT = 2500
TILE_D = (10, 12, 15, 16, 17, 20, 24, 31, 32)


def _dev_case(seed, batch, n, d, scaled, with_sub=True, dtype=F64):
    ld, ls, g1, g2 = adjoint_case(seed, batch, n, d, scaled)
    if not with_sub:
        ls = g2 = None
    return tuple(None if x is None else x.to(device=DEV, dtype=dtype) for x in (ld, ls, g1, g2))


def _leaf(x):
    return None if x is None else x.clone().requires_grad_(True)


def _assert_close(got, want, ref):
    """fp64 tolerances of this file: against dense autograd 1e-8 x the reference's largest entry, tensor by tensor (as in
    test_cholesky_solve_inverse_blocks_and_products_vs_dense_autograd); against the block loops 1e-9 x the largest entry (the
    couplings' gradient on the scale of the larger of the two, as in test_hip_operator_adjoints_against_the_torch_recursions)."""
    scale = max(float(want[0].abs().max()), 1e-30)
    errs = [float((got[0] - want[0]).abs().max()) / scale]
    if want[1] is not None:
        s1 = float(want[1].abs().max())
        errs.append(float((got[1] - want[1]).abs().max()) / (s1 if ref == "dense" else max(s1, scale)))
    print(f"  relative error ({ref}): " + ", ".join(f"{e:.3g}" for e in errs))
    for e in errs:
        assert e <= (1e-8 if ref == "dense" else 1e-9)
    return errs


def _cholesky_through_backward(calls, ld, ls, g1, g2, which="both"):
    """``SymmetricBlockTriDiagonal(diag, sub).cholesky`` of ``L L^T`` under a real ``loss.backward()``: (gradients w.r.t. the
    matrix' blocks, the factor the forward kernel produced)."""
    dg, sb = spd_blocks_of_factor(ld, ls)
    a, b = _leaf(dg), _leaf(sb)
    before = (calls[CHOL_GRAD], calls[INV_GRAD])
    chol = mfa.SymmetricBlockTriDiagonal(a, b).cholesky
    loss = 0.0
    if which in ("both", "diag"):
        loss = loss + torch.sum(chol.block_diagonal * g1)
    if which in ("both", "sub") and b is not None:
        loss = loss + torch.sum(chol.block_sub_diagonal * g2)
    loss.backward()
    assert (calls[CHOL_GRAD] - before[0], calls[INV_GRAD] - before[1]) == (1, 0), "mf_btd_cholesky_grad has to take this backward"
    cs = chol.block_sub_diagonal
    return (a.grad, None if b is None else b.grad), (chol.block_diagonal.detach(), None if cs is None else cs.detach()), (dg, sb)


def _cholesky_dense_reference(dg, sb, g1, g2, which="both"):
    a, b = _leaf(dg), _leaf(sb)
    cd, cs = dense_cholesky_blocks(a, b)
    loss = 0.0
    if which in ("both", "diag"):
        loss = loss + torch.sum(torch.tril(cd) * g1)
    if which in ("both", "sub") and b is not None:
        loss = loss + torch.sum(cs * g2)
    loss.backward()
    return a.grad, None if b is None else b.grad


def _inverse_through_backward(calls, ld, ls, g1, g2, which="both", want_sub=True):
    a, b = _leaf(ld), _leaf(ls)
    before = (calls[CHOL_GRAD], calls[INV_GRAD])
    op = mfa.LowerTriangularBlockTriDiagonal(a, b)
    if want_sub:
        od, osub = op._diag_and_sub_of_inverse(want_sub=True)
    else:
        od, osub = op.block_diagonal_of_inverse(), None
    loss = 0.0
    if which in ("both", "diag"):
        loss = loss + torch.sum(od * g1)
    if which in ("both", "sub") and osub is not None:
        loss = loss + torch.sum(osub * g2)
    loss.backward()
    assert (calls[CHOL_GRAD] - before[0], calls[INV_GRAD] - before[1]) == (0, 1), "mf_btd_diag_of_inverse_grad has to take this backward"
    return a.grad, None if b is None else b.grad


def _inverse_dense_reference(ld, ls, g1, g2, which="both", want_sub=True):
    a, b = _leaf(ld), _leaf(ls)
    od, osub = dense_inverse_blocks(a, b)
    loss = 0.0
    if which in ("both", "diag"):
        loss = loss + torch.sum(od * g1)
    if which in ("both", "sub") and osub is not None and want_sub:
        loss = loss + torch.sum(osub * g2)
    loss.backward()
    return torch.tril(a.grad), None if b is None else b.grad


def _both_operators(calls, batch, n, d, scaled, ref, with_sub=True, which="both", want_sub=True):
    ld, ls, g1, g2 = _dev_case(21, batch, n, d, scaled, with_sub)
    assert ref == "loop" or n * d <= DENSE_LIMIT
    assert ag._hip_grad_ws(ld) is not None
    only = lambda g, name: g if which in ("both", name) else None                       # noqa: E731
    got, (cd, cs), (dg, sb) = _cholesky_through_backward(calls, ld, ls, g1, g2, which)
    if ref == "dense":
        want = _cholesky_dense_reference(dg, sb, g1, g2, which)
    else:
        want = ag._cholesky_backward_torch(cd, cs, only(g1, "diag"), None if cs is None else only(g2, "sub"))
    _assert_close(got, want, ref)
    got = _inverse_through_backward(calls, ld, ls, g1, g2, which, want_sub)
    if ref == "dense":
        want = _inverse_dense_reference(ld, ls, g1, g2, which, want_sub)
    else:
        gl, gw = ag._inverse_blocks_backward_torch(ld, ls, only(g1, "diag"), only(g2, "sub") if (ls is not None and want_sub) else None)
        want = (gl if gl is not None else torch.zeros_like(ld), None if ls is None else (gw if gw is not None else torch.zeros_like(ls)))
    _assert_close(got, want, ref)


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33])
@pytest.mark.parametrize("d", TILE_D + (30,))
def test_tile_adjoints_around_the_hand_over_to_the_scans_vs_dense_autograd(abi_calls, n, d):
    """Every state dimension of the tile kernels, either side of ADJ_PAR_MIN_BLOCKS = 32 (sequential kernel below, local terms + scan
    from there on), a single block, a single coupling; the scaling of long chains."""
    _both_operators(abi_calls, (2,), n, d, True, "dense")


# Unscaled, n = 12, d >= 24 takes the block loops as its reference, evaluated at the factor the forward kernel produced.  There
# ``L L^T`` is ill-conditioned (the gradients reach 1e9 at d = 32) and dense autograd linearises at ITS OWN Cholesky factor, which
# differs from the kernel's by cond x eps: measured against dense autograd, ``cholesky``'s gradients differ by 8e-10 (d = 24), 2.0e-6
# (d = 31) and 3.4e-6 (d = 32) of the largest entry, while the inverse blocks' adjoint of the same factors - no factorisation in front
# of it - agrees with dense autograd to 1e-15, and so does the cholesky adjoint with the loops at a common factor.  The 1e-8 bound
# is beyond the dense reference itself there; tests/test_autograd_ops.py pins the loops on dense autograd for these very inputs.
@pytest.mark.parametrize("d,n,ref", [(d, n, "dense") for d in TILE_D for n in (2, 5)] + [(d, 12, "dense") for d in TILE_D if d < 24]
                         + [(d, 12, "loop") for d in TILE_D if d >= 24])
def test_tile_adjoints_on_unscaled_factors(abi_calls, d, n, ref):
    """Short chains with the unscaled factor: the tiles see entries of ordinary size (and gradients that grow by an order of
    magnitude per block at d = 32: the bounds are relative to the largest entry)."""
    _both_operators(abi_calls, (3,), n, d, False, ref)


@pytest.mark.parametrize("batch,n,d,ref", [
    # ragged chunk partitions of the scans
    ((1,), 77, 10, "dense"), ((1,), 77, 16, "dense"), ((1,), 77, 17, "dense"), ((1,), 77, 32, "dense"), ((3,), 77, 24, "loop"),
    ((1,), 130, 10, "dense"), ((1,), 130, 12, "dense"), ((1,), 130, 15, "dense"), ((1,), 130, 16, "dense"), ((1,), 130, 17, "dense"),
    ((2,), 130, 20, "loop"), ((2,), 130, 31, "loop"), ((1,), 130, 32, "loop"),
    # the reference's largest tested operator shape (tests/unit/test_ssm_gaussian_transformations.py:40-46) and its neighbours
    ((1,), 1001, 30, "loop"), ((2,), 1001, 10, "loop"), ((1,), 1001, 16, "loop"), ((1,), 1001, 17, "loop"),
    # many series: a wavefront each (sequential) / per block (local terms); more series than compute units
    ((70,), 45, 15, "loop"), ((70,), 33, 17, "dense"), ((70,), 12, 32, "dense"), ((600,), 2, 16, "dense"), ((600,), 5, 24, "loop"),
    ((600,), 33, 10, "loop"), ((600,), 31, 20, "loop"),
    # two leading batch dimensions
    ((2, 3), 33, 12, "dense"), ((2, 2), 7, 20, "dense"), ((3, 2), 40, 31, "dense"),
])
def test_tile_adjoints_long_chains_and_many_series(abi_calls, batch, n, d, ref):
    _both_operators(abi_calls, batch, n, d, True, ref)


@pytest.mark.parametrize("batch,n,d", [((2,), 9, 17), ((3,), 1, 10), ((3,), 1, 20), ((2,), 1, 32), ((3,), 40, 12), ((2,), 33, 32),
                                       ((1,), 5, 15), ((2, 2), 31, 16), ((70,), 4, 24)])
def test_tile_adjoints_of_a_block_diagonal_factor(abi_calls, batch, n, d):
    """``lsub is None``: B n independent blocks (n = 1 and n > 1).  d = 17, n = 9 raised NotImplementedError inside backward()
    before the entry points re-entered with every block as a series of its own."""
    _both_operators(abi_calls, batch, n, d, True, "dense", with_sub=False)
    _both_operators(abi_calls, batch, n, d, False, "dense", with_sub=False)


@pytest.mark.parametrize("which", ["diag", "sub"])
@pytest.mark.parametrize("batch,n,d", [((2,), 12, 10), ((2,), 40, 16), ((2,), 12, 24), ((2,), 40, 31)])
def test_tile_adjoints_with_one_output_in_the_loss(abi_calls, batch, n, d, which):
    """Only the diagonal or only the sub-diagonal blocks enter the loss (autograd hands the kernel zeros for the other)."""
    _both_operators(abi_calls, batch, n, d, True, "dense", which=which)


@pytest.mark.parametrize("batch,n,d", [((2,), 12, 10), ((2,), 40, 10), ((3,), 12, 17), ((2,), 40, 17), ((2,), 12, 32), ((1,), 40, 32),
                                       ((2,), 33, 16)])
def test_tile_adjoint_of_block_diagonal_of_inverse_without_the_sub_diagonal_output(abi_calls, batch, n, d):
    """``block_diagonal_of_inverse()`` (``want_sub=False``) of a factor WITH couplings: no incoming gradient for the sub-diagonal
    blocks of the inverse (NULL at the C ABI), still a gradient for the couplings."""
    ld, ls, g1, g2 = _dev_case(22, batch, n, d, True)
    got = _inverse_through_backward(abi_calls, ld, ls, g1, g2, want_sub=False)
    _assert_close(got, _inverse_dense_reference(ld, ls, g1, g2, want_sub=False), "dense")
    assert float(got[1].abs().max()) > 0


# fp32 at d >= 10.  The yardstick is the error of the block loops evaluated in float32 against the same loops in float64 on identical
# (float32-representable) inputs, adjoint_case(12, ...), measured on the CPU with the metric of _fp32_error below:
#     case (batch, n, d, scaled)      cholesky adjoint    inverse blocks' adjoint
FP32_LOOP_ERROR = {
    ((3,), 5, 10, False): (3.2e-07, 9.3e-08),
    ((3,), 12, 10, True): (1.9e-07, 2.6e-07),
    ((2,), 200, 10, True): (2e-07, 1.6e-07),
    ((3,), 5, 16, False): (4.5e-07, 1.8e-07),
    ((3,), 12, 16, True): (2e-07, 2.5e-07),
    ((2,), 200, 16, True): (3.1e-07, 2.2e-07),
    ((3,), 5, 24, False): (1.8e-07, 2.7e-07),
    ((3,), 12, 24, True): (2.3e-07, 1.5e-07),
    ((2,), 200, 24, True): (3.3e-07, 2.8e-07),
    ((3,), 5, 32, False): (7.5e-07, 6e-07),
    ((3,), 12, 32, True): (2.6e-07, 2.2e-07),
    ((2,), 200, 32, True): (4.5e-07, 3.2e-07),
}
# The kernels are allowed FP32_FACTOR x the per-case figure: the MFMA accumulation order and the scans' reassociation differ from
# the loops'; nothing else justifies more.
FP32_FACTOR = 4.0


def _fp32_error(got, want):
    sd = float(want[0].abs().max())
    ss = max(float(want[1].abs().max()), sd)
    return max(float((got[0].double() - want[0]).abs().max()) / sd, float((got[1].double() - want[1]).abs().max()) / ss)


@pytest.mark.parametrize("case", list(FP32_LOOP_ERROR), ids=lambda c: "B%s-n%d-d%d-%s" % ("x".join(map(str, c[0])), c[1], c[2], "scaled" if c[3] else "plain"))
def test_tile_adjoints_fp32(abi_calls, case):
    """float32 through backward(), short and long chains: against the block loops in float64 on the inputs the kernel saw (for
    ``cholesky``: the factor its float32 forward produced)."""
    batch, n, d, scaled = case
    f32 = torch.float32
    ld, ls, g1, g2 = _dev_case(12, batch, n, d, scaled, dtype=f32)
    assert ag._hip_grad_ws(ld) is not None
    up = lambda x: x.double()                                                            # noqa: E731
    got, (cd, cs), _ = _cholesky_through_backward(abi_calls, ld, ls, g1, g2)
    assert got[0].dtype == f32
    e_chol = _fp32_error(got, ag._cholesky_backward_torch(up(cd), up(cs), up(g1), up(g2)))
    got = _inverse_through_backward(abi_calls, ld, ls, g1, g2)
    e_inv = _fp32_error(got, ag._inverse_blocks_backward_torch(up(ld), up(ls), up(g1), up(g2)))
    print(f"  fp32 relative error: cholesky {e_chol:.3g} (loops {FP32_LOOP_ERROR[case][0]:.3g}), inverse blocks {e_inv:.3g} "
          f"(loops {FP32_LOOP_ERROR[case][1]:.3g})")
    assert e_chol <= FP32_FACTOR * FP32_LOOP_ERROR[case][0]
    assert e_inv <= FP32_FACTOR * FP32_LOOP_ERROR[case][1]


# ---- robustness: no further reference needed ---------------------------------------------------------------------------------------
def _direct_backwards(calls, ld, ls, sigma, g_ldiag, g1, g2):
    """Both ``backward``s called directly with the tape off (a saved factor cannot be given junk through the public API);
    ``g_ldiag``: the cholesky adjoint's incoming gradient of the factor's diagonal blocks, ``g1``: the inverse blocks' adjoint's
    incoming gradient of the diagonal blocks of the inverse (a full matrix: nothing to ignore there)."""
    before = (calls[CHOL_GRAD], calls[INV_GRAD])
    none = ld.new_zeros(0)
    with torch.no_grad():
        ctx = Ctx()
        ctx.has_sub = ls is not None
        ctx.saved_tensors = (ld, ls if ls is not None else none)
        _, gd, gs = ag.BtdCholesky.backward(ctx, g_ldiag, g2)
        ctx = Ctx()
        ctx.has_sub = ctx.want_sub = ls is not None
        ctx.saved_tensors = (ld, ls if ls is not None else none, sigma)
        _, gl, gw, _ = ag.BtdInverseBlocks.backward(ctx, g1, g2)
    assert (calls[CHOL_GRAD] - before[0], calls[INV_GRAD] - before[1]) == (1, 1)
    return [x for x in (gd, gs, gl, gw) if x is not None]


@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("batch,n,d", [((2,), 12, 10), ((2,), 40, 15), ((2,), 12, 16), ((2,), 40, 17), ((2,), 12, 31), ((2,), 40, 32),
                                       ((2,), 1, 24)])
def test_tile_adjoints_ignore_the_strict_upper_triangles(abi_calls, batch, n, d, scaled):
    """Finite junk in the strict upper triangles of ``ldiag`` and of the incoming ``g_ldiag`` must not change a result."""
    if not scaled and n > 12:
        n = 7
    ld, ls, g1, g2 = _dev_case(23, batch, n, d, scaled)
    sigma = mfa.LowerTriangularBlockTriDiagonal(ld, ls)._diag_and_sub_of_inverse(want_sub=False)[0].contiguous()
    junk = torch.triu(torch.tensor(np.random.default_rng(5).normal(size=tuple(ld.shape)), dtype=F64, device=DEV) * 3.0 + 1.0, 1)
    clean = _direct_backwards(abi_calls, ld, ls, sigma, torch.tril(g1), g1, g2)
    dirty = _direct_backwards(abi_calls, ld + junk, ls, sigma, torch.tril(g1) + 2.0 * junk, g1, g2)
    assert len(clean) == len(dirty) == (4 if ls is not None else 2)
    for x, y in zip(clean, dirty):
        assert float((x - y).abs().max()) <= 1e-12 * float(x.abs().max())
    # ... and the factor's junk reaches neither the forward kernel nor its adjoint through the public API
    got = _inverse_through_backward(abi_calls, ld + junk, ls, g1, g2)
    gl = clean[2 if ls is not None else 1]
    assert float((got[0] - gl).abs().max()) <= 1e-12 * float(gl.abs().max())


def _abi_adjoints(ld, ls, g1, g2, with_ws):
    """Both entry points through the raw C ABI, output buffers filled with NaN beforehand; ``with_ws`` False: ``ws = NULL,
    ws_bytes = 0`` (the sequential kernels, whatever the length of the chain)."""
    d, n = ld.shape[-1], ld.shape[-3]
    flat = lambda t: None if t is None else t.reshape((-1, t.shape[-3], d, d)).contiguous()            # noqa: E731
    ld, ls, g1, g2 = flat(ld), flat(ls), flat(g1), flat(g2)
    bsz = ld.shape[0]
    sigma = mfa.LowerTriangularBlockTriDiagonal(ld, ls)._diag_and_sub_of_inverse(want_sub=False)[0].contiguous()
    wsb = int(_lib.load().mf_btd_grad_workspace_bytes(bsz, n, d, ld.element_size())) if with_ws else 0
    assert wsb > 0 or not with_ws
    ws = _lib.workspace(wsb, ld.device)
    nan = lambda t: None if t is None else torch.full_like(t, float("nan"))             # noqa: E731
    gd, gs, gl, gw = nan(ld), nan(ls), nan(ld), nan(ls)
    st = _lib.stream_ptr(ld.device)
    rc = _lib.call_rc(CHOL_GRAD, ld.dtype, bsz, n, d, _lib.ptr(ld), _lib.ptr(ls), _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(gd),
                      _lib.ptr(gs), _lib.ptr(ws), wsb, st)
    assert rc == 0, rc
    rc = _lib.call_rc(INV_GRAD, ld.dtype, bsz, n, d, _lib.ptr(ld), _lib.ptr(ls), _lib.ptr(sigma), _lib.ptr(g1), _lib.ptr(g2),
                      _lib.ptr(gl), _lib.ptr(gw), _lib.ptr(ws), wsb, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [x for x in (gd, gs, gl, gw) if x is not None]


@pytest.mark.parametrize("with_ws", [True, False])
@pytest.mark.parametrize("with_sub", [True, False])
@pytest.mark.parametrize("n,d", [(1, 10), (31, 15), (33, 12), (77, 16), (2, 17), (33, 20), (31, 31), (77, 31), (33, 32), (1, 32)])
def test_tile_adjoints_write_every_promised_element(n, d, with_sub, with_ws):
    """Every element of ``g_diag`` / ``g_sub`` / ``g_ldiag`` / ``g_lsub`` is written (the Python layer hands ``torch.empty``
    buffers over and returns them as the gradients), the strict upper triangle of ``g_ldiag`` with zeros."""
    ld, ls, g1, g2 = _dev_case(24, (3,), n, d, True, with_sub)
    outs = _abi_adjoints(ld, ls, g1, g2, with_ws)
    for x in outs:
        assert bool(torch.isfinite(x).all()), "an element was left unwritten"
    gl = outs[2 if ls is not None else 1]
    assert float(torch.triu(gl, 1).abs().max()) == 0.0
    gd = outs[0]
    assert float((gd - gd.transpose(-1, -2)).abs().max()) <= 1e-13 * float(gd.abs().max())


@pytest.mark.parametrize("which", ["both", "diag", "sub"])
@pytest.mark.parametrize("batch,n,d", [((1,), 32, 10), ((3,), 77, 12), ((2,), 130, 15), ((3,), 33, 16), ((1,), 130, 16), ((3,), 32, 17),
                                       ((2,), 77, 20), ((1,), 130, 24), ((3,), 33, 31), ((2,), 77, 32), ((70,), 33, 32)])
def test_tile_adjoints_scan_form_against_sequential_form(batch, n, d, which):
    """The two implementations of each recurrence: with the full workspace (n >= 32: local terms + congruence scan, parallel in
    time) and with ``ws = NULL`` (``adj_carve`` declines: one wavefront per series walks the chain).  Same inputs, fp64 tolerance
    of the loop comparisons."""
    ld, ls, g1, g2 = _dev_case(25, batch, n, d, True)
    g1, g2 = (g1 if which != "sub" else None), (g2 if which != "diag" else None)
    par = _abi_adjoints(ld, ls, g1, g2, True)
    seq = _abi_adjoints(ld, ls, g1, g2, False)
    scale_c, scale_i = float(seq[0].abs().max()), float(seq[2].abs().max())
    for x, y, scale in zip(par, seq, (scale_c, scale_c, scale_i, scale_i)):
        assert float((x - y).abs().max()) <= 1e-9 * max(float(y.abs().max()), scale)
