"""
float32 of ``StateSpaceModel.kl_divergence`` and ``StateSpaceModel.marginals``, value and gradient, on every live route - the
float32 instantiations of the kernels tests/test_gpu_gradients.py pins in float64 (mf_ssm_kl_divergence_f32, mf_ssm_kl_grad_f32,
mf_kf_loglik_grad_f32 with H = NULL, mf_ssm_marginals_f32, mf_ssm_marginals_grad_f32; csrc/mf_kl_grad.hpp, the row forms and
wave_kl_walk_kernel).  Through the public API on float32 tensors made from float32-rounded draws; every case asserts the route that
ran.  Judged as tests/helpers/kl_fp32_cases.py states: against the closed form in float64 on the inputs the kernel saw, within
FP32_FACTOR x the error of the same closed form in float32 (tests/helpers/kl_fp32_table.py).  Then, in both dtypes and without a
tolerance: the strict upper triangles of the factors' gradients are exactly zero, the raw entry points write every element of
their outputs, and a NULL incoming gradient of mf_ssm_marginals_grad is a zero one.

What would be caught (worked once on paper): an adjoint sweep that drops the (N_k, n_k) of the LAST block with inputs leaves
lam_{T-2}, M_{T-2} without transition T-2's own term: g(q1.a_s), g(q1.b_s) of that transition are off by O(1) of their size at
every shape of the first three routes, (1, 2, 2) included where that block is the only one; the marginals' adjoint with its
incoming gradient of the last time point dropped fails test_marginals_fp32 the same way (g.a_s, g.b_s, g.chol_q).
"""
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from helpers import kl_closed_forms as KC
from helpers import kl_fp32_cases as C
from helpers import kl_fp32_table as TABLE
from helpers.kl_fp32_cases import abi_calls  # noqa: F401  (fixture)
from test_gpu_kalman import DEV, tt

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
KL_PARAMS = [(route,) + shape for route, shapes in C.KL_CASES.items() for shape in shapes]


def ran(calls, dtype=F32):
    return C.ran(calls, dtype)


def leaves(kw, dtype, requires_grad):
    return [tt(kw[k], dtype).requires_grad_(requires_grad) for k in KC.CHAIN]


def report(what, errs, yard):
    """Print every figure, then assert: measured error <= FP32_FACTOR x the closed form's in float32."""
    worst = max(errs[name] / yard[name] for name in errs)
    for name, e in errs.items():
        print(f"  fp32 {what} {name}: error {e:.3g} (closed form in float32 {yard[name]:.3g}, ratio {e / yard[name]:.2f})")
    print(f"  fp32 {what}: worst ratio {worst:.2f}")
    for name, e in errs.items():
        assert e <= C.FP32_FACTOR * yard[name], (what, name, e, yard[name])


def assert_forward_route(route, d, t, bsz, names):
    small = _lib.small_state_dim(d, bsz, t, 4)
    ws_bytes = int(_lib.load().mf_ssm_kl_workspace_bytes(bsz, t, d, 4))
    if route == "sweep":                   # one lane per series
        assert small and d <= 9 and ws_bytes == 0 and names == ["mf_ssm_kl_divergence"]
    elif route == "scan":                  # q1's marginals by the scans in time, a lane per (series, step)
        assert small and d <= 9 and ws_bytes > 0 and names == ["mf_ssm_kl_divergence"]
    elif route == "row":
        assert small and 10 <= d <= 15 and ws_bytes > 0 and names == ["mf_ssm_kl_divergence"]
    elif route == "walk":                  # one walk per (series, chunk): no moments, no precision, not the from-moments kernel
        assert not small and 16 <= d <= 32 and ws_bytes > 0 and names == ["mf_ssm_kl_divergence"]
    else:                                  # the composition over the operator kernels: HIP calls only, none of the fused ones
        assert route == "operators" and not small and d > 32 and ws_bytes == 0
        assert "mf_ssm_precision" in names and "mf_ssm_kl_divergence" not in names and "mf_ssm_kl_from_moments" not in names


@pytest.mark.parametrize("route,d,t,bsz", KL_PARAMS)
def test_kl_divergence_fp32(abi_calls, route, d, t, bsz):
    kw1, kw2, weights, want, want_grads, want_same = C.kl_reference(route, d, t, bsz)
    yard = TABLE.KL[(route, d, t, bsz)]
    with_grads = route in C.ADJOINT_ROUTES
    g1, g2 = leaves(kw1, F32, with_grads), leaves(kw2, F32, with_grads)
    kl = mfa.StateSpaceModel(*g1).kl_divergence(mfa.StateSpaceModel(*g2))
    assert kl.dtype == F32 and tuple(kl.shape) == (bsz,)
    assert_forward_route(route, d, t, bsz, ran(abi_calls))
    errs = {"kl": KC.value_error(kl.detach(), want, t, d)}
    if with_grads:
        del abi_calls[:]
        torch.sum(kl * tt(weights, F32)).backward()
        # the adjoint sweep of q1 and the local kernel of q2 (H = NULL) - not the re-evaluation in torch
        assert {"mf_ssm_kl_grad", "mf_kf_loglik_grad"} <= set(ran(abi_calls))
        for name, leaf, w in zip(C.GRAD_NAMES, g1 + g2, want_grads):
            assert leaf.grad.dtype == F32
            errs[name] = KC.tensor_error(leaf.grad, w)
            if name.endswith(("chol_p0", "chol_q")):
                assert float(torch.triu(leaf.grad, diagonal=1).abs().max()) == 0.0, name
    with torch.no_grad():
        del abi_calls[:]
        same = mfa.StateSpaceModel(*(x.detach() for x in g1)).kl_divergence(mfa.StateSpaceModel(*(x.detach().clone() for x in g1)))
        assert_forward_route(route, d, t, bsz, ran(abi_calls))
    errs["kl_same"] = KC.value_error(same, want_same, t, d)
    report(f"kl {route} d={d} T={t} B={bsz}", errs, yard)


@pytest.mark.parametrize("d,t,bsz", C.MARGINALS_CASES)
def test_marginals_fp32(abi_calls, d, t, bsz):
    kw, w_means, w_covs, want = C.marginals_reference(d, t, bsz)
    assert _lib.small_state_dim(d, bsz, t, 4)
    assert (int(_lib.load().mf_ssm_marginals_workspace_bytes(bsz, t, d, 4)) > 0) == C.marginals_scans(t)
    g = leaves(kw, F32, True)
    means, covs = mfa.StateSpaceModel(*g).marginals
    forward = ran(abi_calls)
    assert forward == ["mf_ssm_marginals"] or forward == ["mf_ssm_marginal_means", "mf_ssm_marginal_covariances"]
    del abi_calls[:]
    (torch.sum(means * tt(w_means, F32)) + torch.sum(covs * tt(w_covs, F32))).backward()
    assert ran(abi_calls) == ["mf_ssm_marginals_grad"]
    got = [means.detach(), covs.detach()] + [x.grad for x in g]
    assert all(x.dtype == F32 for x in got)
    assert float(torch.triu(g[1].grad, diagonal=1).abs().max()) == 0.0 and float(torch.triu(g[4].grad, diagonal=1).abs().max()) == 0.0
    errs = {name: KC.tensor_error(x, w) for name, x, w in zip(C.MARGINALS_NAMES, got, want)}
    report(f"marginals d={d} T={t} B={bsz}", errs, TABLE.MARGINALS[(d, t, bsz)])


@pytest.mark.parametrize("d,t,bsz", [(3, 40, 2), (8, 90, 1), (12, 80, 2)])
def test_gradient_triangles_are_exactly_zero_fp64(d, t, bsz):
    """(float32: asserted by the two tests above on every shape.)"""
    kw1, kw2, weights = C.draw_kl(C.DEFAULT_SEED, d, t, bsz)
    g1, g2 = leaves(kw1, F64, True), leaves(kw2, F64, True)
    torch.sum(mfa.StateSpaceModel(*g1).kl_divergence(mfa.StateSpaceModel(*g2)) * tt(weights)).backward()
    g3 = leaves(kw1, F64, True)
    means, covs = mfa.StateSpaceModel(*g3).marginals
    (means.sum() + torch.sum(covs * torch.randn_like(covs))).backward()
    for chain in (g1, g2, g3):
        for i in (1, 4):
            assert float(torch.triu(chain[i].grad, diagonal=1).abs().max()) == 0.0
            assert float(torch.tril(chain[i].grad).abs().max()) > 0.0


# ---- the raw entry points -------------------------------------------------------------------------------------------------------
RAW_SHAPES = [(3, 9, 3), (3, 70, 2), (8, 9, 3), (8, 70, 2), (12, 9, 2), (12, 80, 2)]       # (d, T, B): both sides of the scans in time


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def gradient_buffers(bsz, t, d, dtype):
    return [nan_like((bsz, d), dtype), nan_like((bsz, d, d), dtype), nan_like((bsz, t - 1, d, d), dtype), nan_like((bsz, t - 1, d), dtype),
            nan_like((bsz, t - 1, d, d), dtype)]


def adjoint_workspace(bsz, t, d, dtype):
    ws_bytes = int(_lib.load().mf_ssm_adjoint_workspace_bytes(bsz, t, d, 4 if dtype == F32 else 8))
    assert ws_bytes > 0
    return torch.empty(ws_bytes, dtype=torch.uint8, device=DEV), ws_bytes


def assert_all_written(outputs):
    for i, x in enumerate(outputs):
        assert bool(torch.isfinite(x).all()), i
        if x.dim() >= 3 and i in (1, 4):
            assert float(torch.triu(x, diagonal=1).abs().max()) == 0.0, i


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("d,t,bsz", RAW_SHAPES)
def test_raw_kl_value_and_gradients_write_every_element(dtype, d, t, bsz):
    """mf_ssm_kl_divergence with every by-product asked for, mf_ssm_kl_grad (the inputs of its recursion from the forward, and at
    d <= 9 also formed by itself: adj_N = adj_n = NULL) and mf_kf_loglik_grad with H = NULL, all into buffers full of NaN; float64
    also against the closed form."""
    esz = 4 if dtype == F32 else 8
    lib, dev = _lib.load(), torch.device(DEV)
    kl_ws_bytes = int(lib.mf_ssm_kl_workspace_bytes(bsz, t, d, esz))
    assert (kl_ws_bytes > 0) == (t >= 64 or d >= 10)                   # sweep per series | scans in time / row form
    kw1, kw2, weights = C.draw_kl(C.DEFAULT_SEED, d, t, bsz)
    q1, q2 = leaves(kw1, dtype, False), leaves(kw2, dtype, False)
    w = tt(weights, dtype)
    info = _lib.new_info(dev)
    p = _lib.ptr
    out = nan_like((bsz,), dtype)
    means, covs, cross = nan_like((bsz, t, d), dtype), nan_like((bsz, t, d, d), dtype), nan_like((bsz, t - 1, d, d), dtype)
    adj_n_mat, adj_n_vec = nan_like((bsz, t, d, d), dtype), nan_like((bsz, t, d), dtype)
    kl_ws = _lib.workspace(kl_ws_bytes, dev)
    _lib.call("mf_ssm_kl_divergence", dtype, bsz, t, d, *[p(x) for x in q1], *[p(x) for x in q2], p(out), p(means), p(covs), p(cross),
              p(adj_n_mat), p(adj_n_vec), p(kl_ws), kl_ws_bytes, p(info), _lib.stream_ptr(dev))
    for x in (out, means, covs, cross, adj_n_mat, adj_n_vec):
        assert bool(torch.isfinite(x).all())
    want_m, want_c, want_x = C.numpy_moments(kw1)
    for got, wv in ((means, want_m), (covs, want_c), (cross, want_x)):
        assert KC.tensor_error(got, wv) < (1e-12 if dtype == F64 else 2e-6)      # (sanity: these feed the calls below)
    results = []
    for given in ((adj_n_mat, adj_n_vec), (None, None)):
        if given[0] is None and d > 9:
            continue               # 10 <= d <= 15 is compiled in row form only: the inputs of the recursion come from the forward
        ws, ws_bytes = adjoint_workspace(bsz, t, d, dtype)
        out1 = gradient_buffers(bsz, t, d, dtype)
        _lib.call("mf_ssm_kl_grad", dtype, bsz, t, d, *[p(x) for x in q1], *[p(x) for x in q2], p(means), p(covs), p(w), p(given[0]),
                  p(given[1]), *[p(x) for x in out1], p(ws), ws_bytes, p(info), _lib.stream_ptr(dev))
        assert_all_written(out1)
        results.append(out1)
    out2 = gradient_buffers(bsz, t, d, dtype)
    neg_w = (-w).contiguous()
    _lib.call("mf_kf_loglik_grad", dtype, bsz, t, d, 1, *[p(x) for x in q2], None, None, None, 0, p(means), p(covs), p(cross),
              *[p(x) for x in out2], None, None, None, p(neg_w), p(info), _lib.stream_ptr(dev))
    assert int(info.item()) == 0
    assert_all_written(out2)
    if dtype == F64:
        value, want = C.kl_closed_form(lambda a, b: KC.kl_local(a, b), kw1, kw2, weights, F64, True)
        assert KC.value_error(out, value, t, d) < 1e-12
        for out1 in results:
            for name, got, wv in zip(C.GRAD_NAMES, out1 + out2, want):
                assert KC.tensor_error(got, wv) < 1e-9, name


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("d,t,bsz", C.MARGINALS_NULL_CASES)
def test_raw_marginals_gradient_null_inputs(dtype, d, t, bsz):
    """mf_ssm_marginals_grad: "either of g_means / g_covs may be NULL = zero" (autograd always hands zeros over, so only the raw
    call reaches those branches).  Each equals the call with an explicit zero tensor bit for bit, writes every element, and is the
    gradient of the functional without that part."""
    kw, w_means, w_covs, _ = C.marginals_reference(d, t, bsz)
    means, covs, _ = (tt(x, dtype) for x in C.numpy_moments(kw))
    cp0, a_s, cq = (tt(kw[k], dtype) for k in ("chol_p0", "a_s", "chol_q"))
    gm, gs = tt(w_means, dtype), tt(w_covs, dtype)
    p = _lib.ptr

    def grad(g_means, g_covs):
        ws, ws_bytes = adjoint_workspace(bsz, t, d, dtype)
        out = gradient_buffers(bsz, t, d, dtype)
        _lib.call("mf_ssm_marginals_grad", dtype, bsz, t, d, p(cp0), p(a_s), p(cq), p(means), p(covs), p(g_means), p(g_covs),
                  *[p(x) for x in out], p(ws), ws_bytes, _lib.stream_ptr(torch.device(DEV)))
        assert_all_written(out)
        return out

    for absent, g_means, g_covs in (("g_means", None, gs), ("g_covs", gm, None)):
        got = grad(g_means, g_covs)
        explicit = grad(torch.zeros_like(gm) if g_means is None else g_means, torch.zeros_like(gs) if g_covs is None else g_covs)
        for a, b in zip(got, explicit):
            assert torch.equal(a, b), absent
        want = C.marginals_closed_form(kw, None if g_means is None else w_means, None if g_covs is None else w_covs, F64, False)[2:]
        errs = {name: KC.tensor_error(x, w) for name, x, w in zip(C.MARGINALS_NAMES[2:], got, want)}
        if dtype == F64:
            assert max(errs.values()) < 1e-9, errs
        else:
            report(f"marginals_grad {absent}=NULL d={d} T={t} B={bsz}", errs, TABLE.MARGINALS_NULL[(d, t, bsz)][absent])
