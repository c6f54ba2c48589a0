"""
GPU parity tests of markovflow_amd/conditionals.py - the function surface of /root/reference/markovflow/conditionals.py
(conditional_predict :29-83, conditional_statistics :87-120, base_conditional_predict :380-421, pairwise_marginals :424-485):

* ``conditional_statistics`` (``mf_sde_conditional_statistics_*``: one lane per new point) against direct Gaussian conditioning on
  the kernel's dense covariance of the triple (x_-, x_t, x_+);
* ``pairwise_marginals -> conditional_predict`` against the dense GP predictive distribution and against the fused route
  ``ConditionalProcess.predict_state`` (``mf_sde_conditional_predict_*``) - the two compositions the reference has
  (posterior.py:207-229 calls exactly these functions);
* shapes and the conditional (no covariances) form.
fp64; tolerances as tests/test_gpu_kernels.py::test_posterior_predict_f_vs_dense_gp.

The strict comparisons (the second half of the file) are those against tests/helpers/conditional_closed_forms.py, in the scheme of
tests/test_gpu_conditional_kernels.py, ``|err| <= 64 eps (magnitude + 1)``:
* ``conditional_statistics`` on Matern kernels of d = 1, 2, 3, 6, 6, 9 with new points inside the gaps, beyond both ends and ON training
  points, the helper fed the kernel's own ``transition_statistics`` - a ``_lib.call`` spy sees ``mf_sde_conditional_statistics`` once;
  measured maxima on an MI355X: D 2.02, E 2.61, T 1.14;
* the torch routes of ``_conditional_statistics_from_transitions`` (broadcast inputs, ``return_precision``, an input under a tape): no
  kernel call, the same bound (measured: at most 1.30);
* ``predict_state`` with ``batch_shape`` () and (2, 3): one ``mf_sde_conditional_predict`` call, equal to the composed route;
* float32 through ``GaussianProcessRegression``: the fused and the composed float32 routes against the float64 ``predict_state`` of the same
  float32-rounded data, errors normalised by the largest posterior standard deviation (squared for covariances): the fused route's is
  at most 4 x the composed route's + 8 eps32.  Measured (mean / covariance): Matern32 fused 5.2e-7 / 1.6e-7 against composed 3.8e-7 / 1.6e-7; Sum(Matern52, Matern12) fused 4.3e-7 / 2.5e-7
  against composed 3.9e-7 / 2.5e-7.
"""
import numpy as np
import pytest
import torch

import markovflow_amd as mfa
from markovflow_amd import _lib
from markovflow_amd import conditionals as C
from oracle import numpy_kernels as K
from helpers import conditional_closed_forms as CC
from test_gpu_kalman import DEV, nn, tt

pytestmark = pytest.mark.gpu
CLS = {1: mfa.Matern12, 3: mfa.Matern32, 5: mfa.Matern52}


def _kernel(sig, ls, var):
    parts = [CLS[o](l, v, device=DEV) for o, l, v in zip(sig, ls, var)]
    return parts[0] if len(parts) == 1 else mfa.Sum(parts, jitter=1e-10)


@pytest.mark.parametrize("sig", [(3,), (5,), (5, 5), (1, 3, 5)])
def test_conditional_statistics_against_direct_gaussian_conditioning(rng, sig):
    """p(x_t | x_-, x_+) = N(P [x_-, x_+], T): from the stationary joint covariance of the three states, built from the kernel's own
    transitions, K = [[P, P A1^T, P A1^T A2^T], [., P, P A2^T], [., ., P]] (stationary: Cov(x_s, x_u) = A(u - s) P for u > s)."""
    bsz, n = 2, 20
    ls, var = [0.6 + 0.5 * j for j in range(len(sig))], [1.0 + 0.3 * j for j in range(len(sig))]
    kern = _kernel(sig, ls, var)
    d = kern.state_dim
    t = np.cumsum(0.2 + rng.exponential(0.3, size=(bsz, n)), axis=-1)
    gaps = np.diff(t, axis=-1)
    t_new = t[:, :-1] + gaps * (0.5 + 0.3 * (rng.random((bsz, n - 1)) - 0.5))        # one new point inside every gap
    n_new = n - 1
    proj, cov = C.conditional_statistics(tt(t_new), tt(t), kern)
    assert tuple(proj.shape) == (bsz, n_new, d, 2 * d) and tuple(cov.shape) == (bsz, n_new, d, d)
    minus, plus = t[:, :-1], t[:, 1:]
    a1, _ = kern.transition_statistics(tt(minus), tt(t_new - minus))
    a2, _ = kern.transition_statistics(tt(t_new), tt(plus - t_new))
    ps = nn(kern.steady_state_covariance).reshape(d, d)
    a1, a2 = nn(a1), nn(a2)
    for s in range(bsz):
        for i in range(n_new):
            k_mt = ps @ a1[s, i].T                      # Cov(x_-, x_t)
            k_tp = ps @ a2[s, i].T                      # Cov(x_t, x_+)
            k_mp = ps @ a1[s, i].T @ a2[s, i].T         # Cov(x_-, x_+)
            k_ends = np.block([[ps, k_mp], [k_mp.T, ps]])
            k_t_ends = np.hstack([k_mt.T, k_tp])
            want_p = k_t_ends @ np.linalg.inv(k_ends)
            want_t = ps - want_p @ k_t_ends.T
            # (the dense reference inverts the 2d x 2d covariance of the two ends, ill-conditioned for Matern-5/2 states)
            np.testing.assert_allclose(nn(proj)[s, i], want_p, rtol=2e-3, atol=2e-5)
            np.testing.assert_allclose(nn(cov)[s, i], want_t, rtol=2e-3, atol=1e-6)


@pytest.mark.parametrize("sig", [(3,), (5, 5), (1, 5)])
def test_pairwise_marginals_then_conditional_predict_against_the_dense_gp_and_the_fused_route(rng, sig):
    bsz, n, noise = 2, 50, 0.05
    ls, var = [0.6 + 0.5 * j for j in range(len(sig))], [1.0 + 0.3 * j for j in range(len(sig))]
    kern = _kernel(sig, ls, var)
    d = kern.state_dim
    t = np.cumsum(0.05 + rng.exponential(0.15, size=(bsz, n)), axis=-1)
    y = rng.normal(size=(bsz, n, 1))
    t_new = np.sort(np.concatenate([t[:, :1] - rng.random((bsz, 4)) * 2.0, t[:, -1:] + rng.random((bsz, 4)) * 2.0, t[:, 3:6],
                                    t[:, :1] + rng.random((bsz, 25)) * (t[:, -1:] - t[:, :1])], axis=-1), axis=-1)
    gpr = mfa.GaussianProcessRegression((tt(t), tt(y)), kern, chol_obs_covariance=tt(np.sqrt(noise) * np.eye(1)))
    post = gpr.posterior
    dist = post.gauss_markov_model
    m0 = kern.initial_mean((bsz,))
    p0 = kern.initial_covariance(tt(t[..., :1]))
    pair_mean, pair_cov = C.pairwise_marginals(dist, m0, p0)
    assert tuple(pair_mean.shape) == (bsz, n + 1, 2 * d) and tuple(pair_cov.shape) == (bsz, n + 1, 2 * d, 2 * d)
    np.testing.assert_allclose(nn(pair_cov), np.swapaxes(nn(pair_cov), -1, -2), atol=1e-12)
    mean, cov = C.conditional_predict(tt(t_new), tt(t), kern, pair_mean, pair_cov)
    fused_mean, fused_cov = post.predict_state(tt(t_new))
    np.testing.assert_allclose(nn(mean), nn(fused_mean), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(nn(cov), nn(fused_cov), rtol=1e-8, atol=1e-10)
    f_mean, f_var = kern.generate_emission_model(tt(t_new)).project_state_marginals_to_f(mean, cov)
    for s in range(bsz):
        want_mean, want_var = K.dense_gp_predict(sig, ls, var, t[s], y[s, :, 0], noise, t_new[s])
        np.testing.assert_allclose(nn(f_mean)[s, :, 0], want_mean, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(nn(f_var)[s, :, 0], want_var, rtol=1e-5, atol=1e-7)
    # without the pairwise covariances: the conditional density given [x_-, x_+] = the pairwise means
    cmean, ccov = C.conditional_predict(tt(t_new), tt(t), kern, pair_mean)
    proj, t_cov = C.conditional_statistics(tt(t_new), tt(t), kern)
    np.testing.assert_allclose(nn(cmean), nn(mean), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(nn(ccov), nn(t_cov), rtol=0, atol=0)
    # base_conditional_predict on hand-made inputs (conditionals.py:380-421)
    states = torch.randn(bsz, t_new.shape[-1], 2 * d, dtype=torch.float64, device=DEV)
    bm, bc = C.base_conditional_predict(proj, t_cov, states)
    np.testing.assert_allclose(nn(bm), nn((proj @ states[..., None])[..., 0]), rtol=1e-12)
    np.testing.assert_allclose(nn(bc), nn(t_cov), rtol=0, atol=0)


def test_pairwise_marginals_carries_gradients_to_the_chain(rng):
    """under a tape ``pairwise_marginals`` is built from the differentiable moments (the reference forms it from
    ``dist.marginals`` / ``dist.covariance_blocks()`` under its tape, conditionals.py:449-450; its sparse / PEP models differentiate
    through it).  Gradient of a scalar of both outputs w.r.t. every parameter of the chain against the dense torch composition
    ``P_{k+1} = A_k P_k A_k^T + Q_k``, ``m_{k+1} = A_k m_k + b_k``, ``Cov(x_{k+1}, x_k) = A_k P_k``; fp64, rtol 1e-8."""
    bsz, n, d = 2, 7, 3
    g = torch.Generator(device=DEV); g.manual_seed(11)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device=DEV, generator=g)                    # noqa: E731
    eye = torch.eye(d, dtype=torch.float64, device=DEV)
    leaves = [rnd(bsz, d), torch.tril(0.3 * rnd(bsz, d, d)) + eye, 0.5 * rnd(bsz, n - 1, d, d), 0.3 * rnd(bsz, n - 1, d),
              torch.tril(0.3 * rnd(bsz, n - 1, d, d)) + eye]
    m0, p0 = rnd(bsz, d), eye.expand(bsz, d, d) * 2.0
    wm, wc = rnd(bsz, n + 1, 2 * d), rnd(bsz, n + 1, 2 * d, 2 * d)

    def scalar(pm, pc):
        return torch.sum(pm * wm) + torch.sum(pc * wc)

    def ours(mu0, cp0, a, b, cq):
        return scalar(*C.pairwise_marginals(mfa.StateSpaceModel(mu0, cp0, a, b, cq), m0, p0))

    def dense(mu0, cp0, a, b, cq):
        means, covs, subs = [mu0], [cp0 @ cp0.transpose(-1, -2)], []
        for k in range(n - 1):
            subs.append(a[:, k] @ covs[-1])
            covs.append(a[:, k] @ covs[-1] @ a[:, k].transpose(-1, -2) + cq[:, k] @ cq[:, k].transpose(-1, -2))
            means.append((a[:, k] @ means[-1][..., None])[..., 0] + b[:, k])
        ext_m = torch.stack([m0] + means + [m0], dim=1)
        ext_c = torch.stack([p0] + covs + [p0], dim=1)
        zero = torch.zeros_like(p0)
        ext_s = torch.stack([zero] + subs + [zero], dim=1)
        pm = torch.cat([ext_m[:, :-1], ext_m[:, 1:]], dim=-1)
        pc = torch.cat([torch.cat([ext_c[:, :-1], ext_s.transpose(-1, -2)], dim=-1), torch.cat([ext_s, ext_c[:, 1:]], dim=-1)], dim=-2)
        return scalar(pm, pc)

    a_leaves = [t.clone().requires_grad_(True) for t in leaves]
    b_leaves = [t.clone().requires_grad_(True) for t in leaves]
    va, vb = ours(*a_leaves), dense(*b_leaves)
    assert float(va.detach()) == pytest.approx(float(vb.detach()), rel=1e-10)
    ga, gb = torch.autograd.grad(va, a_leaves), torch.autograd.grad(vb, b_leaves)
    for x, y, name in zip(ga, gb, ("mu0", "cholP0", "A", "b", "cholQ")):
        if name.startswith("chol"):
            x, y = torch.tril(x), torch.tril(y)
        np.testing.assert_allclose(nn(x), nn(y), rtol=1e-8, atol=1e-10, err_msg=name)


# ---- against tests/helpers/conditional_closed_forms.py ----------------------------------------------------------------------------
EPS, EPS32, K_F64 = 2.0 ** -52, 2.0 ** -23, 64.0


def count_calls(monkeypatch):
    seen = []
    real = _lib.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    return seen


def within_bound(what, got, want, mag):
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    scaled = np.abs(got - want) / (np.asarray(mag) + 1.0)
    ratio = float(scaled.max() / EPS)
    print(f"RATIO f64 {what}: {ratio:.2f}")
    assert ratio <= K_F64, f"{what}: {ratio:.1f} eps (magnitude + 1) at {np.unravel_index(int(scaled.argmax()), scaled.shape)}"


@pytest.mark.parametrize("sig", [(1,), (3,), (5,), (5, 5), (1, 3, 5), (5, 5, 5)], ids=lambda s: "m" + "".join(map(str, s)))
def test_conditional_statistics_on_matern_kernels_against_the_closed_forms(rng, monkeypatch, sig):
    """d = 1, 2, 3, 6, 6, 9.  Training gaps 0.6 + Exp(0.3) and the interior new points in the central 0.5 +- 0.15 of their gap: no
    new point is closer than 0.21 to a neighbour (the float64 helper stays within 4.5 eps (magnitude + 1) of long double down to gaps
    of 0.05, tests/test_conditional_closed_forms_host.py).  Two new points before the first training point and two after the last
    (the neighbour is the stationary prior at -/+ APPROX_INF: A = 0, Q = Pinf), and two exactly ON training points (A_tp = I,
    Q_tp = jitter I)."""
    bsz, n = 2, 20
    ls, var = [0.6 + 0.5 * j for j in range(len(sig))], [1.0 + 0.3 * j for j in range(len(sig))]
    kern = _kernel(sig, ls, var)
    d = kern.state_dim
    t = np.cumsum(0.6 + rng.exponential(0.3, size=(bsz, n)), axis=-1)
    inside = t[:, :-1] + np.diff(t, axis=-1) * (0.5 + 0.3 * (rng.random((bsz, n - 1)) - 0.5))
    t_new = np.sort(np.concatenate([t[:, :1] - 1.5, t[:, :1] - 0.4, inside, t[:, [3, 10]], t[:, -1:] + 0.5, t[:, -1:] + 2.0], axis=-1), axis=-1)
    n_new = t_new.shape[-1]
    seen = count_calls(monkeypatch)
    proj, cov = C.conditional_statistics(tt(t_new), tt(t), kern)
    assert seen.count("mf_sde_conditional_statistics") == 1
    assert tuple(proj.shape) == (bsz, n_new, d, 2 * d) and tuple(cov.shape) == (bsz, n_new, d, d)
    # the kernel's own transitions around every new point, exactly as conditionals._conditional_statistics asks for them
    index = np.stack([np.searchsorted(t[s], t_new[s]) for s in range(bsz)])
    assert {0, 3, 10, n} <= set(index.ravel())
    aug = np.concatenate([np.full((bsz, 1), -C.APPROX_INF), t, np.full((bsz, 1), C.APPROX_INF)], axis=-1)
    minus, plus = np.take_along_axis(aug, index, -1), np.take_along_axis(aug, index + 1, -1)
    assert np.sum(plus == t_new) == 2 * bsz, "two new points per series sit exactly on a training point"
    a_mt, q_mt = kern.transition_statistics(tt(minus), tt(t_new - minus))
    a_tp, q_tp = kern.transition_statistics(tt(t_new), tt(plus - t_new))
    flat = lambda x: nn(x).reshape(-1, d, d)                                                         # noqa: E731
    (want_d, want_e, want_t), (mag_d, mag_e, mag_t) = CC.statistics(flat(a_mt), flat(q_mt), flat(a_tp), flat(q_tp))
    got = nn(proj).reshape(-1, d, 2 * d)
    within_bound(f"conditional_statistics {sig} D", got[..., :d], want_d, mag_d)
    within_bound(f"conditional_statistics {sig} E", got[..., d:], want_e, mag_e)
    within_bound(f"conditional_statistics {sig} T", nn(cov).reshape(-1, d, d), want_t, mag_t)


def test_conditional_statistics_torch_routes_run_no_kernel_and_agree_with_the_closed_forms(monkeypatch):
    """Broadcastable inputs of unequal shape, ``return_precision=True`` and an input that requires a gradient under a tape take the torch
    route of ``_conditional_statistics_from_transitions``."""
    n, d = 11, 3
    a_mt, q_mt, a_tp, q_tp = CC.draw_statistics_inputs(np.random.default_rng(5), n, d)
    (want_d, want_e, want_t), (mag_d, mag_e, mag_t) = CC.statistics(a_mt, q_mt, a_tp, q_tp)
    seen = count_calls(monkeypatch)
    fn = C._conditional_statistics_from_transitions

    def compare(tag, got, third=True):
        within_bound(f"torch route {tag} D", nn(got[0]), want_d, mag_d)
        within_bound(f"torch route {tag} E", nn(got[1]), want_e, mag_e)
        if third:
            within_bound(f"torch route {tag} T", nn(got[2]), want_t, mag_t)

    # an input under a tape
    leaf = tt(a_mt).requires_grad_(True)
    got = fn(leaf, tt(q_mt), tt(a_tp), tt(q_tp))
    assert got[0].requires_grad
    compare("tape", [g.detach() for g in got])
    # the precision T^-1 = Q_mt^-1 + A_tp^T Q_tp^-1 A_tp: the same expression with the helper's hand-written inverse, its magnitude
    got = fn(tt(a_mt), tt(q_mt), tt(a_tp), tt(q_tp), return_precision=True)
    compare("precision", got, third=False)
    inv_mt, inv_tp = CC.inverse_spd(q_mt), CC.inverse_spd(q_tp)
    tr = lambda x: np.swapaxes(x, -1, -2)                                                            # noqa: E731
    within_bound("torch route precision T^-1", nn(got[2]), inv_mt + tr(a_tp) @ inv_tp @ a_tp,
                 np.abs(inv_mt) + np.abs(tr(a_tp)) @ np.abs(inv_tp) @ np.abs(a_tp))
    # broadcast: ONE transition from the new point onwards for all of them
    b_tp, b_q = a_tp[:1], q_tp[:1]
    (want_d, want_e, want_t), (mag_d, mag_e, mag_t) = CC.statistics(a_mt, q_mt, np.broadcast_to(b_tp, a_mt.shape), np.broadcast_to(b_q, a_mt.shape))
    got = fn(tt(a_mt), tt(q_mt), tt(b_tp), tt(b_q))
    assert tuple(got[0].shape) == (n, d, d) and tuple(got[2].shape) == (n, d, d)
    compare("broadcast", got)
    assert "mf_sde_conditional_statistics" not in seen
    fn(tt(a_mt), tt(q_mt), tt(a_tp), tt(q_tp))                                                       # (the spy does see the kernel route)
    assert seen.count("mf_sde_conditional_statistics") == 1


def _random_chain(batch, n, d, seed):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device=DEV, generator=g)                    # noqa: E731
    eye = torch.eye(d, dtype=torch.float64, device=DEV)
    return [rnd(*batch, d), torch.tril(0.3 * rnd(*batch, d, d)) + eye, 0.5 * rnd(*batch, n - 1, d, d), 0.3 * rnd(*batch, n - 1, d),
            torch.tril(0.3 * rnd(*batch, n - 1, d, d)) + eye]


@pytest.mark.parametrize("n", [6, 1 + 1], ids=["N6", "N2"])
def test_predict_state_with_no_batch_axis_and_with_two(rng, monkeypatch, n):
    """``bsz = max(1, prod(batch_shape))``: a chain without a batch axis is one series, a (2, 3) batch six - with time points of their
    own per series, so that a series reading another one's data would show."""
    batch, n_new = (2, 3), 9
    kern = _kernel((3, 1), [0.7, 1.1], [1.0, 1.3])
    d = kern.state_dim
    params = _random_chain(batch, n, d, seed=17)
    t = np.cumsum(0.3 + rng.exponential(0.4, size=batch + (n,)), axis=-1)
    t_new = np.sort(np.concatenate([t[..., :1] - 0.7, t[..., -1:] + 0.9, t[..., :1] + rng.random(batch + (n_new - 2,)) * (t[..., -1:] - t[..., :1])],
                                   axis=-1), axis=-1)
    seen = count_calls(monkeypatch)

    def both_routes(pick):
        dist = mfa.StateSpaceModel(*[pick(p) for p in params])
        train, new = pick(tt(t)), pick(tt(t_new))
        assert tuple(dist.batch_shape) == tuple(train.shape[:-1])
        del seen[:]
        fused = mfa.ConditionalProcess(dist, kern, train).predict_state(new)
        assert seen.count("mf_sde_conditional_predict") == 1
        lead = tuple(train.shape[:-1])
        assert tuple(fused[0].shape) == lead + (n_new, d) and tuple(fused[1].shape) == lead + (n_new, d, d)
        m0, p0 = kern.initial_mean(lead), kern.initial_covariance(train[..., :1])
        composed = C.conditional_predict(new, train, kern, *C.pairwise_marginals(dist, m0, p0))
        for f, c in zip(fused, composed):
            np.testing.assert_allclose(nn(f), nn(c), rtol=1e-8, atol=1e-10)
        return fused

    whole = both_routes(lambda x: x)
    none = both_routes(lambda x: x[1, 2])
    one = both_routes(lambda x: x[1, 2][None])
    for a, b, w in zip(none, one, whole):
        assert torch.equal(a, b[0]), "no batch axis: the bits of the same series in a batch of one"
        # (the chain's moments of six series and of one may come from different sweeps: no bits, but the same series)
        np.testing.assert_allclose(nn(w[1, 2]), nn(a), rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("sig", [(3,), (5, 1)], ids=["m3", "m5+m1"])
def test_float32_prediction_through_the_public_api_against_float64(rng, sig):
    """GaussianProcessRegression in float32: the fused route (``predict_state``, ``mf_sde_conditional_predict_f32``) and the composed one
    (``pairwise_marginals -> conditional_predict``, ``mf_sde_conditional_statistics_f32``) share the float32 posterior chain; what the fused
    kernel adds to its error must not exceed 4 x what the composed route makes of it.  Points at least 0.3 of the shortest length scale
    apart (0.5; training gaps 0.45 + Exp(0.3), a new point in the central 0.5 +- 0.15 of every gap): below that the float32 process covariances lose their digits in either route."""
    bsz, n, noise = 2, 30, np.float32(0.05)
    ls, var = [0.5 + 0.75 * j for j in range(len(sig))], [1.0 + 0.5 * j for j in range(len(sig))]
    r32 = lambda a: np.asarray(a).astype(np.float32)                                                 # noqa: E731
    t = r32(np.cumsum(0.45 + rng.exponential(0.3, size=(bsz, n)), axis=-1))
    y = r32(rng.normal(size=(bsz, n, 1)))
    inside = t[:, :-1] + np.diff(t, axis=-1) * (0.5 + 0.3 * (rng.random((bsz, n - 1)) - 0.5))
    t_new = r32(np.sort(np.concatenate([t[:, :1] - 1.0, inside, t[:, -1:] + 1.0], axis=-1), axis=-1))
    chol_r = r32(np.sqrt(noise) * np.eye(1))
    assert np.diff(np.sort(np.concatenate([t, t_new], axis=-1), axis=-1), axis=-1).min() >= 0.3 * min(ls) * 0.999

    def model(dtype):
        parts = [CLS[o](l, v, device=DEV, dtype=dtype) for o, l, v in zip(sig, ls, var)]
        kern = parts[0] if len(parts) == 1 else mfa.Sum(parts, jitter=1e-6)
        return kern, mfa.GaussianProcessRegression((tt(t, dtype), tt(y, dtype)), kern, chol_obs_covariance=tt(chol_r, dtype))

    _, gpr64 = model(torch.float64)
    want = [nn(x) for x in gpr64.posterior.predict_state(tt(t_new))]
    kern, gpr = model(torch.float32)
    post = gpr.posterior
    new = tt(t_new, torch.float32)
    fused = post.predict_state(new)
    m0, p0 = kern.initial_mean((bsz,)), kern.initial_covariance(new[..., :1])
    composed = C.conditional_predict(new, tt(t, torch.float32), kern, *C.pairwise_marginals(post.gauss_markov_model, m0, p0))
    assert fused[0].dtype == torch.float32 and composed[1].dtype == torch.float32
    scale = float(np.sqrt(np.max(np.diagonal(want[1], axis1=-2, axis2=-1))))
    for name, f, c, w, s in zip(("mean", "covariance"), fused, composed, want, (scale, scale ** 2)):
        err_f = float(np.max(np.abs(nn(f).astype(np.float64) - w))) / s
        err_c = float(np.max(np.abs(nn(c).astype(np.float64) - w))) / s
        print(f"ERR f32 api {sig} {name}: fused {err_f:.3e}  composed {err_c:.3e}")
        assert np.isfinite(err_f) and err_f <= 4.0 * err_c + 8.0 * EPS32, f"{name}: fused {err_f:.3e} against composed {err_c:.3e}"
