"""
Reference of the spatio-temporal sparse CVI site update - TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Independent of markovflow_amd/models/spatio_temporal.py and csrc/mf_st.hip.  ``st_cvi_site_update`` states one step of
markovflow/models/spatio_temporal_variational.py:509-552 literally, for one series in numpy, in any numpy float type: the marginals
of every point (``st_closed_forms.st_expectations``), the gradients of its variational expectation in ``[mu, var + mu^2]``, the DENSE
projection ``P [N, 1, n]``, ``back_project_nats``, the partition of the points by their ``searchsorted`` index, the sum over each
part and the blend - with the magnitude ``sum |terms|`` of every output.  As in ``st_expectations`` the likelihood's own expectations
are float64 numbers at most: with ``dtype = numpy.longdouble`` everything around them runs in long double.

A likelihood is the ``(name, params)`` tuple of likelihood_closed_forms.py.
"""
import numpy as np

from helpers import likelihood_closed_forms as L
from helpers import st_closed_forms as ST


def dense_projection(a, wt):
    """``P A`` of the reference, ``[N, 1, n]``: row ``k`` is ``W_k[half D + s d_t + i] = a[k, s] wt[k, half d_t + i]``."""
    return ST.kron_rows(a, wt)[:, None, :]


def back_project_nats(g1, g2, proj):
    """``[theta_1 C, theta_2 C^T C]`` per point (variational_cvi.py:423-445): ``g1``, ``g2`` ``[N, 1]``, ``proj [N, 1, n]``."""
    return np.sum(proj * g1[:, :, None], axis=1), np.sum(g2[:, :, None, None] * proj[:, :, :, None] * proj[:, :, None, :], axis=1)


def st_cvi_site_sums(lik, a, wt, c, y, offsets, pair_mean, pair_cov, nq=20, dtype=np.float64):
    """One series, everything of the step that does not depend on the old sites.  Inputs as ``st_closed_forms.st_expectations``.
    Returns a dict with ``theta1 [S, n]``, ``theta2 [S, n, n]``, ``ve_sum [S]``, ``fmu``, ``fvar`` ``[N]`` in ``dtype`` and
    ``mag_<name>`` (float64) for each."""
    ty = dtype
    base = ST.st_expectations(lik, a, wt, c, y, offsets, pair_mean, pair_cov, nq, ty)
    fmu, fvar = base["fmu"], base["fvar"]
    a, wt, y = (np.asarray(v, dtype=ty) for v in (a, wt, y))
    npts, segs = a.shape[0], len(offsets) - 1
    pair = a.shape[1] * wt.shape[1]
    if npts:
        args = (fmu, fvar, y) if ty != np.longdouble else tuple(x.astype(np.float64) for x in (fmu, fvar, y))
        (ve, gm, gv), mags = L.expectations(lik, *args, nq, dtype=ty if ty != np.longdouble else np.float64)
        ve, gm, gv = (x.astype(ty) for x in (ve, gm, gv))
    else:
        ve = gm = gv = np.zeros(0, dtype=ty)
        mags = (np.zeros(0),) * 3
    # gradient_transformation_mean_var_to_expectation
    g1, g2 = gm - ty(2) * gv * fmu, gv
    mag_g1 = mags[1] + 2.0 * mags[2] * base["mag_fmu"]
    proj = dense_projection(a, wt)
    absw = np.abs(proj[:, 0, :].astype(np.float64))
    # the reference's tf.searchsorted(inducing_time, t) of a point is the number of its segment
    index = np.searchsorted(np.asarray(offsets)[1:], np.arange(npts), side="right")
    out = dict(fmu=fmu, fvar=fvar, mag_fmu=base["mag_fmu"], mag_fvar=base["mag_fvar"], theta1=np.zeros((segs, pair), dtype=ty),
               theta2=np.zeros((segs, pair, pair), dtype=ty), ve_sum=np.zeros(segs, dtype=ty), mag_theta1=np.zeros((segs, pair)),
               mag_theta2=np.zeros((segs, pair, pair)), mag_ve_sum=np.zeros(segs))
    for s in range(segs):
        part = index == s
        theta1, theta2 = back_project_nats(g1[part, None], g2[part, None], proj[part])            # [Ns, n], [Ns, n, n]
        out["theta1"][s], out["theta2"][s] = np.sum(theta1, axis=0, dtype=ty), np.sum(theta2, axis=0, dtype=ty)
        out["ve_sum"][s] = np.sum(ve[part], dtype=ty)
        out["mag_theta1"][s] = np.einsum("k,ki->i", mag_g1[part], absw[part])
        out["mag_theta2"][s] = np.einsum("k,ki,kj->ij", mags[2][part], absw[part], absw[part])
        out["mag_ve_sum"][s] = np.sum(mags[0][part])
    return out


def blend(sums, lr, nat1, nat2, dtype=np.float64):
    """``nat <- (1 - lr) nat + lr sum`` on the sums of ``st_cvi_site_sums``: ``nat1``, ``nat2`` and their magnitudes."""
    ty = dtype
    nat1, nat2 = np.asarray(nat1, dtype=ty), np.asarray(nat2, dtype=ty)
    one_minus = ty(1) - ty(lr)
    keep, step = abs(float(one_minus)), abs(float(lr))
    return dict(nat1=one_minus * nat1 + ty(lr) * sums["theta1"], nat2=one_minus * nat2 + ty(lr) * sums["theta2"],
                mag_nat1=keep * np.abs(nat1.astype(np.float64)) + step * sums["mag_theta1"],
                mag_nat2=keep * np.abs(nat2.astype(np.float64)) + step * sums["mag_theta2"])


def st_cvi_site_update(lik, a, wt, c, y, offsets, pair_mean, pair_cov, lr, nat1, nat2, nq=20, dtype=np.float64):
    """One series, one step from the old sites ``nat1 [S, n]``, ``nat2 [S, n, n]`` (not written).  Returns a dict with ``nat1``,
    ``nat2``, ``ve_sum``, ``fmu``, ``fvar`` in ``dtype`` and ``mag_<name>`` (float64)."""
    sums = st_cvi_site_sums(lik, a, wt, c, y, offsets, pair_mean, pair_cov, nq, dtype)
    return {**{k: v for k, v in sums.items() if "theta" not in k}, **blend(sums, lr, nat1, nat2, dtype)}
