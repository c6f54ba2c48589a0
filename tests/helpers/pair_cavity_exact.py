"""The pair cavity of sparse power EP at 50 digits (``mpmath``), by dense inverses as ``sparse_pep_closed_forms.pair_cavity`` states it:
``S^-1``, the cavity precision ``S^-1 + 2 beta sym(nat2)``, ITS inverse, the two ``G(m, S) = (log det S + m^T S^-1 m) / 2``.  Both matrices
are positive definite by construction (``draw``), so inverse and log-determinant go through the Cholesky factor: a sixth of the
multiplications of ``mpmath.inverse`` + ``mpmath.det``, which keeps 140 pairs of 18 x 18 within a second or two."""
import mpmath as mp
import numpy as np

KEYS = ("pair_mean", "pair_cov", "nat1", "nat2", "beta")
OUTPUTS = ("cav_mean", "cav_cov", "gamma")
BETAS = (0.0, 1.0, 1.0 / 3.0, 1.0 / 129.0)


def draw(bsz, segs, n, dtype=np.float64, seed=0):
    """Per pair ``P0 = Q diag(lam) Q^T`` (``lam`` uniform in [0.5, 4], ``Q`` from a QR), ``N = sum_k c_k v_k v_k^T`` (1 ... n terms,
    ``c_k`` in (0, 4], ``E |v_k|^2 = 1``), ``nat2 = -N / 2`` + an antisymmetric part, ``S = (P0 + N)^-1`` symmetrised, Gaussian ``m`` and
    ``nat1``, ``beta`` from ``BETAS`` in turn: the cavity precision is ``P0 + (1 - beta) N > 0``.  Rounded to ``dtype``, as float64."""
    rng = np.random.default_rng(seed)
    case = {"pair_mean": rng.normal(size=(bsz, segs, n)), "nat1": rng.normal(size=(bsz, segs, n)), "pair_cov": np.empty((bsz, segs, n, n)),
            "nat2": np.empty((bsz, segs, n, n)), "beta": np.resize(BETAS, bsz * segs).reshape(bsz, segs)}
    for at in np.ndindex(bsz, segs):
        q = np.linalg.qr(rng.normal(size=(n, n)))[0]
        v = rng.normal(size=(rng.integers(1, n + 1), n)) / np.sqrt(n)
        site = (v.T * (4.0 - 4.0 * rng.random(len(v)))) @ v
        skew = rng.normal(size=(n, n))
        sigma = np.linalg.inv((q * rng.uniform(0.5, 4.0, size=n)) @ q.T + site)
        case["nat2"][at], case["pair_cov"][at] = -0.5 * site + 0.25 * (skew - skew.T), 0.5 * (sigma + sigma.T)
    return {k: v.astype(dtype).astype(np.float64) for k, v in case.items()}


def _spd_inverse(a):
    """``(A^-1, log det A)`` of a symmetric positive definite ``A`` (rows of mpf): ``A = L L^T``, ``X = L^-1``, ``A^-1 = X^T X``."""
    n = len(a)
    low, x = [[mp.mpf(0)] * n for _ in range(n)], [[mp.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            s = a[i][j] - mp.fdot(low[i][:j], low[j][:j])
            low[i][j] = mp.sqrt(s) if i == j else s / low[j][j]
    for j in range(n):
        for i in range(j, n):
            x[i][j] = (int(i == j) - mp.fdot(low[i][j:i], [x[k][j] for k in range(j, i)])) / low[i][i]
    cols = [[x[k][i] for k in range(n)] for i in range(n)]
    return [[mp.fdot(cols[i], cols[j]) for j in range(n)] for i in range(n)], 2 * sum(mp.log(low[i][i]) for i in range(n))


def exact(case, skip=()):
    """``{cav_mean, cav_cov, gamma}`` as float64 arrays, every pair at 50 digits; the pairs in ``skip`` stay NaN."""
    lead, n = case["beta"].shape, case["pair_mean"].shape[-1]
    out = {k: np.full(lead + shape, np.nan) for k, shape in zip(OUTPUTS, ((n,), (n, n), ()))}
    with mp.workdps(50):
        for at in (at for at in np.ndindex(*lead) if at not in skip):
            m, n1 = ([mp.mpf(v) for v in case[k][at].tolist()] for k in ("pair_mean", "nat1"))
            sig, n2 = ([[mp.mpf(v) for v in row] for row in case[k][at].tolist()] for k in ("pair_cov", "nat2"))
            beta = mp.mpf(float(case["beta"][at]))
            prec, logdet_s = _spd_inverse(sig)
            ccov, logdet_p = _spd_inverse([[prec[i][j] + beta * (n2[i][j] + n2[j][i]) for j in range(n)] for i in range(n)])
            lin = [mp.fdot(row, m) for row in prec]
            clin = [a - beta * b for a, b in zip(lin, n1)]
            cmean = [mp.fdot(row, clin) for row in ccov]
            gamma = (-logdet_p + mp.fdot(cmean, clin) - logdet_s - mp.fdot(m, lin)) / 2
            assert mp.im(gamma) == 0, "a pivot of the reference is negative: the case is not what draw() promises"
            out["cav_mean"][at], out["cav_cov"][at], out["gamma"][at] = [float(v) for v in cmean], [[float(v) for v in r] for r in ccov], float(gamma)
    return out


def within_four(tag, got, own, want, keep=...):
    """Per output of a launch: ``max |err| / (|reference| + 1)`` of ``got`` is at most 4 x that of ``own`` on the pairs ``keep``."""
    top, base = ({k: float((np.abs(np.asarray(res[k], dtype=np.float64) - want[k]) / (np.abs(want[k]) + 1.0))[keep].max()) for k in OUTPUTS}
                 for res in (got, own))
    for k in OUTPUTS:
        print(f"ERR {tag} {k}: kernel {top[k]:.3e}  torch {base[k]:.3e}")
    return [f"{tag} {k}: kernel {top[k]:.3e} against torch {base[k]:.3e}" for k in OUTPUTS if not top[k] <= 4.0 * base[k]]
