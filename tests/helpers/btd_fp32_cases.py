"""
Cases, draws and yardsticks of the float32 checks of the block-tridiagonal operators (tests/test_gpu_btd_float32.py): ``cholesky``,
``solve``, ``dense_mult``, ``abs_log_det``, the blocks of the inverse, ``upper_diagonal_lower`` (+ the posterior chain's extras)
and the fused ``mf_btd_logdet_quad``.

The rule is the one of tests/helpers/kl_fp32_cases.py, unchanged (one rule, one set of numbers: imported from there): a float32
kernel is compared with the SEQUENTIAL closed form in float64 on the float32-representable inputs it saw, and its error may be
FP32_FACTOR x the error of the closed forms of tests/helpers/btd_fp32_closed_forms.py evaluated in float32 on the CPU - the larger
of SEEDS draws, never below 2^-24.  The products of ``dense_mult`` are measured by two forms, numpy's own product and the textbook
running sum (``matvec_running_sum``), the larger of the two on every route.  On a route that may cut the time axis the yardstick is the larger of the sequential and the
partitioned form, the latter with the chunk lengths the library computes for the shape (restated below with their sources; where
two engines can take a call, the larger over both plans - the STREAMED rule of tests/helpers/loglik_fp32_cases.py).  The committed
numbers are tests/helpers/btd_fp32_table.py; scripts/btd_fp32_yardsticks.py prints that file (CPU only).  Nothing is derived from
a GPU's output.

Draws (by seed, rounded to float32):
  * ``cholesky``, ``upper_diagonal_lower``, ``logdet_quad``, symmetric ``dense_mult``: the matrix of
    test_gpu_block_tri_diag.random_spd_btd(well=True) - restated block by block (``spd_btd``: the same draws from the generator and
    the same products without the (T d)^2 dense matrix, which 4096 series would not fit; tests/test_btd_closed_forms_host.py pins
    the two against each other) - and at one shape per route the same without a sub-diagonal;
  * ``solve``, lower ``dense_mult``, ``abs_log_det``, the inverse blocks: a FACTOR drawn directly
    (test_gpu_btd_parallel.factor_and_matrix, restated as ``factor_btd`` and pinned the same way): kernel and reference see the
    same factor, one operator's error is not charged to another;
  * right-hand sides, ``eta``: standard normal;
  * from d = 16 on both generators run with a smaller off-diagonal scale (``off_scale`` says why: at their own 0.3 the rounded
    matrices are not positive definite there).
"""
import functools

import numpy as np

from helpers import btd_fp32_closed_forms as F
from helpers import kl_closed_forms as KC
from helpers.kl_fp32_cases import DEFAULT_SEED, SEEDS, FP32_FACTOR, FP32_FLOOR, rounded, abi_calls, ran  # noqa: F401

# route -> (d, T, B): the smallest shapes that reach it (predicates: tests/test_gpu_btd_float32.py::assert_route)
ROUTES = {
    "sweep": [(1, 1, 3), (3, 4, 3), (6, 63, 2), (9, 17, 2), (2, 64, 4096)],            # one lane per series
    "lane_par": [(1, 64, 1), (3, 70, 2), (4, 209, 1), (2, 777, 3)],                    # a lane per chunk; ragged tail; three levels
    "row_par": [(5, 65, 1), (6, 64, 1), (7, 70, 2), (9, 209, 1)],                      # a 16-lane row per chunk
    "row": [(10, 2, 3), (15, 15, 1), (12, 80, 2), (15, 70, 1)],                        # row-only builds; the first two: one chunk per series
    "tile": [(12, 1, 2)],
    "wave": [(16, 9, 3), (21, 67, 2), (32, 130, 1)],
    "panel": [(33, 5, 2), (48, 20, 1), (64, 12, 1)],
}
CASES = [(route,) + shape for route, shapes in ROUTES.items() for shape in shapes]
# one shape per route without a sub-diagonal (cholesky of a block-diagonal matrix, symmetric dense_mult)
NO_SUB_CASES = [("sweep", 3, 4, 3), ("lane_par", 3, 70, 2), ("row_par", 7, 70, 2), ("row", 12, 80, 2), ("tile", 12, 1, 2),
                ("wave", 21, 67, 2), ("panel", 33, 5, 2)]
# mf_btd_logdet_quad_f32: the d <= 9 shapes, on both sides of T = 64; beyond d = 9 the entry point returns -100
LOGDET_QUAD_CASES = [c for c in CASES if c[1] <= 9]
LOGDET_QUAD_UNSUPPORTED = [(12, 80, 2), (16, 9, 3), (40, 5, 1)]

SPD_NAMES = ("chol.diag", "chol.sub", "sym.mult", "udl.u_t", "udl.chol_d", "eta.u_t", "eta.chol_d", "eta.m_post", "eta.chol_dinv")
FACTOR_NAMES = ("solve", "solve_t", "mult", "mult_t", "logdet", "inv.diag", "inv.sub")
NO_SUB_NAMES = ("chol.diag", "sym.mult")


def names_of(t):
    """The outputs a shape has: a single block has no sub-diagonal, hence no U D U^T either."""
    if t == 1:
        return ("chol.diag", "sym.mult"), tuple(n for n in FACTOR_NAMES if n != "inv.sub")
    return SPD_NAMES, FACTOR_NAMES


# ---- the plans of the library, restated ---------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


PAR_RADIX = 5                            # csrc/mf_inst.hip: PAR_RADIX (par_radix(); the shipped library reads no knob, csrc/mf_env.hpp)


def par_len0(bsz, t, d):
    """csrc/mf_inst.hip, par_len0: the level-0 chunk length of the register / row kernels, 0 = one sweep per series.  d <= 9 never
    cuts chains shorter than PAR_MIN_BLOCKS = 64 or PAR_MAX_SERIES = 4096 series; chunks of max(ceil(B T / 65536), RED_CHUNK = 8)
    blocks when that leaves at least two chunks; the row-only builds (10 <= d <= 15) otherwise run ONE chunk per series."""
    lane = d <= 9
    if lane and (bsz >= 4096 or t < 64):
        return 0
    length = max(_cdiv(bsz * t, 65536), 8)
    if t >= 2 * length:
        return length
    return t if (not lane and t >= 2) else 0


def bigpar_plan(bsz, t, d):
    """csrc/mf_bigpar_impl.hpp, bigpar_partition (tile / panel engine, d >= 10): chunk length, or None for one workgroup per series."""
    dp = 16 if d <= 16 else 32 if d <= 32 else 48 if d <= 48 else 64
    per_cu = min(max((160 * 1024) // ((7 * dp * (dp + 4) + 4000) * 4), 1), 4)
    want = max(min((256 * per_cu) // bsz, t // 8), 1)
    length = _cdiv(t, want)
    return None if _cdiv(t, length) < 4 else length


def wave_udl_plan(bsz, t, d, min_chunks=2):
    """csrc/mf_wave_inst.hip, wave_udl_partition (float32; cholesky, U D U^T: more than one chunk; inverse blocks: more than two)."""
    target = 1024 * (4 if d <= 16 else 2)
    want = max(min(_cdiv(target, bsz), 256, t // 16), 1)
    length = _cdiv(t, want)
    return length if _cdiv(t, length) >= min_chunks else None


def wave_solve_plan(bsz, t, d):
    """csrc/mf_wave_inst.hip, wave_solve_partition (as many right-hand sides as factors)."""
    if t < 128:
        return None
    want = min((3072 if d <= 16 else 1024) // bsz, t // 32, 64)
    if want < (2 if d <= 16 else 4):
        return None
    length = _cdiv(t, want)
    return length if _cdiv(t, length) >= 2 else None


def plans(route, operator, d, t, bsz):
    """The ``(len0, radix)`` a call of ``operator`` ("cholesky", "udl", "udl_eta", "solve", "inverse", "logdet_quad") can run with
    at this shape (radix None: one reduced level, walked serially); empty: the sequential recursion only."""
    if operator == "logdet_quad":           # csrc/mf_inst.hip, btd_logdet_quad -> reduce_levels: RED_DEFAULT blocks per chunk on every level
        chunk = 4 if d >= 7 else 8
        return [(chunk, chunk)] if t > chunk else []
    out = []
    if d <= 15:
        length = par_len0(bsz, t, d)
        if 0 < length < t:
            out.append((length, PAR_RADIX))
        # 10 <= d <= 15 with eta in the plain layout: the row kernels write the chain layout only, the tile engine takes the call
        if d >= 10 and operator == "udl_eta" and bigpar_plan(bsz, t, d):
            out.append((bigpar_plan(bsz, t, d), None))
        return out
    if d <= 32:
        wave = {"solve": wave_solve_plan(bsz, t, d), "inverse": wave_udl_plan(bsz, t, d, 3)}.get(operator, wave_udl_plan(bsz, t, d))
        if wave:
            out.append((wave, None))
    if bigpar_plan(bsz, t, d):              # the engine behind the wave kernels' "not mine", and the only one at d > 32
        out.append((bigpar_plan(bsz, t, d), None))
    return out


# ---- draws --------------------------------------------------------------------------------------------------------------------------
def off_scale(d):
    """The generators' scale of everything off the factor's diagonal: their 0.3 up to d = 15.  Beyond that 0.3 gives no test: a
    triangular block of d x d entries 0.3 N(0, 1) under a diagonal of 1 + |N(0, 1)| has an inverse that grows exponentially in d -
    measured on the CPU in float64, the rounded matrix of random_spd_btd is not positive definite in 6 of 8 draws at (32, 130, 1)
    and in all 8 at d = 48 and 64, and the drawn factor's inverse blocks reach 1e42 at (32, 130, 1), past float32's range.  From
    d = 16 on the scale is 0.3 sqrt(12 / d): the variance of a row of the factor stays what it is at d = 12, the largest
    dimension at which the float32 entitlement of these draws was measured (inverse blocks then stay below 12 at every shape)."""
    return 0.3 if d <= 15 else 0.3 * (12.0 / d) ** 0.5


def spd_btd(rng, bsz, t, d, has_sub, scale=0.3):
    """test_gpu_block_tri_diag.random_spd_btd(rng, (bsz,), t, d, has_sub, well=True) block by block: ``(diag, sub or None)``."""
    ldiag = np.tril(rng.normal(loc=1.0, size=(bsz, t, d, d)))
    lsub = rng.normal(size=(bsz, t - 1, d, d)) if has_sub else None
    idx = np.arange(d)
    dg = 1.0 + np.abs(ldiag[..., idx, idx])
    ldiag = scale * (ldiag - 1.0)
    ldiag[..., idx, idx] = dg
    ldiag = np.tril(ldiag)
    diag = ldiag @ np.swapaxes(ldiag, -1, -2)
    if not has_sub:
        return diag, None
    lsub = scale * lsub
    diag[:, 1:] += lsub @ np.swapaxes(lsub, -1, -2)
    return diag, lsub @ np.swapaxes(ldiag[:, :-1], -1, -2)


def factor_btd(rng, bsz, t, d, scale=0.3):
    """The factor of test_gpu_btd_parallel.factor_and_matrix(rng, (bsz,), t, d): ``(ldiag, lsub)``, the same draws in the same order."""
    ldiag = np.tril(scale * rng.normal(size=(bsz, t, d, d)))
    idx = np.arange(d)
    ldiag[..., idx, idx] = 1.0 + np.abs(rng.normal(size=(bsz, t, d)))
    return ldiag, scale * rng.normal(size=(bsz, t - 1, d, d))


def draw_spd(seed, d, t, bsz, has_sub=True):
    """``(diag, sub or None, x, eta)``: the matrix, a vector to multiply and an information vector."""
    rng = np.random.default_rng(seed)
    diag, sub = spd_btd(rng, bsz, t, d, has_sub and t > 1, off_scale(d))
    return rounded(diag), None if sub is None else rounded(sub), rounded(rng.normal(size=(bsz, t, d))), rounded(rng.normal(size=(bsz, t, d)))


def draw_factor(seed, d, t, bsz):
    """``(ldiag, lsub or None, rhs)``: the factor itself."""
    rng = np.random.default_rng(seed)
    ldiag, lsub = factor_btd(rng, bsz, t, d, off_scale(d))
    return rounded(ldiag), rounded(lsub) if t > 1 else None, rounded(rng.normal(size=(bsz, t, d)))


# ---- the closed forms of a case, in one dtype ------------------------------------------------------------------------------------------
def spd_forms(diag, sub, x, eta, dtype, plan_chol=None, plan_udl=None, plan_eta=None):
    """name -> array.  A plan of None: the sequential form."""
    diag, x, eta = diag.astype(dtype), x.astype(dtype), eta.astype(dtype)
    sub = None if sub is None else sub.astype(dtype)
    ld, ls = F.cholesky_sequential(diag, sub) if plan_chol is None else F.cholesky_partitioned(diag, sub, *plan_chol)
    out = {"chol.diag": ld, "sym.mult": F.matvec(diag, sub, x, 2)}
    if sub is not None:
        out["chol.sub"] = ls
        out["udl.u_t"], out["udl.chol_d"] = F.udl_sequential(diag, sub) if plan_udl is None else F.udl_partitioned(diag, sub, *plan_udl)
        res = F.udl_sequential(diag, sub, eta) if plan_eta is None else F.udl_partitioned(diag, sub, *plan_eta, eta=eta)
        out.update(zip(("eta.u_t", "eta.chol_d", "eta.m_post", "eta.chol_dinv"), res))
    return out


def factor_forms(ldiag, lsub, rhs, dtype, plan_solve=None, plan_inv=None):
    ldiag, rhs = ldiag.astype(dtype), rhs.astype(dtype)
    lsub = None if lsub is None else lsub.astype(dtype)
    out = {}
    for name, tr in (("solve", False), ("solve_t", True)):
        out[name] = F.solve_sequential(ldiag, lsub, rhs, tr) if plan_solve is None else F.solve_partitioned(ldiag, lsub, rhs, *plan_solve, transpose=tr)
    out["mult"], out["mult_t"] = F.matvec(ldiag, lsub, rhs, 0), F.matvec(ldiag, lsub, rhs, 1)
    out["logdet"] = F.abs_log_det(ldiag)
    inv = F.inverse_blocks_sequential(ldiag, lsub) if plan_inv is None else F.inverse_blocks_partitioned(ldiag, lsub, *plan_inv)
    out["inv.diag"] = inv[0]
    if lsub is not None:
        out["inv.sub"] = inv[1]
    return out


def error(name, got, want, t, d):
    """The project's metrics: per-series scalars by ``value_error``, tensors by ``tensor_error``."""
    if name in ("logdet", "logdet_quad"):
        return KC.value_error(got, want, t, d)
    return KC.tensor_error(got, want)


@functools.lru_cache(maxsize=None)
def spd_reference(d, t, bsz, seed=DEFAULT_SEED, has_sub=True):
    """``(diag, sub, x, eta, name -> float64 sequential form)`` - computed once, shared by the tests, never modified."""
    draw = draw_spd(seed, d, t, bsz, has_sub)
    return draw + (spd_forms(*draw, np.float64),)


@functools.lru_cache(maxsize=None)
def factor_reference(d, t, bsz, seed=DEFAULT_SEED):
    draw = draw_factor(seed, d, t, bsz)
    return draw + (factor_forms(*draw, np.float64),)


@functools.lru_cache(maxsize=None)
def logdet_quad_reference(d, t, bsz, seed=DEFAULT_SEED):
    diag, sub, x, _, _ = spd_reference(d, t, bsz, seed)
    return diag, sub, x, F.logdet_quad(diag, sub, x)


def _f32(arrays):
    return tuple(None if a is None else a.astype(np.float32) for a in arrays)


def _larger(worst, errs):
    for name, e in errs.items():
        worst[name] = max(worst.get(name, FP32_FLOOR), e)


def _variants(*plan_lists):
    """The sequential form, then each list's plans in turn (the other operators sequential: every output depends on one list)."""
    yield tuple(None for _ in plan_lists)
    for i, lst in enumerate(plan_lists):
        for plan in lst:
            yield tuple(plan if j == i else None for j in range(len(plan_lists)))


def yardstick(route, d, t, bsz, seeds=SEEDS):
    """name -> the float32 closed forms' error against the float64 sequential form, the larger of ``seeds`` draws and of the forms
    the route can evaluate."""
    worst = {}
    for i in range(seeds):
        draw = spd_reference(d, t, bsz, DEFAULT_SEED + i)
        for pc, pu, pe in _variants(plans(route, "cholesky", d, t, bsz), plans(route, "udl", d, t, bsz), plans(route, "udl_eta", d, t, bsz)):
            got = spd_forms(*draw[:4], np.float32, pc, pu, pe)
            _larger(worst, {name: error(name, g, draw[4][name], t, d) for name, g in got.items()})
        _larger(worst, {"sym.mult": error("sym.mult", F.matvec_running_sum(*_f32(draw[:3]), 2), draw[4]["sym.mult"], t, d)})
        draw = factor_reference(d, t, bsz, DEFAULT_SEED + i)
        _larger(worst, {name: error(name, F.matvec_running_sum(*_f32(draw[:3]), mode), draw[3][name], t, d)
                        for mode, name in enumerate(("mult", "mult_t"))})
        for ps, pi in _variants(plans(route, "solve", d, t, bsz), plans(route, "inverse", d, t, bsz)):
            got = factor_forms(*draw[:3], np.float32, ps, pi)
            _larger(worst, {name: error(name, g, draw[3][name], t, d) for name, g in got.items()})
    return worst


def no_sub_yardstick(route, d, t, bsz, seeds=SEEDS):
    worst = {}
    for i in range(seeds):
        draw = spd_reference(d, t, bsz, DEFAULT_SEED + i, False)
        got = spd_forms(*draw[:4], np.float32)
        _larger(worst, {name: error(name, g, draw[4][name], t, d) for name, g in got.items()})
        _larger(worst, {"sym.mult": error("sym.mult", F.matvec_running_sum(*_f32(draw[:3]), 2), draw[4]["sym.mult"], t, d)})
    return worst


def logdet_quad_yardstick(route, d, t, bsz, seeds=SEEDS):
    worst = FP32_FLOOR
    f32 = lambda a: None if a is None else a.astype(np.float32)          # noqa: E731
    for i in range(seeds):
        diag, sub, x, want = logdet_quad_reference(d, t, bsz, DEFAULT_SEED + i)
        for plan in [None] + plans(route, "logdet_quad", d, t, bsz):
            worst = max(worst, error("logdet_quad", F.logdet_quad(f32(diag), f32(sub), f32(x), plan), want, t, d))
    return worst
