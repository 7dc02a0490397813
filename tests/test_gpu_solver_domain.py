"""The kernels on the cells of tests/solver_domain.py — spatial scale 2^k, direction length 2^j, origins 4, 12 and 100
bounding radii away, r/R down to 0.02, a centre far from the world origin — 1,024 rays a cell (16 blocks of 64, no
tail) and one cell at 1,000 (a tail).  trt_trace stays bit-equal to the oracle with every solver (the CPU file holds the
oracle to the FP64 truth on the same cells); trt_occluded, trt_crossings and an oriented torus, which the oracle does
not restate, are held to the truth directly."""
import numpy as np
import pytest

import oriented_truth
import solver_domain as sd
from toroidal_ray_tracing_amd import abi

pytestmark = pytest.mark.gpu

N = sd.N_GPU
GEOM = ("t", "px", "py", "pz", "nx", "ny", "nz")
ALL_SOLVERS = [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64, abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_DK_F64, abi.TRT_SOLVE_FERRARI_F32,
               abi.TRT_SOLVE_FERRARI_F64]
ALL_SOLVER_IDS = ["f32", "f64", "dk32", "dk64", "ferrari32", "ferrari64"]
DEFAULT = [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64]
DEFAULT_IDS = ["f32", "f64"]
BAR = {abi.TRT_SOLVE_F32: sd.BAR_F32, abi.TRT_SOLVE_F64: sd.BAR_F64}
TAIL_CELL = sd.Cell(0, -10, 100.0, 0.02, (0.0, 0.0, 0.0))   # … and with 1,000 rays: 15 blocks and a tail of 40


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


class solver:
    """`with solver(tr, p):` — the ctx solves with p inside, with the default afterwards."""
    def __init__(self, tr, precision):
        self.tr, self.p = tr, precision

    def __enter__(self):
        self.tr.set_solver(self.p)

    def __exit__(self, *exc):
        self.tr.set_solver(abi.TRT_SOLVE_F32)


def cells_for(precision):
    return sd.GRID_DEFAULT + (sd.GRID_F64_ONLY if precision == abi.TRT_SOLVE_F64 else [])


def assert_trace_equals_oracle(tr, oracle, c, precision, n):
    o, d = sd.rays(c, n)
    tmin, tmax, _ = sd.interval(c)
    with solver(tr, precision):
        got = tr.trace(sd.scene(c), o, d, tmin, tmax)
    want, _ = oracle.trace(sd.scene(c), o, d, tmin, tmax, precision=precision, nthreads=8)
    assert np.array_equal(got["id"], want["id"]), sd.cell_id(c)
    for k in GEOM:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (sd.cell_id(c), k)
    return got


@pytest.mark.parametrize("precision", ALL_SOLVERS, ids=ALL_SOLVER_IDS)
def test_trace_bit_equal_to_the_oracle_on_every_cell(tr, oracle, precision):
    """Every output stream of trt_trace, bit for bit, on every cell of the grid (the dist = 1e4 cells with the FP64
    default solver), and on one cell with 1,000 rays.  With the default solvers the hits are then also those the CPU file
    holds to the truth; a default solver that reports fewer than 200 hits on a cell has not been given its rays."""
    for c in cells_for(precision):
        got = assert_trace_equals_oracle(tr, oracle, c, precision, N)
        if precision in DEFAULT:
            assert np.isfinite(got["t"]).sum() >= sd.MIN_HITS, sd.cell_id(c)
    assert_trace_equals_oracle(tr, oracle, TAIL_CELL, precision, 1000)


@pytest.mark.parametrize("precision", DEFAULT, ids=DEFAULT_IDS)
def test_trace_vs_truth_on_every_cell(tr, precision):
    """The kernels against the truth directly, at this file's ray count: hit/miss and id on every robust ray, t within
    the bar (what test_solver_domain_cpu.py asserts of the oracle at 4,000 rays)."""
    for c in cells_for(precision):
        tru = sd.first_hit_truth(c, N)
        sd.check_inputs(c, tru)
        o, d = sd.rays(c, N)
        tmin, tmax, _ = sd.interval(c)
        with solver(tr, precision):
            got = tr.trace(sd.scene(c), o, d, tmin, tmax)
        hit, hit_t = np.isfinite(got["t"]), ~np.isnan(tru.t)
        assert not np.any((hit != hit_t) & tru.robust), sd.cell_id(c)
        both = hit & hit_t & tru.robust
        assert np.array_equal(got["id"][both], tru.id[both])
        err = sd.position_error(c, got["t"], tru, both)
        assert err.max() <= BAR[precision], (sd.cell_id(c), err.max())


@pytest.mark.parametrize("precision", DEFAULT, ids=DEFAULT_IDS)
@pytest.mark.parametrize("factor", [1.5, 0.5])
def test_occluded_with_a_bound_either_side_of_the_first_hit(tr, precision, factor):
    """trt_occluded with a per-ray tmax of 1.5 and 0.5 times the truth's first-hit t (the cell's tmax where the truth
    misses): the bit equals "truth's first hit < tmax" on every robust ray whose t is not within t_tol of that tmax."""
    for c in cells_for(precision):
        tru = sd.first_hit_truth(c, N)
        o, d = sd.rays(c, N)
        tmin, tmax, t_tol = sd.interval(c)
        hit_t = ~np.isnan(tru.t)
        bound = np.where(hit_t, factor * np.where(hit_t, tru.t, 0.0), tmax).astype(np.float32)
        with solver(tr, precision):
            got = tr.occluded(sd.scene(c), o, d, tmin, tmax, tmax_per_ray=bound)
        want = hit_t & (np.where(hit_t, tru.t, np.inf) < bound.astype(np.float64))
        ok = tru.robust & ~(hit_t & (np.abs(np.where(hit_t, tru.t, 0.0) - bound) <= t_tol))
        assert ok.sum() >= sd.MIN_HITS + sd.MIN_MISSES
        assert np.array_equal(got[ok], want[ok]), (sd.cell_id(c), int((got[ok] != want[ok]).sum()))
        assert want[ok].sum() >= (sd.MIN_HITS if factor > 1.0 else 0)


@pytest.mark.parametrize("precision", DEFAULT, ids=DEFAULT_IDS)
@pytest.mark.parametrize("nested", [False, True], ids=["one", "nested"])
def test_crossings_equal_the_truth_on_every_cell(tr, precision, nested):
    """trt_crossings on a cell's torus alone, and with a second torus nested about the same centre circle (half the tube
    radius, inside; for the thin cells twice, outside, so that both stay within the grid's r/R): count,
    order, ids and entering equal crossings_truth.all_crossings on every ray that is robust by classify_margin_all
    (delta 1e-3, t_tol 1e-2·(R + r)/|d| — in the thin cells that leaves out the rays whose crossings of the two walls,
    r apart, lie within t_tol of each other; at least 100 rays with crossings remain in every cell), each t within the
    bar, and slot 0 is trt_trace's hit bit for bit."""
    for c in cells_for(precision):
        o, d = sd.rays(c, N)
        tmin, tmax, _ = sd.interval(c)
        _, R, r, dlen = sd.geometry(c)
        tori = sd.nested_tori(c)
        sc = sd.scene(c, tori[1:] if nested else ())
        want = sd.crossings_truth_of(c, nested, N)
        K = want.t.shape[1]
        with solver(tr, precision):
            t, tid, en, cnt = tr.crossings(sc, o, d, tmin, tmax, max_per_ray=K)
            first = tr.trace(sc, o, d, tmin, tmax)
        t, tid, en, cnt = np.ascontiguousarray(t.T), np.ascontiguousarray(tid.T), np.ascontiguousarray(en.T), cnt.astype(np.int64)
        tag = sd.cell_id(c)
        # slot 0 is the closest hit
        assert np.array_equal(cnt > 0, first["id"] >= 0), tag
        assert np.array_equal(t[:, 0].view(np.uint32), first["t"].view(np.uint32)) and np.array_equal(tid[:, 0], first["id"]), tag
        ok = want.robust
        assert (ok & (want.count > 0)).sum() >= 100, (tag, int((ok & (want.count > 0)).sum()))
        assert np.array_equal(cnt[ok], want.count[ok]), (tag, int((cnt[ok] != want.count[ok]).sum()))
        assert np.array_equal(tid[ok], want.id[ok]) and np.array_equal(en[ok], want.entering[ok]), tag
        used = (want.id >= 0) & ok[:, None]
        tt = np.where(used, want.t, 1.0)
        err = np.where(used, np.abs(np.where(used, t, 1.0).astype(np.float64) - tt) * dlen / np.maximum(R + r, tt * dlen), 0.0)
        assert err.max() <= BAR[precision], (tag, err.max())


@pytest.mark.parametrize("precision", DEFAULT, ids=DEFAULT_IDS)
@pytest.mark.parametrize("j", [-10, 0])
def test_oriented_torus_far_away(tr, precision, j):
    """One torus about a tilted axis (trt_set_torus_axes), r/R = 0.02, origins 100 bounding radii away, |d| = 2^-10 and
    1, against oriented_truth to the same bar.  The oracle knows no axes: this is the check of the rotated path off the
    unit scale.  The rays are the cell's, carried into the torus' frame and rounded to FP32 there — what the truth sees."""
    c = sd.Cell(0, j, 100.0, 0.02, (0.0, 0.0, 0.0))
    C, R, r, dlen = sd.geometry(c)
    axis = (0.25, 0.75, -0.5)   # FP32 numbers: the library and the truth normalise the same vector
    M = oriented_truth.frame(axis)
    ol, dl = sd.rays(c, N)
    o, d = (ol.astype(np.float64) @ M).astype(np.float32), (dl.astype(np.float64) @ M).astype(np.float32)   # world = M.T @ local
    tmin, tmax, t_tol = sd.interval(c)
    tori = [(C, axis, R, r)]
    t, tid = oriented_truth.first_hit(o, d, tori, tmin, tmax)
    rob = oriented_truth.classify_margin(o, d, tori, tmin, tmax, delta=sd.DELTA, t_tol=t_tol)
    tru = sd.Truth(t, tid, rob)
    sd.check_inputs(c, tru)
    from toroidal_ray_tracing_amd import camera
    sc = abi.Scene([(tuple(C), R, r, 0)], [camera.MIRROR], axes=[axis])
    with solver(tr, precision):
        got = tr.trace(sc, o, d, tmin, tmax)
    hit, hit_t = np.isfinite(got["t"]), ~np.isnan(t)
    assert not np.any((hit != hit_t) & rob), int(((hit != hit_t) & rob).sum())
    both = hit & hit_t & rob
    err = sd.position_error(c, got["t"], tru, both)
    assert err.max() <= BAR[precision], err.max()
    P = np.stack([got["px"], got["py"], got["pz"]], 1)[both].astype(np.float64)
    Ng = np.stack([got["nx"], got["ny"], got["nz"]], 1)[both].astype(np.float64)
    assert np.abs(Ng - oriented_truth.normal(P, C, axis, R)).max() < 2e-5 * max(1.0, R / r)
