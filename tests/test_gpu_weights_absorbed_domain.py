"""trt_glow_weights_absorbed on the cells of tests/media_domain.py — spatial scale 2^k, direction length 2^j, origins 4, 12 and
100 bounding radii away, r/R down to 0.02, a centre far from the world origin — on both scenes, with the `curved` tables of
its media times 2^-k, at 1 and 8 sub-steps.

  a. every scaled cell equals its unit cell: weights times 2^-k in bits, trans in bits, on every ray;
  b. the unit cells against absorbed_truth.same_rule at the bars of tests/test_gpu_weights_absorbed.py, 4., with
     max(1, t_last) written as tests/test_gpu_media_domain.py writes it: max(R + r, t_last·len) / len.
"""
import functools

import numpy as np
import pytest

import absorbed_truth as at
import media_domain as md
import solver_domain as sd
import test_gpu_media as gm
import test_gpu_media_domain as tgd
import test_gpu_weights_absorbed as ga
from toroidal_ray_tracing_amd import abi

pytestmark = pytest.mark.gpu

COLOR_RTOL = gm.COLOR_RTOL
SOLVERS, SOLVER_IDS = gm.SOLVERS, gm.SOLVER_IDS
f32, u32 = np.float32, gm.u32
SHAPE = "curved"
COMBOS = [(s, kind, scene) for s in SOLVERS for kind in md.KINDS for scene in md.SCENES]


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


@functools.lru_cache(maxsize=None)
def unit_truth(u, kind, scene, steps, n):
    W, T = at.same_rule(md.truth(u, kind, scene, n), md.tables_of(u, scene, SHAPE), steps)
    W.setflags(write=False)
    T.setflags(write=False)
    return W, T


@pytest.mark.parametrize("solver,kind,scene", COMBOS, ids=lambda p: p if isinstance(p, str) else SOLVER_IDS[SOLVERS.index(p)])
def test_scaled_cells_are_their_unit_cells_and_unit_cells_the_rule(tr, solver, kind, scene):
    """Measured on an MI355X: 632 cells against their unit cells, no ray differs in any bit; the unit cells at 0.143 of the bar
    at the most for a weight and 0.107 for trans (f32 segments, nested), 0.017 and 0.014 with the FP64 solve
    (profiles/r28_glow_weights_absorbed.txt)."""
    cells = [(c, md.N) for c in md.cells(kind)] + [(md.TAIL_CELL, md.N_TAIL), (sd.unit_of(md.TAIL_CELL), md.N_TAIL)]
    out = {}
    for c, n in cells:
        o, d, tmin, tmax = md.rays(c, kind, n)
        tables = md.tables_of(c, scene, SHAPE)
        out[c, n] = {steps: ga.absorbed_dev(tr, md.scene_of(c, scene), o, d, tables, steps, solver, tmin, tmax) for steps in md.STEPS}
    # a. the scale identity, bit for bit
    bad, compared = [], 0
    for c, n in cells:
        u = sd.unit_of(c)
        if c == u:
            continue
        s = f32(2.0 ** -c.k)
        for steps in md.STEPS:
            (W, T), (Wu, Tu) = out[c, n][steps], out[u, n][steps]
            diff = int((u32(W * s) != u32(Wu)).any((0, 1)).sum()), int((u32(T) != u32(Tu)).sum())
            if any(diff):
                bad.append((sd.cell_id(c), n, steps, diff))
        compared += 1
    print(f"{compared} cells against their unit cells: {len(bad)} differ in bits")
    assert not bad, bad[:10]
    assert compared == len(cells) - len(md.unit_cells(kind)) - 1
    # b. the unit cells against the rule in FP64
    worst, worst_T, over = 0.0, 0.0, []
    for u, n in [(c, n) for c, n in cells if c == sd.unit_of(c)]:
        tru = md.truth(u, kind, scene, n)
        ok, far = tru["robust"], md.far_of(u, tru)
        tables = md.tables_of(u, scene, SHAPE)
        bar_T = tgd.profile_bars(tru, tables, gm.ROOT_BAR[solver], far)[1]
        for steps in md.STEPS:
            want, want_T = unit_truth(u, kind, scene, steps, n)
            W, T = out[u, n][steps]
            err, bar = np.abs(W.astype(np.float64) - want), ga.knot_bar(tru, solver, want, bar_T, far)
            err_T = np.abs(T.astype(np.float64) - want_T)
            q, q_T = float((err / bar)[:, :, ok].max()), float((err_T / (bar_T + COLOR_RTOL))[ok].max())
            print(f"{sd.cell_id(u)} n{n} {steps} steps: robust {ok.mean():.4f}; weights {err[:, :, ok].max():.3e} ({q:.3f} of the bar), "
                  f"trans {err_T[ok].max():.3e} ({q_T:.3f})")
            worst, worst_T = max(worst, q), max(worst_T, q_T)
            if q > 1.0 or q_T > 1.0:
                over.append((sd.cell_id(u), n, steps, q, q_T))
        assert (want_T[ok] < 0.99).mean() > 0.2 and (want.sum(1)[:, ok] > 0).any(0).mean() > 0.2, sd.cell_id(u)
    print(f"largest error / bar: weights {worst:.3f}, trans {worst_T:.3f}")
    assert not over, over[:10]
