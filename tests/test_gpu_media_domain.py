"""trt_chords, trt_glow, trt_glow_profile and trt_glow_weights on the cells of tests/media_domain.py — spatial scale 2^k,
direction length 2^j, origins 4, 12 and 100 bounding radii away, r/R down to 0.02, a centre far from the world origin; lines
of sight and segments that start and end inside the tubes; the cell's torus alone and two nested ones — 1,024 rays a cell
and one cell at 1,000 (a tail).  The oracle does not restate this family: the kernels are held to the FP64 truth directly.

Anchors, from the strictest down:
  a. trt_crossings on the segments — the roots under everything else, for origins and window ends inside a tube;
  b. the library's own crossings — trt_chords is the pairing rule applied in numpy FP32 to what trt_crossings_dev lists,
     bit for bit wherever the window's end points are clear; torus j of the nested scene is torus j alone on every ray;
  c. the scale identities — every output of every cell is its unit cell's times the power of two, bit for bit, on every
     ray: an absolute constant, an overflow or an underflow anywhere in the kernels breaks it;
  d. e. the FP64 truth at the bars of the unit-scale tests with their one absolute term, max(1, t_last)·len, made scale
     free: max(R + r, t_last·len) — the form in which solver_domain states the bar on a root;
  f. an oriented torus;  g. the closed forms of rays parallel to the axis.
Far away the bars are loose by the number format alone: an FP32 t of 100 bounding radii carries the root bar of 1e-5 of
its own size, 1e-3·(R + r) — for the tube of r/R = 0.02 the chord bar 4·BAR·t·len is 4e-3 R, about 13 % of a chord of 1.5 r.
Anchors b and c carry those cells: they do not loosen with distance.

Every test prints, per cell, the largest error and error / bar of each family on the robust rays and how many non-robust
rays exceed a bar; profiles/r27_media_domain.txt is that table as measured on an MI355X.
"""
import numpy as np
import pytest

import media_domain as md
import oriented_truth
import profile_truth as pt
import solver_domain as sd
import test_gpu_media as gm
import test_gpu_profile as gp
import test_gpu_weights as gw
import weights_truth as wt
from toroidal_ray_tracing_amd import abi

pytestmark = pytest.mark.gpu

COLOR_RTOL, COLOR_ATOL = gm.COLOR_RTOL, gm.COLOR_ATOL
SOLVERS, SOLVER_IDS = gm.SOLVERS, gm.SOLVER_IDS
BAR = {abi.TRT_SOLVE_F32: sd.BAR_F32, abi.TRT_SOLVE_F64: sd.BAR_F64}
assert BAR == gm.ROOT_BAR   # (the helpers of the unit-scale tests take the root bar from there)
f32, u32 = np.float32, gm.u32
PROFILE_CALLS = (("slanted", 1), ("curved", 8))   # (shape, steps) of the two trt_glow_profile calls a cell gets
K_KEPT = 8                                        # slots of a crossings list kept: two tori have at most eight
COMBOS = [(s, kind, scene) for s in SOLVERS for kind in md.KINDS for scene in md.SCENES]


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def sid(solver):
    return SOLVER_IDS[SOLVERS.index(solver)]


def calls(tr, sc, o, d, tmin, tmax, media, tables, solver, alone=()):
    """Every output of one cell: dict(cross (t, id, entering) (K_KEPT, n), chords, glow, prof[(shape, steps)], W[steps],
    alone[j]: the chords of the scene that holds torus j alone)."""
    w = dict(solver=solver, tmin=tmin, tmax=tmax)
    t, tid, en = gm.crossings_dev(tr, sc, o, d, solver, tmin, tmax)
    assert (tid[K_KEPT:] < 0).all()
    out = dict(cross=(t[:K_KEPT].copy(), tid[:K_KEPT].copy(), en[:K_KEPT].copy()),
               chords=gm.chords_dev(tr, sc, o, d, **w), glow=gm.glow_dev(tr, sc, o, d, media, **w),
               prof={(shape, steps): gp.profile_dev(tr, sc, o, d, tables[shape], steps, **w) for shape, steps in PROFILE_CALLS},
               W={steps: gw.weights_dev(tr, sc, o, d, steps, **w) for steps in md.STEPS},
               alone=[gm.chords_dev(tr, one, o, d, **w) for one in alone])
    return out


class Run:
    """The outputs of every cell of one (solver, kind, scene), made once and shared by the tests b to e."""
    def __init__(self, tr, solver, kind, scene):
        self.solver, self.kind, self.scene, self.bar = solver, kind, scene, BAR[solver]
        self.cells = [(c, md.N) for c in md.cells(kind)] + [(md.TAIL_CELL, md.N_TAIL), (sd.unit_of(md.TAIL_CELL), md.N_TAIL)]
        self.out = {}
        for c, n in self.cells:
            o, d, tmin, tmax = md.rays(c, kind, n)
            alone = [md.scene_of(c, "one")] + [self.second_alone(c)] if scene == "nested" else []
            self.out[c, n] = calls(tr, md.scene_of(c, scene), o, d, tmin, tmax, md.media_of(c, scene),
                                   {shape: md.tables_of(c, scene, shape) for shape in md.SHAPES}, solver, alone)

    @staticmethod
    def second_alone(c):
        from toroidal_ray_tracing_amd import camera
        C, R, r = md.geo_of(c, "nested")[1]
        return abi.Scene([(C, R, r, 0)], [camera.PLASTIC])

    def tag(self, c, n):
        return f"{sid(self.solver)} {self.kind} {self.scene} {sd.cell_id(c)}" + (f" n{n}" if n != md.N else "")

    def truth(self, c, n):
        return md.truth(c, self.kind, self.scene, n)


@pytest.fixture(scope="module", params=COMBOS, ids=lambda p: f"{sid(p[0])}-{p[1]}-{p[2]}")
def run(request, tr):
    return Run(tr, *request.param)


def report(lines, bad):
    print("\n".join(lines))
    assert not bad, bad[:10]


def ratio_of(err, bar, sel):
    """(largest error, largest error / bar) over the rays sel (last axis), and the rays of ~sel over their bar."""
    e, q = np.where(sel, err, 0.0), np.where(sel, err / bar, 0.0)
    over = (err > bar) & ~sel
    return float(e.max()), float(q.max()), int(over.reshape(-1, over.shape[-1]).any(0).sum())


# ---------------------------------------------------------------------------------------------------------------------
# a. crossings of segments
# ---------------------------------------------------------------------------------------------------------------------
def test_crossings_equal_the_truth(run):
    """trt_crossings on rays that start and end inside the tubes, window (1e-3, 1)·2^(-j): count, ids and entering equal
    crossings_truth.all_crossings on every robust ray, each t within the bar in its scale-free form
    |dt|·|d| <= bar·max(R + r, t·|d|) — test_crossings_equal_the_truth_on_every_cell, extended to origins and window ends
    inside a tube.  (The lines of sight are that test's own rays; they run through the same lines here, on this file's
    robust rays, so that every list the other anchors build on has been held to the truth in this file.)
    Measured on an MI355X: no list wrong on a robust ray; largest |dt| / bar 0.30 on the segments (f32, the thin tube at the
    far centre, nested) and 0.07 on the lines of sight; 0.03 with the FP64 solver.  DESIGN.md's known item — Newton's early
    stop on a shallow chord of the thin tube — does not show on these segments."""
    lines, bad = [], []
    for c, n in run.cells:
        tru, tag = run.truth(c, n), run.tag(c, n)
        u = sd.unit_of(c)
        _, R, r, _ = sd.geometry(u)
        want_t, want_id, want_en, want_cnt = md.crossings_of(c, run.kind, run.scene, n)
        t, tid, en = (np.ascontiguousarray(a.T) for a in run.out[c, n]["cross"])
        ok = tru["robust"]
        cnt = (tid >= 0).sum(1)
        K = want_t.shape[1]
        same = (cnt == want_cnt) & (tid[:, :K] == want_id).all(1) & (en[:, :K] == want_en).all(1)
        used = (want_id >= 0) & ok[:, None] & same[:, None]
        tt = np.where(used, want_t, 1.0)
        got = np.where(used, t[:, :K].astype(np.float64) / md.t_scale(c, run.kind), 1.0)
        err = np.abs(got - tt) * tru["len"][:, None] / np.maximum(R + r, tt * tru["len"][:, None])
        lines.append(f"{tag}: crossings: robust {ok.mean():.4f}, lists wrong on robust rays {int((~same & ok).sum())}, "
                     f"on others {int((~same & ~ok).sum())}; largest t error / bar {err.max() / run.bar:.3f}")
        if (~same & ok).any() or err.max() > run.bar:
            bad.append((tag, int((~same & ok).sum()), err.max() / run.bar))
        assert (ok & (want_cnt > 0)).sum() >= sd.MIN_HITS, tag
    report(lines, bad)


# ---------------------------------------------------------------------------------------------------------------------
# b. chords from the library's own crossings; a torus in the nested scene against the torus alone
# ---------------------------------------------------------------------------------------------------------------------
def test_chords_are_the_pairing_of_the_librarys_crossings(run):
    """trt_chords equals gm.pair_f32 — the pairing rule in numpy FP32 — applied to what trt_crossings_dev lists, with the
    truth's in0 / in1, bit for bit wherever both end points of the window are clear of every surface (by 1e-2·r_j); and
    torus j of the nested scene is torus j alone, bit for bit on every ray.  Nothing here loosens with distance.
    Measured on an MI355X: no ray differs in any cell, with clear ends or without."""
    lines, bad = [], []
    for c, n in run.cells:
        tru, tag, out = run.truth(c, n), run.tag(c, n), run.out[c, n]
        o, d, tmin, tmax = md.rays(c, run.kind, n)
        t, tid, en = out["cross"]
        want = gm.pair_f32(t, tid, en, md.n_tori(run.scene), tru["info"]["in0"], tru["info"]["in1"], tmin, tmax, gm.length_f32(d))
        differ = (u32(out["chords"]) != u32(want)).any(0)
        clear = tru["ends_clear"]
        lines.append(f"{tag}: chords vs pairing: {int(differ.sum())} rays differ in bits, {int((differ & clear).sum())} of them with clear ends "
                     f"(not clear: {int((~clear).sum())})")
        if (differ & clear).any():
            bad.append((tag, "pairing", int((differ & clear).sum())))
        for j, alone in enumerate(out["alone"]):
            if not np.array_equal(u32(out["chords"][j]), u32(alone[0])):
                bad.append((tag, "alone", j))
        assert (out["chords"] >= 0).all() and (out["chords"] > 0).any(0).sum() >= md.MIN_CHORD, tag
    report(lines, bad)


# ---------------------------------------------------------------------------------------------------------------------
# c. scale identities
# ---------------------------------------------------------------------------------------------------------------------
def test_every_cell_is_its_unit_cell_scaled_bit_for_bit(run):
    """The kernels use only + - x / sqrt fma on top of the scale-free solve, and every constant in them is a ratio (the
    series threshold and the exponential act on optical depths, the table index on rho² / r²): with the scene, the origins
    and the window scaled by 2^k, the directions by 2^j and the media by 2^(-k), chords·2^(-k) and weights·2^(-k) are the
    unit cell's bit for bit, and so is the rgba of trt_glow and trt_glow_profile — on every ray, robust or not.  (The
    crossings under them are compared too: t·2^(j - k), ids, entering.)  Measured on an MI355X: 632 cells against their
    unit cells, no ray differs in any output.  With `< r2 + 1e-6f` in tube_inside, tried once, every k = -10 segment cell
    differs on some 450 rays, and b, d and e fail with it."""
    lines, bad = [], []
    for c, n in run.cells:
        u = sd.unit_of(c)
        if c == u or (u, n) not in run.out:
            continue
        got, base, tag = run.out[c, n], run.out[u, n], run.tag(c, n)
        s = f32(2.0 ** -c.k)
        diffs = {"crossings": int((u32(got["cross"][0] * f32(1.0 / md.t_scale(c, run.kind))) != u32(base["cross"][0])).any(0).sum()
                                  + (got["cross"][1] != base["cross"][1]).any(0).sum() + (got["cross"][2] != base["cross"][2]).any(0).sum()),
                 "chords": int((u32(got["chords"] * s) != u32(base["chords"])).any(0).sum()),
                 "glow": int((u32(got["glow"]) != u32(base["glow"])).any(1).sum())}
        for key in PROFILE_CALLS:
            diffs[f"profile {key[0]} {key[1]}"] = int((u32(got["prof"][key]) != u32(base["prof"][key])).any(1).sum())
        for steps in md.STEPS:
            diffs[f"weights {steps}"] = int((u32(got["W"][steps] * s) != u32(base["W"][steps])).any((0, 1)).sum())
        lines.append(f"{tag}: rays that differ from the unit cell in bits: " + ", ".join(f"{k} {v}" for k, v in diffs.items()))
        if any(diffs.values()):
            bad.append((tag, {k: v for k, v in diffs.items() if v}))
    report(lines, bad)
    assert len(lines) == len(run.cells) - len(md.unit_cells(run.kind)) - 1   # (every cell but the unit cells, the tail's included)


# ---------------------------------------------------------------------------------------------------------------------
# d. the FP64 truth: chords
# ---------------------------------------------------------------------------------------------------------------------
def test_chords_against_the_fp64_truth(run):
    """Every interval end that is not an end of the window is a trt_crossings root, held to |dt|·len <= BAR·max(R + r, t·len)
    (a above, and test_gpu_solver_domain.py for the lines of sight).  A torus has at most four of them, and t <= t_last:
      |d chord_j| <= 4·BAR·max(R + r, t_last·len) + COLOR_RTOL·chord_j
    — test_against_the_fp64_truth's bar with max(1, t_last)·len made scale free; the second term is for the FP32 sum
    (v - u)·len of at most two intervals.  Compared in the unit frame: chords·2^(-k), an exact scaling.
    From 100 bounding radii the first term is 4e-3·(R + r) with the FP32 solver — about 13 % of a thin tube's chord of
    1.5 r: loose by the number format, not by choice; b and c carry those cells.  Measured on an MI355X: error / bar at
    most 0.12 (f32 segments, the thin tube at the far centre, nested: 2.3e-6 absolute), 0.035 on the lines of sight
    (1.9e-5 absolute at dist 100), 0.018 with the FP64 solver; one non-robust ray over the bar (thin tube, far centre)."""
    lines, bad = [], []
    for c, n in run.cells:
        tru, tag = run.truth(c, n), run.tag(c, n)
        ok = tru["robust"]
        geom = run.bar * md.far_of(sd.unit_of(c), tru) * tru["len"]
        got = run.out[c, n]["chords"].astype(np.float64) * 2.0 ** -c.k
        err, bar = np.abs(got - tru["chords"]), 4.0 * geom[None, :] + COLOR_RTOL * tru["chords"]
        e, q, over = ratio_of(err, bar, ok[None, :])
        lines.append(f"{tag}: chords: robust {ok.mean():.4f}, largest error {e:.3e} ({q:.3f} of the bar); non-robust rays over the bar: "
                     f"{over} of {int((~ok).sum())}")
        if q > 1.0:
            bad.append((tag, q))
    report(lines, bad)


# ---------------------------------------------------------------------------------------------------------------------
# e. the FP64 truth: glow, profile, weights
# ---------------------------------------------------------------------------------------------------------------------
def test_glow_against_the_fp64_truth(run):
    """L and T of trt_glow at test_against_the_fp64_truth's bars, scale free: moving one of the ray's E_n interval ends by
    dt changes L_c by at most (sum_j eps_j,c)·dt·len and T by at most (sum_j sigma_j)·dt·len, with
    dt·len <= BAR·max(R + r, t_last·len):
      |dL_c| <= (sum eps_c)·E_n·BAR·max(R + r, t_last·len) + COLOR_RTOL·|L_c| + COLOR_ATOL,
      |dT|   <= (sum sigma)·E_n·BAR·max(R + r, t_last·len) + COLOR_RTOL
    in the unit frame (a cell of scale 2^k has media times 2^(-k): L and T are the unit cell's).
    Measured on an MI355X: error / bar at most 0.093 for L and 0.059 for T (f32 segments, the thin tube at the far centre),
    0.065 and 0.052 on the lines of sight, 0.026 with the FP64 solver."""
    lines, bad = [], []
    for c, n in run.cells:
        tru, tag = run.truth(c, n), run.tag(c, n)
        ok = tru["robust"]
        geom = run.bar * md.far_of(sd.unit_of(c), tru) * tru["len"]
        eps = np.array([m[0] for m in tru["media"]]).sum(0)
        sig = sum(m[1] for m in tru["media"])
        rgba = run.out[c, n]["glow"].astype(np.float64)
        err_L, bar_L = np.abs(rgba[:, :3] - tru["L"]), eps[None, :] * (tru["ends"] * geom)[:, None] + COLOR_RTOL * np.abs(tru["L"]) + COLOR_ATOL
        err_T, bar_T = np.abs(rgba[:, 3] - tru["T"]), sig * tru["ends"] * geom + COLOR_RTOL
        eL, qL, oL = ratio_of(err_L.T, bar_L.T, ok[None, :])
        eT, qT, oT = ratio_of(err_T, bar_T, ok)
        lines.append(f"{tag}: glow: L {eL:.3e} ({qL:.3f}), T {eT:.3e} ({qT:.3f}); non-robust rays over a bar: {max(oL, oT)} of {int((~ok).sum())}")
        if max(qL, qT) > 1.0:
            bad.append((tag, qL, qT))
        assert (tru["L"][ok].max(1) > 1e-3).mean() > 0.2 and (tru["T"][ok] < 0.99).mean() > 0.2, tag   # (the set sees the media)
    report(lines, bad)


def profile_bars(tru, tables, bar, far):
    """test_gpu_profile.bars with max(1, t_last) replaced by far = max(R + r, t_last·len) / len."""
    top = np.array([np.asarray(t, np.float64).max(0) for t in tables]).sum(0)
    geom = bar * far * tru["len"]
    moved = pt.slope_term(tru, tables, bar, far)
    return top[None, :3] * (tru["ends"] * geom)[:, None] + moved[:, :3], top[3] * tru["ends"] * geom + moved[:, 3]


def test_profile_against_the_same_rule_in_fp64(run):
    """trt_glow_profile (slanted tables at 1 sub-step, curved ones at 8) against profile_truth.same_rule at the same step
    count, at the bars of test_gpu_profile.py's test_against_the_same_rule_in_fp64 with max(1, t_last)·len replaced by
    max(R + r, t_last·len) in both of its terms: (a) the E_n ends that move by dt lengthen or shorten a piece —
    top_c·E_n·BAR·max(R + r, t_last·len); (b) the samples sit at fixed fractions of a piece and move with its ends —
    slope_c·(2 / r_min)·BAR·max(R + r, t_last·len)·chords (profile_truth.slope_term); (c) COLOR_RTOL·|L_c| + COLOR_ATOL and
    COLOR_RTOL for FP32 in the sums.  The sample parameters are formed in float even with the FP64 solver: at 100 bounding
    radii a sample's t carries 2^-24·t·len = 6e-6·(R + r) of position, inside (b)'s 1e-5 (FP32) and above its 2e-6 (FP64) —
    but a sample's shift moves x by |dx/dt|·dt and the bar integrates the largest slope over the whole chord, so it
    holds with room: measured on an MI355X, FP64 solver at dist 100, 0.016 of the bar at the most (T, thin tube, far
    centre: 1.2e-5 absolute).  Largest error / bar overall: 0.138 for L and 0.111 for T (f32 segments, slanted at one
    sub-step, the thin tube at the far centre: 2.1e-5 absolute); 0.039 on the lines of sight."""
    lines, bad = [], []
    for c, n in run.cells:
        tru, tag = run.truth(c, n), run.tag(c, n)
        ok, u = tru["robust"], sd.unit_of(c)
        far = md.far_of(u, tru)
        for shape, steps in PROFILE_CALLS:
            tables = md.tables_of(u, run.scene, shape)
            want_L, want_T = md.profile_truth_of(c, run.kind, run.scene, shape, steps, n)
            got = run.out[c, n]["prof"][shape, steps].astype(np.float64)
            bar_L, bar_T = profile_bars(tru, tables, run.bar, far)
            bar_L, bar_T = bar_L + COLOR_RTOL * np.abs(want_L) + COLOR_ATOL, bar_T + COLOR_RTOL
            eL, qL, oL = ratio_of(np.abs(got[:, :3] - want_L).T, bar_L.T, ok[None, :])
            eT, qT, oT = ratio_of(np.abs(got[:, 3] - want_T), bar_T, ok)
            lines.append(f"{tag}: profile {shape} {steps}: L {eL:.3e} ({qL:.3f}), T {eT:.3e} ({qT:.3f}); non-robust rays over a bar: "
                         f"{max(oL, oT)} of {int((~ok).sum())}")
            if max(qL, qT) > 1.0:
                bad.append((tag, shape, steps, qL, qT))
    report(lines, bad)


def test_weights_against_the_same_rule_in_fp64(run):
    """trt_glow_weights at 1 and 8 sub-steps against weights_truth.same_rule, at test_gpu_weights.py's knot_bar with
    max(1, t_last) replaced by max(R + r, t_last·len) / len: (a) E_j·BAR·max(R + r, t_last·len); (b) 16·(2 / r_j)·(BAR + 2^-23)·
    max(R + r, t_last·len)·chord_j — the 2^-23 is the samples' own FP32 rounding of t; (c) COLOR_RTOL·W_k + COLOR_ATOL.
    And the partition: the 17 weights of a torus sum to its trt_chords length within test_gpu_weights.partition_bar, a
    count of roundings that is scale free as it stands.  Compared in the unit frame: weights·2^(-k).
    Measured on an MI355X: error / bar at most 0.144 (f32 segments, 1 sub-step, the thin tube at the far centre: 4.2e-4
    absolute), 0.087 on the lines of sight, 0.021 with the FP64 solver; the sums at most 0.086 of the partition's bar."""
    lines, bad = [], []
    for c, n in run.cells:
        tru, tag, out = run.truth(c, n), run.tag(c, n), run.out[c, n]
        ok = tru["robust"]
        far = md.far_of(sd.unit_of(c), tru)
        length = out["chords"].astype(np.float64)
        for steps in md.STEPS:
            want = md.weights_truth_of(c, run.kind, run.scene, steps, n)
            W = out["W"][steps].astype(np.float64)
            e, q, over = ratio_of(np.abs(W * 2.0 ** -c.k - want), gw.knot_bar(tru, run.solver, want, far), ok[None, None, :])
            part, part_bar = np.abs(W.sum(1) - length), gw.partition_bar(steps, length)
            with np.errstate(invalid="ignore", divide="ignore"):
                qp = float(np.nanmax(np.where(length > 0, part / part_bar, 0.0)))
            lines.append(f"{tag}: weights {steps}: {e:.3e} ({q:.3f}), sum against the chord {qp:.3f} of its bar; non-robust rays over the bar: "
                         f"{over} of {int((~ok).sum())}")
            if q > 1.0 or not (part <= part_bar).all():
                bad.append((tag, steps, q, qp))
            assert (u32(out["W"][steps])[np.broadcast_to((length == 0)[:, None, :], W.shape)] == 0).all(), tag   # no chord: 17 zeros in bits
    report(lines, bad)


# ---------------------------------------------------------------------------------------------------------------------
# f. an oriented torus
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind", md.KINDS)
@pytest.mark.parametrize("j", [-10, 0])
def test_oriented_torus_far_away(tr, j, kind, solver):
    """One torus about the tilted axis of test_gpu_solver_domain.py's test_oriented_torus_far_away, r/R = 0.02, |d| = 2^-10
    and 1: the lines of sight from 100 bounding radii and the segments of that cell, carried into the torus' frame and
    rounded to FP32 there — what the truth sees.  Chords, glow and one profile call (curved, 8 sub-steps) at the bars of d
    and e; the inside tests and the samples run in the rotated frame here.  Measured on an MI355X: error / bar at most
    0.29 (chords, f64 segments: 3.8e-6 absolute, against 5.0e-6 with the FP32 solver, whose bar is five times wider: 0.11)
    and 0.20 (glow L, the same rays); the lines of sight at most 0.04."""
    c = sd.Cell(0, j, 100.0, 0.02, (0.0, 0.0, 0.0))
    axis = (0.25, 0.75, -0.5)
    M = oriented_truth.frame(axis)
    ol, dl, tmin, tmax = md.rays(c, kind)
    o, d = (ol.astype(np.float64) @ M).astype(f32), (dl.astype(np.float64) @ M).astype(f32)
    _, R, r, _ = sd.geometry(c)
    geo, media, tables = md.geo_of(c, "one"), md.media_of(c, "one"), md.tables_of(c, "one", "curved")
    tru = md.truth_on(o, d, geo, [axis], media, tmin, tmax, R + r)
    ok = tru["robust"]
    assert 1.0 - ok.mean() <= (md.CAP["los"] if kind == "los" else md.CAP["seg_thin"]) and ((tru["chords"][0] > 0) & ok).sum() >= md.MIN_CHORD
    sc = md.scene_of(c, "one", axis)
    w = dict(solver=solver, tmin=tmin, tmax=tmax)
    bar, far = BAR[solver], md.far_of(c, tru)
    geom = bar * far * tru["len"]
    chord = gm.chords_dev(tr, sc, o, d, **w).astype(np.float64)
    rgba = gm.glow_dev(tr, sc, o, d, media, **w).astype(np.float64)
    prof = gp.profile_dev(tr, sc, o, d, tables, 8, **w).astype(np.float64)
    want_L, want_T = pt.same_rule(tru, tables, 8)
    eps, sig = np.array(media[0][0]), media[0][1]
    pL, pT = profile_bars(tru, tables, bar, far)
    checks = {
        "chords": (np.abs(chord - tru["chords"]), 4.0 * geom[None, :] + COLOR_RTOL * tru["chords"]),
        "glow L": (np.abs(rgba[:, :3] - tru["L"]).T, (eps[None, :] * (tru["ends"] * geom)[:, None] + COLOR_RTOL * np.abs(tru["L"]) + COLOR_ATOL).T),
        "glow T": (np.abs(rgba[:, 3] - tru["T"])[None, :], (sig * tru["ends"] * geom + COLOR_RTOL)[None, :]),
        "profile L": (np.abs(prof[:, :3] - want_L).T, (pL + COLOR_RTOL * np.abs(want_L) + COLOR_ATOL).T),
        "profile T": (np.abs(prof[:, 3] - want_T)[None, :], (pT + COLOR_RTOL)[None, :]),
    }
    res = {k: ratio_of(err, b, ok[None, :]) for k, (err, b) in checks.items()}
    print(f"{sid(solver)} {kind} oriented {sd.cell_id(c)}: robust {ok.mean():.4f}; " + "; ".join(f"{k} {e:.3e} ({q:.3f})" for k, (e, q, _) in res.items())
          + f"; non-robust rays over a bar: {max(v[2] for v in res.values())} of {int((~ok).sum())}")
    assert all(q <= 1.0 for _, q, _ in res.values()), res


# ---------------------------------------------------------------------------------------------------------------------
# g. known answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("k,j", [(17, -10), (-10, 10)])
def test_the_known_answers_off_the_unit_scale(tr, k, j, solver):
    """Rays parallel to the axis through the tube, on the three tube ratios of the grid, scaled by 2^k with |d| = 2^j:
    the chord is 2a·2^k; the profile e·(1 - x)·2^(-k) with sigma 0 gives L = e·4a³/(3r²) in the unit frame at 1 and 8
    sub-steps (two Gauss points integrate the cubic exactly) and T = 1 in bits; the three moments of the weights·2^(-k) are
    weights_truth.axis_moments.  Closed forms, no solver in the truth; the bars are d's and e's.  Measured on an MI355X:
    error / bar at most 0.012 (chords, f64, r/R = 0.02), the same figures at both scalings."""
    from toroidal_ray_tracing_amd import camera
    for ratio in sd.RATIOS:
        tru, _, a = md.axis_case(ratio)
        geo, o, d, tmin, tmax, table = md.axis_scaled(ratio, k, j)
        r = tru["geo"][0][2]
        sc = abi.Scene([(geo[0][0], geo[0][1], geo[0][2], 0)], [camera.PLASTIC])
        w = dict(solver=solver, tmin=tmin, tmax=tmax)
        bar = BAR[solver]
        far = np.maximum(1.0 + r, tru["t_last"] * tru["len"]) / tru["len"]
        assert tru["robust"].all()
        chord = gm.chords_dev(tr, sc, o, d, **w).astype(np.float64)[0] * 2.0 ** -k
        err_c, bar_c = np.abs(chord - 2.0 * a), 4.0 * bar * far * tru["len"] + COLOR_RTOL * 2.0 * a
        want_L = md.AXIS_E[None, :] * (4.0 * a ** 3 / (3.0 * r * r))[:, None]
        moments = wt.axis_moments(a, r)
        unit_table = table * f32(2.0 ** k)
        worst = {"chords": float((err_c / bar_c).max())}
        for steps in md.STEPS:
            got = gp.profile_dev(tr, sc, o, d, [table], steps, **w)
            assert (u32(got[:, 3]) == u32(f32(1.0))).all()
            bar_L, _ = profile_bars(tru, [unit_table], bar, far)
            worst[f"profile {steps}"] = float((np.abs(got[:, :3].astype(np.float64) - want_L) / (bar_L + COLOR_RTOL * want_L + COLOR_ATOL)).max())
            W = gw.weights_dev(tr, sc, o, d, steps, **w)[0].astype(np.float64) * 2.0 ** -k
            worst[f"moments {steps}"] = float((np.abs(wt.moments_of(W) - moments) / gw.knot_bar(tru, solver, moments[None], far)[0]).max())
        print(f"{sid(solver)} axis rays k{k} j{j} r{ratio:g}: error / bar: " + ", ".join(f"{key} {v:.3f}" for key, v in worst.items()))
        assert all(v <= 1.0 for v in worst.values()), (ratio, worst)
