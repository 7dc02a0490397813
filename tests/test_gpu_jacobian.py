"""trt_glow_tangent[_dev] and trt_glow_adjoint[_dev]: J delta and J^T y of trt_glow_project's map with respect to all four
channels of the tables (include/trt.h).

Anchors, from the strictest down:
  1. the existing calls — an emission-only direction gives trt_glow_project of that emission (dT = +0.0f in bits), and
     channels 0..2 of the adjoint are W^T y of trt_glow_weights_absorbed_dev's own W at trt_glow_backproject's bar;
  2. the FP64 truth (tests/jacobian_truth.py: forward mode for the tangent, reverse mode for the adjoint) at the same
     step count, at derived bars (tangent_bar, adjoint_ray_bar and adjoint_sigma_bar below);
  3. <y, tangent(delta)> = <adjoint(y), delta> on the chip, at the sum of those bars;
  4. the scale identity on media_domain's cells of the single torus.
Then order, determinism, capture and replay, the windows, the layout and the refusals.  Sets are media_truth's: 4096 rays;
wherever rays are left out it is by the case's own `robust` mask, whose share is held to the case's cap.
"""
import ctypes as C
import math

import numpy as np
import pytest

import absorbed_truth as at
import crossings_truth as ct
import jacobian_truth as jt
import media_domain as md
import media_truth as mt
import project_truth as prt
import solver_domain as sd
import test_gpu_media as gm
import test_gpu_profile as gp
import test_gpu_weights_absorbed as gwa
from test_absorbed_cpu import tables_of
from test_gpu_project import backproject_dev, image_y, project_dev, u64
from test_gpu_weights_absorbed import absorbed_dev, sid, window
from toroidal_ray_tracing_amd import abi

pytestmark = pytest.mark.gpu

COLOR_RTOL, COLOR_ATOL, ROOT_BAR = gm.COLOR_RTOL, gm.COLOR_ATOL, gm.ROOT_BAR
SOLVERS, SOLVER_IDS = gm.SOLVERS, gm.SOLVER_IDS
SENTINEL, PAD = gm.SENTINEL, gm.PAD
f32, f64, u32 = np.float32, np.float64, gm.u32
STEPS = (1, 4, 64)
K = abi.TRT_PROFILE_KNOTS
EPS = 2.0 ** -24
U = 2.0 ** -53
CASES = [("single", "los"), ("rings2", "cut"), ("nest3", "seg"), ("nest8", "los")]   # 256, 256, 128 and 64 lanes a block


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def delta_of(name, seed=41, channels=(0, 1, 2, 3)):
    """A direction of mixed sign per torus, float32 (17, 4): the scene's own table times a uniform draw from (-1, 1)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in tables_of(name):
        v = np.zeros((K, 4), f32)
        v[:, channels] = (t * rng.uniform(-1.0, 1.0, (K, 4)).astype(f32))[:, channels]
        out.append(v)
    return out


def tangent_dev(tr, sc, o, d, tables, delta, steps, solver=abi.TRT_SOLVE_F32, tmin=ct.TMIN, tmax=ct.TMAX, bound=None, stats=False):
    out, st = gm._call(tr, lambda sc_, p, n, ptr, b, stream: tr.glow_tangent_dev(sc_, p, n, tables, delta, ptr, steps=steps, tmax_ptr=b,
                                                                                 tmin=tmin, tmax=tmax, stream=stream),
                       sc, o, d, solver, stats, 4 * len(o), bound)
    out = out.reshape(len(o), 4)
    return (out, st) if stats else out


def adjoint_dev(tr, sc, o, d, y, tables, steps, solver=abi.TRT_SOLVE_F32, tmin=ct.TMIN, tmax=ct.TMAX, bound=None, stats=False):
    """(n_tori, 17, 4) float64 of the _dev call, written into a sentinel-filled buffer whose pad behind is checked."""
    import torch
    yd = torch.from_numpy(np.ascontiguousarray(y, f32)).to("cuda:0") if len(o) else None
    out, st = gm._call(tr, lambda sc_, p, n, ptr, b, stream: tr.glow_adjoint_dev(sc_, p, n, yd.data_ptr() if n else 0, ptr, tables, steps=steps,
                                                                                 tmax_ptr=b, tmin=tmin, tmax=tmax, stream=stream),
                       sc, o, d, solver, stats, 2 * 4 * K * sc.n_tori, bound)
    grad = out.view(f64).reshape(sc.n_tori, K, 4)
    return (grad, st) if stats else grad


def pick(c, sel):
    """(o, d, bound) of the rays `sel` of a case."""
    return c["o"][sel], c["d"][sel], None if c["bound"] is None else c["bound"][sel]


# ---------------------------------------------------------------------------------------------------------------------
# the truth, once per (scene, kind, steps), shared by both solvers and never written
# ---------------------------------------------------------------------------------------------------------------------
_truth, _heads = {}, {}
N_AT_64 = 1024   # rays of a set that the 64-step comparisons take: the truth of 4096 rays at 64 sub-steps takes a quarter of a minute


def case_at(name, kind, steps):
    """media_truth.case(name, kind), or at 64 steps its first N_AT_64 rays (every per-ray entry cut alike): the truth's time goes
    with rays x sub-steps.  `robust_share` is the whole set's, which the cap is stated for."""
    c = mt.case(name, kind)
    if steps < 64:
        return dict(c, robust_share=c["robust"].mean())
    if (name, kind) not in _heads:
        n = len(c["o"])

        def cut(v):
            if isinstance(v, dict):
                return {k: cut(x) for k, x in v.items()}
            if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == n:
                return v[:N_AT_64]
            if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[1] == n:
                return v[:, :N_AT_64]
            return v

        _heads[name, kind] = dict(cut(dict(c)), robust_share=c["robust"].mean())
    return _heads[name, kind]


def truth(name, kind, steps):
    """dict(tan: jacobian_truth.tangent's d, abs, D, peak; adj: G3 (n_tori, 17, n) the sigma entry per ray, abs_L, peak; P (n,):
    the ray's non-empty pieces with an active torus) on delta_of(name) and image_y(n)."""
    key = (name, kind, steps)
    if key not in _truth:
        c, tables = case_at(name, kind, steps), tables_of(name)
        geo = jt.geometry(c, steps)
        tan = jt.tangent(c, tables, delta_of(name), steps, geo)
        adj = jt.adjoint(c, tables, image_y(len(c["o"])), steps, geo)
        out = dict(tan={k: tan[k] for k in ("d", "abs", "D", "peak")},
                   adj=dict(G3=np.ascontiguousarray(adj["G"][:, :, 3]), abs_L=adj["abs_L"], peak=adj["peak"]), P=at.pieces_per_torus(c)[1])
        for part in (out["tan"], out["adj"]):
            for v in part.values():
                v.setflags(write=False)
        _truth[key] = out
    return _truth[key]


def geometry_terms(c, solver):
    """(ends (n,), samples (n_tori, n)): what moved interval ends and moved samples change of an integral along the ray whose
    integrand is 1 per unit of world length — test_gpu_weights_absorbed.knot_bar's (a) and (b): every end of every torus
    is a root held to ROOT_BAR · max(1, t) and moves the total by dt · len; a sample moves with the ends and carries its
    own FP32 rounding of t, a hat has the slope 16 in x and |dx / dt| <= 2 · len / r_j, integrated over the summed chords."""
    far = np.maximum(1.0, c["t_last"])
    r = np.array([g[2] for g in c["geo"]])[:, None]
    ends = c["ends"] * ROOT_BAR[solver] * far * c["len"]
    samples = 16.0 * (2.0 * c["len"][None, :] / r) * (ROOT_BAR[solver] + 2.0 ** -23) * far[None, :] * c["chords"].sum(0)[None, :]
    return ends, samples


def tangent_bar(c, tables, solver, steps, t):
    """(n, 4), built as knot_bar is.  For a colour:
      (a) + (b) the moved ends and the moved samples of geometry_terms, times the ray's largest integrand per unit of length
          (truth: peak, which is taken per unit of the transmittance in front as well, so it bounds the integrand).  The
          integrand is a combination of hats whose coefficients differ by at most twice the largest, so (b) counts twice;
          the samples of every torus the ray runs through move: (b) summed over the tori;
      (c) chords · bar_T · peak: the transmittance in front is off by at most gp.bars' bar on T for the same tables, and
          peak is the integrand per unit of T;
      (d) the roundings of the walk, counted, times the truth's sum of the absolute terms: per sub-step one fma into L_c,
          five for the running T (its product and the four units of E's exp2 polynomial) and two for the running D — 8 per
          sub-step, steps · P sub-steps — and per term the two lookups (three operations per torus and point, the
          average: 6 · n_tori + 2), tau, E (4), w (8: its series), w' (14: its series, or the quotient at 2.8 · 3), and six
          products and fma: (8 · steps · P + 6 · n_tori + 40) · 2^-24;
      (e) COLOR_RTOL · |want| + COLOR_ATOL.
    For dT = -T · D: bar_T · D, (a) + (b) times the largest |dsg|, and (d), (e) alike."""
    ends, samples = geometry_terms(c, solver)
    bar_T = gp.bars(c, tables, solver)[1]
    count = (8 * steps * t["P"] + 6 * len(tables) + 40) * EPS
    geo = ends + 2.0 * samples.sum(0)
    tan = t["tan"]
    colour = (geo + c["chords"].sum(0) * bar_T)[:, None] * tan["peak"][:, :3]
    trans = bar_T * tan["D"] + geo * tan["peak"][:, 3]
    return np.concatenate([colour, trans[:, None]], 1) + count[:, None] * tan["abs"] + COLOR_RTOL * np.abs(tan["d"]) + COLOR_ATOL


def adjoint_ray_bar(c, tables, solver, steps, t):
    """(n_tori, 17, n): the bar on G_i[j][k] = sum_s lambda_s · hat_s[j][k] of one ray, |y| inside: knot_bar with the ray's
    largest |lambda| per unit of length and of T in front (truth: peak) as the integrand's size —
    (all ends + twice torus j's moved samples over the summed chords + chord_j · bar_T) · peak — plus the counted
    roundings times the truth's absolute sum WITH L_c IN PLACE OF B_c (abs_L: the walk forms B = L_c - prefix, which
    rounds relative to L_c): per sub-step two fma into an accumulator, twelve for L_c and the prefix (six each: the fma,
    and T's five), five for T in front; per term the lookups (6 · n_tori + 2), tau, E, w, w' (27), lambda's eleven
    products and fma, g and 1 - f: (20 · steps · P + 6 · n_tori + 48) · 2^-24; plus COLOR_RTOL · |G_i| + COLOR_ATOL."""
    ends, samples = geometry_terms(c, solver)
    bar_T = gp.bars(c, tables, solver)[1]
    count = (20 * steps * t["P"] + 6 * len(tables) + 48) * EPS
    adj = t["adj"]
    geo = ends[None, :] + 2.0 * samples + c["chords"] * bar_T[None, :]
    return (geo * adj["peak"][None, :])[:, None, :] + count[None, None, :] * adj["abs_L"] + COLOR_RTOL * np.abs(adj["G3"]) + COLOR_ATOL


def adjoint_sigma_bar(c, tables, solver, steps, t, ok):
    """(n_tori, 17): the sum over the rays `ok` of the per-ray bars, plus n · 2^-53 · sum |G_i| for the FP64 sum of any order."""
    per_ray = adjoint_ray_bar(c, tables, solver, steps, t)[:, :, ok]
    return per_ray.sum(-1) + ok.sum() * U * np.abs(t["adj"]["G3"][:, :, ok]).sum(-1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the existing calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name,kind", CASES)
def test_an_emission_only_direction_is_glow_project(tr, name, kind, solver):
    """delta >= 0 with no sigma entry: dT is +0.0f in bits, and dL is trt_glow_project's L on (delta's emission, profiles'
    sigma) within test_gpu_weights_absorbed's counted forward bar, (2 · steps · P + 2 · n_tori + 24) · 2^-24 · sum_j S_j · top_jc
    with S_j the summed weights of torus j and top_jc the largest knot of delta: the tangent's sub-step is
    trt_glow_profile's there (the sigma terms are zeros), and trt_glow_project sums the same products otherwise.
    Measured on an MI355X: 0.095 of the bar at the most."""
    c = mt.case(name, kind)
    sc, tables = gm.scene_of(name), tables_of(name)
    delta = [np.abs(v) for v in delta_of(name, channels=(0, 1, 2))]
    mixed = [np.concatenate([v[:, :3], t[:, 3:]], 1) for t, v in zip(tables, delta)]
    P = at.pieces_per_torus(c)[1]
    top = np.array([v.astype(f64).max(0)[:3] for v in delta])
    for steps in STEPS:
        got = tangent_dev(tr, sc, c["o"], c["d"], tables, delta, steps, **window(c, solver))
        want = project_dev(tr, sc, c["o"], c["d"], mixed, steps, **window(c, solver))
        W, _ = absorbed_dev(tr, sc, c["o"], c["d"], tables, steps, **window(c, solver))
        assert (u32(got[:, 3]) == 0).all(), steps
        err = np.abs(got[:, :3].astype(f64) - want[:, :3].astype(f64))
        bar = ((2 * steps * P + 2 * sc.n_tori + 24) * EPS)[:, None] * np.einsum("jn,jc->nc", W.astype(f64).sum(1), top)
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"{name} {kind} {steps} steps {sid(solver)}: largest error / bar {np.nanmax(np.where(bar > 0, err / bar, 0.0)):.3f}")
        assert (err <= bar).all(), (steps, np.nanmax(err / np.where(bar > 0, bar, 1.0)))
    assert (want[:, :3].max(1) > 1e-3).mean() > 0.05


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name,kind", CASES)
def test_the_emission_channels_of_the_adjoint_are_backproject(tr, name, kind, solver):
    """Channels 0..2 against project_truth.backproject_exact on trt_glow_weights_absorbed_dev's own W, within backproject_bar;
    0.0 in bits where there is no term, and trt_glow_backproject_dev's own bits.  4096 rays at 1 and 4 steps, then 1, 63, 65 and
    1000 rays.  Measured on an MI355X: 0.043 of the bar at the most (`nest3`, 65 rays)."""
    c = mt.case(name, kind)
    sc, tables = gm.scene_of(name), tables_of(name)
    y_all = image_y(len(c["o"]))
    for steps, n in ((1, 4096), (4, 4096), (4, 1), (4, 63), (4, 65), (4, 1000)):
        s = slice(200, 200 + n) if n < 4096 else slice(None)
        o, d, y = c["o"][s], c["d"][s], y_all[s]
        w = dict(solver=solver, tmin=c["tmin"], tmax=c["tmax"], bound=None if c["bound"] is None else c["bound"][s])
        W, _ = absorbed_dev(tr, sc, o, d, tables, steps, **w)
        grad = adjoint_dev(tr, sc, o, d, y, tables, steps, **w)
        exact, bar = prt.backproject_exact(W, y)[:, :, :3], prt.backproject_bar(W, y)[:, :, :3]
        err = np.abs(grad[:, :, :3] - exact)
        print(f"{name} {kind} {steps} steps {sid(solver)} n {n}: largest error / bar "
              f"{float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0))):.4f}")
        assert (err <= bar).all(), (steps, n)
        assert (u64(grad[:, :, :3])[bar == 0] == 0).all(), (steps, n)
        assert np.array_equal(u64(grad[:, :, :3]), u64(backproject_dev(tr, sc, o, d, y, tables, steps, **w)[:, :, :3])), (steps, n)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the FP64 truth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", mt.NAMES)
def test_the_tangent_against_forward_mode_in_fp64(tr, name, kind, steps, solver):
    """Against jacobian_truth.tangent at the same step count on the `robust` rays, at tangent_bar.  The largest error / bar
    per case is printed.  Measured on an MI355X over the 72 cases: 0.070 of the bar at the most for a colour (`rings2`, lines
    of sight, 1 step, f32: 2.3e-5 absolute), 0.033 for dT (profiles/r31_glow_jacobian.txt)."""
    c = case_at(name, kind, steps)
    tables, t = tables_of(name), truth(name, kind, steps)
    got = tangent_dev(tr, gm.scene_of(name), c["o"], c["d"], tables, delta_of(name), steps, **window(c, solver))
    ok = c["robust"]
    assert 1.0 - c["robust_share"] <= c["cap"]
    err, bar = np.abs(got.astype(f64) - t["tan"]["d"]), tangent_bar(c, tables, solver, steps, t)
    ratio = (err / bar)[ok]
    print(f"{name} {kind} {steps} steps {sid(solver)}: robust {ok.mean():.4f}; tangent: largest error {err[ok][:, :3].max():.3e} (dT {err[ok][:, 3].max():.3e}), "
          f"largest error / bar {ratio[:, :3].max():.3f} (dT {ratio[:, 3].max():.3f})")
    assert (ratio <= 1.0).all(), ratio.max()
    assert (np.abs(t["tan"]["d"][ok][:, :3]).max(1) > 1e-4).mean() > 0.1 and (np.abs(t["tan"]["d"][ok][:, 3]) > 1e-4).mean() > 0.1


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", mt.NAMES)
def test_the_sigma_gradient_against_reverse_mode_in_fp64(tr, name, kind, steps, solver):
    """The call on the `robust` rays alone (a ragged n) against the sum of jacobian_truth.adjoint's per-ray G over them, at
    adjoint_sigma_bar.  The largest error / bar per case is printed.  Measured on an MI355X over the 72 cases: under 0.0005 of
    the bar everywhere, the largest error 4.5e-5 of the largest entry — the bar adds the per-ray bars linearly and is loose by
    that much; test_the_sigma_gradient_of_single_rays holds single rays (profiles/r31_glow_jacobian.txt)."""
    c = case_at(name, kind, steps)
    tables, t = tables_of(name), truth(name, kind, steps)
    ok = c["robust"]
    assert 1.0 - c["robust_share"] <= c["cap"]
    o, d, bound = pick(c, ok)
    grad = adjoint_dev(tr, gm.scene_of(name), o, d, image_y(len(c["o"]))[ok], tables, steps, solver=solver, tmin=c["tmin"], tmax=c["tmax"], bound=bound)
    want = t["adj"]["G3"][:, :, ok].sum(-1)
    err, bar = np.abs(grad[:, :, 3] - want), adjoint_sigma_bar(c, tables, solver, steps, t, ok)
    print(f"{name} {kind} {steps} steps {sid(solver)}: n {int(ok.sum())}; sigma gradient: largest error {err.max():.3e} of {np.abs(want).max():.3e}, "
          f"largest error / bar {(err / bar).max():.3f}")
    assert (err <= bar).all(), (err / bar).max()
    assert (np.abs(want) > 1e-2).mean() > 0.5


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name,kind", CASES)
def test_the_sigma_gradient_of_single_rays(tr, name, kind, solver):
    """The sum over the rays hides a ray: its bar is the sum of the per-ray bars, thousands of times a single one.  A call
    with ONE ray returns G_i itself (the FP64 sum of one value is that value): 40 robust rays spread over the set, each held
    to adjoint_ray_bar alone, at 4 steps.  Measured on an MI355X: 0.002 of the bar at the most."""
    steps = 4
    c = mt.case(name, kind)
    sc, tables, t = gm.scene_of(name), tables_of(name), truth(name, kind, steps)
    y = image_y(len(c["o"]))
    seen = np.nonzero(c["robust"] & (np.abs(t["adj"]["G3"]).max((0, 1)) > 1e-3))[0]
    rays = seen[np.linspace(0, len(seen) - 1, 40).astype(int)]
    bar = adjoint_ray_bar(c, tables, solver, steps, t)
    worst = 0.0
    for i in rays:
        s = slice(i, i + 1)
        grad = adjoint_dev(tr, sc, c["o"][s], c["d"][s], y[s], tables, steps, solver=solver, tmin=c["tmin"], tmax=c["tmax"],
                           bound=None if c["bound"] is None else c["bound"][s])
        ratio = np.abs(grad[:, :, 3] - t["adj"]["G3"][:, :, i]) / bar[:, :, i]
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (int(i), float(ratio.max()))
    print(f"{name} {kind} {steps} steps {sid(solver)}: sigma gradient of single rays: largest error / bar {worst:.3f}")
    assert len(set(rays.tolist())) >= 30


# ---------------------------------------------------------------------------------------------------------------------
# 3. the two are adjoint on the chip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name,kind", CASES)
def test_tangent_and_adjoint_are_adjoint_on_the_chip(tr, name, kind, solver):
    """<y, tangent(delta)> against <adjoint(y), delta> on the `robust` rays at 4 steps, both summed exactly (math.fsum), within
    sum_i |y_i| · bar_tangent_i + sum_jk |delta_jk| · bar_adjoint_jk: the truth's two modes are adjoint to FP64 rounding
    (tests/test_jacobian_cpu.py), and each call is within its bar of its truth.  The bar of an emission entry of the
    adjoint is the sum over the rays of |y_ic| times test_gpu_weights_absorbed.knot_bar of W[j][k][i], plus n · 2^-53 · sum |W y|."""
    steps = 4
    c = case_at(name, kind, steps)
    sc, tables, delta, t = gm.scene_of(name), tables_of(name), delta_of(name), truth(name, kind, steps)
    ok = c["robust"]
    assert 1.0 - c["robust_share"] <= c["cap"]
    o, d, bound = pick(c, ok)
    y = image_y(len(c["o"]))[ok]
    w = dict(solver=solver, tmin=c["tmin"], tmax=c["tmax"], bound=bound)
    tan = tangent_dev(tr, sc, o, d, tables, delta, steps, **w)
    grad = adjoint_dev(tr, sc, o, d, y, tables, steps, **w)
    lhs = math.fsum((y.astype(f64) * tan.astype(f64)).ravel().tolist())
    rhs = math.fsum((grad * np.stack(delta).astype(f64)).ravel().tolist())
    want_W, _ = gwa.same_rule(name, kind, steps)
    bar_T = gp.bars(c, tables, solver)[1]
    w_bar = gwa.knot_bar(c, solver, want_W, bar_T)[:, :, ok]                                   # (n_tori, 17, n)
    ay = np.abs(y.astype(f64))
    bar_e = np.einsum("jkn,nc->jkc", w_bar, ay[:, :3]) + ok.sum() * U * np.einsum("jkn,nc->jkc", want_W[:, :, ok], ay[:, :3])
    bar_adj = np.concatenate([bar_e, adjoint_sigma_bar(c, tables, solver, steps, t, ok)[:, :, None]], 2)
    bar = (ay * tangent_bar(c, tables, solver, steps, t)[ok]).sum() + (np.abs(np.stack(delta).astype(f64)) * bar_adj).sum()
    print(f"{name} {kind} {sid(solver)}: <y, J d> = {lhs:.9e}, <J^T y, d> = {rhs:.9e}, difference / bar {abs(lhs - rhs) / bar:.4f}")
    assert abs(lhs - rhs) <= bar
    assert abs(lhs) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 4. scale
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind", md.KINDS)
def test_every_cell_is_its_unit_cell_scaled_bit_for_bit(tr, kind, solver):
    """media_domain's cells of the single torus: geometry times 2^k, directions times 2^j, tables and delta times 2^-k.  The
    walk scales by products with powers of two and its thresholds act on tau alone, so the tangent is the unit cell's bit
    for bit, and the adjoint — a derivative with respect to knots that carry 2^-k, summed in FP64 from per-ray values that
    scale exactly — is the unit cell's times 2^k bit for bit in all four channels; y is the unit cell's."""
    steps, shape = 8, "curved"
    base, lines, bad = {}, [], []
    cells = sorted(md.cells(kind), key=lambda c: not (c.k == 0 and c.j == 0))   # the unit cells first
    for c in cells:
        u = sd.unit_of(c)
        o, d, tmin, tmax = md.rays(c, kind)
        tables = md.tables_of(c, "one", shape)
        rng = np.random.default_rng(43)
        delta = [(t * rng.uniform(-1.0, 1.0, (K, 4)).astype(f32)).astype(f32) for t in md.tables_of(u, "one", shape)]
        delta = [v * f32(2.0 ** -c.k) for v in delta]
        y = image_y(len(o))
        w = dict(solver=solver, tmin=tmin, tmax=tmax)
        sc = md.scene_of(c, "one")
        tan = tangent_dev(tr, sc, o, d, tables, delta, steps, **w)
        grad = adjoint_dev(tr, sc, o, d, y, tables, steps, **w)
        grad = grad * 2.0 ** -c.k
        if c == u:
            base[u] = (tan, grad)
            assert (np.abs(tan).max(1) > 1e-4).mean() > 0.1
            continue
        bt, bg = base[u]
        n_t, n_g = int((u32(tan) != u32(bt)).any(1).sum()), int((u64(grad) != u64(bg)).sum())
        lines.append(f"{sid(solver)} {kind} {sd.cell_id(c)}: tangent rays that differ from the unit cell in bits {n_t}, adjoint entries {n_g}")
        if n_t or n_g:
            bad.append((sd.cell_id(c), n_t, n_g))
    print("\n".join(lines))
    assert not bad, bad[:10]
    assert len(lines) == len(cells) - len(md.unit_cells(kind))


# ---------------------------------------------------------------------------------------------------------------------
# order and determinism
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name,kind", CASES)
def test_the_tangent_does_not_depend_on_the_order_of_the_rays(tr, name, kind, solver):
    c = mt.case(name, kind)
    sc, n, tables, delta = gm.scene_of(name), len(c["o"]), tables_of(name), delta_of(name)
    w = dict(solver=solver, tmin=c["tmin"], tmax=c["tmax"])
    got = tangent_dev(tr, sc, c["o"], c["d"], tables, delta, 4, bound=c["bound"], **w)
    perm = np.random.default_rng(11).permutation(n)[:n - 37]   # (ragged)
    pb = None if c["bound"] is None else c["bound"][perm]
    assert np.array_equal(u32(tangent_dev(tr, sc, c["o"][perm], c["d"][perm], tables, delta, 4, bound=pb, **w)), u32(got[perm]))
    assert len(np.unique(u32(got), axis=0)) > 1000


@pytest.mark.parametrize("name,kind", CASES)
def test_the_adjoint_gives_the_same_bits_from_every_call(tr, name, kind):
    c = mt.case(name, kind)
    sc, tables, y = gm.scene_of(name), tables_of(name), image_y(len(c["o"]))
    first = adjoint_dev(tr, sc, c["o"], c["d"], y, tables, 4, **window(c))
    other = adjoint_dev(tr, gm.scene_of("single"), c["o"][:300], c["d"][:300], y[:300], tables_of("single"), 2)   # (the scratch is shared)
    assert (other != 0).any()
    for _ in range(2):
        assert np.array_equal(u64(first), u64(adjoint_dev(tr, sc, c["o"], c["d"], y, tables, 4, **window(c))))
    assert len(np.unique(u64(first))) > 10 * sc.n_tori


def test_capture_and_replay(tr):
    """Both _dev calls captured on a side stream into one graph, behind eager calls that have sized the context's scratch.
    Each replay gives the eager bits, with an eager call of another scene — another block width, the same scratch — in
    between.  A context whose scratch is too small for the captured call refuses it."""
    import torch
    from toroidal_ray_tracing_amd.tracer import Tracer, TrtError
    c = mt.case("nest3", "seg")
    sc, w, tables, delta = gm.scene_of("nest3"), dict(tmin=c["tmin"], tmax=c["tmax"]), tables_of("nest3"), delta_of("nest3")
    n = 256 * 5 + 33
    o, d, y = c["o"][:n], c["d"][:n], image_y(n)
    bound = np.linspace(0.3, 1.5, n).astype(f32)
    eager_tan = tangent_dev(tr, sc, o, d, tables, delta, 3, bound=bound, **w)
    eager_grad = adjoint_dev(tr, sc, o, d, y, tables, 3, bound=bound, **w)
    keep, ptrs = gm.upload(o, d)
    b, yd = torch.from_numpy(bound).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    n_grad = 2 * 4 * K * sc.n_tori
    rgba, grad = gm.image(4 * n), gm.image(n_grad)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            tr.glow_tangent_dev(sc, ptrs, n, tables, delta, rgba.data_ptr(), steps=3, tmax_ptr=b.data_ptr(), stream=side.cuda_stream, **w)
            tr.glow_adjoint_dev(sc, ptrs, n, yd.data_ptr(), grad.data_ptr(), tables, steps=3, tmax_ptr=b.data_ptr(), stream=side.cuda_stream, **w)
    cur.wait_stream(side)
    s = mt.case("single", "los")
    for k in range(2):
        rgba.fill_(SENTINEL)
        grad.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u32(gm.read(rgba, 4 * n).reshape(n, 4)), u32(eager_tan)), k
        assert np.array_equal(gm.read(grad, n_grad).view(np.uint64), u64(eager_grad).ravel()), k
        other = adjoint_dev(tr, gm.scene_of("single"), s["o"][:500], s["d"][:500], image_y(500), tables_of("single"), 7)   # 256 lanes
        assert (other != 0).any()
        assert (tangent_dev(tr, gm.scene_of("single"), s["o"][:500], s["d"][:500], tables_of("single"), delta_of("single"), 7) != 0).any()
    assert len(np.unique(u64(eager_grad))) > 50
    # a ctx sized by a smaller eager call: the capture would have to grow the scratch and is refused
    t2 = Tracer(0)
    try:
        small = t2.glow_adjoint(sc, o[:64], d[:64], y[:64], tables, steps=3, **w)
        assert (small != 0).any()
        gx = torch.cuda.CUDAGraph()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            with torch.cuda.graph(gx, stream=side):
                with pytest.raises(TrtError) as e:
                    t2.glow_adjoint_dev(sc, ptrs, n, yd.data_ptr(), grad.data_ptr(), tables, steps=3, stream=side.cuda_stream, **w)
                assert e.value.code == abi.TRT_E_INVALID and "captured" in str(e.value)
                with pytest.raises(TrtError) as e:   # the tangent's area has never been allocated in this ctx
                    t2.glow_tangent_dev(sc, ptrs, n, tables, delta, rgba.data_ptr(), steps=3, stream=side.cuda_stream, **w)
                assert e.value.code == abi.TRT_E_INVALID and "captured" in str(e.value)
                torch.zeros(1, device="cuda:0")   # keep the capture non-empty
        cur.wait_stream(side)
    finally:
        t2.close()


# ---------------------------------------------------------------------------------------------------------------------
# windows, layout, the host forms, an oriented torus
# ---------------------------------------------------------------------------------------------------------------------
def test_layout_windows_and_the_host_forms(tr):
    import torch
    c = mt.case("nest3", "cut")
    sc, o, d, tables, delta = gm.scene_of("nest3"), c["o"], c["d"], tables_of("nest3"), delta_of("nest3")
    n, n_grad = len(o), 4 * K * sc.n_tori
    w, y = dict(tmin=c["tmin"], tmax=c["tmax"]), image_y(len(o))
    # both outputs in the middle of sentinel-filled buffers: pads in front and behind
    keep, ptrs = gm.upload(o, d)
    b, yd = torch.from_numpy(np.array(c["bound"], f32)).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    rbuf = torch.full((PAD + 4 * n + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    gbuf = torch.full((PAD + 2 * n_grad + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    tr.glow_tangent_dev(sc, ptrs, n, tables, delta, rbuf.data_ptr() + 4 * PAD, steps=4, tmax_ptr=b.data_ptr(), **w)
    tr.glow_adjoint_dev(sc, ptrs, n, yd.data_ptr(), gbuf.data_ptr() + 4 * PAD, tables, steps=4, tmax_ptr=b.data_ptr(), **w)
    torch.cuda.synchronize()
    rraw, graw = rbuf.cpu().numpy(), gbuf.cpu().numpy()
    for raw, m in ((rraw, 4 * n), (graw, 2 * n_grad)):
        assert (raw[:PAD] == f32(SENTINEL)).all() and (raw[PAD + m:] == f32(SENTINEL)).all()
    tan, grad = rraw[PAD:PAD + 4 * n].reshape(n, 4), graw[PAD:PAD + 2 * n_grad].copy().view(f64).reshape(sc.n_tori, K, 4)
    assert np.array_equal(u32(tan), u32(tangent_dev(tr, sc, o, d, tables, delta, 4, bound=c["bound"], **w)))
    assert np.array_equal(u64(grad), u64(adjoint_dev(tr, sc, o, d, y, tables, 4, bound=c["bound"], **w)))
    # the empty windows of the set (a bound at tmin, below it, NaN, -inf): (0, 0, 0, 0) — the fourth entry is a derivative —
    # no term in the sums whatever y holds there, no test
    empty = ~c["info"]["nonempty"]
    assert empty.sum() == (n + 4) // 5 and np.isnan(c["bound"][empty]).any()
    assert (u32(tan[empty]) == 0).all() and (tan[~empty, 3] != 0).any()
    loud = np.array(y)
    loud[empty] = 1e30
    assert np.array_equal(u64(adjoint_dev(tr, sc, o, d, loud, tables, 4, bound=c["bound"], **w)), u64(grad))
    for call in (lambda **kw: tangent_dev(tr, sc, o, d, tables, delta, 4, **kw), lambda **kw: adjoint_dev(tr, sc, o, d, y, tables, 4, **kw)):
        out, st = call(bound=c["bound"], stats=True, **w)
        assert st["primary_tests"] == 3 * (n - empty.sum()) == st["traced_tests"] and st["pixels"] == n
        out, st = call(tmax=-1.0, stats=True)
        assert st["primary_tests"] == st["traced_tests"] == 0
        assert (u64(out) == 0).all() if out.dtype == f64 else (u32(out) == 0).all()
    # channel 3 of y IS read: clearing it changes the sigma entries and nothing else
    flat = np.array(y)
    flat[:, 3] = 0.0
    other = adjoint_dev(tr, sc, o, d, flat, tables, 4, bound=c["bound"], **w)
    assert np.array_equal(u64(other[:, :, :3]), u64(grad[:, :, :3])) and (other[:, :, 3] != grad[:, :, 3]).mean() > 0.9
    # with y >= 0 every sigma entry is <= 0
    assert (adjoint_dev(tr, sc, o, d, np.abs(y), tables, 4, bound=c["bound"], **w)[:, :, 3] < 0).all()
    # a negative delta is accepted, and the tangent is odd in delta: every operation of the walk is (zeros compare equal)
    neg = tangent_dev(tr, sc, o, d, tables, [-v for v in delta], 4, bound=c["bound"], **w)
    assert np.array_equal(neg, -tan) and (tan[:, :3] < 0).any() and (tan[:, :3] > 0).any()
    # n == 0: the adjoint writes zeros, the tangent nothing
    z = np.zeros((0, 3), f32)
    assert (u64(adjoint_dev(tr, sc, z, z, np.zeros((0, 4), f32), tables, 4)) == 0).all()
    assert tangent_dev(tr, sc, z, z, tables, delta, 4).shape == (0, 4)
    assert tr.glow_tangent(sc, z, z, tables, delta).shape == (0, 4)
    grad0 = tr.glow_adjoint(sc, z, z, np.zeros((0, 4), f32), tables)
    assert grad0.shape == (sc.n_tori, K, 4) and (u64(grad0) == 0).all()
    # the host forms
    host_tan = tr.glow_tangent(sc, o, d, tables, delta, steps=4, tmax_per_ray=c["bound"], **w)
    host_grad = tr.glow_adjoint(sc, o, d, y, tables, steps=4, tmax_per_ray=c["bound"], **w)
    assert host_tan.shape == (n, 4) and host_tan.dtype == f32 and np.array_equal(u32(host_tan), u32(tan))
    assert host_grad.shape == (sc.n_tori, K, 4) and host_grad.dtype == f64 and np.array_equal(u64(host_grad), u64(grad))


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
def test_an_oriented_torus(tr, solver):
    """`rings2` has a tilted ring: its cases above run the ORIENT kernels.  Here the tilted ring alone, against the truth."""
    geo, axes = ct.SCENES["rings2"]
    j = next(k for k, a in enumerate(axes) if a is not None and tuple(a) != (0.0, 1.0, 0.0))
    c = mt.case("rings2", "los")
    sc = gm.scene_of("rings2", only=[j])
    tables, delta = [tables_of("rings2")[j]], [delta_of("rings2")[j]]
    tru = mt.truth_of(c["o"], c["d"], [geo[j]], [axes[j]], [mt.MEDIA["rings2"][j]], c["tmin"], c["tmax"])
    tru.update(o=c["o"], d=c["d"], geo=[geo[j]], axes=[axes[j]])
    steps = 4
    g = jt.geometry(tru, steps)
    y = image_y(len(c["o"]))
    t = dict(tan=jt.tangent(tru, tables, delta, steps, g), P=at.pieces_per_torus(tru)[1])
    adj = jt.adjoint(tru, tables, y, steps, g)
    t["adj"] = dict(G3=adj["G"][:, :, 3], abs_L=adj["abs_L"], peak=adj["peak"])
    ok = tru["robust"]
    got = tangent_dev(tr, sc, c["o"], c["d"], tables, delta, steps, solver, c["tmin"], c["tmax"])
    ratio = (np.abs(got.astype(f64) - t["tan"]["d"]) / tangent_bar(tru, tables, solver, steps, t))[ok]
    grad = adjoint_dev(tr, sc, c["o"][ok], c["d"][ok], y[ok], tables, steps, solver, c["tmin"], c["tmax"])
    err, bar = np.abs(grad[:, :, 3] - t["adj"]["G3"][:, :, ok].sum(-1)), adjoint_sigma_bar(tru, tables, solver, steps, t, ok)
    print(f"tilted ring {sid(solver)}: robust {ok.mean():.4f}; tangent error / bar {ratio.max():.3f}, sigma gradient error / bar {(err / bar).max():.3f}")
    assert ok.mean() > 0.9 and (ratio <= 1.0).all() and (err <= bar).all()
    assert (np.abs(t["tan"]["d"][ok]).max(1) > 1e-4).mean() > 0.1


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable_and_the_outputs_unwritten(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    c = mt.case("rings2", "seg")
    sc, w, tables, delta = gm.scene_of("rings2"), dict(tmin=c["tmin"], tmax=c["tmax"]), tables_of("rings2"), delta_of("rings2")
    n = 300
    o, d, y = c["o"][:n], c["d"][:n], image_y(n)
    want_tan, want_grad = tangent_dev(tr, sc, o, d, tables, delta, 4, **w), adjoint_dev(tr, sc, o, d, y, tables, 4, **w)
    keep, ptrs = gm.upload(o, d)
    yd = torch.from_numpy(y).to("cuda:0")
    n_grad = 2 * 4 * K * sc.n_tori
    rgba, grad = gm.image(4 * n), gm.image(n_grad)
    L = tr._L
    rays = abi.rays_struct(ptrs, n)
    prof, dprof = abi.profiles(tables), abi.profiles(delta)
    scp = C.byref(sc.c)

    def good():
        assert np.array_equal(u32(tangent_dev(tr, sc, o, d, tables, delta, 4, **w)), u32(want_tan))
        assert np.array_equal(u64(adjoint_dev(tr, sc, o, d, y, tables, 4, **w)), u64(want_grad))

    def refused(who, call, *needles):
        with pytest.raises(TrtError) as e:
            call()
        assert e.value.code == abi.TRT_E_INVALID, str(e.value)
        for needle in (who,) + needles:
            assert needle in str(e.value), str(e.value)
        good()

    fwd = lambda tabs=tables, dl=delta, p=ptrs, out=None, **kw: tr.glow_tangent_dev(sc, p, n, tabs, dl, rgba.data_ptr() if out is None else out,
                                                                                    **dict(w, **kw))
    bwd = lambda tabs=tables, p=ptrs, yp=None, out=None, **kw: tr.glow_adjoint_dev(sc, p, n, yd.data_ptr() if yp is None else yp,
                                                                                   grad.data_ptr() if out is None else out, tabs, **dict(w, **kw))
    good()
    for who, call in (("trt_glow_tangent", fwd), ("trt_glow_adjoint", bwd)):
        refused(who, lambda: call(out=0), "NULL output")
        refused(who, lambda: call(p=ptrs[:2] + [0] + ptrs[3:]), "NULL ray stream")
        refused(who, lambda: call(out=(rgba if call is fwd else grad).data_ptr() + 4), "16-byte aligned")
        for steps in (0, abi.TRT_MAX_GLOW_STEPS + 1):
            refused(who, lambda: call(steps=steps), "steps", "TRT_MAX_GLOW_STEPS")
        # NULL profiles: refused by both — the emission enters the sigma gradient
        refused(who, lambda: call(tabs=None), "NULL profiles")
        # a negative sigma knot and a negative emission knot of the profiles: both calls read all four channels
        broken = [np.array(t) for t in tables]
        broken[1][7, 3] = -0.5
        refused(who, lambda: call(tabs=broken), "torus 1", "knot 7", "sigma")
        dim = [np.array(t) for t in tables]
        dim[0][9, 1] = -0.25
        refused(who, lambda: call(tabs=dim), "torus 0", "knot 9", "emission")
        for solver in (abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_FERRARI_F64):
            tr.set_solver(solver)
            try:
                with pytest.raises(TrtError) as e:
                    call()
                assert e.value.code == abi.TRT_E_INVALID and who in str(e.value), str(e.value)
                assert "the enumeration runs the default solver (TRT_SOLVE_F32 / _F64) only" in str(e.value)
            finally:
                tr.set_solver(abi.TRT_SOLVE_F32)
            good()
    # NULL rays, NULL scene (raw calls)
    rp, gp_, yp = C.c_void_p(rgba.data_ptr()), C.c_void_p(grad.data_ptr()), C.c_void_p(yd.data_ptr())
    for call, who in ((lambda: L.trt_glow_tangent_dev(tr._h, None, None, scp, prof, dprof, 4, 0.001, 1.0, rp, None), b"trt_glow_tangent"),
                      (lambda: L.trt_glow_adjoint_dev(tr._h, None, None, scp, prof, 4, 0.001, 1.0, yp, gp_, None), b"trt_glow_adjoint"),
                      (lambda: L.trt_glow_tangent_dev(tr._h, C.byref(rays), None, None, prof, dprof, 4, 0.001, 1.0, rp, None), b"scene"),
                      (lambda: L.trt_glow_adjoint_dev(tr._h, C.byref(rays), None, None, prof, 4, 0.001, 1.0, yp, gp_, None), b"scene")):
        assert call() == abi.TRT_E_INVALID and who in L.trt_last_error(tr._h)
        good()
    # tangent only: NULL delta, a delta entry that is not finite (a negative one is accepted)
    refused("trt_glow_tangent", lambda: fwd(dl=None), "NULL delta")
    for j, k, ch, v in ((0, 3, 0, np.nan), (1, 16, 3, np.inf), (1, 0, 2, -np.inf)):
        odd = [np.array(v_) for v_ in delta]
        odd[j][k, ch] = v
        refused("trt_glow_tangent", lambda: fwd(dl=odd), f"torus {j}", f"knot {k}", "finite")
    # adjoint only: NULL y, a misaligned y
    refused("trt_glow_adjoint", lambda: bwd(yp=0), "NULL y")
    refused("trt_glow_adjoint", lambda: bwd(yp=yd.data_ptr() + 4), "16-byte aligned")
    torch.cuda.synchronize()
    assert (rgba.cpu().numpy() == f32(SENTINEL)).all() and (grad.cpu().numpy() == f32(SENTINEL)).all()   # a refused call writes nothing
    assert L.trt_glow_tangent_dev(None, C.byref(rays), None, scp, prof, dprof, 4, 0.001, 1.0, rp, None) == abi.TRT_E_INVALID
    assert L.trt_glow_adjoint_dev(None, C.byref(rays), None, scp, prof, 4, 0.001, 1.0, yp, gp_, None) == abi.TRT_E_INVALID
    good()
