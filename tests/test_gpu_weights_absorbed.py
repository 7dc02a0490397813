"""trt_glow_weights_absorbed[_dev]: the response of every line of sight to every emission knot behind media that absorb
(include/trt.h).

Anchors, from the strictest down:
  1. no absorption — where no tubes overlap the weights are trt_glow_weights' bit for bit and trans is 1.0f; where they
     do, the weights of a torus still sum to its chord;
  2. trt_glow_profile — trans is its T bit for bit;
  3. trt_glow_profile — sum_jk W[j][k] · knot_j[k][c] is its L_c, at a bar counted from the roundings;
  4. the FP64 restatement of the rule (tests/absorbed_truth.py: same_rule) at the same step count, at derived bars;
  5. the known answer: a ray parallel to the axis through a flat sigma.
Then order and layout (the three block widths among them), the windows, capture and replay, and the refusals.  Sets are
media_truth's: 4096 rays.
"""
import ctypes as C

import numpy as np
import pytest

import absorbed_truth as at
import crossings_truth as ct
import media_truth as mt
import profile_truth as pt
import test_gpu_media as gm
import test_gpu_profile as gp
import test_gpu_weights as gw
import weights_truth as wt
from test_absorbed_cpu import KNOWN_SIGMA, tables_of
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

COLOR_RTOL, COLOR_ATOL, ROOT_BAR = gm.COLOR_RTOL, gm.COLOR_ATOL, gm.ROOT_BAR
SOLVERS, SOLVER_IDS = gm.SOLVERS, gm.SOLVER_IDS
SENTINEL, PAD = gm.SENTINEL, gm.PAD
f32, u32 = np.float32, gm.u32
STEPS = (1, 4, 64)
K = abi.TRT_PROFILE_KNOTS
EPS = 2.0 ** -24
ONE = u32(f32(1.0))


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def sid(solver):
    return SOLVER_IDS[SOLVERS.index(solver)]


def absorbed_dev(tr, sc, o, d, tables, steps, solver=abi.TRT_SOLVE_F32, tmin=ct.TMIN, tmax=ct.TMAX, bound=None, stats=False, trans=True):
    """(W (n_tori, 17, n), T (n,)[, stats]) of the _dev call: one sentinel-filled buffer holds the weights, a pad, the
    transmittance and a pad; both pads are checked.  trans=False passes a NULL trans: T comes back as sentinels."""
    n, total = len(o), sc.n_tori * K * len(o)

    def fn(sc_, p, n_, ptr, b, stream):
        tr.glow_weights_absorbed_dev(sc_, p, n_, tables, ptr, trans_ptr=ptr + 4 * (total + PAD) if trans else 0, steps=steps, tmax_ptr=b,
                                     tmin=tmin, tmax=tmax, stream=stream)

    out, st = gm._call(tr, fn, sc, o, d, solver, stats, total + PAD + n, bound)
    assert (out[total:total + PAD] == f32(SENTINEL)).all(), "written between the outputs"
    W, T = out[:total].reshape(sc.n_tori, K, n), out[total + PAD:]
    return (W, T, st) if stats else (W, T)


def window(c, solver=abi.TRT_SOLVE_F32):
    return dict(solver=solver, tmin=c["tmin"], tmax=c["tmax"], bound=c["bound"])


def zero_tables(n_tori):
    return [np.zeros((K, 4), f32) for _ in range(n_tori)]


_truth, _pieces = {}, {}


def same_rule(name, kind, steps):
    """absorbed_truth.same_rule of a case on tables_of(name), made once and shared by both solvers."""
    key = (name, kind, steps)
    if key not in _truth:
        W, T = at.same_rule(mt.case(name, kind), tables_of(name), steps)
        W.setflags(write=False)
        T.setflags(write=False)
        _truth[key] = (W, T)
    return _truth[key]


def pieces(name, kind):
    key = (name, kind)
    if key not in _pieces:
        _pieces[key] = at.pieces_per_torus(mt.case(name, kind))
    return _pieces[key]


# ---------------------------------------------------------------------------------------------------------------------
# 1. no absorption
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name,only", [("single", None), ("rings2", None), ("nest3", [0]), ("nest3", [1]), ("nest3", [2])])
def test_without_absorption_and_overlap_the_weights_are_the_plain_ones(tr, name, only, kind, solver):
    c = mt.case(name, kind)
    sc = gm.scene_of(name, only=only)
    for steps in STEPS:
        W, T = absorbed_dev(tr, sc, c["o"], c["d"], zero_tables(sc.n_tori), steps, **window(c, solver))
        plain = gw.weights_dev(tr, sc, c["o"], c["d"], steps, **window(c, solver))
        assert np.array_equal(u32(W), u32(plain)), steps
        assert (u32(T) == ONE).all(), steps
    assert (W.sum(1) > 0).any(0).mean() > 0.1


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", ["nest3", "nest8"])
def test_without_absorption_the_weights_sum_to_the_chord(tr, name, kind, solver):
    """Overlapping tubes: the pieces are cut at every torus' walls, so an accumulator of torus j takes 2 points x steps
    additions on each of the P_j pieces on which j is active (P_j from the truth's merged ends): test_gpu_weights.py's
    partition_bar with steps · P_j in place of steps.  Measured on an MI355X: 0.116 of the bar at the most
    (`nest8`, segments, 1 step), 0.070 at 4 steps, 0.043 at 64 (profiles/r28_glow_weights_absorbed.txt)."""
    c = mt.case(name, kind)
    sc = gm.scene_of(name)
    Pj, _ = pieces(name, kind)
    length = gm.chords_dev(tr, sc, c["o"], c["d"], **window(c, solver)).astype(np.float64)
    assert (length > 0).mean() > 0.1
    for steps in STEPS:
        W, T = absorbed_dev(tr, sc, c["o"], c["d"], zero_tables(sc.n_tori), steps, **window(c, solver))
        err = np.abs(W.astype(np.float64).sum(1) - length)
        bar = gw.partition_bar(steps * Pj, length)
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"{name} {kind} {steps} steps {sid(solver)}: largest error / bar {np.nanmax(np.where(length > 0, err / bar, 0.0)):.3f}")
        assert (err <= bar).all(), (steps, np.nanmax(err / np.where(bar > 0, bar, 1.0)))
        assert (u32(W)[np.broadcast_to((length == 0)[:, None, :], W.shape)] == 0).all()   # no chord: 17 zeros in bits
        assert (u32(T) == ONE).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. and 3. trt_glow_profile: its T in bits, its L at a counted bar
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", mt.NAMES)
def test_trans_and_forward_are_glow_profile(tr, name, kind, solver):
    """trans equals trt_glow_profile's T in bits (every torus has a non-zero table: torus 5 of `nest8` gets torus 4's), and
    |sum_jk W[j][k] · knot_j[k][c] - L_c| <= (2 · steps · P + 2 · n_tori + 24) · 2^-24 · sum_j S_j · top_jc, evaluated in
    float64, with S_j = sum_k W[j][k], top_jc torus j's largest knot of channel c and P the ray's number of non-empty
    pieces with an active torus (from the truth).  The count: per accumulator 2 · steps · P_j <= 2 · steps · P fma
    additions of non-negative terms, each within 2^-24 of the running sum, plus g's two products and 1 - f; on
    trt_glow_profile's side hi - lo and the fma per torus, the sum over the active tori (n_tori), the average, e · w and
    the fma into L per sub-step (the other n_tori and the 24).  w, E and T are the same bits on both sides.
    Measured on an MI355X: 0.107 of the bar at the most (`single`, 1 step), 0.078 at 4 steps, 0.090 at 64
    (profiles/r28_glow_weights_absorbed.txt)."""
    c = mt.case(name, kind)
    sc = gm.scene_of(name)
    tables = tables_of(name)
    _, P = pieces(name, kind)
    top = np.array([t.astype(np.float64).max(0)[:3] for t in tables])   # (n_tori, 3)
    for steps in STEPS:
        W, T = absorbed_dev(tr, sc, c["o"], c["d"], tables, steps, **window(c, solver))
        rgba = gp.profile_dev(tr, sc, c["o"], c["d"], tables, steps, **window(c, solver))
        assert np.array_equal(u32(T), u32(rgba[:, 3])), steps
        W64 = W.astype(np.float64)
        got = wt.forward(W64, tables)[:, :3]
        err = np.abs(got - rgba[:, :3].astype(np.float64))
        bar = ((2 * steps * P + 2 * sc.n_tori + 24) * EPS)[:, None] * np.einsum("jn,jc->nc", W64.sum(1), top)
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"{name} {kind} {steps} steps {sid(solver)}: largest error / bar {np.nanmax(np.where(bar > 0, err / bar, 0.0)):.3f}")
        assert (err <= bar).all(), (steps, np.nanmax(err / np.where(bar > 0, bar, 1.0)))
    assert (rgba[:, :3].max(1) > 1e-3).mean() > 0.05 and (rgba[:, 3] < 0.99).mean() > 0.2


# ---------------------------------------------------------------------------------------------------------------------
# 4. and 5. the rule in FP64; the known answer
# ---------------------------------------------------------------------------------------------------------------------
def knot_bar(c, solver, want, bar_T, far=None):
    """(n_tori, 17, n): test_gpu_weights.knot_bar with the ray's ends of ALL tori in (a) and the summed chords in (b) — a
    moved wall of any torus moves the samples of the pieces it bounds — plus chord_j · bar_T: |dT| <= |dtau|, and a hat
    times T integrates to at most the chord."""
    far = (np.maximum(1.0, c["t_last"]) if far is None else far)[None, :]
    r = np.array([g[2] for g in c["geo"]])[:, None]
    moved_ends = c["ends"][None, :] * ROOT_BAR[solver] * far * c["len"][None, :]
    moved_samples = 16.0 * (2.0 * c["len"][None, :] / r) * (ROOT_BAR[solver] + 2.0 ** -23) * far * c["chords"].sum(0)[None, :]
    return (moved_ends + moved_samples + c["chords"] * bar_T[None, :])[:, None, :] + COLOR_RTOL * np.abs(want) + COLOR_ATOL


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", mt.NAMES)
def test_against_the_same_rule_in_fp64(tr, name, kind, steps, solver):
    """Against absorbed_truth.same_rule at the same step count on media_truth's `robust` rays.  Per knot the bar is
    knot_bar above — test_gpu_weights.py's (a), (b), (c) with all tori's ends and the summed chords, plus chord_j · bar_T,
    bar_T being test_gpu_profile.bars' bar on T for the same tables; trans is held to bar_T + COLOR_RTOL.
    Measured on an MI355X over the 72 cases: 0.192 of the bar at the most for a weight (`rings2`, lines of sight and their cut
    form, f32: 2.7e-5 absolute), 0.122 for trans (profiles/r28_glow_weights_absorbed.txt)."""
    c = mt.case(name, kind)
    tables = tables_of(name)
    want, want_T = same_rule(name, kind, steps)
    W, T = absorbed_dev(tr, gm.scene_of(name), c["o"], c["d"], tables, steps, **window(c, solver))
    ok = c["robust"]
    assert 1.0 - ok.mean() <= c["cap"]
    bar_T = gp.bars(c, tables, solver)[1]
    err, bar = np.abs(W.astype(np.float64) - want), knot_bar(c, solver, want, bar_T)
    err_T = np.abs(T.astype(np.float64) - want_T)
    ratio, ratio_T = (err / bar)[:, :, ok], (err_T / (bar_T + COLOR_RTOL))[ok]
    print(f"{name} {kind} {steps} steps {sid(solver)}: robust {ok.mean():.4f}; largest error {err[:, :, ok].max():.3e}, "
          f"largest error / bar {ratio.max():.3f}; trans {err_T[ok].max():.3e}, error / bar {ratio_T.max():.3f}")
    assert (ratio <= 1.0).all(), ratio.max()
    assert (ratio_T <= 1.0).all(), ratio_T.max()
    assert (want_T[ok] < 0.99).mean() > 0.2                   # the set sees the media
    assert (want.sum(1)[:, ok] > 1e-3).any(0).mean() > 0.2    # weights exist
    if kind == "seg":   # windows wholly inside a tube, rays that start or end inside one
        assert (c["inside_whole"] & ok).mean() > 0.01 and (c["to_end"] & ok).mean() > 0.1 and (c["info"]["in0"].any(0) & ok).mean() > 0.3


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
def test_the_known_answer(tr, solver):
    """Rays parallel to the axis through a flat sigma: sum_k W_k = (1 - exp(-2 a sigma)) / sigma and T = exp(-2 a sigma) at
    any step count (tests/test_absorbed_cpu.py), at the bars of the FP64 comparison — the sum has coefficients 1.
    Measured on an MI355X: 4.8e-7 at the most, 0.001 of the bar; trans 6.8e-7, 0.014 of its bar."""
    c, _, e, want_L = pt.known_answer_case()
    r = c["geo"][0][2]
    a = np.cbrt(want_L[:, 0] / e[0] * 3.0 * r * r / 4.0)
    table = np.zeros((K, 4), f32)
    table[:, 3] = KNOWN_SIGMA
    want = -np.expm1(-2.0 * a * KNOWN_SIGMA) / KNOWN_SIGMA
    want_T = np.exp(-2.0 * a * KNOWN_SIGMA)
    sc = abi.Scene([(c["geo"][0][0], c["geo"][0][1], r, 0)], [camera.PLASTIC])
    bar_T = gp.bars(c, [table], solver)[1]
    assert c["robust"].all() and (want > 0.1).all()
    for steps in (1, 4):
        W, T = absorbed_dev(tr, sc, c["o"], c["d"], [table], steps, solver)
        err, bar = np.abs(W[0].astype(np.float64).sum(0) - want), knot_bar(c, solver, want[None, None], bar_T)[0, 0]
        err_T = np.abs(T.astype(np.float64) - want_T)
        print(f"known answer, {steps} steps {sid(solver)}: largest error {err.max():.3e}, error / bar {(err / bar).max():.3f}; "
              f"trans {err_T.max():.3e}, error / bar {(err_T / (bar_T + COLOR_RTOL)).max():.3f}")
        assert (err <= bar).all() and (err_T <= bar_T + COLOR_RTOL).all(), steps


# ---------------------------------------------------------------------------------------------------------------------
# 6. order and layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name,kind", [("single", "los"), ("nest3", "seg"), ("rings2", "cut"), ("nest8", "los")])
def test_rays_permute(tr, name, kind, solver):
    """One, two, three and eight tori: the three block widths."""
    c = mt.case(name, kind)
    sc, n, tables = gm.scene_of(name), len(c["o"]), tables_of(name)
    w = dict(solver=solver, tmin=c["tmin"], tmax=c["tmax"])
    W, T = absorbed_dev(tr, sc, c["o"], c["d"], tables, 4, bound=c["bound"], **w)
    perm = np.random.default_rng(11).permutation(n)[:n - 37]   # (ragged for every width)
    pb = None if c["bound"] is None else c["bound"][perm]
    Wp, Tp = absorbed_dev(tr, sc, c["o"][perm], c["d"][perm], tables, 4, bound=pb, **w)
    assert np.array_equal(u32(Wp), u32(W[:, :, perm])) and np.array_equal(u32(Tp), u32(T[perm]))
    assert len(np.unique(u32(W.reshape(-1, n)), axis=1).T) > 1000 and (W.sum(1) > 0).any(0).mean() > 0.2


@pytest.mark.parametrize("name,n_min", [("nest3", 100), ("nest8", 20)])
def test_the_result_does_not_depend_on_the_block_width(tr, name, n_min):
    """Torus j's rows in the scene (three tori: 128 lanes; eight: 64) on the rays that miss every other torus equal the
    call on the scene that holds j alone (256 lanes) in bits, and so does trans: the same pieces, the same T in front."""
    c = mt.case(name, "los")
    sc, tables = gm.scene_of(name), tables_of(name)
    length = gm.chords_dev(tr, sc, c["o"], c["d"])
    W, T = absorbed_dev(tr, sc, c["o"], c["d"], tables, 4)
    compared = 0
    for j in range(sc.n_tori):
        sel = (length[j] > 0) & (np.delete(length, j, 0) == 0).all(0)
        if not sel.any():
            continue
        Wj, Tj = absorbed_dev(tr, gm.scene_of(name, only=[j]), c["o"][sel], c["d"][sel], [tables[j]], 4)
        assert np.array_equal(u32(W[j][:, sel]), u32(Wj[0])) and np.array_equal(u32(T[sel]), u32(Tj)), j
        assert (u32(np.delete(W, j, 0)[:, :, sel]) == 0).all()
        compared += int(sel.sum())
    assert compared >= n_min, compared


def test_layout_and_both_forms(tr):
    import torch
    for name, kind in (("rings2", "seg"), ("nest3", "cut")):
        c = mt.case(name, kind)
        sc, o, d, w, tables = gm.scene_of(name), c["o"], c["d"], dict(tmin=c["tmin"], tmax=c["tmax"]), tables_of(name)
        for steps in (1, 5):
            dev, dev_T = absorbed_dev(tr, sc, o, d, tables, steps, bound=c["bound"], **w)   # (sentinel pads between and behind)
            host, host_T = tr.glow_weights_absorbed(sc, o, d, tables, steps=steps, tmax_per_ray=c["bound"], **w)
            assert host.shape == (sc.n_tori, K, len(o)) and host.dtype == np.float32 and np.array_equal(u32(host), u32(dev)), steps
            assert host_T.shape == (len(o),) and np.array_equal(u32(host_T), u32(dev_T)), steps
        for m in (64, 1):
            s = slice(100, 100 + m)
            sb = None if c["bound"] is None else c["bound"][s]
            Ws, Ts = absorbed_dev(tr, sc, o[s], d[s], tables, 5, bound=sb, **w)
            assert np.array_equal(u32(Ws), u32(dev[:, :, s])) and np.array_equal(u32(Ts), u32(dev_T[s])), m
            Wh, Th = tr.glow_weights_absorbed(sc, o[s], d[s], tables, steps=5, tmax_per_ray=sb, **w)
            assert np.array_equal(u32(Wh), u32(dev[:, :, s])) and np.array_equal(u32(Th), u32(dev_T[s])), m
        # trans == NULL: the weights' bits unchanged, nothing written where trans would be
        Wn, Tn = absorbed_dev(tr, sc, o, d, tables, 5, bound=c["bound"], trans=False, **w)
        assert np.array_equal(u32(Wn), u32(dev)) and (Tn == f32(SENTINEL)).all()
        assert len(np.unique(u32(dev.reshape(-1, len(o))), axis=1).T) > 1000
    # pads in front as well: both outputs in the middle of sentinel-filled buffers
    n = 777
    total = sc.n_tori * K * n
    keep, ptrs = gm.upload(o[:n], d[:n])
    buf = torch.full((PAD + total + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    tbuf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    tr.glow_weights_absorbed_dev(sc, ptrs, n, tables, buf.data_ptr() + 4 * PAD, trans_ptr=tbuf.data_ptr() + 4 * PAD, steps=5, **w)
    torch.cuda.synchronize()
    raw, traw = buf.cpu().numpy(), tbuf.cpu().numpy()
    assert (raw[:PAD] == f32(SENTINEL)).all() and (raw[PAD + total:] == f32(SENTINEL)).all()
    assert (traw[:PAD] == f32(SENTINEL)).all() and (traw[PAD + n:] == f32(SENTINEL)).all()
    Wd, Td = absorbed_dev(tr, sc, o[:n], d[:n], tables, 5, **w)
    assert np.array_equal(u32(raw[PAD:PAD + total].reshape(sc.n_tori, K, n)), u32(Wd)) and np.array_equal(u32(traw[PAD:PAD + n]), u32(Td))
    # n == 0: nothing launched, nothing written
    z = np.zeros((0, 3), f32)
    W0, T0 = tr.glow_weights_absorbed(sc, z, z, tables)
    assert W0.shape == (sc.n_tori, K, 0) and T0.shape == (0,)
    buf = gm.image(16)
    tr.glow_weights_absorbed_dev(sc, [0] * 6, 0, tables, buf.data_ptr(), trans_ptr=buf.data_ptr() + 32)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == f32(SENTINEL)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7. windows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
def test_windows(tr, solver):
    c = mt.case("nest3", "los")
    sc, o, d, n, tables = gm.scene_of("nest3"), c["o"], c["d"], len(c["o"]), tables_of("nest3")
    # the empty bounds (at tmin, below it, NaN, -inf), one after the other on every fifth ray: zeros, trans 1 and no test
    k = mt.case("nest3", "cut")
    empty = ~k["info"]["nonempty"]
    W, T, st = absorbed_dev(tr, sc, o, d, tables, 4, solver, bound=k["bound"], stats=True)
    assert empty.sum() == (n + 4) // 5 and set(u32(mt.EMPTY_BOUNDS)) <= set(u32(k["bound"][empty]))
    assert (u32(W[:, :, empty]) == 0).all() and (u32(T[empty]) == ONE).all()
    assert st["primary_tests"] == 3 * (n - empty.sum()) == st["traced_tests"] and st["pixels"] == n
    assert (W[:, :, ~empty] > 0).any() and (T[~empty] < 1).any()
    for b in mt.EMPTY_BOUNDS:
        W, T, st = absorbed_dev(tr, sc, o[:300], d[:300], tables, 4, solver, bound=np.full(300, b, f32), stats=True)
        assert (u32(W) == 0).all() and (u32(T) == ONE).all() and st["primary_tests"] == st["traced_tests"] == 0, b
    # tmax <= tmin for every ray: no test at all, with and without bounds
    for tmax in (float(f32(ct.TMIN)), np.nan, -1.0, -np.inf):
        for bound in (None,) if np.isnan(tmax) else (None, np.full(n, 5.0, f32)):   # (a NaN scalar clips no bound: b > NaN is false)
            W, T, st = absorbed_dev(tr, sc, o, d, tables, 4, solver, tmax=tmax, bound=bound, stats=True)
            assert (u32(W) == 0).all() and (u32(T) == ONE).all(), tmax
            assert st["primary_tests"] == st["traced_tests"] == 0, tmax
    # the full window: every torus of every ray is started
    W, T, st = absorbed_dev(tr, sc, o, d, tables, 4, solver, stats=True)
    assert st["primary_tests"] == 3 * n and st["pixels"] == n


# ---------------------------------------------------------------------------------------------------------------------
# 8. capture and replay
# ---------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay(tr):
    """The _dev call captured on a side stream with two step counts, one graph each (kernel nodes only, no ctx scratch, the
    tables and the step count in the launch's arguments): each replay gives its own eager bits, with an eager call of
    another scene — another block width — in between."""
    import torch
    c = mt.case("nest3", "seg")
    sc, w, tables = gm.scene_of("nest3"), dict(tmin=c["tmin"], tmax=c["tmax"]), tables_of("nest3")
    n = 256 * 5 + 33
    total = sc.n_tori * K * n
    o, d = c["o"][:n], c["d"][:n]
    bound = np.linspace(0.3, 1.5, n).astype(f32)
    eager = {steps: absorbed_dev(tr, sc, o, d, tables, steps, bound=bound, **w) for steps in (3, 16)}
    assert not np.array_equal(u32(eager[3][0]), u32(eager[16][0]))
    keep, ptrs = gm.upload(o, d)
    b = torch.from_numpy(bound).to("cuda:0")
    bufs = {steps: (gm.image(total), gm.image(n)) for steps in eager}
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    graphs = {}
    with torch.cuda.stream(side):
        for steps in eager:
            graphs[steps] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[steps], stream=side):
                tr.glow_weights_absorbed_dev(sc, ptrs, n, tables, bufs[steps][0].data_ptr(), trans_ptr=bufs[steps][1].data_ptr(), steps=steps,
                                             tmax_ptr=b.data_ptr(), stream=side.cuda_stream, **w)
    cur.wait_stream(side)
    s = mt.case("single", "los")
    for k in range(2):
        for steps in (3, 16) if k == 0 else (16, 3):
            bufs[steps][0].fill_(SENTINEL)
            bufs[steps][1].fill_(SENTINEL)
            graphs[steps].replay()
            torch.cuda.synchronize()
            assert np.array_equal(u32(gm.read(bufs[steps][0], total).reshape(sc.n_tori, K, n)), u32(eager[steps][0])), (k, steps)
            assert np.array_equal(u32(gm.read(bufs[steps][1], n)), u32(eager[steps][1])), (k, steps)
            other, _ = absorbed_dev(tr, gm.scene_of("single"), s["o"][:500], s["d"][:500], tables_of("single"), 7)   # 256 lanes
            assert (other > 0).any()
    assert len(np.unique(u32(eager[3][0].reshape(-1, n)), axis=1).T) > 50


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable_and_the_outputs_unwritten(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    c = mt.case("rings2", "seg")
    sc, w, tables = gm.scene_of("rings2"), dict(tmin=c["tmin"], tmax=c["tmax"]), tables_of("rings2")
    n = 300
    o, d = c["o"][:n], c["d"][:n]
    want, want_T = absorbed_dev(tr, sc, o, d, tables, 4, **w)
    keep, ptrs = gm.upload(o, d)
    out, tout = gm.image(sc.n_tori * K * n), gm.image(n)
    host_out, host_T = np.full((sc.n_tori, K, n + 1), SENTINEL, f32), np.full(n + 1, SENTINEL, f32)
    L = tr._L
    rays = abi.rays_struct(ptrs, n)
    host_rays = abi.rays_struct([np.ascontiguousarray(a[:, k]) for a in (o, d) for k in range(3)], n)
    prof = abi.profiles(tables)

    def good():
        W, T = absorbed_dev(tr, sc, o, d, tables, 4, **w)
        assert np.array_equal(u32(W), u32(want)) and np.array_equal(u32(T), u32(want_T))

    def refused(call, *needles):
        with pytest.raises(TrtError) as e:
            call()
        assert e.value.code == abi.TRT_E_INVALID, str(e.value)
        for needle in ("trt_glow_weights_absorbed",) + needles:
            assert needle in str(e.value), str(e.value)
        good()

    def refused_raw(rc, who=b"trt_glow_weights_absorbed"):
        assert rc == abi.TRT_E_INVALID
        assert who in L.trt_last_error(tr._h)
        good()

    dev = lambda tabs=tables, p=ptrs, wp=None, **kw: tr.glow_weights_absorbed_dev(sc, p, n, tabs, out.data_ptr() if wp is None else wp,
                                                                                 trans_ptr=tout.data_ptr(), **dict(w, **kw))
    good()
    # everything trt_glow_weights refuses
    refused(lambda: dev(wp=0), "NULL output")
    refused(lambda: dev(p=ptrs[:2] + [0] + ptrs[3:]), "NULL ray stream")
    scp, outp, toutp = C.byref(sc.c), C.c_void_p(out.data_ptr()), C.c_void_p(tout.data_ptr())
    refused_raw(L.trt_glow_weights_absorbed_dev(tr._h, None, None, scp, prof, 4, 0.001, 1.0, outp, toutp, None))
    refused_raw(L.trt_glow_weights_absorbed_dev(tr._h, C.byref(rays), None, None, prof, 4, 0.001, 1.0, outp, toutp, None), b"scene")
    refused_raw(L.trt_glow_weights_absorbed(tr._h, C.byref(host_rays), None, scp, prof, 4, 0.001, 1.0, None, host_T.ctypes.data))
    refused_raw(L.trt_glow_weights_absorbed(tr._h, C.byref(host_rays), None, None, prof, 4, 0.001, 1.0, host_out.ctypes.data, host_T.ctypes.data), b"scene")
    for big in (2 ** 63, 2 ** 60):   # 2 tori · 17 · n
        refused_raw(L.trt_glow_weights_absorbed_dev(tr._h, C.byref(abi.rays_struct(ptrs, big)), None, scp, prof, 4, 0.001, 1.0, outp, toutp, None),
                    b"overflows")
    # NULL profiles
    refused(lambda: dev(tabs=None), "NULL profiles")
    refused_raw(L.trt_glow_weights_absorbed(tr._h, C.byref(host_rays), None, scp, None, 4, 0.001, 1.0, host_out.ctypes.data, host_T.ctypes.data),
                b"NULL profiles")
    # steps outside 1..TRT_MAX_GLOW_STEPS
    for steps in (0, abi.TRT_MAX_GLOW_STEPS + 1, 2 ** 32 - 1):
        refused(lambda: dev(steps=steps), "steps", "TRT_MAX_GLOW_STEPS")
        refused(lambda: tr.glow_weights_absorbed(sc, o, d, tables, steps=steps, **w), "steps")
    # a sigma knot that is negative, NaN or infinite: the message names the torus and the knot
    for j, k, v in ((0, 0, -1.0), (1, 16, np.nan), (1, 7, np.inf), (0, 9, -0.5)):
        broken = [np.array(t) for t in tables]
        broken[j][k, 3] = v
        refused(lambda: dev(tabs=broken), f"torus {j}", f"knot {k}", "sigma")
    refused(lambda: tr.glow_weights_absorbed(sc, o, d, broken, steps=4, **w), "torus 0", "knot 9")
    # the emission entries are not read: a NaN there is NOT refused and changes nothing
    odd = [np.array(t) for t in tables]
    odd[0][3, 0], odd[1][16, 2], odd[1][0, 1] = np.nan, -np.inf, -4.0
    W, T = absorbed_dev(tr, sc, o, d, odd, 4, **w)
    assert np.array_equal(u32(W), u32(want)) and np.array_equal(u32(T), u32(want_T))
    # the enumeration is the default solver's: every other one is refused, worded like trt_crossings' refusal
    for solver in (abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_DK_F64, abi.TRT_SOLVE_FERRARI_F32, abi.TRT_SOLVE_FERRARI_F64):
        tr.set_solver(solver)
        try:
            for call in (lambda: dev(), lambda: tr.glow_weights_absorbed(sc, o, d, tables)):
                with pytest.raises(TrtError) as e:
                    call()
                assert e.value.code == abi.TRT_E_INVALID and "trt_glow_weights_absorbed" in str(e.value), str(e.value)
                assert "the enumeration runs the default solver (TRT_SOLVE_F32 / _F64) only" in str(e.value)
        finally:
            tr.set_solver(abi.TRT_SOLVE_F32)
        good()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == f32(SENTINEL)).all() and (tout.cpu().numpy() == f32(SENTINEL)).all()   # a refused call writes nothing
    assert (host_out == f32(SENTINEL)).all() and (host_T == f32(SENTINEL)).all()
    assert L.trt_glow_weights_absorbed_dev(None, C.byref(rays), None, scp, prof, 4, 0.001, 1.0, outp, toutp, None) == abi.TRT_E_INVALID
    good()
