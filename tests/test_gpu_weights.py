"""trt_glow_weights[_dev]: the response of every line of sight to every knot of every torus' profile (include/trt.h).

Anchors, from the strictest down:
  1. the torus alone — the 17 rows of torus j in a scene equal the call on the scene that holds j alone, bit for bit;
  2. trt_chords — the 17 weights of a torus sum to its chord, at a bar counted from the roundings of the rule;
  3. trt_glow_profile — one torus, sigma 0: sum_k W_k · knot_k is its L at the same steps, at a bar counted likewise;
  4. the FP64 restatement of the rule (tests/weights_truth.py: same_rule) at the same step count, at derived bars;
  5. the known answer: the three moments of a ray parallel to the axis.
Then order and layout, the windows, capture and replay, and the refusals.  Sets are media_truth's: 4096 rays.
"""
import ctypes as C

import numpy as np
import pytest

import crossings_truth as ct
import media_truth as mt
import profile_truth as pt
import test_gpu_media as gm
import test_gpu_profile as gp
import weights_truth as wt
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

COLOR_RTOL, COLOR_ATOL, ROOT_BAR = gm.COLOR_RTOL, gm.COLOR_ATOL, gm.ROOT_BAR   # the bars of tests/test_gpu_media.py
SOLVERS, SOLVER_IDS = gm.SOLVERS, gm.SOLVER_IDS
SENTINEL, PAD = gm.SENTINEL, gm.PAD
f32, u32 = np.float32, gm.u32
STEPS = (1, 4, 64)
K = abi.TRT_PROFILE_KNOTS
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def weights_dev(tr, sc, o, d, steps, solver=abi.TRT_SOLVE_F32, tmin=ct.TMIN, tmax=ct.TMAX, bound=None, stats=False):
    out, st = gm._call(tr, lambda sc_, p, n, ptr, b, stream: tr.glow_weights_dev(sc_, p, n, ptr, steps=steps, tmax_ptr=b, tmin=tmin,
                                                                                tmax=tmax, stream=stream),
                       sc, o, d, solver, stats, sc.n_tori * K * len(o), bound)
    out = out.reshape(sc.n_tori, K, len(o))
    return (out, st) if stats else out


def window(c, solver=abi.TRT_SOLVE_F32):
    return dict(solver=solver, tmin=c["tmin"], tmax=c["tmax"], bound=c["bound"])


_truth = {}


def same_rule(name, kind, steps):
    """weights_truth.same_rule of a case, made once and shared by both solvers."""
    key = (name, kind, steps)
    if key not in _truth:
        W = wt.same_rule(mt.case(name, kind), steps)
        W.setflags(write=False)
        _truth[key] = W
    return _truth[key]


def single_torus_scenes():
    """(name, j): `single`, and each torus of `nest3` and `rings2` alone."""
    return [("single", 0)] + [("nest3", j) for j in range(3)] + [("rings2", j) for j in range(2)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the torus alone, bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", ["nest3", "rings2", "nest8"])
def test_a_torus_in_the_scene_is_the_torus_alone(tr, name, kind, solver):
    c = mt.case(name, kind)
    sc = gm.scene_of(name)
    n_windows = int(c["info"]["nonempty"].sum())
    got, st = weights_dev(tr, sc, c["o"], c["d"], 4, stats=True, **window(c, solver))
    assert st["primary_tests"] == sc.n_tori * n_windows == st["traced_tests"] and st["pixels"] == len(c["o"])
    for j in range(sc.n_tori) if name != "nest8" else (0, 7):
        alone, st1 = weights_dev(tr, gm.scene_of(name, only=[j]), c["o"], c["d"], 4, stats=True, **window(c, solver))
        assert alone.shape == (1, K, len(c["o"])) and np.array_equal(u32(got[j]), u32(alone[0])), j
        assert st1["primary_tests"] == n_windows
        assert len(np.unique(u32(got[j]), axis=1).T) > 50 and (got[j] >= 0).all(), j


# ---------------------------------------------------------------------------------------------------------------------
# 2. partition: the weights of a torus sum to its chord
# ---------------------------------------------------------------------------------------------------------------------
def partition_bar(steps, length):
    """An accumulator takes at most 2 intervals x 2 points x steps fma additions of non-negative terms, each within 2^-24 of
    the running sum; inv_steps, h, l, 1 - f and the chord's own three operations account for the rest.  Measured on an
    MI355X: 0.098 of the bar at the most (1 step), 0.043 at 64 steps."""
    return (4 * steps + 16) * EPS * length


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", mt.NAMES)
def test_the_weights_sum_to_the_chord(tr, name, kind, solver):
    c = mt.case(name, kind)
    sc = gm.scene_of(name)
    length = gm.chords_dev(tr, sc, c["o"], c["d"], **window(c, solver)).astype(np.float64)
    assert (length > 0).mean() > 0.1
    for steps in STEPS:
        W = weights_dev(tr, sc, c["o"], c["d"], steps, **window(c, solver))
        err = np.abs(W.astype(np.float64).sum(1) - length)
        bar = partition_bar(steps, length)
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"{name} {kind} {steps} steps {SOLVER_IDS[SOLVERS.index(solver)]}: largest error / bar {np.nanmax(np.where(length > 0, err / bar, 0.0)):.3f}")
        assert (err <= bar).all(), (steps, np.nanmax(err / np.where(bar > 0, bar, 1.0)))
        assert (u32(W)[np.broadcast_to((length == 0)[:, None, :], W.shape)] == 0).all()   # no chord: 17 zeros in bits


# ---------------------------------------------------------------------------------------------------------------------
# 3. forward: one torus with sigma 0 is trt_glow_profile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name,j", single_torus_scenes())
def test_forward_is_glow_profile(tr, name, j, kind, solver):
    """|sum_k W_k · knot_k[c] - L_c| <= (4 · steps + 24) · 2^-24 · length · max_k knot_k[c], evaluated in float64: the rounding
    count of the partition, plus the table's hi - lo, its fma, and the average of the two points.  Measured on an MI355X:
    0.108 of the bar at the most (1 step), 0.077 at 64 steps."""
    c = mt.case(name, kind)
    sc = gm.scene_of(name, only=[j])
    table = np.array(pt.PROFILES[name]["curved"][j])
    table[:, 3] = 0.0
    length = gm.chords_dev(tr, sc, c["o"], c["d"], **window(c, solver))[0].astype(np.float64)
    top = table.astype(np.float64).max(0)[:3]
    for steps in STEPS:
        W = weights_dev(tr, sc, c["o"], c["d"], steps, **window(c, solver))
        rgba = gp.profile_dev(tr, sc, c["o"], c["d"], [table], steps, **window(c, solver))
        assert (u32(rgba[:, 3]) == u32(f32(1.0))).all()   # nothing absorbs: T == 1 in bits
        got = wt.forward(W.astype(np.float64), [table])[:, :3]
        err = np.abs(got - rgba[:, :3].astype(np.float64))
        bar = (4 * steps + 24) * EPS * length[:, None] * top[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"{name}[{j}] {kind} {steps} steps {SOLVER_IDS[SOLVERS.index(solver)]}: largest error / bar "
                  f"{np.nanmax(np.where(bar > 0, err / bar, 0.0)):.3f}")
        assert (err <= bar).all(), (steps, np.nanmax(err / np.where(bar > 0, bar, 1.0)))
    assert (rgba[:, :3].max(1) > 1e-3).mean() > 0.05


# ---------------------------------------------------------------------------------------------------------------------
# 4. and 5. the rule in FP64; the known answer
# ---------------------------------------------------------------------------------------------------------------------
def knot_bar(c, solver, want, far=None):
    """(n_tori, 1, n) + the terms that depend on the value: the bar on one weight (or on a sum of weights with
    coefficients in [-1, 1] whose integrand has a slope of at most 16 in x) — see test_against_the_same_rule_in_fp64.
    `far` (n,) replaces max(1, t_last) where the root bar is stated otherwise (tests/test_gpu_media_domain.py)."""
    ends = (~np.isnan(c["A"])).sum(2) + (~np.isnan(c["B"])).sum(2)                       # E_j (n_tori, n)
    far = (np.maximum(1.0, c["t_last"]) if far is None else far)[None, :]
    r = np.array([g[2] for g in c["geo"]])[:, None]
    moved_ends = ends * ROOT_BAR[solver] * far * c["len"][None, :]
    moved_samples = 16.0 * (2.0 * c["len"][None, :] / r) * (ROOT_BAR[solver] + 2.0 ** -23) * far * c["chords"]
    return (moved_ends + moved_samples)[:, None, :] + COLOR_RTOL * np.abs(want) + COLOR_ATOL


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", mt.NAMES)
def test_against_the_same_rule_in_fp64(tr, name, kind, steps, solver):
    """Against weights_truth.same_rule at the same step count on media_truth's `robust` rays.  The rule is the same on both
    sides; what differs is where torus j's intervals end, and FP32.  Per knot the bar is the sum of
    (a) E_j · ROOT_BAR · max(1, t_last) · len: every interval end of torus j that is not an end of the window is a
        trt_crossings root, held to |dt| <= ROOT_BAR · max(1, t); an end that moves by dt moves the total by dt · len, and
        any one knot by no more (a hat is at most 1);
    (b) 16 · (2 · len / r_j) · (ROOT_BAR + 2^-23) · max(1, t_last) · chord_j: a hat has slope 16 in x, |dx / dt| <= 2 · len / r,
        the samples sit at fixed fractions of an interval and move with its ends, carry their own FP32 rounding of t
        (2^-23 relative covers m and the Gauss point), and the change is integrated over the chord — profile_truth.slope_term
        with the slope 16;
    (c) COLOR_RTOL · W_k + COLOR_ATOL: FP32 in the label, f and the sums, the project's bars on colours.
    The largest error / bar per case is printed.  On an MI355X the largest over all 72 cases was 0.197 (`rings2`, lines of
    sight and their cut form, f32, at every step count: 2.7e-5 absolute) and 0.102 with the FP64 solve; the largest absolute
    error was 8.1e-5 (the nest of eight, segments, 1 step, f32: 0.044 of its bar).  The roots are far better than their bar,
    so the bars are loose; what the comparison would catch is a rule that differs."""
    c = mt.case(name, kind)
    want = same_rule(name, kind, steps)
    got = weights_dev(tr, gm.scene_of(name), c["o"], c["d"], steps, **window(c, solver)).astype(np.float64)
    ok = c["robust"]
    assert 1.0 - ok.mean() <= c["cap"]
    err, bar = np.abs(got - want), knot_bar(c, solver, want)
    ratio = (err / bar)[:, :, ok]
    print(f"{name} {kind} {steps} steps {SOLVER_IDS[SOLVERS.index(solver)]}: robust {ok.mean():.4f}; largest error {err[:, :, ok].max():.3e}, "
          f"largest error / bar {ratio.max():.3f}; non-robust rays over a bar: {int((err > bar).any((0, 1))[~ok].sum())} of {int((~ok).sum())}")
    assert (ratio <= 1.0).all(), ratio.max()
    assert (want.sum(1)[:, ok] > 1e-3).any(0).mean() > 0.2   # (the set sees the tubes)
    if kind == "seg":   # windows wholly inside a tube, rays that start or end inside one
        assert (c["inside_whole"] & ok).mean() > 0.01 and (c["to_end"] & ok).mean() > 0.1 and (c["info"]["in0"].any(0) & ok).mean() > 0.3


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
def test_the_known_answer(tr, solver):
    """Rays parallel to the axis: sum W_k = 2a, sum W_k x_k = the integral of x, sum W_k (1 - x_k) = 4a³ / (3r²), exact for
    the rule at any step count (tests/test_weights_cpu.py).  Each moment is a sum of weights with coefficients in [0, 1]
    whose integrand is at most 1 and has a slope of at most 1 in x: the bar of one weight holds for it.  Measured on an
    MI355X: 8.6e-7 at the most, 0.002 of the bar."""
    c, table, e, want_L = pt.known_answer_case()
    r = c["geo"][0][2]
    a = np.cbrt(want_L[:, 0] / e[0] * 3.0 * r * r / 4.0)
    want = wt.axis_moments(a, r)
    sc = abi.Scene([(c["geo"][0][0], c["geo"][0][1], r, 0)], [camera.PLASTIC])
    assert c["robust"].all() and (want[2] > 0.01).all()
    for steps in (1, 4):
        got = wt.moments_of(weights_dev(tr, sc, c["o"], c["d"], steps, solver)[0].astype(np.float64))
        err, bar = np.abs(got - want), knot_bar(c, solver, want[None])[0]
        print(f"known answer, {steps} steps {SOLVER_IDS[SOLVERS.index(solver)]}: largest error {err.max():.3e}, error / bar {(err / bar).max():.3f}")
        assert (err <= bar).all(), (steps, (err / bar).max())


# ---------------------------------------------------------------------------------------------------------------------
# 6. order and layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name,kind", [("nest3", "seg"), ("rings2", "cut"), ("nest8", "los")])
def test_rays_permute(tr, name, kind, solver):
    c = mt.case(name, kind)
    sc, n = gm.scene_of(name), len(c["o"])
    w = dict(solver=solver, tmin=c["tmin"], tmax=c["tmax"])
    got = weights_dev(tr, sc, c["o"], c["d"], 4, bound=c["bound"], **w)
    perm = np.random.default_rng(11).permutation(n)[:n - 37]   # (ragged: 15 full blocks and 219 rays)
    pb = None if c["bound"] is None else c["bound"][perm]
    assert np.array_equal(u32(weights_dev(tr, sc, c["o"][perm], c["d"][perm], 4, bound=pb, **w)), u32(got[:, :, perm]))
    assert len(np.unique(u32(got.reshape(-1, n)), axis=1).T) > 1000 and (got.sum(1) > 0).any(0).mean() > 0.2


def test_layout_and_both_forms(tr):
    import torch
    for name, kind in (("rings2", "seg"), ("nest3", "cut")):
        c = mt.case(name, kind)
        sc, o, d, w = gm.scene_of(name), c["o"], c["d"], dict(tmin=c["tmin"], tmax=c["tmax"])
        for steps in (1, 5):
            dev = weights_dev(tr, sc, o, d, steps, bound=c["bound"], **w)   # (a sentinel pad behind the output is checked)
            host = tr.glow_weights(sc, o, d, steps=steps, tmax_per_ray=c["bound"], **w)
            assert host.shape == (sc.n_tori, K, len(o)) and host.dtype == np.float32 and np.array_equal(u32(host), u32(dev)), steps
        for m in (64, 1):
            s = slice(100, 100 + m)
            sb = None if c["bound"] is None else c["bound"][s]
            assert np.array_equal(u32(weights_dev(tr, sc, o[s], d[s], 5, bound=sb, **w)), u32(dev[:, :, s])), m
            assert np.array_equal(u32(tr.glow_weights(sc, o[s], d[s], steps=5, tmax_per_ray=sb, **w)), u32(dev[:, :, s])), m
        assert len(np.unique(u32(dev.reshape(-1, len(o))), axis=1).T) > 1000
    # a pad in front as well: the output in the middle of a sentinel-filled buffer
    n = 777
    total = sc.n_tori * K * n
    keep, ptrs = gm.upload(o[:n], d[:n])
    buf = torch.full((PAD + total + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    tr.glow_weights_dev(sc, ptrs, n, buf.data_ptr() + 4 * PAD, steps=5, **w)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:PAD] == f32(SENTINEL)).all() and (raw[PAD + total:] == f32(SENTINEL)).all()
    assert np.array_equal(u32(raw[PAD:PAD + total].reshape(sc.n_tori, K, n)), u32(weights_dev(tr, sc, o[:n], d[:n], 5, **w)))
    # n == 0: nothing launched, nothing written
    z = np.zeros((0, 3), f32)
    assert tr.glow_weights(sc, z, z).shape == (sc.n_tori, K, 0)
    buf = gm.image(16)
    tr.glow_weights_dev(sc, [0] * 6, 0, buf.data_ptr())
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == f32(SENTINEL)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7. windows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
def test_windows(tr, solver):
    c = mt.case("nest3", "los")
    sc, o, d, n = gm.scene_of("nest3"), c["o"], c["d"], len(c["o"])
    whole = weights_dev(tr, sc, o, d, 4, solver)
    # every bound equal to the scalar, or beyond it (the scalar clips): the scalar path's bits
    for b in (ct.TMAX, np.inf, 3.0e38):
        assert np.array_equal(u32(weights_dev(tr, sc, o, d, 4, solver, bound=np.full(n, b, f32))), u32(whole)), b
    # the empty bounds (at tmin, below it, NaN, -inf), one after the other on every fifth ray: zeros and no test
    k = mt.case("nest3", "cut")
    empty = ~k["info"]["nonempty"]
    got, st = weights_dev(tr, sc, o, d, 4, solver, bound=k["bound"], stats=True)
    assert empty.sum() == (n + 4) // 5 and set(u32(mt.EMPTY_BOUNDS)) <= set(u32(k["bound"][empty]))
    assert (u32(got[:, :, empty]) == 0).all()
    assert st["primary_tests"] == 3 * (n - empty.sum()) == st["traced_tests"] and (got[:, :, ~empty] > 0).any()
    for b in mt.EMPTY_BOUNDS:
        got, st = weights_dev(tr, sc, o[:300], d[:300], 4, solver, bound=np.full(300, b, f32), stats=True)
        assert (u32(got) == 0).all() and st["primary_tests"] == st["traced_tests"] == 0, b
    # tmax <= tmin for every ray: no test at all, with and without bounds
    for tmax in (float(f32(ct.TMIN)), np.nan, -1.0, -np.inf):
        for bound in (None,) if np.isnan(tmax) else (None, np.full(n, 5.0, f32)):   # (a NaN scalar clips no bound: b > NaN is false)
            got, st = weights_dev(tr, sc, o, d, 4, solver, tmax=tmax, bound=bound, stats=True)
            assert (u32(got) == 0).all(), tmax
            assert st["primary_tests"] == st["traced_tests"] == 0, tmax
    # a window wholly inside a tube, and rays that start or end inside one: the segment set holds them, and they are held
    # to the chord and to the FP64 rule in tests 2 and 4; here: they have positive weight
    s = mt.case("nest3", "seg")
    got = weights_dev(tr, sc, s["o"], s["d"], 4, solver, s["tmin"], s["tmax"]).sum(1)
    inside = s["inside_whole"] & s["robust"]
    assert inside.sum() > 40 and (got[:, inside].max(0) > 0).all()
    started = s["info"]["in0"].any(0) & ~s["inside_whole"] & s["robust"]
    assert started.sum() > 1000 and (got[:, started].max(0) > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. capture and replay
# ---------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay(tr):
    """The _dev call captured on a side stream with two step counts, one graph each (kernel nodes only, no ctx scratch, the
    step count in the launch's arguments): each replay gives its own eager bits, whatever was launched in between."""
    import torch
    c = mt.case("nest3", "seg")
    sc, w = gm.scene_of("nest3"), dict(tmin=c["tmin"], tmax=c["tmax"])
    n = 256 * 5 + 33
    total = sc.n_tori * K * n
    o, d = c["o"][:n], c["d"][:n]
    bound = np.linspace(0.3, 1.5, n).astype(f32)
    eager = {steps: weights_dev(tr, sc, o, d, steps, bound=bound, **w) for steps in (3, 16)}
    assert not np.array_equal(u32(eager[3]), u32(eager[16]))
    keep, ptrs = gm.upload(o, d)
    b = torch.from_numpy(bound).to("cuda:0")
    bufs = {steps: gm.image(total) for steps in eager}
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    graphs = {}
    with torch.cuda.stream(side):
        for steps in eager:
            graphs[steps] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[steps], stream=side):
                tr.glow_weights_dev(sc, ptrs, n, bufs[steps].data_ptr(), steps=steps, tmax_ptr=b.data_ptr(), stream=side.cuda_stream, **w)
    cur.wait_stream(side)
    for k in range(2):
        for steps in (3, 16) if k == 0 else (16, 3):
            bufs[steps].fill_(SENTINEL)
            graphs[steps].replay()
            torch.cuda.synchronize()
            assert np.array_equal(u32(gm.read(bufs[steps], total).reshape(sc.n_tori, K, n)), u32(eager[steps])), (k, steps)
            other = weights_dev(tr, sc, o[:500], d[:500], 7, **w)   # an eager call of another step count in between
            assert not np.array_equal(u32(other), u32(eager[steps][:, :, :500]))
    assert len(np.unique(u32(eager[3].reshape(-1, n)), axis=1).T) > 50


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable_and_the_outputs_unwritten(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    c = mt.case("rings2", "seg")
    sc, w = gm.scene_of("rings2"), dict(tmin=c["tmin"], tmax=c["tmax"])
    n = 300
    o, d = c["o"][:n], c["d"][:n]
    want = weights_dev(tr, sc, o, d, 4, **w)
    keep, ptrs = gm.upload(o, d)
    out = gm.image(sc.n_tori * K * n)
    host_out = np.full((sc.n_tori, K, n + 1), SENTINEL, f32)
    L = tr._L
    rays = abi.rays_struct(ptrs, n)
    host_rays = abi.rays_struct([np.ascontiguousarray(a[:, k]) for a in (o, d) for k in range(3)], n)

    def good():
        assert np.array_equal(u32(weights_dev(tr, sc, o, d, 4, **w)), u32(want))

    def refused(call, *needles):
        with pytest.raises(TrtError) as e:
            call()
        assert e.value.code == abi.TRT_E_INVALID, str(e.value)
        for needle in ("trt_glow_weights",) + needles:
            assert needle in str(e.value), str(e.value)
        good()

    def refused_raw(rc, who=b"trt_glow_weights"):
        assert rc == abi.TRT_E_INVALID
        assert who in L.trt_last_error(tr._h)
        good()

    good()
    # everything trt_chords refuses
    refused(lambda: tr.glow_weights_dev(sc, ptrs, n, 0), "NULL output")
    refused(lambda: tr.glow_weights_dev(sc, ptrs[:2] + [0] + ptrs[3:], n, out.data_ptr()), "NULL ray stream")
    scp, outp = C.byref(sc.c), C.c_void_p(out.data_ptr())
    refused_raw(L.trt_glow_weights_dev(tr._h, None, None, scp, 4, 0.001, 1.0, outp, None))
    refused_raw(L.trt_glow_weights_dev(tr._h, C.byref(rays), None, None, 4, 0.001, 1.0, outp, None), b"scene")
    refused_raw(L.trt_glow_weights(tr._h, C.byref(host_rays), None, scp, 4, 0.001, 1.0, None))
    refused_raw(L.trt_glow_weights(tr._h, C.byref(host_rays), None, None, 4, 0.001, 1.0, host_out.ctypes.data), b"scene")
    for big in (2 ** 63, 2 ** 60):   # 2 tori · 17 · n
        refused_raw(L.trt_glow_weights_dev(tr._h, C.byref(abi.rays_struct(ptrs, big)), None, scp, 4, 0.001, 1.0, outp, None), b"overflows")
    # steps outside 1..TRT_MAX_GLOW_STEPS
    for steps in (0, abi.TRT_MAX_GLOW_STEPS + 1, 2 ** 32 - 1):
        refused(lambda: tr.glow_weights_dev(sc, ptrs, n, out.data_ptr(), steps=steps, **w), "steps", "TRT_MAX_GLOW_STEPS")
        refused(lambda: tr.glow_weights(sc, o, d, steps=steps, **w), "steps")
    assert np.array_equal(u32(tr.glow_weights(sc, o, d, steps=abi.TRT_MAX_GLOW_STEPS, **w)),
                          u32(weights_dev(tr, sc, o, d, abi.TRT_MAX_GLOW_STEPS, **w)))
    # the enumeration is the default solver's: every other one is refused, worded like trt_crossings' refusal
    for solver in (abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_DK_F64, abi.TRT_SOLVE_FERRARI_F32, abi.TRT_SOLVE_FERRARI_F64):
        tr.set_solver(solver)
        try:
            for call in (lambda: tr.glow_weights_dev(sc, ptrs, n, out.data_ptr()), lambda: tr.glow_weights(sc, o, d)):
                with pytest.raises(TrtError) as e:
                    call()
                assert e.value.code == abi.TRT_E_INVALID and "trt_glow_weights" in str(e.value), str(e.value)
                assert "the enumeration runs the default solver (TRT_SOLVE_F32 / _F64) only" in str(e.value)
        finally:
            tr.set_solver(abi.TRT_SOLVE_F32)
        good()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == f32(SENTINEL)).all() and (host_out == f32(SENTINEL)).all()   # a refused call writes nothing
    assert L.trt_glow_weights_dev(None, C.byref(rays), None, scp, 4, 0.001, 1.0, outp, None) == abi.TRT_E_INVALID
    good()
