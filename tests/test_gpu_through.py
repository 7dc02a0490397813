"""trt_transmittance[_dev] / trt_shade_through[_dev]: translucent shells composited along a ray (include/trt.h).

Anchors, from the strictest down:
  1. the library's own crossings — T is, bit for bit and on every ray, the product of the pass factors over the ids
     trt_crossings_dev lists (opacities chosen so that the product is exact in FP32, whatever the order);
  2. trt_shade_dev — with every surface opaque and one torus the colours are its colours bit for bit, except where the
     truth says the ray is non-robust (a first root that falls to the interval test); with several tori, at the
     project's colour bars on robust rays;
  3. the scene without the torus — a torus of opacity 0 is absent, bit for bit, on every ray;
  4. the FP64 truth of tests/through_truth.py at the bars of tests/test_oracle.py's FP64 comparison.
Then the layout, the paths (host, device, captured) and the refusals.  Sets are crossings_truth's 4096 rays.
"""
import ctypes as C

import numpy as np
import pytest

import crossings_truth as ct
import through_truth as tt
from camera_support import stream_handle
from shade_support import (QUERY_KEYS, SENTINEL, SOLVER_IDS, SOLVERS, bracket, image, meets_truth_bars, rays_call, read, shade_dev, tr,  # noqa: F401
                           u32, upload)
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

COLOR_RTOL, COLOR_ATOL = 1e-5, 1e-6   # the project's bars on colours (tests/test_gpu_parity.py)
K_ALL = abi.TRT_MAX_CROSSINGS
f32 = np.float32


def scene_of(name, alpha, mats=None, only=None):
    """SCENES[name] (or its tori `only`) with one material per torus carrying alpha[j] as dissolve."""
    geo, axes = ct.SCENES[name]
    pick = list(range(len(geo))) if only is None else list(only)
    mats = mats or [camera.PLASTIC] * len(geo)
    return abi.Scene([(geo[j][0], geo[j][1], geo[j][2], i) for i, j in enumerate(pick)],
                     [dict(mats[j], dissolve=alpha[j]) for j in pick], axes=None if axes is None else [axes[j] for j in pick])


def transmittance_dev(tr, sc, o, d, solver=abi.TRT_SOLVE_F32, tmin=ct.TMIN, tmax=ct.TMAX, bound=None, stats=False):
    """One float per ray, not an image: the bracket of rays_call around trt_transmittance_dev."""
    import torch
    b = None if bound is None else torch.from_numpy(np.ascontiguousarray(bound, np.float32)).to("cuda:0")
    keep, ptrs = upload(o, d) if len(o) else (None, [0] * 6)
    buf = image(len(o))
    with bracket(tr, solver, stats) as got:
        tr.transmittance_dev(sc, ptrs, len(o), buf.data_ptr(), tmax_ptr=0 if b is None else b.data_ptr(), tmin=tmin, tmax=tmax,
                             stream=stream_handle())
    T = read(buf, len(o))
    return (T, got["stats"]) if stats else T


def through_dev(tr, sc, o, d, pc, samples=1, solver=abi.TRT_SOLVE_F32, stats=False):
    return rays_call(tr, "shade_through_dev", sc, o, d, pc, samples, solver, stats)


def crossings_dev(tr, sc, o, d, solver, tmin=ct.TMIN, tmax=ct.TMAX):
    """(t (K, n), id (K, n)) of trt_crossings_dev with all 32 slots."""
    import torch
    n = len(o)
    keep, ptrs = upload(o, d)
    t = torch.empty((K_ALL, n), dtype=torch.float32, device="cuda:0")
    tid = torch.empty((K_ALL, n), dtype=torch.int32, device="cuda:0")
    with bracket(tr, solver):
        tr.crossings_dev(sc, ptrs, n, {"t": t.data_ptr(), "id": tid.data_ptr()}, max_per_ray=K_ALL, tmin=tmin, tmax=tmax,
                         stream=stream_handle())
    return t.cpu().numpy(), tid.cpu().numpy()


def product_over(tid, alpha):
    """FP32 product of 1 - a_id over the listed ids, slot by slot (exact for the opacities of these tests: any order)."""
    p = np.append(f32(1.0) - np.clip(np.asarray(alpha, f32), f32(0), f32(1)), f32(1.0))   # id -1 -> 1
    T = np.ones(tid.shape[1], f32)
    for k in range(tid.shape[0]):
        T = T * p[tid[k]]
    assert T.dtype == np.float32
    return T


# ---------------------------------------------------------------------------------------------------------------------
# 1. transmittance against the library's own crossings
# ---------------------------------------------------------------------------------------------------------------------
ALPHAS = {"single": [0.5], "nest3": [0.25, 0.5, 0.75], "rings2": [0.75, 0.25], "nest8": [0.5, 0.0, 0.5, 1.0, 0.0, 0.5, 0.5, 0.0]}


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", list(ALPHAS))
def test_transmittance_is_the_product_over_the_crossings(tr, name, solver):
    s, alpha = ct.ray_set(name), ALPHAS[name]
    sc = scene_of(name, alpha)
    _, tid = crossings_dev(tr, sc, s["o"], s["d"], solver)
    want = product_over(tid, alpha)
    got, st = transmittance_dev(tr, sc, s["o"], s["d"], solver, stats=True)
    assert np.array_equal(u32(got), u32(want)), int((u32(got) != u32(want)).sum())
    assert len(np.unique(got)) >= (3 if name != "single" else 2) and (got < 1).mean() > 0.3
    n_t = len(alpha)
    assert st["primary_tests"] == st["bounce_tests"] == 0 and st["pixels"] == len(got)
    if name == "nest8":   # an opaque shell ends the query: fewer tori started than n x n_tori, at least one per ray
        assert (got == 0).any() and len(got) <= st["shadow_tests"] < len(got) * n_t
    else:                 # nothing is opaque: every torus of every ray is started
        assert st["shadow_tests"] == len(got) * n_t
    assert 0 < st["solved_tests"] <= st["traced_tests"] == st["shadow_tests"] and st["evaluations"] >= st["solved_tests"]


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
def test_transmittance_per_ray_bounds_and_empty_windows(tr, solver):
    s, alpha = ct.ray_set("nest3"), ALPHAS["nest3"]
    sc = scene_of("nest3", alpha)
    o, d, n = s["o"], s["d"], len(s["o"])
    whole = transmittance_dev(tr, sc, o, d, solver)
    # every bound = the scalar: the same bits through the other path
    assert np.array_equal(u32(transmittance_dev(tr, sc, o, d, solver, tmax=-1.0, bound=np.full(n, ct.TMAX, f32))), u32(whole))
    # a bound between crossing k - 1 and crossing k of the ray's own list (robust rays: neighbours >= 1e-3 apart) keeps
    # the first k crossings; every fifth ray gets an empty window (the bound at tmin, below it, or NaN)
    t, tid = crossings_dev(tr, sc, o, d, solver)
    cnt = (tid >= 0).sum(0)
    k = np.arange(n) % (cnt + 1)
    tt_ = np.concatenate([np.full((1, n), ct.TMIN, f32), t])          # row k: the crossing before the cut (tmin for k = 0)
    lo = tt_[k, np.arange(n)]
    hi = np.where(k < cnt, t[np.minimum(k, K_ALL - 1), np.arange(n)], lo + f32(1.0))
    bound = (lo + (hi - lo) * f32(0.5)).astype(f32)
    empty = np.arange(n) % 5 == 0
    bound[empty] = np.resize(f32([ct.TMIN, 0.0, np.nan, -np.inf, -3.0]), empty.sum())
    want = product_over(np.where(np.arange(K_ALL)[:, None] < k[None, :], tid, -1), alpha)
    want[empty] = 1.0
    got = transmittance_dev(tr, sc, o, d, solver, tmax=-1.0, bound=bound)
    ok = s["robust"] | empty
    assert np.array_equal(u32(got[ok]), u32(want[ok])), int((u32(got[ok]) != u32(want[ok])).sum())
    print(f"per-ray bounds: {int((u32(got) != u32(want)).sum())} non-robust rays differ")
    assert (u32(got[empty]) == u32(f32(1.0))).all() and (got[~empty] < whole[~empty]).sum() == 0 and (got != whole).mean() > 0.3
    # a window that is empty for every ray: T = 1 and no test executed
    for tmax in (ct.TMIN, np.nan, -1.0):
        T, st = transmittance_dev(tr, sc, o, d, solver, tmax=tmax, stats=True)
        assert (u32(T) == u32(f32(1.0))).all() and st["shadow_tests"] == st["traced_tests"] == 0, tmax


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", ["single", "nest3", "rings2"])
def test_opaque_transmittance_is_the_occluded_flag(tr, name, solver):
    import torch
    s = ct.ray_set(name)
    sc = scene_of(name, [1.0] * len(ct.SCENES[name][0]))
    T = transmittance_dev(tr, sc, s["o"], s["d"], solver)
    assert set(np.unique(T).tolist()) == {0.0, 1.0}
    keep, ptrs = upload(s["o"], s["d"])
    flag = torch.full((len(T),), 9, dtype=torch.uint8, device="cuda:0")
    tr.set_solver(solver)
    try:
        tr.occluded_dev(sc, ptrs, len(T), flag_ptr=flag.data_ptr(), tmin=ct.TMIN, tmax=ct.TMAX)
    finally:
        tr.set_solver(abi.TRT_SOLVE_F32)
        tr.set_torus_axes(None)
    torch.cuda.synchronize()
    hit = flag.cpu().numpy() == 1
    differ = (T == 0) != hit
    print(f"{name}: (T == 0) differs from the occluded flag on {int(differ.sum())} rays, all non-robust")
    assert not differ[s["robust"]].any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. one opaque torus: trt_shade_dev's colours
# ---------------------------------------------------------------------------------------------------------------------
MATERIALS = {"mirror": camera.MIRROR, "plastic": camera.PLASTIC, "matte": camera.MATTE, "flat": camera.FLAT}
_camera_rays = {}


def camera_rays(tr):
    if not _camera_rays:
        g = camera.baseline_camera(64, 64)
        o, d = tr.camera_rays(g, camera.baseline_push(1), 64, 64)
        o.setflags(write=False)
        d.setflags(write=False)
        _camera_rays["rays"] = (o, d)
    return _camera_rays["rays"]


def _robust_opaque(o, d, tori, mats, pc, axes):
    return tt.shade_through(o, d, tori, mats, [1.0] * len(tori), tt.push_dict(pc), axes)[1]


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("material", list(MATERIALS))
def test_one_opaque_torus_gives_shades_colours(tr, material, solver):
    """maxDepth 1 and 5, point and directional light, the torus on +y and on an axis of its own, 1 and 4 samples, on the
    render's primary rays of a 64x64 frame and on the `single` set.  A ray whose colour bits differ must be one the truth
    calls non-robust; where none differs the three ray-class counters are trt_shade_dev's."""
    geo = ct.SCENES["single"][0]
    co, cd = camera_rays(tr)
    s = ct.ray_set("single")
    differing = {}
    for axis in (None, (0.3, 1.0, -0.4)):
        sc = abi.Scene([(geo[0][0], geo[0][1], geo[0][2], 0)], [dict(MATERIALS[material], dissolve=1.0)], axes=None if axis is None else [axis])
        axes = None if axis is None else [axis]
        for depth, light in ((1, 0), (5, 0), (1, 1), (5, 1)) if axis is None else ((5, 0),):
            pc = abi.make_push(max_depth=depth, light_type=light)
            for rays, (o, d) in (("camera", (co, cd)), ("set", (s["o"], s["d"]))):
                for samples in (1, 4) if depth == 5 and light == 0 else (1,):
                    want, wst = shade_dev(tr, sc, o, d, pc, samples, solver, stats=True)
                    got, st = through_dev(tr, sc, o, d, pc, samples, solver, stats=True)
                    diff = (u32(got) != u32(want)).any(axis=1)
                    key = (rays, "axis" if axis else "+y", depth, light, samples)
                    differing[key] = int(diff.sum())
                    if diff.any():
                        idx = (np.flatnonzero(diff)[None, :] + (len(o) // samples) * np.arange(samples)[:, None]).reshape(-1)   # every sample of the outputs
                        robust = _robust_opaque(o[idx], d[idx], sc.tori_list(), tt.material_dicts(sc), pc, axes).reshape(samples, -1)
                        assert not robust.all(axis=0).any(), (key, int(robust.all(axis=0).sum()))
                    else:
                        assert {k: st[k] for k in QUERY_KEYS} == {k: wst[k] for k in QUERY_KEYS}, key
                    assert st["pixels"] == len(o) and st["primary_tests"] == len(o)
                    assert len(np.unique(u32(got), axis=0)) > 20, key
    print(f"{material}: outputs whose bits differ from trt_shade_dev: {differing}")
    assert all(v == 0 for k, v in differing.items() if k[0] == "camera"), differing


# ---------------------------------------------------------------------------------------------------------------------
# 3. several opaque tori: trt_shade_dev at the colour bars
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", ["nest3", "rings2"])
def test_opaque_scenes_give_shades_colours(tr, name, solver):
    s = ct.ray_set(name)
    geo, axes = ct.SCENES[name]
    mats = [camera.PLASTIC, camera.MIRROR, camera.MATTE][:len(geo)]
    if name == "nest3":
        mats = [camera.PLASTIC, camera.MATTE, camera.MIRROR]   # (torus 2 is the outermost shell: the mirror is seen)
    sc = scene_of(name, [1.0] * len(geo), mats)
    pc = camera.baseline_push(4)
    want = shade_dev(tr, sc, s["o"], s["d"], pc, solver=solver)
    got = through_dev(tr, sc, s["o"], s["d"], pc, solver=solver)
    robust = _robust_opaque(s["o"], s["d"], sc.tori_list(), tt.material_dicts(sc), pc, axes)
    print(f"{name}: {int((u32(got) != u32(want)).any(axis=1).sum())} rays differ in bits from trt_shade_dev, robust share {robust.mean():.3f}")
    assert robust.mean() > 0.9
    np.testing.assert_allclose(got[robust], want[robust], rtol=COLOR_RTOL, atol=COLOR_ATOL)
    assert len(np.unique(u32(got), axis=0)) > 100


# ---------------------------------------------------------------------------------------------------------------------
# 4. a transparent torus is absent
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
def test_a_transparent_torus_is_absent(tr, solver):
    s = ct.ray_set("nest3")
    mats = [camera.MIRROR, camera.PLASTIC, camera.MATTE]
    pc = camera.baseline_push(3)
    with_it = through_dev(tr, scene_of("nest3", [0.0, 0.5, 0.75], mats), s["o"], s["d"], pc, solver=solver)
    without = through_dev(tr, scene_of("nest3", [0.0, 0.5, 0.75], mats, only=(1, 2)), s["o"], s["d"], pc, solver=solver)
    assert np.array_equal(u32(with_it), u32(without))
    assert len(np.unique(u32(with_it), axis=0)) > 100
    T3 = transmittance_dev(tr, scene_of("nest3", [0.0, 0.5, 0.75]), s["o"], s["d"], solver)
    T2 = transmittance_dev(tr, scene_of("nest3", [0.0, 0.5, 0.75], only=(1, 2)), s["o"], s["d"], solver)
    assert np.array_equal(u32(T3), u32(T2))
    # every torus transparent: the miss colour of trt_shade_dev on every ray, and not one shadow ray
    pc = abi.make_push(clear=(0.3, 0.55, 0.7, 0.25), max_depth=3)
    got, st = through_dev(tr, scene_of("nest3", [0.0, -1.0, 0.0], mats), s["o"], s["d"], pc, solver=solver, stats=True)
    far = s["o"] + f32(100.0)   # rays that miss everything, through trt_shade_dev
    miss = shade_dev(tr, scene_of("nest3", [1.0, 1.0, 1.0], mats), far, np.tile(f32([0.0, 1.0, 0.0]), (len(far), 1)), pc, solver=solver)
    assert (u32(miss) == u32(miss[0])).all() and np.array_equal(u32(miss[0, :3]), u32(f32([0.3, 0.55, 0.7]) * f32(0.8)))
    assert (u32(got) == u32(miss[0])[None, :]).all()
    assert st["shadow_tests"] == 0 and st["bounce_tests"] == 0 and st["primary_tests"] == 3 * len(got)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the FP64 truth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", list(tt.cases()))
def test_against_the_fp64_truth(tr, name, solver):
    """The bars of tests/test_oracle.py's FP64 comparison: rel = |got - want| / (|want| + 1e-5), rel <= 1e-4 on at least
    99.5 % of the robust rays and max <= 2e-3."""
    c = tt.case(name)
    assert 1.0 - c["robust"].mean() <= c["cap"]
    got = through_dev(tr, c["sc"], c["o"], c["d"], c["pc"], solver=solver)[:, :3].astype(np.float64)
    meets_truth_bars(got, c, f"{name} {SOLVER_IDS[SOLVERS.index(solver)]}")
    miss = np.asarray(c["pc"].clearColor[:3]) * 0.8
    assert (np.abs(c["rgb"] - miss).max(1) > 1e-3).mean() > 0.5   # (most rays of a set see a shell)


# ---------------------------------------------------------------------------------------------------------------------
# 6. layout and paths
# ---------------------------------------------------------------------------------------------------------------------
def test_layout_and_both_forms(tr):
    import torch
    c = tt.case("nest3_mirror_core")
    sc, pc, o, d = c["sc"], c["pc"], c["o"], c["d"]
    n = len(o)
    dev = through_dev(tr, sc, o, d, pc)
    host = tr.shade_through(sc, o, d, pc)
    assert host.shape == (n, 4) and host.dtype == np.float32 and np.array_equal(u32(host), u32(dev))
    assert (u32(dev[:, 3]) == u32(f32(1.0))).all()
    Td = transmittance_dev(tr, sc, o, d)
    assert np.array_equal(u32(tr.transmittance(sc, o, d)), u32(Td))
    bound = np.linspace(0.5, 1.5, n).astype(f32)
    assert np.array_equal(u32(tr.transmittance(sc, o, d, tmax_per_ray=bound)), u32(transmittance_dev(tr, sc, o, d, tmax=-1.0, bound=bound)))
    # samples: trt_shade's rule — acc = c_0, then plain FP32 adds in order, one correctly rounded division
    for samples in (2, 4):
        got = through_dev(tr, sc, o, d, pc, samples=samples)
        parts = dev[:, :3].reshape(samples, n // samples, 3)
        acc = parts[0].copy()
        for k in range(1, samples):
            acc = acc + parts[k]
        want = acc / f32(samples)
        assert want.dtype == np.float32 and got.shape == (n // samples, 4)
        assert np.array_equal(u32(got[:, :3]), u32(want)) and np.array_equal(u32(got), u32(tr.shade_through(sc, o, d, pc, samples=samples)))
    # rays are independent: a permutation of the inputs permutes the outputs (cut ragged: 15 full blocks and 219 rays)
    perm = np.random.default_rng(11).permutation(n)[:n - 37]
    assert np.array_equal(u32(through_dev(tr, sc, o[perm], d[perm], pc)), u32(dev[perm]))
    assert np.array_equal(u32(transmittance_dev(tr, sc, o[perm], d[perm])), u32(Td[perm]))
    for m in (64, 1):
        assert np.array_equal(u32(through_dev(tr, sc, o[100:100 + m], d[100:100 + m], pc)), u32(dev[100:100 + m])), m
    # n == 0: nothing launched, nothing written
    z = np.zeros((0, 3), f32)
    assert tr.shade_through(sc, z, z, pc).shape == (0, 4) and tr.transmittance(sc, z, z).shape == (0,)
    buf = image(16)
    tr.shade_through_dev(sc, [0] * 6, 0, pc, buf.data_ptr())
    tr.transmittance_dev(sc, [0] * 6, 0, buf.data_ptr())
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == f32(SENTINEL)).all()


def test_capture_and_replay(tr):
    """Both _dev calls captured on one stream into a graph and replayed give the eager bits (kernel nodes only, no ctx
    scratch); an eager call with other opacities between the replays changes nothing."""
    import torch
    c = tt.case("nest3_all_through")
    sc, pc = c["sc"], c["pc"]
    n = 256 * 5 + 33
    o, d = c["o"][:2 * n], c["d"][:2 * n]
    eager = through_dev(tr, sc, o, d, pc, samples=2)
    eager_T = transmittance_dev(tr, sc, o, d)
    keep, ptrs = upload(o, d)
    buf, bufT = image(n * 4), image(2 * n)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            tr.shade_through_dev(sc, ptrs, 2 * n, pc, buf.data_ptr(), samples=2, stream=side.cuda_stream)
            tr.transmittance_dev(sc, ptrs, 2 * n, bufT.data_ptr(), stream=side.cuda_stream)
    cur.wait_stream(side)
    other = tt.case("single_half")
    for k in range(2):
        buf.fill_(SENTINEL)
        bufT.fill_(SENTINEL)
        gr.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u32(read(buf, n * 4).reshape(n, 4)), u32(eager)), k
        assert np.array_equal(u32(read(bufT, 2 * n)), u32(eager_T)), k
        through_dev(tr, other["sc"], other["o"][:500], other["d"][:500], other["pc"])   # an eager call in between
    assert len(np.unique(u32(eager), axis=0)) > 50 and len(np.unique(eager_T)) > 3


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable_and_the_outputs_unwritten(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    c = tt.case("single_half")
    sc, pc = c["sc"], c["pc"]
    n = 300
    o, d = c["o"][:n], c["d"][:n]
    want = through_dev(tr, sc, o, d, pc)
    want_T = transmittance_dev(tr, sc, o, d)
    keep, ptrs = upload(o, d)
    out = image(n * 4)
    host_out = np.full((n + 1, 4), SENTINEL, f32)
    L = tr._L
    rays = abi.rays_struct(ptrs, n)
    host_rays = abi.rays_struct([np.ascontiguousarray(a[:, k]) for a in (o, d) for k in range(3)], n)

    def good():
        assert np.array_equal(u32(through_dev(tr, sc, o, d, pc)), u32(want))
        assert np.array_equal(u32(transmittance_dev(tr, sc, o, d)), u32(want_T))

    def refused(call, who, *needles, code=abi.TRT_E_INVALID):
        with pytest.raises(TrtError) as e:
            call()
        assert e.value.code == code, str(e.value)
        for needle in (who,) + needles:
            assert needle in str(e.value), str(e.value)
        good()

    def refused_raw(rc, who):
        assert rc == abi.TRT_E_INVALID
        assert who in L.trt_last_error(tr._h)
        good()

    good()
    st = "trt_shade_through"
    refused(lambda: tr.shade_through_dev(sc, ptrs, n, pc, out.data_ptr(), samples=0), st, "samples")
    refused(lambda: tr.shade_through_dev(sc, ptrs, n, pc, out.data_ptr(), samples=7), st, "multiple")        # 300 % 7 != 0
    refused(lambda: tr.shade_through_dev(sc, ptrs, n, pc, out.data_ptr() + 4), st, "aligned")
    refused(lambda: tr.shade_through_dev(sc, ptrs, n, pc, 0), st, "NULL")
    refused(lambda: tr.shade_through_dev(sc, ptrs[:2] + [0] + ptrs[3:], n, pc, out.data_ptr()), st, "NULL ray stream")
    refused(lambda: tr.shade_through(sc, o, d, pc, samples=0), st, "samples")
    refused(lambda: tr.shade_through(sc, o, d, pc, samples=7), st, "multiple")
    refused(lambda: tr.transmittance_dev(sc, ptrs, n, 0), "trt_transmittance", "NULL")
    refused(lambda: tr.transmittance_dev(sc, ptrs[:4] + [0] + ptrs[5:], n, out.data_ptr()), "trt_transmittance", "NULL ray stream")
    scp, pcp, outp = C.byref(sc.c), C.byref(pc), C.c_void_p(out.data_ptr())
    refused_raw(L.trt_shade_through_dev(tr._h, None, 1, pcp, scp, outp, None), b"trt_shade_through")
    refused_raw(L.trt_shade_through_dev(tr._h, C.byref(rays), 1, None, scp, outp, None), b"trt_shade_through")
    refused_raw(L.trt_shade_through_dev(tr._h, C.byref(rays), 1, pcp, None, outp, None), b"scene")
    refused_raw(L.trt_shade_through(tr._h, C.byref(host_rays), 1, pcp, scp, None), b"trt_shade_through")
    refused_raw(L.trt_shade_through(tr._h, C.byref(host_rays), 1, pcp, scp, host_out.ctypes.data + 4), b"trt_shade_through")
    refused_raw(L.trt_transmittance_dev(tr._h, None, None, scp, 0.001, 1.0, outp, None), b"trt_transmittance")
    refused_raw(L.trt_transmittance_dev(tr._h, C.byref(rays), None, None, 0.001, 1.0, outp, None), b"scene")
    refused_raw(L.trt_transmittance(tr._h, C.byref(host_rays), None, scp, 0.001, 1.0, None), b"trt_transmittance")
    # the enumeration is the default solver's: every other one is refused, worded like trt_crossings' refusal
    for solver in (abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_DK_F64, abi.TRT_SOLVE_FERRARI_F32, abi.TRT_SOLVE_FERRARI_F64):
        tr.set_solver(solver)
        try:
            for call, who in ((lambda: tr.shade_through_dev(sc, ptrs, n, pc, out.data_ptr()), st),
                              (lambda: tr.shade_through(sc, o, d, pc), st),
                              (lambda: tr.transmittance_dev(sc, ptrs, n, out.data_ptr()), "trt_transmittance"),
                              (lambda: tr.transmittance(sc, o, d), "trt_transmittance")):
                with pytest.raises(TrtError) as e:
                    call()
                assert e.value.code == abi.TRT_E_INVALID and who in str(e.value), str(e.value)
                assert "the enumeration runs the default solver (TRT_SOLVE_F32 / _F64) only" in str(e.value)
        finally:
            tr.set_solver(abi.TRT_SOLVE_F32)
        good()
    # a NaN dissolve: TRT_E_SCENE from these calls, naming the material; trt_shade_dev does not read the field
    geo = ct.SCENES["single"][0]
    nan_sc = abi.Scene([(geo[0][0], geo[0][1], geo[0][2], 1)], [camera.MATTE, dict(camera.PLASTIC, dissolve=float("nan"))])
    refused(lambda: tr.shade_through_dev(nan_sc, ptrs, n, pc, out.data_ptr()), st, "material 1", "dissolve", code=abi.TRT_E_SCENE)
    refused(lambda: tr.transmittance_dev(nan_sc, ptrs, n, out.data_ptr()), "trt_transmittance", "material 1", "dissolve", code=abi.TRT_E_SCENE)
    refused(lambda: tr.shade_through(nan_sc, o, d, pc), st, "material 1", code=abi.TRT_E_SCENE)
    refused(lambda: tr.transmittance(nan_sc, o, d), "trt_transmittance", "material 1", code=abi.TRT_E_SCENE)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == f32(SENTINEL)).all() and (host_out == f32(SENTINEL)).all()   # a refused call writes nothing
    opaque = abi.Scene([(geo[0][0], geo[0][1], geo[0][2], 0)], [camera.PLASTIC])
    assert np.array_equal(u32(shade_dev(tr, nan_sc, o, d, pc)), u32(shade_dev(tr, opaque, o, d, pc)))
    assert L.trt_shade_through_dev(None, C.byref(rays), 1, pcp, scp, outp, None) == abi.TRT_E_INVALID
    assert L.trt_transmittance_dev(None, C.byref(rays), None, scp, 0.001, 1.0, outp, None) == abi.TRT_E_INVALID
    good()
