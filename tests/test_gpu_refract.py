"""trt_shade_refract[_dev] / trt_shade_refract_camera[_dev]: glass tori, refraction along caller and camera rays (include/trt.h).

Anchors, from the strictest down:
  1. trt_shade_dev — with no glass material in use the colours are its colours bit for bit on every ray, the three
     ray-class counters too;
  2. the fused camera form is trt_camera_rays_dev followed by trt_shade_refract_dev, bit for bit, stats included;
  3. the FP64 truth of tests/refract_truth.py at the bars of tests/test_oracle.py's FP64 comparison;
  4. index-matched black glass is the scene without the torus; a black filter ends in black.
Then the layout, the paths (host, device, captured) and the refusals.  Sets are crossings_truth's 4096 rays, frames 64x64.
"""
import ctypes as C

import numpy as np
import pytest

import camera_truth
import crossings_truth as ct
import refract_truth as rt
import through_truth as tt
from camera_support import n_rays, ray_buffers, stream_handle
from shade_support import (ALL_SOLVER_IDS, ALL_SOLVERS, QUERY_KEYS, SENTINEL, SOLVER_IDS, SOLVERS, camera_call, frame_image, image,
                           meets_truth_bars, rays_call, read, read_image, shade_dev, tr, u32, upload)  # noqa: F401 (tr: a fixture)
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

COLOR_RTOL, COLOR_ATOL = 1e-5, 1e-6   # the project's bars on colours (tests/test_gpu_parity.py)
W = H = 64
BAND = (5, 59)
f32 = np.float32


def refract_dev(tr, sc, o, d, pc, samples=1, solver=abi.TRT_SOLVE_F32, stats=False):
    return rays_call(tr, "shade_refract_dev", sc, o, d, pc, samples, solver, stats)


def refract_camera_dev(tr, sc, g, pc, cam, samples=1, offsets=None, rows=None, solver=abi.TRT_SOLVE_F32, stats=False):
    return camera_call(tr, "shade_refract_camera_dev", sc, g, pc, W, H, cam, samples, offsets, rows, solver, stats)


_camera_rays = {}


def camera_rays(tr):
    if not _camera_rays:
        o, d = tr.camera_rays(camera.baseline_camera(W, H), camera.baseline_push(1), W, H)
        o.setflags(write=False)
        d.setflags(write=False)
        _camera_rays["rays"] = (o, d)
    return _camera_rays["rays"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. no glass: trt_shade_dev, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
# illum 0, 2 and 3 only; "rings2" has the oriented tori, "nest3" the enclosure masks (the mirror is the outer shell)
NO_GLASS = {
    "nest3": ("nest3", [camera.FLAT, camera.PLASTIC, camera.MIRROR]),
    "rings2": ("rings2", [camera.MIRROR, camera.PLASTIC]),
    "single_flat": ("single", [camera.FLAT]),
}


@pytest.mark.parametrize("solver", ALL_SOLVERS, ids=ALL_SOLVER_IDS)
def test_without_glass_it_is_shade_bit_for_bit(tr, solver):
    """maxDepth 1 and 5, both light types, 1 and 4 samples, the render's primary rays of a 64x64 frame and the ray sets;
    ior = 0 and a NaN filter on those materials are not even looked at."""
    co, cd = camera_rays(tr)
    for name, (set_name, mats) in NO_GLASS.items():
        geo, axes = ct.SCENES[set_name]
        sc = abi.Scene([(C_, R, r, j) for j, (C_, R, r) in enumerate(geo)],
                       [dict(m, ior=0.0, transmittance=(float("nan"), -1.0, 0.0)) for m in mats], axes=axes)
        s = ct.ray_set(set_name)
        for depth, light in ((1, 0), (5, 0), (1, 1), (5, 1)):
            pc = abi.make_push(max_depth=depth, light_type=light)
            for rays, (o, d) in (("camera", (co, cd)), ("set", (s["o"], s["d"]))):
                for samples in (1, 4) if depth == 5 and light == 0 else (1,):
                    want, wst = shade_dev(tr, sc, o, d, pc, samples, solver, stats=True)
                    got, st = refract_dev(tr, sc, o, d, pc, samples, solver, stats=True)
                    key = (name, rays, depth, light, samples)
                    assert np.array_equal(u32(got), u32(want)), (key, int((u32(got) != u32(want)).any(axis=1).sum()))
                    assert {k: st[k] for k in QUERY_KEYS} == {k: wst[k] for k in QUERY_KEYS}, key
                    assert st["pixels"] == len(o) and st["primary_tests"] == len(o) * len(geo)
                    if rays == "set":
                        assert len(np.unique(u32(got), axis=0)) > 20, key


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fused camera form is camera_rays_dev -> shade_refract_dev
# ---------------------------------------------------------------------------------------------------------------------
def glass_frame(cam_name):
    """A glass shell around a plastic core, in front of the pinhole camera or around the toroidal one's line of sight."""
    if cam_name == "pinhole":
        tori = [((0.0, 0.0, 0.0), 1.0, 0.3, 0), ((0.0, 0.0, 0.0), 1.0, 0.12, 1)]
        g, pc, cam = camera.baseline_camera(W, H), camera.baseline_push(8), abi.TRT_CAMERA_PINHOLE
    else:
        tori = [((0.0, 0.0, 0.0), 6.0, 1.5, 0), ((0.0, 0.0, 0.0), 6.0, 0.6, 1)]
        g, pc, cam = (camera.toroidal_camera(W, H, eye=(0.5, 0.4, -0.3), center=(4.0, -1.0, 7.0)),
                      abi.make_push(max_depth=8, rho=3.0), abi.TRT_CAMERA_TOROIDAL)
    return abi.Scene(tori, [rt.glass(), camera.PLASTIC]), g, pc, cam


def chain(tr, sc, g, pc, cam, samples, offsets, rows, solver):
    """trt_camera_rays_dev into device streams, then trt_shade_refract_dev on them: the band's image and the stats."""
    import torch
    r0, r1 = (0, H) if rows is None else rows
    n = n_rays(W, H, samples, rows)
    bufs = ray_buffers(n)
    ptrs = [b.data_ptr() for b in bufs]
    out = torch.full(((r1 - r0) * W * 4,), SENTINEL, dtype=torch.float32, device="cuda:0")
    tr.set_solver(solver)
    tr.enable_stats(True)
    try:
        tr.camera_rays_dev(g, pc, W, H, ptrs, camera=cam, samples=samples, offsets=offsets, rows=rows, stream=stream_handle())
        tr.shade_refract_dev(sc, ptrs, n, pc, out.data_ptr(), samples=samples, stream=stream_handle())
        st = tr.stats()
    finally:
        tr.enable_stats(False)
        tr.set_solver(abi.TRT_SOLVE_F32)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(r1 - r0, W, 4), st


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("cam_name", ["pinhole", "toroidal"])
def test_the_fused_camera_is_camera_rays_then_shade_refract(tr, cam_name, samples, solver):
    sc, g, pc, cam = glass_frame(cam_name)
    off = None if samples == 1 else camera_truth.grid_2x2(cam)
    for rows in (None, BAND):
        got, st = refract_camera_dev(tr, sc, g, pc, cam, samples=samples, offsets=off, rows=rows, solver=solver, stats=True)
        want, wst = chain(tr, sc, g, pc, cam, samples, off, rows, solver)
        r0, r1 = (0, H) if rows is None else rows
        n_px = (r1 - r0) * W
        assert np.array_equal(u32(got[r0:r1]), u32(want)), (rows, int((u32(got[r0:r1]) != u32(want)).any(axis=2).sum()))
        assert st == wst and st["pixels"] == samples * n_px and st["primary_tests"] == samples * n_px * sc.n_tori
        assert st["bounce_tests"] > 0 and (u32(got[r0:r1, :, 3]) == u32(f32(1.0))).all()
    plain = shade_dev(tr, sc, *tr.camera_rays(g, pc, W, H, camera=cam), pc, solver=solver).reshape(H, W, 4)
    full = refract_camera_dev(tr, sc, g, pc, cam, solver=solver)
    assert (u32(full) != u32(plain)).any(axis=2).mean() > 0.05   # the glass is in the picture, and it bends


# ---------------------------------------------------------------------------------------------------------------------
# 3. the FP64 truth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", list(rt.cases()))
def test_against_the_fp64_truth(tr, name, solver):
    """The bars of tests/test_oracle.py's FP64 comparison: rel = |got - want| / (|want| + 1e-5), rel <= 1e-4 on at least
    99.5 % of the robust rays and max <= 2e-3."""
    c = rt.case(name)
    assert c["robust"].mean() > 0.9
    got = refract_dev(tr, c["sc"], c["o"], c["d"], c["pc"], solver=solver)[:, :3].astype(np.float64)
    meets_truth_bars(got, c, f"{name} {SOLVER_IDS[SOLVERS.index(solver)]}")
    miss = np.asarray(c["pc"].clearColor[:3]) * 0.8
    assert (np.abs(c["rgb"] - miss).max(1) > 1e-3).mean() > 0.5   # (most rays of a set see a surface)


# ---------------------------------------------------------------------------------------------------------------------
# 4. index-matched glass is invisible; a black filter ends in black
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
def test_index_matched_black_glass_is_invisible(tr, solver):
    """refract_truth.APART: two rings side by side, the light above the gap, so that the glass ring — an opaque shadow
    caster by the rule — shades nothing of the other.  Robust: the truth's flags of both scenes."""
    geo = rt.APART
    o, d = rt.rays_of((geo, None))
    ghost = dict(rt.BLACK, illum=7, ior=1.0, transmittance=(1.0, 1.0, 1.0))
    pc = abi.make_push(light_pos=rt.APART_LIGHT, max_depth=rt.MAX_DEPTH)
    both = abi.Scene([(geo[0][0], geo[0][1], geo[0][2], 0), (geo[1][0], geo[1][1], geo[1][2], 1)], [camera.PLASTIC, ghost])
    alone = abi.Scene([(geo[0][0], geo[0][1], geo[0][2], 0)], [camera.PLASTIC])
    _, r_both = rt.shade_refract(o, d, both.tori_list(), rt.material_dicts(both), tt.push_dict(pc))
    _, r_alone = rt.shade_refract(o, d, alone.tori_list(), rt.material_dicts(alone), tt.push_dict(pc))
    robust = r_both & r_alone
    got = refract_dev(tr, both, o, d, pc, solver=solver)
    want = shade_dev(tr, alone, o, d, pc, solver=solver)
    err = np.abs(got[robust] - want[robust]) - COLOR_RTOL * np.abs(want[robust])
    print(f"index-matched {SOLVER_IDS[SOLVERS.index(solver)]}: robust {robust.mean():.4f}, {int((u32(got) != u32(want)).any(axis=1).sum())} rays differ in bits, "
          f"worst |got - want| - rtol |want| = {err.max():.3e} (atol {COLOR_ATOL:g})")
    assert robust.mean() > 0.9
    np.testing.assert_allclose(got[robust], want[robust], rtol=COLOR_RTOL, atol=COLOR_ATOL)
    hit_plastic = np.abs(want[:, :3] - f32(0.8)).max(1) > 1e-3
    assert hit_plastic.mean() > 0.3 and len(np.unique(u32(got), axis=0)) > 100


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
def test_a_black_filter_on_black_glass_gives_exactly_zero(tr, solver):
    """Tf = 0 and a black glass torus: rgb is exactly 0 on every ray whose first hit (trt_trace's, with the same solver) is
    that torus entered from outside — whatever lies behind, the mirror and the miss colour included."""
    s = ct.ray_set("rings2")
    geo, axes = ct.SCENES["rings2"]
    dark = dict(rt.BLACK, illum=6, ior=1.5, transmittance=(0.0, 0.0, 0.0))
    sc = abi.Scene([(geo[0][0], geo[0][1], geo[0][2], 0), (geo[1][0], geo[1][1], geo[1][2], 1)], [dark, camera.MIRROR], axes=axes)
    pc = camera.baseline_push(8)
    tr.set_solver(solver)
    try:
        hits = tr.trace(sc, s["o"], s["d"])
    finally:
        tr.set_solver(abi.TRT_SOLVE_F32)
        tr.set_torus_axes(None)
    nd = hits["nx"] * s["d"][:, 0] + hits["ny"] * s["d"][:, 1] + hits["nz"] * s["d"][:, 2]
    into_glass = (hits["id"] == 0) & (nd < 0)
    got = refract_dev(tr, sc, s["o"], s["d"], pc, solver=solver)
    assert into_glass.mean() > 0.3
    assert (got[into_glass, :3] == 0.0).all(), int((got[into_glass, :3] != 0.0).any(axis=1).sum())
    assert (got[hits["id"] < 0, :3] != 0.0).all() and (u32(got[:, 3]) == u32(f32(1.0))).all()   # (a miss is the miss colour)


# ---------------------------------------------------------------------------------------------------------------------
# 5. layout and paths
# ---------------------------------------------------------------------------------------------------------------------
def test_layout_and_both_forms(tr):
    import torch
    c = rt.case("rings2_glass_mirror")
    sc, pc, o, d = c["sc"], c["pc"], c["o"], c["d"]
    n = len(o)
    dev = refract_dev(tr, sc, o, d, pc)
    host = tr.shade_refract(sc, o, d, pc)
    tr.set_torus_axes(None)
    assert host.shape == (n, 4) and host.dtype == np.float32 and np.array_equal(u32(host), u32(dev))
    assert (u32(dev[:, 3]) == u32(f32(1.0))).all()
    # samples: trt_shade's rule — acc = c_0, then plain FP32 adds in order, one correctly rounded division
    for samples in (2, 4):
        got = refract_dev(tr, sc, o, d, pc, samples=samples)
        parts = dev[:, :3].reshape(samples, n // samples, 3)
        acc = parts[0].copy()
        for k in range(1, samples):
            acc = acc + parts[k]
        want = acc / f32(samples)
        assert want.dtype == np.float32 and got.shape == (n // samples, 4)
        assert np.array_equal(u32(got[:, :3]), u32(want))
        assert np.array_equal(u32(got), u32(tr.shade_refract(sc, o, d, pc, samples=samples)))
        tr.set_torus_axes(None)
    # rays are independent: a permutation of the inputs permutes the outputs (cut ragged: 15 full blocks and 219 rays)
    perm = np.random.default_rng(11).permutation(n)[:n - 37]
    assert np.array_equal(u32(refract_dev(tr, sc, o[perm], d[perm], pc)), u32(dev[perm]))
    for m in (64, 1):
        assert np.array_equal(u32(refract_dev(tr, sc, o[100:100 + m], d[100:100 + m], pc)), u32(dev[100:100 + m])), m
    # the camera form: host == device, in the band and for the frame; rows outside the band of the host image are 0
    gsc, g, gpc, cam = glass_frame("toroidal")
    off = camera_truth.grid_2x2(cam)
    for rows in (None, BAND):
        devi = refract_camera_dev(tr, gsc, g, gpc, cam, samples=4, offsets=off, rows=rows)
        hosti = tr.shade_refract_camera(gsc, g, gpc, W, H, camera=cam, samples=4, offsets=off, rows=rows)
        r0, r1 = (0, H) if rows is None else rows
        assert np.array_equal(u32(hosti[r0:r1]), u32(devi[r0:r1])) and not hosti[:r0].any() and not hosti[r1:].any()
    # n == 0 and row_begin == row_end: nothing launched, nothing written
    z = np.zeros((0, 3), f32)
    assert tr.shade_refract(sc, z, z, pc).shape == (0, 4)
    assert not tr.shade_refract_camera(gsc, g, gpc, W, H, camera=cam, rows=(7, 7)).any()
    buf = image(16)
    tr.enable_stats(True)
    try:
        tr.shade_refract_dev(sc, [0] * 6, 0, pc, buf.data_ptr())
        st0 = tr.stats()
        tr.shade_refract_camera_dev(gsc, g, gpc, W, H, buf.data_ptr(), camera=cam, rows=(7, 7))
        st1 = tr.stats()
    finally:
        tr.enable_stats(False)
        tr.set_torus_axes(None)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == f32(SENTINEL)).all()
    for st in (st0, st1):
        assert st["pixels"] == 0 and all(st[k] == 0 for k in QUERY_KEYS)


def test_capture_and_replay(tr):
    """Both _dev calls captured on one stream into a graph and replayed twice give the eager bits (kernel nodes only, no ctx
    scratch but the toroidal tables: the toroidal call is made eagerly once first); an eager call with another scene
    between the replays changes nothing."""
    import torch
    c = rt.case("nest3_glass_shell")
    sc, pc = c["sc"], c["pc"]
    n = 256 * 5 + 33
    o, d = c["o"][:2 * n], c["d"][:2 * n]
    eager = refract_dev(tr, sc, o, d, pc, samples=2)
    gsc, g, gpc, cam = glass_frame("toroidal")
    off = camera_truth.grid_2x2(cam)
    eager_img = refract_camera_dev(tr, gsc, g, gpc, cam, samples=4, offsets=off, rows=BAND)   # (uploads the tables)
    keep, ptrs = upload(o, d)
    buf, img = image(n * 4), frame_image(W, H)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            tr.shade_refract_dev(sc, ptrs, 2 * n, pc, buf.data_ptr(), samples=2, stream=side.cuda_stream)
            tr.shade_refract_camera_dev(gsc, g, gpc, W, H, img.data_ptr(), camera=cam, samples=4, offsets=off, rows=BAND,
                                        stream=side.cuda_stream)
    cur.wait_stream(side)
    other = rt.case("single_glass")
    for k in range(2):
        buf.fill_(SENTINEL)
        img.fill_(SENTINEL)
        gr.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u32(read(buf, n * 4).reshape(n, 4)), u32(eager)), k
        assert np.array_equal(u32(read_image(img, W, H, BAND)), u32(eager_img)), k
        refract_dev(tr, other["sc"], other["o"][:500], other["d"][:500], other["pc"])   # an eager call in between
    assert len(np.unique(u32(eager), axis=0)) > 50


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable_and_the_outputs_unwritten(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    c = rt.case("single_glass")
    sc, pc = c["sc"], c["pc"]
    n = 300
    o, d = c["o"][:n], c["d"][:n]
    want = refract_dev(tr, sc, o, d, pc)
    gsc, g, gpc, cam = glass_frame("pinhole")
    want_img = refract_camera_dev(tr, gsc, g, gpc, cam)
    keep, ptrs = upload(o, d)
    out = image(n * 4)
    img = frame_image(W, H)
    host_out = np.full((n + 1, 4), SENTINEL, f32)
    L = tr._L
    rays = abi.rays_struct(ptrs, n)
    host_rays = abi.rays_struct([np.ascontiguousarray(a[:, k]) for a in (o, d) for k in range(3)], n)

    def good():
        assert np.array_equal(u32(refract_dev(tr, sc, o, d, pc)), u32(want))
        assert np.array_equal(u32(refract_camera_dev(tr, gsc, g, gpc, cam)), u32(want_img))

    def refused(call, who, *needles, code=abi.TRT_E_INVALID):
        with pytest.raises(TrtError) as e:
            call()
        assert e.value.code == code, str(e.value)
        for needle in (who + ":",) + needles:
            assert needle in str(e.value), str(e.value)
        good()

    def refused_raw(rc, who):
        assert rc == abi.TRT_E_INVALID
        assert who in L.trt_last_error(tr._h)
        good()

    good()
    sr, src = "trt_shade_refract", "trt_shade_refract_camera"
    # everything trt_shade* refuses, with this call's name
    refused(lambda: tr.shade_refract_dev(sc, ptrs, n, pc, out.data_ptr(), samples=0), sr, "samples")
    refused(lambda: tr.shade_refract_dev(sc, ptrs, n, pc, out.data_ptr(), samples=7), sr, "multiple")        # 300 % 7 != 0
    refused(lambda: tr.shade_refract_dev(sc, ptrs, n, pc, out.data_ptr() + 4), sr, "aligned")
    refused(lambda: tr.shade_refract_dev(sc, ptrs, n, pc, 0), sr, "NULL")
    refused(lambda: tr.shade_refract_dev(sc, ptrs[:2] + [0] + ptrs[3:], n, pc, out.data_ptr()), sr, "NULL ray stream")
    refused(lambda: tr.shade_refract(sc, o, d, pc, samples=0), sr, "samples")
    refused(lambda: tr.shade_refract(sc, o, d, pc, samples=7), sr, "multiple")
    scp, pcp, outp = C.byref(sc.c), C.byref(pc), C.c_void_p(out.data_ptr())
    refused_raw(L.trt_shade_refract_dev(tr._h, None, 1, pcp, scp, outp, None), b"trt_shade_refract:")
    refused_raw(L.trt_shade_refract_dev(tr._h, C.byref(rays), 1, None, scp, outp, None), b"trt_shade_refract:")
    refused_raw(L.trt_shade_refract_dev(tr._h, C.byref(rays), 1, pcp, None, outp, None), b"scene")
    refused_raw(L.trt_shade_refract(tr._h, C.byref(host_rays), 1, pcp, scp, None), b"trt_shade_refract:")
    refused_raw(L.trt_shade_refract(tr._h, C.byref(host_rays), 1, pcp, scp, host_out.ctypes.data + 4), b"trt_shade_refract:")
    # everything trt_shade_camera* refuses, with this call's name
    cam_dev = lambda **kw: tr.shade_refract_camera_dev(gsc, g, gpc, kw.pop("W", W), kw.pop("H", H), kw.pop("ptr", img.data_ptr()),
                                                       camera=kw.pop("camera", cam), **kw)
    refused(lambda: cam_dev(W=0), src, "bad size")
    refused(lambda: cam_dev(rows=(9, 5)), src, "bad size")
    refused(lambda: cam_dev(rows=(0, H + 1)), src, "bad size")
    refused(lambda: cam_dev(camera=5), src, "unknown camera")
    refused(lambda: cam_dev(samples=0), src, "samples")
    refused(lambda: cam_dev(samples=abi.TRT_MAX_CAMERA_SAMPLES + 1, offsets=np.zeros((abi.TRT_MAX_CAMERA_SAMPLES + 1, 2), f32)), src, "samples")
    refused(lambda: cam_dev(samples=2, offsets=f32([[0.0, 0.0], [1.5, 0.0]])), src, "offset")
    refused(lambda: cam_dev(samples=2, offsets=f32([[0.0, np.nan], [0.0, 0.0]])), src, "offset")
    refused(lambda: cam_dev(ptr=img.data_ptr() + 4), src, "aligned")
    refused(lambda: cam_dev(ptr=0), src, "NULL")
    refused(lambda: tr.shade_refract_camera(gsc, g, gpc, W, H, camera=5), src, "unknown camera")
    gp, gpcp, gscp, imgp = C.byref(g), C.byref(gpc), C.byref(gsc.c), C.c_void_p(img.data_ptr())
    refused_raw(L.trt_shade_refract_camera_dev(tr._h, None, gpcp, gscp, W, H, 0, H, cam, 1, None, imgp, None), b"trt_shade_refract_camera:")
    refused_raw(L.trt_shade_refract_camera_dev(tr._h, gp, None, gscp, W, H, 0, H, cam, 1, None, imgp, None), b"trt_shade_refract_camera:")
    refused_raw(L.trt_shade_refract_camera_dev(tr._h, gp, gpcp, None, W, H, 0, H, cam, 1, None, imgp, None), b"scene")
    # a glass material in use with a bad ior or filter: TRT_E_SCENE from these calls alone, naming the material
    geo = ct.SCENES["single"][0]
    torus = (geo[0][0], geo[0][1], geo[0][2], 1)
    nan, inf = float("nan"), float("inf")
    bad = [dict(ior=0.0), dict(ior=nan), dict(ior=inf), dict(ior=-1.5), dict(transmittance=(0.9, -0.1, 1.0)),
           dict(transmittance=(nan, 1.0, 1.0)), dict(transmittance=(1.0, 1.0, inf))]
    opaque = abi.Scene([(geo[0][0], geo[0][1], geo[0][2], 0)], [camera.PLASTIC])
    for fields in bad:
        word = "ior" if "ior" in fields else "transmittance"
        for illum in (6, 7):
            bad_sc = abi.Scene([torus], [camera.MATTE, dict(rt.glass(illum=illum), **fields)])
            refused(lambda: tr.shade_refract_dev(bad_sc, ptrs, n, pc, out.data_ptr()), sr, "material 1", word, code=abi.TRT_E_SCENE)
            refused(lambda: tr.shade_refract(bad_sc, o, d, pc), sr, "material 1", word, code=abi.TRT_E_SCENE)
            refused(lambda: tr.shade_refract_camera_dev(bad_sc, g, gpc, W, H, img.data_ptr(), camera=cam), src, "material 1", word, code=abi.TRT_E_SCENE)
            refused(lambda: tr.shade_refract_camera(bad_sc, g, gpc, W, H, camera=cam), src, "material 1", word, code=abi.TRT_E_SCENE)
        # trt_shade_dev reads neither field: the same scene is not refused
        assert np.array_equal(u32(shade_dev(tr, bad_sc, o, d, pc)), u32(shade_dev(tr, abi.Scene([torus], [camera.MATTE, rt.glass()]), o, d, pc)))
        # the same value on a material no torus uses, and on a material that is not glass, is accepted
        unused = abi.Scene([(geo[0][0], geo[0][1], geo[0][2], 0)], [rt.glass(), dict(rt.glass(), **fields)])
        assert np.array_equal(u32(refract_dev(tr, unused, o, d, pc)), u32(want))
        plain = abi.Scene([(geo[0][0], geo[0][1], geo[0][2], 0)], [dict(camera.PLASTIC, **fields)])
        assert np.array_equal(u32(refract_dev(tr, plain, o, d, pc)), u32(shade_dev(tr, opaque, o, d, pc)))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == f32(SENTINEL)).all() and (host_out == f32(SENTINEL)).all()   # a refused call writes nothing
    assert (img.cpu().numpy() == f32(SENTINEL)).all()
    assert L.trt_shade_refract_dev(None, C.byref(rays), 1, pcp, scp, outp, None) == abi.TRT_E_INVALID
    assert L.trt_shade_refract_camera_dev(None, gp, gpcp, gscp, W, H, 0, H, cam, 1, None, imgp, None) == abi.TRT_E_INVALID
    good()
