"""trt_shade_scene[_dev] / trt_shade_scene_camera[_dev]: the light table, the bound textures and glass in one call, and the
shadow query that lets light through glass (include/trt.h).

Anchors, from the strictest down — bits compared as uint32, counters primary_tests / bounce_tests / shadow_tests:
  1. lights=None, no glass, no texture in use: trt_shade_dev, for all six solvers; the host form is the dev form;
  2. lights=None, glass: trt_shade_refract_dev on refract_truth's cases;
  3. lights=None, textures: trt_shade_textured_dev on textured_truth's cases;
  4. a table, no glass, no textures: trt_shade_lit_dev on lights_truth's cases, area lights included;
  5. the flag without glass changes no bit and no counter; with glass of Tf = (0, 0, 0) it changes no colour bit and
     shadow_tests does not shrink;
  6. the fused camera forms are trt_camera_rays_dev followed by trt_shade_scene_dev, bit for bit, stats included;
  7. the FP64 truth of tests/scene_truth.py on the mixed cases, flag off and on, at the project's bars;
  8. capture and replay; the refusals.
Sets are crossings_truth's 4096 rays, frames 24x16 with the band (3, 13).
"""
import ctypes as C

import numpy as np
import pytest

import camera_truth
import crossings_truth as ct
import lights_truth as lt
import refract_truth as rt
import scene_truth as sct
import textured_truth as tt
from camera_support import n_rays, ray_buffers, stream_handle
from shade_support import (ALL_SOLVER_IDS, ALL_SOLVERS, SENTINEL, SOLVER_IDS, SOLVERS, camera_call, frame_image, image,
                           meets_truth_bars, rays_call, read, read_image, same, tr, u32, upload)  # noqa: F401 (tr: a fixture)
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

W, H = 24, 16
BAND = (3, 13)
f32 = np.float32


def scene_dev(tr, sc, o, d, pc, textures=None, **kw):
    """(`textures` bound around the call; without, nothing is bound)"""
    return rays_call(tr, "shade_scene_dev", sc, o, d, pc, textures=textures, **kw)


def scene_camera_dev(tr, sc, g, pc, cam, samples=1, offsets=None, rows=None, solver=abi.TRT_SOLVE_F32, stats=False, textures=None, **kw):
    return camera_call(tr, "shade_scene_camera_dev", sc, g, pc, W, H, cam, samples, offsets, rows, solver, stats, textures, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. nothing in use: trt_shade_dev
# ---------------------------------------------------------------------------------------------------------------------
PLAIN = {
    "nest3": ("nest3", [camera.FLAT, camera.PLASTIC, camera.MIRROR]),
    "rings2": ("rings2", [camera.MIRROR, camera.PLASTIC]),
}


@pytest.mark.parametrize("solver", ALL_SOLVERS, ids=ALL_SOLVER_IDS)
def test_nothing_in_use_is_shade_bit_for_bit(tr, solver):
    """Point and directional light of pc, 1 and 3 samples (4095 of the 4096 rays), depth 5; textures are bound, no
    material names one.  The flag changes nothing without glass; the host form is the dev form."""
    bound = tt.case("rings2_both")["tex"]
    for name, (set_name, mats) in PLAIN.items():
        geo, axes = ct.SCENES[set_name]
        sc = abi.Scene([(C_, R, r, j) for j, (C_, R, r) in enumerate(geo)], mats, axes=axes)
        s = ct.ray_set(set_name)
        o, d = s["o"][:4095], s["d"][:4095]
        for light_type in (0, 1):
            pc = abi.make_push(max_depth=5, light_type=light_type, light_pos=(3.0, 5.0, 2.0) if light_type else lt.BASELINE_LIGHT,
                               light_intensity=1.0 if light_type else 100.0)
            for samples in (1, 3):
                want = rays_call(tr, "shade_dev", sc, o, d, pc, samples, solver, stats=True)
                for flag in (False, True):
                    got = scene_dev(tr, sc, o, d, pc, samples=samples, solver=solver, stats=True, textures=bound, glass_shadows=flag)
                    same(got, want, (name, light_type, samples, flag))
                    assert got[1]["pixels"] == len(o) and got[1]["primary_tests"] == len(o) * len(geo)
            assert len(np.unique(u32(want[0]), axis=0)) > 20 and want[1]["shadow_tests"] > 0, (name, light_type)
        tr.set_solver(solver)
        try:
            host = tr.shade_scene(sc, o, d, pc, samples=3)
        finally:
            tr.set_solver(abi.TRT_SOLVE_F32)
            tr.set_torus_axes(None)
        assert host.shape == (1365, 4) and host.dtype == np.float32 and np.array_equal(u32(host), u32(want[0]))


# ---------------------------------------------------------------------------------------------------------------------
# 2. - 4. one ingredient in use: that ingredient's own call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", sorted(rt.cases()))
def test_glass_alone_is_shade_refract(tr, name, solver):
    c = rt.case(name)
    want = rays_call(tr, "shade_refract_dev", c["sc"], c["o"], c["d"], c["pc"], solver=solver, stats=True)
    got = scene_dev(tr, c["sc"], c["o"], c["d"], c["pc"], solver=solver, stats=True)
    same(got, want, name)
    assert want[1]["bounce_tests"] > 0


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", sorted(tt.cases()))
def test_textures_alone_are_shade_textured(tr, name, solver):
    c = tt.case(name)
    want = rays_call(tr, "shade_textured_dev", c["sc"], c["o"], c["d"], c["pc"], solver=solver, stats=True, textures=c["tex"])
    for flag in (False, True):
        got = scene_dev(tr, c["sc"], c["o"], c["d"], c["pc"], solver=solver, stats=True, textures=c["tex"], glass_shadows=flag)
        same(got, want, (name, flag))
    plain = rays_call(tr, "shade_dev", tt.case_scene(name, textured=False)[0], c["o"], c["d"], c["pc"], solver=solver)
    assert (u32(plain) != u32(want[0])).any(axis=1).mean() > 0.2   # (the textures are in the picture)


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", sorted(lt.cases()))
def test_a_table_alone_is_shade_lit(tr, name, solver):
    c = lt.case(name)
    kw = dict(lights=c["lights"], shadow_samples=c["K"], disc=c["disc"])
    want = rays_call(tr, "shade_lit_dev", c["sc"], c["o"], c["d"], c["pc"], solver=solver, stats=True, **kw)
    for flag in (False, True):
        got = scene_dev(tr, c["sc"], c["o"], c["d"], c["pc"], solver=solver, stats=True, glass_shadows=flag, **kw)
        same(got, want, (name, flag))
    assert want[1]["shadow_tests"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. the flag: black glass casts the opaque shadow; clear glass lets the light through
# ---------------------------------------------------------------------------------------------------------------------
def mixed_scene(name, tf=None):
    """The abi.Scene of a mixed case, its glass with another transmittance if `tf` is given."""
    sc, tori, axes, pc, mats, textures, lights, K = sct.case_scene(name)
    if tf is None:
        return sc
    mats = [dict(m, transmittance=tf) if m["illum"] in (6, 7) else m for m in mats]
    return abi.Scene(tori, mats, axes=axes)


def mixed_kw(c, flag):
    return dict(textures=c["tex"], lights=c["lights"], shadow_samples=c["K"], disc=c["disc"], glass_shadows=flag)


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", sct.MULTI_TORUS)
def test_black_glass_under_the_flag_casts_the_opaque_shadow(tr, name, solver):
    c = sct.case(name, False)
    black = mixed_scene(name, (0.0, 0.0, 0.0))
    off, soff = scene_dev(tr, black, c["o"], c["d"], c["pc"], solver=solver, stats=True, **mixed_kw(c, False))
    on, son = scene_dev(tr, black, c["o"], c["d"], c["pc"], solver=solver, stats=True, **mixed_kw(c, True))
    assert np.array_equal(u32(on), u32(off)), int((u32(on) != u32(off)).any(axis=1).sum())
    assert son["primary_tests"] == soff["primary_tests"] and son["bounce_tests"] == soff["bounce_tests"]
    assert son["shadow_tests"] >= soff["shadow_tests"] > 0
    # and with the case's own glass the light gets through: brighter on many rays, darker on none
    clear = scene_dev(tr, c["sc"], c["o"], c["d"], c["pc"], solver=solver, **mixed_kw(c, True))
    opaque = scene_dev(tr, c["sc"], c["o"], c["d"], c["pc"], solver=solver, **mixed_kw(c, False))
    assert ((clear[:, :3] - opaque[:, :3]).max(axis=1) > 1e-3).mean() >= 0.05
    assert (clear[:, :3] >= opaque[:, :3] - 1e-5).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the fused camera form is camera_rays_dev -> shade_scene_dev
# ---------------------------------------------------------------------------------------------------------------------
def mix_frame(cam_name):
    """A glass ring in front of a checker-textured plastic ring for the pinhole camera, or a textured plastic shell around
    a glass core about the toroidal one's line of sight; a soft key light, a coloured hard fill, K = 8."""
    glass = rt.glass(tf=sct.GLASS_TF)
    tex = tt.abi_textures([tt.texture(tt.checker_image(8, 4), (6.0, 2.0), False)])
    if cam_name == "pinhole":
        tori = [((0.0, 0.6, 0.0), 0.5, 0.12, 0), ((0.0, 0.0, 0.0), 1.0, 0.3, 1)]
        mats = [glass, dict(camera.PLASTIC, textureId=0)]
        g, pc, cam = camera.baseline_camera(W, H), camera.baseline_push(6), abi.TRT_CAMERA_PINHOLE
        lights = [abi.make_light(lt.BASELINE_LIGHT, radius=2.0), abi.make_light((-3.0, 4.0, -2.0), 20.0, (1.0, 0.8, 0.5))]
    else:
        tori = [((0.0, 0.0, 0.0), 6.0, 1.5, 0), ((0.0, 0.0, 0.0), 6.0, 0.6, 1)]
        mats = [dict(camera.PLASTIC, textureId=0), glass]
        g, pc, cam = (camera.toroidal_camera(W, H, eye=(0.5, 0.4, -0.3), center=(4.0, -1.0, 7.0)),
                      abi.make_push(max_depth=6, rho=3.0), abi.TRT_CAMERA_TOROIDAL)
        lights = [abi.make_light((0.0, 5.0, 0.0), 60.0, radius=1.5), abi.make_light((1.0, -2.0, 0.5), 8.0, (1.0, 0.8, 0.5))]
    return abi.Scene(tori, mats), g, pc, cam, lights, tex


def chain(tr, sc, g, pc, cam, lights, tex, flag, samples, offsets, rows, solver):
    """trt_camera_rays_dev into device streams, then trt_shade_scene_dev on them: the band's image and the stats."""
    import torch
    r0, r1 = (0, H) if rows is None else rows
    n = n_rays(W, H, samples, rows)
    bufs = ray_buffers(n)
    ptrs = [b.data_ptr() for b in bufs]
    out = torch.full(((r1 - r0) * W * 4,), SENTINEL, dtype=torch.float32, device="cuda:0")
    tr.set_solver(solver)
    tr.enable_stats(True)
    tr.set_textures(tex)
    try:
        tr.camera_rays_dev(g, pc, W, H, ptrs, camera=cam, samples=samples, offsets=offsets, rows=rows, stream=stream_handle())
        tr.shade_scene_dev(sc, ptrs, n, pc, out.data_ptr(), samples=samples, stream=stream_handle(), lights=lights, shadow_samples=8,
                           glass_shadows=flag)
        st = tr.stats()
        torch.cuda.synchronize()
    finally:
        tr.enable_stats(False)
        tr.set_solver(abi.TRT_SOLVE_F32)
        tr.set_textures(None)
    return out.cpu().numpy().reshape(r1 - r0, W, 4), st


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("cam_name", ["pinhole", "toroidal"])
def test_the_fused_camera_is_camera_rays_then_shade_scene(tr, cam_name, samples, solver):
    sc, g, pc, cam, lights, tex = mix_frame(cam_name)
    off = None if samples == 1 else camera_truth.grid_2x2(cam)
    kw = dict(textures=tex, lights=lights, shadow_samples=8)
    for rows in (None, BAND):
        for flag in (False, True):
            got, st = scene_camera_dev(tr, sc, g, pc, cam, samples=samples, offsets=off, rows=rows, solver=solver, stats=True,
                                       glass_shadows=flag, **kw)   # (read_image: rows outside the band keep the sentinel)
            want, wst = chain(tr, sc, g, pc, cam, lights, tex, flag, samples, off, rows, solver)
            r0, r1 = (0, H) if rows is None else rows
            n_px = (r1 - r0) * W
            assert np.array_equal(u32(got[r0:r1]), u32(want)), (rows, flag, int((u32(got[r0:r1]) != u32(want)).any(axis=2).sum()))
            assert st == wst and st["pixels"] == samples * n_px and st["primary_tests"] == samples * n_px * sc.n_tori
            assert st["shadow_tests"] > 0 and (u32(got[r0:r1, :, 3]) == u32(f32(1.0))).all()
    if samples == 1:
        on = scene_camera_dev(tr, sc, g, pc, cam, solver=solver, glass_shadows=True, **kw)
        offi = scene_camera_dev(tr, sc, g, pc, cam, solver=solver, glass_shadows=False, **kw)
        host = None
        tr.set_solver(solver)
        tr.set_textures(tex)
        try:
            host = tr.shade_scene_camera(sc, g, pc, W, H, camera=cam, rows=BAND, lights=lights, shadow_samples=8, glass_shadows=True)
        finally:
            tr.set_solver(abi.TRT_SOLVE_F32)
            tr.set_textures(None)
        assert np.array_equal(u32(host[BAND[0]:BAND[1]]), u32(on[BAND[0]:BAND[1]])) and not host[:BAND[0]].any() and not host[BAND[1]:].any()
        print(f"{cam_name}: the flag changes {int((u32(on) != u32(offi)).any(axis=2).sum())} of {W * H} pixels")


# ---------------------------------------------------------------------------------------------------------------------
# 7. the FP64 truth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("flag", [False, True], ids=["opaque", "through"])
@pytest.mark.parametrize("name", sorted(sct.cases()))
def test_against_the_fp64_truth(tr, name, flag, solver):
    """The project's bars: rel = |got - want| / (|want| + 1e-5), rel <= 1e-4 on at least 99.5 % of the robust rays and
    max <= 2e-3."""
    c = sct.case(name, flag)
    got = scene_dev(tr, c["sc"], c["o"], c["d"], c["pc"], solver=solver, **mixed_kw(c, flag))[:, :3].astype(np.float64)
    meets_truth_bars(got, c, f"{name} flag={flag} {SOLVER_IDS[SOLVERS.index(solver)]}")


# ---------------------------------------------------------------------------------------------------------------------
# 8. capture and replay; refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay(tr):
    """Both _dev calls captured on one stream into a graph and replayed twice give the eager bits (the toroidal call is
    made eagerly once first: it uploads the camera's tables); an eager call with another scene in between changes nothing."""
    import torch
    c = sct.case("nest3_glass_shell_area", True)
    n = 256 * 3 + 33
    o, d = c["o"][:2 * n], c["d"][:2 * n]
    eager = scene_dev(tr, c["sc"], o, d, c["pc"], samples=2, **mixed_kw(c, True))
    gsc, g, gpc, cam, glights, gtex = mix_frame("toroidal")
    # one binding for both calls: the frame's texture is texture 1 of it
    tex = list(c["tex"]) + list(gtex)
    gsc = abi.Scene([((0.0, 0.0, 0.0), 6.0, 1.5, 0), ((0.0, 0.0, 0.0), 6.0, 0.6, 1)],
                    [dict(camera.PLASTIC, textureId=1), rt.glass(tf=sct.GLASS_TF)])
    off = camera_truth.grid_2x2(cam)
    ckw = dict(lights=glights, shadow_samples=8, glass_shadows=True)
    eager_img = scene_camera_dev(tr, gsc, g, gpc, cam, samples=4, offsets=off, rows=BAND, textures=tex, **ckw)
    keep, ptrs = upload(o, d)
    buf, img = image(n * 4), frame_image(W, H)
    other = lt.case("single_three")
    tr.set_textures(tex)
    try:
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                tr.shade_scene_dev(c["sc"], ptrs, 2 * n, c["pc"], buf.data_ptr(), samples=2, stream=side.cuda_stream, lights=c["lights"],
                                   shadow_samples=c["K"], disc=c["disc"], glass_shadows=True)
                tr.shade_scene_camera_dev(gsc, g, gpc, W, H, img.data_ptr(), camera=cam, samples=4, offsets=off, rows=BAND,
                                          stream=side.cuda_stream, **ckw)
        cur.wait_stream(side)
        for k in range(2):
            buf.fill_(SENTINEL)
            img.fill_(SENTINEL)
            gr.replay()
            torch.cuda.synchronize()
            assert np.array_equal(u32(read(buf, n * 4).reshape(n, 4)), u32(eager)), k
            assert np.array_equal(u32(read_image(img, W, H, BAND)), u32(eager_img)), k
            tr.shade_scene_dev(other["sc"], ptrs, 500, other["pc"], image(500 * 4).data_ptr(), lights=other["lights"],
                               shadow_samples=other["K"], disc=other["disc"])   # an eager call in between
            torch.cuda.synchronize()
    finally:
        tr.set_textures(None)
        tr.set_torus_axes(None)
    assert len(np.unique(u32(eager), axis=0)) > 50


def test_refusals_leave_the_ctx_the_binding_and_the_outputs_as_they_were(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    c = sct.case("rings2_glass_over_textured", True)
    sc, pc, K, disc, lights = c["sc"], c["pc"], c["K"], c["disc"], c["lights"]
    n = 300
    o, d = c["o"][:n], c["d"][:n]
    want = scene_dev(tr, sc, o, d, pc, **mixed_kw(c, True))
    gsc, g, gpc, cam, glights, gtex = mix_frame("pinhole")
    gkw = dict(lights=glights, shadow_samples=8, glass_shadows=True)
    want_img = scene_camera_dev(tr, gsc, g, gpc, cam, textures=c["tex"], **gkw)
    keep, ptrs = upload(o, d)
    out, img = image(n * 4), frame_image(W, H)
    host_out = np.full((n + 1, 4), SENTINEL, f32)
    L = tr._L
    rays = abi.rays_struct(ptrs, n)
    sceneS, sceneC = "trt_shade_scene", "trt_shade_scene_camera"
    # the checker texture of both scenes is texture 0 of ONE binding, which the refused calls must leave in force
    tr.set_textures(c["tex"])

    def good():
        tr.set_torus_axes(None)
        got = image(n * 4)
        tr.shade_scene_dev(sc, ptrs, n, pc, got.data_ptr(), lights=lights, shadow_samples=K, disc=disc, glass_shadows=True)
        torch.cuda.synchronize()
        tr.set_torus_axes(None)
        assert np.array_equal(u32(read(got, n * 4).reshape(n, 4)), u32(want))

    def refused(call, code, *needles):
        with pytest.raises(TrtError) as e:
            call()
        assert e.value.code == code, str(e.value)
        for needle in needles:
            assert needle in str(e.value), str(e.value)
        good()

    try:
        good()
        lk = dict(lights=lights, shadow_samples=K, disc=disc)
        forms = [
            (sceneS, lambda s_, **kw: tr.shade_scene_dev(s_, ptrs, n, pc, out.data_ptr(), **kw)),
            (sceneS, lambda s_, **kw: tr.shade_scene(s_, o, d, pc, **kw)),
            (sceneC, lambda s_, **kw: tr.shade_scene_camera_dev(s_, g, gpc, W, H, img.data_ptr(), camera=cam, **kw)),
            (sceneC, lambda s_, **kw: tr.shade_scene_camera(s_, g, gpc, W, H, camera=cam, **kw)),
        ]
        base = dict(position=(1.0, 5.0, 2.0), intensity=50.0, color=(1.0, 1.0, 1.0), type=0, radius=0.5)
        mk = lambda **f: abi.make_light(**dict(base, **f))
        nan = float("nan")
        _, tori, axes, _, mats, _, _, _ = sct.case_scene("rings2_glass_over_textured")
        for who, call in forms:
            tr.set_torus_axes(None)
            # a bad flag
            for bad in (2, 3, 0x80000000):
                refused(lambda: call(sc, glass_shadows=bad, **lk), abi.TRT_E_INVALID, who + ":", "flags", "TRT_SCENE_GLASS_SHADOWS")
            # what trt_shade_lit refuses of a table
            refused(lambda: call(sc, lights=[mk()] * 9, shadow_samples=8), abi.TRT_E_INVALID, who + ":", "n_lights")
            refused(lambda: call(sc, lights=[mk(type=2)], shadow_samples=8), abi.TRT_E_INVALID, who + ":", "light 0", "type")
            refused(lambda: call(sc, lights=[mk(), mk(radius=-0.5)], shadow_samples=8), abi.TRT_E_INVALID, who + ":", "light 1", "radius")
            refused(lambda: call(sc, lights=[mk(position=(nan, 0.0, 0.0))], shadow_samples=8), abi.TRT_E_INVALID, who + ":", "position")
            refused(lambda: call(sc, lights=[mk(color=(1.0, nan, 1.0))], shadow_samples=8), abi.TRT_E_INVALID, who + ":", "color")
            refused(lambda: call(sc, lights=[mk(intensity=nan)], shadow_samples=8), abi.TRT_E_INVALID, who + ":", "intensity")
            refused(lambda: call(sc, lights=[mk()], shadow_samples=0), abi.TRT_E_INVALID, who + ":", "shadow_samples")
            refused(lambda: call(sc, lights=[mk()], shadow_samples=abi.TRT_MAX_LIGHT_SAMPLES + 1,
                                 disc=np.zeros((abi.TRT_MAX_LIGHT_SAMPLES + 1, 2), f32)), abi.TRT_E_INVALID, who + ":", "shadow_samples")
            bad_disc = abi.disc_samples(8)
            bad_disc[5, 1] = nan
            refused(lambda: call(sc, lights=[mk()], shadow_samples=8, disc=bad_disc), abi.TRT_E_INVALID, who + ":", "disc", "sample 5")
            # what trt_shade_textured refuses of a textureId
            for k in (1, 7, -2):
                far = abi.Scene(tori, [mats[0], dict(mats[1], textureId=k)], axes=axes)
                refused(lambda: call(far, **lk), abi.TRT_E_SCENE, who + ":", "material 1", "textureId")
            # what trt_shade_refract refuses of a glass material: an ior of 0 (a zero-initialised material), a bad filter
            for ior in (0.0, -1.5, nan, float("inf")):
                refused(lambda: call(abi.Scene(tori, [dict(mats[0], ior=ior), mats[1]], axes=axes), **lk), abi.TRT_E_SCENE, who + ":", "ior")
            refused(lambda: call(abi.Scene(tori, [dict(mats[0], transmittance=(0.5, -0.1, 0.5)), mats[1]], axes=axes), **lk),
                    abi.TRT_E_SCENE, who + ":", "transmittance")
        tr.set_torus_axes(None)
        # what trt_shade* / trt_shade_camera* refuse, with this call's name
        refused(lambda: tr.shade_scene_dev(sc, ptrs, n, pc, out.data_ptr(), samples=0, **lk), abi.TRT_E_INVALID, sceneS + ":", "samples")
        refused(lambda: tr.shade_scene_dev(sc, ptrs, n, pc, out.data_ptr(), samples=7, **lk), abi.TRT_E_INVALID, sceneS + ":", "multiple")
        refused(lambda: tr.shade_scene_dev(sc, ptrs, n, pc, out.data_ptr() + 4, **lk), abi.TRT_E_INVALID, sceneS + ":", "aligned")
        refused(lambda: tr.shade_scene_dev(sc, ptrs, n, pc, 0, **lk), abi.TRT_E_INVALID, sceneS + ":", "NULL")
        refused(lambda: tr.shade_scene_camera_dev(gsc, g, gpc, 0, H, img.data_ptr(), camera=cam, **gkw), abi.TRT_E_INVALID, sceneC + ":", "bad size")
        refused(lambda: tr.shade_scene_camera_dev(gsc, g, gpc, W, H, img.data_ptr(), camera=5, **gkw), abi.TRT_E_INVALID, sceneC + ":", "unknown camera")
        refused(lambda: tr.shade_scene_camera_dev(gsc, g, gpc, W, H, img.data_ptr(), camera=cam, samples=0, **gkw), abi.TRT_E_INVALID, sceneC + ":", "samples")
        refused(lambda: tr.shade_scene_camera_dev(gsc, g, gpc, W, H, img.data_ptr() + 4, camera=cam, **gkw), abi.TRT_E_INVALID, sceneC + ":", "aligned")
        # what the binding cannot express: a NULL table with n_lights > 0, a NULL disc with an area light
        one, keep_1 = abi.lights_struct([mk()], 8)
        pcp, scp, outp = C.byref(pc), C.byref(sc.c), C.c_void_p(out.data_ptr())
        for tbl, needle in ((abi.trt_lights(None, 2, 8, one.disc), b"NULL light table"), (abi.trt_lights(one.lights, 1, 8, None), b"NULL disc")):
            assert L.trt_shade_scene_dev(tr._h, C.byref(rays), 1, pcp, C.byref(tbl), 1, scp, outp, None) == abi.TRT_E_INVALID
            assert needle in L.trt_last_error(tr._h) and b"trt_shade_scene:" in L.trt_last_error(tr._h)
            good()
        assert L.trt_shade_scene_dev(None, C.byref(rays), 1, pcp, None, 0, scp, outp, None) == abi.TRT_E_INVALID
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == f32(SENTINEL)).all() and (host_out == f32(SENTINEL)).all()   # a refused call writes nothing
        assert (img.cpu().numpy() == f32(SENTINEL)).all()
        # the frame's scene under the same binding: the ctx renders as before
        got_img = frame_image(W, H)
        tr.shade_scene_camera_dev(gsc, g, gpc, W, H, got_img.data_ptr(), camera=cam, **gkw)
        torch.cuda.synchronize()
        assert np.array_equal(u32(read_image(got_img, W, H)), u32(want_img))
    finally:
        tr.set_textures(None)
        tr.set_torus_axes(None)
