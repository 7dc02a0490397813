"""trt_shade_camera[_dev]: supersampled frames from camera rays made in registers (include/trt.h).

Three exact anchors, all on merged code: the image is what trt_camera_rays_dev followed by trt_shade_dev gives, bit for
bit, stats included; with one sample and no offsets it is trt_render_dev's image; with the regular 2x2 pattern it is the
2W x 2H render box-averaged in the stated order.  Then bands, both forms, capture, errors.

Frames are 100x68 and 52x36 (ragged last wave, waves that straddle rows); the band is rows [5, 61) of the first.
"""
import ctypes as C

import numpy as np
import pytest

import camera_truth
from camera_support import (BANDS, CAMERAS, SENTINEL, SHAPE_IDS, SHAPES, image, n_rays, ray_buffers, read_image, render_frame,
                            shade_camera_dev, stream_handle, u32)
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

W, H = SHAPES[0]
N = W * H
BAND = BANDS[H]
SOLVERS = [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64]
SOLVER_IDS = ["f32", "f64"]

# the frames of FRAMES in tests/test_gpu_shade.py (RENDERS of tests/test_gpu_parity.py, and the nests), restated
RENDERS = {
    "mirror_d1": lambda: (camera.single_torus_scene(), camera.baseline_camera(W, H), camera.baseline_push(1), 0),
    "mirror_d5": lambda: (camera.single_torus_scene(), camera.baseline_camera(W, H), camera.baseline_push(5), 0),
    "plastic_dir": lambda: (camera.single_torus_scene(material=camera.PLASTIC), camera.baseline_camera(W, H),
                            abi.make_push(max_depth=3, light_type=1), 0),
    "matte": lambda: (camera.single_torus_scene(material=camera.MATTE), camera.baseline_camera(W, H), camera.baseline_push(4), 0),
    "nested_d5": lambda: (camera.nested_tori_scene(), camera.baseline_camera(W, H), camera.baseline_push(5), 0),
    "toroidal_interior": lambda: (camera.single_torus_scene(R=6.0, r=1.5, material=camera.PLASTIC), camera.toroidal_camera(W, H),
                                  abi.make_push(max_depth=5, rho=4.0), 1),
    "toroidal_tilted": lambda: (camera.single_torus_scene(R=6.0, r=1.5, material=camera.MIRROR),
                                camera.toroidal_camera(W, H, eye=(0.5, 0.4, -0.3), center=(4.0, -1.0, 7.0)),
                                abi.make_push(max_depth=4, rho=3.0), 1),
}


def _nests():
    P, M = camera.PLASTIC, camera.MIRROR
    return [camera.nested_tori_scene(),
            abi.Scene([((0, 0, 0), 1.0, 0.4, 1), ((0, 0, 0), 1.05, 0.3, 0), ((0, 0.05, 0), 0.97, 0.2, 1), ((0, 0, 0), 1.0, 0.1, 0),
                       ((2.5, 0, 0), 0.6, 0.2, 1), ((2.5, 0, 0), 0.6, 0.1, 0)], [P, M]),
            abi.Scene([((0, 0, 0), 2.0, 1.2, 1), ((0, 0, 0), 2.0, 0.5, 1), ((0, 0, 0), 2.0, 0.2, 0)], [P, M])]


NEST_EYES = {"outside": (0.0, 1.5, -4.0), "between": (1.1, 0.0, 0.0)}   # the second one inside the outer tube of each nest


def _nest_frame(scene, eye, cam):
    def make():
        g = camera.globals_for(NEST_EYES[eye], (0.0, 0.0, 0.0) if cam == abi.TRT_CAMERA_PINHOLE else (3.0, 0.1, 0.5), W, H)
        pc = abi.make_push(max_depth=4, rho=0.3 if cam == abi.TRT_CAMERA_TOROIDAL else 0.0, light_type=int(eye == "between"))
        return _nests()[scene], g, pc, cam
    return make


FRAMES = dict(RENDERS)
for _s in (0, 1, 2):
    for _e in NEST_EYES:
        for _c in (abi.TRT_CAMERA_PINHOLE, abi.TRT_CAMERA_TOROIDAL):
            FRAMES[f"nest{_s}_{_e}_{'pinhole' if _c == 0 else 'toroidal'}"] = _nest_frame(_s, _e, _c)

# what the chain test runs on: a mirror, the toroidal camera with the theta branch, tori on axes of their own, a nest
# seen from between two shells with either camera
CHAIN = {
    "mirror_d5": FRAMES["mirror_d5"],
    "toroidal_tilted": FRAMES["toroidal_tilted"],
    "linked_rings": lambda: (camera.linked_rings_scene(), camera.linked_rings_camera(W, H), camera.baseline_push(5), 0),
    "nest0_between_pinhole": FRAMES["nest0_between_pinhole"],
    "nest1_between_toroidal": FRAMES["nest1_between_toroidal"],
}


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def offsets_for(samples, cam):
    """None for one sample, the regular grid for four, seeded offsets in (-0.5, 0.5) otherwise."""
    if samples == 1:
        return None
    if samples == 4:
        return camera_truth.grid_2x2(cam)
    return np.random.default_rng(samples).uniform(-0.5, 0.5, (samples, 2)).astype(np.float32)


def chain(tr, sc, g, pc, w, h, cam, samples, offsets, rows=None, solver=abi.TRT_SOLVE_F32):
    """trt_camera_rays_dev into device streams, then trt_shade_dev on them: the band's image (rows, w, 4) and the stats."""
    import torch
    r0, r1 = (0, h) if rows is None else rows
    n = n_rays(w, h, samples, rows)
    bufs = ray_buffers(n)
    ptrs = [b.data_ptr() for b in bufs]
    out = torch.full(((r1 - r0) * w * 4,), SENTINEL, dtype=torch.float32, device="cuda:0")
    tr.set_solver(solver)
    tr.enable_stats(True)
    try:
        tr.camera_rays_dev(g, pc, w, h, ptrs, camera=cam, samples=samples, offsets=offsets, rows=rows, stream=stream_handle())
        tr.shade_dev(sc, ptrs, n, pc, out.data_ptr(), samples=samples, stream=stream_handle())
        st = tr.stats()
    finally:
        tr.enable_stats(False)
        tr.set_solver(abi.TRT_SOLVE_F32)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(r1 - r0, w, 4), st


# ---------------------------------------------------------------------------------------------------------------------
# 1. the image is trt_camera_rays_dev -> trt_shade_dev
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("samples", [1, 4, 5])
@pytest.mark.parametrize("name", list(CHAIN))
def test_the_image_is_camera_rays_then_shade(tr, name, samples, solver):
    sc, g, pc, cam = CHAIN[name]()
    off = offsets_for(samples, cam)
    try:
        got, st = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=samples, offsets=off, solver=solver, stats=True)
        want, wst = chain(tr, sc, g, pc, W, H, cam, samples, off, solver=solver)
    finally:
        tr.set_torus_axes(None)
    diff = u32(got) != u32(want)
    assert not diff.any(), (name, int(diff.any(axis=2).sum()))
    assert st == wst and st["pixels"] == samples * N and st["primary_tests"] == samples * N * sc.n_tori
    assert (u32(got[..., 3]) == u32(np.float32(1.0))).all()
    miss = u32(np.float32(pc.clearColor[0]) * np.float32(0.8))
    assert (u32(got[..., 0]) != miss).mean() > 0.02   # the frame holds hits


@pytest.mark.parametrize("solver", [abi.TRT_SOLVE_DK_F32, abi.TRT_SOLVE_FERRARI_F64], ids=["dk32", "ferrari64"])
def test_alternative_solvers(tr, solver):
    sc, g, pc, cam = CHAIN["mirror_d5"]()
    off = offsets_for(4, cam)
    got, st = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=4, offsets=off, solver=solver, stats=True)
    want, wst = chain(tr, sc, g, pc, W, H, cam, 4, off, solver=solver)
    assert np.array_equal(u32(got), u32(want)) and st == wst
    assert len(np.unique(u32(got.reshape(-1, 4)), axis=0)) > 100


def test_the_average_is_not_a_sample(tr):
    """Four samples change the picture where the scene has an edge, and five seeded ones change it again."""
    sc, g, pc, cam = CHAIN["mirror_d5"]()
    one = shade_camera_dev(tr, sc, g, pc, W, H, cam)
    four = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=4, offsets=offsets_for(4, cam))
    five = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=5, offsets=offsets_for(5, cam))
    for a, b in ((one, four), (four, five)):
        assert 50 < (u32(a) != u32(b)).any(axis=2).sum() < N
    # the same offset twice over is the one-sample image: (c + c) / 2 is exact
    same = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=2, offsets=np.zeros((2, 2), np.float32))
    assert np.array_equal(u32(same), u32(one))


# ---------------------------------------------------------------------------------------------------------------------
# 2. one sample, no offsets: the render
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("name", list(FRAMES))
def test_one_sample_is_the_render(tr, name, solver):
    sc, g, pc, cam = FRAMES[name]()
    f = render_frame(tr, ("shade_camera", name), sc, g, pc, W, H, cam, solver=solver)
    got = shade_camera_dev(tr, sc, g, pc, W, H, cam, solver=solver)
    diff = u32(got) != u32(f["rgba"])
    assert not diff.any(), (name, int(diff.any(axis=2).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the 2x2 pattern: the double-resolution render, box-averaged
# ---------------------------------------------------------------------------------------------------------------------
DOUBLE = {
    "mirror_d5": lambda w, h: (camera.single_torus_scene(), camera.baseline_camera(w, h), camera.baseline_push(5), 0),
    "toroidal_mirror_d5": lambda w, h: (camera.single_torus_scene(R=6.0, r=1.5, material=camera.MIRROR),
                                        camera.toroidal_camera(w, h, eye=(0.5, 0.4, -0.3), center=(4.0, -1.0, 7.0)),
                                        abi.make_push(max_depth=5, rho=3.0), 1),
}


@pytest.mark.parametrize("solver", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", list(DOUBLE))
def test_2x2_is_the_double_resolution_render_box_averaged(tr, name, w, h, solver):
    sc, g, pc, cam = DOUBLE[name](w, h)
    f = render_frame(tr, ("double", name), sc, g, pc, 2 * w, 2 * h, cam, solver=solver)
    big = f["rgba"]                                             # (2h, 2w, 4)
    c = [big[ky::2, kx::2, :3] for ky in (0, 1) for kx in (0, 1)]   # sample s = 2*ky + kx
    want = (((c[0] + c[1]) + c[2]) + c[3]) / np.float32(4.0)
    assert want.dtype == np.float32 and want.shape == (h, w, 3)
    got = shade_camera_dev(tr, sc, g, pc, w, h, cam, samples=4, offsets=camera_truth.grid_2x2(cam), solver=solver)
    diff = u32(got[..., :3]) != u32(want)
    assert not diff.any(), (name, int(diff.any(axis=2).sum()))
    assert (u32(got[..., 3]) == u32(np.float32(1.0))).all()
    assert (u32(want) != u32(c[0])).any(axis=2).sum() > 50     # the average is not its first sample


# ---------------------------------------------------------------------------------------------------------------------
# 4. row bands, both forms, capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mirror_d5", "toroidal_tilted"])
def test_a_band_writes_only_its_rows(tr, name):
    sc, g, pc, cam = CHAIN[name]()
    off = offsets_for(4, cam)
    full = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=4, offsets=off)
    for rows in (BAND, (0, 1), (H - 1, H), (7, 7)):
        got = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=4, offsets=off, rows=rows)   # (sentinels outside: camera_support.read_image)
        assert np.array_equal(u32(got[rows[0]:rows[1]]), u32(full[rows[0]:rows[1]])), rows
    want, _ = chain(tr, sc, g, pc, W, H, cam, 4, off, rows=BAND)
    assert np.array_equal(u32(full[BAND[0]:BAND[1]]), u32(want))


@pytest.mark.parametrize("name", ["mirror_d5", "toroidal_tilted"])
def test_host_and_device_forms_agree(tr, name):
    sc, g, pc, cam = CHAIN[name]()
    off = offsets_for(4, cam)
    dev = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=4, offsets=off)
    host = tr.shade_camera(sc, g, pc, W, H, camera=cam, samples=4, offsets=off)
    assert host.shape == (H, W, 4) and host.dtype == np.float32 and np.array_equal(u32(host), u32(dev))
    assert np.array_equal(u32(tr.shade_camera(sc, g, pc, W, H, camera=cam)), u32(shade_camera_dev(tr, sc, g, pc, W, H, cam)))
    # a band through the host form: its rows of the caller's full-frame image, nothing else
    buf = np.full(N * 4 + 8, SENTINEL, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    img = np.frombuffer((C.c_float * (N * 4)).from_address(base), np.float32)
    o4 = abi.camera_offsets(off, 4).ctypes.data_as(abi.f32p)
    for rows in (BAND, (7, 7)):
        img[:] = SENTINEL
        assert tr._L.trt_shade_camera(tr._h, C.byref(g), C.byref(pc), tr._scene(sc), W, H, rows[0], rows[1], cam, 4, o4, base) == 0
        out = img.reshape(H, W, 4)
        assert np.array_equal(u32(out[rows[0]:rows[1]]), u32(dev[rows[0]:rows[1]]))
        assert (out[:rows[0]] == np.float32(SENTINEL)).all() and (out[rows[1]:] == np.float32(SENTINEL)).all()


@pytest.mark.parametrize("name", ["mirror_d5", "toroidal_tilted"])
def test_capture_and_replay(tr, name):
    import torch
    sc, g, pc, cam = CHAIN[name]()
    off = offsets_for(4, cam)
    eager = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=4, offsets=off, rows=BAND)
    buf = image(W, H)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            tr.shade_camera_dev(sc, g, pc, W, H, buf.data_ptr(), camera=cam, samples=4, offsets=off, rows=BAND, stream=side.cuda_stream)
    cur.wait_stream(side)
    for k in range(2):
        buf.fill_(SENTINEL)
        gr.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u32(read_image(buf, W, H, BAND)), u32(eager)), k
        g2, pc2, cam2 = CAMERAS["pinhole"](52, 36)
        shade_camera_dev(tr, camera.nested_tori_scene(), g2, pc2, 52, 36, cam2, samples=2, offsets=[[0.1, 0.2], [-0.3, 0.4]])   # an eager call in between
    assert len(np.unique(u32(eager[BAND[0]:BAND[1]].reshape(-1, 4)), axis=0)) > 50


def test_a_toroidal_capture_with_cold_tables_is_refused(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    sc, g, pc, cam = CHAIN["toroidal_tilted"]()
    shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=2, offsets=[[0.125, 0.25], [-0.375, 0.0]])
    buf = image(W, H)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            with pytest.raises(TrtError) as e:
                tr.shade_camera_dev(sc, g, pc, W, H, buf.data_ptr(), camera=cam, samples=2, offsets=[[0.125, 0.25], [-0.375, 0.5]],
                                    stream=side.cuda_stream)
            tr.shade_camera_dev(sc, g, pc, W, H, buf.data_ptr(), camera=cam, samples=2, offsets=[[0.125, 0.25], [-0.375, 0.0]],
                                stream=side.cuda_stream)
    cur.wait_stream(side)
    assert e.value.code == abi.TRT_E_INVALID and "captured" in str(e.value) and "tables" in str(e.value)
    gr.replay()
    torch.cuda.synchronize()
    want = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=2, offsets=[[0.125, 0.25], [-0.375, 0.0]])
    assert np.array_equal(u32(read_image(buf, W, H)), u32(want))


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_ctx_usable(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    sc, g, pc, cam = CHAIN["toroidal_tilted"]()
    off = offsets_for(4, cam)
    want = shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=4, offsets=off, rows=BAND)
    out = image(W, H)
    host = np.full(N * 4 + 8, SENTINEL, np.float32)
    hbase = host.ctypes.data + (-host.ctypes.data) % 16
    L = tr._L

    def good():
        assert np.array_equal(u32(shade_camera_dev(tr, sc, g, pc, W, H, cam, samples=4, offsets=off, rows=BAND)), u32(want))

    def refused(needle, W_=W, H_=H, rows=BAND, camera_=cam, samples=4, offsets=off, ptr=None):
        with pytest.raises(TrtError) as e:
            tr.shade_camera_dev(sc, g, pc, W_, H_, out.data_ptr() if ptr is None else ptr, camera=camera_, samples=samples,
                                offsets=offsets, rows=rows)
        assert e.value.code == abi.TRT_E_INVALID
        assert "trt_shade_camera" in str(e.value) and needle in str(e.value), str(e.value)
        good()

    def refused_raw(rc):
        assert rc == abi.TRT_E_INVALID
        assert b"trt_shade_camera" in L.trt_last_error(tr._h)
        good()

    refused("NULL", ptr=0)
    refused("aligned", ptr=out.data_ptr() + 4)
    refused("bad size", W_=0)
    refused("bad size", H_=0, rows=(0, 0))
    refused("rows", rows=(9, 8))
    refused("rows", rows=(5, H + 1))
    refused("unknown camera", camera_=2)
    refused("samples", samples=0, offsets=None)
    refused("samples", samples=abi.TRT_MAX_CAMERA_SAMPLES + 1, offsets=None)
    for bad in (np.nan, np.inf, -np.inf, 1.5, -1.0000001):
        for slot in (0, 7):
            o = off.copy().reshape(-1)
            o[slot] = bad
            refused("offset", offsets=o)
    refused("overflows", W_=0xffffffff, H_=0xffffffff, rows=(0, 0xffffffff), samples=64, offsets=None, camera_=abi.TRT_CAMERA_PINHOLE)
    gp, pcp, scp = C.byref(g), C.byref(pc), tr._scene(sc)
    o4 = abi.camera_offsets(off, 4).ctypes.data_as(abi.f32p)
    tail = (W, H, BAND[0], BAND[1], cam, 4, o4)
    outp = C.c_void_p(out.data_ptr())
    refused_raw(L.trt_shade_camera_dev(tr._h, None, pcp, scp, *tail, outp, None))
    refused_raw(L.trt_shade_camera_dev(tr._h, gp, None, scp, *tail, outp, None))
    refused_raw(L.trt_shade_camera_dev(tr._h, gp, pcp, scp, *tail, None, None))
    refused_raw(L.trt_shade_camera(tr._h, None, pcp, scp, *tail, hbase))
    refused_raw(L.trt_shade_camera(tr._h, gp, None, scp, *tail, hbase))
    refused_raw(L.trt_shade_camera(tr._h, gp, pcp, scp, *tail, None))
    refused_raw(L.trt_shade_camera(tr._h, gp, pcp, scp, *tail, hbase + 4))   # a misaligned host image
    assert L.trt_shade_camera_dev(tr._h, gp, pcp, None, *tail, outp, None) == abi.TRT_E_INVALID   # no scene
    good()
    assert L.trt_shade_camera_dev(None, gp, pcp, scp, *tail, outp, None) == abi.TRT_E_INVALID
    assert L.trt_shade_camera(None, gp, pcp, scp, *tail, hbase) == abi.TRT_E_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == np.float32(SENTINEL)).all() and (host == np.float32(SENTINEL)).all()   # a refused call writes nothing
