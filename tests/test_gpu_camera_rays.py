"""trt_camera_rays[_dev]: the two cameras of trt_render* as ray streams with sub-pixel offsets (include/trt.h).

The anchors are exact and already merged: with zero offsets a ray is, bit for bit, the primary ray trt_render_dev exports
in RenderedData (and oracle.raygen's); with the regular 2x2 pattern the four rays of a pixel are pixel-centre rays of the
2W x 2H frame (tests/test_camera_rays_cpu.py has the arithmetic).  Arbitrary offsets are held to the project's 1e-5 bar
against an FP64 restatement (tests/camera_truth.py).  The rest is what the call adds: bands, optional streams, both
forms, capture, the render's table key left alone, errors, counters left alone.

Frames are 100x68 and 52x36: widths that are no multiple of 8 or 64 (the last wave of a sample is ragged, and a wave
straddles rows), 27 and 8 blocks per sample.
"""
import ctypes as C

import numpy as np
import pytest

import camera_truth
from camera_support import (BANDS, CAMERAS, PAD, SENTINEL, SHAPE_IDS, SHAPES, n_rays, ray_buffers, rays_dev, read_rays, render_frame,
                            scene_for, stream_handle, u32)
from toroidal_ray_tracing_amd import abi

pytestmark = pytest.mark.gpu

W, H = SHAPES[0]
BAND = BANDS[H]


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def rendered(tr, name, w, h):
    g, pc, cam = CAMERAS[name](w, h)
    f = render_frame(tr, name, scene_for(cam), g, pc, w, h, cam)
    assert np.isfinite(f["o"]).all() and np.isfinite(f["d"]).all()   # the anchors are stated for NaN-free frames
    return f


def same_rays(got, want):
    return all(np.array_equal(u32(a), u32(b)) for a, b in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# 1. zero offsets: the render's rays, the oracle's rays
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_zero_offsets_are_the_renders_rays(tr, oracle, name, w, h):
    g, pc, cam = CAMERAS[name](w, h)
    f = rendered(tr, name, w, h)
    o, d = rays_dev(tr, g, pc, w, h, cam)
    assert o.shape == d.shape == (w * h, 3)
    assert same_rays((o, d), (f["o"], f["d"]))
    zeros = rays_dev(tr, g, pc, w, h, cam, offsets=np.zeros((1, 2), np.float32))   # explicit zeros are NULL offsets
    assert same_rays(zeros, (o, d))
    want = np.array([np.concatenate(oracle.raygen(g, pc, w, h, cam, x, y)) for y in range(h) for x in range(w)])
    assert same_rays((o, d), (want[:, :3], want[:, 3:]))
    assert len(np.unique(u32(d), axis=0)) > 0.9 * w * h   # (nearly) every pixel has a direction of its own


# ---------------------------------------------------------------------------------------------------------------------
# 2. the 2x2 pattern: the double-resolution render, de-interleaved
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_2x2_offsets_are_the_double_resolution_renders_rays(tr, name, w, h):
    g, pc, cam = CAMERAS[name](w, h)
    g2, pc2, _ = CAMERAS[name](2 * w, 2 * h)
    assert bytes(g) == bytes(g2) and bytes(pc) == bytes(pc2)   # the same camera (aspect ratio 2W / 2H = W / H, exactly)
    f = rendered(tr, name, 2 * w, 2 * h)
    o, d = rays_dev(tr, g, pc, w, h, cam, samples=4, offsets=camera_truth.grid_2x2(cam))
    idx = camera_truth.double_frame_index(w, h).reshape(-1)    # [s][i] -> pixel of the 2W x 2H frame, s = 2*ky + kx
    assert o.shape == (4 * w * h, 3) and same_rays((o, d), (f["o"][idx], f["d"][idx]))
    assert sorted(idx) == list(range(4 * w * h))               # every ray of the big frame, once


# ---------------------------------------------------------------------------------------------------------------------
# 3. row bands, optional streams, both forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", ["pinhole", "toroidal_theta"])
def test_a_band_is_the_slice_of_the_full_call(tr, name, w, h):
    g, pc, cam = CAMERAS[name](w, h)
    off = camera_truth.grid_2x2(cam)
    full = [a.reshape(4, h, w, 3) for a in rays_dev(tr, g, pc, w, h, cam, samples=4, offsets=off)]
    r0, r1 = BANDS[h]
    band = rays_dev(tr, g, pc, w, h, cam, samples=4, offsets=off, rows=(r0, r1))
    assert band[0].shape == (4 * (r1 - r0) * w, 3)   # compact: sample s of the band starts at s * n_px
    assert same_rays(band, [a[:, r0:r1].reshape(-1, 3) for a in full])
    for rows in ((0, 1), (h - 1, h)):                # one row: less than a block per sample
        got = rays_dev(tr, g, pc, w, h, cam, samples=4, offsets=off, rows=rows)
        assert same_rays(got, [a[:, rows[0]:rows[1]].reshape(-1, 3) for a in full])
    empty = rays_dev(tr, g, pc, w, h, cam, samples=4, offsets=off, rows=(7, 7))   # valid, launches nothing (pads checked)
    assert empty[0].shape == (0, 3)


def test_null_streams_are_skipped(tr):
    g, pc, cam = CAMERAS["toroidal_theta"](W, H)
    off = camera_truth.grid_2x2(cam)
    o, d = rays_dev(tr, g, pc, W, H, cam, samples=4, offsets=off, rows=BAND)
    every = np.concatenate([o, d], 1)
    for want in ((1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1), (0, 1, 0, 1, 1, 0), (1, 1, 1, 0, 0, 0)):
        got = np.concatenate(rays_dev(tr, g, pc, W, H, cam, samples=4, offsets=off, rows=BAND, want=want), 1)   # (guards: camera_support.read_rays)
        for k in range(6):
            assert np.array_equal(u32(got[:, k]), u32(every[:, k])) if want[k] else (got[:, k] == np.float32(SENTINEL)).all(), (want, k)


@pytest.mark.parametrize("name", list(CAMERAS))
def test_host_and_device_forms_agree(tr, name):
    g, pc, cam = CAMERAS[name](W, H)
    off = camera_truth.grid_2x2(cam)
    for samples, offsets, rows in ((1, None, None), (4, off, BAND), (4, off, (7, 7))):
        host = tr.camera_rays(g, pc, W, H, camera=cam, samples=samples, offsets=offsets, rows=rows)
        assert host[0].dtype == np.float32 and host[0].shape == host[1].shape == (n_rays(W, H, samples, rows), 3)
        assert same_rays(host, rays_dev(tr, g, pc, W, H, cam, samples=samples, offsets=offsets, rows=rows))
    # the host form skips NULL streams too, and writes nothing behind the ones it fills
    n = n_rays(W, H, 4, BAND)
    bufs = [np.full(n + PAD, SENTINEL, np.float32) for _ in range(6)]
    out = abi.rays_out_struct([bufs[0], None, None, None, bufs[4], None])
    o4 = abi.camera_offsets(off, 4)
    assert tr._L.trt_camera_rays(tr._h, C.byref(g), C.byref(pc), W, H, BAND[0], BAND[1], cam, 4, o4.ctypes.data_as(abi.f32p), C.byref(out)) == 0
    want = rays_dev(tr, g, pc, W, H, cam, samples=4, offsets=off, rows=BAND)
    assert np.array_equal(u32(bufs[0][:n]), u32(want[0][:, 0])) and np.array_equal(u32(bufs[4][:n]), u32(want[1][:, 1]))
    assert all((b[n:] == np.float32(SENTINEL)).all() for b in bufs) and all((bufs[k] == np.float32(SENTINEL)).all() for k in (1, 2, 3, 5))


# ---------------------------------------------------------------------------------------------------------------------
# 4. capture and replay
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pinhole", "toroidal_theta"])
def test_capture_and_replay(tr, name):
    """A captured call replays the eager bits (kernel nodes only; the toroidal tables are on the device from the eager call)."""
    import torch
    g, pc, cam = CAMERAS[name](W, H)
    off = camera_truth.grid_2x2(cam)
    eager = rays_dev(tr, g, pc, W, H, cam, samples=4, offsets=off, rows=BAND)
    n = n_rays(W, H, 4, BAND)
    bufs = ray_buffers(n)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            tr.camera_rays_dev(g, pc, W, H, [b.data_ptr() for b in bufs], camera=cam, samples=4, offsets=off, rows=BAND, stream=side.cuda_stream)
    cur.wait_stream(side)
    for k in range(2):
        for b in bufs:
            b.fill_(SENTINEL)
        gr.replay()
        torch.cuda.synchronize()
        assert same_rays(read_rays(bufs, n), eager), k
        g2, pc2, cam2 = CAMERAS["pinhole"](52, 36)
        rays_dev(tr, g2, pc2, 52, 36, cam2, samples=2, offsets=[[0.1, 0.2], [-0.3, 0.4]])   # an eager call in between


def test_a_toroidal_capture_with_cold_tables_is_refused(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    g, pc, cam = CAMERAS["toroidal"](W, H)
    warm = np.float32([[0.125, 0.25], [-0.375, 0.0]])
    cold = np.float32([[0.125, 0.25], [-0.375, 0.03125]])   # one offset differs: other tables
    eager = rays_dev(tr, g, pc, W, H, cam, samples=2, offsets=warm)
    n = n_rays(W, H, 2, None)
    bufs = ray_buffers(n)
    ptrs = [b.data_ptr() for b in bufs]
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            with pytest.raises(TrtError) as e:
                tr.camera_rays_dev(g, pc, W, H, ptrs, camera=cam, samples=2, offsets=cold, stream=side.cuda_stream)
            tr.camera_rays_dev(g, pc, W, H, ptrs, camera=cam, samples=2, offsets=warm, stream=side.cuda_stream)   # the warm one records
    cur.wait_stream(side)
    assert e.value.code == abi.TRT_E_INVALID
    assert "captured" in str(e.value) and "tables" in str(e.value) and "eagerly" in str(e.value)
    gr.replay()
    torch.cuda.synchronize()
    assert same_rays(read_rays(bufs, n), eager)
    assert same_rays(rays_dev(tr, g, pc, W, H, cam, samples=2, offsets=cold), rays_dev(tr, g, pc, W, H, cam, samples=2, offsets=cold))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the render's tables and their key are not touched
# ---------------------------------------------------------------------------------------------------------------------
def test_the_renders_table_key_is_undisturbed(tr):
    """A toroidal render, a trt_camera_rays call with offsets on the same camera (and one on another frame shape), the
    render again: the same image and the same rays, and the camera rays are not disturbed by the render either."""
    import torch
    g, pc, cam = CAMERAS["toroidal_theta"](W, H)
    sc = scene_for(cam)
    first = rendered(tr, "toroidal_theta", W, H)
    off = np.float32([[0.4, -0.3], [-0.2, 0.45], [0.0, 0.0]])
    rays = rays_dev(tr, g, pc, W, H, cam, samples=3, offsets=off)
    assert same_rays([a[2 * W * H:] for a in rays], (first["o"], first["d"]))   # the sample at (0, 0) is the render's ray
    assert not np.array_equal(u32(rays[1][:W * H]), u32(first["d"]))
    g2, pc2, cam2 = CAMERAS["toroidal"](52, 36)
    rays_dev(tr, g2, pc2, 52, 36, cam2, samples=2, offsets=[[0.5, 0.5], [0.25, 0.0]])
    dev = torch.device("cuda:0")
    for k in range(3):   # (the third frame of a key reuses the tile lists: the reuse sees no change either)
        rgba = torch.full((H, W, 4), -5.0, device=dev)
        rd = torch.full((W * H, 16), -5.0, device=dev)
        tr.render_dev(sc, g, pc, W, H, rgba.data_ptr(), camera=cam, rendered_ptr=rd.data_ptr(), stream=stream_handle())
        torch.cuda.synchronize()
        assert np.array_equal(u32(rgba.cpu().numpy()), u32(first["rgba"])), k
        rec = rd.cpu().numpy().reshape(W, H, 16).transpose(1, 0, 2).reshape(H * W, 16)
        assert same_rays((rec[:, 8:11], rec[:, 12:15]), (first["o"], first["d"])), k
    assert same_rays(rays_dev(tr, g, pc, W, H, cam, samples=3, offsets=off), rays)


def test_the_counters_of_the_last_counted_call_stay(tr):
    g, pc, cam = CAMERAS["pinhole"](W, H)
    f = rendered(tr, "pinhole", W, H)
    import torch
    soa = [torch.from_numpy(np.ascontiguousarray(a[:, k])).to("cuda:0") for a in (f["o"], f["d"]) for k in range(3)]
    img = torch.empty(W * H * 4, device="cuda:0")
    tr.enable_stats(True)
    try:
        tr.shade_dev(scene_for(cam), [a.data_ptr() for a in soa], W * H, pc, img.data_ptr(), stream=stream_handle())
        before = tr.stats()
        rays_dev(tr, g, pc, W, H, cam, samples=4, offsets=camera_truth.grid_2x2(cam))
        assert tr.stats() == before and before["pixels"] == W * H and before["primary_tests"] == W * H
    finally:
        tr.enable_stats(False)


# ---------------------------------------------------------------------------------------------------------------------
# 6. arbitrary offsets against FP64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_arbitrary_offsets_against_fp64(tr, oracle, name, w, h):
    """Seeded offsets in (-0.5, 0.5), five samples, a band: positions within 1e-5 * max(1, |rho|, |eye|), directions (unit
    vectors for both cameras) within 1e-5 of the FP64 restatement built on the oracle's FP32 camera frame."""
    g, pc, cam = CAMERAS[name](w, h)
    rng = np.random.default_rng(20 + w)
    off = rng.uniform(-0.5, 0.5, (5, 2)).astype(np.float32)
    assert (np.abs(off) < 0.5).all() and (off != 0).all()
    fr = oracle.toroidal_frame(g, pc)
    if cam == abi.TRT_CAMERA_TOROIDAL:
        assert (fr["theta"] != 0.0) == (name == "toroidal_theta")
    rows = BANDS[h]
    o, d = rays_dev(tr, g, pc, w, h, cam, samples=5, offsets=off, rows=rows)
    wo, wd = camera_truth.camera_rays(g, pc, w, h, cam, off, rows=rows, frame=fr)
    eo, ed = np.abs(o - wo).max(), np.abs(d - wd).max()
    bar = camera_truth.RAY_RTOL * camera_truth.scale(pc, fr["eye"] if cam == abi.TRT_CAMERA_TOROIDAL else wo[0])
    print(f"{name} {w}x{h}: origin error {eo:.3e} (bar {bar:.3e}), direction error {ed:.3e} (bar {camera_truth.RAY_RTOL:.0e})")
    assert eo <= bar and ed <= camera_truth.RAY_RTOL
    assert np.abs(np.linalg.norm(wd, axis=1) - 1.0).max() < 1e-6   # (pinhole: as far as the FP32 viewInverse is a rotation)
    # the offsets are felt: a sample differs from the zero-offset ray by far more than the bar
    zo, zd = camera_truth.camera_rays(g, pc, w, h, cam, None, rows=rows, frame=fr)
    assert np.abs(wd[:len(zd)] - zd).max() > 100 * camera_truth.RAY_RTOL


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_ctx_usable(tr):
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    g, pc, cam = CAMERAS["toroidal_theta"](W, H)
    off = camera_truth.grid_2x2(cam)
    want = rays_dev(tr, g, pc, W, H, cam, samples=4, offsets=off, rows=BAND)
    n = n_rays(W, H, 4, BAND)
    bufs = ray_buffers(n)
    ptrs = [b.data_ptr() for b in bufs]
    host = [np.full(n, SENTINEL, np.float32) for _ in range(6)]
    L = tr._L

    def good():
        assert same_rays(rays_dev(tr, g, pc, W, H, cam, samples=4, offsets=off, rows=BAND), want)

    def refused(needle, W_=W, H_=H, rows=BAND, camera=cam, samples=4, offsets=off, out_ptrs=ptrs):
        for call in (lambda: tr.camera_rays_dev(g, pc, W_, H_, out_ptrs, camera=camera, samples=samples, offsets=offsets, rows=rows),):
            with pytest.raises(TrtError) as e:
                call()
            assert e.value.code == abi.TRT_E_INVALID
            assert "trt_camera_rays" in str(e.value) and needle in str(e.value), str(e.value)
        good()

    def refused_raw(rc):
        assert rc == abi.TRT_E_INVALID
        assert b"trt_camera_rays" in L.trt_last_error(tr._h)
        good()

    refused("all six streams NULL", out_ptrs=[0] * 6)
    refused("bad size", W_=0)
    refused("bad size", H_=0, rows=(0, 0))
    refused("rows", rows=(9, 8))             # row_begin > row_end
    refused("rows", rows=(5, H + 1))         # row_end > H
    refused("unknown camera", camera=2)
    refused("unknown camera", camera=-1)
    refused("samples", samples=0, offsets=None)
    refused("samples", samples=abi.TRT_MAX_CAMERA_SAMPLES + 1, offsets=None)
    for bad in (np.nan, np.inf, -np.inf, 1.5, -1.0000001):
        for slot in (0, 7):
            o = off.copy().reshape(-1)
            o[slot] = bad
            refused("offset", offsets=o)
    refused("overflows", W_=0xffffffff, H_=0xffffffff, rows=(0, 0xffffffff), samples=64, offsets=None, camera=abi.TRT_CAMERA_PINHOLE)
    # offsets of exactly 1 in magnitude, and the largest sample count, are accepted
    edge = rays_dev(tr, g, pc, 52, 36, cam, samples=2, offsets=[[1.0, -1.0], [-1.0, 1.0]])
    assert np.isfinite(edge[0]).all() and np.isfinite(edge[1]).all()
    most = rays_dev(tr, g, pc, 52, 36, cam, samples=abi.TRT_MAX_CAMERA_SAMPLES, rows=(3, 5))
    assert most[0].shape == (64 * 2 * 52, 3) and same_rays([a[:104] for a in most], [a[-104:] for a in most])
    # NULL arguments, through the raw bindings, both forms
    gp, pcp = C.byref(g), C.byref(pc)
    o4 = abi.camera_offsets(off, 4).ctypes.data_as(abi.f32p)
    dout, hout = abi.rays_out_struct(ptrs), abi.rays_out_struct(host)
    tail = (W, H, BAND[0], BAND[1], cam, 4, o4)
    refused_raw(L.trt_camera_rays_dev(tr._h, None, pcp, *tail, C.byref(dout), None))
    refused_raw(L.trt_camera_rays_dev(tr._h, gp, None, *tail, C.byref(dout), None))
    refused_raw(L.trt_camera_rays_dev(tr._h, gp, pcp, *tail, None, None))
    refused_raw(L.trt_camera_rays(tr._h, None, pcp, *tail, C.byref(hout)))
    refused_raw(L.trt_camera_rays(tr._h, gp, None, *tail, C.byref(hout)))
    refused_raw(L.trt_camera_rays(tr._h, gp, pcp, *tail, None))
    refused_raw(L.trt_camera_rays(tr._h, gp, pcp, *tail, C.byref(abi.trt_rays_out())))
    refused_raw(L.trt_camera_rays(tr._h, gp, pcp, W, H, 9, 8, cam, 4, o4, C.byref(hout)))
    assert L.trt_camera_rays_dev(None, gp, pcp, *tail, C.byref(dout), None) == abi.TRT_E_INVALID
    assert L.trt_camera_rays(None, gp, pcp, *tail, C.byref(hout)) == abi.TRT_E_INVALID
    good()
    torch.cuda.synchronize()
    assert all((b.cpu().numpy() == np.float32(SENTINEL)).all() for b in bufs) and all((h == np.float32(SENTINEL)).all() for h in host)   # a refused call writes nothing
