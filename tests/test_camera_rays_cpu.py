"""trt_camera_rays / trt_shade_camera, the part that needs no GPU: the ctypes prototypes against the header, the four
entry points exported, bound and refusing a NULL ctx without a device, the version unchanged, the Tracer methods, the
example wired into the host Makefile — and the arithmetic fact the GPU tests lean on: the regular 2x2 pattern on a W x H
frame feeds the cameras, bit for bit, the inputs of the pixel centres of the 2W x 2H frame."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import camera_truth
from conftest import ROOT
from toroidal_ray_tracing_amd import abi, camera, lib

HEADER = os.path.join(ROOT, "include", "trt.h")
NAMES = ("trt_camera_rays", "trt_camera_rays_dev", "trt_shade_camera", "trt_shade_camera_dev")
SHAPES = [(100, 68), (52, 36)]
f32 = np.float32

# C parameter type -> what the binding declares for it
CTYPES = {
    "trt_ctx*": C.c_void_p, "const trt_globals*": C.POINTER(abi.trt_globals), "const trt_push*": C.POINTER(abi.trt_push),
    "const trt_scene*": C.POINTER(abi.trt_scene), "uint32_t": C.c_uint32, "int": C.c_int, "const float*": abi.f32p,
    "const trt_rays_out*": C.POINTER(abi.trt_rays_out), "float*": C.c_void_p, "void*": C.c_void_p,
}


def _prototype(src, name):
    m = re.search(r"^int %s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    return [re.match(r"(.*?)\s*\b\w+$", p).group(1).strip() for p in params]   # drop the parameter names


def test_prototypes_match_the_header():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    frame = ["uint32_t", "uint32_t", "uint32_t", "uint32_t", "int", "uint32_t", "const float*"]   # W, H, rows, camera, samples, offsets
    rays = ["trt_ctx*", "const trt_globals*", "const trt_push*"] + frame + ["const trt_rays_out*"]
    shade = ["trt_ctx*", "const trt_globals*", "const trt_push*", "const trt_scene*"] + frame + ["float*"]
    want = {"trt_camera_rays": rays, "trt_camera_rays_dev": rays + ["void*"],
            "trt_shade_camera": shade, "trt_shade_camera_dev": shade + ["void*"]}
    for name in NAMES:
        assert _prototype(src, name) == want[name], name
        res, args = lib.SYMBOLS[name]
        assert res is C.c_int and args == [CTYPES[p] for p in want[name]], name
    assert re.search(r"#define TRT_MAX_CAMERA_SAMPLES (\d+)", src).group(1) == str(abi.TRT_MAX_CAMERA_SAMPLES) == "64"
    fields = re.search(r"typedef struct trt_rays_out \{(.*?)\} trt_rays_out;", src, flags=re.S).group(1)
    assert re.findall(r"float\* (\w+);", fields) == [k for k, _ in abi.trt_rays_out._fields_] == list(abi.RAY_FIELDS)
    assert C.sizeof(abi.trt_rays_out) == 48
    # the header's table of what replaces what names the calls on the raygen rows of both shaders
    assert re.search(r"REFL/shaders/raytrace\.rgen:42-48,\s*\n \*.*BEF/shaders/raytrace\.rgen:21-57\s+trt_camera_rays\* / trt_shade_camera\*", text)
    assert "#define TRT_VERSION_MINOR 3" in text


def test_entry_points_are_exported_and_refuse_a_null_ctx():
    L = lib.load()
    for name in NAMES:
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert L.trt_version() == 3
    g, pc = camera.baseline_camera(8, 8), abi.make_push()
    buf = np.full((6, 64), 7.0, f32)
    out = abi.rays_out_struct(list(buf))
    rgba = np.full(8 * 8 * 4, 7.0, f32)
    args = (C.byref(g), C.byref(pc), 8, 8, 0, 8, abi.TRT_CAMERA_PINHOLE, 1, None)
    assert L.trt_camera_rays(None, *args, C.byref(out)) == abi.TRT_E_INVALID
    assert L.trt_camera_rays_dev(None, *args, C.byref(out), None) == abi.TRT_E_INVALID
    args = (C.byref(g), C.byref(pc), None, 8, 8, 0, 8, abi.TRT_CAMERA_PINHOLE, 1, None)
    assert L.trt_shade_camera(None, *args, rgba.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_shade_camera_dev(None, *args, rgba.ctypes.data, None) == abi.TRT_E_INVALID
    assert (buf == 7.0).all() and (rgba == 7.0).all()


def test_tracer_has_the_bindings():
    from toroidal_ray_tracing_amd.tracer import Tracer
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Tracer.camera_rays) == ["self", "g", "pc", "W", "H", "camera", "samples", "offsets", "rows"]
    assert sig(Tracer.camera_rays_dev) == ["self", "g", "pc", "W", "H", "out_ptrs", "camera", "samples", "offsets", "rows", "stream"]
    assert sig(Tracer.shade_camera) == ["self", "scene", "g", "pc", "W", "H", "camera", "samples", "offsets", "rows"]
    assert sig(Tracer.shade_camera_dev) == ["self", "scene", "g", "pc", "W", "H", "rgba_ptr", "camera", "samples", "offsets", "rows", "stream"]
    for f in (Tracer.camera_rays, Tracer.camera_rays_dev, Tracer.shade_camera, Tracer.shade_camera_dev):
        p = inspect.signature(f).parameters
        assert p["samples"].default == 1 and p["offsets"].default is None and p["rows"].default is None
        assert p["camera"].default == abi.TRT_CAMERA_PINHOLE
    a = abi.camera_offsets([[0.25, -0.25], [0.0, 0.5]], 2)
    assert a.dtype == np.float32 and a.tolist() == [0.25, -0.25, 0.0, 0.5] and abi.camera_offsets(None, 3) is None
    with pytest.raises(ValueError):
        abi.camera_offsets([0.1, 0.2, 0.3], 2)


def test_example_is_in_the_makefile():
    src = os.path.join(ROOT, "examples", "antialias_main.cpp")
    text = open(src).read()
    body = text[text.rindex("#include"):]
    for call in ("trt_shade_camera(", "trt_camera_rays(", "trt_crossings(", "TRT_CAMERA_TOROIDAL"):
        assert call in body, call
    assert "hello_hip" not in body and "trt_render" not in body   # the plain C ABI, and the new calls alone make the frame
    mk = open(os.path.join(ROOT, "toroidal_ray_tracing_amd", "host", "Makefile")).read()
    all_rule = re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    clean_rule = re.search(r"^clean:(.*?)\n\.PHONY", mk, flags=re.S | re.M).group(1)
    assert "../../examples/antialias" in all_rule.split() and "../../examples/antialias" in clean_rule.split()
    assert "examples/antialias" in open(os.path.join(ROOT, ".gitignore")).read().split()


# ---------------------------------------------------------------------------------------------------------------------
# the doubling identity
# ---------------------------------------------------------------------------------------------------------------------
def u32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("W,H", SHAPES)
def test_the_2x2_pattern_feeds_the_cameras_the_inputs_of_the_double_frame(W, H):
    """In numpy float32, one rounding per operation, as include/trt.h writes the offset arithmetic: what the cameras
    compute from (pixel, offset) on W x H is what they compute from the pixel centre on 2W x 2H — the quotient u (pinhole:
    both operands scaled by 2), the angle alfa (toroidal: d' is exactly half of d).  Everything after is a function of
    these alone."""
    for n in (W, H):
        x = np.arange(n, dtype=f32)
        for k, j in enumerate(camera_truth.grid_2x2(abi.TRT_CAMERA_PINHOLE)[:2, 0]):   # -0.25, +0.25
            px = (x + f32(0.5)) + f32(j)
            assert np.array_equal(px.astype(np.float64), x.astype(np.float64) + 0.5 + float(j))   # exact in FP32
            u = px / f32(n)
            u2 = ((f32(2) * x + f32(k)) + f32(0.5)) / f32(2 * n)
            assert u.dtype == u2.dtype == np.float32 and np.array_equal(u32(u), u32(u2))
        d, d2 = f32(360.0) / f32(n), f32(360.0) / f32(2 * n)
        assert u32(d2 * f32(2)) == u32(d)
        for k, j in enumerate(camera_truth.grid_2x2(abi.TRT_CAMERA_TOROIDAL)[:2, 0]):   # 0, 0.5
            alfa = d * (x + f32(j))
            alfa2 = d2 * (f32(2) * x + f32(k))
            assert alfa.dtype == alfa2.dtype == np.float32 and np.array_equal(u32(alfa), u32(alfa2))


CAMERAS = {
    "pinhole": lambda W, H: (camera.baseline_camera(W, H), camera.baseline_push(1), abi.TRT_CAMERA_PINHOLE),
    "toroidal": lambda W, H: (camera.toroidal_camera(W, H), abi.make_push(rho=4.0), abi.TRT_CAMERA_TOROIDAL),
    "toroidal_theta": lambda W, H: (camera.toroidal_camera(W, H, eye=(0.5, 0.4, -0.3), center=(4.0, -1.0, 7.0)),
                                    abi.make_push(rho=3.0), abi.TRT_CAMERA_TOROIDAL),
}


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_the_2x2_pattern_is_the_double_frame_of_the_oracle(oracle, name, W, H):
    """The stated sample order and layout against oracle.raygen on the 2W x 2H grid: the FP64 restatement of the offset
    arithmetic (tests/camera_truth.py), sample s = 2*ky + kx of pixel (x, y), is the oracle's ray of pixel (2x + kx, 2y + ky)
    to the project's 1e-5 bar — the oracle rounds in FP32, the restatement does not.  The cameras are the same for both
    shapes: the aspect ratio W / H is that of 2W / 2H, as a double, exactly."""
    g, pc, cam = CAMERAS[name](W, H)
    g2, pc2, _ = CAMERAS[name](2 * W, 2 * H)
    assert bytes(g) == bytes(g2) and bytes(pc) == bytes(pc2)
    fr = oracle.toroidal_frame(g, pc)
    if cam == abi.TRT_CAMERA_TOROIDAL:
        assert (fr["theta"] != 0.0) == (name == "toroidal_theta")
    o, d = camera_truth.camera_rays(g, pc, W, H, cam, camera_truth.grid_2x2(cam), frame=fr)
    want = np.array([np.concatenate(oracle.raygen(g, pc, 2 * W, 2 * H, cam, x, y)) for y in range(2 * H) for x in range(2 * W)])
    assert np.isfinite(want).all()
    idx = camera_truth.double_frame_index(W, H).reshape(-1)
    bar = camera_truth.RAY_RTOL * camera_truth.scale(pc, fr["eye"])
    assert np.abs(o - want[idx, :3]).max() <= bar
    assert np.abs(d - want[idx, 3:]).max() <= camera_truth.RAY_RTOL
    # and a wrong sample order would not pass: the neighbouring sample is further away than the bar
    assert np.abs(d[:W * H] - d[W * H:2 * W * H]).max() > 100 * camera_truth.RAY_RTOL
