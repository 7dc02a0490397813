"""trt_transmittance / trt_shade_through, the part that needs no GPU: the ctypes prototypes against the header, the four
entry points exported, bound and refusing a NULL ctx without a device, the Tracer and HelloHip bindings, the example
wired into the host Makefile — and the tests' FP64 truth (tests/through_truth.py) against the independent shading chain
of oracle/truth.py, against itself with a transparent torus, and held to the share of rays it may call non-robust."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import crossings_truth as ct
import through_truth as tt
from conftest import ROOT
from oracle import truth
from toroidal_ray_tracing_amd import abi, camera, lib

HEADER = os.path.join(ROOT, "include", "trt.h")
NAMES = ("trt_transmittance", "trt_transmittance_dev", "trt_shade_through", "trt_shade_through_dev")

CTYPES = {
    "trt_ctx*": C.c_void_p, "const trt_rays*": C.POINTER(abi.trt_rays), "uint32_t": C.c_uint32, "float": C.c_float,
    "const trt_push*": C.POINTER(abi.trt_push), "const trt_scene*": C.POINTER(abi.trt_scene),
    "const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p,
}


def _prototype(src, name):
    m = re.search(r"^int %s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    return [re.match(r"(.*?)\s*\b\w+$", p).group(1).strip() for p in params]   # drop the parameter names


def test_prototypes_match_the_header():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    want = {
        "trt_transmittance": ["trt_ctx*", "const trt_rays*", "const float*", "const trt_scene*", "float", "float", "float*"],
        "trt_shade_through": ["trt_ctx*", "const trt_rays*", "uint32_t", "const trt_push*", "const trt_scene*", "float*"],
    }
    for name, params in want.items():
        assert _prototype(src, name) == params, name
        assert _prototype(src, name + "_dev") == params + ["void*"], name
        for sym, ps in ((name, params), (name + "_dev", params + ["void*"])):
            res, args = lib.SYMBOLS[sym]
            assert res is C.c_int and args == [CTYPES[p] for p in ps], sym
    # the table of what replaces what has the two rows; the trap of a zero-initialised material is stated loudly
    assert re.search(r"trt_transmittance\*\n", text) and re.search(r"trt_shade_through\*\n", text)
    assert re.search(r"ZERO-INITIALISED trt_material HAS dissolve == 0", text)
    assert re.search(r"fan_occluded, transmittance or shade_through\s*\n \* call made with counting enabled", text)
    assert "#define TRT_VERSION_MINOR 3" in text


def test_the_calls_are_exported_and_refuse_a_null_ctx():
    L = lib.load()
    for name in NAMES:
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert L.trt_version() == 3
    rays = abi.trt_rays()
    pc = abi.make_push()
    out = np.full(8, 7.0, np.float32)
    assert L.trt_transmittance(None, C.byref(rays), None, None, 0.001, 1.0, out.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_transmittance_dev(None, C.byref(rays), None, None, 0.001, 1.0, out.ctypes.data, None) == abi.TRT_E_INVALID
    assert L.trt_shade_through(None, C.byref(rays), 1, C.byref(pc), None, out.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_shade_through_dev(None, C.byref(rays), 1, C.byref(pc), None, out.ctypes.data, None) == abi.TRT_E_INVALID
    assert (out == 7.0).all()


def test_tracer_and_host_mirror_have_the_bindings():
    from toroidal_ray_tracing_amd.tracer import Tracer
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Tracer.transmittance) == sig(Tracer.occluded) == ["self", "scene", "o", "d", "tmin", "tmax", "tmax_per_ray"]
    assert sig(Tracer.transmittance_dev) == ["self", "scene", "ray_ptrs", "n", "T_ptr", "tmax_ptr", "tmin", "tmax", "stream"]
    assert sig(Tracer.shade_through) == sig(Tracer.shade)
    assert sig(Tracer.shade_through_dev) == sig(Tracer.shade_dev)
    host = os.path.join(ROOT, "toroidal_ray_tracing_amd", "host")
    assert re.search(r"void shadeThrough\(void\* stream,", open(os.path.join(host, "hello_hip.hpp")).read())
    body = open(os.path.join(host, "hello_hip.cpp")).read()
    assert "void HelloHip::shadeThrough(" in body and "trt_shade_through_dev(" in body
    # Scene carries dissolve through the ABI, 1 by default
    sc = abi.Scene([((0, 0, 0), 1.0, 0.25, 0), ((0, 0, 0), 1.0, 0.1, 1)], [camera.PLASTIC, dict(camera.MATTE, dissolve=0.25)])
    assert [m.dissolve for m in sc._mats] == [1.0, 0.25]


def test_example_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "examples", "see_through_main.cpp")
    text = open(src).read()
    code = text[text.rindex("#include"):]
    assert "trt_camera_rays(" in code and "trt_shade_through(" in code and "trt_shade(" in code and "0.25f" in code
    mk = open(os.path.join(ROOT, "toroidal_ray_tracing_amd", "host", "Makefile")).read()
    all_rule = re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    assert "../../examples/see_through" in all_rule and "../../examples/supersample" in all_rule
    assert "examples/see_through" in open(os.path.join(ROOT, ".gitignore")).read().split()
    pkg = os.path.join(ROOT, "toroidal_ray_tracing_amd")
    exe = str(tmp_path / "see_through")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, src, "-L" + pkg, "-ltrt", "-Wl,-rpath," + pkg],
                       capture_output=True, text=True)
    assert p.returncode == 0 and os.path.exists(exe), p.stdout + p.stderr


# ---------------------------------------------------------------------------------------------------------------------
# the truth against the independent chain, and against itself
# ---------------------------------------------------------------------------------------------------------------------
W = H = 32
mat4 = lambda a: np.array(a[:], np.float64).reshape(4, 4).T   # column-major storage -> M[row, col]
NEST3 = [((0.0, 0.0, 0.0), 1.0, 0.35, 1), ((0.0, 0.0, 0.0), 1.0, 0.25, 0), ((0.0, 0.0, 0.0), 1.0, 0.15, 1)]


@pytest.mark.parametrize("name", ["mirror", "plastic", "nest3"])
def test_truth_with_every_surface_opaque_is_shade_frame(name):
    """Self-check 1: a = 1 everywhere, on the primary rays of a 32x32 frame — the compositing walk must collapse to the
    first hit, the transmittance to the shadow bit, and the mirror must weigh its own colour by Ks as rchit:149 does."""
    if name == "nest3":
        sc = abi.Scene(NEST3, [camera.PLASTIC, camera.MIRROR])
    else:
        sc = camera.single_torus_scene(material=camera.MIRROR if name == "mirror" else camera.PLASTIC)
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(5)
    push, mats = tt.push_dict(pc), tt.material_dicts(sc)
    want, _, _ = truth.shade_frame(sc.tori_list(), mats, mat4(g.viewInverse), mat4(g.projInverse), g.center[:], push, W, H, 0)
    o, d = truth.primary_rays(mat4(g.viewInverse), mat4(g.projInverse), g.center[:], 0.0, W, H, 0)
    got, _ = tt.shade_through(o, d, sc.tori_list(), mats, [1.0] * sc.n_tori, push)
    np.testing.assert_allclose(got, want.reshape(-1, 4)[:, :3], rtol=0, atol=1e-9)
    miss = np.asarray(pc.clearColor[:3]) * 0.8
    assert 0.05 < (np.abs(got - miss).max(1) > 1e-6).mean() < 0.95   # the frame holds hits and misses


def test_truth_with_a_transparent_torus_is_the_scene_without_it():
    """Self-check 2: a_j = 0 equals removing torus j — from the primary walk and from every shadow ray."""
    s = ct.ray_set("nest3")
    geo, _ = ct.SCENES["nest3"]
    mats = [camera.PLASTIC, camera.MATTE, camera.MIRROR]
    push = tt.push_dict(camera.baseline_push(3))
    o, d = s["o"][:1024], s["d"][:1024]
    for j in range(3):
        alpha = [0.5, 0.75, 1.0]
        alpha[j] = 0.0
        keep = [k for k in range(3) if k != j]
        with_j, _ = tt.shade_through(o, d, [(C, R, r, k) for k, (C, R, r) in enumerate(geo)], mats, alpha, push)
        without, _ = tt.shade_through(o, d, [(*geo[k], i) for i, k in enumerate(keep)], [mats[k] for k in keep],
                                      [alpha[k] for k in keep], push)
        np.testing.assert_allclose(with_j, without, rtol=0, atol=1e-12)
    T, _ = tt.transmittance(o, d, geo, [0.0, 0.5, 0.75])
    T2, _ = tt.transmittance(o, d, geo[1:], [0.5, 0.75])
    assert np.array_equal(T, T2) and len(np.unique(T)) > 3


@pytest.mark.parametrize("name", list(tt.cases()))
def test_truth_leaves_few_rays_out(name):
    """Self-check 3: the share of rays the truth calls non-robust stays within the cap of its set — 5 %, the
    robust.mean() > 0.95 bar of tests/test_oracle.py; 7 % for the nest with every shell translucent."""
    c = tt.case(name)
    share = 1.0 - c["robust"].mean()
    print(f"{name}: non-robust {100 * share:.2f} % (cap {100 * c['cap']:.0f} %)")
    assert share <= c["cap"], (name, share)
    assert len(c["o"]) == ct.N_RAYS and np.isfinite(c["rgb"]).all()
