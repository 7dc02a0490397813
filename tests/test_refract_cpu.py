"""trt_shade_refract / trt_shade_refract_camera, the part that needs no GPU: the four entry points declared, exported and
bound with the argument types of their trt_shade* twins — and the tests' FP64 truth (tests/refract_truth.py) held to
Snell's law, to its energy bookkeeping, to itself with an index-matched torus, and to the share of rays it may call
non-robust."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import crossings_truth as ct
import refract_truth as rt
import through_truth as tt
from conftest import ROOT
from toroidal_ray_tracing_amd import abi, camera, lib

TWINS = {"trt_shade_refract": "trt_shade", "trt_shade_refract_dev": "trt_shade_dev",
         "trt_shade_refract_camera": "trt_shade_camera", "trt_shade_refract_camera_dev": "trt_shade_camera_dev"}


def test_the_four_calls_are_declared_exported_and_typed_like_their_twins():
    L = lib.load()
    for name, twin in TWINS.items():
        assert name in lib.SYMBOLS and hasattr(L, name), name
        assert lib.SYMBOLS[name] == lib.SYMBOLS[twin], name
    assert L.trt_version() == 3
    rays, pc, g = abi.trt_rays(), abi.make_push(), abi.trt_globals()
    out = np.full(8, 7.0, np.float32)
    assert L.trt_shade_refract(None, C.byref(rays), 1, C.byref(pc), None, out.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_shade_refract_dev(None, C.byref(rays), 1, C.byref(pc), None, out.ctypes.data, None) == abi.TRT_E_INVALID
    assert L.trt_shade_refract_camera(None, C.byref(g), C.byref(pc), None, 1, 1, 0, 1, 0, 1, None, out.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_shade_refract_camera_dev(None, C.byref(g), C.byref(pc), None, 1, 1, 0, 1, 0, 1, None, out.ctypes.data, None) == abi.TRT_E_INVALID
    assert (out == 7.0).all()
    from toroidal_ray_tracing_amd.tracer import Tracer
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Tracer.shade_refract) == sig(Tracer.shade) and sig(Tracer.shade_refract_dev) == sig(Tracer.shade_dev)
    assert sig(Tracer.shade_refract_camera) == sig(Tracer.shade_camera)
    assert sig(Tracer.shade_refract_camera_dev) == sig(Tracer.shade_camera_dev)


def test_header_host_mirror_and_example(tmp_path):
    text = open(os.path.join(ROOT, "include", "trt.h")).read()
    assert re.search(r"trt_shade_refract\* /\n", text) and re.search(r"trt_shade_refract_camera\*\n", text)   # the table at the top
    assert re.search(r"ZERO-INITIALISED trt_material HAS ior == 0", text) and "#define TRT_VERSION_MINOR 3" in text
    host = os.path.join(ROOT, "toroidal_ray_tracing_amd", "host")
    hpp, body = open(os.path.join(host, "hello_hip.hpp")).read(), open(os.path.join(host, "hello_hip.cpp")).read()
    assert re.search(r"void shadeRefract\(void\* stream,", hpp) and re.search(r"void raytraceRefract\(void\* stream,", hpp)
    assert "trt_shade_refract_dev(" in body and "trt_shade_refract_camera_dev(" in body
    # Scene carries ior and the filter through the ABI; ior is 1 by default
    sc = abi.Scene([((0, 0, 0), 1.0, 0.25, 0), ((0, 0, 0), 1.0, 0.1, 1)], [camera.PLASTIC, rt.glass()])
    assert [m.ior for m in sc._mats] == [1.0, 1.5] and [round(v, 6) for v in sc._mats[1].transmittance] == [0.9, 0.95, 1.0]
    src = os.path.join(ROOT, "examples", "glass_ring_main.cpp")
    code = open(src).read()
    code = code[code.rindex("#include"):]
    assert "trt_shade_refract_camera(" in code and "trt_shade_camera(" in code and "TRT_CAMERA_TOROIDAL, 4, grid" in code
    mk = open(os.path.join(host, "Makefile")).read()
    assert "../../examples/glass_ring" in re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    assert "examples/glass_ring" in open(os.path.join(ROOT, ".gitignore")).read().split()
    pkg = os.path.join(ROOT, "toroidal_ray_tracing_amd")
    exe = str(tmp_path / "glass_ring")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, src, "-L" + pkg, "-ltrt", "-Wl,-rpath," + pkg],
                       capture_output=True, text=True)
    assert p.returncode == 0 and os.path.exists(exe), p.stdout + p.stderr


@pytest.mark.parametrize("name", list(rt.cases()))
def test_the_truth_obeys_snell_and_stays_inside_the_cap(name):
    """sin(theta_t) = sin(theta_i) / n on the way in, n * sin(theta_i) on the way out, to 1e-12 at every refraction; a
    total internal reflection keeps the angle; and the truth calls at most a tenth of the rays non-robust."""
    c = rt.case(name)
    ev = c["events"]
    assert len(ev["ray"]) > 1000 and c["pc"].maxDepth == 8
    eta = np.where(ev["entering"], 1.0 / ev["n"], ev["n"])
    bent = ~ev["tir"]
    assert np.abs(ev["sin_t"][bent] - eta[bent] * ev["sin_i"][bent]).max() <= 1e-12
    assert np.abs(ev["sin_t"][~bent] - ev["sin_i"][~bent]).max(initial=0.0) <= 1e-12
    assert not (ev["tir"] & ev["entering"]).any()          # (n > 1: only the way out can fail to refract)
    assert (ev["entering"] & bent).sum() > 500 and (~ev["entering"] & bent).sum() > 500
    assert c["robust"].mean() > 0.9, 1.0 - c["robust"].mean()
    miss = np.asarray(c["pc"].clearColor[:3]) * 0.8
    assert (c["first"]["id"] >= 0).mean() > 0.5            # (most rays of a set see a surface)
    assert np.isfinite(c["rgb"]).all() and (np.abs(c["rgb"] - miss).max(1) > 1e-3).mean() > 0.5


def test_the_diamond_reflects_totally_on_at_least_a_hundredth_of_the_rays():
    ev = rt.case("single_diamond")["events"]
    share = len(np.unique(ev["ray"][ev["tir"]])) / ct.N_RAYS
    assert share >= 0.01, share


def test_energy_bookkeeping_of_one_passage():
    """In through a wall and out through the next: the attenuation is Tf, applied once, on the way in.  A total internal
    reflection leaves it at what it was, and the directions stay unit vectors."""
    rng = np.random.default_rng(3)
    m = 2000
    N = rng.normal(size=(m, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    I = rng.normal(size=(m, 3))
    I /= np.linalg.norm(I, axis=1, keepdims=True)
    I[np.einsum("ni,ni->n", N, I) > 0] *= -1.0              # all of them arrive from outside
    n, Tf, one = np.full(m, 1.5), np.tile([0.9, 0.95, 1.0], (m, 1)), np.ones((m, 3))
    d1, A1, tir1, ent1, *_ = rt.refract_step(I, N, n, Tf, one)
    assert ent1.all() and not tir1.any() and np.array_equal(A1, Tf)
    assert np.abs(np.linalg.norm(d1, axis=1) - 1.0).max() < 1e-12
    # the far wall of a slab: the outward normal there is -N; the ray leaves parallel to how it came, the filter not applied again
    d2, A2, tir2, ent2, *_ = rt.refract_step(d1, -N, n, Tf, A1)
    assert not ent2.any() and not tir2.any() and np.array_equal(A2, Tf) and np.abs(d2 - I).max() < 1e-12
    # from inside at a grazing angle: no refracted ray, the reflection, the attenuation untouched
    T = np.cross(N, rng.normal(size=(m, 3)))
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    G = 0.3 * N + T * np.sqrt(1.0 - 0.09)                   # cos 0.3 < sqrt(1 - 1/1.5^2) = 0.745: beyond the critical angle
    d3, A3, tir3, ent3, *_ = rt.refract_step(G, N, n, Tf, A1)
    assert tir3.all() and not ent3.any() and np.array_equal(A3, A1)
    assert np.abs(d3 - (G - 0.6 * N)).max() < 1e-12


def test_index_matched_black_glass_is_the_scene_without_the_torus():
    """n = 1, Tf = 1 and a black material: every passage goes straight on and adds nothing, so the truth's colour is the
    truth's colour of the scene without that torus, to 1e-9 — on refract_truth.APART, where the glass ring (an opaque
    shadow caster by the rule) cannot shade the other one, and with at most 4 + 1 segments of the 8 allowed."""
    geo = rt.APART
    o, d = rt.rays_of((geo, None))
    ghost = dict(rt.BLACK, illum=7, ior=1.0, transmittance=(1.0, 1.0, 1.0))
    push = tt.push_dict(abi.make_push(light_pos=rt.APART_LIGHT, max_depth=rt.MAX_DEPTH))
    both = [(geo[0][0], geo[0][1], geo[0][2], 0), (geo[1][0], geo[1][1], geo[1][2], 1)]
    with_it, _, ev, first = rt.shade_refract(o, d, both, [camera.PLASTIC, ghost], push, info=True)
    without, _ = rt.shade_refract(o, d, both[:1], [camera.PLASTIC], push)
    assert (first["id"] == 1).mean() > 0.3 and len(ev["ray"]) > 3000 and not ev["tir"].any()
    assert np.abs(with_it - without).max() <= 1e-9
    miss = 0.8
    assert (np.abs(without - miss).max(1) > 1e-3).mean() > 0.3   # (the plastic ring is seen, also through the ghost)
