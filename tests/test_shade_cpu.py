"""trt_shade, the part that needs no GPU: the ctypes prototypes against the header, both entry points exported, bound and
refusing a NULL ctx without a device, the version unchanged, and the example wired into the host Makefile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from toroidal_ray_tracing_amd import abi, lib

HEADER = os.path.join(ROOT, "include", "trt.h")

# C parameter type -> what the binding declares for it
CTYPES = {
    "trt_ctx*": C.c_void_p, "const trt_rays*": C.POINTER(abi.trt_rays), "uint32_t": C.c_uint32,
    "const trt_push*": C.POINTER(abi.trt_push), "const trt_scene*": C.POINTER(abi.trt_scene),
    "float*": C.c_void_p, "void*": C.c_void_p,
}


def _prototype(src, name):
    m = re.search(r"^int %s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    return [re.match(r"(.*?)\s*\b\w+$", p).group(1).strip() for p in params]   # drop the parameter names


def test_prototypes_match_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    host = _prototype(src, "trt_shade")
    dev = _prototype(src, "trt_shade_dev")
    assert host == ["trt_ctx*", "const trt_rays*", "uint32_t", "const trt_push*", "const trt_scene*", "float*"]
    assert dev == host + ["void*"]
    for name, params in (("trt_shade", host), ("trt_shade_dev", dev)):
        res, args = lib.SYMBOLS[name]
        assert res is C.c_int and args == [CTYPES[p] for p in params], name
    # the header's table of what replaces what names the call and the shader lines it stands for
    assert re.search(r"raytrace\.rgen:54-87 bounce\s*\n \*\s+loop \+ rchit/rmiss\s+trt_shade\*", open(HEADER).read())


def test_shade_is_exported_and_refuses_a_null_ctx():
    L = lib.load()
    for name in ("trt_shade", "trt_shade_dev"):
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert L.trt_version() == 3
    rays = abi.trt_rays()
    pc = abi.make_push()
    rgba = np.full(8, 7.0, np.float32)
    assert L.trt_shade(None, C.byref(rays), 1, C.byref(pc), None, rgba.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_shade_dev(None, C.byref(rays), 1, C.byref(pc), None, rgba.ctypes.data, None) == abi.TRT_E_INVALID
    assert (rgba == 7.0).all()


def test_tracer_has_the_bindings():
    from toroidal_ray_tracing_amd.tracer import Tracer
    import inspect
    assert list(inspect.signature(Tracer.shade).parameters) == ["self", "scene", "o", "d", "pc", "samples"]
    assert list(inspect.signature(Tracer.shade_dev).parameters) == ["self", "scene", "ray_ptrs", "n", "pc", "rgba_ptr", "samples", "stream"]
    assert inspect.signature(Tracer.shade).parameters["samples"].default == 1
    assert inspect.signature(Tracer.shade_dev).parameters["samples"].default == 1


def test_example_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "examples", "supersample_main.cpp")
    text = open(src).read()
    assert "trt_shade(" in text and "trt_render" not in text[text.rindex("#include"):]   # host buffers, and no library camera
    mk = open(os.path.join(ROOT, "toroidal_ray_tracing_amd", "host", "Makefile")).read()
    all_rule = re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    assert "../../examples/supersample" in all_rule and "../../examples/shell_chords" in all_rule
    assert "examples/supersample" in open(os.path.join(ROOT, ".gitignore")).read().split()
    pkg = os.path.join(ROOT, "toroidal_ray_tracing_amd")
    exe = str(tmp_path / "supersample")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, src, "-L" + pkg, "-ltrt", "-Wl,-rpath," + pkg],
                       capture_output=True, text=True)
    assert p.returncode == 0 and os.path.exists(exe), p.stdout + p.stderr
