"""trt_chords / trt_glow, the part that needs no GPU: the ctypes prototypes against the header, the four entry points
exported, bound and refusing a NULL ctx without a device, trt_medium's layout, the Tracer and HelloHip bindings, the
example wired into the host Makefile — and the tests' FP64 truth (tests/media_truth.py) against the project's older
chord code, against itself without a torus, in the two limits where the integral is a chord, and held to the share of
rays it may call non-robust."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import crossings_truth as ct
import media_truth as mt
from conftest import ROOT
from toroidal_ray_tracing_amd import abi, lib

HEADER = os.path.join(ROOT, "include", "trt.h")
NAMES = ("trt_chords", "trt_chords_dev", "trt_glow", "trt_glow_dev")

CTYPES = {
    "trt_ctx*": C.c_void_p, "const trt_rays*": C.POINTER(abi.trt_rays), "float": C.c_float,
    "const trt_scene*": C.POINTER(abi.trt_scene), "const trt_medium*": C.POINTER(abi.trt_medium),
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
        "trt_chords": ["trt_ctx*", "const trt_rays*", "const float*", "const trt_scene*", "float", "float", "float*"],
        "trt_glow": ["trt_ctx*", "const trt_rays*", "const float*", "const trt_scene*", "const trt_medium*", "float", "float", "float*"],
    }
    for name, params in want.items():
        assert _prototype(src, name) == params, name
        assert _prototype(src, name + "_dev") == params + ["void*"], name
        for sym, ps in ((name, params), (name + "_dev", params + ["void*"])):
            res, args = lib.SYMBOLS[sym]
            assert res is C.c_int and args == [CTYPES[p] for p in ps], sym
    # the table of what replaces what has the two rows, both build-defined; the counters' sentence names the calls
    assert re.search(r"\(none: build-defined[^\n]*\n[^\n]*trt_chords\*\n", text)
    assert re.search(r"\(none: build-defined[^\n]*\n[^\n]*trt_glow\*\n", text)
    assert re.search(r"call made with counting enabled\.\s+trt_chords and trt_glow count as well\.", text)
    assert re.search(r"typedef struct trt_medium \{\s*float emission\[3\];.*?float sigma;.*?\} trt_medium;", src, flags=re.S)
    assert "#define TRT_VERSION_MINOR 3" in text


def test_the_calls_are_exported_and_refuse_a_null_ctx():
    L = lib.load()
    for name in NAMES:
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert L.trt_version() == 3
    assert C.sizeof(abi.trt_medium) == 16 and abi.trt_medium.sigma.offset == 12
    rays = abi.trt_rays()
    media = abi.media([((1.0, 0.5, 0.25), 2.0)])
    out = np.full(8, 7.0, np.float32)
    assert L.trt_chords(None, C.byref(rays), None, None, 0.001, 1.0, out.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_chords_dev(None, C.byref(rays), None, None, 0.001, 1.0, out.ctypes.data, None) == abi.TRT_E_INVALID
    assert L.trt_glow(None, C.byref(rays), None, None, media, 0.001, 1.0, out.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_glow_dev(None, C.byref(rays), None, None, media, 0.001, 1.0, out.ctypes.data, None) == abi.TRT_E_INVALID
    assert (out == 7.0).all()


def test_the_media_helper():
    m = abi.media([((1.0, 0.5, 0.25), 2.0), None, dict(sigma=0.5), dict(emission=(0.0, 1.0, 0.0))])
    assert len(m) == 4 and abi.media(m) is m
    assert [(tuple(x.emission), x.sigma) for x in m] == [((1.0, 0.5, 0.25), 2.0), ((0.0, 0.0, 0.0), 0.0), ((0.0, 0.0, 0.0), 0.5),
                                                          ((0.0, 1.0, 0.0), 0.0)]


def test_tracer_and_host_mirror_have_the_bindings():
    from toroidal_ray_tracing_amd.tracer import Tracer
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Tracer.chords) == sig(Tracer.transmittance) == ["self", "scene", "o", "d", "tmin", "tmax", "tmax_per_ray"]
    assert sig(Tracer.glow) == ["self", "scene", "o", "d", "media", "tmin", "tmax", "tmax_per_ray"]
    assert sig(Tracer.chords_dev) == ["self", "scene", "ray_ptrs", "n", "length_ptr", "tmax_ptr", "tmin", "tmax", "stream"]
    assert sig(Tracer.glow_dev) == ["self", "scene", "ray_ptrs", "n", "media", "rgba_ptr", "tmax_ptr", "tmin", "tmax", "stream"]
    defaults = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not p.empty}
    assert defaults(Tracer.chords) == defaults(Tracer.transmittance) == defaults(Tracer.glow)
    host = os.path.join(ROOT, "toroidal_ray_tracing_amd", "host")
    hpp = open(os.path.join(host, "hello_hip.hpp")).read()
    assert re.search(r"void chords\(void\* stream,", hpp) and re.search(r"void glow\(void\* stream,", hpp)
    body = open(os.path.join(host, "hello_hip.cpp")).read()
    assert "void HelloHip::chords(" in body and "trt_chords_dev(" in body
    assert "void HelloHip::glow(" in body and "trt_glow_dev(" in body


def test_example_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "examples", "plasma_glow_main.cpp")
    text = open(src).read()
    code = text[text.rindex("#include"):]
    for call in ("trt_camera_rays(", "trt_chords(", "trt_glow(", "trt_trace(", "clearColor"):
        assert call in code, call
    assert len(re.findall(r"trt_glow\(", code)) == 2 and "t_ring.data(), &scene" in code   # the second call is bounded by trt_trace's t
    mk = open(os.path.join(ROOT, "toroidal_ray_tracing_amd", "host", "Makefile")).read()
    all_rule = re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    assert "../../examples/plasma_glow" in all_rule and "../../examples/see_through" in all_rule
    assert "../../examples/plasma_glow" in re.search(r"^clean:(.*?)\n\.PHONY", mk, flags=re.S | re.M).group(1)
    assert "examples/plasma_glow" in open(os.path.join(ROOT, ".gitignore")).read().split()
    pkg = os.path.join(ROOT, "toroidal_ray_tracing_amd")
    exe = str(tmp_path / "plasma_glow")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src, "-L" + pkg, "-ltrt", "-Wl,-rpath," + pkg],
                       capture_output=True, text=True)
    assert p.returncode == 0 and os.path.exists(exe), p.stdout + p.stderr


# ---------------------------------------------------------------------------------------------------------------------
# the truth against the project's older chord code, and against itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mt.NAMES)
def test_truth_chords_are_the_older_chord_lengths(name):
    """Self-check 1: on lines of sight from outside over the full window, the pairing rule gives what
    crossings_truth.chord_lengths forms from the enter / leave pairs, times |d| — on the rays whose list is robust (a
    grazing pair the older code counts and the rule drops is not)."""
    s, c = ct.ray_set(name), mt.case(name, "los")
    n_t = len(c["geo"])
    old = ct.chord_lengths(np.where(np.isfinite(s["t"]), s["t"], 0.0), s["id"], s["entering"], n_t).T * c["len"][None, :]
    ok = c["robust"]
    np.testing.assert_allclose(c["chords"][:, ok], old[:, ok], rtol=1e-12, atol=1e-12)
    assert not c["info"]["in0"].any() and not c["info"]["in1"].any()
    assert (c["chords"] > 0).any(axis=1).all() and (c["chords"] >= 0).all()


def test_truth_without_a_medium_is_the_scene_without_the_torus():
    """Self-check 2: a zero medium equals removing the torus."""
    for kind in ("los", "seg"):
        c = mt.case("nest3", kind)
        o, d = c["o"][:1024], c["d"][:1024]
        for j in range(3):
            media = list(c["media"])
            media[j] = ((0.0, 0.0, 0.0), 0.0)
            keep = [k for k in range(3) if k != j]
            with_j = mt.truth_of(o, d, c["geo"], None, media, c["tmin"], c["tmax"])
            without = mt.truth_of(o, d, [c["geo"][k] for k in keep], None, [media[k] for k in keep], c["tmin"], c["tmax"])
            np.testing.assert_allclose(with_j["L"], without["L"], rtol=0, atol=1e-13)
            np.testing.assert_allclose(with_j["T"], without["T"], rtol=0, atol=1e-13)
            assert np.array_equal(with_j["chords"][keep], without["chords"])


@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", mt.NAMES)
def test_truth_limits_are_chords(name, kind):
    """Self-checks 3 and 4: with sigma = 0 and unit emission on torus j alone L_r is chord j; T = exp(-sum sigma_j chord_j)."""
    c = mt.case(name, kind)
    n_t = len(c["geo"])
    sel = slice(0, 1024)
    o, d = c["o"][sel], c["d"][sel]
    bound = None if c["bound"] is None else c["bound"][sel]
    for j in range(n_t):
        media = [((1.0, 0.5, 0.25), 0.0) if k == j else ((0.0, 0.0, 0.0), 0.0) for k in range(n_t)]
        one = mt.truth_of(o, d, c["geo"], c["axes"], media, c["tmin"], c["tmax"], bound)
        np.testing.assert_allclose(one["L"][:, 0], c["chords"][j, sel], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(one["L"][:, 1], 0.5 * c["chords"][j, sel], rtol=1e-12, atol=1e-13)
        assert (one["T"] == 1.0).all()
    sig = np.array([m[1] for m in c["media"]])
    np.testing.assert_allclose(c["T"], np.exp(-(sig[:, None] * c["chords"]).sum(0)), rtol=1e-12, atol=0)
    assert np.isfinite(c["L"]).all() and (c["L"] >= 0).all() and ((c["T"] > 0) & (c["T"] <= 1)).all()


@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", mt.NAMES)
def test_truth_leaves_few_rays_out(name, kind):
    """Self-check 5: the share of rays the truth calls non-robust stays within the cap of its scene; the segment sets hold
    what they are for — windows that start and end inside a tube, windows wholly inside one, intervals closed by the
    window's end — and the cut sets their empty windows."""
    c = mt.case(name, kind)
    share = 1.0 - c["robust"].mean()
    info = c["info"]
    print(f"{name} {kind}: non-robust {100 * share:.2f} % (cap {100 * c['cap']:.0f} %), start inside {100 * info['in0'].any(0).mean():.1f} %, "
          f"end inside {100 * info['in1'].any(0).mean():.1f} %, wholly inside {100 * c['inside_whole'].mean():.1f} %, "
          f"closed by the end {100 * c['to_end'].mean():.1f} %")
    assert share <= c["cap"], (name, kind, share)
    assert len(c["o"]) == ct.N_RAYS
    if kind == "seg":
        assert info["in0"].any(0).mean() > 0.4 and info["in1"].any(0).mean() > 0.4
        assert c["inside_whole"].mean() > 0.01 and c["to_end"].mean() > 0.1
    if kind == "cut":
        assert (~info["nonempty"]).mean() == pytest.approx(0.2, abs=1e-3) and c["to_end"].mean() > 0.05
        assert (c["chords"][:, ~info["nonempty"]] == 0).all() and (c["T"][~info["nonempty"]] == 1).all()
