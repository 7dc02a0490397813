"""trt_glow_profile, the part that needs no GPU: the prototypes against the header, the entry points exported, bound and
refusing a NULL ctx without a device, trt_profile's layout, the helpers of abi.py, the Tracer and HelloHip bindings, the
example wired into the host Makefile — and the rule itself, restated in FP64 by tests/profile_truth.py: a known answer,
its order of convergence, its flat limit, and the share of rays the GPU tests may leave out."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import media_truth as mt
import profile_truth as pt
from conftest import ROOT
from toroidal_ray_tracing_amd import abi, lib

HEADER = os.path.join(ROOT, "include", "trt.h")
PARAMS = ["trt_ctx*", "const trt_rays*", "const float*", "const trt_scene*", "const trt_profile*", "uint32_t", "float", "float", "float*"]
CTYPES = {
    "trt_ctx*": C.c_void_p, "const trt_rays*": C.POINTER(abi.trt_rays), "float": C.c_float, "uint32_t": C.c_uint32,
    "const trt_scene*": C.POINTER(abi.trt_scene), "const trt_profile*": C.POINTER(abi.trt_profile),
    "const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p,
}


def test_prototypes_match_the_header():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, params in (("trt_glow_profile", PARAMS), ("trt_glow_profile_dev", PARAMS + ["void*"])):
        m = re.search(r"^int %s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        got = [re.match(r"(.*?)\s*\b\w+$", " ".join(p.split())).group(1).strip() for p in m.group(1).split(",")]
        assert got == params, name
        res, args = lib.SYMBOLS[name]
        assert res is C.c_int and args == [CTYPES[p] for p in params], name
    assert re.search(r"#define TRT_PROFILE_KNOTS\s+17\b", text) and re.search(r"#define TRT_MAX_GLOW_STEPS\s+64\b", text)
    assert re.search(r"typedef struct trt_profile \{\s*float knot\[TRT_PROFILE_KNOTS\]\[4\];.*?\} trt_profile;", src, flags=re.S)
    assert re.search(r"\(none: build-defined[^\n]*\n[^\n]*trt_glow_profile\*\n", text)
    # the rule is stated operation for operation, and so is what is out of scope
    for needle in ("inv_steps = 1.0f / (float)steps", "fma((float)k + 0.5f, h, u)", "0.288675135f", "1.0f / (r * r)", "kn = min((int)y, 15)",
                   "(a-_c + a+_c) * 0.5f", "a fused camera form", "shaped cross-sections", "knot counts other than 17",
                   "adapt per piece", "(e s' - e' s) h^3 / 12"):
        assert needle in text, needle


def test_the_calls_are_exported_and_refuse_a_null_ctx():
    L = lib.load()
    assert hasattr(L, "trt_glow_profile") and hasattr(L, "trt_glow_profile_dev")
    assert C.sizeof(abi.trt_profile) == 272 and abi.TRT_PROFILE_KNOTS == 17 and abi.TRT_MAX_GLOW_STEPS == 64
    rays = abi.trt_rays()
    prof = abi.profiles([((1.0, 0.5, 0.25), 2.0)])
    out = np.full(8, 7.0, np.float32)
    assert L.trt_glow_profile(None, C.byref(rays), None, None, prof, 4, 0.001, 1.0, out.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_glow_profile_dev(None, C.byref(rays), None, None, prof, 4, 0.001, 1.0, out.ctypes.data, None) == abi.TRT_E_INVALID
    assert (out == 7.0).all()


def test_the_profile_helpers():
    knots = lambda p: np.array([[p.knot[k][c] for c in range(4)] for k in range(17)], np.float32)
    line = abi.profile_from(lambda x: ((1.0 - x, 0.5, x), 2.0 * x))
    assert np.array_equal(knots(line), np.float32([[1.0 - k / 16.0, 0.5, k / 16.0, k / 8.0] for k in range(17)]))
    assert np.array_equal(knots(abi.profile_from(lambda x: (x, 0.0, 1.0, 3.0))), np.float32([[k / 16.0, 0.0, 1.0, 3.0] for k in range(17)]))
    table = pt.PROFILES["single"]["curved"][0]
    arr = abi.profiles([line, None, ((1.0, 0.5, 0.25), 2.0), lambda x: ((x * x, 0.0, 0.0), 0.0), table])
    assert len(arr) == 5 and abi.profiles(arr) is arr and arr._type_ is abi.trt_profile
    assert np.array_equal(knots(arr[0]), knots(line)) and not knots(arr[1]).any()
    assert np.array_equal(knots(arr[2]), np.tile(np.float32([1.0, 0.5, 0.25, 2.0]), (17, 1)))
    assert np.array_equal(knots(arr[3])[:, 0], np.float32([(k / 16.0) ** 2 for k in range(17)]))
    assert np.array_equal(knots(arr[4]), table)


def test_tracer_and_host_mirror_have_the_bindings():
    from toroidal_ray_tracing_amd.tracer import Tracer
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Tracer.glow_profile) == ["self", "scene", "o", "d", "profiles", "steps", "tmin", "tmax", "tmax_per_ray"]
    assert sig(Tracer.glow_profile_dev) == ["self", "scene", "ray_ptrs", "n", "profiles", "rgba_ptr", "steps", "tmax_ptr", "tmin", "tmax", "stream"]
    defaults = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not p.empty}
    assert {k: v for k, v in defaults(Tracer.glow_profile).items() if k != "steps"} == defaults(Tracer.glow)
    host = os.path.join(ROOT, "toroidal_ray_tracing_amd", "host")
    assert re.search(r"void glowProfile\(void\* stream,", open(os.path.join(host, "hello_hip.hpp")).read())
    body = open(os.path.join(host, "hello_hip.cpp")).read()
    assert "void HelloHip::glowProfile(" in body and "trt_glow_profile_dev(" in body


def test_example_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "examples", "plasma_profile_main.cpp")
    text = open(src).read()
    code = text[text.rindex("#include"):]
    for call in ("trt_camera_rays(", "trt_chords(", "trt_glow_profile(", "TRT_PROFILE_KNOTS"):
        assert call in code, call
    mk = open(os.path.join(ROOT, "toroidal_ray_tracing_amd", "host", "Makefile")).read()
    assert "../../examples/plasma_profile" in re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    assert "../../examples/plasma_profile" in re.search(r"^clean:(.*?)\n\.PHONY", mk, flags=re.S | re.M).group(1)
    assert "examples/plasma_profile" in open(os.path.join(ROOT, ".gitignore")).read().split()
    pkg = os.path.join(ROOT, "toroidal_ray_tracing_amd")
    exe = str(tmp_path / "plasma_profile")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src, "-L" + pkg, "-ltrt", "-Wl,-rpath," + pkg],
                       capture_output=True, text=True)
    assert p.returncode == 0 and os.path.exists(exe), p.stdout + p.stderr


# ---------------------------------------------------------------------------------------------------------------------
# the rule in FP64
# ---------------------------------------------------------------------------------------------------------------------
def test_known_answer():
    """Along a ray parallel to the axis at offset q, rho² = q² + s² with s the height: the profile e · (1 - x) is a
    parabola in s, its integral e · 4 a³ / (3 r²), and two Gauss points integrate a cubic exactly — one sub-step meets
    it at FP64 rounding, and so does every other step count."""
    c, table, e, want = pt.known_answer_case()
    assert (c["chords"][0] > 0.2).all() and c["robust"].all()
    for steps in (1, 2, 7):
        L, T = pt.same_rule(c, [table], steps)
        np.testing.assert_allclose(L, want, rtol=1e-12, atol=0)
        assert (T == 1.0).all()


def test_order():
    """The order of the rule, on the first 1024 lines of sight of `single` (sigma up to 0.75 per unit length), for the rays
    whose error at 8 steps stands above 1e-9 — FP64 noise is near 1e-15 — against `converged`.
    Linear profiles, the four channels on one line (emission / sigma constant along a sub-step), with absorption: the
    largest error of L over those rays, and the median of the rays' own ratios, fall by at least 8 per doubling over
    2 -> 4 -> 8 steps (theory: 16, the margin of 2 for the pre-asymptotic range; measured: 21.6 and 15.2 for the largest
    error, 15.96 and 16.00 in the median).  A single ray may fall short where its error changes sign or a long piece is
    still pre-asymptotic at 2 steps.
    A line of its own per channel (`slanted`): emission / sigma varies along a sub-step and the homogeneous step leaves
    (e s' - e' s) h³ / 12 — second order, a factor 4 per doubling (measured 2.8 and 3.5 for the largest error, 3.45 and
    3.87 in the median): at least 2 is asserted, the same margin of 2, and less than 8, so that include/trt.h does not
    promise more than the rule gives."""
    full = mt.case("single", "los")
    sel = slice(0, 1024)
    c = mt.truth_of(full["o"][sel], full["d"][sel], full["geo"], full["axes"], full["media"], full["tmin"], full["tmax"])
    c.update(o=full["o"][sel], d=full["d"][sel], geo=full["geo"], axes=full["axes"])
    for shape, lo, hi in (("linear", 8.0, np.inf), ("slanted", 2.0, 8.0)):
        tables = pt.PROFILES["single"][shape]
        Lc, Tc, change = pt.converged(c, tables) if shape == "linear" else pt.same_rule(c, tables, 2048) + (None,)
        err = {s: np.abs(pt.same_rule(c, tables, s)[0] - Lc).max(1) for s in (2, 4, 8)}
        above = err[8] > 1e-9
        worst = [err[s][above].max() for s in (2, 4, 8)]
        median = [np.median(err[a][above] / err[b][above]) for a, b in ((2, 4), (4, 8))]
        print(f"{shape}: {int(above.sum())} rays; largest error at 2, 4, 8 steps {worst[0]:.3e} {worst[1]:.3e} {worst[2]:.3e} "
              f"(ratios {worst[0] / worst[1]:.2f}, {worst[1] / worst[2]:.2f}); median ratio per ray {median[0]:.2f}, {median[1]:.2f}; "
              f"last change of the reference {change}")
        assert above.sum() > 500
        if change is not None:
            assert change <= 1e-11
        for ratio in (worst[0] / worst[1], worst[1] / worst[2], median[0], median[1]):
            assert lo <= ratio < hi, (shape, ratio)


@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", mt.NAMES)
def test_a_flat_profile_is_the_closed_form(name, kind):
    """Every knot of torus j equal to medium j: whatever the steps, the sub-steps of a piece multiply up to the piece's
    closed form — media_truth's glow, at FP64 rounding."""
    c = mt.case(name, kind)
    tables = pt.PROFILES[name]["flat"]
    media = [(tuple(float(v) for v in t[0, :3]), float(t[0, 3])) for t in tables]   # (the media as FP32 holds them)
    want_L, want_T = mt.glow(c["A"], c["B"], c["d"], media, c["tmin"], c["info"]["tmax_i"])
    for steps in (1, 3, 16):
        L, T = pt.same_rule(c, tables, steps)
        np.testing.assert_allclose(L, want_L, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(T, want_T, rtol=1e-12, atol=0)
    assert (want_L.max(1) > 1e-3).mean() > 0.2


@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", mt.NAMES)
def test_the_gpu_tests_leave_few_rays_out(name, kind):
    """tests/test_gpu_profile.py compares on media_truth's `robust` rays: their share stays within media_truth.CAPS."""
    c = mt.case(name, kind)
    assert 1.0 - c["robust"].mean() <= mt.CAPS[name], (name, kind)
    tables = pt.PROFILES[name]["curved"]
    assert all(t.shape == (17, 4) and t.dtype == np.float32 and (t >= 0).all() for t in tables)
    assert [bool(t.any()) for t in tables] == [any(v != 0 for v in (*m[0], m[1])) for m in mt.MEDIA[name]]


def test_a_zero_table_is_the_scene_without_the_torus():
    """Torus 5 of the nest of eight holds no medium: its walls are no break points, so the sub-steps of its neighbours'
    pieces sit where they sit in the scene of seven — the same numbers at FP64 rounding, at a step count coarse enough
    to tell."""
    c = mt.case("nest8", "los")
    tables = pt.PROFILES["nest8"]["curved"]
    keep = [j for j in range(8) if j != 5]
    sel = slice(0, 512)
    o, d = c["o"][sel], c["d"][sel]
    with_it = mt.truth_of(o, d, c["geo"], c["axes"], c["media"], c["tmin"], c["tmax"])
    with_it.update(o=o, d=d, geo=c["geo"], axes=c["axes"])
    geo7, axes7 = [c["geo"][j] for j in keep], None if c["axes"] is None else [c["axes"][j] for j in keep]
    without = mt.truth_of(o, d, geo7, axes7, [c["media"][j] for j in keep], c["tmin"], c["tmax"])
    without.update(o=o, d=d, geo=geo7, axes=axes7)
    L8, T8 = pt.same_rule(with_it, tables, 2)
    L7, T7 = pt.same_rule(without, [tables[j] for j in keep], 2)
    np.testing.assert_allclose(L8, L7, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(T8, T7, rtol=1e-12, atol=0)
    assert (L8.max(1) > 1e-3).mean() > 0.2
