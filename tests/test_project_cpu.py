"""trt_glow_project / trt_glow_backproject, the part that needs no GPU: the prototypes against the header and lib.SYMBOLS,
the bindings, the example wired into the host Makefile — and the truth the GPU tests hold the calls to
(tests/project_truth.py), checked before the GPU is held to it: its two operators are adjoint, and ANY order of the
additions stays within its bar."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import absorbed_truth as at
import media_truth as mt
import project_truth as prt
from conftest import ROOT
from test_absorbed_cpu import CTYPES, HEADER, tables_of
from toroidal_ray_tracing_amd import abi, lib

f32, f64 = np.float32, np.float64
HEAD = ["trt_ctx*", "const trt_rays*", "const float*", "const trt_scene*", "const trt_profile*", "uint32_t", "float", "float"]
PROTOTYPES = {
    "trt_glow_project": HEAD + ["float*"],
    "trt_glow_project_dev": HEAD + ["float*", "void*"],
    "trt_glow_backproject": HEAD + ["const float*", "double*"],
    "trt_glow_backproject_dev": HEAD + ["const float*", "double*", "void*"],
}
N = 500


@pytest.fixture(scope="module")
def small():
    """(W float32 (3, 17, N), tables, y float32 (N, 4) of mixed sign): the rule in FP64 on `nest3`'s segments, rounded to
    the float matrix the library returns."""
    c = mt.case("nest3", "seg")
    tables = tables_of("nest3")
    W, _ = at.same_rule(c, tables, 4)
    W = np.ascontiguousarray(W[:, :, :N].astype(f32))
    y = np.random.default_rng(5).normal(size=(N, 4)).astype(f32)
    assert (W > 0).any(2).sum() > 20 and (y[:, :3] < 0).any() and (y[:, :3] > 0).any()
    return W, tables, y


def test_prototypes_match_the_header_and_the_bindings_exist():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctypes_of = dict(CTYPES, **{"double*": C.c_void_p})
    for name, params in PROTOTYPES.items():
        m = re.search(r"^int %s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        got = [re.match(r"(.*?)\s*\b\w+$", " ".join(p.split())).group(1).strip() for p in m.group(1).split(",")]
        assert got == params, name
        res, args = lib.SYMBOLS[name]
        assert res is C.c_int and args == [ctypes_of[p] for p in params], name
    assert re.search(r"\(none: build-defined[^\n]*\n[^\n]*trt_glow_project\* / trt_glow_backproject\*\n", text)
    body = text[text.index("glow_project(rays_in"):]
    for needle in ("BIT FOR BIT", "p = p + (double)W[j][k][i] * (double)knot_j[k][c];", "L_c = (float)p;", "(0, 0, 0, 1)",
                   "back[(j * 17 + k) * 4 + c] = sum over i of W[j][k][i] * y[4 i + c]", "back[(j * 17 + k) * 4 + 3] = sum over i of W[j][k][i]",
                   "channel 3 is IGNORED", "NOT trt_glow_weights' uncut intervals", "n * 2^-53 * sum over i of |W * y|",
                   "a sum whose terms are all zero is 0.0", "no floating-point atomics", "writes n_tori * 17 * 4 zeros",
                   "W^T W", "a torus mask", "a fused camera form", "a solver for the fit", "make one eager call"):
        assert needle in body, needle
    # the "Not here" lists of the two weight calls no longer count the matrix-free products among what is missing
    for start in ("glow_weights(rays_in", "glow_weights_absorbed(rays_in"):
        part = text[text.index(start):]
        not_here = part[part.index("Not here:"):part.index("Host buffers:")]
        assert "trt_glow_backproject" in not_here and "W^T W" in not_here, start
    L = lib.load()
    rays = abi.trt_rays()
    out = np.full(17 * 4, 7.0, f64)
    prof = (abi.trt_profile * 1)()
    for call in (lambda: L.trt_glow_project(None, C.byref(rays), None, None, prof, 4, 0.001, 1.0, out.ctypes.data),
                 lambda: L.trt_glow_project_dev(None, C.byref(rays), None, None, prof, 4, 0.001, 1.0, out.ctypes.data, None),
                 lambda: L.trt_glow_backproject(None, C.byref(rays), None, None, prof, 4, 0.001, 1.0, out.ctypes.data, out.ctypes.data),
                 lambda: L.trt_glow_backproject_dev(None, C.byref(rays), None, None, prof, 4, 0.001, 1.0, out.ctypes.data, out.ctypes.data, None)):
        assert call() == abi.TRT_E_INVALID
    assert (out == 7.0).all()
    from toroidal_ray_tracing_amd.tracer import Tracer
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Tracer.glow_project) == ["self", "scene", "o", "d", "profiles", "steps", "tmin", "tmax", "tmax_per_ray"]
    assert sig(Tracer.glow_project_dev) == ["self", "scene", "ray_ptrs", "n", "profiles", "rgba_ptr", "steps", "tmax_ptr", "tmin", "tmax", "stream"]
    assert sig(Tracer.glow_backproject) == ["self", "scene", "o", "d", "y", "profiles", "steps", "tmin", "tmax", "tmax_per_ray"]
    assert sig(Tracer.glow_backproject_dev) == ["self", "scene", "ray_ptrs", "n", "y_ptr", "back_ptr", "profiles", "steps", "tmax_ptr", "tmin",
                                                "tmax", "stream"]
    host = os.path.join(ROOT, "toroidal_ray_tracing_amd", "host")
    hpp, code = open(os.path.join(host, "hello_hip.hpp")).read(), open(os.path.join(host, "hello_hip.cpp")).read()
    for method, entry in (("glowProject", "trt_glow_project_dev("), ("glowBackproject", "trt_glow_backproject_dev(")):
        assert re.search(r"void %s\(void\* stream," % method, hpp) and "void HelloHip::%s(" % method in code and entry in code, method
    mk = open(os.path.join(host, "Makefile")).read()
    assert "../../examples/matrix_free_fit" in re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    assert "../../examples/matrix_free_fit" in re.search(r"^clean:(.*?)\n\.PHONY", mk, flags=re.S | re.M).group(1)
    assert "examples/matrix_free_fit" in open(os.path.join(ROOT, ".gitignore")).read().split()
    example = open(os.path.join(ROOT, "examples", "matrix_free_fit_main.cpp")).read()
    assert "trt_glow_project(" in example and "trt_glow_backproject(" in example and "trt_glow_weights" not in example


def test_the_truths_operators_are_adjoint(small):
    """<y, project(W, x)> against <backproject_exact(W, y), x> per channel, at project_truth.adjoint_bar with the exact
    back-projection's one rounding: the float rounding of every forward output is all that separates the two."""
    W, tables, y = small
    L = prt.project(W, tables)
    back = prt.backproject_exact(W, y)
    lhs, rhs = prt.inner_forward(y, L), prt.inner_back(back, tables)
    bar = prt.adjoint_bar(W, tables, y, L, 1)
    print(f"adjoint on the truth: |lhs - rhs| / bar {np.abs(lhs - rhs) / bar}, relative {np.abs(lhs - rhs) / np.abs(lhs)}")
    assert (np.abs(lhs - rhs) <= bar).all() and (np.abs(lhs) > 100 * bar).all()
    # without the float rounding the identity holds to the FP64 part of the bar alone
    p = np.zeros((N, 3))
    for j in range(W.shape[0]):
        for k in range(17):
            p = p + W[j, k].astype(f64)[:, None] * tables[j][k, :3].astype(f64)[None, :]
    exact_lhs = np.array([math.fsum((y[:, c].astype(f64) * p[:, c]).tolist()) for c in range(3)])
    assert (np.abs(exact_lhs - rhs) <= bar - 2.0 ** -24 * np.abs(y[:, :3].astype(f64) * L).sum(0)).all()
    # the forward chain is the stated one: one ray by hand, in Python floats
    i = int(np.argmax(W.sum((0, 1))))
    for c in range(3):
        acc = 0.0
        for j in range(W.shape[0]):
            for k in range(17):
                acc = acc + float(W[j, k, i]) * float(f32(tables[j][k, c]))
        assert f32(acc) == L[i, c] and L[i, c] > 0


def test_any_order_of_the_additions_stays_within_the_bar(small):
    """Sequential in several shuffled orders, blocked (64 lanes, then the blocks — the kernel's shape) and a pairwise tree:
    all within backproject_bar of backproject_exact, every entry, and an entry without a non-zero term is 0.0 in bits."""
    W, tables, y = small
    W = np.array(W)
    W[1, 5] = 0.0   # a knot no ray of the set sees: its terms are +0.0 and -0.0, by the sign of y
    exact, bar, t = prt.backproject_exact(W, y), prt.backproject_bar(W, y), prt.terms(W, y)
    rng = np.random.default_rng(17)

    def sequential(order):
        s = np.zeros(t.shape[:3])
        for i in order:
            s = s + t[..., i]
        return s

    def pairwise(v):
        while v.shape[-1] > 1:
            if v.shape[-1] % 2:
                v = np.concatenate([v, np.zeros(v.shape[:-1] + (1,))], -1)
            v = v[..., 0::2] + v[..., 1::2]
        return v[..., 0]

    def blocked(width):
        s = np.zeros(t.shape[:3])
        for b in range(0, N, width):
            s = s + sequential(range(b, min(b + width, N)))
        return s

    sums = [sequential(range(N)), sequential(range(N - 1, -1, -1))] + [sequential(rng.permutation(N)) for _ in range(4)]
    sums += [pairwise(t), blocked(64), blocked(256)]
    worst = max(np.nanmax(np.where(bar > 0, np.abs(s - exact) / np.where(bar > 0, bar, 1.0), 0.0)) for s in sums)
    print(f"largest error / bar over {len(sums)} orders: {worst:.4f}")
    for s in sums:
        assert (np.abs(s - exact) <= bar).all()
        assert (s[bar == 0].view(np.uint64) == 0).all()
    assert len({s.tobytes() for s in sums}) > 1, "the orders do differ in bits"
    assert (bar == 0).any() and (bar > 0).sum() > 50 and 0 < worst < 1
    # channel 3 is the column sum, whatever y holds there
    odd = np.array(y)
    odd[:, 3] = np.nan
    assert np.array_equal(prt.backproject_exact(W, odd), exact)
    assert np.allclose(exact[:, :, 3], W.astype(f64).sum(2), rtol=1e-12, atol=0)
