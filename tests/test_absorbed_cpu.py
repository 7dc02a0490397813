"""trt_glow_weights_absorbed, the part that needs no GPU: the prototypes against the header and lib.SYMBOLS, the bindings,
the example wired into the host Makefile — and the rule itself, restated in FP64 by tests/absorbed_truth.py: the forward
identity with trt_glow_profile's rule at any sigma and any number of tori, the plain weights and the chords without
absorption, the closed form of an axis-parallel ray through a flat sigma, the order at which the single weights converge,
and the condition number of the example's normal matrix."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import absorbed_truth as at
import media_truth as mt
import profile_truth as pt
import weights_truth as wt
from conftest import ROOT
from toroidal_ray_tracing_amd import abi, lib

HEADER = os.path.join(ROOT, "include", "trt.h")
PARAMS = ["trt_ctx*", "const trt_rays*", "const float*", "const trt_scene*", "const trt_profile*", "uint32_t", "float", "float",
          "float*", "float*"]
CTYPES = {
    "trt_ctx*": C.c_void_p, "const trt_rays*": C.POINTER(abi.trt_rays), "float": C.c_float, "uint32_t": C.c_uint32,
    "const trt_scene*": C.POINTER(abi.trt_scene), "const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p,
    "const trt_profile*": C.POINTER(abi.trt_profile),
}
#: the condition number of the example's normal matrix (test_the_condition_number_of_the_example pins it)
EXAMPLE_COND = 5.80e3


def tables_of(name, shape="curved"):
    """The scene's tables with every torus present: torus 5 of `nest8` (all zero) gets torus 4's, so that
    trt_glow_profile's rule and this one cut the same pieces."""
    tables = [np.array(t) for t in pt.PROFILES[name][shape]]
    if name == "nest8":
        tables[5] = np.array(tables[4])
    assert all(t.any() for t in tables)
    return tables


def test_prototypes_match_the_header_and_the_bindings_exist():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, params in (("trt_glow_weights_absorbed", PARAMS), ("trt_glow_weights_absorbed_dev", PARAMS + ["void*"])):
        m = re.search(r"^int %s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        got = [re.match(r"(.*?)\s*\b\w+$", " ".join(p.split())).group(1).strip() for p in m.group(1).split(",")]
        assert got == params, name
        res, args = lib.SYMBOLS[name]
        assert res is C.c_int and args == [CTYPES[p] for p in params], name
    assert re.search(r"\(none: build-defined[^\n]*\n[^\n]*trt_glow_weights_absorbed\*\n", text)
    body = text[text.index("glow_weights_absorbed(rays_in"):]
    for needle in ("a = a + fma(f, sigma_j[kn + 1] - sigma_j[kn], sigma_j[kn])", "sg = (a- + a+) * 0.5f;", "g = (w * 0.5f) * T",
                   "W[j][kn]     = fma(g, 1.0f - f, W[j][kn]);", "W[j][kn + 1] = fma(g, f, W[j][kn + 1]);", "T = T * E.",
                   "The order of the additions into each accumulator is part of the contract", "Transmittance.", "Forward.",
                   "No absorption.", "A torus alone.", "Partition.", "Scale.", "the response to a sigma knot", "a matrix-free",
                   "a torus mask", "a fused camera form", "a solver for the fit"):
        assert needle in body, needle
    L = lib.load()
    rays = abi.trt_rays()
    out = np.full(17 * 2, 7.0, np.float32)
    prof = (abi.trt_profile * 1)()
    assert L.trt_glow_weights_absorbed(None, C.byref(rays), None, None, prof, 4, 0.001, 1.0, out.ctypes.data, None) == abi.TRT_E_INVALID
    assert L.trt_glow_weights_absorbed_dev(None, C.byref(rays), None, None, prof, 4, 0.001, 1.0, out.ctypes.data, None, None) == abi.TRT_E_INVALID
    assert (out == 7.0).all()
    from toroidal_ray_tracing_amd.tracer import Tracer
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Tracer.glow_weights_absorbed) == ["self", "scene", "o", "d", "profiles", "steps", "tmin", "tmax", "tmax_per_ray"]
    assert sig(Tracer.glow_weights_absorbed_dev) == ["self", "scene", "ray_ptrs", "n", "profiles", "weight_ptr", "trans_ptr", "steps",
                                                     "tmax_ptr", "tmin", "tmax", "stream"]
    host = os.path.join(ROOT, "toroidal_ray_tracing_amd", "host")
    assert re.search(r"void glowWeightsAbsorbed\(void\* stream,", open(os.path.join(host, "hello_hip.hpp")).read())
    code = open(os.path.join(host, "hello_hip.cpp")).read()
    assert "void HelloHip::glowWeightsAbsorbed(" in code and "trt_glow_weights_absorbed_dev(" in code
    mk = open(os.path.join(host, "Makefile")).read()
    assert "../../examples/absorbed_fit" in re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    assert "../../examples/absorbed_fit" in re.search(r"^clean:(.*?)\n\.PHONY", mk, flags=re.S | re.M).group(1)
    assert "examples/absorbed_fit" in open(os.path.join(ROOT, ".gitignore")).read().split()
    example = open(os.path.join(ROOT, "examples", "absorbed_fit_main.cpp")).read()
    assert "condition number of the absorbed matrix is 5.80e3" in example and EXAMPLE_COND == 5.80e3


@pytest.mark.parametrize("kind", mt.KINDS)
@pytest.mark.parametrize("name", ["nest3", "rings2", "nest8"])
def test_forward_is_the_profile_rule_with_any_sigma(name, kind):
    """sum_jk W[j][k] · knot_j[k][c] is profile_truth.same_rule's L at the same steps, and T is equal: any number of tori,
    any sigma, every torus present on both sides."""
    c = mt.case(name, kind)
    tables = tables_of(name)
    for steps in (1, 4):
        L, T = pt.same_rule(c, tables, steps)
        W, Tw = at.same_rule(c, tables, steps)
        got = wt.forward(W, tables)[:, :3]
        err = np.abs(got - L) / (1.0 + np.abs(L))
        print(f"{name} {kind} {steps} steps: forward {err.max():.2e}, T {np.abs(Tw - T).max():.2e}")
        assert (err <= 1e-13).all() and np.array_equal(Tw, T)
        assert (W >= 0).all() and (T < 0.99).mean() > 0.2


def zero_tables(n_tori):
    return [np.zeros(17) for _ in range(n_tori)]


def test_without_absorption_the_weights_are_the_plain_ones_where_no_tubes_overlap():
    for name in ("single", "rings2"):
        for kind in mt.KINDS:
            c = mt.case(name, kind)
            A, B = c["A"], c["B"]
            for j in range(len(A)):   # no interval of torus j overlaps one of a later torus, on any ray
                for i in range(j + 1, len(A)):
                    with np.errstate(invalid="ignore"):
                        lap = (A[j][:, :, None] < B[i][:, None, :]) & (A[i][:, None, :] < B[j][:, :, None])
                    assert not lap.any(), (name, kind, j, i)
            for steps in (1, 4):
                W, T = at.same_rule(c, zero_tables(len(A)), steps)
                np.testing.assert_allclose(W, wt.same_rule(c, steps), rtol=1e-13, atol=1e-16)
                assert (T == 1.0).all()


@pytest.mark.parametrize("name", mt.NAMES)
def test_without_absorption_the_weights_sum_to_the_chords(name):
    for kind in mt.KINDS:
        c = mt.case(name, kind)
        W, T = at.same_rule(c, zero_tables(len(c["geo"])), 4)
        np.testing.assert_allclose(W.sum(1), c["chords"], rtol=1e-12, atol=1e-14)
        assert (T == 1.0).all()


def axis_case():
    c, table, e, want = pt.known_answer_case()
    r = c["geo"][0][2]
    a = np.cbrt(want[:, 0] / e[0] * 3.0 * r * r / 4.0)   # the half chord, as tests/test_gpu_weights.py recovers it
    return c, r, a


KNOWN_SIGMA = 1.25


def test_the_known_answer():
    """A ray parallel to the axis through a flat sigma: every sub-step sees the same sigma, so the steps telescope —
    sum_k W_k = (1 - exp(-2 a sigma)) / sigma to rounding at any step count, and T = exp(-2 a sigma)."""
    c, r, a = axis_case()
    for steps in (1, 4, 7):
        W, T = at.same_rule(c, [np.full(17, KNOWN_SIGMA)], steps)
        np.testing.assert_allclose(W[0].sum(0), -np.expm1(-2.0 * a * KNOWN_SIGMA) / KNOWN_SIGMA, rtol=1e-12)
        np.testing.assert_allclose(T, np.exp(-2.0 * a * KNOWN_SIGMA), rtol=1e-12)


def test_order_of_the_single_weights():
    """Against profile_truth.converged: the weight of knot k is the radiance of the table whose emission is the hat of knot
    k (three knots a call, one per channel) behind the same sigma.  A hat has kinks at the knots, so the rule is of second
    order in the single weights: halving the sub-steps divides the error of a ray's worst weight by about 4.  The median
    ratio over the rays is printed; asserted: between 2 and 8.  Measured: 3.99 (8 -> 16 steps) and 4.99 (16 -> 32)."""
    c, r, a = axis_case()
    sigma = at.example_sigma().astype(np.float64)
    want = np.zeros((17, len(a)))
    for k0 in range(0, 17, 3):
        table = np.zeros((17, 4))
        table[:, 3] = sigma
        ks = [k for k in range(k0, min(k0 + 3, 17))]
        for ch, k in enumerate(ks):
            table[k, ch] = 1.0
        L, _, _ = pt.converged(c, [table], start=256, limit=512)
        want[ks] = L[:, :len(ks)].T
    err = {s: np.abs(at.same_rule(c, [sigma], s)[0][0] - want).max(0) for s in (8, 16, 32)}
    assert (err[32] > 1e-7).all()   # far above what is left at the converged count
    for s0, s1 in ((8, 16), (16, 32)):
        median = np.median(err[s0] / err[s1])
        print(f"{s0} -> {s1} steps: largest error {err[s0].max():.3e} -> {err[s1].max():.3e}; median ratio per ray {median:.2f}")
        assert 2.0 <= median <= 8.0, (s0, s1, median)


def test_the_condition_number_of_the_example():
    """examples/absorbed_fit_main.cpp's normal matrix on its 32 x 24 camera rays at 64 steps, in FP64; the fit through the
    absorbed weights gives the table back, the fit through the plain ones does not."""
    c = at.example_case()
    table = at.example_table().astype(np.float64)
    W, T = at.same_rule(c, [table], at.EXAMPLE_STEPS)
    cond = np.linalg.cond(wt.normal_matrix(W[0]))
    print(f"condition number {cond:.4e}; min T {T.min():.4f}")
    np.testing.assert_allclose(cond, EXAMPLE_COND, rtol=0.01)
    assert T.min() < 0.6
    y = W[0].T @ table[:, :3]
    got = np.linalg.solve(wt.normal_matrix(W[0]), W[0] @ y)
    assert np.abs(got - table[:, :3]).max() < cond * wt.EXAMPLE_RIDGE
    plain = wt.same_rule(c, at.EXAMPLE_STEPS)[0]
    biased = np.linalg.solve(wt.normal_matrix(plain), plain @ y)
    assert np.abs(biased - table[:, :3]).max() > 0.05
