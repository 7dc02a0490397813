"""trt_glow_tangent / trt_glow_adjoint, the part that needs no GPU: the prototypes against the header and lib.SYMBOLS, the
bindings, the example wired into the host Makefile — and the FP64 truth of tests/jacobian_truth.py held to what it does
not share anything with: central differences of the forward rule (absorbed_truth.same_rule), the forward rule itself in
an emission-only direction, the closed form of an axis-parallel ray through a flat medium, its own other mode (the inner
product identity), same_rule's W, and the sign of the sigma gradient."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import absorbed_truth as at
import jacobian_truth as jt
import media_truth as mt
import profile_truth as pt
from conftest import ROOT
from test_absorbed_cpu import CTYPES, tables_of
from toroidal_ray_tracing_amd import abi, lib

HEADER = os.path.join(ROOT, "include", "trt.h")
HEAD = ["trt_ctx*", "const trt_rays*", "const float*", "const trt_scene*", "const trt_profile*"]
TANGENT = HEAD + ["const trt_profile*", "uint32_t", "float", "float", "float*"]
ADJOINT = HEAD + ["uint32_t", "float", "float", "const float*", "double*"]
U = 2.0 ** -53
N_RAYS = 384   # a slice of a media_truth set: enough rays of every kind, and the truth in a second or two
STEPS = 4


def sub_case(name, kind, n=N_RAYS, start=100):
    """The rays start .. start + n of a media_truth case, as the truth modules read a case."""
    c = mt.case(name, kind)
    s = slice(start, start + n)
    return dict(A=c["A"][:, s], B=c["B"][:, s], o=c["o"][s], d=c["d"][s], geo=c["geo"], axes=c["axes"])


def random_direction(tables, seed, channels=(0, 1, 2, 3)):
    """A direction of mixed sign, every entry within the size of the table's own: tables + t * delta stays positive for |t| < 1."""
    rng = np.random.default_rng(seed)
    out = []
    for t in tables:
        v = np.zeros((17, 4))
        v[:, channels] = (np.asarray(t, np.float64) * rng.uniform(-1.0, 1.0, (17, 4)))[:, channels]
        out.append(v)
    return out


_shared = {}


def shared(name, kind):
    """(case, tables, geometry, direction, image, tangent, adjoint) of a sub-case at STEPS, made once."""
    key = (name, kind)
    if key not in _shared:
        c, tables = sub_case(name, kind), tables_of(name)
        geo = jt.geometry(c, STEPS)
        delta = random_direction(tables, 5)
        y = np.random.default_rng(7).normal(size=(N_RAYS, 4))
        _shared[key] = (c, tables, geo, delta, y, jt.tangent(c, tables, delta, STEPS, geo), jt.adjoint(c, tables, y, STEPS, geo))
    return _shared[key]


def count_of(geo, n_tori):
    """The count of test_forward_and_reverse_mode_are_adjoint's docstring: 2 * S + 16 * n_tori + 64, S the most sub-steps of a ray."""
    S = np.zeros(N_RAYS)
    for piece in geo:
        S[piece["rows"]] += STEPS
    return 2 * S.max() + 16 * n_tori + 64


def forward_rule(c, tables, steps):
    """(n, 4) of absorbed_truth.same_rule: sum_jk W knot per colour, and T."""
    W, T = at.same_rule(c, tables, steps)
    L = np.einsum("jkn,jkc->nc", W, np.stack([np.asarray(t, np.float64)[:, :3] for t in tables]))
    return np.concatenate([L, T[:, None]], 1)


def test_prototypes_match_the_header_and_the_bindings_exist():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    types = dict(CTYPES, **{"double*": C.c_void_p})
    for name, params in (("trt_glow_tangent", TANGENT), ("trt_glow_tangent_dev", TANGENT + ["void*"]),
                         ("trt_glow_adjoint", ADJOINT), ("trt_glow_adjoint_dev", ADJOINT + ["void*"])):
        m = re.search(r"^int %s\s*\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        got = [re.match(r"(.*?)\s*\b\w+$", " ".join(p.split())).group(1).strip() for p in m.group(1).split(",")]
        assert got == params, name
        res, args = lib.SYMBOLS[name]
        assert res is C.c_int and args == [types[p] for p in params], name
    assert re.search(r"trt_glow_tangent\* / trt_glow_adjoint\*\n", text)
    body = text[text.index("glow_tangent(rays_in"):]
    for needle in ("ALL FOUR CHANNELS ARE READ", "WHICH IGNORES CHANNEL 3", "THE ORDER OF THE FP32 OPERATIONS IS NOT PART OF EITHER CONTRACT",
                   "ANY SIGN", "(0, 0, 0, 0)", "l^2 * Q(tau)", "trt_glow_backproject_dev's rule"):
        assert needle in body, needle
    L = lib.load()
    rays = abi.trt_rays()
    out = np.full(17 * 4, 7.0, np.float64)
    prof = (abi.trt_profile * 1)()
    assert L.trt_glow_tangent(None, C.byref(rays), None, None, prof, prof, 4, 0.001, 1.0, out.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_glow_tangent_dev(None, C.byref(rays), None, None, prof, prof, 4, 0.001, 1.0, out.ctypes.data, None) == abi.TRT_E_INVALID
    assert L.trt_glow_adjoint(None, C.byref(rays), None, None, prof, 4, 0.001, 1.0, None, out.ctypes.data) == abi.TRT_E_INVALID
    assert L.trt_glow_adjoint_dev(None, C.byref(rays), None, None, prof, 4, 0.001, 1.0, None, out.ctypes.data, None) == abi.TRT_E_INVALID
    assert (out == 7.0).all()
    from toroidal_ray_tracing_amd.tracer import Tracer
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Tracer.glow_tangent) == ["self", "scene", "o", "d", "profiles", "delta", "steps", "tmin", "tmax", "tmax_per_ray"]
    assert sig(Tracer.glow_tangent_dev) == ["self", "scene", "ray_ptrs", "n", "profiles", "delta", "rgba_ptr", "steps", "tmax_ptr", "tmin",
                                            "tmax", "stream"]
    assert sig(Tracer.glow_adjoint) == ["self", "scene", "o", "d", "y", "profiles", "steps", "tmin", "tmax", "tmax_per_ray"]
    assert sig(Tracer.glow_adjoint_dev) == ["self", "scene", "ray_ptrs", "n", "y_ptr", "grad_ptr", "profiles", "steps", "tmax_ptr", "tmin",
                                            "tmax", "stream"]
    host = os.path.join(ROOT, "toroidal_ray_tracing_amd", "host")
    hpp, code = open(os.path.join(host, "hello_hip.hpp")).read(), open(os.path.join(host, "hello_hip.cpp")).read()
    assert re.search(r"void glowTangent\(void\* stream,", hpp) and re.search(r"void glowAdjoint\(void\* stream,", hpp)
    assert "trt_glow_tangent_dev(" in code and "trt_glow_adjoint_dev(" in code
    mk = open(os.path.join(host, "Makefile")).read()
    assert "../../examples/sigma_fit" in re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    assert "../../examples/sigma_fit" in re.search(r"^clean:(.*?)\n\.PHONY", mk, flags=re.S | re.M).group(1)
    assert "examples/sigma_fit" in open(os.path.join(ROOT, ".gitignore")).read().split()


@pytest.mark.parametrize("name,kind", [("single", "los"), ("nest3", "seg"), ("rings2", "cut")])
def test_the_tangent_is_the_limit_of_central_differences(name, kind):
    """(F(p + t delta) - F(p - t delta)) / 2t with F = absorbed_truth.same_rule's (sum W knot, T) differs from the tangent
    by t^2 F''' / 6: over the entries whose disagreement at t stands above the roundoff floor 2^-53 |F| / t, it falls by
    about 4 from t to t / 2 in the median.  Measured: a median of 4.000 in all three cases."""
    c, tables, geo, delta, _, tan, _ = shared(name, kind)
    F0 = np.abs(forward_rule(c, tables, STEPS))

    def disagreement(t):
        plus = forward_rule(c, [np.asarray(p, np.float64) + t * v for p, v in zip(tables, delta)], STEPS)
        minus = forward_rule(c, [np.asarray(p, np.float64) - t * v for p, v in zip(tables, delta)], STEPS)
        return np.abs((plus - minus) / (2.0 * t) - tan["d"])

    t = 2.0 ** -5
    e1, e2 = disagreement(t), disagreement(t / 2)
    above = e1 > U * F0 / t
    ratio = np.median(e1[above] / e2[above])
    print(f"{name} {kind}: {above.sum()} of {above.size} entries above the floor; largest disagreement {e1.max():.3e} at t, {e2.max():.3e} at t / 2; "
          f"median ratio {ratio:.3f}")
    assert above.sum() > 200 and 3.5 < ratio < 4.5


@pytest.mark.parametrize("name,kind", [("nest3", "seg"), ("nest8", "los")])
def test_an_emission_only_direction_gives_the_forward_rule_of_that_emission(name, kind):
    """F is linear in the emission: with delta's sigma zero the tangent is F(delta's emission, profiles' sigma) to FP64
    rounding — the count of test_forward_and_reverse_mode_are_adjoint times 2^-53 times the sum of the absolute terms: the
    same products, associated otherwise — and dT is exactly 0."""
    c, tables, geo, _, _, _, _ = shared(name, kind)
    delta = random_direction(tables, 9, channels=(0, 1, 2))
    tan = jt.tangent(c, tables, delta, STEPS, geo)
    mixed = [np.concatenate([v[:, :3], np.asarray(p, np.float64)[:, 3:]], 1) for p, v in zip(tables, delta)]
    want = forward_rule(c, mixed, STEPS)
    assert (tan["d"][:, 3] == 0.0).all()
    assert (np.abs(tan["d"][:, :3] - want[:, :3]) <= count_of(geo, len(tables)) * U * tan["abs"][:, :3]).all()
    assert (np.abs(tan["d"][:, :3]).max(1) > 1e-4).mean() > 0.2


def test_the_known_answer():
    """Axis-parallel rays through a flat medium (e, sigma): L = e (1 - E) / sigma with E = exp(-2 a sigma), whatever the
    step count, so in the flat sigma direction dL = e (2 a sigma E - (1 - E)) / sigma^2 and dT = -2 a T."""
    c, _, e, want_L = pt.known_answer_case()
    r = c["geo"][0][2]
    a = np.cbrt(want_L[:, 0] / e[0] * 3.0 * r * r / 4.0)
    sigma = 0.75
    table = np.tile(np.array([e[0], e[1], e[2], sigma]), (17, 1))
    delta = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (17, 1))
    E = np.exp(-2.0 * a * sigma)
    want = np.concatenate([e[None, :] * ((2.0 * a * sigma * E + np.expm1(-2.0 * a * sigma)) / sigma ** 2)[:, None], (-2.0 * a * E)[:, None]], 1)
    for steps in (1, 4, 7):
        tan = jt.tangent(c, [table], [delta], steps)
        # `a` comes from the case's own closed form through a cube root: 1e-9 relative covers its rounding
        assert np.allclose(tan["d"], want, rtol=1e-9, atol=1e-12), steps
        adj = jt.adjoint(c, [table], np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (len(a), 1)), steps)
        assert np.isclose(adj["grad"][0, :, 3].sum(), want[:, 0].sum(), rtol=1e-9), steps
    assert (want[:, :3] < 0).all() and (np.abs(want[:, 0]) > 1e-3).all()


@pytest.mark.parametrize("name,kind", [("single", "los"), ("nest3", "seg"), ("rings2", "cut"), ("nest8", "los")])
def test_forward_and_reverse_mode_are_adjoint(name, kind):
    """<y, tangent(delta)> = <adjoint(y), delta>, both inner products summed exactly (math.fsum), within
    count * 2^-53 * sum |terms|.  The count, per ray with S sub-steps in all: the same (E, w, w') bits enter both modes, so
    what differs is how the products are associated and summed.  Forward mode makes per sub-step 3 rounded products and an
    addition for each of its three terms of dL and 3 operations for dT (<= 16), reverse mode 4 for Tbar, 6 for sgbar, 2
    per hat and channel, and each of the at most 4 * n_tori hats of a sub-step is applied to delta with 2 more (<= 16 +
    8 * n_tori); a term passes through at most S such sub-steps of the running dT or Tbar (each multiplies by E: one
    rounding a step).  With the table lookup (4 per torus and point) and the final dot products: count = 2 * S + 16 *
    n_tori + 64.  Measured: at most 3e-4 of the bar."""
    c, tables, geo, delta, y, tan, adj = shared(name, kind)
    nt = len(tables)
    lhs = math.fsum((y * tan["d"]).ravel().tolist())
    rhs = math.fsum((adj["grad"] * np.stack(delta)).ravel().tolist())
    count = count_of(geo, nt)
    terms = (np.abs(y) * tan["abs"]).sum() + (adj["abs"].sum(-1) * np.abs(np.stack(delta))).sum()
    print(f"{name} {kind}: <y, J d> = {lhs:.12e}, <J^T y, d> = {rhs:.12e}, difference / bar {abs(lhs - rhs) / (count * U * terms):.4f}")
    assert abs(lhs - rhs) <= count * U * terms
    assert abs(lhs) > 1e6 * count * U * terms   # the identity is not 0 = 0: both sides stand far above the bar


@pytest.mark.parametrize("name,kind", [("nest3", "seg"), ("rings2", "cut")])
def test_the_emission_channels_of_the_adjoint_are_w_transposed_y(name, kind):
    c, tables, _, _, y, _, adj = shared(name, kind)
    W, _ = at.same_rule(c, tables, STEPS)
    want = np.einsum("jkn,nc->jkc", W, y[:, :3])
    bar = (count_of(shared(name, kind)[2], len(tables)) + N_RAYS) * U * np.einsum("jkn,nc->jkc", W, np.abs(y[:, :3]))   # (and the sum over the rays)
    assert (np.abs(adj["grad"][:, :, :3] - want) <= bar).all() and (np.abs(want) > 1e-3).mean() > 0.5


@pytest.mark.parametrize("name,kind", [("single", "los"), ("nest8", "los")])
def test_more_absorption_never_brightens(name, kind):
    """With y >= 0 every sigma entry of the adjoint is <= 0: w' <= 0, B >= 0, T >= 0."""
    c, tables, geo, _, y, _, _ = shared(name, kind)
    adj = jt.adjoint(c, tables, np.abs(y), STEPS, geo)
    assert (adj["G"][:, :, 3] <= 0.0).all() and (adj["grad"][:, :, 3] < 0.0).any()
    assert (adj["abs_L"] >= adj["abs"][:, :, 3] * (1 - 1e-12)).all()   # B <= L
