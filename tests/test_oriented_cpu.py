"""Tori on any axis, the part that needs no GPU: the new entry point is exported and bound, the FP64 helper the GPU
tests rely on (tests/oriented_truth.py) agrees with closed forms it shares nothing with, and the example builds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oriented_truth as ot
from conftest import ROOT
from toroidal_ray_tracing_amd import abi, camera, lib


def test_set_torus_axes_is_exported_and_bound():
    assert "trt_set_torus_axes" in lib.SYMBOLS
    L = lib.load()
    assert hasattr(L, "trt_set_torus_axes")
    axes = (C.c_float * 3)(0.0, 0.0, 1.0)
    assert L.trt_set_torus_axes(None, axes, 1) == abi.TRT_E_INVALID     # no ctx: refused without touching a device
    assert L.trt_set_torus_axes(None, None, 0) == abi.TRT_E_INVALID
    assert L.trt_version() == 3 and C.sizeof(abi.trt_torus) == 24 and C.sizeof(abi.trt_scene) == 32


def test_scene_helpers_carry_axes():
    assert camera.single_torus_scene().axes is None and camera.nested_tori_scene().axes is None
    sc = camera.single_torus_scene(axis=(1, 0, 0))
    assert sc.axes.shape == (1, 3) and sc.axes.dtype == np.float32
    rings = camera.linked_rings_scene()
    assert rings.n_tori == 8 and rings.axes.shape == (8, 3)
    # neighbours interlock without touching: each ring's circle crosses the neighbour's plane inside the hole,
    # farther than 2r from the neighbour's centre circle; axes perpendicular to the chain and to each other
    tori = rings.tori_list()
    for (c0, R0, r0, _), (c1, R1, r1, _), a0, a1 in zip(tori, tori[1:], rings.axes, rings.axes[1:]):
        gap = c1[0] - c0[0]
        assert abs(float(a0 @ a1)) < 1e-6 and a0[0] == 0 and a1[0] == 0
        assert abs(gap - R1) + r1 < R0 - r0 and abs(gap - R0) + r0 < R1 - r1
    with pytest.raises(ValueError):
        abi.Scene([((0, 0, 0), 1.0, 0.25, 0)], [camera.MIRROR], axes=[(0, 1, 0), (1, 0, 0)])


def test_frame_is_a_rotation_that_maps_the_axis_to_y():
    rng = np.random.default_rng(5)
    for axis in [(1, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 3, 0), (1, 1, 1)] + list(rng.normal(size=(20, 3))):
        M = ot.frame(axis)
        assert np.allclose(M @ M.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(M) - 1) < 1e-14
        assert np.allclose(M @ ot.unit(axis), (0, 1, 0), atol=1e-14)


@pytest.mark.parametrize("shape", [(1.0, 0.05), (1.0, 0.25), (2.0, 0.9)], ids=["r/R=0.05", "r/R=0.25", "r/R=0.45"])
@pytest.mark.parametrize("family", ["equatorial", "meridional", "axial"])
def test_helper_matches_closed_forms_under_random_rotations(family, shape):
    """first_hit (companion-matrix roots in the torus' frame) against the closed-form families carried out of the +y
    frame by a random rotation, in float64 throughout: 1e-9 relative on the rays the family calls robust; the normals
    agree too.  The helper's frame of the rotated axis is not the rotation the rays were carried by — only the axis is
    shared — so this also checks that the choice of frame does not matter."""
    R, r = shape
    rng = np.random.default_rng(11)
    for k, Cc in enumerate([(0.0, 0.0, 0.0), (3.0, -2.0, 5.0), (-0.75, 1.5, 0.25)]):
        Q = ot.random_rotation(rng)
        o, d, t, N, ok, axis = ot.rotated_family(family, 20_000, 100 + k, Cc, Q, R, r)
        got, gid = ot.first_hit(o, d, [(Cc, axis, R, r)])
        hit_t, hit_g = np.isfinite(t), ~np.isnan(got)
        assert not np.any((hit_t != hit_g) & ok)
        both = hit_t & hit_g & ok
        assert both.sum() > 1000
        rel = np.abs(got[both] - t[both]) / np.maximum(1.0, t[both])
        assert rel.max() < 1e-9, rel.max()
        P = o[both] + got[both, None] * d[both]
        Ng = ot.normal(P, Cc, axis, R)
        assert np.abs(np.linalg.norm(Ng, axis=1) - 1).max() < 1e-12
        assert np.abs(Ng - N[both]).max() < 1e-7 * max(1.0, R / r)


def test_margin_of_one_torus_is_truths_margin_in_the_frame():
    o, d = ot.aimed_rays(5000, 3, (1.0, 2.0, -3.0), 1.0, 0.25)
    tori = [((1.0, 2.0, -3.0), (0.3, -0.5, 0.8), 1.0, 0.25)]
    ok = ot.classify_margin(o, d, tori)
    assert 0.98 < ok.mean() <= 1.0
    # two copies of one torus: the general rule over first_hit() gives the same flags as truth's own rule
    assert np.array_equal(ok, ot.classify_margin(o, d, tori + [((50.0, 0.0, 0.0), (0, 1, 0), 1.0, 0.25)]))


def test_example_and_host_library_compile_and_link(tmp_path):
    """examples/linked_rings_main.cpp against the host mirror and libtrt.so (built here into a scratch directory)."""
    pkg = os.path.join(ROOT, "toroidal_ray_tracing_amd")
    assert os.path.exists(os.path.join(pkg, "libtrt.so"))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    host = str(tmp_path / "libhello_hip.so")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-fPIC", "-shared", "-o", host, os.path.join(pkg, "host", "hello_hip.cpp"),
                    "-L" + pkg, "-ltrt"], check=True)
    exe = str(tmp_path / "linked_rings")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "examples", "linked_rings_main.cpp"),
                    "-L" + str(tmp_path), "-lhello_hip", "-L" + pkg, "-ltrt"], check=True)
    syms = subprocess.run(["nm", "-D", "--undefined-only", host], capture_output=True, text=True, check=True).stdout
    assert "trt_set_torus_axes" in syms
    assert "setTorusAxes" in subprocess.run(["nm", "-D", "-C", "--undefined-only", exe], capture_output=True, text=True, check=True).stdout
