"""trt_crossings, the part that needs no GPU: the tests' FP64 truth against closed forms, the ctypes mirror of
trt_crossing_streams against the header, both entry points exported, bound and refusing a NULL ctx without a device, and
the example wired into the host Makefile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import crossings_truth as ct
from conftest import ROOT
from toroidal_ray_tracing_amd import abi, lib

HEADER = os.path.join(ROOT, "include", "trt.h")


@pytest.mark.parametrize("R, r", [(1.0, 0.25), (1.0, 0.05), (2.0, 0.45)])
def test_truth_equatorial_ray_through_the_centre(R, r):
    """A ray in the equatorial plane through the centre crosses the tube at distance R ± r on either side: four
    crossings, alternating enter and leave."""
    C0 = (0.25, -0.5, 0.125)
    ang = np.linspace(0.1, 6.0, 7)
    d = np.stack([np.cos(ang), np.zeros_like(ang), np.sin(ang)], 1)
    o = np.asarray(C0) - 5.0 * d
    t, tid, en, cnt = ct.all_crossings(o, d, [(C0, R, r)])
    assert (cnt == 4).all() and (tid == 0).all()
    np.testing.assert_allclose(t, np.tile([5 - R - r, 5 - R + r, 5 + R - r, 5 + R + r], (len(o), 1)), rtol=0, atol=1e-9)
    assert (en == [True, False, True, False]).all()
    assert ct.classify_margin_all(o, d, [(C0, R, r)]).all()
    np.testing.assert_allclose(ct.chord_lengths(t, tid, en, 1)[:, 0], 4 * r, atol=1e-9)
    # the window is open and cuts the list; an origin inside the tube leaves first
    t2, _, en2, cnt2 = ct.all_crossings(o, d, [(C0, R, r)], tmin=5 - R, tmax=5 + R)
    assert (cnt2 == 2).all() and (en2[:, :2] == [False, True]).all() and np.isinf(t2[:, 2:]).all()


def test_truth_axial_and_oriented_rays():
    """Down the axis through the tube (two crossings at height ±r), through the hole (none); the same torus on a tilted
    axis, asked along that axis; two nested shells merge in order with their ids."""
    tori = [((0.0, 0.0, 0.0), 1.0, 0.25)]
    t, tid, en, cnt = ct.all_crossings([[1.0, 5.0, 0.0], [0.0, 5.0, 0.0]], [[0.0, -1.0, 0.0]] * 2, tori)
    assert cnt.tolist() == [2, 0]
    np.testing.assert_allclose(t[0, :2], [4.75, 5.25], atol=1e-9)
    assert en[0, :2].tolist() == [True, False] and tid[1].tolist() == [-1] * 4
    axis = np.array([0.3, 1.0, -0.4])
    a = axis / np.linalg.norm(axis)
    u = np.cross(a, [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)                      # a unit vector perpendicular to the axis: a point of the centre circle
    t, _, en, cnt = ct.all_crossings([u + 5.0 * a], [-a], tori, axes=[axis])
    assert cnt[0] == 2 and en[0, :2].tolist() == [True, False]
    np.testing.assert_allclose(t[0, :2], [4.75, 5.25], atol=1e-9)
    nest = [((0.0, 0.0, 0.0), 1.0, 0.35), ((0.0, 0.0, 0.0), 1.0, 0.15)]
    t, tid, en, cnt = ct.all_crossings([[1.0, 5.0, 0.0]], [[0.0, -1.0, 0.0]], nest)
    assert cnt[0] == 4 and tid[0, :4].tolist() == [0, 1, 1, 0] and en[0, :4].tolist() == [True, True, False, False]
    np.testing.assert_allclose(ct.chord_lengths(t, tid, en, 2)[0], [0.7, 0.3], atol=1e-9)


def test_recipe_leaves_few_rays_out():
    """The margin rule on the recipe's rays, by the truth alone: at most 0.5 % of a set is non-robust."""
    for name in ct.SCENES:
        s = ct.ray_set(name)
        assert s["o"].dtype == np.float32 and len(s["o"]) == ct.N_RAYS
        assert 1.0 - s["robust"].mean() <= 0.005, name
        assert (s["count"] % 2 == 0).all() and s["count"].max() >= 4


def test_abi_layout_matches_the_header():
    src = open(HEADER).read()
    body = re.search(r"typedef struct trt_crossing_streams \{(.*?)\} trt_crossing_streams;", src, flags=re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\*\s+(\w+);", body, flags=re.M)
    assert fields == [("float", "t"), ("int32_t", "id"), ("uint8_t", "entering"), ("uint32_t", "count")]
    assert [f[0] for f in abi.trt_crossing_streams._fields_] == [name for _, name in fields] == list(abi.CROSSING_FIELDS)
    assert all(f[1] is C.c_void_p for f in abi.trt_crossing_streams._fields_)
    assert C.sizeof(abi.trt_crossing_streams) == 4 * C.sizeof(C.c_void_p)
    assert [getattr(abi.trt_crossing_streams, name).offset for _, name in fields] == [0, 8, 16, 24]
    ctype = {"float": np.float32, "int32_t": np.int32, "uint8_t": np.uint8, "uint32_t": np.uint32}
    assert {name: ctype[c] for c, name in fields} == abi.CROSSING_DTYPES
    assert re.search(r"#define TRT_MAX_CROSSINGS \(4 \* TRT_MAX_TORI\)", src)
    assert abi.TRT_MAX_CROSSINGS == 4 * abi.TRT_MAX_TORI == 32
    out = abi.alloc_crossings(5, 3)
    assert out["t"].shape == out["id"].shape == out["entering"].shape == (3, 5) and out["count"].shape == (5,)
    cs = abi.crossing_streams_struct({"t": out["t"], "count": 1234})
    assert cs.t == out["t"].ctypes.data and cs.id is None and cs.entering is None and cs.count == 1234


def test_crossings_are_exported_and_refuse_a_null_ctx():
    L = lib.load()
    for name in ("trt_crossings", "trt_crossings_dev"):
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert L.trt_version() == 3
    rays = abi.trt_rays()
    count = np.full(4, 7, np.uint32)
    cs = abi.crossing_streams_struct({"count": count})
    assert L.trt_crossings(None, C.byref(rays), None, 0.001, 1.0, 4, C.byref(cs)) == abi.TRT_E_INVALID
    assert L.trt_crossings_dev(None, C.byref(rays), None, 0.001, 1.0, 4, C.byref(cs), None) == abi.TRT_E_INVALID
    assert count.tolist() == [7, 7, 7, 7]


def test_example_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "examples", "shell_chords_main.cpp")
    text = open(src).read()
    assert "trt_crossings(" in text and "entering" in text
    mk = open(os.path.join(ROOT, "toroidal_ray_tracing_amd", "host", "Makefile")).read()
    all_rule = re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    assert "../../examples/shell_chords" in all_rule and "../../examples/light_visibility" in all_rule
    pkg = os.path.join(ROOT, "toroidal_ray_tracing_amd")
    exe = str(tmp_path / "shell_chords")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", exe, src, "-L" + pkg, "-ltrt", "-Wl,-rpath," + pkg],
                       capture_output=True, text=True)
    assert p.returncode == 0 and os.path.exists(exe), p.stdout + p.stderr
