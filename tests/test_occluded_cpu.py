"""trt_occluded, the part that needs no GPU: both entry points are exported and bound, refuse a NULL ctx without a device,
and the mask layout of include/trt.h round-trips between abi.unpack_mask and the tests' own packer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import occlusion_truth as ot
from conftest import ROOT
from toroidal_ray_tracing_amd import abi, lib


def test_occluded_is_exported_and_bound():
    L = lib.load()
    for name in ("trt_occluded", "trt_occluded_dev"):
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert L.trt_version() == 3


def test_null_ctx_is_refused_without_a_device():
    L = lib.load()
    rays = abi.trt_rays()
    flag = (C.c_uint8 * 4)(7, 7, 7, 7)
    assert L.trt_occluded(None, C.byref(rays), None, None, 0.001, 1.0, flag, None) == abi.TRT_E_INVALID
    assert L.trt_occluded_dev(None, C.byref(rays), None, None, 0.001, 1.0, flag, None, None) == abi.TRT_E_INVALID
    assert list(flag) == [7, 7, 7, 7]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200])
def test_mask_layout_round_trips(n):
    rng = np.random.default_rng(n)
    f = rng.uniform(size=n) < 0.5
    if n:
        f[-1] = True   # the last ray's bit is the one next to the unused ones
    w = ot.pack_mask(f)
    assert w.dtype == np.uint64 and len(w) == (n + 63) // 64 == abi.mask_words(n) == ot.mask_words(n)
    for i in range(n):   # the layout, bit by bit, as include/trt.h states it
        assert bool((int(w[i >> 6]) >> (i & 63)) & 1) == bool(f[i]), i
    if n % 64:
        assert int(w[-1]) >> (n % 64) == 0   # the unused high bits are zero
    got = abi.unpack_mask(w, n)
    assert got.dtype == bool and got.shape == (n,) and np.array_equal(got, f)
    # words beyond the mask are ignored
    assert np.array_equal(abi.unpack_mask(np.concatenate([w, np.full(2, 0xFFFFFFFFFFFFFFFF, np.uint64)]), n), f)


def test_occluded_from_hits_is_id_at_least_zero():
    assert ot.occluded_from_hits({"id": np.int32([-1, 0, 3, -1])}).tolist() == [False, True, True, False]


def test_example_source_and_makefile_target_exist():
    assert os.path.exists(os.path.join(ROOT, "examples", "light_visibility_main.cpp"))
    mk = open(os.path.join(ROOT, "toroidal_ray_tracing_amd", "host", "Makefile")).read()
    all_rule = re.search(r"^all:(.*?)\n\n", mk, flags=re.S | re.M).group(1)
    assert "../../examples/light_visibility" in all_rule
    src = open(os.path.join(ROOT, "examples", "light_visibility_main.cpp")).read()
    assert "trt_occluded(" in src and "trt_render(" in src
