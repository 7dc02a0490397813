"""Capture -> point cloud, the part that needs no GPU: trt_cloud_dev is exported and bound, and the numpy restatement the
GPU tests compare against (tests/cloud_truth.py) does what include/trt.h says on a capture written out by hand."""
import ctypes as C

import numpy as np

import cloud_truth as ct
from toroidal_ray_tracing_amd import abi, lib


def test_cloud_dev_is_exported_and_bound():
    assert "trt_cloud_dev" in lib.SYMBOLS
    L = lib.load()
    assert hasattr(L, "trt_cloud_dev")
    counts = (C.c_uint64 * 2)(7, 9)
    # no ctx: refused without touching a device or the counts
    assert L.trt_cloud_dev(None, None, 0, abi.TRT_CLOUD_COMPACT, 0, None, 0, counts, None) == abi.TRT_E_INVALID
    assert list(counts) == [7, 9]
    assert (abi.TRT_CLOUD_KEEP_ALL, abi.TRT_CLOUD_MARK_MISSES, abi.TRT_CLOUD_COMPACT) == (0, 1, 2)
    assert (ct.KEEP_ALL, ct.MARK_MISSES, ct.COMPACT) == (0, 1, 2)


def test_version_is_still_3():
    assert lib.load().trt_version() == 3


F = np.float32
LOW = F(-3.4028234663852886e38)
NAN, NNAN = F(np.nan), np.uint32(0xFFC00001).view(np.float32)   # a quiet NaN of each sign (the second with a payload)


def _capture():
    """Eight records: hit, miss, -0.0 miss, NaN position, NaN colour, hit with one zero component, hit with two zero
    components and a -0.0, miss whose colour is not the clear colour.  pos.w = 1 everywhere, as the kernels write it."""
    r = np.zeros((8, 16), np.float32)
    r[:, 3] = 1.0
    r[:, 7] = 1.0
    r[:, 8:16] = np.arange(64, dtype=np.float32).reshape(8, 8) + 0.5     # the ray half: never read
    r[0, 0:3], r[0, 4:7] = (1.0, 2.0, 3.0), (0.1, 0.2, 0.3)
    r[1, 0:3], r[1, 4:7] = (0.0, 0.0, 0.0), (0.8, 0.8, 0.8)
    r[2, 0:3], r[2, 4:7] = (-0.0, 0.0, -0.0), (0.8, 0.8, 0.8)
    r[3, 0:3], r[3, 4:7] = (NAN, 0.0, 0.0), (0.4, 0.5, 0.6)
    r[4, 0:3], r[4, 4:7] = (4.0, 5.0, 6.0), (0.7, NNAN, 0.9)
    r[5, 0:3], r[5, 4:7] = (7.0, 0.0, 8.0), (0.25, 0.5, 0.75)
    r[6, 0:3], r[6, 4:7] = (0.0, -0.0, 1e-45), (1.0, 1.0, 1.0)          # a denormal is not zero
    r[7, 0:3], r[7, 4:7] = (0.0, 0.0, 0.0), (0.3, 0.2, 0.1)
    return r


def _pt(pos, col):
    return np.array([*pos, 0.0, *col, 0.0], np.float32).view(np.uint32)


def test_truth_on_a_hand_written_capture():
    r = _capture()
    assert ct.is_miss(r).tolist() == [False, True, True, False, False, False, False, True]
    keep = ct.points_of(r, ct.KEEP_ALL)
    want = np.stack([
        _pt((1.0, 2.0, 3.0), (0.1, 0.2, 0.3)),
        _pt((0.0, 0.0, 0.0), (0.8, 0.8, 0.8)),
        _pt((-0.0, 0.0, -0.0), (0.8, 0.8, 0.8)),          # bit for bit: the sign of zero stays
        _pt((LOW, 0.0, 0.0), (0.4, 0.5, 0.6)),            # NaN -> lowest(), the record is not a miss
        _pt((4.0, 5.0, 6.0), (0.7, LOW, 0.9)),            # either sign of NaN, in the colour too
        _pt((7.0, 0.0, 8.0), (0.25, 0.5, 0.75)),
        _pt((0.0, -0.0, 1e-45), (1.0, 1.0, 1.0)),
        _pt((0.0, 0.0, 0.0), (0.3, 0.2, 0.1)),
    ])
    assert keep.dtype == np.uint32 and np.array_equal(keep, want)
    mark = ct.points_of(r, ct.MARK_MISSES)
    for i in (1, 2, 7):
        want[i, 0:3] = ct.LOWEST                           # the colour of a marked miss stays
    assert np.array_equal(mark, want)
    comp = ct.points_of(r, ct.COMPACT)
    assert np.array_equal(comp, want[[0, 3, 4, 5, 6]])     # relative order kept


def test_truth_append_and_capacity():
    r = _capture()
    poison = np.full((6, 8), 0xDEADBEEF, np.uint32)
    pts, counts = ct.cloud(r, ct.COMPACT, poison)
    assert counts == (5, 5) and np.array_equal(pts[:5], ct.points_of(r, ct.COMPACT)) and (pts[5] == 0xDEADBEEF).all()
    # appending the same capture: one more point fits, the counts tell that four did not
    pts2, counts2 = ct.cloud(r, ct.COMPACT, pts, counts, append=True)
    assert counts2 == (6, 10) and np.array_equal(pts2[:5], pts[:5]) and np.array_equal(pts2[5], pts[0])
    # a full buffer takes nothing more; without append the counts restart
    pts3, counts3 = ct.cloud(r, ct.KEEP_ALL, pts2, counts2, append=True)
    assert counts3 == (6, 18) and np.array_equal(pts3, pts2)
    pts4, counts4 = ct.cloud(r[:2], ct.MARK_MISSES, pts3, counts3)
    assert counts4 == (2, 2) and np.array_equal(pts4[:2], ct.points_of(r[:2], ct.MARK_MISSES)) and np.array_equal(pts4[2:], pts3[2:])
    # no records: only the counts move
    assert ct.cloud(r[:0], ct.COMPACT, pts4, counts4, append=True)[1] == (2, 2)
    assert ct.cloud(r[:0], ct.COMPACT, pts4, counts4)[1] == (0, 0)
    assert (poison == 0xDEADBEEF).all()   # the buffer passed in is not written
