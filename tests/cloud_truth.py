"""Capture -> point cloud in numpy — TEST INFRASTRUCTURE (a helper module: no tests, no fixtures).

A restatement of what include/trt.h says trt_cloud_dev does, sharing nothing with the kernels: the per-record rule, the
miss rule, the three modes, append and capacity.  Everything is done on uint32 views, so "copied bit for bit" is literal
(numpy float copies would do the same, but a view cannot even quieten a signalling NaN on the way).
"""
import numpy as np

KEEP_ALL, MARK_MISSES, COMPACT = 0, 1, 2
LOWEST = np.float32(-3.4028234663852886e38).view(np.uint32)   # -FLT_MAX, numeric_limits<float>::lowest(): 0xff7fffff
assert int(LOWEST) == 0xFF7FFFFF


def records(a):
    """(n, 16) float32 view of a capture: pos[4], color[4], rayOrigin[4], rayDir[4] per record."""
    a = np.ascontiguousarray(a)
    return a.view(np.float32).reshape(-1, 16)


def is_miss(rec):
    """True where pos[0], pos[1] and pos[2] all compare equal to 0.0f (-0.0 == 0.0; a NaN equals nothing)."""
    rec = records(rec)
    return (rec[:, 0] == 0) & (rec[:, 1] == 0) & (rec[:, 2] == 0)


def points_of(rec, mode):
    """The points of the records, one per record in KEEP_ALL and MARK_MISSES, the non-misses in COMPACT: (m, 8) uint32."""
    rec = records(rec)
    bits = rec.view(np.uint32)
    out = np.zeros((len(rec), 8), np.uint32)        # both .w = 0
    out[:, 0:3] = bits[:, 0:3]
    out[:, 4:7] = bits[:, 4:7]
    nan = np.zeros((len(rec), 8), bool)
    nan[:, 0:3] = np.isnan(rec[:, 0:3])
    nan[:, 4:7] = np.isnan(rec[:, 4:7])
    out[nan] = LOWEST
    miss = is_miss(rec)
    if mode == MARK_MISSES:
        out[miss, 0:3] = LOWEST
    elif mode == COMPACT:
        out = out[~miss]
    else:
        assert mode == KEEP_ALL
    return out


def cloud(rec, mode, points, counts=(0, 0), append=False):
    """One call: ``points`` ((capacity, 8) uint32, what the buffer held) and ``counts`` (what counts_dev held) in,
    (points after the call, (counts[0], counts[1]) after the call) out.  Nothing at or beyond the capacity is written."""
    points = np.array(points, np.uint32, copy=True).reshape(-1, 8)
    capacity = len(points)
    new = points_of(rec, mode)
    start = int(counts[0]) if append else 0
    wanted_before = int(counts[1]) if append else 0
    fits = max(0, min(len(new), capacity - start))
    if fits:
        points[start:start + fits] = new[:fits]
    return points, (min(start + len(new), capacity), wanted_before + len(new))
