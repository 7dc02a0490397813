"""examples/see_through: the nest of eight shells with its outer four at dissolve 0.25, the pinhole camera's rays from
trt_camera_rays through trt_shade and trt_shade_through on host buffers — the printed scanline against the Python calls
on the same scene and camera, rebuilt here value for value."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

W, H = 32, 24
COLOR_RTOL, COLOR_ATOL = 1e-5, 1e-6


def test_see_through_example():
    exe = os.path.join(ROOT, "examples", "see_through")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    head = re.search(r"nest of 8, outer shells at dissolve 0.25, (\d+)x(\d+), scanline (\d+)", p.stdout)
    assert head and [int(v) for v in head.groups()] == [W, H, H // 2], p.stdout
    num = r"([-+.\deE]+)"
    rows = re.findall(r"pixel +(\d+): opaque %s %s %s  through %s %s %s" % ((num,) * 6), p.stdout)
    assert [int(r[0]) for r in rows] == list(range(W)), p.stdout
    got = np.array([[float(v) for v in r[1:]] for r in rows])

    from toroidal_ray_tracing_amd.tracer import Tracer
    tori = [((0.0, 0.0, 0.0), 1.0, float(np.float32(0.05) * np.float32(i + 1)), 0 if i < 4 else 1) for i in range(8)]
    sc = abi.Scene(tori, [dict(camera.PLASTIC, dissolve=1.0), dict(camera.MIRROR, dissolve=0.25)])
    pc = abi.make_push(clear=(0.1, 0.2, 0.4, 1.0), light_pos=(10.0, 15.0, 8.0), light_intensity=100.0, light_type=0, max_depth=5)
    g = abi.trt_globals()
    g.viewProj[0] = g.viewProj[5] = g.viewProj[10] = g.viewProj[15] = 1.0
    g.projInverse[0], g.projInverse[5], g.projInverse[10], g.projInverse[15] = 0.6, 0.45, 1.0, 1.0
    g.viewInverse[0] = 1.0
    g.viewInverse[5], g.viewInverse[6] = 0.8, 0.6
    g.viewInverse[9], g.viewInverse[10] = -0.6, 0.8
    g.viewInverse[12], g.viewInverse[13], g.viewInverse[14], g.viewInverse[15] = 0.0, 3.0, -4.0, 1.0
    with Tracer(0) as tr:
        o, d = tr.camera_rays(g, pc, W, H)
        opaque = tr.shade(sc, o, d, pc)
        through = tr.shade_through(sc, o, d, pc)
    line = slice((H // 2) * W, (H // 2 + 1) * W)
    want = np.concatenate([opaque[line, :3], through[line, :3]], 1).astype(np.float64)
    np.testing.assert_allclose(got, want, rtol=COLOR_RTOL, atol=COLOR_ATOL)
    miss = (np.float32([0.1, 0.2, 0.4]) * np.float32(0.8)).astype(np.float64)
    hit = np.abs(got[:, :3] - miss).max(1) > 1e-6
    assert 4 <= hit.sum() <= W - 2                                            # the scanline holds hits and misses
    assert (np.abs(got[hit, :3] - got[hit, 3:]).max(1) > 1e-3).mean() > 0.9   # looking through changes the pixels that see the nest
    assert (np.abs(got[~hit, :3] - got[~hit, 3:]).max(1) <= 1e-6).all()       # ... and no other
