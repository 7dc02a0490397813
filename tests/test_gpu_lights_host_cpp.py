"""examples/soft_shadows: a plastic ring over a matte one seen by the pinhole camera through the plain C ABI, once under the
reference's hard light and once under that light with a radius plus a coloured fill light — the printed scanline (nine
significant digits: every bit of a float) against Tracer.shade_lit_camera on the same scene, camera, lights and disc
table, rebuilt here value for value, bit for bit; and the hard frame against Tracer.shade_camera with that light in pc."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

W, H = 48, 36
f32 = np.float32


def test_soft_shadows_example():
    exe = os.path.join(ROOT, "examples", "soft_shadows")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    head = re.search(r"soft shadows, pinhole (\d+)x(\d+), scanline (\d+)", p.stdout)
    assert head and [int(v) for v in head.groups()] == [W, H, H // 2], p.stdout
    num = r"([-+.\deE]+)"
    rows = re.findall(r"pixel +(\d+): hard %s %s %s  soft %s %s %s" % ((num,) * 6), p.stdout)
    assert [int(r[0]) for r in rows] == list(range(W)), p.stdout
    got = np.array([[f32(v) for v in r[1:]] for r in rows], f32)

    from toroidal_ray_tracing_amd.tracer import Tracer
    sc = abi.Scene([((0.0, 0.875, 0.0), 0.6, 0.15, 0), ((0.0, 0.0, 0.0), 1.6, 0.45, 1)], [camera.PLASTIC, camera.MATTE])
    pc = abi.make_push(clear=(0.1, 0.2, 0.4, 1.0), light_pos=(0.0, 0.0, 0.0), light_intensity=0.0, light_type=0, max_depth=1)
    g = abi.trt_globals()
    g.viewProj[0] = g.viewProj[5] = g.viewProj[10] = g.viewProj[15] = 1.0
    g.projInverse[0], g.projInverse[5], g.projInverse[10], g.projInverse[15] = 0.6, 0.45, 1.0, 1.0
    g.viewInverse[0] = 1.0
    g.viewInverse[5], g.viewInverse[6] = 0.8, 0.6
    g.viewInverse[9], g.viewInverse[10] = -0.6, 0.8
    g.viewInverse[12], g.viewInverse[13], g.viewInverse[14], g.viewInverse[15] = 0.0, 3.0, -4.0, 1.0
    fill = abi.make_light((-1.0, 0.5, -1.0), 0.125, (0.5, 0.625, 1.0), type=1)
    disc = [[0.25, 0.0], [-0.25, 0.0], [0.0, 0.625], [0.0, -0.625], [0.625, 0.625], [-0.625, 0.625], [0.625, -0.625], [-0.625, -0.625]]
    with Tracer(0) as tr:
        hard = tr.shade_lit_camera(sc, g, pc, W, H, lights=[abi.make_light((10.0, 15.0, 8.0), 100.0)])
        soft = tr.shade_lit_camera(sc, g, pc, W, H, lights=[abi.make_light((10.0, 15.0, 8.0), 100.0, radius=2.5), fill], shadow_samples=8, disc=disc)
        area = tr.shade_lit_camera(sc, g, pc, W, H, lights=[abi.make_light((10.0, 15.0, 8.0), 100.0, radius=2.5)], shadow_samples=8, disc=disc)
        ref = tr.shade_camera(sc, g, abi.make_push(clear=(0.1, 0.2, 0.4, 1.0), light_pos=(10.0, 15.0, 8.0), max_depth=1), W, H)
    want = np.concatenate([hard[H // 2, :, :3], soft[H // 2, :, :3]], 1)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(hard.view(np.uint32), ref.view(np.uint32))         # one hard white light: trt_shade_camera's frame
    miss = f32([0.1, 0.2, 0.4]) * f32(0.8)
    sees = np.abs(got[:, :3] - miss).max(1) > 1e-6
    assert 4 <= sees.sum() <= W - 2                                           # the scanline holds hits and misses
    assert (np.abs(got[sees, :3] - got[sees, 3:]).max(1) > 1e-3).mean() > 0.9   # the fill light is on every surface it faces
    assert np.array_equal(got[~sees, :3].view(np.uint32), got[~sees, 3:].view(np.uint32))   # ... and a miss is a miss
    assert int((area.view(np.uint32) != hard.view(np.uint32)).any(axis=2).sum()) >= 8   # terminator and penumbra are in the frame
