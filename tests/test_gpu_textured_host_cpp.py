"""examples/textured_ring: a checker-textured plastic ring beside a mirror ring that reflects it, seen by the pinhole camera
through the C++ host mirror (HelloHip::setTextures / raytraceTextured) — the printed scanline (nine significant digits:
every bit of a float) against Tracer.shade_textured_camera on the same scene, axes, texture, camera and offsets, rebuilt
here value for value, bit for bit."""
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


def test_textured_ring_example():
    exe = os.path.join(ROOT, "examples", "textured_ring")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    head = re.search(r"textured ring, pinhole (\d+)x(\d+), scanline (\d+)", p.stdout)
    assert head and [int(v) for v in head.groups()] == [W, H, H // 2], p.stdout
    num = r"([-+.\deE]+)"
    rows = re.findall(r"pixel +(\d+): one %s %s %s  four %s %s %s" % ((num,) * 6), p.stdout)
    assert [int(r[0]) for r in rows] == list(range(W)), p.stdout
    got = np.array([[f32(v) for v in r[1:]] for r in rows], f32)

    from toroidal_ray_tracing_amd.tracer import Tracer
    plastic = dict(camera.PLASTIC, diffuse=(0.75, 0.75, 0.75), textureId=0)
    tori = [((-0.75, 0.0, 0.0), 1.0, 0.35, 0), ((1.25, 0.25, 0.0), 0.75, 0.25, 1)]
    sc = abi.Scene(tori, [plastic, camera.MIRROR], axes=[(0.0, 1.0, 0.0), (1.0, 0.0, 0.0)])
    bare = abi.Scene(tori, [dict(plastic, textureId=-1), camera.MIRROR], axes=[(0.0, 1.0, 0.0), (1.0, 0.0, 0.0)])
    pc = abi.make_push(clear=(0.1, 0.2, 0.4, 1.0), max_depth=4)        # the light of PushConstantRaster: (10, 15, 8), 100, a point
    g = abi.trt_globals()
    g.viewProj[0] = g.viewProj[5] = g.viewProj[10] = g.viewProj[15] = 1.0
    g.projInverse[0], g.projInverse[5], g.projInverse[10], g.projInverse[15] = 0.6, 0.45, 1.0, 1.0
    g.viewInverse[0] = 1.0
    g.viewInverse[5], g.viewInverse[6] = 0.8, 0.6
    g.viewInverse[9], g.viewInverse[10] = -0.6, 0.8
    g.viewInverse[12], g.viewInverse[13], g.viewInverse[14], g.viewInverse[15] = 0.0, 3.0, -4.0, 1.0
    yy, xx = np.mgrid[0:4, 0:8]
    light = ((xx + yy) % 2 == 0)[:, :, None]
    img = np.where(light, np.uint8([255, 240, 208, 255]), np.uint8([96, 112, 160, 255])).astype(np.uint8)
    grid = [[-0.25, -0.25], [0.25, -0.25], [-0.25, 0.25], [0.25, 0.25]]
    with Tracer(0) as tr:
        tr.set_textures([abi.make_texture(img, (4, 2), abi.TRT_TEX_LINEAR)])
        one = tr.shade_textured_camera(sc, g, pc, W, H)
        four = tr.shade_textured_camera(sc, g, pc, W, H, samples=4, offsets=grid)
        plain = tr.shade_camera(bare, g, pc, W, H)
    want = np.concatenate([one[H // 2, :, :3], four[H // 2, :, :3]], 1)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), np.abs(got - want).max()
    miss = f32([0.1, 0.2, 0.4]) * f32(0.8)
    sees = np.abs(got[:, :3] - miss).max(1) > 1e-6
    assert 4 <= sees.sum() <= W - 2                                           # the scanline holds hits and misses
    assert (np.abs(got[sees, :3] - got[sees, 3:]).max(1) > 1e-4).mean() > 0.5   # four samples filter the checker
    assert int((one.view(np.uint32) != plain.view(np.uint32)).any(axis=2).sum()) >= 50   # the checker is in the frame
