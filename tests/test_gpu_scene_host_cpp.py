"""examples/scene_mix: a checker-textured plastic ring under a soft key light and a coloured fill light, seen through a
glass ring, by the pinhole camera through the C++ host mirror (HelloHip::setTextures / raytraceScene) — the printed
scanline, once with glass casting its opaque shadow and once with TRT_SCENE_GLASS_SHADOWS (nine significant digits: every
bit of a float), against Tracer.shade_scene_camera on the same scene, texture, lights, disc table and camera, rebuilt here
value for value, bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

W, H, ROW = 48, 36, 15
f32 = np.float32


def test_scene_mix_example():
    exe = os.path.join(ROOT, "examples", "scene_mix")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    head = re.search(r"scene mix, pinhole (\d+)x(\d+), scanline (\d+)", p.stdout)
    assert head and [int(v) for v in head.groups()] == [W, H, ROW], p.stdout
    num = r"([-+.\deE]+)"
    rows = re.findall(r"pixel +(\d+): opaque %s %s %s  through %s %s %s" % ((num,) * 6), p.stdout)
    assert [int(r[0]) for r in rows] == list(range(W)), p.stdout
    got = np.array([[f32(v) for v in r[1:]] for r in rows], f32)

    from toroidal_ray_tracing_amd.tracer import Tracer
    plastic = dict(camera.PLASTIC, diffuse=(0.75, 0.75, 0.75), textureId=0)
    glass = dict(ambient=(0.0, 0.0, 0.0), diffuse=(0.05, 0.05, 0.05), specular=(0.5, 0.5, 0.5), shininess=64.0, illum=7, ior=1.5,
                 transmittance=(0.95, 0.8, 0.6))
    sc = abi.Scene([((0.0, 0.0, 0.0), 1.0, 0.35, 0), ((0.0, 0.75, 0.0), 1.0, 0.125, 1)], [plastic, glass])
    pc = abi.make_push(clear=(0.1, 0.2, 0.4, 1.0), max_depth=6)
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
    lights = [abi.make_light((0.5, 6.0, -0.5), 40.0, (1.0, 1.0, 1.0), 0, 0.5), abi.make_light((-4.0, 2.0, -3.0), 10.0, (0.25, 0.5, 1.0), 0, 0.0)]
    disc = f32([[0.25, 0.0], [-0.25, 0.0], [0.0, 0.25], [0.0, -0.25], [0.625, 0.625], [-0.625, 0.625], [0.625, -0.625], [-0.625, -0.625]])
    with Tracer(0) as tr:
        tr.set_textures([abi.make_texture(img, (4, 2), abi.TRT_TEX_LINEAR)])
        kw = dict(lights=lights, shadow_samples=8, disc=disc)
        opaque = tr.shade_scene_camera(sc, g, pc, W, H, glass_shadows=False, **kw)
        through = tr.shade_scene_camera(sc, g, pc, W, H, glass_shadows=True, **kw)
    want = np.concatenate([opaque[ROW, :, :3], through[ROW, :, :3]], 1)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), np.abs(got - want).max()
    miss = f32([0.1, 0.2, 0.4]) * f32(0.8)
    sees = np.abs(got[:, :3] - miss).max(1) > 1e-6
    assert 4 <= sees.sum() <= W - 2                                           # the scanline holds hits and misses
    differ = (np.ascontiguousarray(got[:, :3]).view(np.uint32) != np.ascontiguousarray(got[:, 3:]).view(np.uint32)).any(axis=1)
    assert differ.sum() >= 8                                                  # light through the glass ring is in the scanline
    assert (got[differ, 3:] >= got[differ, :3] - 1e-6).all()                  # and only ever adds light
