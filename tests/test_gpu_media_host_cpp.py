"""examples/plasma_glow: three nested shells as three media, the pinhole camera's rays from trt_camera_rays through
trt_chords and trt_glow on host buffers, then bounded by trt_trace's t of a ring in front — the printed numbers against
the Python calls on the same scenes and camera, rebuilt here value for value."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

W, H = 32, 24
COLOR_RTOL = 1e-5


def test_plasma_glow_example():
    exe = os.path.join(ROOT, "examples", "plasma_glow")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    head = re.search(r"plasma glow, 3 shells, (\d+)x(\d+)", p.stdout)
    assert head and [int(v) for v in head.groups()] == [W, H], p.stdout
    num = r"([-+.\deE]+)"
    shells = re.findall(r"shell (\d): mean chord %s" % num, p.stdout)
    assert [int(s[0]) for s in shells] == [0, 1, 2], p.stdout
    got_mean = np.array([float(s[1]) for s in shells])
    got_open = float(re.search(r"image: checksum %s" % num, p.stdout).group(1))
    behind = re.search(r"behind the ring: (\d+) pixels hidden, checksum %s" % num, p.stdout)
    got_hidden, got_cut = int(behind.group(1)), float(behind.group(2))

    from toroidal_ray_tracing_amd.tracer import Tracer
    sc = abi.Scene([((0.0, 0.0, 0.0), 1.0, r, 0) for r in (0.15, 0.25, 0.35)], [camera.PLASTIC])
    front = abi.Scene([((0.0, 1.5, -2.0), 0.5, 0.1, 0)], [camera.PLASTIC])
    media = [((2.0, 0.5, 0.25), 0.0), ((0.25, 0.5, 1.0), 0.5), ((0.0, 0.125, 0.25), 1.0)]
    clear = np.float32([0.1, 0.2, 0.4])
    pc = abi.make_push()
    g = abi.trt_globals()
    g.viewProj[0] = g.viewProj[5] = g.viewProj[10] = g.viewProj[15] = 1.0
    g.projInverse[0], g.projInverse[5], g.projInverse[10], g.projInverse[15] = 0.6, 0.45, 1.0, 1.0
    g.viewInverse[0] = 1.0
    g.viewInverse[5], g.viewInverse[6] = 0.8, 0.6
    g.viewInverse[9], g.viewInverse[10] = -0.6, 0.8
    g.viewInverse[12], g.viewInverse[13], g.viewInverse[14], g.viewInverse[15] = 0.0, 3.0, -4.0, 1.0
    with Tracer(0) as tr:
        o, d = tr.camera_rays(g, pc, W, H)
        length = tr.chords(sc, o, d)
        glow = tr.glow(sc, o, d, media)
        t = tr.trace(front, o, d)["t"]
        cut = tr.glow(sc, o, d, media, tmax_per_ray=t)
    ringed = np.isfinite(t)
    want_open = (glow[:, :3] + glow[:, 3:] * clear[None, :]).astype(np.float64).sum()
    want_cut = (cut[:, :3].astype(np.float64) + np.where(ringed[:, None], np.float32(0), cut[:, 3:] * clear[None, :])).sum()
    np.testing.assert_allclose(got_mean, length.astype(np.float64).mean(1), rtol=COLOR_RTOL)
    np.testing.assert_allclose([got_open, got_cut], [want_open, want_cut], rtol=COLOR_RTOL)
    assert got_hidden == ringed.sum() and 4 <= got_hidden <= W * H // 2      # the ring hides some pixels, not most
    assert (got_mean > 0.01).all() and got_mean[0] < got_mean[1] < got_mean[2]   # wider shells, longer chords
    assert got_cut < got_open                                                 # black behind the ring, and less glow in front of it
