"""examples/light_visibility: a small frame rendered with first-hit records, one segment ray per hit pixel towards the point
light, trt_occluded on host buffers — the printed counts against the same query through the Python binding."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu


def test_light_visibility_example():
    exe = os.path.join(ROOT, "examples", "light_visibility")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    W, H = 96, 64
    p = subprocess.run([exe, str(W), str(H)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"96x64: (\d+) hit pixels, (\d+) lit, (\d+) in shadow", p.stdout)
    assert m, p.stdout
    hits, lit, shadow = map(int, m.groups())
    assert 0 < lit <= hits and lit + shadow == hits and hits < W * H
    # the same through the Python binding: the scene, camera and light of the example
    from toroidal_ray_tracing_amd.tracer import Tracer
    sc = abi.Scene([((0.0, 0.0, 0.0), 1.0, 0.25, 0), ((0.6, 0.9, 0.5), 0.5, 0.1, 0)], [dict(camera.PLASTIC, ambient=(0, 0, 0), specular=(0, 0, 0))])
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(1)
    with Tracer(0) as tr:
        _, first = tr.render(sc, g, pc, W, H)
        hit = first["id"] >= 0
        P = np.stack([first["px"], first["py"], first["pz"]], 1)[hit]
        L = np.float32(list(pc.lightPosition))
        occ = tr.occluded(sc, P, L - P, 0.001, 1.0)
    # (the camera matrices of the example are built in float, those of camera.py in double: a pixel on a silhouette
    # may differ, the counts agree closely)
    assert abs(int(hit.sum()) - hits) <= 0.02 * hits and abs(int((~occ).sum()) - lit) <= 0.03 * hits
    assert 0 < shadow
