"""examples/ambient_occlusion: a small frame rendered with its first-hit record on the device, trt_fan_occluded_dev on that
record as it stands (K = 16 cosine-distributed directions about the normal, tmax = 0.5) — the printed counts against the
same query through the Python binding."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu


def example_table(K):
    """The fixed table of the example: radius sqrt(u_s), angle 2 pi v_s on the disc, u_s = (s + 1/2) / K, v_s = frac(s * 0.618…),
    lifted onto the hemisphere; doubles, rounded once."""
    s = np.arange(K, dtype=np.float64)
    u, v = (s + 0.5) / K, np.fmod(s * 0.6180339887498949, 1.0)
    r, phi = np.sqrt(u), 6.283185307179586 * v
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u)], 1).astype(np.float32)


def test_ambient_occlusion_example():
    exe = os.path.join(ROOT, "examples", "ambient_occlusion")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    W, H, K = 96, 64, 16
    p = subprocess.run([exe, str(W), str(H), str(K)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"96x64: (\d+) hit pixels, (\d+) fully open, mean open ([0-9.]+)", p.stdout)
    assert m, p.stdout
    hits, fully, mean = int(m.group(1)), int(m.group(2)), float(m.group(3))
    assert 0 < fully < hits < W * H and 0.5 < mean < 1.0
    # the same through the Python binding: the scene and camera of the example (those of examples/light_visibility)
    from toroidal_ray_tracing_amd.tracer import Tracer
    sc = abi.Scene([((0.0, 0.0, 0.0), 1.0, 0.25, 0), ((0.6, 0.9, 0.5), 0.5, 0.1, 0)], [dict(camera.PLASTIC, ambient=(0, 0, 0), specular=(0, 0, 0))])
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(1)
    with Tracer(0) as tr:
        _, first = tr.render(sc, g, pc, W, H)
        bits, opn = tr.fan_occluded(sc, first, example_table(K), tmin=0.001, tmax=0.5)
    hit = first["id"] >= 0
    assert not bits[~hit].any() and (opn[~hit] == 1.0).all()
    print(f"example: {hits} hit, {fully} fully open, mean {mean:.6f}; binding: {int(hit.sum())} hit, "
          f"{int((opn[hit] == 1.0).sum())} fully open, mean {float(opn[hit].mean()):.6f}")
    # The silhouette allowance of test_gpu_occluded_host_cpp.py: the camera matrices of the example are built in float,
    # those of camera.py in double, so a pixel on a silhouette may be hit in one frame and missed in the other — 2 % of the
    # hit pixels there, 3 % for a count derived from them.  A pixel that differs moves the sum of open by at most 1, so the
    # mean over the hit pixels moves by at most that share: 0.03.
    assert abs(int(hit.sum()) - hits) <= 0.02 * hits
    assert abs(int((opn[hit] == 1.0).sum()) - fully) <= 0.03 * hits
    assert abs(float(opn[hit].mean()) - mean) <= 0.03
