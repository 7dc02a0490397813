"""examples/capture_reproject: the rho sweep of toroidal_sweep and the re-projection of reproject in one program, the
captures appended into one compacted cloud on the device (HelloHip::createCloudDataBufferFromCapture) with no file in
between — its printed count against cloud_truth on the same captures from the oracle."""
import os
import re
import subprocess

import pytest

import cloud_truth as ct
from conftest import ROOT
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu


def test_capture_reproject_example(tmp_path, oracle):
    exe = os.path.join(ROOT, "examples", "capture_reproject")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    cw, ch, W, H = 96, 40, 128, 96                       # not square: the device path pairs nothing by line number
    ppm = tmp_path / "cloud.ppm"
    p = subprocess.run([exe, str(cw), str(ch), str(W), str(H), str(ppm)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) captures of 96x40: (\d+) records, (\d+) points kept \((\d+) wanted\), (\d+) misses dropped", p.stdout)
    assert m, p.stdout
    captures, records, kept, wanted, dropped = map(int, m.groups())
    # the same captures from the oracle: the scene and the sweep of examples/toroidal_sweep (BEF/main.cpp:236-258)
    sc = camera.single_torus_scene(R=14.0, r=3.0, material=camera.PLASTIC)
    g = camera.toroidal_camera(cw, ch)
    hits = 0
    rhos = [4.5 + 0.5 * k for k in range(12)]
    for rho in rhos:
        pc = abi.make_push(max_depth=10, rho=rho)
        _, _, rendered, _ = oracle.render(sc, g, pc, cw, ch, abi.TRT_CAMERA_TOROIDAL, nthreads=4, want_hits=False, want_rendered=True)
        hits += int((~ct.is_miss(rendered)).sum())
    assert captures == len(rhos) and records == len(rhos) * cw * ch
    assert 0.1 * records < hits < 0.9 * records
    assert kept == wanted == hits and dropped == records - hits
    m = re.search(r"(\d+) points -> 128x96, (\d+) pixels covered", p.stdout)
    assert m and int(m.group(1)) == kept and 0 < int(m.group(2)) < W * H, p.stdout
    raw = ppm.read_bytes()
    assert raw.startswith(b"P6\n128 96\n255\n") and len(raw) == len(b"P6\n128 96\n255\n") + W * H * 3
