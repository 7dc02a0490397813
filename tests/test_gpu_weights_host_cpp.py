"""examples/emission_fit: one torus whose emission varies across the tube, "measured" by trt_glow_profile without
absorption and fitted back through trt_glow_weights and the 17 x 17 normal equations; the printed numbers against the
Python calls on the same scene, camera and table (tests/weights_truth.py rebuilds them value for value)."""
import os
import re
import subprocess

import numpy as np
import pytest

import weights_truth as wt
from conftest import ROOT
from test_weights_cpu import EXAMPLE_COND
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

COLOR_RTOL = 1e-5
K = abi.TRT_PROFILE_KNOTS


def test_emission_fit_example():
    exe = os.path.join(ROOT, "examples", "emission_fit")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    head = re.search(r"emission fit, 1 torus, (\d+)x(\d+), steps (\d+)", p.stdout)
    assert head and [int(v) for v in head.groups()] == [wt.EXAMPLE_W, wt.EXAMPLE_H, wt.EXAMPLE_STEPS], p.stdout
    num = r"([-+.\deE]+)"
    sums = re.search(r"column sums:((?: %s){%d})\n" % (num[1:-1], K), p.stdout)
    assert sums, p.stdout
    got_sums = np.array(sums.group(1).split(), np.float64)
    res = re.search(r"forward residual: largest %s, over chord \* largest knot %s" % (num, num), p.stdout)
    got_abs, got_rel = float(res.group(1)), float(res.group(2))
    knots = re.findall(r"knot +(\d+): red %s \(true %s\) blue %s \(true %s\)" % (num, num, num, num), p.stdout)
    assert [int(m[0]) for m in knots] == list(range(K)), p.stdout
    got_fit = np.array([[float(m[1]), float(m[3])] for m in knots])
    got_true = np.array([[float(m[2]), float(m[4])] for m in knots])

    from toroidal_ray_tracing_amd.tracer import Tracer
    sc = abi.Scene([(wt.EXAMPLE_GEO[0], wt.EXAMPLE_GEO[1], wt.EXAMPLE_GEO[2], 0)], [camera.PLASTIC])
    table = wt.example_table()
    with Tracer(0) as tr:
        o, d = tr.camera_rays(wt.example_globals(), abi.make_push(), wt.EXAMPLE_W, wt.EXAMPLE_H)
        length = tr.chords(sc, o, d)[0].astype(np.float64)
        L = tr.glow_profile(sc, o, d, [table], steps=wt.EXAMPLE_STEPS).astype(np.float64)
        W = tr.glow_weights(sc, o, d, steps=wt.EXAMPLE_STEPS)[0].astype(np.float64)
    assert (L[:, 3] == 1.0).all() and np.array_equal(got_true.astype(np.float32), table[:, [0, 2]])   # (nine digits give an FP32 back)
    np.testing.assert_allclose(got_sums, W.sum(1), rtol=COLOR_RTOL)
    # the forward identity, and its bar (tests/test_gpu_weights.py, 3.)
    err = np.abs(W.T @ table[:, :3].astype(np.float64) - L[:, :3])
    top = table[:, :3].astype(np.float64).max(0)
    hit = length > 0
    rel = (err[hit][:, [0, 2]] / (length[hit, None] * top[None, [0, 2]])).max()
    np.testing.assert_allclose([got_abs, got_rel], [err.max(), rel], rtol=COLOR_RTOL)
    assert got_rel <= (4 * wt.EXAMPLE_STEPS + 24) * 2.0 ** -24 and (err[~hit] == 0).all()
    # the recovered knots against Python's own solve of the same normal equations, at the condition number's tolerance
    want_fit = np.linalg.solve(wt.normal_matrix(W), W @ L[:, [0, 2]])
    print(f"recovered knots: largest difference from Python's solve {np.abs(got_fit - want_fit).max():.3e}, "
          f"from the true table {np.abs(got_fit - got_true).max():.3e} (reported, not asserted)")
    np.testing.assert_allclose(got_fit, want_fit, rtol=0, atol=EXAMPLE_COND * COLOR_RTOL * np.abs(want_fit).max())
