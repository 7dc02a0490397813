"""examples/absorbed_fit: one torus whose plasma emits and absorbs, "measured" by trt_glow_profile and fitted back twice
through the 17 x 17 normal equations — through trt_glow_weights, which ignores the absorption, and through
trt_glow_weights_absorbed; the printed numbers against the Python calls on the same scene, camera and table
(tests/absorbed_truth.py rebuilds them value for value)."""
import os
import re
import subprocess

import numpy as np
import pytest

import absorbed_truth as at
import weights_truth as wt
from conftest import ROOT
from test_absorbed_cpu import EXAMPLE_COND
from test_weights_cpu import EXAMPLE_COND as PLAIN_COND
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

COLOR_RTOL = 1e-5
K = abi.TRT_PROFILE_KNOTS


def test_absorbed_fit_example():
    exe = os.path.join(ROOT, "examples", "absorbed_fit")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    head = re.search(r"absorbed fit, 1 torus, (\d+)x(\d+), steps (\d+)", p.stdout)
    assert head and [int(v) for v in head.groups()] == [at.EXAMPLE_W, at.EXAMPLE_H, at.EXAMPLE_STEPS], p.stdout
    num = r"([-+.\deE]+)"
    sums = re.search(r"column sums:((?: %s){%d})\n" % (num[1:-1], K), p.stdout)
    assert sums, p.stdout
    got_sums = np.array(sums.group(1).split(), np.float64)
    res = re.search(r"forward residual: largest %s, over weighted chord \* largest knot %s" % (num, num), p.stdout)
    got_abs, got_rel = float(res.group(1)), float(res.group(2))
    got_min_T = float(re.search(r"min T: %s" % num, p.stdout).group(1))
    knots = re.findall(r"knot +(\d+): red plain %s absorbed %s \(true %s\) blue plain %s absorbed %s \(true %s\)" % ((num,) * 6), p.stdout)
    assert [int(m[0]) for m in knots] == list(range(K)), p.stdout
    got_plain = np.array([[float(m[1]), float(m[4])] for m in knots])
    got_fit = np.array([[float(m[2]), float(m[5])] for m in knots])
    got_true = np.array([[float(m[3]), float(m[6])] for m in knots])

    from toroidal_ray_tracing_amd.tracer import Tracer
    sc = abi.Scene([(wt.EXAMPLE_GEO[0], wt.EXAMPLE_GEO[1], wt.EXAMPLE_GEO[2], 0)], [camera.PLASTIC])
    table = at.example_table()
    with Tracer(0) as tr:
        o, d = tr.camera_rays(wt.example_globals(), abi.make_push(), at.EXAMPLE_W, at.EXAMPLE_H)
        L = tr.glow_profile(sc, o, d, [table], steps=at.EXAMPLE_STEPS).astype(np.float64)
        plain = tr.glow_weights(sc, o, d, steps=at.EXAMPLE_STEPS)[0].astype(np.float64)
        W, T = tr.glow_weights_absorbed(sc, o, d, [table], steps=at.EXAMPLE_STEPS)
    assert np.array_equal(T.view(np.uint32), L[:, 3].astype(np.float32).view(np.uint32))
    assert np.array_equal(got_true.astype(np.float32), table[:, [0, 2]])   # (nine digits give an FP32 back)
    W = W[0].astype(np.float64)
    np.testing.assert_allclose(got_sums, W.sum(1), rtol=COLOR_RTOL)
    np.testing.assert_allclose(got_min_T, T.min(), rtol=COLOR_RTOL)
    assert got_min_T < 0.6   # the plasma has optical depth
    # the forward identity, and its bar (tests/test_gpu_weights_absorbed.py, 3.: one torus, one piece)
    err = np.abs(W.T @ table[:, :3].astype(np.float64) - L[:, :3])
    top = table[:, :3].astype(np.float64).max(0)
    S = W.sum(0)
    hit = S > 0
    rel = (err[hit][:, [0, 2]] / (S[hit, None] * top[None, [0, 2]])).max()
    np.testing.assert_allclose([got_abs, got_rel], [err.max(), rel], rtol=COLOR_RTOL)
    assert got_rel <= (2 * at.EXAMPLE_STEPS + 2 + 24) * 2.0 ** -24 and (err[~hit] == 0).all()
    # both fits against Python's own solve of the same normal equations, at the condition number's tolerance
    y = L[:, [0, 2]]
    want_fit = np.linalg.solve(wt.normal_matrix(W), W @ y)
    want_plain = np.linalg.solve(wt.normal_matrix(plain), plain @ y)
    np.testing.assert_allclose(got_fit, want_fit, rtol=0, atol=EXAMPLE_COND * COLOR_RTOL * np.abs(want_fit).max())
    np.testing.assert_allclose(got_plain, want_plain, rtol=0, atol=PLAIN_COND * COLOR_RTOL * np.abs(want_plain).max())
    err_fit, err_plain = np.abs(got_fit - got_true).max(), np.abs(got_plain - got_true).max()
    print(f"largest knot error over red and blue: through trt_glow_weights {err_plain:.3e}, through trt_glow_weights_absorbed {err_fit:.3e}; "
          f"from Python's solve {np.abs(got_fit - want_fit).max():.3e}")
    assert err_fit < err_plain
