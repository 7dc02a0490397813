"""examples/matrix_free_fit: absorbed_fit's plasma — one torus that emits and absorbs — "measured" by trt_glow_project and
fitted back by CGLS on trt_glow_project and trt_glow_backproject alone: the geometry matrix never leaves the GPU.  The
recovered knots are held to the KNOWN table, never to the code under test."""
import os
import re
import subprocess

import numpy as np
import pytest

import absorbed_truth as at
import weights_truth as wt
from conftest import ROOT
from test_absorbed_cpu import EXAMPLE_COND
from toroidal_ray_tracing_amd import abi

pytestmark = pytest.mark.gpu

K = abi.TRT_PROFILE_KNOTS
TIME_LIMIT = 120   # seconds; the run takes about a hundred pairs of calls on 768 rays


def test_matrix_free_fit_example():
    """The bar is the one the same plasma at the same step count is held to against its known table
    (tests/test_absorbed_cpu.py: the condition number of the normal matrix times the ridge, 5.80e3 * 1e-6): CGLS
    runs on exactly those normal equations, without forming them and without the ridge, on measurements that are W x
    rounded to float.  The iteration count is printed; no value is fixed for it."""
    exe = os.path.join(ROOT, "examples", "matrix_free_fit")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=TIME_LIMIT)
    assert p.returncode == 0, p.stdout + p.stderr
    head = re.search(r"matrix-free fit, 1 torus, (\d+)x(\d+), steps (\d+)", p.stdout)
    assert head and [int(v) for v in head.groups()] == [at.EXAMPLE_W, at.EXAMPLE_H, at.EXAMPLE_STEPS], p.stdout
    num = r"([-+.\deE]+)"
    sums = re.search(r"column sums:((?: %s){%d})\n" % (num[1:-1], K), p.stdout)
    assert sums, p.stdout
    got_sums = np.array(sums.group(1).split(), np.float64)
    iterations = int(re.search(r"iterations: (\d+)", p.stdout).group(1))
    knots = re.findall(r"knot +(\d+): red %s \(true %s\) blue %s \(true %s\)" % ((num,) * 4), p.stdout)
    assert [int(m[0]) for m in knots] == list(range(K)), p.stdout
    got = np.array([[float(m[1]), float(m[3])] for m in knots])
    got_true = np.array([[float(m[2]), float(m[4])] for m in knots])
    table = at.example_table()
    assert np.array_equal(got_true.astype(np.float32), table[:, [0, 2]])   # (nine digits give an FP32 back)
    err = np.abs(got - table[:, [0, 2]].astype(np.float64)).max()
    bar = EXAMPLE_COND * wt.EXAMPLE_RIDGE
    print(f"matrix-free fit: {iterations} iterations; largest knot error over red and blue {err:.3e}, bar {bar:.3e}")
    assert err < bar
    assert iterations >= 1 and (got_sums > 0).all()
