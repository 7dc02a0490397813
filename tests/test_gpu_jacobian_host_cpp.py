"""examples/sigma_fit: absorbed_fit's plasma "measured" by trt_glow_project — radiance and transmittance of one view — and
fitted back by Gauss-Newton on trt_glow_tangent and trt_glow_adjoint, emission AND sigma unknown.  The recovered knots are
held to the KNOWN table, never to the code under test."""
import os
import re
import subprocess

import numpy as np
import pytest

import absorbed_truth as at
from conftest import ROOT
from toroidal_ray_tracing_amd import abi

pytestmark = pytest.mark.gpu

K = abi.TRT_PROFILE_KNOTS
TIME_LIMIT = 180   # seconds; the run takes some two thousand calls on 768 rays


def test_sigma_fit_example():
    """The residual falls from the first outer step to the last, and the joint fit's largest knot error — over the emission
    and over sigma — is smaller than that of the emission-only fit with sigma held at the start value.  Both errors are
    printed.  Measured on an MI355X (profiles/r31_glow_jacobian.txt): the residual falls from 4.59 to 1.3e-6 in 11 outer steps;
    joint fit 7.9e-7 (emission) and 1.5e-5 (sigma: all 17 knots from ONE view, because T is measured); emission-only fit at
    the start sigma 0.29.  The tighter bars are those errors times 4, which covers the spread of CGLS's stopping point
    between the two solvers: 3.2e-6 and 6.1e-5."""
    exe = os.path.join(ROOT, "examples", "sigma_fit")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=TIME_LIMIT)
    assert p.returncode == 0, p.stdout + p.stderr
    print(p.stdout)
    head = re.search(r"sigma fit, 1 torus, (\d+)x(\d+), steps (\d+)", p.stdout)
    assert head and [int(v) for v in head.groups()] == [at.EXAMPLE_W, at.EXAMPLE_H, at.EXAMPLE_STEPS], p.stdout
    num = r"([-+.\deE]+)"
    steps = [(float(a), float(b)) for a, b in re.findall(r"^joint outer step \d+: residual %s -> %s " % (num, num), p.stdout, flags=re.M)]
    final = float(re.search(r"^joint final residual: %s$" % num, p.stdout, flags=re.M).group(1))
    assert len(steps) >= 2 and final < steps[0][0] and steps[-1][1] <= steps[0][1], p.stdout
    knots = re.findall(r"knot +(\d+): red %s / %s \(true %s\) blue %s / %s \(true %s\) sigma %s / %s \(true %s\)" % ((num,) * 9), p.stdout)
    assert [int(m[0]) for m in knots] == list(range(K)), p.stdout
    v = np.array([[float(x) for x in m[1:]] for m in knots])                  # joint, held, true per red, blue, sigma
    table = at.example_table().astype(np.float64)
    assert np.allclose(v[:, [2, 5, 8]], table[:, [0, 2, 3]], rtol=1e-6, atol=1e-9)
    err_joint = np.abs(v[:, [0, 3, 6]] - table[:, [0, 2, 3]]).max(0)
    err_held = np.abs(v[:, [1, 4, 7]] - table[:, [0, 2, 3]]).max(0)
    print(f"sigma fit: residual {steps[0][0]:.3e} -> {final:.3e} in {len(steps)} outer steps; largest knot error, joint fit: emission "
          f"{err_joint[:2].max():.3e}, sigma {err_joint[2]:.3e}; emission-only fit at the start sigma: emission {err_held[:2].max():.3e}, "
          f"sigma {err_held[2]:.3e}")
    said = re.search(r"joint fit: largest emission knot error %s, largest sigma knot error %s" % (num, num), p.stdout)
    assert said and np.isclose(float(said.group(1)), err_joint[:2].max(), rtol=1e-2, atol=1e-7), p.stdout
    assert err_joint.max() < err_held.max()
    assert err_joint[:2].max() < 3.2e-6 and err_joint[2] < 6.1e-5
    assert err_joint[:2].max() < err_held[:2].max()
