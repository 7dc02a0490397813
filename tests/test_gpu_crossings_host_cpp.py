"""examples/shell_chords: lines of sight through a nest of three shells, trt_crossings on host buffers, the per-shell chord
lengths formed from the enter / leave pairs — the printed chords against the FP64 truth of tests/crossings_truth.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import crossings_truth as ct
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_shell_chords_example():
    exe = os.path.join(ROOT, "examples", "shell_chords")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    n = 16
    p = subprocess.run([exe, str(n)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = re.findall(r"line (\d+): y = ([-+.\d]+), (\d+) crossings, chords ([.\d]+) ([.\d]+) ([.\d]+)", p.stdout)
    assert len(rows) == n, p.stdout
    got = np.array([[float(v) for v in r] for r in rows])
    # the lines of the example, as it builds them in float
    y = (np.float32(-0.4) + np.float32(0.8) * (np.arange(n, dtype=np.float32) + np.float32(0.5)) / np.float32(n)).astype(np.float32)
    np.testing.assert_allclose(got[:, 1], y, atol=6e-5)   # (printed with four decimals)
    o = np.stack([np.full(n, -3.0, np.float32), y, np.full(n, 0.1, np.float32)], 1)
    d = np.tile(np.float32([1.0, 0.0, 0.0]), (n, 1))
    tori = ct.SCENES["nest3"][0]
    assert ct.classify_margin_all(o, d, tori).all()
    t, tid, en, cnt = ct.all_crossings(o, d, tori)
    assert np.array_equal(got[:, 2].astype(int), cnt) and cnt.max() == 12 and cnt.min() == 0
    # a chord is a sum of at most two differences of crossings at t < 4.5, each within 1e-5·t of the truth (the bar of
    # tests/test_gpu_crossings.py): 4 × 4.5e-5, and half a unit of the six printed decimals
    np.testing.assert_allclose(got[:, 3:], ct.chord_lengths(t, tid, en, 3), rtol=0, atol=4 * 4.5e-5 + 5e-7)
    assert (got[:, 3:].max(0) > [0.15, 0.25, 0.35]).all()
