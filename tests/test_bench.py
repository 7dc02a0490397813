"""bench.py without a GPU: its options, and the pixels --dump-outputs writes (the same in every run, within 64 MB)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_index_is_fixed_and_bounded():
    b = _bench()
    assert np.array_equal(b.dump_index(256 * 256), np.arange(256 * 256))
    n = 4096 * 4096
    i1, i2 = b.dump_index(n), b.dump_index(n)
    assert np.array_equal(i1, i2) and len(i1) == b.DUMP_PIXELS
    assert np.all(np.diff(i1) > 0) and i1[0] >= 0 and i1[-1] < n
    # rgba (16 B), the hit mask and the seven first-hit streams (4 B each) as float32, the index as float64
    assert b.DUMP_PIXELS * (16 + 8 * 4 + 8) <= 64 << 20


def test_bench_options():
    def run(*args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                              cwd=ROOT, timeout=120)
    p = run("--help")
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        p = run(*bad)
        assert p.returncode == 2 and "{" not in p.stdout
