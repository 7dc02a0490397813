#!/usr/bin/env python3
"""fuzz_parity.py for the reuse of the tile lists (GPU box): N seeded random scenes / cameras / sizes / variants / solvers /
classification levels through ONE context with the reuse on, every frame repeated a random 1-4 times, and EVERY repeat
compared with the CPU oracle (first-hit records bit for bit, query counts equal, colours within the tolerance of tests/) and,
bit for bit, with the frame's first repeat.  The last line reports how many of the calls reused the lists: a run that
reused none has tested nothing.
usage: fuzz_list_reuse.py [N=300] [first_seed=100]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import oracle   # the checker, never the thing measured
from toroidal_ray_tracing_amd import abi
from toroidal_ray_tracing_amd.tracer import Tracer
from test_gpu_parity import random_case, assert_hits_equal, q, COLOR_RTOL, COLOR_ATOL

n, first = (int(sys.argv[1]) if len(sys.argv) > 1 else 300), (int(sys.argv[2]) if len(sys.argv) > 2 else 100)
oracle.lib()
t = Tracer(0)
rng = np.random.default_rng(first)
t0, bad, calls = time.time(), 0, 0
for k in range(n):
    sc, g, pc, W, H, cam = random_case(first + k)
    variant = ["listed", "persistent", "static"][int(rng.integers(0, 3))]
    solver = [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64, abi.TRT_SOLVE_FERRARI_F32][int(rng.integers(0, 3))]
    if variant == "persistent" and solver == abi.TRT_SOLVE_FERRARI_F32:
        solver = abi.TRT_SOLVE_F32
    counted = bool(rng.integers(0, 2))
    t.set_render_variant(variant); t.set_solver(solver); t.set_classification(int(rng.integers(-1, 2))); t.enable_stats(counted)
    wr, wh, _, wst = oracle.render(sc, g, pc, W, H, cam, precision=solver, nthreads=16)
    what = f"seed {first + k} ({variant}, solver {solver}, {W}x{H}, cam {cam})"
    first_rgba = None
    for rep in range(int(rng.integers(1, 5))):
        rgba, hits = t.render(sc, g, pc, W, H, cam)
        calls += 1
        st = t.stats() if counted else None
        try:
            assert_hits_equal(hits, wh, f"{what} repeat {rep}")
            np.testing.assert_allclose(rgba, wr, rtol=COLOR_RTOL, atol=COLOR_ATOL)
            assert st is None or q(st) == q(wst), (q(st), q(wst))
            assert first_rgba is None or np.array_equal(rgba.view(np.int32), first_rgba.view(np.int32)), "repeats differ"
        except AssertionError as e:
            bad += 1
            print(f"MISMATCH {what} repeat {rep}: {str(e)[:300]}", flush=True)
        if first_rgba is None:
            first_rgba = rgba
    if k % 50 == 49:
        print(f"{k + 1} frames, {calls} calls, {bad} mismatches, {t.list_reuse()}, {time.time() - t0:.0f} s", flush=True)
lr = t.list_reuse()
t.close()
print(f"fuzz: {n} frames, {calls} calls, classified {lr['classified']}, reused {lr['reused']}, {bad} mismatches")
sys.exit(1 if bad or not lr["reused"] else 0)
