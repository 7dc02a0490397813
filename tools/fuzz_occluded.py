#!/usr/bin/env python3
"""Long differential run of trt_occluded_dev against trt_trace_dev (GPU box): N rounds of a seeded random scene (1-8 tori,
random axes in one round out of three) with up to 200,000 random rays — uniform origins, directions aimed at the scene or
uniform on the sphere, non-unit lengths, a random tmin — and per-ray bounds drawn from a handful of values (a NaN and one
equal to tmin among them).  trt_trace_dev runs once per distinct bound on that bound's rays; flag bytes and mask bits must
both equal its id >= 0, for all six solvers.  usage: fuzz_occluded.py [N=200] [seed=1]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from toroidal_ray_tracing_amd import abi
from toroidal_ray_tracing_amd.tracer import Tracer
from test_gpu_parity import random_case

n, seed = (int(sys.argv[1]) if len(sys.argv) > 1 else 200), (int(sys.argv[2]) if len(sys.argv) > 2 else 1)
t = Tracer(0)
dev = torch.device("cuda:0")
rng = np.random.default_rng(seed)
bad, rays, t0 = 0, 0, time.time()
up = lambda a: [torch.from_numpy(np.ascontiguousarray(a[:, k])).to(dev) for k in range(3)]
for k in range(n):
    sc = random_case(seed * 100000 + k)[0]
    if rng.integers(0, 3) == 0:
        sc.axes = abi.axes_array(rng.normal(size=(sc.n_tori, 3)), sc.n_tori)
    m = int(rng.integers(1, 200001))
    o = rng.uniform(-6.0, 6.0, (m, 3)).astype(np.float32)
    d = (rng.normal(size=(m, 3)) * rng.uniform(0.2, 3.0) - o) if rng.integers(0, 2) else rng.normal(size=(m, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    if rng.integers(0, 4) == 0:
        d *= np.float32(rng.uniform(0.25, 4.0))          # directions need not be unit vectors
    tmin = float(rng.choice([0.001, 0.0, 0.5]))
    values = np.float32([10000.0, 6.0, 2.5, tmin, np.nan, rng.uniform(0.5, 9.0)])
    pick = rng.integers(0, len(values), m)
    solver = int(rng.integers(0, 6))
    t.set_solver(solver)
    keep = up(o) + up(d)
    ptrs = [a.data_ptr() for a in keep]
    bound = torch.from_numpy(values[pick]).to(dev)
    flag = torch.full((m,), 9, dtype=torch.uint8, device=dev)
    mask = torch.full((abi.mask_words(m),), -1, dtype=torch.int64, device=dev)
    t.occluded_dev(sc, ptrs, m, flag_ptr=flag.data_ptr(), mask_ptr=mask.data_ptr(), tmax_ptr=bound.data_ptr(), tmin=tmin, tmax=-1.0)
    torch.cuda.synchronize()
    got = flag.cpu().numpy()
    want = np.zeros(m, np.uint8)                          # NaN and tmax == tmin: not occluded, whatever trt_trace does
    for j, v in enumerate(values):
        sub = np.flatnonzero(pick == j)
        if len(sub) == 0 or not v > np.float32(tmin):
            continue
        ks = up(o[sub]) + up(d[sub])
        ids = torch.empty(len(sub), dtype=torch.int32, device=dev)
        t.trace_dev(sc, [a.data_ptr() for a in ks], len(sub), {"id": ids.data_ptr()}, tmin=tmin, tmax=float(v))
        torch.cuda.synchronize()
        want[sub] = ids.cpu().numpy() >= 0
    ok = np.array_equal(got, want) and np.array_equal(abi.unpack_mask(mask.cpu().numpy().view(np.uint64), m), want.astype(bool))
    if not ok:
        bad += 1
        print(f"MISMATCH round {k}: solver {solver}, {m} rays, tmin {tmin}, {int((got != want).sum())} flags differ", flush=True)
    rays += m
    if k % 25 == 24:
        print(f"{k + 1} rounds, {rays / 1e6:.1f} M rays, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
t.close()
print(f"fuzz_occluded: {n} rounds, {rays / 1e6:.1f} M rays, {bad} mismatches")
sys.exit(1 if bad else 0)
