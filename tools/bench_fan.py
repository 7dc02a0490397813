#!/usr/bin/env python3
"""trt_fan_occluded_dev (K = 16 cosine-distributed directions about the normal, tmax = 0.5) in both of its forms
(TRT_FAN_FORM, tuning build) against the composition a caller had before it: explicit rays built on the device by torch,
trt_occluded_dev, a torch reduce of the flags to one word and one number per point.

Workloads: the first-hit record of the 4096² config-3 frame (single torus, pinhole; ~85 % of its points are dead), as it
stands; and 2²² all-live points — that record compacted, and repeated to fill (a 4096² frame has ~2.5 M live points).
The composition is timed whole and in its three parts; on the frame record also in the form a careful caller would write,
which compacts the live points first and scatters the result back.  One process, alternating launches, medians of
device-event times; every form's words are compared with the fused default's.
usage: bench_fan.py [--out profiles/r14_fan_occluded.txt] [--size 4096] [--reps 5] [--rounds 7]"""
import os, sys, statistics, subprocess
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tuning  # noqa: E402  (loads the -DTRT_TUNING build, see _tuning.py)
import numpy as np
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path, SIZE, REPS, ROUNDS = arg("--out", ""), arg("--size", 4096), arg("--reps", 5), arg("--rounds", 7)
K, TMIN, TMAX = 16, 0.001, 0.5
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()
sc = camera.single_torus_scene()
lines = []


def say(line):
    print(line, flush=True); lines.append(line)


def table(k):
    """The fixed table of examples/ambient_occlusion_main.cpp."""
    i = np.arange(k, dtype=np.float64)
    u, v = (i + 0.5) / k, np.fmod(i * 0.6180339887498949, 1.0)
    return np.stack([np.sqrt(u) * np.cos(2 * np.pi * v), np.sqrt(u) * np.sin(2 * np.pi * v), np.sqrt(1 - u)], 1).astype(np.float32)


DIRS = table(K)
T_DIRS = torch.from_numpy(DIRS).to(dev)


def frame_record():
    W = H = SIZE
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(1)
    rec = {k: torch.empty(W * H, device=dev, dtype=torch.int32 if k == "id" else torch.float32) for k in abi.HIT_FIELDS[1:]}
    tr.render_dev(sc, g, pc, W, H, 0, hit_ptrs={k: v.data_ptr() for k, v in rec.items()}, stream=s.cuda_stream)
    torch.cuda.synchronize()
    return rec


def all_live(rec, n):
    live = rec["id"] >= 0
    idx = torch.nonzero(live).squeeze(1)
    idx = idx.repeat((n + len(idx) - 1) // len(idx))[:n]
    return {k: v[idx].contiguous() for k, v in rec.items()}


def build_rays(P, N):
    """The header's arithmetic in torch (FP32; torch fuses nothing across operators): six streams of K * n floats."""
    nx, ny, nz = N
    sg = torch.copysign(torch.ones_like(nz), nz)
    a = -1.0 / (sg + nz)
    b = (nx * ny) * a
    T = (1.0 + ((sg * nx) * nx) * a, sg * b, (-sg) * nx)
    B = (b, sg + (ny * ny) * a, -ny)
    lx, ly, lz = T_DIRS[:, 0:1], T_DIRS[:, 1:2], T_DIRS[:, 2:3]
    d = [(((lx * T[k][None]) + (ly * B[k][None])) + (lz * N[k][None])).reshape(-1) for k in range(3)]
    o = [P[k][None].expand(K, -1).reshape(-1) for k in range(3)]
    return o + d


SHIFT = torch.arange(K, device=dev, dtype=torch.int64)[:, None]


def reduce_flags(flag, n):
    f = flag.view(K, n)
    bits = (f.to(torch.int64) << SHIFT).sum(0)
    opn = (K - f.sum(0, dtype=torch.int32)).to(torch.float32) / float(K)
    return bits, opn


def measure(name, rec, compacted_too):
    n = rec["px"].numel()
    ptrs = {k: v.data_ptr() for k, v in rec.items()}
    P, N = [rec[k] for k in ("px", "py", "pz")], [rec[k] for k in ("nx", "ny", "nz")]
    live_share = float((rec["id"] >= 0).float().mean())
    bits = {f: torch.empty(n, dtype=torch.int64, device=dev) for f in (0, 1)}
    opn = {f: torch.empty(n, dtype=torch.float32, device=dev) for f in (0, 1)}
    flag = torch.empty(K * n, dtype=torch.uint8, device=dev)
    keep = {}

    def fused(form):
        def run():
            tr.fan_occluded_dev(sc, ptrs, n, DIRS, bits_ptr=bits[form].data_ptr(), open_ptr=opn[form].data_ptr(), tmin=TMIN, tmax=TMAX,
                                stream=s.cuda_stream)
        return run

    def comp_build():
        keep["rays"] = build_rays(P, N)

    def comp_query():
        tr.occluded_dev(sc, [r.data_ptr() for r in keep["rays"]], K * n, flag_ptr=flag.data_ptr(), tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)

    def comp_reduce():
        keep["bits"], keep["open"] = reduce_flags(flag, n)
        dead = rec["id"] < 0   # the contract's dead points: bits 0, open 1
        keep["bits"].masked_fill_(dead, 0); keep["open"].masked_fill_(dead, 1.0)

    def comp_all():
        comp_build(); comp_query(); comp_reduce()

    def comp_compacted():
        idx = torch.nonzero(rec["id"] >= 0).squeeze(1)
        m = idx.numel()   # (a host read-back: the caller needs the ray count)
        rays = build_rays([p[idx] for p in P], [q[idx] for q in N])
        fl = flag[:K * m]
        tr.occluded_dev(sc, [r.data_ptr() for r in rays], K * m, flag_ptr=fl.data_ptr(), tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)
        b, o = reduce_flags(fl, m)
        keep["cbits"] = torch.zeros(n, dtype=torch.int64, device=dev).index_copy_(0, idx, b)
        keep["copen"] = torch.ones(n, dtype=torch.float32, device=dev).index_copy_(0, idx, o)

    cases = {"fused form A (lane)": (0, fused(0)), "fused form B (block)": (1, fused(1)), "composition: whole": (None, comp_all),
             "composition: ray build (torch)": (None, comp_build), "composition: trt_occluded_dev": (None, comp_query),
             "composition: reduce (torch)": (None, comp_reduce)}
    if compacted_too:
        cases["composition on compacted live points: whole"] = (None, comp_compacted)
    res = {k: [] for k in cases}
    for r in range(ROUNDS + 1):   # round 0 warms up and is dropped; every round times every case once
        for k, (form, fn) in cases.items():
            if form is not None:
                os.environ["TRT_FAN_FORM"] = str(form); _tuning.reload(tr)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(REPS): fn()
            e1.record(s); torch.cuda.synchronize()
            if r: res[k].append(e0.elapsed_time(e1) / REPS)
    say(f"{name}: n = {n} points, live share {live_share:.3f}, K = {K}, window ({TMIN}, {TMAX}); median of {ROUNDS} rounds of {REPS} calls (min .. max)")
    for k in cases:
        say(f"  {k:46s} {statistics.median(res[k]):9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})")
    same = torch.equal(bits[0], bits[1]) and torch.equal(opn[0], opn[1])
    comp = torch.equal(bits[0], keep["bits"]) and torch.equal(opn[0], keep["open"])
    say(f"  forms A and B identical: {same}; composition identical to the fused words and open: {comp}"
        + (f"; compacted composition identical: {torch.equal(bits[0], keep['cbits']) and torch.equal(opn[0], keep['copen'])}" if compacted_too else ""))
    occ = float((opn[0][rec['id'] >= 0] < 1.0).float().mean()) if live_share else 0.0
    say(f"  live points with an occluded sample: {occ:.3f}; mean open over live points {float(opn[0][rec['id'] >= 0].mean()):.4f}")
    fused_b = n * (28 + 12)
    comp_b = n * 28 + 2 * 24 * K * n + 2 * K * n + 12 * n
    say(f"  bytes (arithmetic): fused {fused_b / 1e6:.0f} MB (28 B read + 12 B written per point; a dead point reads its 4-B id only); "
        f"composition {comp_b / 1e6:.0f} MB (rays written and read back at 24 B x K, flags 1 B x K twice, torch temporaries not counted)")
    return {k: statistics.median(v) for k, v in res.items()}


say(f"bench_fan: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
try:   # the box state, read only
    smi = subprocess.run(["rocm-smi", "--showuse", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=60).stdout
    for ln in smi.splitlines():
        if "GPU[0]" in ln: say("  box: " + " ".join(ln.split()))
except Exception as e:   # noqa: BLE001
    say(f"  box: rocm-smi not available ({e})")
rec = frame_record()
a = measure(f"frame record {SIZE}x{SIZE} (config 3)", rec, True)
b = measure("all-live points (the record compacted and repeated)", all_live(rec, 1 << 22), False)
fa, fb = a["fused form A (lane)"], a["fused form B (block)"]
say(f"on the frame record form {'A' if fa <= fb else 'B'} is faster ({min(fa, fb):.4f} against {max(fa, fb):.4f} ms); "
    f"the composition takes {a['composition: whole']:.4f} ms, {a['composition: whole'] / min(fa, fb):.1f} x the faster fused form")
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
