#!/usr/bin/env python3
"""trt_chords_dev and trt_glow_dev against the unfused route they replace, on the same rays.

The unfused route is what a caller had before: trt_crossings_dev with all 4 · n_tori slots (t, id, entering: 9 bytes per
slot and ray), then the pairing of entries and exits and the reduction in torch on the device — one pass over the slots
for the chords, one for the emission–absorption integral.  Rays: the pinhole camera's primary rays of a square frame
(trt_camera_rays_dev, left on the device; origins outside every tube, the full window — the one case the unfused route
handles without inside tests).  Scenes: config 3's torus and config 4's nest of eight shells (FP64 and FP32 solve), every
shell holding a medium.

One process, the calls alternating inside every round, medians of device-event times with the spread beside them; the
unfused route is timed whole and in its two parts.  The outputs of both routes are compared (largest difference), and
the bytes per ray each route writes and reads back are computed from the shapes.  --remarks FILE: the stderr of
`make asm` (toroidal_ray_tracing_amd/csrc), from which the resource report of the two kernels' instantiations is copied;
--accuracy FILE: the output of `pytest -s tests/test_gpu_media.py`, from which the lines with the measured maxima
against the FP64 truth are copied.
usage: bench_glow.py [--out profiles/r17_glow.txt] [--sizes 1024,2048] [--reps 2] [--rounds 5] [--remarks F] [--accuracy F]"""
import os, re, sys, statistics, subprocess
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path, SIZES, REPS, ROUNDS = arg("--out", ""), arg("--sizes", "1024,2048"), arg("--reps", 2), arg("--rounds", 5)
remarks, accuracy = arg("--remarks", ""), arg("--accuracy", "")
TMIN, TMAX = 0.001, 10000.0
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()
lines = []


def say(line):
    print(line, flush=True); lines.append(line)


def scenes():
    single = abi.Scene([((0.0, 0.0, 0.0), 1.0, 0.25, 0)], [camera.PLASTIC])
    nest = abi.Scene([((0.0, 0.0, 0.0), 1.0, 0.05 * (i + 1), 0) for i in range(8)], [camera.PLASTIC])
    m1 = [((1.0, 0.5, 0.25), 0.75)]
    m8 = [((0.25 * (i % 3) + 0.125, 0.125 * i, 1.0 / (i + 1)), 0.25 * (i % 4)) for i in range(8)]
    return {"config 3 torus": (single, m1, abi.TRT_SOLVE_F32), "config 4 nest (FP64 solve)": (nest, m8, abi.TRT_SOLVE_F64),
            "config 4 nest (FP32 solve)": (nest, m8, abi.TRT_SOLVE_F32)}


def timed(calls):
    """calls: name -> callable; every round times every callable once (REPS calls), round 0 is dropped."""
    res = {k: [] for k in calls}
    for r in range(ROUNDS + 1):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(REPS): fn()
            e1.record(s); torch.cuda.synchronize()
            if r: res[k].append(e0.elapsed_time(e1) / REPS)
    return res


def pair_chords(t, tid, en, n_tori, length):
    """The pairing rule on a slot-major list (origins outside, nothing open at the end of the window): (n_tori, n)."""
    K, n = t.shape
    rows = torch.arange(n, device=dev)
    acc = torch.zeros((n_tori, n), dtype=torch.float32, device=dev)
    opened = torch.zeros_like(acc)
    has = torch.zeros((n_tori, n), dtype=torch.bool, device=dev)
    for k in range(K):
        used = tid[k] >= 0
        j = tid[k].clamp(min=0).long()
        mine, at = has[j, rows], opened[j, rows]
        op = used & en[k] & ~mine
        cl = used & ~en[k] & mine
        opened[j, rows] = torch.where(op, t[k], at)
        acc[j, rows] = acc[j, rows] + torch.where(cl, (t[k] - at) * length, torch.zeros_like(at))
        has[j, rows] = (mine | op) & ~cl
    return acc


def integrate(t, tid, en, eps, sig, length):
    """The emission–absorption integral over the pieces between consecutive crossings of a slot-major list: (n, 4)."""
    K, n = t.shape
    rows = torch.arange(n, device=dev)
    active = torch.zeros((n, len(sig)), dtype=torch.float32, device=dev)
    u = torch.full((n,), TMIN, dtype=torch.float32, device=dev)
    L = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    T = torch.ones(n, dtype=torch.float32, device=dev)
    for k in range(K):
        used = tid[k] >= 0
        v = torch.where(used, t[k], u)
        e, sg = active @ eps, active @ sig
        ell = (v - u) * length
        tau = sg * ell
        w = torch.where(sg > 0, -torch.expm1(-tau) / sg.clamp(min=1e-30), ell)
        L += e * (w * T)[:, None]
        T = T * torch.exp(-tau)
        j = tid[k].clamp(min=0).long()
        active[rows, j] = torch.where(used, en[k].to(torch.float32), active[rows, j])
        u = v
    return torch.cat([L, T[:, None]], 1)


def measure(size):
    W = H = size
    n = W * H
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(1)
    rays = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(6)]
    ptrs = [r.data_ptr() for r in rays]
    tr.camera_rays_dev(g, pc, W, H, ptrs, stream=s.cuda_stream)
    length = torch.sqrt((rays[3] * rays[3] + rays[4] * rays[4]) + rays[5] * rays[5])
    for name, (sc, media, solver) in scenes().items():
        tr.set_solver(solver)
        nt = sc.n_tori
        K = 4 * nt
        med = abi.media(media)
        eps = torch.tensor([m[0] for m in media], dtype=torch.float32, device=dev)
        sig = torch.tensor([m[1] for m in media], dtype=torch.float32, device=dev)
        chord = torch.empty((nt, n), dtype=torch.float32, device=dev)
        rgba = torch.empty((n, 4), dtype=torch.float32, device=dev)
        t = torch.empty((K, n), dtype=torch.float32, device=dev)
        tid = torch.empty((K, n), dtype=torch.int32, device=dev)
        en = torch.empty((K, n), dtype=torch.uint8, device=dev)
        outs = {"t": t.data_ptr(), "id": tid.data_ptr(), "entering": en.data_ptr()}
        keep = {}

        def crossings():
            tr.crossings_dev(sc, ptrs, n, outs, max_per_ray=K, tmin=TMIN, tmax=TMAX, stream=s.cuda_stream)

        def reduce_chords():
            keep["chords"] = pair_chords(t, tid, en != 0, nt, length)

        def reduce_glow():
            keep["glow"] = integrate(t, tid, en != 0, eps, sig, length)

        calls = {
            "trt_chords_dev": lambda: tr.chords_dev(sc, ptrs, n, chord.data_ptr(), tmin=TMIN, tmax=TMAX, stream=s.cuda_stream),
            "trt_glow_dev": lambda: tr.glow_dev(sc, ptrs, n, med, rgba.data_ptr(), tmin=TMIN, tmax=TMAX, stream=s.cuda_stream),
            "trt_crossings_dev, all slots": crossings,
            "torch: pair and sum chords": reduce_chords,
            "torch: integrate the pieces": reduce_glow,
            "unfused chords (both parts)": lambda: (crossings(), reduce_chords()),
            "unfused glow (both parts)": lambda: (crossings(), reduce_glow()),
        }
        crossings(); torch.cuda.synchronize()
        res = timed(calls)
        med_ms = {k: statistics.median(v) for k, v in res.items()}
        say(f"{name}, {W}x{H} = {n} camera rays, {nt} tori, K = {K} slots: median of {ROUNDS} rounds of {REPS} calls (min .. max)")
        for k in calls:
            say(f"  {k:30s} {med_ms[k]:9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})")
        say(f"  unfused / fused: chords {med_ms['unfused chords (both parts)'] / med_ms['trt_chords_dev']:.2f}, "
            f"glow {med_ms['unfused glow (both parts)'] / med_ms['trt_glow_dev']:.2f}; "
            f"crossings alone / fused: chords {med_ms['trt_crossings_dev, all slots'] / med_ms['trt_chords_dev']:.2f}, "
            f"glow {med_ms['trt_crossings_dev, all slots'] / med_ms['trt_glow_dev']:.2f}")
        say(f"  bytes per ray beyond the 24 B of the ray itself: unfused {9 * K} B written by trt_crossings_dev and read again by the "
            f"reduction; fused {4 * nt} B (chords) / 16 B (glow) written")
        dc = (keep["chords"] - chord).abs()
        dg = (keep["glow"] - rgba).abs()
        say(f"  fused against unfused: chords differ in bits on {int((keep['chords'].view(torch.int32) != chord.view(torch.int32)).any(0).sum())} "
            f"of {n} rays (max {float(dc.max()):.3e}); glow max |dL| {float(dg[:, :3].max()):.3e}, max |dT| {float(dg[:, 3].max()):.3e}; "
            f"rays that see a medium: {float((rgba[:, 3] < 1).float().mean()):.3f}")
    tr.set_solver(abi.TRT_SOLVE_F32)


say(f"bench_glow: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
try:   # the box state, read only
    smi = subprocess.run(["rocm-smi", "--showuse", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=60).stdout
    for ln in smi.splitlines():
        if "GPU[0]" in ln: say("  box: " + " ".join(ln.split()))
except Exception as e:   # noqa: BLE001
    say(f"  box: rocm-smi not available ({e})")
for size in [int(v) for v in SIZES.split(",")]:
    measure(size)
if remarks:
    say("resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; glow_kernel adds 5 KiB of dynamic LDS per torus):")
    keep_line = False
    for ln in open(remarks):
        m = re.search(r"remark:\s*(Function Name: (\S+)|(?:VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|TotalSGPRs): \S+)", ln)
        if not m:
            continue
        if m.group(2):
            keep_line = "chords_kernel" in m.group(2) or "glow_kernel" in m.group(2)
        if keep_line:
            say(("  " if m.group(2) else "    ") + m.group(1))
if accuracy:
    say("against the FP64 truth (tests/test_gpu_media.py::test_against_the_fp64_truth; error, and error / derived bar, on robust rays):")
    for ln in open(accuracy):
        if "max error (and error / bar)" in ln:
            say("  " + ln.strip().lstrip("."))
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
