#!/usr/bin/env python3
"""trt_shade_through_dev against trt_shade_dev, and trt_transmittance_dev against trt_occluded_dev, on the same rays.

  * the price of full enumeration: both shade calls on an ALL-OPAQUE scene — config 3's torus and config 4's nest of
    eight — on the pinhole camera's primary rays of a 1024² and a 4096² frame (trt_camera_rays_dev, left on the device);
  * the same with the outer shells translucent (the torus, and the four outer shells of the nest, at dissolve 0.25);
  * the soft shadow query against the any-hit query (flag bytes out) on those rays, opaque and translucent.

One process, the calls of a pair alternating inside every round, medians of device-event times with the spread beside
them (release library: there is no knob to turn).  --remarks FILE: the stderr of `make asm` (toroidal_ray_tracing_amd/
csrc), from which the resource report of the two kernels' instantiations is copied; --accuracy FILE: the output of
`pytest -s tests/test_gpu_through.py`, from which the lines with the measured maxima against the FP64 truth are copied.
usage: bench_through.py [--out profiles/r16_shade_through.txt] [--sizes 1024,4096] [--reps 2] [--rounds 5] [--remarks F] [--accuracy F]"""
import os, re, sys, statistics, subprocess
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from toroidal_ray_tracing_amd import abi, camera
from toroidal_ray_tracing_amd.tracer import Tracer


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


out_path, SIZES, REPS, ROUNDS = arg("--out", ""), arg("--sizes", "1024,4096"), arg("--reps", 2), arg("--rounds", 5)
remarks, accuracy = arg("--remarks", ""), arg("--accuracy", "")
dev = torch.device("cuda:0"); tr = Tracer(0); s = torch.cuda.current_stream()
lines = []


def say(line):
    print(line, flush=True); lines.append(line)


def scenes(outer):
    """config 3's torus and config 4's nest; `outer`: the dissolve of the torus / of the four outer shells of the nest."""
    single = abi.Scene([((0.0, 0.0, 0.0), 1.0, 0.25, 0)], [dict(camera.MIRROR, dissolve=outer)])
    nest = abi.Scene([((0.0, 0.0, 0.0), 1.0, 0.05 * (i + 1), 0 if i < 4 else 1) for i in range(8)],
                     [dict(camera.PLASTIC, dissolve=1.0), dict(camera.MIRROR, dissolve=outer)])
    return {"config 3 torus": (single, abi.TRT_SOLVE_F32), "config 4 nest (FP64 solve)": (nest, abi.TRT_SOLVE_F64),
            "config 4 nest (FP32 solve)": (nest, abi.TRT_SOLVE_F32)}


def timed(pairs):
    """pairs: name -> callable; every round times every callable once (REPS calls), round 0 is dropped."""
    res = {k: [] for k in pairs}
    for r in range(ROUNDS + 1):
        for k, fn in pairs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(REPS): fn()
            e1.record(s); torch.cuda.synchronize()
            if r: res[k].append(e0.elapsed_time(e1) / REPS)
    return res


def measure(size):
    W = H = size
    n = W * H
    g, pc = camera.baseline_camera(W, H), camera.baseline_push(5)
    rays = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(6)]
    ptrs = [r.data_ptr() for r in rays]
    tr.camera_rays_dev(g, pc, W, H, ptrs, stream=s.cuda_stream)
    img = {k: torch.empty(n * 4, dtype=torch.float32, device=dev) for k in ("shade", "through")}
    T = torch.empty(n, dtype=torch.float32, device=dev)
    flag = torch.empty(n, dtype=torch.uint8, device=dev)
    for outer in (1.0, 0.25):
        for name, (sc, solver) in scenes(outer).items():
            tr.set_solver(solver)
            pairs = {
                "trt_shade_dev": lambda: tr.shade_dev(sc, ptrs, n, pc, img["shade"].data_ptr(), stream=s.cuda_stream),
                "trt_shade_through_dev": lambda: tr.shade_through_dev(sc, ptrs, n, pc, img["through"].data_ptr(), stream=s.cuda_stream),
                "trt_occluded_dev (flags)": lambda: tr.occluded_dev(sc, ptrs, n, flag_ptr=flag.data_ptr(), stream=s.cuda_stream),
                "trt_transmittance_dev": lambda: tr.transmittance_dev(sc, ptrs, n, T.data_ptr(), stream=s.cuda_stream),
            }
            res = timed(pairs)
            tr.enable_stats(True)
            counts = {}
            for k in ("trt_shade_dev", "trt_shade_through_dev"):
                pairs[k](); counts[k] = tr.stats()
            tr.enable_stats(False)
            say(f"{name}, {W}x{H} = {n} camera rays, maxDepth 5, outer dissolve {outer}: median of {ROUNDS} rounds of {REPS} calls (min .. max)")
            for k in pairs:
                say(f"  {k:26s} {statistics.median(res[k]):9.4f} ms  ({min(res[k]):.4f} .. {max(res[k]):.4f})")
            a, b = statistics.median(res["trt_shade_dev"]), statistics.median(res["trt_shade_through_dev"])
            c, d = statistics.median(res["trt_occluded_dev (flags)"]), statistics.median(res["trt_transmittance_dev"])
            say(f"  through / shade = {b / a:.2f}; transmittance / occluded = {d / c:.2f}")
            for k, st in counts.items():
                tests = st["primary_tests"] + st["bounce_tests"] + st["shadow_tests"]
                say(f"  {k:26s} tests {tests} (primary {st['primary_tests']}, bounce {st['bounce_tests']}, shadow {st['shadow_tests']}), "
                    f"quartics solved {st['solved_tests']}, walk evaluations {st['evaluations']}")
            if outer == 1.0:
                same = torch.equal(img["shade"].view(torch.int32), img["through"].view(torch.int32))
                diff = int((img["shade"].view(n, 4) != img["through"].view(n, 4)).any(1).sum())
                say(f"  all opaque: images bit-identical: {same} ({diff} pixels differ); (T == 0) == flag on {int(((T == 0) == (flag == 1)).sum())} of {n} rays")
    tr.set_solver(abi.TRT_SOLVE_F32)


say(f"bench_through: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}")
try:   # the box state, read only
    smi = subprocess.run(["rocm-smi", "--showuse", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=60).stdout
    for ln in smi.splitlines():
        if "GPU[0]" in ln: say("  box: " + " ".join(ln.split()))
except Exception as e:   # noqa: BLE001
    say(f"  box: rocm-smi not available ({e})")
for size in [int(v) for v in SIZES.split(",")]:
    measure(size)
if remarks:
    say("resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
    keep = False
    for ln in open(remarks):
        m = re.search(r"remark:\s*(Function Name: (\S+)|(?:VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|TotalSGPRs): \S+)", ln)
        if not m:
            continue
        if m.group(2):
            keep = "transmittance_kernel" in m.group(2) or "shade_through_kernel" in m.group(2)
        if keep:
            say(("  " if m.group(2) else "    ") + m.group(1))
if accuracy:
    say("against the FP64 truth (tests/test_gpu_through.py::test_against_the_fp64_truth; bars: rel <= 1e-4 on 99.5 % of robust rays, max <= 2e-3):")
    for ln in open(accuracy):
        if "rel max" in ln:
            say("  " + ln.strip().lstrip("."))
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
