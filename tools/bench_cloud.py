#!/usr/bin/env python3
"""Capture -> point cloud (trt_cloud_dev) on the 4096x2048 toroidal capture of bench_splat.py: the three modes, the
four-strided-torch-copies assembly they replace (bench_splat.py), and what the re-projection (trt_splat_dev) makes of the
KEEP_ALL, MARK_MISSES and COMPACT clouds for the view used there.  One process, the cases in alternating rounds; ms are
medians over the rounds of device-event times around `reps` back-to-back calls.
GB/s are ALGORITHMIC bytes over that time: KEEP / MARK / torch 32 B read + 32 B written per record, COMPACT 2 x 32 B read
per record + 32 B written per kept point; "fetched" counts what the memory system moves when it fetches a record's whole
64-B line for the 32 B (or, in COMPACT's count pass, 16 B) a lane asks for.
usage: python tools/bench_cloud.py [--reps 10] [--rounds 7] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402
from toroidal_ray_tracing_amd import abi, camera  # noqa: E402
from toroidal_ray_tracing_amd.tracer import Tracer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
opt = ap.parse_args()

dev = torch.device("cuda:0")
tr = Tracer(0)
s = torch.cuda.current_stream()
W, H = 4096, 2048
n = W * H
sc = camera.single_torus_scene(R=6.0, r=1.5, material=camera.PLASTIC)
g, pc = camera.toroidal_camera(W, H), abi.make_push(max_depth=3, rho=4.0)
rend = torch.empty(n, 16, device=dev)
tr.render_dev(sc, g, pc, W, H, 0, camera=abi.TRT_CAMERA_TOROIDAL, rendered_ptr=rend.data_ptr(), stream=s.cuda_stream)
vp = camera.perspective_vk(60, 1.0) @ camera.look_at((0.5, 1.0, -1.0), (6.0, 0.0, 2.0))
img = torch.empty(2048, 2048, 4, device=dev)
counts = torch.zeros(2, dtype=torch.int64, device=dev)
clouds = {m: torch.zeros(n, 8, device=dev) for m in ("keep", "mark", "compact", "torch")}
MODE = {"keep": abi.TRT_CLOUD_KEEP_ALL, "mark": abi.TRT_CLOUD_MARK_MISSES, "compact": abi.TRT_CLOUD_COMPACT}


def build(name):
    tr.cloud_dev(rend.data_ptr(), n, clouds[name].data_ptr(), n, counts.data_ptr(), mode=MODE[name], stream=s.cuda_stream)


def torch_assembly():   # tools/bench_splat.py: the only way to do this without trt_cloud_dev
    cloud = clouds["torch"]
    cloud[:, :3] = rend[:, 0:3]; cloud[:, 3] = 0; cloud[:, 4:7] = rend[:, 4:7]; cloud[:, 7] = 0


n_pts = {}
for name in MODE:
    n_pts[name] = tr.cloud(rend, clouds[name], mode=MODE[name], counts=counts, stream=s.cuda_stream)[0]
torch_assembly()
torch.cuda.synchronize()
n_pts["torch"] = n
kept = n_pts["compact"]
torch_same = torch.equal(clouds["torch"].view(torch.int32), clouds["keep"].view(torch.int32))   # unless the capture holds a NaN


def splat(name):
    tr.splat_dev(clouds[name].data_ptr(), n_pts[name], vp, 2048, 2048, img.data_ptr(), stream=s.cuda_stream)


covered, shown = {}, {}
for name in ("keep", "mark", "compact"):
    splat(name)
    torch.cuda.synchronize()
    covered[name] = (img[..., :3] != 0.8).any(dim=2).float().mean().item()
    shown[name] = img.clone()
assert torch.equal(shown["mark"].view(torch.int32), shown["compact"].view(torch.int32)), "the MARK and the COMPACT cloud re-project differently"
del shown

cases = [("cloud KEEP_ALL", lambda: build("keep")), ("cloud MARK_MISSES", lambda: build("mark")),
         ("cloud COMPACT", lambda: build("compact")), ("torch, 4 strided copies", torch_assembly),
         ("splat of KEEP_ALL cloud", lambda: splat("keep")), ("splat of MARK cloud", lambda: splat("mark")),
         ("splat of COMPACT cloud", lambda: splat("compact"))]
times = {name: [] for name, _ in cases}
for rnd in range(opt.rounds + 1):           # round 0 warms every shape up and is dropped
    for name, fn in cases:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(opt.reps):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        if rnd:
            times[name].append(e0.elapsed_time(e1) / opt.reps)

alg = {"cloud KEEP_ALL": 64 * n, "cloud MARK_MISSES": 64 * n, "torch, 4 strided copies": 64 * n, "cloud COMPACT": 64 * n + 32 * kept}
fetched = {"cloud KEEP_ALL": 96 * n, "cloud MARK_MISSES": 96 * n, "cloud COMPACT": 128 * n + 32 * kept}
lines = [f"{W}x{H} toroidal capture: {n} records, {kept} hits ({100 * kept / n:.1f} %), {n - kept} misses; "
         f"{opt.rounds} alternating rounds of {opt.reps} calls, median (min .. max) ms",
         f"view covered: KEEP_ALL {100 * covered['keep']:.1f} %, MARK_MISSES {100 * covered['mark']:.1f} %, COMPACT {100 * covered['compact']:.1f} % "
         "(MARK and COMPACT images identical; KEEP_ALL also draws the misses at the origin)"]
lines.append("KEEP_ALL cloud == torch assembly, bit for bit: " + ("yes" if torch_same else "NO (a NaN in the capture: the torch assembly keeps it)"))
for name, _ in cases:
    t = times[name]
    med = statistics.median(t)
    line = f"{name:26s} {med:8.4f} ms ({min(t):.4f} .. {max(t):.4f})"
    if name in alg:
        line += f"  {alg[name] / med / 1e6:7.0f} GB/s algorithmic"
    if name in fetched:
        line += f", {fetched[name] / med / 1e6:7.0f} GB/s if whole 64-B records are fetched"
    lines.append(line)
base = statistics.median(times["torch, 4 strided copies"])
for name in ("cloud KEEP_ALL", "cloud MARK_MISSES", "cloud COMPACT"):
    lines.append(f"{name} vs torch assembly: {base / statistics.median(times[name]):.2f}x")
for a, b in (("cloud MARK_MISSES", "splat of MARK cloud"), ("cloud COMPACT", "splat of COMPACT cloud"), ("torch, 4 strided copies", "splat of KEEP_ALL cloud")):
    lines.append(f"{a} + {b}: {statistics.median(times[a]) + statistics.median(times[b]):.4f} ms")
text = "\n".join(lines)
print(text)
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")
