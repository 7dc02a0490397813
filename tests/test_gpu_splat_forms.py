"""The two-pass sorted form of trt_splat_dev (splat_count_kernel<4096, 4, true>, splat_scatter_sorted_kernel,
splat_resolve_bins_kernel<false>) against the oracle's sequential rasteriser, bit for bit.

The release library takes that form only for clouds the page scheme cannot address (tens of millions of points) and reads
no environment variable, so the test starts ONE fresh child process that loads the -DTRT_TUNING build build() makes
(libtrt_tuning.so) and switches forms with TRT_SPLAT_VARIANT + trt_debug_reload_tuning, as tools/check_splat_forms.py
does.  Before every call the child asks trt_debug_splat_mode which form the call takes: a knob that was silently ignored
would otherwise let the paged form pass this test."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORTED, PAGED, ONE_PASS = 1, 3, 0          # SplatMode (trt_splat.hpp)
N_SORTED_CALLS, N_OTHER_CALLS = 6, 2       # what _child() makes; the parent checks that it made them all


def _child():
    os.environ["TRT_LIB"] = os.path.join(ROOT, "toroidal_ray_tracing_amd", "libtrt_tuning.so")
    sys.path.insert(0, ROOT)
    import ctypes as C
    import numpy as np
    import torch
    from oracle import oracle
    from toroidal_ray_tracing_amd import camera
    from toroidal_ray_tracing_amd.tracer import Tracer

    oracle.lib()
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(33)
    made = {SORTED: 0, PAGED: 0, ONE_PASS: 0}
    with Tracer(0) as tr:
        reload_tuning, splat_mode = tr._L.trt_debug_reload_tuning, tr._L.trt_debug_splat_mode
        reload_tuning.restype, reload_tuning.argtypes = C.c_int, [C.c_void_p]
        splat_mode.restype, splat_mode.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_uint64]

        def call(variant, mode, d_pts, n, vp, W, H, out, want, what, **kw):
            """one trt_splat_dev call in the form `mode` (asserted), its image against `want`"""
            if variant is None:
                os.environ.pop("TRT_SPLAT_VARIANT", None)
            else:
                os.environ["TRT_SPLAT_VARIANT"] = str(variant)
            assert reload_tuning(tr._h) == 0
            got_mode = splat_mode(tr._h, W, H, kw.get("point_size", 2.5), n)
            assert got_mode == mode, f"{what}: splat_plan takes form {got_mode}, the test needs {mode}"
            out.fill_(-1.0)
            tr.splat_dev(d_pts.data_ptr() if n else 0, n, vp, W, H, out.data_ptr(), stream=s, **kw)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            bad = int((got != want.view(np.uint32)).any(axis=2).sum())
            print(f"{what}: form {got_mode}, {bad} of {W * H} pixels differ", flush=True)
            assert bad == 0, what
            made[mode] += 1

        def cloud(n, ties):
            pts = np.zeros((n, 8), np.float32)
            pts[:, :3] = rng.uniform(-3, 3, (n, 3))
            pts[:, 4:7] = rng.uniform(0, 1, (n, 3))
            pts[n // 3:n // 3 + ties] = pts[:ties]                     # duplicates: equal depth (across bins too), …
            pts[n // 3:n // 3 + ties, 4:7] = rng.uniform(0, 1, (ties, 3))   # … another colour: the smaller index wins
            pts[::97, :3] = np.finfo(np.float32).min                   # the "-nan" convention of loadPoints()
            pts[5::101, 0] = np.nan
            return pts

        def records_per_chunk(pts, vp, W, H, size):
            """host estimate (float64) of the records each chunk of 4,096 points has: one per 128x64 bin a point's rectangle touches"""
            with np.errstate(all="ignore"):
                cx, cy, cz, cw = (np.c_[pts[:, :3].astype(np.float64), np.ones(len(pts))] @ np.asarray(vp, np.float64).T).T
                ok = (cw > 0) & (np.abs(cx) <= cw) & (np.abs(cy) <= cw) & (cz >= 0) & (cz <= cw)
                xf, yf = np.where(ok, (cx / cw * 0.5 + 0.5) * W, 0.0), np.where(ok, (cy / cw * 0.5 + 0.5) * H, 0.0)
            x0, x1 = np.maximum(np.ceil(xf - size / 2 - 0.5), 0).astype(int), np.minimum(np.ceil(xf + size / 2 - 0.5), W).astype(int)
            y0, y1 = np.maximum(np.ceil(yf - size / 2 - 0.5), 0).astype(int), np.minimum(np.ceil(yf + size / 2 - 0.5), H).astype(int)
            ok &= (x0 < x1) & (y0 < y1)
            bins = np.where(ok, ((x1 - 1) // 128 - x0 // 128 + 1) * ((y1 - 1) // 64 - y0 // 64 + 1), 0)
            return np.add.reduceat(bins, np.arange(0, len(pts), 4096))

        # ragged image of 3 x 4 bins; 40,000 points = 9 chunks of 4,096 and a tail of 3,136: the count kernel runs 3 blocks of
        # 4 sub-chunks, the last two of them beyond n.  At point size 31.5 a chunk has more records than the staging area holds.
        W, H, n = 300, 200, 40_000
        pts = cloud(n, 2000)
        vp = camera.perspective_vk(70, W / H) @ camera.look_at((0.5, 1.0, 5.0), (0, 0, 0))
        d_pts = torch.from_numpy(pts).to(dev)
        out = torch.empty(H, W, 4, device=dev)
        want = {size: oracle.splat(pts, vp, W, H, point_size=size) for size in (2.5, 31.5)}
        # the cases this cloud is here for: at 2.5 every chunk fits the 4,608-slot staging area, at 31.5 chunks overflow it
        # (the straight-to-global path), and the last chunk is a tail
        small, big = records_per_chunk(pts, vp, W, H, 2.5), records_per_chunk(pts, vp, W, H, 31.5)
        print(f"records per chunk: point size 2.5 max {small.max()}, point size 31.5 min {big[:-1].min()} max {big.max()}", flush=True)
        assert len(big) == 10 and n % 4096 == 3136 and small.max() < 4608 * 0.9 and big[:-1].min() > 4608 * 1.1
        for size in (2.5, 31.5):
            call(1, SORTED, d_pts, n, vp, W, H, out, want[size], f"300x200 sorted, point size {size}", point_size=size)
        # the forms share the ctx's bin words: every call finds them zero and leaves them zero
        call(None, PAGED, d_pts, n, vp, W, H, out, want[2.5], "300x200 paged after sorted", point_size=2.5)
        call(1, SORTED, d_pts, n, vp, W, H, out, want[2.5], "300x200 sorted after paged", point_size=2.5)
        call(0, ONE_PASS, d_pts, n, vp, W, H, out, want[2.5], "300x200 one-pass after sorted", point_size=2.5)
        call(1, SORTED, d_pts, n, vp, W, H, out, want[31.5], "300x200 sorted after one-pass, point size 31.5", point_size=31.5)
        # no points at all in the sorted form: the clear colour everywhere
        clear = (0.1, 0.2, 0.3, 1.0)
        call(1, SORTED, d_pts, 0, vp, W, H, out, np.broadcast_to(np.float32(clear), (H, W, 4)).copy(), "300x200 sorted, no points", clear=clear)
        del d_pts, out
        # just over 512 bins (17 x 32 = 544): the instantiation whose LDS arrays hold kSortBins bins, four per thread
        W2, H2, n2 = 2176, 2048, 120_000
        pts2 = cloud(n2, 2000)
        vp2 = camera.perspective_vk(70, W2 / H2) @ camera.look_at((0.5, 1.0, 5.0), (0, 0, 0))
        d2 = torch.from_numpy(pts2).to(dev)
        out2 = torch.empty(H2, W2, 4, device=dev)
        call(1, SORTED, d2, n2, vp2, W2, H2, out2, oracle.splat(pts2, vp2, W2, H2, point_size=2.5), "2176x2048 sorted", point_size=2.5)
    print(f"sorted calls {made[SORTED]}, other calls {made[PAGED] + made[ONE_PASS]}, all bit-exact", flush=True)


@pytest.mark.gpu
def test_sorted_form_bit_exact():
    """Ragged 300x200 image (tail chunk, count-block tail, staging-area overflow at point size 31.5, depth ties, lowest()
    and NaN points), sorted / paged / sorted / one-pass in one ctx on shared bin words, no points, and 2176x2048 (544 bins:
    the wider instantiation) — every image equal to oracle.splat as uint32, every call's form asserted."""
    env = {k: v for k, v in os.environ.items() if k not in ("TRT_LIB", "TRT_SPLAT_VARIANT")}
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert f"sorted calls {N_SORTED_CALLS}, other calls {N_OTHER_CALLS}, all bit-exact" in p.stdout


if __name__ == "__main__":
    _child()
