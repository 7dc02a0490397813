"""trt_cloud_dev — capture -> point cloud on the device — against its numpy restatement (tests/cloud_truth.py).
Every comparison is bit for bit (uint32 views); no tolerance is involved."""
import ctypes as C

import numpy as np
import pytest

import cloud_truth as ct
from toroidal_ray_tracing_amd import abi, camera, lib

pytestmark = pytest.mark.gpu

CHUNK = abi.TRT_CLOUD_CHUNK          # kCloudChunk (csrc/trt_cloud.hpp): records per block of the count and scatter passes
assert CHUNK == 1024                 # 256 lanes x 4 records; a wave's trip is 64 records, a block's trip 256
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17)
PATTERNS = ("none", "all", "alternating", "last_chunk", "last_record", "first_miss", "random15")
MODES = (abi.TRT_CLOUD_KEEP_ALL, abi.TRT_CLOUD_MARK_MISSES, abi.TRT_CLOUD_COMPACT)
POISON = np.uint32(0xDEADBEEF)
GUARD = 96                           # points behind `capacity` that must stay poisoned


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def miss_mask(pattern, n, rng):
    i = np.arange(n)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "alternating":
        return i % 2 == 1
    if pattern == "last_chunk":      # hits only in the last chunk
        return i < (max(n, 1) - 1) // CHUNK * CHUNK
    if pattern == "last_record":     # a single hit, in the last record
        return i != n - 1
    if pattern == "first_miss":      # a single miss, in the first record
        return i == 0
    assert pattern == "random15"
    return rng.uniform(size=n) >= 0.15


def synthetic(n, miss, rng):
    """n records of random BITS (so NaNs of both signs, infinities and denormals occur in positions and colours, and the
    ray half is noise that must not matter); a miss gets pos.xyz = +-0, some hits one or two zero components."""
    bits = rng.integers(0, 2 ** 32, size=(n, 16), dtype=np.uint64).astype(np.uint32)
    hit = np.flatnonzero(~miss)
    bits[hit[::5], 1] = 0                                   # hits with a zero component (pos.y, some also pos.x = -0)
    bits[hit[::15], 0] = 0x80000000
    bits[hit, 2] |= 1                                       # … but never three: pos.z of a hit is not a zero
    sign = rng.integers(0, 2, size=(int(miss.sum()), 3), dtype=np.uint64).astype(np.uint32) << np.uint32(31)
    bits[miss, 0:3] = sign
    return bits.view(np.float32)


def to_dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def poisoned(capacity, torch):
    return torch.from_numpy(np.full((capacity + GUARD, 8), POISON, np.uint32).view(np.int32)).to("cuda:0")


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("mode", MODES)
def test_synthetic_records(tr, mode):
    """Record counts that straddle a wave's trip (64), a block's trip (256) and the chunk (1024), every miss pattern: output
    points and both counts equal cloud_truth; the guard behind `capacity` stays poisoned."""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(100 + mode)
    cases = [(n, p, n) for n in SIZES for p in PATTERNS]
    cases += [(3 * CHUNK + 17, p, 2 * CHUNK + 5) for p in ("none", "random15")]   # a capacity that is too small
    cases += [(CHUNK + 1, "none", 0)]                                              # … and none at all
    for n, pattern, capacity in cases:
        rec = synthetic(n, miss_mask(pattern, n, rng), rng)
        d_rec = to_dev(rec, torch)
        d_pts = poisoned(capacity, torch)
        d_cnt = torch.tensor([12345, 67890], dtype=torch.int64, device="cuda:0")   # not appending: ignored
        tr.cloud_dev(d_rec.data_ptr(), n, d_pts.data_ptr(), capacity, d_cnt.data_ptr(), mode=mode, stream=s)
        torch.cuda.synchronize()
        want, counts = ct.cloud(rec, mode, np.full((capacity, 8), POISON, np.uint32))
        got = as_u32(d_pts)
        what = f"mode {mode}, {n} records, {pattern}, capacity {capacity}"
        assert tuple(d_cnt.tolist()) == counts, what
        np.testing.assert_array_equal(got[:capacity], want, err_msg=what)
        assert (got[capacity:] == POISON).all(), what


def test_append(tr):
    """Three captures of different sizes appended in COMPACT mode, nothing synchronised in between: the concatenation of
    cloud_truth's clouds — also when the capacity falls in the middle of the second capture."""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    recs = [synthetic(n, rng.uniform(size=n) >= 0.4, rng) for n in (1500, 2 * CHUNK + 3, 700)]
    d_recs = [to_dev(r, torch) for r in recs]
    parts = [ct.points_of(r, ct.COMPACT) for r in recs]
    total = sum(len(p) for p in parts)
    assert all(len(p) > 100 for p in parts)
    for capacity in (total + 10, total, len(parts[0]) + len(parts[1]) // 2):
        d_pts = poisoned(capacity, torch)
        d_cnt = torch.tensor([55, 66], dtype=torch.int64, device="cuda:0")
        want, counts = np.full((capacity, 8), POISON, np.uint32), (55, 66)
        for k, (r, d) in enumerate(zip(recs, d_recs)):
            tr.cloud_dev(d.data_ptr(), len(r), d_pts.data_ptr(), capacity, d_cnt.data_ptr(), mode=abi.TRT_CLOUD_COMPACT,
                         append=k > 0, stream=s)
            want, counts = ct.cloud(r, ct.COMPACT, want, counts, append=k > 0)
        torch.cuda.synchronize()
        got = as_u32(d_pts)
        assert tuple(d_cnt.tolist()) == counts == (min(total, capacity), total)
        np.testing.assert_array_equal(got[:capacity], want)
        np.testing.assert_array_equal(got[:counts[0]], np.concatenate(parts)[:counts[0]])
        assert (got[counts[0]:] == POISON).all()
    # modes may be mixed in one cloud, and an empty capture only moves the counts
    capacity = len(recs[0]) + len(parts[1]) + 5
    d_pts = poisoned(capacity, torch)
    d_cnt = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    tr.cloud_dev(d_recs[0].data_ptr(), len(recs[0]), d_pts.data_ptr(), capacity, d_cnt.data_ptr(), mode=abi.TRT_CLOUD_MARK_MISSES, stream=s)
    tr.cloud_dev(0, 0, d_pts.data_ptr(), capacity, d_cnt.data_ptr(), mode=abi.TRT_CLOUD_COMPACT, append=True, stream=s)
    tr.cloud_dev(d_recs[1].data_ptr(), len(recs[1]), d_pts.data_ptr(), capacity, d_cnt.data_ptr(), mode=abi.TRT_CLOUD_COMPACT, append=True, stream=s)
    torch.cuda.synchronize()
    want, counts = ct.cloud(recs[0], ct.MARK_MISSES, np.full((capacity, 8), POISON, np.uint32))
    want, counts = ct.cloud(recs[1], ct.COMPACT, want, counts, append=True)
    assert tuple(d_cnt.tolist()) == counts == (capacity - 5, capacity - 5)
    np.testing.assert_array_equal(as_u32(d_pts)[:capacity], want)
    assert tr.cloud(d_recs[2].view(torch.float32), d_pts[:capacity].view(torch.float32), counts=d_cnt, append=True) == (capacity, capacity - 5 + len(parts[2]))


# The capture of the end-to-end tests: the plastic torus and toroidal camera of tools/bench_splat.py at 256x128
EW, EH = 256, 128
VW, VH = 192, 160


def capture_setup():
    sc = camera.single_torus_scene(R=6.0, r=1.5, material=camera.PLASTIC)
    g, pc = camera.toroidal_camera(EW, EH), abi.make_push(max_depth=3, rho=4.0)
    vp = camera.perspective_vk(60, VW / VH) @ camera.look_at((0.5, 1.0, -1.0), (6.0, 0.0, 2.0))
    return sc, g, pc, vp


def test_capture_to_cloud_to_reprojection(tr, oracle):
    """Toroidal capture -> cloud in each mode == cloud_truth of the same RenderedData; the re-projections of the MARK and of
    the COMPACT cloud are the same image, the one oracle.splat draws from the numpy cloud."""
    import torch
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    sc, g, pc, vp = capture_setup()
    n = EW * EH
    rend = torch.empty(n, 16, device=dev)
    tr.render_dev(sc, g, pc, EW, EH, 0, camera=abi.TRT_CAMERA_TOROIDAL, rendered_ptr=rend.data_ptr(), stream=s)
    torch.cuda.synchronize()
    rec = rend.cpu().numpy()
    miss = ct.is_miss(rec)
    assert 0.05 < miss.mean() < 0.95, miss.mean()          # both hits and misses, or the test would pass vacuously
    images = {}
    for mode in MODES:
        d_pts = poisoned(n, torch)
        have, wanted = tr.cloud(rend, d_pts[:n].view(torch.float32), mode=mode, stream=s)
        want, counts = ct.cloud(rec, mode, np.full((n, 8), POISON, np.uint32))
        assert (have, wanted) == counts
        assert have == (n if mode != abi.TRT_CLOUD_COMPACT else int((~miss).sum()))
        got = as_u32(d_pts)
        np.testing.assert_array_equal(got[:n], want)
        assert (got[n:] == POISON).all()
        if mode != abi.TRT_CLOUD_KEEP_ALL:
            out = torch.zeros(VH, VW, 4, device=dev)
            tr.splat_dev(d_pts.data_ptr(), have, vp, VW, VH, out.data_ptr(), stream=s)
            torch.cuda.synchronize()
            images[mode] = out.cpu().numpy().view(np.uint32)
    want_img = oracle.splat(ct.points_of(rec, ct.COMPACT).view(np.float32), vp, VW, VH).view(np.uint32)
    np.testing.assert_array_equal(images[abi.TRT_CLOUD_COMPACT], want_img)
    np.testing.assert_array_equal(images[abi.TRT_CLOUD_MARK_MISSES], want_img)
    covered = (want_img.view(np.float32)[..., :3] != np.float32(0.8)).any(axis=2).mean()
    assert 0.02 < covered < 0.98


def test_cloud_in_a_graph(tr):
    """render + trt_cloud_dev (COMPACT, then MARK) + trt_splat_dev of the MARK cloud in one hipGraph, captured the way
    test_graph_of_32_frames_and_mixed_eager_replay captures: replayed twice with an eager call on another capture in
    between, the outputs equal the eager ones; a call that would grow the scratch under capture is refused."""
    import torch
    from toroidal_ray_tracing_amd.tracer import Tracer, TrtError
    dev = torch.device("cuda:0")
    sc, g, pc, vp = capture_setup()
    n = EW * EH
    cur = torch.cuda.current_stream()

    def buffers():
        return dict(rend=torch.zeros(n, 16, device=dev), comp=poisoned(n, torch), mark=poisoned(n, torch),
                    ccnt=torch.zeros(2, dtype=torch.int64, device=dev), mcnt=torch.zeros(2, dtype=torch.int64, device=dev),
                    img=torch.zeros(VH, VW, 4, device=dev))

    def frame(b, stream):
        tr.render_dev(sc, g, pc, EW, EH, 0, camera=abi.TRT_CAMERA_TOROIDAL, rendered_ptr=b["rend"].data_ptr(), stream=stream)
        tr.cloud_dev(b["rend"].data_ptr(), n, b["comp"].data_ptr(), n, b["ccnt"].data_ptr(), mode=abi.TRT_CLOUD_COMPACT, stream=stream)
        tr.cloud_dev(b["rend"].data_ptr(), n, b["mark"].data_ptr(), n, b["mcnt"].data_ptr(), mode=abi.TRT_CLOUD_MARK_MISSES, stream=stream)
        tr.splat_dev(b["mark"].data_ptr(), n, vp, VW, VH, b["img"].data_ptr(), stream=stream)

    eager, replayed = buffers(), buffers()
    frame(eager, cur.cuda_stream)                   # also sizes the ctx's scratch and uploads the camera tables
    torch.cuda.synchronize()
    kept = int(eager["ccnt"][0])
    assert 0 < kept < n and eager["ccnt"].tolist() == [kept, kept] and eager["mcnt"].tolist() == [n, n]
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            frame(replayed, side.cuda_stream)
    cur.wait_stream(side)
    other = to_dev(synthetic(5000, np.arange(5000) % 3 == 0, np.random.default_rng(1)), torch)
    for k in range(2):
        for key in ("comp", "mark"):
            replayed[key].fill_(int(POISON.view(np.int32)))
        for key in ("rend", "ccnt", "mcnt", "img"):
            replayed[key].zero_()
        gr.replay()
        torch.cuda.synchronize()
        for key in eager:
            assert torch.equal(eager[key].view(torch.int32) if eager[key].dtype == torch.float32 else eager[key],
                               replayed[key].view(torch.int32) if replayed[key].dtype == torch.float32 else replayed[key]), (k, key)
        if k == 0:                                  # an eager call on the same ctx (and scratch) between the replays
            d_pts, d_cnt = poisoned(5000, torch), torch.zeros(2, dtype=torch.int64, device=dev)
            tr.cloud_dev(other.data_ptr(), 5000, d_pts.data_ptr(), 5000, d_cnt.data_ptr(), mode=abi.TRT_CLOUD_COMPACT, stream=cur.cuda_stream)
            torch.cuda.synchronize()
            want, counts = ct.cloud(as_u32(other).view(np.float32), ct.COMPACT, np.full((5000, 8), POISON, np.uint32))
            assert tuple(d_cnt.tolist()) == counts
            np.testing.assert_array_equal(as_u32(d_pts)[:5000], want)
    # a ctx whose scratch was never sized: refused inside a capture, not allocated
    t2 = Tracer(0)
    try:
        gx = torch.cuda.CUDAGraph()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            with torch.cuda.graph(gx, stream=side):
                with pytest.raises(TrtError) as e:
                    t2.cloud_dev(eager["rend"].data_ptr(), n, replayed["comp"].data_ptr(), n, replayed["ccnt"].data_ptr(),
                                 mode=abi.TRT_CLOUD_COMPACT, stream=side.cuda_stream)
                assert e.value.code == abi.TRT_E_INVALID and "captured" in str(e.value)
                torch.zeros(1, device=dev)   # keep the capture non-empty
        cur.wait_stream(side)
    finally:
        t2.close()


def test_errors_change_nothing(tr):
    """Every TRT_E_INVALID of include/trt.h; after each the points and the counts hold what they held."""
    import torch
    from toroidal_ray_tracing_amd.tracer import TrtError
    s = torch.cuda.current_stream().cuda_stream
    n = 2000
    rng = np.random.default_rng(3)
    rec = synthetic(n, rng.uniform(size=n) >= 0.5, rng)
    d_rec = to_dev(rec, torch)
    d_pts = poisoned(n, torch)
    d_cnt = torch.tensor([11, 22], dtype=torch.int64, device="cuda:0")
    R, P, Cn = d_rec.data_ptr(), d_pts.data_ptr(), d_cnt.data_ptr()
    K = abi.TRT_CLOUD_COMPACT
    bad = {
        "NULL capture": (0, n, P, n, Cn, K),
        "NULL points": (R, n, 0, n, Cn, K),
        "NULL counts": (R, n, P, n, 0, K),
        "NULL counts, no records": (0, 0, 0, 0, 0, K),
        "mode 3": (R, n, P, n, Cn, 3),
        "mode -1": (R, n, P, n, Cn, -1),
        "capture not 16-byte aligned": (R + 4, n - 1, P, n, Cn, K),
        "points not 16-byte aligned": (R, n, P + 8, n - 1, Cn, K),
        "n_records above 2^32-1": (R, 1 << 32, P, n, Cn, K),
        "capacity above 2^32-1": (R, n, P, 1 << 32, Cn, K),
        "points inside the capture": (R, n, R + 64, n // 4, Cn, K),
        "capture inside the points": (P + 32 * 8, 8, P, n, Cn, K),
    }
    for what, (r, nr, p, cap, c, mode) in bad.items():
        for append in (False, True):
            with pytest.raises(TrtError) as e:
                tr.cloud_dev(r, nr, p, cap, c, mode=mode, append=append, stream=s)
            assert e.value.code == abi.TRT_E_INVALID, what
    L = lib.load()
    assert L.trt_cloud_dev(None, C.c_void_p(R), n, K, 0, C.c_void_p(P), n, C.c_void_p(Cn), None) == abi.TRT_E_INVALID   # NULL ctx
    torch.cuda.synchronize()
    assert d_cnt.tolist() == [11, 22] and (as_u32(d_pts) == POISON).all()
    assert np.array_equal(as_u32(d_rec), rec.view(np.uint32))
    # … and the same arguments, valid, still work
    tr.cloud_dev(R, n, P, n, Cn, mode=K, append=False, stream=s)
    torch.cuda.synchronize()
    want, counts = ct.cloud(rec, ct.COMPACT, np.full((n, 8), POISON, np.uint32))
    assert tuple(d_cnt.tolist()) == counts
    np.testing.assert_array_equal(as_u32(d_pts)[:n], want)
