"""The host-side idioms the entry points of csrc/trt_api.hip share: the staging of the ray streams (trt_trace,
trt_occluded), that of six output ray streams (trt_camera_rays, trt_fan_rays), and the bracket of a counted launch
(zero the query counters, launch, record the event trt_get_stats waits for — never into a capture).  Every comparison is equality, against the *_dev form of the same call or against
the same call repeated; the single-torus scene throughout."""
import numpy as np
import pytest

from conftest import seeded_rays
from test_gpu_parity import assert_hits_equal
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu


@pytest.fixture()
def tr():
    """A ctx of the test's own: what its scratch holds is part of what is tested."""
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def upload(o, d):
    import torch
    soa = [torch.from_numpy(np.ascontiguousarray(a[:, k])).to("cuda:0") for a in (o, d) for k in range(3)]
    return soa, [a.data_ptr() for a in soa]


def hit_buffers(n):
    import torch
    out = {k: torch.empty(max(n, 1), dtype=torch.int32 if k == "id" else torch.float32, device="cuda:0") for k in abi.HIT_FIELDS}
    return out, {k: v.data_ptr() for k, v in out.items()}


def trace_dev(tr, sc, o, d):
    import torch
    keep, ptrs = upload(o, d)
    out, hp = hit_buffers(len(o))
    tr.trace_dev(sc, ptrs, len(o), hp)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy()[:len(o)] for k, v in out.items()}


def occluded_dev(tr, sc, o, d):
    import torch
    n = len(o)
    keep, ptrs = upload(o, d) if n else (None, [0] * 6)
    flag = torch.full((max(n, 1),), 0xA5, dtype=torch.uint8, device="cuda:0")
    tr.occluded_dev(sc, ptrs, n, flag_ptr=flag.data_ptr())
    torch.cuda.synchronize()
    got = flag.cpu().numpy()
    assert (got[n:] == 0xA5).all() and (got[:n] <= 1).all()
    return got[:n].astype(bool)


def test_ray_staging_shared_by_trace_and_occluded(tr):
    """One ctx, the host forms in turn: trace n = 64 (the ray staging is allocated), occluded n = 1000 (it grows, and
    the staging of trace's hit streams becomes that of the flags), trace n = 65 (reused, larger than needed), occluded
    n = 0 (nothing staged).  Each equals the *_dev form on the same rays."""
    sc = camera.single_torus_scene()
    for query, n in (("trace", 64), ("occluded", 1000), ("trace", 65), ("occluded", 0)):
        o, d = seeded_rays(max(n, 1), 500 + n)
        o, d = o[:n], d[:n]
        if query == "trace":
            got, want = tr.trace(sc, o, d), trace_dev(tr, sc, o, d)
            assert_hits_equal(got, want, f"trace n={n}")
            assert (want["id"] >= 0).any() and (want["id"] < 0).any()
        else:
            got, want = tr.occluded(sc, o, d), occluded_dev(tr, sc, o, d)
            assert got.shape == (n,) and np.array_equal(got, want)
            assert n == 0 or (want.any() and not want.all())


def fan_rays_dev(tr, at, dirs, frame):
    """trt_fan_rays_dev on the host arrays `at`, into sentinel-filled padded streams: (o, d) of shape (samples * n, 3)."""
    import torch
    from camera_support import ray_buffers, read_rays
    n = len(at["px"])
    keep = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in at.items()}
    bufs = ray_buffers(len(dirs) * n)
    tr.fan_rays_dev({k: v.data_ptr() for k, v in keep.items()}, n, dirs, [b.data_ptr() for b in bufs], frame=frame)
    torch.cuda.synchronize()
    return read_rays(bufs, len(dirs) * n)


def test_ray_out_staging_shared_by_camera_rays_and_fan_rays(tr):
    """One ctx, the host forms that write six ray streams in turn: camera_rays of a band of a 52x36 toroidal frame with 3
    samples (the output staging is allocated, the per-sample tables are uploaded), fan_rays of 100 points x 4 directions
    about the normal with an id stream (P and N through the ray-stream staging, id beside them; the output staging is
    reused), camera_rays of a 20x12 pinhole frame (reused, larger than needed), fan_rays in world axes without normals
    (three input streams).  Each equals the *_dev form on the same inputs bit for bit, and the first call repeated at the
    end equals its first result."""
    from camera_support import CAMERAS, rays_dev, u32
    same = lambda got, want: all(a.shape == b.shape and np.array_equal(u32(a), u32(b)) for a, b in zip(got, want))
    rng = np.random.default_rng(77)
    n, K = 100, 4
    P = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    N = rng.normal(size=(n, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    ids = np.where(rng.random(n) < 0.3, -1, 0).astype(np.int32)
    dead = ids < 0
    assert dead.any() and not dead.all()
    at = {"px": P[:, 0], "py": P[:, 1], "pz": P[:, 2], "nx": N[:, 0], "ny": N[:, 1], "nz": N[:, 2], "id": ids}
    dirs = rng.normal(size=(K, 3)).astype(np.float32)
    off = np.float32([[0.125, 0.25], [-0.375, 0.03125], [0.5, -0.5]])

    g, pc, cam = CAMERAS["toroidal_theta"](52, 36)
    big = dict(camera=cam, samples=3, offsets=off, rows=(5, 31))
    first = tr.camera_rays(g, pc, 52, 36, **big)
    assert first[0].shape == (3 * 26 * 52, 3)
    assert same(first, rays_dev(tr, g, pc, 52, 36, cam, samples=3, offsets=off, rows=(5, 31)))
    # the samples differ: the offsets arrived
    assert not same(first, [a.reshape(3, -1, 3)[[1, 2, 0]].reshape(-1, 3) for a in first])

    o, d = local = tr.fan_rays(at, dirs, frame=abi.TRT_FAN_LOCAL)
    assert same(local, fan_rays_dev(tr, at, dirs, abi.TRT_FAN_LOCAL))
    assert np.array_equal(o, np.tile(P, (K, 1)))
    d = d.reshape(K, n, 3)
    assert (d[:, dead] == 0.0).all() and (np.abs(d[:, ~dead]).sum(axis=2) > 0.0).all()         # the id stream arrived

    g2, pc2, cam2 = CAMERAS["pinhole"](20, 12)
    small = tr.camera_rays(g2, pc2, 20, 12, camera=cam2)
    assert small[0].shape == (240, 3) and same(small, rays_dev(tr, g2, pc2, 20, 12, cam2))

    points = {k: at[k] for k in ("px", "py", "pz")}
    world = tr.fan_rays(points, dirs, frame=abi.TRT_FAN_WORLD)
    assert same(world, fan_rays_dev(tr, points, dirs, abi.TRT_FAN_WORLD))
    assert np.array_equal(world[0], np.tile(P, (K, 1))) and np.array_equal(world[1], np.repeat(dirs, n, axis=0))

    assert same(tr.camera_rays(g, pc, 52, 36, **big), first)


def test_counted_trace_in_a_graph(tr):
    """trt_trace_dev with the statistics on, captured and replayed: the counters of the replay are those of the eager
    call, trt_get_stats returns them without error, and the next counted eager call counts as usual.
    (Until the counted launches shared one bracket, trt_trace_dev alone recorded its statistics event into the capture,
    where the event belongs to the graph and trt_get_stats may not wait for it.)"""
    import torch
    n = 257   # one ray past a block
    sc = camera.single_torus_scene()
    o, d = seeded_rays(n, 61)
    keep, ptrs = upload(o, d)
    out, hp = hit_buffers(n)
    tr.enable_stats(True)
    tr.trace_dev(sc, ptrs, n, hp)
    torch.cuda.synchronize()
    S = tr.stats()
    print("eager:", S)
    assert S["pixels"] == n and S["primary_tests"] == n and S["shadow_tests"] == 0 and 0 < S["solved_tests"] <= n
    eager_id = out["id"].cpu().numpy().copy()
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            tr.trace_dev(sc, ptrs, n, hp, stream=side.cuda_stream)
    cur.wait_stream(side)
    out["id"].fill_(-7)
    gr.replay()
    torch.cuda.synchronize()
    got = tr.stats()
    print("replay:", got)
    assert got == S
    assert np.array_equal(out["id"].cpu().numpy(), eager_id)
    flag = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    tr.occluded_dev(sc, ptrs, n, flag_ptr=flag.data_ptr())
    torch.cuda.synchronize()
    st = tr.stats()
    print("occluded:", st)
    assert st["pixels"] == 257 and st["shadow_tests"] == n and st["primary_tests"] == 0 and st["bounce_tests"] == 0
    assert int(flag.sum()) == int((eager_id >= 0).sum())


def test_render_bracket(tr):
    """A counted frame, an uncounted one, a counted one (listed variant, 33x9: a ragged tile column and row): the counted
    frames count the same, and the uncounted frame leaves the first frame's numbers to be read."""
    W, H = 33, 9
    sc, g, pc = camera.single_torus_scene(), camera.baseline_camera(W, H), camera.baseline_push(3)
    tr.set_render_variant("listed")
    tr.enable_stats(True)
    first_rgba, _ = tr.render(sc, g, pc, W, H)
    first = tr.stats()
    print("first:", first)
    assert first["pixels"] == W * H and first["primary_tests"] == W * H
    tr.enable_stats(False)
    tr.render(sc, g, pc, W, H)
    assert tr.stats() == first
    tr.enable_stats(True)
    rgba, _ = tr.render(sc, g, pc, W, H)
    assert tr.stats() == first
    assert np.array_equal(rgba, first_rgba)
