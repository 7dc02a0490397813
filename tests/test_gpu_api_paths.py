"""The host-side idioms the entry points of csrc/trt_api.hip share: the staging of the ray streams (trt_trace,
trt_occluded), that of six output ray streams (trt_camera_rays, trt_fan_rays), the host bodies of the shade forms and of
the bounded ray queries, and the bracket of a counted launch
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


def _mean_of_misses(pc, samples):
    """The colour of an output whose `samples` rays all miss, by the kernels' arithmetic: c_0 = clearColor * 0.8, plain FP32
    adds in order, one division unless samples == 1."""
    f32 = np.float32
    m = np.asarray(pc.clearColor[:3], f32) * f32(0.8)
    acc = m.copy()
    for _ in range(samples - 1):
        acc = (acc + m).astype(f32)
    return acc if samples == 1 else (acc / f32(samples)).astype(f32)


def _hits_and_misses(rgba, pc, samples):
    """Whether the image (.., 4) holds outputs of the miss colour and others of more than a few colours, alpha 1 in all."""
    from camera_support import u32
    px = rgba.reshape(-1, 4)
    missed = (px[:, :3] == _mean_of_misses(pc, samples)).all(axis=1)
    return missed.any() and not missed.all() and len(np.unique(u32(px), axis=0)) > 4 and (px[:, 3] == 1.0).all()


def _camera_dev(call, W, H, rows):
    """A trt_shade*_camera_dev call (`call(image address)`) into a sentinel-filled full frame: (H, W, 4), after checking
    that the rows outside the band kept the sentinel."""
    import torch
    from camera_support import image, read_image
    buf = image(W, H)
    call(buf.data_ptr())
    torch.cuda.synchronize()
    return read_image(buf, W, H, rows)


def test_shade_and_bounded_query_staging_shared_by_their_forms(tr):
    """One ctx, the host forms that share a staging path in turn, each equal in bits to its *_dev form on the same inputs.
    Stream forms of shade: shade n = 300 (ray and image staging allocated), shade_lit 900 rays of 3 samples (the rays
    grow, the image is reused), shade_through n = 64 (both reused, larger than needed), shade_refract n = 0 (nothing
    staged, an empty result), then shade n = 300 again, which equals its first result.  Bounded queries with a bound per
    ray: glow n = 100 (the bound staging allocated), transmittance n = 1000 (it grows), chords n = 65, occluded n = 0,
    then glow n = 100 without bounds.  Camera forms on rows (3, 9) of a 13x11 frame with 2 samples — ragged tiles on both
    edges, a band offset that is not zero: the band equals the *_dev form's, the rows outside it are 0 in the host form
    and untouched in the *_dev form's buffer.  Every result that is not empty holds hits and misses."""
    import crossings_truth as ct
    import lights_truth as lt
    import media_truth as mt
    import refract_truth as rt
    import through_truth as tt
    import test_gpu_lights as lights
    import test_gpu_media as media
    import test_gpu_refract as refract
    import test_gpu_through as through
    from camera_support import CAMERAS, scene_for, u32
    from test_gpu_shade import shade_dev
    same = lambda got, want: got.shape == want.shape and got.dtype == np.float32 and np.array_equal(u32(got), u32(want))

    # -- the four stream forms of shade ---------------------------------------------------------------------------
    single, nest3, rings2 = ct.ray_set("single"), ct.ray_set("nest3"), ct.ray_set("rings2")
    sc, pc = camera.single_torus_scene(), camera.baseline_push(5)
    o, d = single["o"][:300], single["d"][:300]
    first = tr.shade(sc, o, d, pc)
    assert same(first, shade_dev(tr, sc, o, d, pc)) and first.shape == (300, 4) and _hits_and_misses(first, pc, 1)

    lsc, _, _, lpc, llights, K = lt.case_scene("single_two_hard")
    llights = lt.abi_lights(llights)
    jitter = np.float32([0.001, -0.001, 0.0005])   # sample s of output i: ray i with its direction moved by s * jitter
    o3 = np.tile(o, (3, 1))
    d3 = np.concatenate([d + np.float32(s) * jitter for s in range(3)]).astype(np.float32)
    got = tr.shade_lit(lsc, o3, d3, lpc, samples=3, lights=llights, shadow_samples=K)
    assert same(got, lights.lit_dev(tr, lsc, o3, d3, lpc, llights, K, samples=3)) and got.shape == (300, 4)
    assert _hits_and_misses(got, lpc, 3)

    tsc, _, _, _, depth, _ = tt.case_scene("nest3_all_through")
    tpc = camera.baseline_push(depth)
    o, d = nest3["o"][:64], nest3["d"][:64]
    got = tr.shade_through(tsc, o, d, tpc)
    assert same(got, through.through_dev(tr, tsc, o, d, tpc)) and got.shape == (64, 4) and _hits_and_misses(got, tpc, 1)

    rsc, _, _, rpc = rt.case_scene("single_glass")
    z = np.zeros((0, 3), np.float32)
    assert tr.shade_refract(rsc, z, z, rpc).shape == (0, 4) and refract.refract_dev(tr, rsc, z, z, rpc).shape == (0, 4)

    assert same(tr.shade(sc, single["o"][:300], single["d"][:300], pc), first)

    # -- the four bounded queries, a bound per ray ----------------------------------------------------------------
    w = dict(tmin=float(np.float32(ct.TMIN)), tmax=ct.TMAX)
    bound = np.random.default_rng(20).uniform(0.25, 3.0, 1000).astype(np.float32)

    gsc, gm = media.scene_of("rings2"), mt.MEDIA["rings2"]
    o, d = rings2["o"][:100], rings2["d"][:100]
    got = tr.glow(gsc, o, d, gm, tmax_per_ray=bound[:100], **w)
    bounded = media.glow_dev(tr, gsc, o, d, gm, bound=bound[:100], **w)
    assert same(got, bounded) and got.shape == (100, 4)
    clear = (got == np.float32([0, 0, 0, 1])).all(axis=1)
    assert clear.any() and not clear.all() and len(np.unique(u32(got), axis=0)) > 8

    xsc = through.scene_of("nest3", through.ALPHAS["nest3"])
    o, d = nest3["o"][:1000], nest3["d"][:1000]
    got = tr.transmittance(xsc, o, d, tmax_per_ray=bound, **w)
    assert same(got, through.transmittance_dev(tr, xsc, o, d, bound=bound, **w)) and got.shape == (1000,)
    assert (got == 1.0).any() and (got < 1.0).any() and len(np.unique(got)) > 4

    o, d = rings2["o"][:65], rings2["d"][:65]
    got = tr.chords(gsc, o, d, tmax_per_ray=bound[:65], **w)
    assert same(got, media.chords_dev(tr, gsc, o, d, bound=bound[:65], **w)) and got.shape == (2, 65)
    assert (got == 0.0).any() and len(np.unique(u32(got))) > 8

    assert tr.occluded(sc, z, z, tmax_per_ray=np.zeros(0, np.float32)).shape == (0,)

    o, d = rings2["o"][:100], rings2["d"][:100]
    got = tr.glow(gsc, o, d, gm, **w)
    assert same(got, media.glow_dev(tr, gsc, o, d, gm, **w)) and not same(got, bounded)

    # -- the three camera forms ------------------------------------------------------------------------------------
    W, H, rows, off = 13, 11, (3, 9), np.float32([[0.25, -0.125], [-0.375, 0.5]])
    g, cpc, cam = CAMERAS["pinhole"](W, H)
    kw = dict(camera=cam, samples=2, offsets=off, rows=rows)
    fsc, _, fpc, _, flights = lights.lit_frame("pinhole")
    rfsc, _, rfpc, _ = refract.glass_frame("pinhole")
    csc = scene_for(cam)
    forms = (
        (cpc, lambda: tr.shade_camera(csc, g, cpc, W, H, **kw), lambda p: tr.shade_camera_dev(csc, g, cpc, W, H, p, **kw)),
        (fpc, lambda: tr.shade_lit_camera(fsc, g, fpc, W, H, lights=flights, shadow_samples=8, **kw),
         lambda p: tr.shade_lit_camera_dev(fsc, g, fpc, W, H, p, lights=flights, shadow_samples=8, **kw)),
        (rfpc, lambda: tr.shade_refract_camera(rfsc, g, rfpc, W, H, **kw), lambda p: tr.shade_refract_camera_dev(rfsc, g, rfpc, W, H, p, **kw)),
    )
    for fpc_, host, dev in forms:
        got, want = host(), _camera_dev(dev, W, H, rows)
        assert got.shape == (H, W, 4) and same(got[rows[0]:rows[1]], want[rows[0]:rows[1]])
        assert (got[:rows[0]] == 0.0).all() and (got[rows[1]:] == 0.0).all()
        assert _hits_and_misses(got[rows[0]:rows[1]], fpc_, 2)
