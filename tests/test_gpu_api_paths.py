"""The host-side idioms the entry points of csrc/trt_api.hip share: the staging of the ray streams (trt_trace,
trt_occluded), and the bracket of a counted launch (zero the query counters, launch, record the event trt_get_stats
waits for — never into a capture).  Every comparison is equality, against the *_dev form of the same call or against
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
