"""The enclosure cull of the kernels against a reference that has none: oracle.render / oracle.shade
with set_enclosure_cull(0) — every torus tested by every query.  The other GPU tests compare with the oracle as it
stands, which implements the library's rule and would share its mistakes.

The frames are those of tests/cull_cases.py, where the rule once changed the image: an eye within tMin of the enclosing
tube, the toroidal camera's origin circle within tMin of it, bounces off a torus that cuts through the nest, caller rays
64 long — and the control on which the cull must go on working.  tests/test_oracle.py and tests/test_shade_oracle_cpu.py
check on the CPU that the oracle with the cull equals the oracle without on each of them, so a failure here points at the
kernels or the host's masks.

Bars (check_render, tests/test_gpu_parity.py): first-hit records bit for bit, colours at COLOR_RTOL / COLOR_ATOL, the
query counts and `pixels` equal.  Every frame is at most 64x64.
"""
import functools

import numpy as np
import pytest

import cull_cases
from toroidal_ray_tracing_amd import abi, camera

pytestmark = pytest.mark.gpu

GEOM = ("t", "px", "py", "pz", "nx", "ny", "nz")
COLOR_RTOL, COLOR_ATOL = 1e-5, 1e-6   # the project's bars on colours against the oracle (tests/test_gpu_parity.py)
QUERY_KEYS = ("primary_tests", "bounce_tests", "shadow_tests", "pixels")
SOLVERS = [abi.TRT_SOLVE_F32, abi.TRT_SOLVE_F64]
SOLVER_IDS = ["f32", "f64"]
VARIANTS = ["static", "persistent", "listed"]
RENDER_FRAMES = ["near_2.5006", "near_2.5008", "near_2.5012", "seam_0.5", "seam_8.0", "tilted_seam", "control", "toroidal_near"]


@pytest.fixture(scope="module")
def tr():
    from toroidal_ray_tracing_amd.tracer import Tracer
    t = Tracer(0)
    yield t
    t.close()


def q(stats):
    return {k: stats[k] for k in QUERY_KEYS}


FRAMES = functools.lru_cache(maxsize=None)(cull_cases.frames)


@functools.lru_cache(maxsize=None)
def _reference(name, precision):
    from oracle import oracle
    return cull_cases.render_without_cull(oracle, FRAMES()[name], precision, nthreads=8, want_rendered=True)


def reference(name, precision):
    """(rgba, hits, RenderedData, stats) of frame `name` from the oracle without the cull; computed once, never written to."""
    return _reference(name, precision)


def assert_frame(rgba, hits, st, want, what):
    wr, wh, _, wst = want
    np.testing.assert_array_equal(hits["id"], wh["id"], err_msg=f"{what} id")
    for k in GEOM:
        np.testing.assert_array_equal(hits[k].view(np.uint32), wh[k].view(np.uint32), err_msg=f"{what} {k} bits")
    np.testing.assert_allclose(rgba, wr, rtol=COLOR_RTOL, atol=COLOR_ATOL, err_msg=what)
    if st is not None:
        assert q(st) == q(wst), what


def render_frame(tr, name, variant, precision):
    sc, g, pc, W, H, cam = FRAMES()[name]
    tr.set_render_variant(variant)
    tr.set_solver(precision)
    tr.enable_stats(True)
    try:
        rgba, hits = tr.render(sc, g, pc, W, H, cam)
        return rgba, hits, tr.stats()
    finally:
        tr.enable_stats(False)
        tr.set_solver(abi.TRT_SOLVE_F32)
        tr.set_render_variant("listed")


@pytest.mark.parametrize("precision", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", RENDER_FRAMES)
def test_render_equals_testing_every_torus(tr, name, variant, precision):
    """trt_render, every kernel variant, both precisions, on every frame of tests/cull_cases.py."""
    rgba, hits, st = render_frame(tr, name, variant, precision)
    assert_frame(rgba, hits, st, reference(name, precision), f"{name} {variant}")


@pytest.mark.parametrize("variant", ["static", "listed"])
def test_render_durand_kerner_on_the_seam(tr, variant):
    """An alternative root solver runs the same masks: Durand–Kerner in FP64 on the seam frame."""
    rgba, hits, st = render_frame(tr, "seam_8.0", variant, abi.TRT_SOLVE_DK_F64)
    assert_frame(rgba, hits, st, reference("seam_8.0", abi.TRT_SOLVE_DK_F64), f"seam_8.0 dk64 {variant}")


@pytest.mark.parametrize("precision", SOLVERS, ids=SOLVER_IDS)
def test_control_keeps_its_cull(tr, oracle, precision):
    """The cull still does its job: on the control — the intruder far from the nest — the static variant, which traces every
    pixel, executes exactly the tests the culling oracle executes, and fewer than queries x tori."""
    sc, g, pc, W, H, cam = FRAMES()["control"]
    _, _, st = render_frame(tr, "control", "static", precision)
    wst = oracle.render(sc, g, pc, W, H, cam, precision=precision, nthreads=8, want_hits=False)[3]
    every = sum(st[k] for k in ("primary_tests", "bounce_tests", "shadow_tests"))
    assert q(st) == q(wst) == q(reference("control", precision)[3])
    assert st["traced_tests"] == wst["traced_tests"] < every == reference("control", precision)[3]["traced_tests"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_rendered_data_on_the_seam(tr, variant):
    """RenderedData (trt_render_dev, want_rendered) of a seam frame: positions and rays bit for bit, colours at the bars."""
    import torch
    sc, g, pc, W, H, cam = FRAMES()["seam_0.5"]
    rend = torch.full((W * H, 16), -3.0, device="cuda:0")
    rgba = torch.full((H, W, 4), -3.0, device="cuda:0")
    tr.set_render_variant(variant)
    try:
        tr.render_dev(sc, g, pc, W, H, rgba.data_ptr(), camera=cam, rendered_ptr=rend.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        tr.set_render_variant("listed")
    wr, _, wrend, _ = reference("seam_0.5", abi.TRT_SOLVE_F32)
    got = rend.cpu().numpy()
    geo = [0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14, 15]
    np.testing.assert_array_equal(got[:, geo].view(np.uint32), wrend[:, geo].view(np.uint32))
    np.testing.assert_allclose(got[:, 4:8], wrend[:, 4:8], rtol=COLOR_RTOL, atol=COLOR_ATOL)
    np.testing.assert_allclose(rgba.cpu().numpy(), wr, rtol=COLOR_RTOL, atol=COLOR_ATOL)


@pytest.mark.parametrize("scene", ["nest", "seam"])
@pytest.mark.parametrize("precision", SOLVERS, ids=SOLVER_IDS)
def test_batch_takes_each_frames_own_mask(tr, oracle, scene, precision):
    """trt_render_batch_dev: four views in one batch — the eye 0.0006 outside the enclosing tube (nothing certified), 0.01
    outside it (the shell culled), and the two seam cameras — of the two-shell nest, where the camera's share of the
    mask differs from frame to frame and one taken from the wrong frame changes every pixel, and of the seam scene.  (Batches run the listed variant.)"""
    import torch
    W = H = 64
    sc = cull_cases.scene(cull_cases.NEST if scene == "nest" else cull_cases.SEAM)
    views = [(camera.globals_for((2.5006, 0.0, 0.0), (2.0, 0.0, 0.0), W, H), abi.make_push(max_depth=4)),
             (camera.globals_for((2.51, 0.0, 0.0), (2.0, 0.0, 0.0), W, H), abi.make_push(max_depth=4)),
             (camera.globals_for(cull_cases.SEAM_EYE, cull_cases.SEAM_AT, W, H, fov_deg=0.5), abi.make_push(max_depth=6)),
             (camera.globals_for(cull_cases.SEAM_EYE, cull_cases.SEAM_AT, W, H, fov_deg=8.0), abi.make_push(max_depth=6))]
    want = [cull_cases.render_without_cull(oracle, (sc, g, pc, W, H, 0), precision, nthreads=8) for g, pc in views]
    keys = GEOM + ("id",)
    outs = []
    for _ in views:
        h = {k: torch.full((W * H,), -5.0, device="cuda:0") for k in GEOM}
        h["id"] = torch.full((W * H,), -5, dtype=torch.int32, device="cuda:0")
        outs.append((torch.full((H, W, 4), -5.0, device="cuda:0"), h))
    fl = [(g, pc, o[0].data_ptr(), {k: o[1][k].data_ptr() for k in keys}) for (g, pc), o in zip(views, outs)]
    tr.set_solver(precision)
    tr.enable_stats(True)
    try:
        tr.render_batch_dev(sc, fl, W, H, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        st = tr.stats()
    finally:
        tr.enable_stats(False)
        tr.set_solver(abi.TRT_SOLVE_F32)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert_frame(o[0].cpu().numpy(), {k: o[1][k].cpu().numpy() for k in keys}, None, w, f"{scene} frame {i}")
    assert q(st) == {k: sum(w[3][k] for w in want) for k in QUERY_KEYS}


def test_list_reuse_keeps_no_stale_mask():
    """One context with the tile lists reused between frames (trt_set_list_reuse(1)): the eye 0.01 outside the enclosing tube,
    then 0.0006 outside it — another view: the lists are classified anew and the second frame carries its own, empty mask;
    then that frame three more times — a scene of two tori classifies the first two frames of a view and reuses the lists
    from the third on.  Each frame equals the oracle without the cull."""
    from toroidal_ray_tracing_amd.tracer import Tracer
    with Tracer(0) as t:
        t.set_list_reuse(True)
        t.set_render_variant("listed")
        before = t.list_reuse()
        for i, name in enumerate(["near_2.51"] + ["near_2.5006"] * 4):
            sc, g, pc, W, H, cam = FRAMES()[name]
            rgba, hits = t.render(sc, g, pc, W, H, cam)
            assert_frame(rgba, hits, None, reference(name, abi.TRT_SOLVE_F32), f"frame {i} ({name})")
        after = t.list_reuse()
    assert after["classified"] - before["classified"] >= 2 and after["reused"] - before["reused"] >= 1


def _upload(o, d):
    import torch
    soa = [torch.from_numpy(np.ascontiguousarray(a[:, k])).to("cuda:0") for a in (o, d) for k in range(3)]
    return soa, [a.data_ptr() for a in soa]


@pytest.mark.parametrize("precision", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("samples", [1, 2])
@pytest.mark.parametrize("scale", [1.0, 64.0])
def test_shade_dev_on_the_seam(tr, oracle, scale, samples, precision):
    """trt_shade_dev on the primary rays of the seam frame (fov 8°), directions multiplied by 1 and by 64 — a direction 64
    long drops a tube's crossing within 0.064 of a bounce —, one sample per output and two (output i averages rays i and
    n_out + i), against oracle.shade without the cull."""
    import torch
    fr = FRAMES()["seam_8.0"]
    sc, _, pc = fr[:3]
    o, d = cull_cases.frame_rays(oracle, fr)
    d = d * np.float32(scale)
    n, n_out = len(o), len(o) // samples
    want, wst = cull_cases.shade_without_cull(oracle, sc, o, d, pc, samples=samples, precision=precision, nthreads=8)
    keep, ptrs = _upload(o, d)
    out = torch.full((n_out, 4), -7.25, device="cuda:0")
    tr.set_solver(precision)
    tr.enable_stats(True)
    try:
        tr.shade_dev(sc, ptrs, n, pc, out.data_ptr(), samples=samples, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        st = tr.stats()
    finally:
        tr.enable_stats(False)
        tr.set_solver(abi.TRT_SOLVE_F32)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=COLOR_RTOL, atol=COLOR_ATOL)
    assert q(st) == q(wst)


@pytest.mark.parametrize("precision", SOLVERS, ids=SOLVER_IDS)
def test_shade_camera_next_to_the_tube(tr, oracle, precision):
    """trt_shade_camera, two samples per pixel with sub-pixel offsets, from the eye 0.0006 outside the enclosing tube: the
    frame equals oracle.shade without the cull on the rays trt_camera_rays gives for the same camera."""
    sc, g, pc, W, H, cam = FRAMES()["near_2.5006"]
    offsets = [(0.25, -0.25), (-0.25, 0.25)]
    tr.set_solver(precision)
    try:
        o, d = tr.camera_rays(g, pc, W, H, cam, samples=2, offsets=offsets)
        got = tr.shade_camera(sc, g, pc, W, H, cam, samples=2, offsets=offsets)
    finally:
        tr.set_solver(abi.TRT_SOLVE_F32)
    want, _ = cull_cases.shade_without_cull(oracle, sc, o, d, pc, samples=2, precision=precision, nthreads=8)
    np.testing.assert_allclose(got.reshape(-1, 4), want, rtol=COLOR_RTOL, atol=COLOR_ATOL)


@pytest.mark.parametrize("precision", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("max_depth", [0, 5])
@pytest.mark.parametrize("scene", ["nested8", "seam"])
def test_shade_dev_on_rays_of_no_frame(tr, oracle, scene, max_depth, precision):
    """trt_shade_dev on 6000 seeded rays that are no camera's — origins all over a box around the scene, inside tubes
    included, directions of lengths 1/4 to 64 (powers of two), three samples per output — against oracle.shade without the
    cull: colours at the bars, query counts equal; maxDepth 0 runs the loop once (rgen:78-79)."""
    import torch
    from conftest import seeded_rays
    sc = camera.nested_tori_scene() if scene == "nested8" else cull_cases.scene(cull_cases.SEAM)
    n, samples = 6000, 3
    o, d = seeded_rays(n, 31 + max_depth, box=3.5, reach=2.6)
    d = d * np.exp2(np.random.default_rng(5).integers(-2, 7, (n, 1))).astype(np.float32)
    pc = abi.make_push(max_depth=max_depth)
    want, wst = cull_cases.shade_without_cull(oracle, sc, o, d, pc, samples=samples, precision=precision, nthreads=8)
    keep, ptrs = _upload(o, d)
    out = torch.full((n // samples, 4), -7.25, device="cuda:0")
    tr.set_solver(precision)
    tr.enable_stats(True)
    try:
        tr.shade_dev(sc, ptrs, n, pc, out.data_ptr(), samples=samples, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        st = tr.stats()
    finally:
        tr.enable_stats(False)
        tr.set_solver(abi.TRT_SOLVE_F32)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=COLOR_RTOL, atol=COLOR_ATOL)
    assert q(st) == q(wst)
    assert max_depth != 0 or st["bounce_tests"] == 0
