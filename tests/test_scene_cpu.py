"""trt_shade_scene*: the FP64 truth of the composed rule (scene_truth) against the truths of its three ingredients, the
quality of the mixed cases, and the binding's prototypes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import lights_truth
import refract_truth
import scene_truth
import textured_truth
import through_truth


# ---------------------------------------------------------------------------------------------------------------------
# the composed truth with two of the three features unused is the third's truth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(refract_truth.cases()))
def test_truth_reproduces_refract(name):
    c = refract_truth.case(name)
    sc, tori, axes, pc = refract_truth.case_scene(name)
    rgb, robust = scene_truth.shade_scene(c["o"], c["d"], tori, refract_truth.material_dicts(sc), [], through_truth.push_dict(pc), axes=axes)
    assert np.max(np.abs(rgb - c["rgb"])) <= 1e-12
    assert np.array_equal(robust, c["robust"])


@pytest.mark.parametrize("name", sorted(lights_truth.cases()))
def test_truth_reproduces_lights(name):
    c = lights_truth.case(name)
    sc, tori, axes, pc, lights, K = lights_truth.case_scene(name)
    rgb, robust = scene_truth.shade_scene(c["o"], c["d"], tori, through_truth.material_dicts(sc), [], through_truth.push_dict(pc),
                                          lights, K, c["disc"], axes=axes)
    assert np.max(np.abs(rgb - c["rgb"])) <= 1e-12
    assert np.array_equal(robust, c["robust"])


@pytest.mark.parametrize("name", sorted(textured_truth.cases()))
def test_truth_reproduces_textured(name):
    c = textured_truth.case(name)
    rgb, robust = scene_truth.shade_scene(c["o"], c["d"], c["tori"], c["mats"], c["textures"], through_truth.push_dict(c["pc"]), axes=c["axes"])
    assert np.max(np.abs(rgb - c["rgb"])) <= 1e-12
    assert np.array_equal(robust, c["robust"])


def test_flag_without_glass_changes_nothing():
    """With no glass in use every filter is 0 or 1: the flag changes the truth by nothing at all."""
    c = lights_truth.case("rings2_area_dir_and_hard")
    sc, tori, axes, pc, lights, K = lights_truth.case_scene("rings2_area_dir_and_hard")
    rgb, robust = scene_truth.shade_scene(c["o"], c["d"], tori, through_truth.material_dicts(sc), [], through_truth.push_dict(pc),
                                          lights, K, c["disc"], glass_shadows=True, axes=axes)
    assert np.max(np.abs(rgb - c["rgb"])) <= 1e-12
    assert np.array_equal(robust, c["robust"])


# ---------------------------------------------------------------------------------------------------------------------
# the mixed cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("name", sorted(scene_truth.cases()))
def test_mixed_cases_are_mostly_robust(name, flag):
    c = scene_truth.case(name, flag)
    share = 1.0 - c["robust"].mean()
    print(f"{name} flag={flag}: robust share {c['robust'].mean():.3f}")
    assert len(c["o"]) == 4096
    assert share <= 0.15, f"{name}: {share:.3f} of the rays are not robust"


@pytest.mark.parametrize("name", scene_truth.MULTI_TORUS)
def test_flag_shows_in_the_multi_torus_cases(name):
    off, on = scene_truth.case(name, False), scene_truth.case(name, True)
    moved = np.max(np.abs(on["rgb"] - off["rgb"]), axis=1) > 1e-3
    print(f"{name}: the flag moves {moved.mean():.3f} of the rays")
    assert moved.mean() >= 0.05
    # light only gets through: no channel of any ray gets darker with the flag (all lights and materials are >= 0)
    assert np.all(on["rgb"] >= off["rgb"] - 1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# the binding
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_prototypes_and_flag():
    from toroidal_ray_tracing_amd import abi, lib
    assert abi.TRT_SCENE_GLASS_SHADOWS == 1
    stream = [C.c_void_p, C.POINTER(abi.trt_rays), C.c_uint32, C.POINTER(abi.trt_push), C.POINTER(abi.trt_lights), C.c_uint32,
              C.POINTER(abi.trt_scene), C.c_void_p]
    cam = [C.c_void_p, C.POINTER(abi.trt_globals), C.POINTER(abi.trt_push), C.POINTER(abi.trt_lights), C.c_uint32,
           C.POINTER(abi.trt_scene), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, abi.f32p, C.c_void_p]
    assert lib.SYMBOLS["trt_shade_scene"] == (C.c_int, stream)
    assert lib.SYMBOLS["trt_shade_scene_dev"] == (C.c_int, stream + [C.c_void_p])
    assert lib.SYMBOLS["trt_shade_scene_camera"] == (C.c_int, cam)
    assert lib.SYMBOLS["trt_shade_scene_camera_dev"] == (C.c_int, cam + [C.c_void_p])


def test_header_declares_the_calls():
    import os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trt.h")).read()
    assert "#define TRT_SCENE_GLASS_SHADOWS 1u" in h
    for name in ("trt_shade_scene", "trt_shade_scene_dev", "trt_shade_scene_camera", "trt_shade_scene_camera_dev"):
        assert f"int {name}(trt_ctx* ctx" in h
