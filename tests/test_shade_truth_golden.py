"""The FP64 truth of the shade family against ``tests/golden/shade_truth_cases.npz``: what refract_truth, lights_truth,
textured_truth and scene_truth gave when each had a payload loop of its own (tests/golden/make_shade_truth_golden.py
records the file and says when).  The one loop of shade_truth has to give the same on every run: 5 refract, 4 lights,
4 textured and 4 scene cases with the flag off and on.  No GPU.

The margins are for another CPU's LAPACK in ``crossings_truth.all_crossings``' eigenvalue solve: a robust ray moves by
under 1e-4 relative when t is perturbed by 2e-6, so root differences of 1e-13 stay orders of magnitude below 1e-9, and a
flag can flip only for a ray that sits that close to a threshold.  On the machine that recorded the file every
difference is zero."""
import importlib.util
import os

import numpy as np
import pytest

import lights_truth
import refract_truth
import scene_truth
import textured_truth
from conftest import GOLDEN

RUNS = ([f"refract/{n}" for n in sorted(refract_truth.cases())] + [f"lights/{n}" for n in sorted(lights_truth.cases())]
        + [f"textured/{n}" for n in sorted(textured_truth.cases())]
        + [f"scene/{n}/{flag}" for n in sorted(scene_truth.cases()) for flag in (0, 1)])


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_shade_truth_golden", os.path.join(GOLDEN, "make_shade_truth_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLDEN, "shade_truth_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_file_holds_exactly_the_runs(recorded):
    assert len(RUNS) == 21
    assert {k.rsplit("/", 1)[0] for k in recorded} == set(RUNS)


@pytest.mark.parametrize("run", RUNS)
def test_the_one_loop_gives_what_the_four_gave(maker, recorded, run):
    tag, name, *flag = run.split("/")
    c = scene_truth.case(name, bool(int(flag[0]))) if tag == "scene" else \
        {"refract": refract_truth, "lights": lights_truth, "textured": textured_truth}[tag].case(name)
    got = maker.record(c)
    want = {k: recorded[f"{run}/{k}"] for k in got}
    assert len([k for k in recorded if k.startswith(run + "/")]) == len(got)
    robust = np.unpackbits(want["robust"]).astype(bool)[::maker.STEP]
    err = np.abs(got["rgb"] - want["rgb"])[robust]
    flips = int(np.unpackbits(got["robust"] ^ want["robust"]).sum())
    print(f"{run}: max |rgb - recorded| {err.max():.3e} on {int(robust.sum())} robust samples, {flips} robust flags differ")
    assert got["rgb"].shape == want["rgb"].shape == (4096 // maker.STEP, 3)
    assert np.all(err <= 1e-9 * (np.abs(want["rgb"])[robust] + 1e-5))
    assert flips <= 2
    assert np.array_equal(got["counts"], want["counts"])
    if "first" in got:
        assert np.array_equal(got["first"], want["first"])
