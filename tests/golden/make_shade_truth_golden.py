"""Regenerates ``tests/golden/shade_truth_cases.npz`` (run from the repo root:
``python tests/golden/make_shade_truth_golden.py [out.npz]``).

The committed file was recorded at parent commit ``046b695``, when refract_truth, lights_truth, textured_truth and
scene_truth each still had a payload loop of their own: it is what those four loops gave, and so what the one loop of
``shade_truth`` has to give.  A regenerated file must compare equal to the committed one by
``tests/test_shade_truth_golden.py``, the test that reads it.

Every run of the family is in it: 5 refract + 4 lights + 4 textured + 4 scene cases x 2 flags = 21.  Per run
``<run>/rgb`` (float64) of every 32nd of the 4096 rays, ``<run>/robust`` of all rays as packed bits, ``<run>/first`` the
first-hit id of the sampled rays where the truth records one, and ``<run>/counts``: the number of glass events, of
total internal reflections among them and of ``fractional`` first hits (-1 where the run has no such record).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP = 32


def runs():
    """name -> the case dict of every run, in the order of the file."""
    import lights_truth
    import refract_truth
    import scene_truth
    import textured_truth
    out = {}
    for mod, tag in ((refract_truth, "refract"), (lights_truth, "lights"), (textured_truth, "textured")):
        for name in sorted(mod.cases()):
            out[f"{tag}/{name}"] = mod.case(name)
    for name in sorted(scene_truth.cases()):
        for flag in (False, True):
            out[f"scene/{name}/{int(flag)}"] = scene_truth.case(name, flag)
    return out


def record(c):
    """The arrays kept of one run."""
    ev, first = c.get("events"), c.get("first")
    first_id = first["id"] if isinstance(first, dict) else first
    counts = [-1 if ev is None else len(ev["ray"]), -1 if ev is None else int(np.count_nonzero(ev["tir"])),
              int(np.count_nonzero(first["fractional"])) if isinstance(first, dict) and "fractional" in first else -1]
    kept = dict(rgb=np.asarray(c["rgb"], np.float64)[::STEP], robust=np.packbits(c["robust"]), counts=np.array(counts, np.int64))
    if first_id is not None:
        kept["first"] = np.asarray(first_id)[::STEP].astype(np.int8)
    return kept


def main(path):
    np.savez_compressed(path, **{f"{run}/{k}": v for run, c in runs().items() for k, v in record(c).items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "shade_truth_cases.npz"))
