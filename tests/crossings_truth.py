"""FP64 truth for trt_crossings — TEST INFRASTRUCTURE (a helper module: no tests, no fixtures).

Every crossing of a ray with every torus of a scene, in order: the real roots of each torus' quartic from the
companion-matrix solver of ``oracle/truth.py`` (through ``tests/oriented_truth.py`` for a torus with an axis), windowed
to the open interval (tmin, tmax) and merged in ascending t; ``entering`` from the sign of N·d with truth's normal.
Nothing of the library's walk is restated here.  Also the margin rule that tags the rays on which FP32 arithmetic may
legitimately count differently, the ray recipe and the scenes of tests/test_gpu_crossings.py, and the per-torus chord
lengths a caller forms from the enter / leave pairs.
"""
import numpy as np

import oriented_truth
from oracle import truth

TMIN, TMAX = 0.001, 10000.0
N_RAYS, SEED = 4096, 7

# name -> (tori [(C, R, r)], axes | None)
SCENES = {
    "single": ([((0.0, 0.0, 0.0), 1.0, 0.25)], None),
    "thin": ([((0.0, 0.0, 0.0), 1.0, 0.05)], None),
    "nest3": ([((0.0, 0.0, 0.0), 1.0, r) for r in (0.15, 0.25, 0.35)], None),
    "nest8": ([((0.0, 0.0, 0.0), 2.0, 0.10 + 0.05 * i) for i in range(8)], None),
    # two links of camera.linked_rings_scene(): centres 1.2 apart along x, axes perpendicular to the chain and to each other
    "rings2": ([((-0.6, 0.0, 0.0), 1.0, 0.2), ((0.6, 0.0, 0.0), 1.0, 0.2)], [(0.0, 1.0, 1.0), (0.0, -1.0, 1.0)]),
}


def scene(name, only=None):
    """abi.Scene of SCENES[name]; only = j: the scene that holds torus j alone, with its axis."""
    from toroidal_ray_tracing_amd import abi, camera
    tori, axes = SCENES[name]
    pick = range(len(tori)) if only is None else [only]
    return abi.Scene([(tori[j][0], tori[j][1], tori[j][2], 0) for j in pick], [camera.PLASTIC],
                     axes=None if axes is None else [axes[j] for j in pick])


def _roots_and_normal(o, d, C, axis, R, r):
    """(roots (n, 4) ascending, NaN padded; N·d at each root (n, 4), NaN where there is none)"""
    if axis is None:
        t = truth.real_roots(o, d, C, float(R), float(r))
    else:
        t = oriented_truth.real_roots(o, d, C, axis, R, r)
    P = o[:, None, :] + np.where(np.isnan(t), 0.0, t)[:, :, None] * d[:, None, :]
    with np.errstate(all="ignore"):
        if axis is None:
            N = truth.normal(P.reshape(-1, 3), C, float(R))
        else:
            N = oriented_truth.normal(P.reshape(-1, 3), C, axis, R)
    nd = np.einsum("nki,ni->nk", N.reshape(len(o), 4, 3), d)
    return t, np.where(np.isnan(t), np.nan, nd)


def all_crossings(o, d, tori, axes=None, tmin=TMIN, tmax=TMAX):
    """Every crossing of rays o, d (n, 3) with tori [(C, R, r), …] (axes: one per torus, or None for +y) inside the open
    interval (tmin, tmax), merged in ascending t.  Returns (t (n, 4·len(tori)) float64, inf padded; id, -1 padded;
    entering bool, False padded; count (n,))."""
    o = np.atleast_2d(np.asarray(o, np.float64))
    d = np.atleast_2d(np.asarray(d, np.float64))
    ts, ids, ens = [], [], []
    for j, (C, R, r) in enumerate(tori):
        t, nd = _roots_and_normal(o, d, C, None if axes is None else axes[j], R, r)
        with np.errstate(invalid="ignore"):
            keep = (t > tmin) & (t < tmax)
            ens.append(keep & (nd < 0.0))
        ts.append(np.where(keep, t, np.inf))
        ids.append(np.where(keep, j, -1))
    t, tid, en = np.concatenate(ts, 1), np.concatenate(ids, 1), np.concatenate(ens, 1)
    order = np.argsort(t, axis=1, kind="stable")
    t, tid, en = (np.take_along_axis(a, order, 1) for a in (t, tid, en))
    return t, tid, en, np.isfinite(t).sum(1)


def classify_margin_all(o, d, tori, axes=None, tmin=TMIN, tmax=TMAX, delta=1e-4, t_tol=1e-3):
    """True where the whole list of crossings is robust: scaling every r by (1 ± delta), with tmin·s and tmax/s, leaves the
    count unchanged and moves every t by less than t_tol, and no two crossings lie within t_tol of each other."""
    t0, _, _, c0 = all_crossings(o, d, tori, axes, tmin, tmax)
    with np.errstate(invalid="ignore"):
        ok = ~np.any(np.diff(t0, axis=1) < t_tol, axis=1)    # (inf - inf = NaN compares False)
        for s in (1.0 - delta, 1.0 + delta):
            ts, _, _, cs = all_crossings(o, d, [(C, R, r * s) for C, R, r in tori], axes, tmin * s, tmax / s)
            ok &= (cs == c0) & ~np.any(np.abs(ts - t0) >= t_tol, axis=1)
    return ok


def recipe_rays(tori, axes=None, n=N_RAYS, seed=SEED):
    """Lines of sight through the tubes: origins on the sphere of radius 4·R_max around the centroid of the centres;
    each ray aimed at a point of a torus of the scene (taken in turn) at a uniform angle about its axis, radial
    coordinate R + r_max·U(-1.2, 1.2), height r_max·U(-1.2, 1.2) — inside or just outside the tubes, so that grazing
    rays, rays through the hole and rays through all four walls all occur.  d = target - origin, not normalised (t = 1 at the
    target, as in a segment query); rounded to FP32."""
    rng = np.random.default_rng(seed)
    Rmax = max(R for _, R, _ in tori)
    rmax = max(r for _, _, r in tori)
    centre = np.mean([np.asarray(C, np.float64) for C, _, _ in tori], axis=0)
    v = rng.normal(size=(n, 3))
    o = centre + 4.0 * Rmax * v / np.linalg.norm(v, axis=1, keepdims=True)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    rad = rng.uniform(-1.2, 1.2, n) * rmax
    hgt = rng.uniform(-1.2, 1.2, n) * rmax
    tgt = np.empty((n, 3))
    for j, (C, R, _) in enumerate(tori):
        sel = np.arange(n) % len(tori) == j
        local = np.stack([(R + rad[sel]) * np.cos(phi[sel]), hgt[sel], (R + rad[sel]) * np.sin(phi[sel])], 1)
        M = np.eye(3) if axes is None else oriented_truth.frame(axes[j])
        tgt[sel] = local @ M + np.asarray(C, np.float64)   # world = Mᵀ · local
    return o.astype(np.float32), (tgt - o).astype(np.float32)


_sets = {}


def ray_set(name):
    """The recipe's rays for SCENES[name] with their truth, made once and never written:
    dict(o, d, t, id, entering, count, robust)."""
    if name not in _sets:
        tori, axes = SCENES[name]
        o, d = recipe_rays(tori, axes)
        t, tid, en, cnt = all_crossings(o, d, tori, axes)
        s = dict(o=o, d=d, t=t, id=tid, entering=en, count=cnt, robust=classify_margin_all(o, d, tori, axes))
        for a in s.values():
            a.setflags(write=False)
        _sets[name] = s
    return _sets[name]


def chord_lengths(t, tid, entering, n_tori):
    """Length of each ray inside each torus' tube, from one ray-major list of crossings (t, id, entering of shape
    (n, K), unused slots id = -1): the sum over the enter / leave pairs of torus j of (t_leave - t_enter), shape
    (n, n_tori).  A leave without an enter before it (the origin inside the tube) counts from t = 0."""
    n, K = t.shape
    chord = np.zeros((n, n_tori))
    opened = np.zeros((n, n_tori))
    rows = np.arange(n)
    for k in range(K):
        used = tid[:, k] >= 0
        j = np.where(used, tid[:, k], 0)
        tk = np.where(used, t[:, k], 0.0)
        en = used & entering[:, k]
        lv = used & ~entering[:, k]
        chord[rows[lv], j[lv]] += tk[lv] - opened[rows[lv], j[lv]]
        opened[rows[en], j[en]] = tk[en]
        opened[rows[lv], j[lv]] = 0.0
    return chord
