"""FP64 truth for trt_chords / trt_glow — TEST INFRASTRUCTURE (a helper module: no tests, no fixtures).

The pairing rule of include/trt.h on top of ``crossings_truth``'s roots (the companion-matrix solver of
``oracle/truth.py``) and FP64 inside tests at the two ends of the window; then the chords, and the emission–absorption
integral in closed form per piece (``expm1``).  numpy float64, vectorised over the rays; no arithmetic shared with the
kernels: the pieces are found by sorting all interval ends and asking each piece's midpoint which intervals hold it.

``robust`` is the conjunction of
  * ``crossings_truth.classify_margin_all`` over the ray's own window,
  * both window end points more than 1e-3 from every tube surface (a non-finite end point is outside and clear),
  * no crossing within 1e-3 of a per-ray bound.

Three kinds of case per scene of ``crossings_truth.SCENES``:
  los  ``ct.ray_set``: lines of sight, origins outside, the full window;
  seg  segments: both end points drawn by ``recipe_rays``' target rule (seed 11), d = b - a, window (0.001, 1);
  cut  the lines of sight with a per-ray bound between two crossings of the ray's own list (every fifth ray: an empty
       window), as tests/test_gpu_through.py builds them.
"""
import numpy as np

import crossings_truth as ct
import oriented_truth

TMIN, TMAX = ct.TMIN, ct.TMAX
NAMES = ("single", "nest3", "rings2", "nest8")
KINDS = ("los", "seg", "cut")
CAPS = {"single": 0.05, "nest3": 0.05, "rings2": 0.05, "nest8": 0.07}   # the two caps of tests/test_through_cpu.py
SEG_SEED = 11
EMPTY_BOUNDS = np.float32([TMIN, 0.0, np.nan, -np.inf, -3.0])

# one medium per torus: ((emission rgb), sigma) per unit world length; torus 5 of the nest of eight holds none
MEDIA = {
    "single": [((1.0, 0.5, 0.25), 0.75)],
    "nest3": [((2.0, 0.5, 0.25), 0.0), ((0.25, 0.5, 1.0), 0.5), ((0.0, 0.125, 0.25), 1.0)],
    "rings2": [((1.0, 0.25, 0.0), 2.0), ((0.0, 0.5, 1.0), 0.25)],
    "nest8": [((0.25 * (i % 3), 0.125 * i, 1.0 / (i + 1)), 0.25 * (i % 4)) if i != 5 else ((0.0, 0.0, 0.0), 0.0) for i in range(8)],
}


def surface_distance(P, C, axis, R, r):
    """Signed distance of points P (n, 3) from the tube surface of the torus (negative inside), float64."""
    p = np.asarray(P, np.float64) - np.asarray(C, np.float64)
    if axis is not None:
        p = p @ oriented_truth.frame(axis).T
    with np.errstate(invalid="ignore", over="ignore"):
        return np.hypot(np.hypot(p[:, 0], p[:, 2]) - R, p[:, 1]) - r


def _bound(n, tmax, bound):
    """tmax_i (n,) float64: the per-ray bound clipped by the scalar, NaN kept; the scalar without a bound."""
    if bound is None:
        return np.full(n, float(tmax))
    b = np.asarray(bound, np.float64).reshape(n)
    with np.errstate(invalid="ignore"):
        return np.where(b > tmax, float(tmax), b)


def intervals(o, d, geo, axes=None, tmin=TMIN, tmax=TMAX, bound=None):
    """The intervals of every torus by the pairing rule.  Returns (a, b, info): a, b of shape (n_tori, n, 3), NaN where
    unused (the rule yields at most two per torus; a third column catches a violation), and info = dict(in0, in1
    (n_tori, n) bool, ncross (n_tori, n), to_end (n_tori, n) bool: an interval closed by the window's end, tmax_i (n,),
    nonempty (n,))."""
    o = np.atleast_2d(np.asarray(o, np.float64))
    d = np.atleast_2d(np.asarray(d, np.float64))
    n, nt = len(o), len(geo)
    tend = _bound(n, tmax, bound)
    with np.errstate(invalid="ignore"):
        nonempty = tend > tmin
    A = np.full((nt, n, 3), np.nan)
    B = np.full((nt, n, 3), np.nan)
    in0 = np.zeros((nt, n), bool)
    in1 = np.zeros((nt, n), bool)
    ncross = np.zeros((nt, n), int)
    to_end = np.zeros((nt, n), bool)
    rows = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        P1 = o + np.where(nonempty, tend, 0.0)[:, None] * d
    for j, (C, R, r) in enumerate(geo):
        axis = None if axes is None else axes[j]
        t, nd = ct._roots_and_normal(o, d, C, axis, R, r)
        with np.errstate(invalid="ignore"):
            keep = (t > tmin) & (t < tend[:, None])
            in0[j] = nonempty & (surface_distance(o + tmin * d, C, axis, R, r) < 0.0)
            in1[j] = nonempty & (surface_distance(P1, C, axis, R, r) < 0.0)
            entering = keep & (nd < 0.0)
        ncross[j] = keep.sum(1)
        opened = np.where(in0[j], tmin, np.nan)
        has = in0[j].copy()
        slot = np.zeros(n, int)
        for k in range(4):   # the roots are ascending
            en = entering[:, k] & ~has
            opened = np.where(en, t[:, k], opened)
            lv = keep[:, k] & ~entering[:, k] & has
            A[j, rows[lv], slot[lv]] = opened[lv]
            B[j, rows[lv], slot[lv]] = t[lv, k]
            slot = slot + lv
            has = (has | en) & ~lv
        tail = has & in1[j]
        A[j, rows[tail], slot[tail]] = opened[tail]
        B[j, rows[tail], slot[tail]] = tend[tail]
        to_end[j] = tail
    assert np.isnan(A[:, :, 2]).all(), "more than two intervals of one torus"
    return A, B, dict(in0=in0, in1=in1, ncross=ncross, to_end=to_end, tmax_i=tend, nonempty=nonempty)


def chords(A, B, d):
    """(n_tori, n): the summed lengths of the intervals in world units."""
    length = np.linalg.norm(np.asarray(d, np.float64), axis=1)
    return np.nansum(B - A, axis=2) * length[None, :]


def glow(A, B, d, media, tmin, tmax_i):
    """(L (n, 3), T (n,)): emission and absorption of the media integrated front to back over the pieces between the
    sorted interval ends, each piece in closed form: L += eps * (-expm1(-tau) / sigma) * T, T *= exp(-tau)."""
    nt, n, _ = A.shape
    length = np.linalg.norm(np.asarray(d, np.float64), axis=1)
    eps = np.array([m[0] for m in media], np.float64)
    sig = np.array([m[1] for m in media], np.float64)
    ends = np.concatenate([A.transpose(1, 0, 2).reshape(n, -1), B.transpose(1, 0, 2).reshape(n, -1)], 1)
    ends = np.sort(np.where(np.isnan(ends), np.inf, ends), axis=1)   # unused ones go behind everything
    L = np.zeros((n, 3))
    T = np.ones(n)
    for k in range(ends.shape[1] - 1):
        u, v = ends[:, k], ends[:, k + 1]
        with np.errstate(invalid="ignore"):
            live = np.isfinite(v) & (v > u)
            mid = np.where(live, 0.5 * (u + v), np.nan)
            on = (A <= mid[None, :, None]) & (mid[None, :, None] <= B)          # (nt, n, 3)
        on = on.any(axis=2) & live[None, :]
        with np.errstate(invalid="ignore"):
            ell = np.where(live, v - u, 0.0) * length
        s = (on * sig[:, None]).sum(0)
        e = np.einsum("jn,jc->nc", on.astype(np.float64), eps)
        tau = s * ell
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(s > 0.0, -np.expm1(-tau) / np.where(s > 0.0, s, 1.0), ell)
        L += e * (w * T)[:, None]
        T = T * np.exp(-tau)
    return L, T


def ends_clear(o, d, geo, axes, tmin, info, margin=1e-3):
    """True where both end points of the window lie more than `margin` (one number, or one per torus) from every tube
    surface (a non-finite end point is outside and clear; so is every ray with an empty window)."""
    o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
    ok = np.ones(len(o64), bool)
    margins = np.broadcast_to(np.asarray(margin, np.float64), (len(geo),))
    with np.errstate(invalid="ignore", over="ignore"):
        P1 = o64 + np.where(info["nonempty"], info["tmax_i"], 0.0)[:, None] * d64
    for j, (C, R, r) in enumerate(geo):
        axis = None if axes is None else axes[j]
        for P in (o64 + tmin * d64, P1):
            dist = surface_distance(P, C, axis, R, r)
            with np.errstate(invalid="ignore"):
                ok &= ~(np.abs(dist) <= margins[j])
    return ok | ~info["nonempty"]


def robust_rays(o, d, geo, axes, tmin, tmax, bound, info, delta=1e-4, t_tol=1e-3, end_margin=1e-3):
    """The module's `robust`.  The margins are absolute, sized for scenes of size 1 and directions of length about 1; a
    caller off that scale passes its own: delta and t_tol go to ``crossings_truth.classify_margin_all`` (t_tol also
    keeps the crossings off a per-ray bound; an (n, 1) array gives every ray its own), end_margin to ``ends_clear``."""
    tend = info["tmax_i"]
    o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
    ok = ct.classify_margin_all(o64, d64, geo, axes, tmin, np.where(info["nonempty"], tend, tmin)[:, None], delta=delta, t_tol=t_tol)
    ok &= ends_clear(o, d, geo, axes, tmin, info, end_margin)
    if bound is not None:
        t, _, _, _ = ct.all_crossings(o64, d64, geo, axes, tmin, np.inf)
        with np.errstate(invalid="ignore"):
            ok &= ~np.any(np.abs(t - tend[:, None]) < t_tol, axis=1)
    return ok | ~info["nonempty"]   # an empty window is decided by the bound alone


def _targets(rng, tori, axes, n):
    """Points by recipe_rays' target rule: on torus (taken in turn) at a uniform angle, radial coordinate
    R + r_max·U(-1.2, 1.2), height r_max·U(-1.2, 1.2)."""
    rmax = max(r for _, _, r in tori)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    rad = rng.uniform(-1.2, 1.2, n) * rmax
    hgt = rng.uniform(-1.2, 1.2, n) * rmax
    tgt = np.empty((n, 3))
    for j, (C, R, _) in enumerate(tori):
        sel = np.arange(n) % len(tori) == j
        local = np.stack([(R + rad[sel]) * np.cos(phi[sel]), hgt[sel], (R + rad[sel]) * np.sin(phi[sel])], 1)
        M = np.eye(3) if axes is None else oriented_truth.frame(axes[j])
        tgt[sel] = local @ M + np.asarray(C, np.float64)
    return tgt


def segment_rays(tori, axes=None, n=ct.N_RAYS, seed=SEG_SEED):
    """Segments between two points of the target rule, rounded to FP32: (o, d = b - a); the window is (0.001, 1)."""
    rng = np.random.default_rng(seed)
    a = _targets(rng, tori, axes, n)
    b = _targets(rng, tori, axes, n)
    return a.astype(np.float32), (b - a).astype(np.float32)


def cut_bounds(t, cnt, tmin=TMIN):
    """Per-ray bounds from a ray-major list of crossings t (n, K) with cnt (n,) used slots: ray i is cut half way between
    crossing k - 1 (tmin for k = 0) and crossing k (one unit behind the last for k = cnt), k = i mod (cnt + 1); every
    fifth ray gets an empty window (the bound at tmin, below it, NaN, -inf).  Returns (bound float32 (n,), empty)."""
    n = len(cnt)
    rows = np.arange(n)
    k = rows % (cnt + 1)
    tt_ = np.concatenate([np.full((n, 1), tmin), np.asarray(t, np.float64)], 1)
    lo = tt_[rows, k]
    hi = np.where(k < cnt, tt_[rows, np.minimum(k + 1, tt_.shape[1] - 1)], lo + 1.0)
    bound = (lo + (hi - lo) * 0.5).astype(np.float32)
    empty = rows % 5 == 0
    bound[empty] = np.resize(EMPTY_BOUNDS, empty.sum())
    return bound, empty


def truth_of(o, d, geo, axes, media, tmin=TMIN, tmax=TMAX, bound=None, delta=1e-4, t_tol=1e-3, end_margin=1e-3):
    """dict(chords (n_tori, n), L (n, 3), T (n,), robust, ends (n,): the number of interval ends of the ray, t_last (n,):
    its largest finite interval end (0 without one), len (n,), inside_whole (n,): some tube holds the whole window
    without a crossing, to_end (n,): some interval is closed by the window's end, ends_clear (n,), A, B, info).
    delta, t_tol and end_margin are robust_rays' margins."""
    A, B, info = intervals(o, d, geo, axes, tmin, tmax, bound)
    L, T = glow(A, B, d, media, tmin, info["tmax_i"])
    fin = np.where(np.isnan(B), 0.0, B)
    return dict(chords=chords(A, B, d), L=L, T=T,
                robust=robust_rays(o, d, geo, axes, tmin, tmax, bound, info, delta, t_tol, end_margin),
                ends_clear=ends_clear(o, d, geo, axes, tmin, info, end_margin),
                ends=(~np.isnan(A)).sum(axis=(0, 2)) + (~np.isnan(B)).sum(axis=(0, 2)), t_last=fin.max(axis=(0, 2)),
                len=np.linalg.norm(np.asarray(d, np.float64), axis=1),
                inside_whole=(info["in0"] & info["in1"] & (info["ncross"] == 0)).any(0), to_end=info["to_end"].any(0),
                A=A, B=B, info=info)


_cases = {}


def case(name, kind):
    """The truth of scene `name` on the rays of `kind` with MEDIA[name], made once and never written:
    dict(o, d, tmin, tmax, bound (None | float32 (n,)), geo, axes, media, cap) plus truth_of's keys."""
    key = (name, kind)
    if key not in _cases:
        geo, axes = ct.SCENES[name]
        tmin, tmax, bound = float(np.float32(TMIN)), TMAX, None   # (the calls take floats: a bound of float32(0.001) is an empty window)
        if kind == "seg":
            o, d = segment_rays(geo, axes)
            tmax = 1.0
        else:
            s = ct.ray_set(name)
            o, d = s["o"], s["d"]
            if kind == "cut":
                bound, _ = cut_bounds(np.where(np.isfinite(s["t"]), s["t"], 0.0), s["count"])
        c = truth_of(o, d, geo, axes, MEDIA[name], tmin, tmax, bound)
        c.update(o=o, d=d, tmin=tmin, tmax=tmax, bound=bound, geo=geo, axes=axes, media=MEDIA[name], cap=CAPS[name])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[key] = c
    return _cases[key]
