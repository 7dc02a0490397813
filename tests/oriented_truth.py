"""FP64 truth for tori on any axis — TEST INFRASTRUCTURE (a helper module: no tests, no fixtures).

``oracle/truth.py`` knows tori that turn about +y.  A torus (C, axis, R, r) is such a torus in a frame of its own, so
everything here rotates into that frame in float64, asks ``truth`` there, and rotates the answer back: no root finder,
margin rule or normal is restated.  The frame is built by a rule of this module's own (Gram–Schmidt against the world
axis least aligned with the torus axis) — not the library's rule: the torus is symmetric about its axis, so any two
frames must give the same answers, and the tests check the library against that.
"""
import numpy as np

from oracle import truth


def unit(a):
    a = np.asarray(a, np.float64)
    return a / np.linalg.norm(a)


def frame(axis):
    """3x3 float64 rotation M with rows (u, a, w), a = unit(axis), right-handed with a in the role of +y:
    local = M @ world, world = M.T @ local; M maps the axis to (0, 1, 0)."""
    a = unit(axis)
    h = np.zeros(3)
    h[int(np.argmin(np.abs(a)))] = 1.0
    u = h - (h @ a) * a
    u /= np.linalg.norm(u)
    w = np.cross(u, a)
    return np.stack([u, a, w])


def random_rotation(rng):
    """A rotation matrix, uniform over SO(3) (QR of a Gaussian matrix, determinant fixed to +1)."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def to_local(o, d, C, axis):
    """Rays (n,3) in the frame of the torus centred at C with the given axis: the torus sits at the origin there, axis +y."""
    M = frame(axis)
    o = np.atleast_2d(np.asarray(o, np.float64)) - np.asarray(C, np.float64)
    d = np.atleast_2d(np.asarray(d, np.float64))
    return o @ M.T, d @ M.T


def real_roots(o, d, C, axis, R, r):
    lo, ld = to_local(o, d, C, axis)
    return truth.real_roots(lo, ld, (0.0, 0.0, 0.0), float(R), float(r))


def first_hit(o, d, tori, tmin=0.001, tmax=10000.0):
    """Closest hit over tori [(C, axis, R, r), …]: (t (NaN = miss), id (-1 = miss)) — truth.first_hit's loop with every
    torus asked in its own frame (t is the same number in every frame)."""
    o = np.atleast_2d(np.asarray(o, np.float64))
    best = np.full(len(o), np.inf)
    bid = np.full(len(o), -1)
    for i, (C, axis, R, r) in enumerate(tori):
        t = real_roots(o, d, C, axis, R, r)
        t = np.where((t > tmin) & (t < tmax), t, np.inf)
        ti = np.min(t, axis=1)
        upd = ti < best
        best = np.where(upd, ti, best)
        bid = np.where(upd, i, bid)
    return np.where(np.isfinite(best), best, np.nan), bid


def classify_margin(o, d, tori, tmin=0.001, tmax=10000.0, delta=1e-4, t_tol=1e-3):
    """True where the first hit is robust.  One torus: truth.classify_margin itself, in the torus' frame.  Several tori
    have several frames, so the same rule (same hit/miss, same torus, |Δt| < t_tol under r·(1 ± delta) and the interval
    bounds ·(1 ± delta)) is applied over first_hit() above."""
    if len(tori) == 1:
        C, axis, R, r = tori[0]
        lo, ld = to_local(o, d, C, axis)
        return truth.classify_margin(lo, ld, [((0.0, 0.0, 0.0), float(R), float(r))], tmin, tmax, delta, t_tol)
    t0, id0 = first_hit(o, d, tori, tmin, tmax)
    ok = np.ones(len(t0), bool)
    for s in (1 - delta, 1 + delta):
        ts, ids = first_hit(o, d, [(C, a, R, r * s) for C, a, R, r in tori], tmin * s, tmax / s)
        same = (np.isnan(ts) == np.isnan(t0)) & (ids == id0)
        with np.errstate(invalid="ignore"):
            close = np.isnan(t0) | (np.abs(ts - t0) < t_tol)
        ok &= same & close
    return ok


def normal(P, C, axis, R):
    """Outward unit normal at world points P (n,3) of the torus (C, axis, R, ·): truth.normal in the frame, rotated back."""
    M = frame(axis)
    pl = (np.asarray(P, np.float64) - np.asarray(C, np.float64)) @ M.T
    return truth.normal(pl, (0.0, 0.0, 0.0), float(R)) @ M


def rotated_family(family, n, seed, C, Q, R, r, tmin=0.001):
    """truth.closed_form_family for the torus at the origin on +y, carried to the torus at C whose frame is the rotation Q
    (world = Q @ local, so its axis is Q @ ŷ): float64 rays (o, d), the closed-form t (inf = miss; rotation and
    translation leave it alone), the world normal and the margin flag.  Returns (o, d, t, N, ok, axis)."""
    o, d, t, N, ok = truth.closed_form_family(family, n, seed, C=(0.0, 0.0, 0.0), R=R, r=r, tmin=tmin)
    Q = np.asarray(Q, np.float64)
    ow = o.astype(np.float64) @ Q.T + np.asarray(C, np.float64)
    return ow, d.astype(np.float64) @ Q.T, t, N @ Q.T, ok, Q @ np.array([0.0, 1.0, 0.0])


def aimed_rays(n, seed, C, R, r):
    """Rays from the sphere of radius 4(R+r) around C aimed at points of the bounding ball (radius R+r), rounded to FP32."""
    rng = np.random.default_rng(seed)
    C = np.asarray(C, np.float64)
    v = rng.normal(size=(n, 3))
    o = C + 4.0 * (R + r) * v / np.linalg.norm(v, axis=1, keepdims=True)
    w = rng.normal(size=(n, 3))
    tgt = C + (R + r) * np.cbrt(rng.uniform(size=(n, 1))) * w / np.linalg.norm(w, axis=1, keepdims=True)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)
