"""FP64 truth for trt_glow_weights_absorbed — TEST INFRASTRUCTURE (a helper module: no tests, no fixtures).

The rule of include/trt.h in numpy float64 on ``media_truth.intervals``' A, B: the pieces are found as
``profile_truth.same_rule`` finds them — all interval ends sorted, each piece's midpoint asked which intervals hold it —
with EVERY torus present, whatever its table; every piece is cut into ``steps`` equal sub-steps with two Gauss–Legendre
points in each; the sigma of the active tori is summed at both points and averaged, the homogeneous step gives the weight
w and what it lets through (``expm1``), and half of w times the transmittance in front of the sub-step is dealt to the two
knots around each point's label in every active torus.  No arithmetic is shared with the kernel: no fma, no series, no
exp2 polynomial, the sub-steps of a piece taken at once (``cumprod`` for the transmittance in front, ``np.add.at`` for
the deposits) instead of one after the other.

  same_rule(c, sigma_tables, steps)   (W (n_tori, 17, n), T (n,)) of case ``c`` (``media_truth.case`` or ``truth_of`` plus
                                      o, d, geo, axes); a table is (17,) sigma knots or a (17, 4) profile, whose column 3 is read
  pieces_per_torus(c)                 (P_j (n_tori, n), P (n,)): the non-empty pieces on which torus j is active, and
                                      those with any active torus, from the truth's merged ends
  example_case(), example_sigma(), example_table()   examples/absorbed_fit_main.cpp, value for value
"""
import numpy as np

import profile_truth as pt
import weights_truth as wt

KNOTS = pt.KNOTS


def _sigma(table):
    t = np.asarray(table, np.float64)
    return t[:, 3] if t.ndim == 2 else t


def _pieces(c):
    """Yields (rows, u, v, on (n_tori, m)) per slot of the sorted ends: the rays whose piece there is non-empty and has
    an active torus."""
    A, B = c["A"], c["B"]
    nt, n, _ = A.shape
    ends = np.concatenate([A.transpose(1, 0, 2).reshape(n, -1), B.transpose(1, 0, 2).reshape(n, -1)], 1)
    ends = np.sort(np.where(np.isnan(ends), np.inf, ends), axis=1)   # unused ones go behind everything
    for k in range(ends.shape[1] - 1):
        with np.errstate(invalid="ignore"):
            live = np.isfinite(ends[:, k + 1]) & (ends[:, k + 1] > ends[:, k])
        rows = np.nonzero(live)[0]
        if not len(rows):
            continue
        u, v = ends[rows, k], ends[rows, k + 1]
        mid = 0.5 * (u + v)
        with np.errstate(invalid="ignore"):
            on = ((A[:, rows] <= mid[None, :, None]) & (mid[None, :, None] <= B[:, rows])).any(axis=2)   # (nt, m)
        keep = on.any(0)
        if keep.any():
            yield rows[keep], u[keep], v[keep], on[:, keep]


def pieces_per_torus(c):
    nt, n, _ = c["A"].shape
    Pj, P = np.zeros((nt, n), int), np.zeros(n, int)
    for rows, _, _, on in _pieces(c):
        Pj[:, rows] += on
        P[rows] += 1
    return Pj, P


def same_rule(c, sigma_tables, steps):
    """(W (n_tori, 17, n), T (n,)) float64: the rule of trt_glow_weights_absorbed on the truth's intervals."""
    nt, n, _ = c["A"].shape
    o, d = np.asarray(c["o"], np.float64), np.asarray(c["d"], np.float64)
    length = np.linalg.norm(d, axis=1)
    sig = [_sigma(t) for t in sigma_tables]
    W = np.zeros((nt, KNOTS, n))
    T = np.ones(n)
    k_sub = (np.arange(steps) + 0.5)[:, None]
    for rows, u, v, on in _pieces(c):
        h = (v - u) / steps
        centre = u[None, :] + k_sub * h[None, :]                                   # (steps, m)
        t = np.stack([centre - pt.GAUSS * h[None, :], centre + pt.GAUSS * h[None, :]])   # (2, steps, m)
        P = o[rows][None, None] + t[..., None] * d[rows][None, None]               # (2, steps, m, 3)
        s_pts = np.zeros(t.shape)
        where = {}
        for j, (C, R, r) in enumerate(c["geo"]):
            if not on[j].any():
                continue
            axis = None if c["axes"] is None else c["axes"][j]
            y = np.minimum(pt.label(P[:, :, on[j]], C, axis, R, r), 1.0) * 16.0
            kn = np.minimum(np.floor(y).astype(int), 15)
            f = y - kn
            s_pts[:, :, on[j]] += sig[j][kn] + f * (sig[j][kn + 1] - sig[j][kn])
            where[j] = (kn, f)
        s = 0.5 * (s_pts[0] + s_pts[1])                                            # (steps, m)
        ell = (h * length[rows])[None, :]
        tau = s * ell
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(s > 0.0, -np.expm1(-tau) / np.where(s > 0.0, s, 1.0), ell)
        E = np.exp(-tau)
        before = T[rows][None, :] * np.concatenate([np.ones((1, len(rows))), np.cumprod(E, axis=0)[:-1]])   # T in front of sub-step k
        g = 0.5 * w * before
        for j, (kn, f) in where.items():
            gj = np.broadcast_to(g[:, on[j]], kn.shape)
            col = np.broadcast_to(rows[on[j]], kn.shape)
            np.add.at(W[j], (kn, col), gj * (1.0 - f))
            np.add.at(W[j], (kn + 1, col), gj * f)
        T[rows] = T[rows] * np.prod(E, axis=0)
    return W, T


# ---------------------------------------------------------------------------------------------------------------------
# examples/absorbed_fit_main.cpp, value for value
# ---------------------------------------------------------------------------------------------------------------------
EXAMPLE_W, EXAMPLE_H, EXAMPLE_STEPS = wt.EXAMPLE_W, wt.EXAMPLE_H, wt.EXAMPLE_STEPS


def example_case():
    """emission_fit's torus and camera rays (weights_truth.example_case)."""
    return wt.example_case()


def example_sigma():
    """(17,) float32: sigma = 1.5 (1 - x), densest on the tube's axis."""
    return np.array([1.5 * (1.0 - k / 16.0) for k in range(KNOTS)], np.float64).astype(np.float32)


def example_table():
    """(17, 4) float32: emission_fit's red and blue lines with example_sigma() in column 3."""
    table = np.array(wt.example_table())
    table[:, 3] = example_sigma()
    return table
