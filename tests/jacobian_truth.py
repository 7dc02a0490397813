"""FP64 truth for trt_glow_tangent and trt_glow_adjoint — TEST INFRASTRUCTURE (a helper module: no tests, no fixtures).

The function that is differentiated is trt_glow_project's rule in exact arithmetic (include/trt.h); its pieces, Gauss points,
knots and fractions are ``absorbed_truth``'s (``_pieces``: every torus present, the pieces cut at every wall) and depend on
the rays and the tori alone.  ``geometry`` forms them once; the two derivatives are written separately on top of them:

  tangent(c, tables, delta, steps)   FORWARD mode, front to back: with every sub-step the derivative of its own (e, sg, E, w)
                                     and of the running (L, T) in the direction delta is carried along (dT as d log T).
  adjoint(c, tables, y, steps)       REVERSE mode: one sweep front to back that keeps (e, E, w, w', T in front) of every
                                     sub-step, then one back to front that carries the adjoint Tbar of the running T
                                     (Tbar = Tbar E + sum_c y_c e_c w, as Tbar T: a sum from behind) and deals the
                                     adjoints of e and sg to the hats.  No B = L - prefix is formed.
Neither is derived from the other; tests/test_jacobian_cpu.py holds them to each other, to central differences of the
forward rule and to a closed form.  No arithmetic is shared with the kernels: ``expm1``, no series, no fma, no exp2
polynomial, and the sub-steps of a piece are taken at once (cumprod, cumsum, bincount) instead of one after the other.  w' = (l E - w) / sg is the FP64 quotient as it stands, (tau E + expm1(-tau)) / sg^2: its absolute error is
about 2^-53 l / sg, nothing against an FP32 bar with the tables of these tests (a sigma is 0 or above 1e-3).

Both also return the sums of the ABSOLUTE values of the terms they add, which the error bars need:
  tangent:  d (n, 4); abs (n, 4): sum_s |de| w T + |dsg| (e |w'| T + l B) per colour, T sum_s l |dsg| for T — |de| and
            |dsg| being the hats applied to |delta|, what a sum of mixed signs rounds relative to;
            D (n,): sum_s l |dsg|;  peak (n, 4): the largest such integrand of the ray per unit of world length AND of
            the transmittance in front, |de| w / l + |dsg| (e |w'| / l + B / T_s) per colour (>= the integrand, T_s <= 1),
            and the largest |dsg| for T.
  adjoint:  grad (n_tori, 17, 4); G (n_tori, 17, 4, n) per ray; abs (n_tori, 17, 4, n) with |y| and every term positive;
            abs_L (n_tori, 17, n): the sigma entry's sum with L_c in place of B_c (B <= L: what a B formed as L minus a
            prefix rounds relative to);  peak (n,): the largest |lambda| per unit of world length and of the transmittance
            in front, sum_c |y_c| (e |w'| / l + B / T_s) + |y_3| T / T_s.
"""
import numpy as np

import absorbed_truth as at
import profile_truth as pt

KNOTS = pt.KNOTS


def geometry(c, steps):
    """The pieces of case ``c`` front to back, each a dict: rows (m,), ell (m,) the world length of a sub-step, hats: per
    active torus (j, sel (m,) bool, kn (2, steps, mj) int, f (2, steps, mj))."""
    o, d = np.asarray(c["o"], np.float64), np.asarray(c["d"], np.float64)
    length = np.linalg.norm(d, axis=1)
    k_sub = (np.arange(steps) + 0.5)[:, None]
    out = []
    for rows, u, v, on in at._pieces(c):
        h = (v - u) / steps
        centre = u[None, :] + k_sub * h[None, :]
        t = np.stack([centre - pt.GAUSS * h[None, :], centre + pt.GAUSS * h[None, :]])   # (2, steps, m)
        P = o[rows][None, None] + t[..., None] * d[rows][None, None]
        hats = []
        for j, (C, R, r) in enumerate(c["geo"]):
            if not on[j].any():
                continue
            axis = None if c["axes"] is None else c["axes"][j]
            y = np.minimum(pt.label(P[:, :, on[j]], C, axis, R, r), 1.0) * 16.0
            kn = np.minimum(np.floor(y).astype(int), 15)
            hats.append((j, on[j], kn, y - kn))
        out.append(dict(rows=rows, ell=h * length[rows], hats=hats, steps=steps))
    return out


def _at_hats(piece, tables):
    """(steps, m, 4): sum_jk hat_s[j][k] * tables[j][k] for every sub-step of the piece."""
    val = np.zeros((piece["steps"], len(piece["rows"]), 4))
    for j, sel, kn, f in piece["hats"]:
        tab = np.asarray(tables[j], np.float64)
        v = (1.0 - f)[..., None] * tab[kn] + f[..., None] * tab[kn + 1]   # (2, steps, mj, 4)
        val[:, sel] += 0.5 * (v[0] + v[1])
    return val


def _step(sg, ell):
    """(E, w, w') of homogeneous steps."""
    tau = sg * ell
    pos = sg > 0.0
    safe = np.where(pos, sg, 1.0)
    E = np.exp(-tau)
    w = np.where(pos, -np.expm1(-tau) / safe, ell)
    wp = np.where(pos, (tau * E + np.expm1(-tau)) / (safe * safe), -0.5 * ell * ell)
    return E, w, wp


def _excl(a):
    """The exclusive running sum along axis 0: what lies in front of every sub-step of a piece."""
    return np.cumsum(a, axis=0) - a


def _before(T0, E):
    """T in front of every sub-step of a piece that T0 enters."""
    return T0[None, :] * np.concatenate([np.ones((1, E.shape[1])), np.cumprod(E, axis=0)[:-1]])


def forward(c, tables, steps, geo=None):
    """(L (n, 3), T (n,)) of the rule itself on the same pieces."""
    n = len(c["o"])
    L, T = np.zeros((n, 3)), np.ones(n)
    for piece in geo if geo is not None else geometry(c, steps):
        rows = piece["rows"]
        e = _at_hats(piece, tables)
        E, w, _ = _step(e[..., 3], piece["ell"][None, :])
        L[rows] += (e[..., :3] * (w * _before(T[rows], E))[..., None]).sum(0)
        T[rows] *= np.prod(E, axis=0)
    return L, T


def tangent(c, tables, delta, steps, geo=None):
    geo = geo if geo is not None else geometry(c, steps)
    n = len(c["o"])
    Ltot, _ = forward(c, tables, steps, geo)
    L, T = np.zeros((n, 3)), np.ones(n)
    dL, dlogT = np.zeros((n, 3)), np.zeros(n)   # dT is carried as d log T: d(T E) / (T E) = dT / T + dE / E
    aL, aD = np.zeros((n, 3)), np.zeros(n)      # the absolute sums; aD = sum_{s' < s} l |dsg|
    peak = np.zeros((n, 4))
    for piece in geo:
        rows, ell = piece["rows"], piece["ell"][None, :]
        e, de = _at_hats(piece, tables), _at_hats(piece, delta)
        ade = _at_hats(piece, [np.abs(np.asarray(v, np.float64)) for v in delta])
        ec, dec, dsg, adsg = e[..., :3], de[..., :3], de[..., 3], ade[..., 3]
        E, w, wp = _step(e[..., 3], ell)
        Tb = _before(T[rows], E)
        dTb = Tb * (dlogT[rows][None, :] + _excl(-ell * dsg))          # dT in front of every sub-step
        # d(e w T) = de w T + e dw T + e w dT
        dL[rows] += (dec * (w * Tb)[..., None] + ec * (wp * dsg * Tb)[..., None] + ec * (w * dTb)[..., None]).sum(0)
        own = ade[..., :3] * (w * Tb)[..., None] + ec * (adsg * np.abs(wp) * Tb)[..., None]
        aDb = aD[rows][None, :] + _excl(ell * adsg)
        aL[rows] += (own + ec * (w * Tb * aDb)[..., None]).sum(0)
        through = L[rows][None] + np.cumsum(ec * (w * Tb)[..., None], axis=0)   # the prefix through every sub-step
        B = np.maximum(Ltot[rows][None] - through, 0.0)
        per = (own + (adsg * ell)[..., None] * B) / (ell * Tb)[..., None]     # (a piece is not empty and T_s > 0)
        peak[rows] = np.maximum(peak[rows], np.concatenate([per.max(0), adsg.max(0)[:, None]], 1))
        L[rows] = through[-1]
        T[rows] *= np.prod(E, axis=0)
        dlogT[rows] += (-ell * dsg).sum(0)
        aD[rows] += (ell * adsg).sum(0)
    return dict(d=np.concatenate([dL, (T * dlogT)[:, None]], 1), abs=np.concatenate([aL, (T * aD)[:, None]], 1), D=aD, peak=peak, L=L, T=T)


def _deal(out, n, kn, f, col, val):
    """out (17, n) += the values val (steps, mj) of every sub-step dealt to the hats of both points: half of (1 - f) to kn, half
    of f to kn + 1, in the columns col (mj,)."""
    for p in range(2):
        for hat, k in ((0.5 * (1.0 - f[p]), kn[p]), (0.5 * f[p], kn[p] + 1)):
            out += np.bincount((k * n + col[None, :]).ravel(), weights=(hat * val).ravel(), minlength=KNOTS * n).reshape(KNOTS, n)


def adjoint(c, tables, y, steps, geo=None):
    geo = geo if geo is not None else geometry(c, steps)
    n, nt = len(c["o"]), len(c["geo"])
    y = np.asarray(y, np.float64).reshape(n, 4)
    ay = np.abs(y)
    # front to back: what every sub-step was
    L, T = np.zeros((n, 3)), np.ones(n)
    tape = []
    for piece in geo:
        rows = piece["rows"]
        e = _at_hats(piece, tables)
        E, w, wp = _step(e[..., 3], piece["ell"][None, :])
        Tb = _before(T[rows], E)
        L[rows] += (e[..., :3] * (w * Tb)[..., None]).sum(0)
        T[rows] *= np.prod(E, axis=0)
        tape.append((e, E, w, wp, Tb))
    # back to front: C = Tbar T, the adjoint of the transmittance behind a sub-step times that transmittance — the recursion
    # Tbar <- Tbar E + sum_c y_c e_c w of the running T, multiplied through by T so that no quotient of two T is formed
    Cb, aCb = y[:, 3] * T, ay[:, 3] * T
    G, A = np.zeros((nt, KNOTS, 4, n)), np.zeros((nt, KNOTS, 4, n))
    AL = np.zeros((nt, KNOTS, n))
    peak = np.zeros(n)
    fixed = (ay[:, :3] * L).sum(1) + ay[:, 3] * T   # sum_c |y_c| L_c + |y_3| T
    for piece, (e, E, w, wp, Tb) in zip(reversed(geo), reversed(tape)):
        rows, ell = piece["rows"], piece["ell"][None, :]
        ec = e[..., :3]
        own, aown = (y[rows, :3][None] * ec).sum(-1), (ay[rows, :3][None] * ec).sum(-1)     # (steps, m)
        gain, again = own * w * Tb, aown * w * Tb
        behind = Cb[rows][None, :] + (np.cumsum(gain[::-1], axis=0)[::-1] - gain)           # C behind every sub-step
        abehind = aCb[rows][None, :] + (np.cumsum(again[::-1], axis=0)[::-1] - again)
        sgbar = own * wp * Tb - ell * behind
        asg = aown * np.abs(wp) * Tb + ell * abehind
        asg_L = aown * np.abs(wp) * Tb + ell * fixed[rows][None, :]
        peak[rows] = np.maximum(peak[rows], (asg / (ell * Tb)).max(0))
        Cb[rows] += gain.sum(0)
        aCb[rows] += again.sum(0)
        for j, sel, kn, f in piece["hats"]:
            col = rows[sel]
            for ch in range(3):
                ebar = y[col, ch][None, :] * (w * Tb)[:, sel]
                _deal(G[j, :, ch], n, kn, f, col, ebar)
                _deal(A[j, :, ch], n, kn, f, col, np.abs(ebar))
            _deal(G[j, :, 3], n, kn, f, col, sgbar[:, sel])
            _deal(A[j, :, 3], n, kn, f, col, asg[:, sel])
            _deal(AL[j], n, kn, f, col, asg_L[:, sel])
    return dict(grad=G.sum(-1), G=G, abs=A, abs_L=AL, peak=peak, L=L, T=T)
