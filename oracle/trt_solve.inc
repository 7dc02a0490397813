/*
 * trt_solve.inc — TEST INFRASTRUCTURE (CPU oracle), type-generic part.
 *
 * Included twice by trt_oracle.c with REAL = float and REAL = double.
 *
 * Ray–torus intersection (SURVEY.md §8a rows T1, T2).  The reference has NO torus
 * primitive (its intersections are hardware triangle queries behind traceRayEXT,
 * REFL/shaders/raytrace.rgen:64-75), so this arithmetic is build-defined: PARITY UNPINNED
 * by the reference; pinned instead by the analytic known-answer vectors in
 * tests/golden/ and by the independent FP64 companion-matrix solver in oracle/truth.py.
 *
 * Only IEEE-754 correctly rounded operations are used (+ - * / sqrt fma), each written
 * explicitly, and the file is compiled with -ffp-contract=off: the HIP kernels execute the
 * same operation DAG and must agree BIT FOR BIT.
 *
 * Semantics taken from the reference: a hit is the SMALLEST ray parameter t with
 * tMin < t < tMax (closest-hit query, open interval: REFL/shaders/raytrace.rgen:50-52,64-75).
 *
 * Algorithm ("depressed quartic + Fourier–Newton walk"):
 *   T1  shift the ray parameter to the point of closest approach to the torus centre
 *       (u = t - tc, q0 = o + tc·d, q0 ⟂ d).  With m=|q0|², κ = m+R²-r², dd=|d|²,
 *       a = dx²+dz², b = q0x·dx+q0z·dz, c = q0x²+q0z² the torus equation
 *       (|p|²+R²-r²)² = 4R²(px²+pz²) along p = q0+u·d has no cubic term:
 *           f(u) = A4·u⁴ + P2·u² + Q1·u + S0
 *           A4 = dd², P2 = 2·dd·κ - 4R²·a, Q1 = -8R²·b, S0 = κ² - 4R²·c.
 *       A bounding sphere of squared radius Rb² = (R+r)²·(1+2⁻⁹) gives the cull m <= Rb² and the
 *       parameter window |u| <= U = sqrt((Rb²-m)/dd), intersected with (tMin-tc, tMax-tc).
 *       (Inflated by ~0.1 % so that the walk starts strictly OUTSIDE the torus: on the
 *       exact bounding sphere f(-U) = 0 at the outer equator and its computed sign is noise.)
 *       The window is then clipped to the bounding slab (T1b in the code).  tc is a rounded number, so a second,
 *       small step tc2 of the same shift follows the cull (T1a in the code): q0 ⟂ d then holds to the rounding of q0
 *       however far away the origin lies, and t = u + tc + tc2.
 *   T2  f'' = 12·A4·u² + 2·P2 has constant sign on at most three pieces of the window
 *       (split at ±w, w = sqrt(-P2/(6·A4)), when P2 < 0; 1/(6·A4) is formed as (1/dd)²·(1/6)).  On a piece [A,B] with
 *       sign(f'') = σ, Fourier's condition says Newton's iteration started where
 *       sign(f) = σ converges monotonically, never overshooting a root:
 *         sign f(A) =  σ : iterate from A to the right.  Either it converges to the first
 *                          root of the piece, or σ·f' turns >= 0 / the iterate leaves the
 *                          piece, which PROVES the piece has no root.
 *         sign f(A) = -σ : the piece holds a root iff sign f(B) = σ, and then exactly
 *                          one; iterate from B to the left.
 *       Pieces are walked left to right, so the first root found is the smallest.
 */

typedef struct SUF(torus_k) {
  REAL cx, cy, cz;
  REAL R;
  REAL r2;      /* r²        */
  REAL rpol2;   /* (r / 32)²: square of the largest distance the geometric polish may move the point */
  REAL k0;      /* R² - r²   */
  REAL Rb2;     /* (R + r)²·(1 + 2⁻⁹): squared radius of the (slightly inflated) bounding sphere */
  REAL rs;      /* r·(1 + 2⁻⁸): half height of the (slightly inflated) bounding slab |y| <= rs */
  REAL fourR2;  /* 4·R²      */
} SUF(torus_k);

static void SUF(torus_prepare)(const trt_torus* t, SUF(torus_k)* k)
{
  const REAL R = (REAL)t->R, r = (REAL)t->r;
  const REAL R2 = R * R, r2 = r * r, s = R + r;
  k->cx = (REAL)t->center[0];
  k->cy = (REAL)t->center[1];
  k->cz = (REAL)t->center[2];
  k->R      = R;
  k->r2     = r2;
  k->rpol2  = (r * (REAL)0.03125) * (r * (REAL)0.03125);
  k->k0     = R2 - r2;
  const REAL s2 = s * s;
  k->Rb2    = FMA(s2, (REAL)0.001953125, s2);
  k->rs     = FMA(r, (REAL)0.00390625, r);
  k->fourR2 = (REAL)4 * R2;
}

#define TRT_NEWTON_CAP 48

/* f and f' of the depressed quartic at u. */
#define TRT_EVAL(u, fx, dx)                                   \
  do {                                                        \
    const REAL e1_ = FMA(A4 * (u), (u), P2);                  \
    const REAL e2_ = FMA(e1_, (u), Q1);                       \
    (fx)           = FMA(e2_, (u), S0);                       \
    const REAL g1_ = FMA(A4x4 * (u), (u), P2x2);              \
    (dx)           = FMA(g1_, (u), Q1);                       \
  } while(0)

/* T2, alternative solver: Durand–Kerner (Weierstrass) iteration on the monic depressed quartic
 * u⁴ + p·u² + q·u + s (p = P2/A4 …; 1/A4 is formed as (1/dd)²).  The four complex iterates start
 * on the classic spiral (0.4+0.9i)^k scaled by the bounding-sphere radius in parameter units,
 * are updated in place (Gauss–Seidel order k = 0..3, product over j = 0..3, j != k) for a FIXED
 * number of sweeps — so that every lane of a wavefront runs the same trip count — and use only
 * + - * / fma: the HIP kernels reproduce them bit for bit.  A root counts as real when
 * |Im| <= TRT_DK_TOL·scale; real candidates get two guarded Newton steps on the real quartic, and
 * the smallest one inside the window [lo,hi] is returned.  Weaknesses (DESIGN.md §4): grazing
 * rays (double roots converge linearly and keep |Im| ~ sqrt(eps)) are classified by the
 * tolerance, not by a proof, and the cost is ≈10x the Fourier–Newton walk. */
#define TRT_DK_SWEEPS 24
static int SUF(dk_first_root)(REAL A4, REAL P2, REAL Q1, REAL S0, REAL inv_dd, REAL lo, REAL hi,
                              REAL Rb2, REAL* root_out)
{
  static const REAL CR[4] = {(REAL)1.0, (REAL)0.4, (REAL)-0.65, (REAL)-0.908};
  static const REAL CI[4] = {(REAL)0.0, (REAL)0.9, (REAL)0.72, (REAL)-0.297};
  const REAL iA4 = inv_dd * inv_dd;
  const REAL p = P2 * iA4, q = Q1 * iA4, s = S0 * iA4;
  const REAL sc  = SQRT(Rb2 * inv_dd);
  const REAL tol = TRT_DK_TOL * sc;
  REAL zr[4], zi[4];
  for(int k = 0; k < 4; ++k) { zr[k] = sc * CR[k]; zi[k] = sc * CI[k]; }
  for(int it = 0; it < TRT_DK_SWEEPS; ++it)
    for(int k = 0; k < 4; ++k)
    {
      const REAL x = zr[k], y = zi[k];
      /* f(z) = ((z² + p)·z + q)·z + s */
      const REAL ar = FMA(x, x, -(y * y)) + p, ai = (x + x) * y;
      const REAL br = FMA(ar, x, -(ai * y)) + q, bi = FMA(ar, y, ai * x);
      const REAL fr = FMA(br, x, -(bi * y)) + s, fi = FMA(br, y, bi * x);
      /* Π_{j != k} (z_k - z_j) */
      REAL dr = (REAL)1, di = (REAL)0;
      for(int j = 0; j < 4; ++j)
        if(j != k)
        {
          const REAL er = x - zr[j], ei = y - zi[j];
          const REAL nr = FMA(dr, er, -(di * ei)), ni = FMA(dr, ei, di * er);
          dr = nr; di = ni;
        }
      const REAL den = FMA(dr, dr, di * di);
      if(den > (REAL)0 && den < (REAL)INFINITY)
      {
        const REAL inv = (REAL)1 / den;
        zr[k] = x - FMA(fr, dr, fi * di) * inv;
        zi[k] = y - FMA(fi, dr, -(fr * di)) * inv;
      }
    }
  int  found = 0;
  REAL best  = (REAL)0;
  const REAL A4x4 = (REAL)4 * A4, P2x2 = (REAL)2 * P2;
  for(int k = 0; k < 4; ++k)
  {
    if(!(FABS(zi[k]) <= tol))
      continue;
    REAL u = zr[k];
    for(int n = 0; n < 2; ++n)
    {
      const REAL e1 = FMA(A4 * u, u, P2), e2 = FMA(e1, u, Q1), fu = FMA(e2, u, S0);
      const REAL g1 = FMA(A4x4 * u, u, P2x2), du = FMA(g1, u, Q1);
      const REAL st = fu / du;
      if(FABS(st) <= tol)
        u = u - st;
    }
    if(u >= lo && u <= hi && (!found || u < best)) { best = u; found = 1; }
  }
  *root_out = best;
  return found;
}

/* T2, second alternative solver: Ferrari's factorisation of the monic depressed quartic
 * u⁴ + p·u² + q·u + s = (u² - σu + p/2 + m + h)(u² + σu + p/2 + m - h), σ = sqrt(2m),
 * h = sign(q)·sqrt(m² + p·m + (p² - 4s)/4), where m >= 0 is a real root of the resolvent cubic
 * C(m) = m³ + p·m² + ((p² - 4s)/4)·m - q²/8.  Textbook Ferrari takes that root with cbrt/acos, which
 * no two maths libraries round alike; here C(0) <= 0 <= C(Cauchy bound) brackets a root, a FIXED
 * number of bisections (every lane the same trip count; Newton from the bound stalls when the
 * cubic's complex pair lies to the right of its real root) narrows the bracket to rounding, and two
 * guarded Newton steps finish; h is formed from the cubic identity q² = 8m(m² + pm + (p² - 4s)/4)
 * instead of q/(2σ), which has no division by a vanishing σ.  Only + - * / sqrt fma: the HIP
 * kernels reproduce it bit for bit.  The four candidates get the same two guarded Newton steps as
 * Durand–Kerner's, and the smallest inside [lo,hi] is returned.  Weakness (DESIGN.md §4): "is this
 * root real" is the sign of a computed discriminant. */
#define TRT_FERRARI_STEPS (sizeof(REAL) == 4 ? 40 : 72)
static int SUF(ferrari_first_root)(REAL A4, REAL P2, REAL Q1, REAL S0, REAL inv_dd, REAL lo, REAL hi,
                                   REAL Rb2, REAL* root_out)
{
  const REAL iA4 = inv_dd * inv_dd;
  const REAL p = P2 * iA4, q = Q1 * iA4, s = S0 * iA4;
  const REAL sc  = SQRT(Rb2 * inv_dd);
  const REAL tol = TRT_DK_TOL * sc;
  const REAL c1  = FMA(p, p, (REAL)-4 * s) * (REAL)0.25;
  const REAL c0  = (q * q) * (REAL)-0.125;
  REAL mlo = (REAL)0, mhi = (REAL)1 + FMAX(FABS(p), FMAX(FABS(c1), FABS(c0)));
  for(int it = 0; it < (int)TRT_FERRARI_STEPS; ++it)
  {
    const REAL mid = (REAL)0.5 * (mlo + mhi);
    const REAL r   = FMA(FMA(mid + p, mid, c1), mid, c0);
    if(r > (REAL)0) mhi = mid;
    else mlo = mid;
  }
  REAL m = (REAL)0.5 * (mlo + mhi);
  for(int it = 0; it < 2; ++it)
  {
    const REAL r  = FMA(FMA(m + p, m, c1), m, c0);
    const REAL dr = FMA(FMA((REAL)3, m, p + p), m, c1);
    const REAL mn = m - r / dr;
    if(dr > (REAL)0 && mn >= mlo && mn <= mhi)
      m = mn;
  }
  const REAL sg = SQRT(m + m);
  const REAL h2 = FMA(m + p, m, c1);
  const REAL h  = (q < (REAL)0 ? (REAL)-1 : (REAL)1) * SQRT(FMAX(h2, (REAL)0));
  const REAL e  = FMA((REAL)0.5, p, m);
  /* discriminants of the two quadratics: σ² - 4(e ± h) */
  const REAL d1 = FMA((REAL)-4, e + h, sg * sg), d2 = FMA((REAL)-4, e - h, sg * sg);
  REAL cand[4];
  int  nc = 0;
  if(d1 >= (REAL)0)
  {
    const REAL w = SQRT(d1);
    cand[nc++] = (REAL)0.5 * (sg - w);
    cand[nc++] = (REAL)0.5 * (sg + w);
  }
  if(d2 >= (REAL)0)
  {
    const REAL w = SQRT(d2);
    cand[nc++] = (REAL)0.5 * (-sg - w);
    cand[nc++] = (REAL)0.5 * (-sg + w);
  }
  int  found = 0;
  REAL best  = (REAL)0;
  const REAL A4x4 = (REAL)4 * A4, P2x2 = (REAL)2 * P2;
  for(int k = 0; k < nc; ++k)
  {
    REAL u = cand[k];
    for(int n = 0; n < 2; ++n)
    {
      const REAL e1 = FMA(A4 * u, u, P2), e2 = FMA(e1, u, Q1), fu = FMA(e2, u, S0);
      const REAL g1 = FMA(A4x4 * u, u, P2x2), du = FMA(g1, u, Q1);
      const REAL st = fu / du;
      if(FABS(st) <= tol)
        u = u - st;
    }
    if(u >= lo && u <= hi && (!found || u < best)) { best = u; found = 1; }
  }
  *root_out = best;
  return found;
}

/* Smallest t in (tmin,tmax) with the ray o + t·d on the torus.  dd = d·d, inv_dd = 1/dd.
 * Returns 1 and *t_out on a hit, 0 on a miss.  *evals counts polynomial evaluations. */
static int SUF(torus_first_hit)(const REAL o[3], const REAL d[3], REAL dd, REAL inv_dd,
                                REAL tmin, REAL tmax, const SUF(torus_k)* T, int dk, REAL* t_out,
                                int* evals)
{
  /* T1: closest approach to the centre, cull, window */
  const REAL ex = o[0] - T->cx, ey = o[1] - T->cy, ez = o[2] - T->cz;
  const REAL n  = FMA(ez, d[2], FMA(ey, d[1], ex * d[0]));
  const REAL tc = -n * inv_dd;
  REAL qx = FMA(tc, d[0], ex), qy = FMA(tc, d[1], ey), qz = FMA(tc, d[2], ez);
  const REAL m  = FMA(qz, qz, FMA(qy, qy, qx * qx));
  if(!(m <= T->Rb2))
    return 0;
  /* T1a: second shift.  tc carries a rounding error of ~|tc|·eps, so q·d is not 0 — but the quartic below is formed as if
   * it were (no u³ term): far from the torus (|tc|·|d| >> R) the dropped terms move the roots by ~|tc|·|d|·eps.  One
   * more step of the same shift, by tc2 = -(q·d)/dd, leaves q ⟂ d to the rounding of q itself; tc2 stays a separate
   * (small) term of t = u + tc + tc2, summed with one rounding at the size of t (below).  After the cull, which most
   * tests do not pass: m, the cull and the window feel q·d only through (q·d)²/dd and a shift of the window's ends by
   * tc2, far inside the margins by which sphere and slab are inflated. */
  /* Taken wherever the dropped terms can reach a sixteenth of what f is worth where the walk starts.  They are worth
   * ≈16·R³·δ, δ = |tc|·|d|·2⁻²⁴ the error of the first shift as a length; f on the inflated slab is ≈R²r²/32
   * (DESIGN.md §4): 16·R³·δ > R²r²/512 is |tc|·|d| > 2¹¹·r²/R, written (n²/dd)·4R² > 2²⁴·(r²)² — 0.8 R for r/R = 0.02,
   * 5 R for 0.05, 128 R for 0.25.  Below that the step changes nothing that survives rounding and is not taken: tc2 = 0
   * leaves q and t = u + tc as they are.  (The FP64 solve takes it at the same distance, sooner than it needs to.) */
  REAL tc2 = (REAL)0;
  if(((n * n) * inv_dd) * T->fourR2 > (REAL)16777216 * (T->r2 * T->r2))
  {
    const REAL n2 = FMA(qz, d[2], FMA(qy, d[1], qx * d[0]));
    tc2 = -n2 * inv_dd;
    qx = FMA(tc2, d[0], qx); qy = FMA(tc2, d[1], qy); qz = FMA(tc2, d[2], qz);
  }
  const REAL U  = SQRT((T->Rb2 - m) * inv_dd);
  REAL lo = FMAX(tmin - tc, -U);
  REAL hi = FMIN(tmax - tc, U);
  if(!(lo < hi))
    return 0;

  const REAL a     = FMA(d[2], d[2], d[0] * d[0]);
  const REAL b     = FMA(qz, d[2], qx * d[0]);
  const REAL c     = FMA(qz, qz, qx * qx);
  /* T1b: clip the window to the bounding slab |y| <= rs (slightly inflated, like the sphere, so that the walk still
   * starts strictly outside the torus).  Sphere ∩ slab holds only ≈1.5·r/(R+r) of the sphere's volume: most rays that
   * pass the sphere but miss the torus end here without a single Newton step, and the others start next to the
   * surface.  (No clip to the bounding cylinder of the same radius: with q ⟂ d, sphere(u) − cylinder(u) =
   * (dy·u + qy)² >= 0 — the sphere's interval always lies inside the cylinder's.) */
  if(d[1] != (REAL)0)
  {
    const REAL iy = (REAL)1 / d[1];
    const REAL u0 = (-T->rs - qy) * iy, u1 = (T->rs - qy) * iy;
    lo = FMAX(lo, FMIN(u0, u1));
    hi = FMIN(hi, FMAX(u0, u1));
  }
  else if(!(FABS(qy) <= T->rs))
    return 0;
  if(!(lo < hi))
    return 0;
  const REAL kappa = m + T->k0;
  const REAL A4    = dd * dd;
  const REAL P2    = FMA(-T->fourR2, a, ((REAL)2 * dd) * kappa);
  const REAL Q1    = ((REAL)-2 * T->fourR2) * b;
  const REAL S0    = FMA(-T->fourR2, c, kappa * kappa);
  const REAL A4x4  = (REAL)4 * A4;
  const REAL P2x2  = (REAL)2 * P2;

  /* T2: pieces of constant sign of f'' */
  const int  split = P2 < (REAL)0;
  const REAL k6    = (inv_dd * inv_dd) * (REAL)(1.0 / 6.0); /* 1/(6·A4) without a division */
  const REAL w     = split ? SQRT(-P2 * k6) : (REAL)0;

  REAL A = lo, fa, da;
  TRT_EVAL(A, fa, da);
  int  ne    = 1;
  int  found = 0;
  REAL root  = (REAL)0;

  if(dk == 2)
  {
    found = SUF(ferrari_first_root)(A4, P2, Q1, S0, inv_dd, lo, hi, T->Rb2, &root);
    ne    = (int)TRT_FERRARI_STEPS;
  }
  else if(dk)
  {
    found = SUF(dk_first_root)(A4, P2, Q1, S0, inv_dd, lo, hi, T->Rb2, &root);
    ne    = 4 * TRT_DK_SWEEPS;
  }
  else for(;;)
  {
    REAL B;
    int  sigma;
    if(split && A < -w)      { B = FMIN(-w, hi); sigma = +1; }
    else if(split && A < w)  { B = FMIN(w, hi);  sigma = -1; }
    else                     { B = hi;           sigma = +1; }
    /* Newton stops once a step is below 2^-12 (FP32; 2^-24 FP64) of the piece: quadratic
     * convergence puts the iterate within ~step²/r of the root, far inside the range where the
     * single geometric Newton step of T2b finishes the job — the one or two evaluations that
     * used to confirm the fixed point are not spent (3.4 instead of 4.7 per hit). */
    const REAL ustop = (B - A) * TRT_USTOP;

    if(fa == (REAL)0) { found = 1; root = A; break; } /* a piece end that is itself a root */
    const int sa = (fa > (REAL)0) ? +1 : -1;
    REAL fb, db;
    if(sa == sigma)
    {
      /* forward: Newton from A; monotone while a root lies ahead */
      REAL x = A, fx = fa, dx = da;
      int  noroot = 0;
      for(int it = 0; it < TRT_NEWTON_CAP; ++it)
      {
        if(!((REAL)sigma * dx < (REAL)0)) { noroot = 1; break; }
        const REAL st = fx / dx;
        const REAL xn = x - st;
        if(!(xn < B)) { noroot = 1; break; }
        if(xn == x) break;
        x = xn;
        if(FABS(st) <= ustop) break; /* within the capture range of the geometric polish (T2b) */
        TRT_EVAL(x, fx, dx);
        ++ne;
        if(fx == (REAL)0 || ((fx > (REAL)0) ? +1 : -1) != sa) break;
      }
      if(!noroot) { found = 1; root = x; break; }
      TRT_EVAL(B, fb, db);
      ++ne;
    }
    else
    {
      TRT_EVAL(B, fb, db);
      ++ne;
      const int sb = (fb > (REAL)0) ? +1 : (fb < (REAL)0) ? -1 : sigma;
      if(sb == sigma)
      {
        /* backward: exactly one root in the piece; Newton from B moves left onto it */
        REAL x = B, fx = fb, dx = db;
        for(int it = 0; it < TRT_NEWTON_CAP; ++it)
        {
          if(fx == (REAL)0 || ((fx > (REAL)0) ? +1 : -1) != sb) break;
          if(!((REAL)sigma * dx > (REAL)0)) break;
          const REAL st = fx / dx;
          const REAL xn = x - st;
          if(!(xn > A)) { x = A; break; }
          if(xn == x) break;
          x = xn;
          if(FABS(st) <= ustop) break;
          TRT_EVAL(x, fx, dx);
          ++ne;
        }
        found = 1;
        root  = x;
        break;
      }
    }
    if(!(B < hi))
      break;
    A  = B;
    fa = fb;
    da = db;
  }
  if(evals) *evals += ne;
  if(!found)
    return 0;
  /* T2b: one Newton step on the geometric form g(u) = (ρ-R)² + py² - r² (ρ = distance from
   * the axis).  g has the same roots as f but its rounding error scales with r², not R⁴,
   * which matters for thin tubes.  A step that would move the point by more than r/32 (grazing: g' ≈ 0) is
   * discarded: |du|·|d| <= r/32, compared as squares — du is a step in the ray PARAMETER, r/32 a length. */
  {
    const REAL px  = FMA(root, d[0], qx), py = FMA(root, d[1], qy), pz = FMA(root, d[2], qz);
    const REAL rho = SQRT(FMA(pz, pz, px * px));
    const REAL e   = rho - T->R;
    const REAL g   = FMA(e, e, FMA(py, py, -T->r2));
    const REAL s   = FMA(pz, d[2], px * d[0]);
    const REAL gh  = FMA(e, s, (py * d[1]) * rho); /* ρ·g'/2 */
    const REAL du  = (REAL)0.5 * ((g * rho) / gh);
    if((du * du) * dd <= T->rpol2)
      root = root - du;
  }
  /* t = u + tc + tc2 with ONE rounding at the size of t, as u + tc had before the second shift: the rounding error of
   * s = big + small is exact in e (Fast2Sum, |big| >= |small|) and joins the small second shift before the last add */
  const int  far = FABS(root) < FABS(tc);
  const REAL big = far ? tc : root, small = far ? root : tc;
  const REAL s   = big + small;
  const REAL e   = small - (s - big);
  const REAL t   = s + (e + tc2);
  if(!(t > tmin && t < tmax))
    return 0;
  *t_out = t;
  return 1;
}

#undef TRT_EVAL
