// trt_device.hpp — device-side arithmetic of the toroidal ray tracer (gfx950 / CDNA4).
//
// Everything a lane needs to answer "where does this ray first meet this torus", plus the
// closest-hit / miss / shadow-miss shader bodies of the reference restated for an analytic
// torus.  Reference paths are relative to vk_raytracing_tutorial_KHR/
// (REFL = ray_tracing_reflections, BEF = ray_tracing__before).
//
// Arithmetic contract: only IEEE-754 correctly rounded operations
// (+ - * / sqrt fma), every fused multiply-add spelled out, translation unit compiled with
// -ffp-contract=off.  hipcc lowers `/` and sqrtf() to correctly rounded sequences by
// default (-fhip-fp32-correctly-rounded-divide-sqrt), so the results are reproducible on
// any IEEE machine; tests/ check them bit for bit against a CPU restatement.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/trt.h"

namespace trt {

// ------------------------------------------------------------------------------------------
// scalar helpers, float / double
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float  fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float  sqrt_(float a) { return sqrtf(a); }
__device__ __forceinline__ double sqrt_(double a) { return sqrt(a); }
__device__ __forceinline__ float  max_(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double max_(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float  min_(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double min_(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float  abs_(float a) { return fabsf(a); }
__device__ __forceinline__ double abs_(double a) { return fabs(a); }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }   // (min(int, uint32_t) resolves to the double overload)

// Timing ablations (skip the CLEAR or the LIVE part of a frame, phases of the re-projection) exist in -DTRT_TUNING builds
// only: the release library has no switch that returns an incomplete image with TRT_OK.
#ifdef TRT_TUNING
#define TRT_SKIP(a, bit) ((a).debug_skip & (bit))
#else
#define TRT_SKIP(a, bit) false
#endif

struct v3 { float x, y, z; };

__device__ __forceinline__ float dot3(v3 a, v3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ v3 sub3(v3 a, v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ v3 scale3(v3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ v3 neg3(v3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ v3 normalize3(v3 a) { return scale3(a, 1.0f / sqrt_(dot3(a, a))); }
// GLSL reflect(I,N) = I - 2·dot(N,I)·N   (REFL/shaders/raytrace.rchit:148)
__device__ __forceinline__ v3 reflect3(v3 i, v3 n)
{
  const float k = 2.0f * dot3(n, i);
  return {fma_(-k, n.x, i.x), fma_(-k, n.y, i.y), fma_(-k, n.z, i.z)};
}
// column-major mat4 · (x,y,z,w), rows 0..2
__device__ __forceinline__ v3 mat4_mul(const float* m, float x, float y, float z, float w)
{
  v3 r;
  r.x = fma_(m[12], w, fma_(m[8], z, fma_(m[4], y, m[0] * x)));
  r.y = fma_(m[13], w, fma_(m[9], z, fma_(m[5], y, m[1] * x)));
  r.z = fma_(m[14], w, fma_(m[10], z, fma_(m[6], y, m[2] * x)));
  return r;
}

// ------------------------------------------------------------------------------------------
// scene as the kernels see it (built on the host by trt_api.hip, staged into LDS per block)
// ------------------------------------------------------------------------------------------
template <class Real>
struct TorusK {   // per-torus constants of the solver
  Real cx, cy, cz;
  Real R;
  Real r2;      // r²
  Real rpol2;   // (r/32)²: square of the largest distance the geometric polish may move the point
  Real k0;      // R² - r²
  Real Rb2;     // (R+r)²·(1+2⁻⁹): squared radius of the slightly inflated bounding sphere
  Real rs;      // r·(1+2⁻⁸): half height of the slightly inflated bounding slab |y| <= rs
  Real fourR2;  // 4R²
};

struct TorusShade {  // what the closest-hit stage needs: centre, R, material index
  float cx, cy, cz, R;
  int   matId;
};

// World → torus-frame rotation of an oriented torus, row-major: rows u, a, w with a the unit axis of symmetry and
// (u, a, w) right-handed, so that the torus turns about the frame's +y like every other one (the frame rule is
// trt_api.hip: torus_frame).  local = m · world; m is orthonormal to FP32 rounding, its transpose rotates back.
struct TorusRot { float m[9]; };

struct MaterialK {  // the WaveFrontMaterial fields the Phong model reads (rchit:95-155)
  float ambient[3];
  float diffuse[3];
  float specular[3];
  float shininess;
  int   illum;
};

// SceneK::alt_solver.  The kernels take the walk as ALT = false and both alternatives as ALT = true, choosing between
// them wave-uniformly at run time (torus_first_hit).
enum AltSolver : int { kSolverWalk = 0, kSolverDurandKerner = 1, kSolverFerrari = 2 };

struct SceneK {
  int            n_tori;
  int            n_mat;
  int            f64;   // 1: FP64 root solve (BASELINE config 4), FP32 I/O
  int            alt_solver;   // AltSolver: the Fourier–Newton walk, or an alternative root solver (kernels with ALT = true)
  int            order[TRT_MAX_TORI];  // test order: descending bounding radius R + r, ties by index
  uint32_t       inside[TRT_MAX_TORI]; // inside[i]: the tori whose tube lies strictly inside torus i's tube, as a mask over TEST-ORDER
                                       // positions (bit k = order[k]) — what a ray that leaves i's surface outwards cannot hit first;
                                       // empty when another torus cuts through i's tube or comes within tMin of it (trt_api.hip cull_keeps_clear)
  uint32_t       oriented;             // bit i: torus i turns about an axis other than +y (trt_set_torus_axes) and has a TorusRot record;
                                       // zero: the scene runs the kernels without ORIENT, which know nothing of all this
  uint32_t       reserved;
  TorusK<float>  k32[TRT_MAX_TORI];
  TorusK<double> k64[TRT_MAX_TORI];
  TorusShade     shade[TRT_MAX_TORI];
  MaterialK      mat[TRT_MAX_MATERIALS];
  TorusRot       rot[TRT_MAX_TORI];    // read for the tori of `oriented` only
};

// Copy the scene constants from the kernel-argument segment into LDS — only the records in use
// (header + test order + enclosure masks, n_tori solver records of the active precision, n_tori shading records,
// n_mat materials, and — in the ORIENT kernels, which run only when some torus is oriented — n_tori rotation records):
// 48 dwords for one FP32 torus instead of the 462 of the full struct, one load per thread.
// Reads in the hot loops then hit LDS at wave-uniform (broadcast) or material-indexed addresses.
// (trt_media.hip has a second staging routine, stage_scene_no_mat, for a SceneK that travels without its materials: a
// change to SceneK's layout or to the words below has to be made there too.)
// The dwords of a SceneK that are in use, numbered 0 .. scene_words() - 1: word i of them sits at dword scene_word(i) of the struct.
constexpr uint32_t kSceneHdr = 22, kSceneK32 = kSceneHdr, kSceneK64 = kSceneK32 + 80, kSceneShade = kSceneK64 + 160, kSceneMat = kSceneShade + 40,
                   kSceneRot = kSceneMat + 88;
template <bool ORIENT = false>
__device__ __forceinline__ uint32_t scene_words(const SceneK& arg)
{
  return kSceneHdr + (arg.f64 ? 20u : 10u) * (uint32_t)arg.n_tori + 5u * (uint32_t)arg.n_tori + 11u * (uint32_t)arg.n_mat
         + (ORIENT ? 9u * (uint32_t)arg.n_tori : 0u);
}
template <bool ORIENT = false>
__device__ __forceinline__ uint32_t scene_word(const SceneK& arg, uint32_t i)
{
  const uint32_t n = (uint32_t)arg.n_tori;
  const uint32_t c0 = kSceneHdr, c1 = c0 + (arg.f64 ? 0u : 10u * n), c2 = c1 + (arg.f64 ? 20u * n : 0u), c3 = c2 + 5u * n;
  if(ORIENT)
  {
    const uint32_t c4 = c3 + 11u * (uint32_t)arg.n_mat;
    if(i >= c4) return kSceneRot + (i - c4);
  }
  return i < c0 ? i : i < c1 ? kSceneK32 + (i - c0) : i < c2 ? kSceneK64 + (i - c1) : i < c3 ? kSceneShade + (i - c2) : kSceneMat + (i - c3);
}
template <bool ORIENT = false>
__device__ __forceinline__ void stage_scene(SceneK* lds, const SceneK& arg)
{
  static_assert(sizeof(SceneK) == 4 * (kSceneRot + 72) && sizeof(TorusK<float>) == 40 && sizeof(TorusShade) == 20
                    && sizeof(MaterialK) == 44 && sizeof(TorusRot) == 36 && offsetof(SceneK, k32) == 4 * kSceneK32
                    && offsetof(SceneK, k64) == 4 * kSceneK64 && offsetof(SceneK, shade) == 4 * kSceneShade
                    && offsetof(SceneK, mat) == 4 * kSceneMat && offsetof(SceneK, rot) == 4 * kSceneRot, "SceneK layout");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&arg);
  uint32_t*       dst = reinterpret_cast<uint32_t*>(lds);
  const uint32_t  c4 = scene_words<ORIENT>(arg);
  for(uint32_t i = threadIdx.x; i < c4; i += blockDim.x)
  {
    const uint32_t off = scene_word<ORIENT>(arg, i);
    dst[off] = src[off];
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------
// T1 + T2: first root of the ray–torus quartic in (tmin, tmax)
// ------------------------------------------------------------------------------------------
// Depressed quartic in u = t - tc (tc = parameter of closest approach to the torus centre):
//   f(u) = A4 u⁴ + P2 u² + Q1 u + S0,  A4 = dd², P2 = 2·dd·κ - 4R²a, Q1 = -8R²b, S0 = κ² - 4R²c
// f'' has constant sign on ≤3 pieces of the window (split at ±w); on each piece Newton's
// iteration started where sign f = sign f'' is monotone (Fourier), so walking the pieces
// left to right finds the smallest root or proves there is none.  The walk is written as
// ONE loop whose every trip evaluates (f, f') at one point per lane — the lanes of a wave
// stay convergent on the evaluation and the division although they sit in different
// pieces/modes.
enum : int { M_FWD = 0, M_BWD = 1, M_PROBE = 2, M_END = 3, M_DONE = 4 };
constexpr int kNewtonCap = 48;
// Newton's early stop, as a fraction of the piece: 2^-12 (FP32), 2^-24 (FP64)
template <class Real> struct StepStop;
template <> struct StepStop<float> { static constexpr float v = 0.000244140625f; };
template <> struct StepStop<double> { static constexpr double v = 5.9604644775390625e-08; };

// One ray-vs-torus test as a resumable state machine: setup() does T1 (returns false when the
// bounding sphere / parameter window culls the ray), every step() evaluates (f, f') once and
// advances the walk (returns false when the test is decided), finish() polishes the root and
// applies the open interval (tmin, tmax).  A lane can park a TorusTest in registers between
// step() calls — the persistent kernel relies on that.
template <class Real>
struct TorusTest {
  // quartic and window
  Real A4, P2, Q1, S0, w, hi, tc, tc2;   // t = u + tc + tc2: the shift and its second, small step (setup)
  Real qx, qy, qz;     // point of closest approach to the torus centre (local frame)
  Real dsq;            // |d|² as setup() was given it (finish_root: the polish guard)
  // walk: piece [A,B] with sign(f'') = sigma; xe = point to evaluate next (END/PROBE: xe == B)
  Real A, B, xe, root;
  int  sigma, sref, it, mode;
  bool split, found;
  static constexpr Real kStepStop = StepStop<Real>::v;

  __device__ __forceinline__ bool setup(Real ox, Real oy, Real oz, Real dx_, Real dy_, Real dz_,
                                        Real dd, Real inv_dd, Real tmin, Real tmax,
                                        const TorusK<Real>& T)
  {
    const Real ex = ox - T.cx, ey = oy - T.cy, ez = oz - T.cz;
    const Real n  = fma_(ez, dz_, fma_(ey, dy_, ex * dx_));
    dsq = dd;
    tc = -n * inv_dd;
    qx = fma_(tc, dx_, ex); qy = fma_(tc, dy_, ey); qz = fma_(tc, dz_, ez);
    const Real m = fma_(qz, qz, fma_(qy, qy, qx * qx));
    mode = M_DONE;
    found = false;
    if(!(m <= T.Rb2))
      return false;
    // T1a: second shift.  tc carries a rounding error of ~|tc|·eps, so q·d is not 0 — but the quartic is formed as if it
    // were (no u³ term): far from the torus the dropped terms move the roots by ~|tc|·|d|·eps.  One more step of the same
    // shift, by tc2 = -(q·d)/dd, leaves q ⟂ d to the rounding of q itself; tc2 stays a separate (small) term of
    // t = u + tc + tc2 (finish_root).  After the cull, which most tests do not pass: m, the cull and the window feel q·d
    // only through (q·d)²/dd and a shift of the window's ends by tc2, far inside the margins of sphere and slab.
    // Taken wherever the dropped terms can reach a sixteenth of what f is worth where the walk starts.  They are worth
    // ≈16·R³·δ, δ = |tc|·|d|·2⁻²⁴ the error of the first shift as a length; f on the inflated slab is ≈R²r²/32:
    // 16·R³·δ > R²r²/512 is |tc|·|d| > 2¹¹·r²/R, written (n²/dd)·4R² > 2²⁴·(r²)² — 0.8 R for r/R = 0.02, 5 R for 0.05, 128 R
    // for 0.25.  Below that the step changes nothing that survives rounding and is not taken: tc2 = 0 leaves q and
    // t = u + tc as they are.  (The FP64 solve takes it at the same distance, sooner than it needs to.)
    tc2 = Real(0);
    if(((n * n) * inv_dd) * T.fourR2 > Real(16777216) * (T.r2 * T.r2))
    {
      const Real n2 = fma_(qz, dz_, fma_(qy, dy_, qx * dx_));
      tc2 = -n2 * inv_dd;
      qx = fma_(tc2, dx_, qx); qy = fma_(tc2, dy_, qy); qz = fma_(tc2, dz_, qz);
    }
    const Real U  = sqrt_((T.Rb2 - m) * inv_dd);
    Real lo = max_(tmin - tc, -U);
    hi = min_(tmax - tc, U);
    if(!(lo < hi))
      return false;
    const Real a     = fma_(dz_, dz_, dx_ * dx_);
    const Real b     = fma_(qz, dz_, qx * dx_);
    const Real c     = fma_(qz, qz, qx * qx);
    // T1b: clip the window to the bounding slab |y| <= rs (slightly inflated, like the sphere, so that the walk still
    // starts strictly outside the torus).  Sphere ∩ slab holds only ≈1.5·r/(R+r) of the sphere's volume: most rays that
    // pass the sphere but miss the torus end here without a single Newton step, and the others start next to the surface.
    // (Round 1 also clipped to the bounding CYLINDER of the same radius — a square root and a division per test for
    // nothing: with q ⟂ d, sphere(u) − cylinder(u) = (dy·u + qy)² >= 0, so the sphere's interval always lies inside the
    // cylinder's.)
    if(dy_ != Real(0))
    {
      const Real inv_dy = Real(1) / dy_;
      const Real u0 = (-T.rs - qy) * inv_dy, u1 = (T.rs - qy) * inv_dy;
      lo = max_(lo, min_(u0, u1));
      hi = min_(hi, max_(u0, u1));
    }
    else if(!(abs_(qy) <= T.rs))
      return false;
    if(!(lo < hi))
      return false;
    const Real kappa = m + T.k0;
    A4    = dd * dd;
    P2    = fma_(-T.fourR2, a, (Real(2) * dd) * kappa);
    Q1    = (Real(-2) * T.fourR2) * b;
    S0    = fma_(-T.fourR2, c, kappa * kappa);
    split = P2 < Real(0);
    const Real k6 = (inv_dd * inv_dd) * Real(1.0 / 6.0);  // 1/(6·A4) without a division
    w     = split ? sqrt_(-P2 * k6) : Real(0);
    A = lo; B = lo; xe = lo; root = Real(0);
    sigma = 1; sref = 1; it = 0; mode = M_END;
    return true;
  }

  // (f, f') at u, the one statement of the quartic: Horner with every multiply-add fused.  A caller that
  // evaluates more than once forms 4·A4 and 2·P2 first and passes them in; the others use the short form.
  // The value is the same: ×4 and ×2 are exact, so (4·A4)·u has one rounding wherever 4·A4 was formed.
  __device__ __forceinline__ void eval(Real u, Real A4x4, Real P2x2, Real& f, Real& d) const
  {
    const Real e1 = fma_(A4 * u, u, P2);
    const Real e2 = fma_(e1, u, Q1);
    f = fma_(e2, u, S0);
    const Real g1 = fma_(A4x4 * u, u, P2x2);
    d = fma_(g1, u, Q1);
  }
  __device__ __forceinline__ void eval(Real u, Real& f, Real& d) const { eval(u, Real(4) * A4, Real(2) * P2, f, d); }

  // One evaluation of (f, f') at xe, then the transitions of the walk — written as straight-
  // line predicated code (compares + selects, one division) so that the lanes of a wave, which
  // sit in different pieces and modes, execute ONE instruction stream per trip.
  // Returns true while the test is undecided.
  //
  //   END    xe == B was evaluated after a forward run found no root in [A,B]: next piece.
  //   PROBE  xe == B was evaluated because sign f(A) = -sigma: a root exists in the piece iff
  //          sign f(B) = sigma; then iterate backward from B, else next piece.
  //   FWD    Newton from the left end; monotone while a root lies ahead, otherwise sigma·f'
  //          turns >= 0 or the iterate leaves the piece (-> END).
  //   BWD    Newton from the right end onto the single root of the piece.
  __device__ __forceinline__ bool step()
  {
    const Real u  = xe;
    Real fe, de;
    eval(u, fe, de);

    const bool mEnd = mode == M_END, mProbe = mode == M_PROBE, mFwd = mode == M_FWD, mBwd = mode == M_BWD;
    const bool pos = fe > Real(0), neg = fe < Real(0), zer = fe == Real(0);
    const int  sfe = pos ? 1 : -1;
    const int  sb  = pos ? 1 : (neg ? -1 : sigma);

    // leaving the piece at B (END, or PROBE without a sign change) / entering the next one
    const bool probe_ok = mProbe && sb == sigma;
    const bool leave    = mEnd || (mProbe && !probe_ok);
    const bool more     = B < hi;
    const bool enter    = leave && more;
    const bool c1 = split && B < -w, c2 = split && B < w;
    const Real Bn = c1 ? min_(-w, hi) : (c2 ? min_(w, hi) : hi);
    const int  sn = (c2 && !c1) ? -1 : 1;
    const bool e_hit = enter && zer;                 // the piece end is itself a root
    const bool e_fwd = enter && !zer && sfe == sn;
    const bool e_prb = enter && !zer && sfe != sn;

    const Real A2     = enter ? B : A;
    const Real B2     = enter ? Bn : B;
    const int  sigma2 = enter ? sn : sigma;
    const int  sref2  = enter ? sfe : (probe_ok ? sb : sref);
    const int  it2    = (mFwd || mBwd) ? it + 1 : 0;

    // Newton step from u (the current iterate is always the point just evaluated)
    const bool f_flip = mFwd && (zer || sfe != sref);      // rounding carried f across zero
    const bool isF    = (mFwd && !f_flip) || e_fwd;
    const bool isB    = mBwd || probe_ok;
    const bool cap    = (isF || isB) && it2 == kNewtonCap;
    const Real sdx    = sigma2 > 0 ? de : -de;
    const Real st     = fe / de;
    const Real xn     = u - st;
    // Newton stops once a step is below 2^-12 (FP32; 2^-24 FP64) of the piece: the iterate is
    // then within ~step²/r of the root, far inside the capture range of finish()'s geometric
    // step — the one or two evaluations that used to confirm the fixed point are not spent
    const bool small  = abs_(st) <= (B2 - A2) * kStepStop;
    const bool f_no   = isF && !cap && (!(sdx < Real(0)) || !(xn < B2));  // no root in [u,B]
    const bool f_cv   = isF && !cap && !f_no && xn == u;
    const bool f_es   = isF && !cap && !f_no && xn != u && small;
    const bool b_stop = (zer || sfe != sref2) || !(sdx > Real(0));
    const bool b_left = !(xn > A2);
    const bool b_hitx = isB && !cap && (b_stop || (!b_left && xn == u));
    const bool b_hitA = isB && !cap && !b_stop && b_left;
    const bool b_es   = isB && !cap && !b_stop && !b_left && xn != u && small;
    const bool go     = (isF && !cap && !f_no && !f_cv && !f_es) || (isB && !cap && !b_stop && !b_left && xn != u && !b_es);

    const bool hit_x = e_hit || f_flip || cap || f_cv || b_hitx;
    const bool hit_n = f_es || b_es;   // accepted at the new iterate
    // a forward run that proves "no root" in the LAST piece decides the test: nothing is
    // evaluated at hi any more (that evaluation carried no information)
    const bool last_no = f_no && !(B2 < hi);
    const bool done  = (leave && !more) || hit_x || hit_n || b_hitA || last_no;
    found = hit_x || hit_n || b_hitA;
    root  = b_hitA ? A2 : (hit_n ? xn : u);
    A = A2; B = B2; sigma = sigma2; sref = sref2; it = it2;
    xe   = (e_prb || f_no) ? B2 : (go ? xn : u);
    mode = done ? M_DONE : (e_prb ? M_PROBE : (f_no ? M_END : (isF ? M_FWD : M_BWD)));
    return !done;
  }

  // step() for a lane that is iterating (mode FWD or BWD): the same arithmetic and the same
  // decisions, minus every piece-transition term.  The solve loops take this path on the
  // trips in which no running lane of the wave sits at a piece end (wave-uniform choice).
  __device__ __forceinline__ bool step_iter()
  {
    const Real u  = xe;
    Real fe, de;
    eval(u, fe, de);
    const bool fwd  = mode == M_FWD;
    const bool flip = fe == Real(0) || ((fe > Real(0)) ? 1 : -1) != sref;
    const int  it2  = it + 1;
    const bool cap  = it2 == kNewtonCap;
    const Real sdx  = sigma > 0 ? de : -de;
    const Real st   = fe / de;
    const Real xn   = u - st;
    const bool small = abs_(st) <= (B - A) * kStepStop;
    // forward: flip -> hit, cap -> hit, slope/range -> END, converged -> hit, small step -> hit(xn)
    // backward: cap -> hit, flip/slope -> hit, left of A -> hit(A), converged -> hit, small step -> hit(xn)
    const bool f_no   = fwd && !flip && !cap && (!(sdx < Real(0)) || !(xn < B));
    const bool b_stop = flip || !(sdx > Real(0));
    const bool b_hitA = !fwd && !cap && !b_stop && !(xn > A);
    const bool hit_x  = fwd ? (flip || cap || (!f_no && xn == u))
                            : (cap || b_stop || (!b_hitA && xn == u));
    const bool hit_n  = !hit_x && !f_no && !b_hitA && small;
    const bool last_no = f_no && !(B < hi);   // "no root" in the last piece: the test is a miss
    const bool done   = hit_x || hit_n || b_hitA || last_no;
    found = hit_x || hit_n || b_hitA;
    root  = b_hitA ? A : (hit_n ? xn : u);
    it    = it2;
    xe    = f_no ? B : (done ? u : xn);
    mode  = done ? M_DONE : (f_no ? M_END : mode);
    return !done;
  }

  // true when step_iter() applies to this lane
  __device__ __forceinline__ bool iterating() const { return mode == M_FWD || mode == M_BWD; }

  // The same walk as step()/step_iter() — same evaluation points, same decisions, hence the same
  // root bit for bit — written as NESTED loops for a lane that owns its test from start to finish
  // (trace, listed and static kernels): an outer loop over the <= 3 pieces of constant sign of f'',
  // an inner Newton loop that serves the forward run (from A, while sign f = sigma) and the backward
  // run (from B, onto the single root of a piece with a sign change) with ONE body: a trip is the
  // evaluation, the division and five compares (~40 issue slots) instead of the ~170 of the general
  // transition table of step(), and the piece bookkeeping runs once per piece instead of once per
  // trip.  Lanes of a wave in different pieces still share the inner loop.  `evals` counts (f, f').
  // Call after a successful setup(); then finish().
  __device__ __forceinline__ void walk(uint32_t& evals)
  {
    const Real A4x4 = Real(4) * A4, P2x2 = Real(2) * P2;
    Real a = A, fa, da;          // setup() leaves the window start in A
    eval(a, A4x4, P2x2, fa, da);
    ++evals;
    found = false;
    root  = Real(0);
    mode  = M_DONE;
    for(;;)
    {
      const bool c1 = split && a < -w, c2 = split && a < w;
      const Real b  = c1 ? min_(-w, hi) : (c2 ? min_(w, hi) : hi);
      const Real sg = (c2 && !c1) ? Real(-1) : Real(1);          // sign of f'' on the piece
      if(fa == Real(0)) { found = true; root = a; break; }       // the piece end is itself a root
      const bool bwd = (fa > Real(0)) != (sg > Real(0));         // sign f(A) = -sigma: probe B
      Real x = a, fx = fa, dx = da;
      bool pos = fa > Real(0);                                   // the sign the run must keep
      bool run = true, noroot = false;
      if(bwd)
      {
        eval(b, A4x4, P2x2, fx, dx);
        ++evals;
        x = b;
        if(fx == Real(0)) { found = true; root = b; break; }     // (oracle: sb = sigma, first check of the run)
        pos = fx > Real(0);
        if(pos != (sg > Real(0))) { run = false; noroot = true; }  // no sign change: no root in the piece
      }
      if(run)
      {
        const Real ustop = (b - a) * kStepStop;
        const Real sd    = bwd ? -sg : sg;      // forward needs sigma·f' < 0, backward sigma·f' > 0
        const Real lim   = bwd ? -a : b;        // forward: xn < B; backward: xn > A  ⇔  -xn < -A
        for(int it = 0; it < kNewtonCap; ++it)
        {
          if(!(sd * dx < Real(0))) { noroot = !bwd; break; }                 // forward: no root ahead; backward: stop here
          const Real st = fx / dx;
          const Real xn = x - st;
          if(!((bwd ? -xn : xn) < lim)) { noroot = !bwd; if(bwd) x = a; break; }
          if(xn == x) break;
          x = xn;
          if(abs_(st) <= ustop) break;
          eval(x, A4x4, P2x2, fx, dx);
          ++evals;
          if(fx == Real(0) || (fx > Real(0)) != pos) break;
        }
        if(!noroot) { found = true; root = x; break; }
      }
      if(!(b < hi)) break;                       // that was the last piece: a miss
      if(!bwd) { eval(b, A4x4, P2x2, fx, dx); ++evals; }     // (a failed probe has evaluated B already)
      a = b; fa = fx; da = dx;
    }
  }

  // EVERY root of the window, left to right (trt_crossings): walk()'s evaluation points and decisions up to and including
  // the first root — u[0] is walk()'s `root` bit for bit — and then, instead of returning, the rest of the pieces.  A
  // piece of constant sign f'' = sigma holds at most two roots: after a forward run has found one, f is evaluated at B
  // (the next piece needs it anyway) and a second root exists exactly when sign f(B) = sigma; the backward run from B
  // finds it, bounded on the left by the first.  A piece entered with sign f(A) = -sigma holds one root or none, as in
  // walk().  A piece end that is itself a root (f = 0 exactly) is reported once, as the START of the next piece — at
  // `hi`, which has no next piece, by whoever evaluated it — and the piece then continues with the sign f takes just
  // right of it (that of f').  At most two runs per piece, each bounded by kNewtonCap; at most 4 roots are kept (a
  // quartic has no more; rounding cannot be allowed to write past u[3]).  Returns their number.
  // Call after a successful setup(); every root then goes through finish_root().
  __device__ __forceinline__ int walk_all(uint32_t& evals, Real (&u)[4])
  {
    const Real A4x4 = Real(4) * A4, P2x2 = Real(2) * P2;
    Real a = A, fa, da;          // setup() leaves the window start in A
    eval(a, A4x4, P2x2, fa, da);
    ++evals;
    int  n    = 0;
    auto push = [&](Real x) {    // (unrolled selects: u[] stays in registers)
#pragma unroll
      for(int k = 0; k < 4; ++k)
        if(k == n) u[k] = x;
      n = n < 4 ? n + 1 : n;
    };
    for(;;)
    {
      const bool c1 = split && a < -w, c2 = split && a < w;
      const Real b  = c1 ? min_(-w, hi) : (c2 ? min_(w, hi) : hi);
      const Real sg = (c2 && !c1) ? Real(-1) : Real(1);          // sign of f'' on the piece
      const bool zero = fa == Real(0);                           // the piece end is itself a root
      if(zero) push(a);
      const bool apos = zero ? da > Real(0) : fa > Real(0);      // sign of f on entering the piece
      const bool bwd  = apos != (sg > Real(0));                  // sign f(A) = -sigma: probe B
      Real fb = Real(0), db = Real(0);                           // (f, f') at B, once evaluated
      bool have_b = false;
      Real x = a, fx = fa, dx = da, left = a;                    // `left`: where a backward run stops
      bool pos  = apos;                                          // the sign the run must keep
      bool back = bwd;
      bool run  = !(zero && !bwd);   // leaving a root with sign f = sigma: f does not come back in this piece
      if(bwd)
      {
        eval(b, A4x4, P2x2, fb, db);
        ++evals;
        have_b = true;
        x = b; fx = fb; dx = db;
        pos = fb > Real(0);
        if(fb == Real(0)) { run = false; if(!(b < hi)) push(b); }
        else if(pos != (sg > Real(0))) run = false;              // no sign change: no root in the piece
      }
      const Real ustop = (b - a) * kStepStop;
      while(run)
      {
        const Real sd  = back ? -sg : sg;        // forward needs sigma·f' < 0, backward sigma·f' > 0
        const Real lim = back ? -left : b;       // forward: xn < B; backward: xn > left  ⇔  -xn < -left
        bool noroot = false;
        for(int it = 0; it < kNewtonCap; ++it)
        {
          if(!(sd * dx < Real(0))) { noroot = !back; break; }
          const Real st = fx / dx;
          const Real xn = x - st;
          if(!((back ? -xn : xn) < lim)) { noroot = !back; if(back) x = left; break; }
          if(xn == x) break;
          x = xn;
          if(abs_(st) <= ustop) break;
          eval(x, A4x4, P2x2, fx, dx);
          ++evals;
          if(fx == Real(0) || (fx > Real(0)) != pos) break;
        }
        if(noroot) break;                        // (forward runs only)
        push(x);
        if(back) break;                          // the last root of the piece
        eval(b, A4x4, P2x2, fb, db);             // a forward run found a root: is there a second one?
        ++evals;
        have_b = true;
        if(fb == Real(0)) { if(!(b < hi)) push(b); break; }
        if((fb > Real(0)) != (sg > Real(0))) break;
        back = true; left = x; x = b; fx = fb; dx = db; pos = fb > Real(0);
      }
      if(!(b < hi)) break;                       // that was the last piece
      if(!have_b) { eval(b, A4x4, P2x2, fb, db); ++evals; }
      a = b; fa = fb; da = db;
    }
    return n;
  }

  // What the two alternative solvers share.  Prologue: the monic depressed quartic u⁴ + p·u² + q·u + s, the scale sc
  // of its roots (the bounding-sphere radius in u), the tolerance tol = kAltTol·sc and the window start lo.
  static constexpr Real kAltTol = sizeof(Real) == 4 ? Real(0.0009765625) : Real(2.384185791015625e-07);  // 2^-10 / 2^-22
  struct Monic { Real p, q, s, sc, tol, lo; };
  __device__ __forceinline__ Monic monic(Real inv_dd, Real Rb2) const
  {
    const Real iA4 = inv_dd * inv_dd;
    const Real p = P2 * iA4, q = Q1 * iA4, s = S0 * iA4;
    const Real sc = sqrt_(Rb2 * inv_dd);
    return {p, q, s, sc, kAltTol * sc, A};   // setup() leaves the window start in A (= B = xe)
  }
  // Epilogue: every candidate that is real (ok(k), asked when its turn comes) gets two guarded Newton steps on the
  // quartic (a step above tol is discarded); the smallest one inside [lo, hi] becomes `root`.
  template <class IsReal>
  __device__ __forceinline__ void polish_and_select(const Real (&cand)[4], IsReal ok, Real lo, Real tol)
  {
    bool f = false;
    Real best = Real(0);
    const Real A4x4 = Real(4) * A4, P2x2 = Real(2) * P2;
#pragma unroll
    for(int k = 0; k < 4; ++k)
    {
      if(!ok(k))
        continue;
      Real u = cand[k];
#pragma unroll
      for(int n = 0; n < 2; ++n)
      {
        Real fu, du;
        eval(u, A4x4, P2x2, fu, du);
        const Real st = fu / du;
        if(abs_(st) <= tol)
          u = u - st;
      }
      if(u >= lo && u <= hi && (!f || u < best)) { best = u; f = true; }
    }
    found = f;
    root  = best;
    mode  = M_DONE;
  }

  // T2, alternative solver (TRT_SOLVE_DK_*): Durand–Kerner iteration on the monic depressed
  // quartic u⁴ + p·u² + q·u + s — four complex iterates from the spiral (0.4+0.9i)^k scaled by the
  // bounding-sphere radius, updated in place for a FIXED number of sweeps (every lane runs the
  // same trip count), only + - * / fma.  Real candidates (|Im| <= tol·scale) get two guarded
  // Newton steps; the smallest one inside [lo,hi] becomes `root`.  (tests/ compare it bit for bit
  // with a CPU restatement.)  Call after a successful setup(); then finish().
  __device__ __forceinline__ void solve_dk(Real inv_dd, Real Rb2)
  {
    constexpr int  kSweeps = 24;
    const Real CR[4] = {Real(1.0), Real(0.4), Real(-0.65), Real(-0.908)};
    const Real CI[4] = {Real(0.0), Real(0.9), Real(0.72), Real(-0.297)};
    const Monic mq = monic(inv_dd, Rb2);
    const Real  p = mq.p, q = mq.q, s = mq.s, sc = mq.sc;
    Real zr[4], zi[4];
#pragma unroll
    for(int k = 0; k < 4; ++k) { zr[k] = sc * CR[k]; zi[k] = sc * CI[k]; }
#pragma unroll 1
    for(int sweep = 0; sweep < kSweeps; ++sweep)
    {
#pragma unroll
      for(int k = 0; k < 4; ++k)
      {
        const Real x = zr[k], y = zi[k];
        const Real ar = fma_(x, x, -(y * y)) + p, ai = (x + x) * y;
        const Real br = fma_(ar, x, -(ai * y)) + q, bi = fma_(ar, y, ai * x);
        const Real fr = fma_(br, x, -(bi * y)) + s, fi = fma_(br, y, bi * x);
        Real dr = Real(1), di = Real(0);
#pragma unroll
        for(int j = 0; j < 4; ++j)
          if(j != k)
          {
            const Real er = x - zr[j], ei = y - zi[j];
            const Real nr = fma_(dr, er, -(di * ei)), ni = fma_(dr, ei, di * er);
            dr = nr; di = ni;
          }
        const Real den = fma_(dr, dr, di * di);
        if(den > Real(0) && den < Real(__builtin_inf()))
        {
          const Real inv = Real(1) / den;
          zr[k] = x - fma_(fr, dr, fi * di) * inv;
          zi[k] = y - fma_(fi, dr, -(fr * di)) * inv;
        }
      }
    }
    polish_and_select(zr, [&](int k) { return abs_(zi[k]) <= mq.tol; }, mq.lo, mq.tol);
  }

  // T2, second alternative solver (TRT_SOLVE_FERRARI_*): Ferrari's factorisation of the monic
  // depressed quartic into (u² - σu + e + h)(u² + σu + e - h), σ = sqrt(2m), e = p/2 + m,
  // h = sign(q)·sqrt(m² + pm + (p² - 4s)/4), m >= 0 a root of the resolvent cubic
  // m³ + pm² + ((p² - 4s)/4)m - q²/8 — bracketed by [0, Cauchy bound], narrowed by a FIXED number
  // of bisections (every lane the same trip count) and two guarded Newton steps, i.e. without the
  // cbrt/acos of the textbook form, only + - * / sqrt fma (bit for bit the CPU restatement of
  // tests/).  Candidates are polished and selected exactly as in solve_dk().
  __device__ __forceinline__ void solve_ferrari(Real inv_dd, Real Rb2)
  {
    constexpr int  kSteps = sizeof(Real) == 4 ? 40 : 72;
    const Monic mq = monic(inv_dd, Rb2);
    const Real  p = mq.p, q = mq.q, s = mq.s;
    const Real c1  = fma_(p, p, Real(-4) * s) * Real(0.25);
    const Real c0  = (q * q) * Real(-0.125);
    Real mlo = Real(0), mhi = Real(1) + max_(abs_(p), max_(abs_(c1), abs_(c0)));
#pragma unroll 1
    for(int i = 0; i < kSteps; ++i)
    {
      const Real mid = Real(0.5) * (mlo + mhi);
      const Real r   = fma_(fma_(mid + p, mid, c1), mid, c0);
      if(r > Real(0)) mhi = mid;
      else mlo = mid;
    }
    Real m = Real(0.5) * (mlo + mhi);
#pragma unroll
    for(int i = 0; i < 2; ++i)
    {
      const Real r  = fma_(fma_(m + p, m, c1), m, c0);
      const Real dr = fma_(fma_(Real(3), m, p + p), m, c1);
      const Real mn = m - r / dr;
      if(dr > Real(0) && mn >= mlo && mn <= mhi)
        m = mn;
    }
    const Real sg = sqrt_(m + m);
    const Real h2 = fma_(m + p, m, c1);
    const Real h  = (q < Real(0) ? Real(-1) : Real(1)) * sqrt_(max_(h2, Real(0)));
    const Real e  = fma_(Real(0.5), p, m);
    const Real d1 = fma_(Real(-4), e + h, sg * sg), d2 = fma_(Real(-4), e - h, sg * sg);
    const Real w1 = sqrt_(max_(d1, Real(0))), w2 = sqrt_(max_(d2, Real(0)));
    const Real cand[4] = {Real(0.5) * (sg - w1), Real(0.5) * (sg + w1), Real(0.5) * (-sg - w2), Real(0.5) * (-sg + w2)};
    const bool ok[4]   = {d1 >= Real(0), d1 >= Real(0), d2 >= Real(0), d2 >= Real(0)};
    polish_and_select(cand, [&](int k) { return ok[k]; }, mq.lo, mq.tol);
  }

  // T2b: one Newton step on g(u) = (ρ-R)² + py² - r², whose rounding error scales with r²
  // instead of R⁴ (a step that would move the point by more than r/32 — grazing, g' ≈ 0 — is discarded); then t = u + tc + tc2 and
  // the open-interval test of the closest-hit query.
  __device__ __forceinline__ bool finish(Real dx_, Real dy_, Real dz_, Real tmin, Real tmax,
                                         const TorusK<Real>& T, Real& t_out) const
  {
    Real gh;
    return found && finish_root(root, dx_, dy_, dz_, tmin, tmax, T, t_out, gh);
  }
  // The same for any root r of the walk (walk_all() returns several).  gh = ρ·g'/2 at the unpolished root, ρ > 0: the
  // sign of g' — negative where the ray goes from outside the tube (g > 0) to inside it.
  __device__ __forceinline__ bool finish_root(Real r, Real dx_, Real dy_, Real dz_, Real tmin, Real tmax,
                                              const TorusK<Real>& T, Real& t_out, Real& gh) const
  {
    const Real px  = fma_(r, dx_, qx), py = fma_(r, dy_, qy), pz = fma_(r, dz_, qz);
    const Real rho = sqrt_(fma_(pz, pz, px * px));
    const Real e   = rho - T.R;
    const Real g   = fma_(e, e, fma_(py, py, -T.r2));
    const Real s   = fma_(pz, dz_, px * dx_);
    gh             = fma_(e, s, (py * dy_) * rho);  // ρ·g'/2
    const Real du  = Real(0.5) * ((g * rho) / gh);
    // du is a step in the ray PARAMETER, r/32 a length: |du|·|d| <= r/32, compared as squares
    if((du * du) * dsq <= T.rpol2)
      r = r - du;
    // t = u + tc + tc2 with ONE rounding at the size of t, as u + tc had before the second shift: the rounding error of
    // s = big + small is exact in er (Fast2Sum, |big| >= |small|) and joins the small second shift before the last add
    const bool far = abs_(r) < abs_(tc);
    const Real big = far ? tc : r, small = far ? r : tc;
    const Real s2  = big + small;
    const Real er  = small - (s2 - big);
    const Real t   = s2 + (er + tc2);
    if(!(t > tmin && t < tmax))
      return false;
    t_out = t;
    return true;
  }
};

// Work counters of a lane (dead code in the kernels that do not store them): of the ray–torus
// tests a lane executed, how many passed TorusTest::setup (a quartic was built and walked) and how
// many evaluations of (f, f') the walks took — the numerator of the FLOP/s figure of bench.py.
struct WorkCount {
  uint32_t traced = 0;  // tests that ran TorusTest::setup (pixels of CLEAR tiles never do)
  uint32_t solved = 0;  // … and passed it
  uint32_t evals  = 0;  // evaluations of (f, f') by the default solver's walk
};

// Which form of the walk a kernel runs (both visit the same points and take the same decisions):
//   kWalkNested  TorusTest::walk(): cheapest per trip, but forward runs, backward runs and the pieces of
//                different lanes execute one after the other — the choice for COHERENT rays (render kernels:
//                config 4 −5 %, against the table);
//   kWalkTable   TorusTest::step(), first trip peeled: every lane advances on every trip whatever its piece and
//                mode — the choice for INCOHERENT rays (trt_trace on random aimed rays: 0.087 against 0.113 ms).
enum : int { kWalkNested = 0, kWalkTable = 1 };
#ifdef TRT_RENDER_WALK_TABLE   // timing builds: the table in the render kernels too
constexpr int kRenderWalk = kWalkTable;
#else
constexpr int kRenderWalk = kWalkNested;
#endif
// occluded_kernel (trt_occluded*): caller-supplied rays of unknown coherence, like trace_kernel's — the table
// (not measured against the nested form yet).
constexpr int kOccludedWalk = kWalkTable;

template <class Real, bool ALT = false, int WALK = kRenderWalk>
__device__ __forceinline__ bool torus_first_hit(Real ox, Real oy, Real oz, Real dx_, Real dy_,
                                                Real dz_, Real dd, Real inv_dd, Real tmin, Real tmax,
                                                const TorusK<Real>& T, Real& t_out, WorkCount& wc, int alt = kSolverDurandKerner)
{
  TorusTest<Real> q;
  ++wc.traced;
  if(!q.setup(ox, oy, oz, dx_, dy_, dz_, dd, inv_dd, tmin, tmax, T))
    return false;
  ++wc.solved;
  if(ALT)
  {
    if(alt == kSolverFerrari) q.solve_ferrari(inv_dd, T.Rb2);   // wave-uniform: the scene's solver
    else q.solve_dk(inv_dd, T.Rb2);
  }
  else
  {
    if(WALK == kWalkTable)
    {
      // the resumable state machine of the persistent kernel, first trip peeled (right after setup()
      // every field the transitions read is a known constant, so the compiler folds step())
      ++wc.evals;
      bool run = q.step();
      // (Letting the lanes at a piece end WAIT while others iterate — so that more trips are the cheap iterate-only ones —
      // was measured: bit-identical, and slower whatever the threshold: aimed rays 0.085 → 0.107 / 0.126 / 0.147 ms with 8 /
      // 16 / 32 waiting lanes, profiles/r03_trace_wait.txt.  Idle lanes cost more than the cheaper trips bring.)
      while(run)
      {
        ++wc.evals;
        if(__any(!q.iterating()))
          run = q.step();
        else
          run = q.step_iter();
      }
    }
    else
      q.walk(wc.evals);
  }
  return q.finish(dx_, dy_, dz_, tmin, tmax, T, t_out);
}

// Solver constants of torus i in the kernel's precision.
template <class Real> __device__ __forceinline__ const TorusK<Real>& torus_k(const SceneK& S, int i);
template <> __device__ __forceinline__ const TorusK<float>&  torus_k<float>(const SceneK& S, int i) { return S.k32[i]; }
template <> __device__ __forceinline__ const TorusK<double>& torus_k<double>(const SceneK& S, int i) { return S.k64[i]; }

// Per-ray constants of a query in the solver precision (FP32 I/O, FP32 or FP64 solve).
template <class Real>
struct RayK {
  // the ray and its interval stay FP32 (their conversion to the solver precision is exact and
  // costs one v_cvt each where a test uses them); only |d|² and its reciprocal are kept in the
  // solver precision — in the FP64 kernels that is 12 VGPRs less per lane
  float ox, oy, oz, dx, dy, dz, tmin, tmax;
  Real  dd, inv_dd;
  __device__ __forceinline__ void set(v3 o, v3 d, float tmin_, float tmax_)
  {
    ox = o.x; oy = o.y; oz = o.z; dx = d.x; dy = d.y; dz = d.z;
    const Real x = dx, y = dy, z = dz;
    dd     = fma_(z, z, fma_(y, y, x * x));
    inv_dd = Real(1) / dd;
    tmin = tmin_; tmax = tmax_;
  }
};

// Result of a test in the solver precision -> FP32 t; rounding may land on the open bounds.
__device__ __forceinline__ bool round_t(float t, float, float, float& out) { out = t; return true; }
__device__ __forceinline__ bool round_t(double t, float tmin, float tmax, float& out)
{
  const float tf = (float)t;
  if(!(tf > tmin && tf < tmax))
    return false;
  out = tf;
  return true;
}

// Oriented tori (SceneK::oriented, ORIENT kernels).  A test against an oriented torus runs in the torus' own frame, where it
// turns about +y and TorusTest applies as it stands: e = O − C is formed in world space (exact in FP64, one rounding
// in FP32 — the same subtraction setup() makes for an unoriented torus), e and D are rotated by the torus' TorusRot in
// the solver precision, and setup() is handed a centre of zero.  Rotating O and a pre-rotated centre separately would
// cancel two independently rounded vectors: an error that grows with the scene's distance from the world origin
// instead of the ray's distance from the torus.  |d|² and its reciprocal are taken from the rotated direction, so the
// local ray is self-consistent; t is the same number in both frames, and P = O + t·D stays in world space.
__device__ __forceinline__ bool is_oriented(const SceneK& S, int i) { return ((S.oriented >> i) & 1u) != 0u; }

template <class Real>
__device__ __forceinline__ void rotate_to_local(const TorusRot& M, Real x, Real y, Real z, Real& lx, Real& ly, Real& lz)
{
  lx = fma_((Real)M.m[2], z, fma_((Real)M.m[1], y, (Real)M.m[0] * x));
  ly = fma_((Real)M.m[5], z, fma_((Real)M.m[4], y, (Real)M.m[3] * x));
  lz = fma_((Real)M.m[8], z, fma_((Real)M.m[7], y, (Real)M.m[6] * x));
}
__device__ __forceinline__ v3 rotate_to_world(const TorusRot& M, v3 l)
{
  return {fma_(M.m[6], l.z, fma_(M.m[3], l.y, M.m[0] * l.x)), fma_(M.m[7], l.z, fma_(M.m[4], l.y, M.m[1] * l.x)),
          fma_(M.m[8], l.z, fma_(M.m[5], l.y, M.m[2] * l.x))};
}

// The ray of a query in the frame of oriented torus i, and that torus' solver constants with the centre at the
// frame's origin: what setup() / finish() take in place of the world ray and torus_k().
template <class Real>
struct LocalRay {
  Real ox, oy, oz, dx, dy, dz, dd, inv_dd;
  __device__ __forceinline__ void direction(const TorusRot& M, float wx, float wy, float wz)
  {
    rotate_to_local<Real>(M, (Real)wx, (Real)wy, (Real)wz, dx, dy, dz);
  }
  __device__ __forceinline__ void set(const SceneK& S, int i, float wox, float woy, float woz, float wdx, float wdy, float wdz)
  {
    const TorusShade& C = S.shade[i];   // the world centre (FP32, as the caller passed it)
    rotate_to_local<Real>(S.rot[i], (Real)wox - (Real)C.cx, (Real)woy - (Real)C.cy, (Real)woz - (Real)C.cz, ox, oy, oz);
    direction(S.rot[i], wdx, wdy, wdz);
    dd     = fma_(dz, dz, fma_(dy, dy, dx * dx));
    inv_dd = Real(1) / dd;
  }
};
template <class Real>
__device__ __forceinline__ TorusK<Real> centred(const TorusK<Real>& T)
{
  TorusK<Real> c = T;
  c.cx = Real(0); c.cy = Real(0); c.cz = Real(0);
  return c;
}

// One ray against torus i over the open interval (tmin, tmax); t rounded to FP32.
template <class Real, bool ALT = false, int WALK = kRenderWalk, bool ORIENT = false>
__device__ __forceinline__ bool torus_hit(const SceneK& S, int i, const RayK<Real>& r, float tmin, float tmax, float& t, WorkCount& wc)
{
  Real tt;
  if constexpr(ORIENT)
  {
    // one copy of the solver for both kinds of torus: the world ray and torus_k(), or — wave-uniform, every lane of a
    // query loop is at the same torus — the local ray and the centred constants
    LocalRay<Real> l = {(Real)r.ox, (Real)r.oy, (Real)r.oz, (Real)r.dx, (Real)r.dy, (Real)r.dz, r.dd, r.inv_dd};
    TorusK<Real>   T = torus_k<Real>(S, i);
    if(is_oriented(S, i))
    {
      l.set(S, i, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
      T = centred(T);
    }
    if(!torus_first_hit<Real, ALT, WALK>(l.ox, l.oy, l.oz, l.dx, l.dy, l.dz, l.dd, l.inv_dd, (Real)r.tmin, (Real)tmax, T, tt, wc, S.alt_solver))
      return false;
    return round_t(tt, tmin, tmax, t);
  }
  if(!torus_first_hit<Real, ALT, WALK>((Real)r.ox, (Real)r.oy, (Real)r.oz, (Real)r.dx, (Real)r.dy, (Real)r.dz, r.dd, r.inv_dd, (Real)r.tmin, (Real)tmax,
                                       torus_k<Real>(S, i), tt, wc, S.alt_solver))
    return false;
  return round_t(tt, tmin, tmax, t);
}

// Closest hit over the tori — the role of traceRayEXT + BVH (REFL/shaders/raytrace.rgen:64-75).
// Tori are tested in S.order (largest bounding sphere first) and the interval of every later
// test ends at the closest hit so far: behind an enclosing shell the remaining tests end in
// their window clip without a Newton step.  Equal t keeps the torus tested first.
// `skip` (a mask over test-order positions) names the tori this ray cannot hit first: tubes that lie strictly inside a
// tube the ray's origin is known to be OUTSIDE of (enclosure cull) — they count as tests and cost nothing.
// Returns the torus index or -1; `tests` counts ray–torus tests.
template <class Real, bool ALT = false, int WALK = kRenderWalk, bool ORIENT = false>
__device__ __forceinline__ int closest_hit(const SceneK& S, v3 o, v3 d, float tmin, float tmax,
                                           float& t_out, uint32_t& tests, WorkCount& wc, uint32_t skip = 0u)
{
  RayK<Real> r;
  r.set(o, d, tmin, tmax);
  int   id   = -1;
  float best = __builtin_inff();
  for(int k = 0; k < S.n_tori; ++k)
  {
    const int i = S.order[k];
    float t;
    ++tests;
    if((skip >> k) & 1u)
      continue;
#ifdef TRT_FULL_WINDOW   // timing experiment only (the tail of config 4): every torus over the FULL interval, minimum afterwards
    if(torus_hit<Real, ALT, WALK, ORIENT>(S, i, r, tmin, tmax, t, wc) && t < best)
#else
    if(torus_hit<Real, ALT, WALK, ORIENT>(S, i, r, tmin, min_(tmax, best), t, wc))
#endif
    {
      best = t;
      id   = i;
    }
  }
  t_out = best;
  return id;
}

// The shadow query: any hit — gl_RayFlagsTerminateOnFirstHitEXT (REFL/shaders/raytrace.rchit:114-131) — with a say for
// the caller at every torus i that is hit: pass(i) == true lets the ray through that torus (trt_shade_scene* with
// TRT_SCENE_GLASS_SHADOWS: the caller filters the light there, once per torus however often the ray crosses it) and the
// query goes on.  Returns whether a torus that does not pass was hit.  Tori are tested in S.order, each over the full
// window; every torus started counts one test, a skipped one too.
template <class Real, bool ALT = false, bool ORIENT = false, int WALK = kRenderWalk, class Pass>
__device__ __forceinline__ bool blocked_hit(const SceneK& S, v3 o, v3 d, float tmin, float tmax,
                                            uint32_t& tests, WorkCount& wc, uint32_t skip, Pass&& pass)
{
  RayK<Real> r;
  r.set(o, d, tmin, tmax);
  for(int k = 0; k < S.n_tori; ++k)
  {
    float t;
    ++tests;
    if((skip >> k) & 1u)
      continue;
    const int i = S.order[k];
    if(torus_hit<Real, ALT, WALK, ORIENT>(S, i, r, tmin, tmax, t, wc) && !pass(i))
      return true;
  }
  return false;
}

// Any hit: the query above with nothing let through.
// Up to and including the first torus (in S.order) with a root in the window this runs the torus_hit calls of
// closest_hit with the same arguments — closest_hit's interval shrinks only after that torus — so, for the same WALK or
// any other (the forms are bit-identical), any_hit() == (closest_hit() >= 0) bit for bit.
template <class Real, bool ALT = false, bool ORIENT = false, int WALK = kRenderWalk>
__device__ __forceinline__ bool any_hit(const SceneK& S, v3 o, v3 d, float tmin, float tmax,
                                        uint32_t& tests, WorkCount& wc, uint32_t skip = 0u)
{
  return blocked_hit<Real, ALT, ORIENT, WALK>(S, o, d, tmin, tmax, tests, wc, skip, [](int) { return false; });
}

// Every crossing of one ray with torus i inside the open interval (r.tmin, r.tmax), left to right: emit(t, entering) per
// crossing, t rounded to FP32.  The test is torus_hit()'s over the same window — the same setup(), the walk that
// TorusTest::walk_all() continues past the first root, and for EVERY root the polish, round_t and the open-interval test
// a closest hit gets — so the first crossing emitted is torus_hit()'s t bit for bit, unless that first root falls to the
// interval test (torus_hit then reports a miss; the enumeration goes on to the next root).  Default solver only.
template <class Real, bool ORIENT = false, class Emit>
__device__ __forceinline__ void torus_crossings(const SceneK& S, int i, const RayK<Real>& r, WorkCount& wc, Emit&& emit)
{
  LocalRay<Real> l = {(Real)r.ox, (Real)r.oy, (Real)r.oz, (Real)r.dx, (Real)r.dy, (Real)r.dz, r.dd, r.inv_dd};
  TorusK<Real>   T = torus_k<Real>(S, i);
  if constexpr(ORIENT)
    if(is_oriented(S, i))   // wave-uniform, as in torus_hit()
    {
      l.set(S, i, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
      T = centred(T);
    }
  TorusTest<Real> q;
  ++wc.traced;
  if(!q.setup(l.ox, l.oy, l.oz, l.dx, l.dy, l.dz, l.dd, l.inv_dd, (Real)r.tmin, (Real)r.tmax, T))
    return;
  ++wc.solved;
  Real      u[4] = {};
  const int n = q.walk_all(wc.evals, u);
  for(int k = 0; k < n; ++k)
  {
    const Real uk = k == 0 ? u[0] : (k == 1 ? u[1] : (k == 2 ? u[2] : u[3]));
    Real  tt, gh;
    float t;
    if(q.finish_root(uk, l.dx, l.dy, l.dz, (Real)r.tmin, (Real)r.tmax, T, tt, gh) && round_t(tt, r.tmin, r.tmax, t))
      emit(t, gh < Real(0));
  }
}

// T4: outward unit normal N = normalize(P - q), q = nearest point of the centre circle
// (role of REFL/shaders/raytrace.rchit:74-75; never flipped towards the ray).
__device__ __forceinline__ v3 torus_normal(const TorusShade& T, v3 P)
{
  const v3    pl  = sub3(P, v3{T.cx, T.cy, T.cz});
  const float rho = sqrt_(fma_(pl.z, pl.z, pl.x * pl.x));
  const float k   = (rho - T.R) / rho;
  return normalize3(v3{pl.x * k, pl.y, pl.z * k});
}
// The same for torus i of the scene; an oriented torus: P − C rotated into its frame, the normal formed there as above
// and rotated back before it is normalised (so |N| = 1 to one rounding, as for every other torus).
template <bool ORIENT>
__device__ __forceinline__ v3 torus_normal(const SceneK& S, int i, v3 P)
{
  const TorusShade& T = S.shade[i];
  if(ORIENT && is_oriented(S, i))
  {
    const v3 pw = sub3(P, v3{T.cx, T.cy, T.cz});
    v3 pl;
    rotate_to_local<float>(S.rot[i], pw.x, pw.y, pw.z, pl.x, pl.y, pl.z);
    const float rho = sqrt_(fma_(pl.z, pl.z, pl.x * pl.x));
    const float k   = (rho - T.R) / rho;
    return normalize3(rotate_to_world(S.rot[i], v3{pl.x * k, pl.y, pl.z * k}));
  }
  return torus_normal(T, P);
}

// ------------------------------------------------------------------------------------------
// Phong helpers — REFL/shaders/wavefront.glsl:22-48
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ v3 compute_diffuse(const MaterialK& m, v3 L, v3 N)
{
  const float dotNL = max_(dot3(N, L), 0.0f);
  v3 c = {m.diffuse[0] * dotNL, m.diffuse[1] * dotNL, m.diffuse[2] * dotNL};
  if(m.illum >= 1)
  {
    c.x += m.ambient[0];
    c.y += m.ambient[1];
    c.z += m.ambient[2];
  }
  return c;
}

__device__ __forceinline__ v3 compute_specular(const MaterialK& m, v3 viewDir, v3 L, v3 N)
{
  if(m.illum < 2)
    return {0.0f, 0.0f, 0.0f};
  const float kPi        = 3.14159265f;
  const float kShininess = max_(m.shininess, 4.0f);
  const float kEnergy    = (2.0f + kShininess) / (2.0f * kPi);
  const v3    V          = normalize3(neg3(viewDir));
  const v3    R          = reflect3(neg3(L), N);
  // GLSL pow(x, y) is specified as exp2(y * log2(x)) (GLSL 4.60 §8.2): v_log_f32 / v_exp_f32,
  // two quarter-rate instructions instead of OCML's 230-instruction correctly-rounded powf.
  // For results that matter (x^y > 1e-3) the relative error stays below 1e-6.
  const float s          = kEnergy * __builtin_amdgcn_exp2f(kShininess * __builtin_amdgcn_logf(max_(dot3(V, R), 0.0f)));
  return {m.specular[0] * s, m.specular[1] * s, m.specular[2] * s};
}

// ------------------------------------------------------------------------------------------
// ray generation
// ------------------------------------------------------------------------------------------
// Per-frame constants of the toroidal camera, computed once on the host
// (BEF/shaders/raytrace.rgen:36-53 depend only on the UBO and rho), and per-column /
// per-row trigonometry tables (BEF rgen:25-28,56-57: alfa depends on x only, beta on y only).
struct ToroCam {
  float        eye[3];
  float        rho;
  const float* cos_a;  // [W]  cos(radians(alfa + omega))
  const float* sin_a;  // [W]
  const float* cos_b;  // [H]  cos(radians(beta + theta))
  const float* sin_b;  // [H]
};

// The ray through film position (px, py) in pixels (pinhole) / of column x and row y of the tables (toroidal): the body
// the two forms below share, so that a pixel centre and a sub-pixel sample run the same instructions.
__device__ __forceinline__ void raygen_at(const trt_globals& g, const ToroCam& tc, uint32_t W, uint32_t H,
                                          int camera, uint32_t x, uint32_t y, float px, float py, v3& origin, v3& dir)
{
  if(camera == TRT_CAMERA_TOROIDAL)
  {
    // the table pointers come out of the LDS-staged arguments: tell hipcc they address global memory
    // (global_load instead of flat_load, which would also count on lgkmcnt)
    typedef __attribute__((address_space(1))) const float* gcf;
    const float ca = ((gcf)tc.cos_a)[x], sa = ((gcf)tc.sin_a)[x], cb = ((gcf)tc.cos_b)[y], sb = ((gcf)tc.sin_b)[y];
    origin = {fma_(tc.rho, ca, tc.eye[0]), tc.eye[1], fma_(tc.rho, sa, tc.eye[2])};  // BEF rgen:56
    dir    = {ca * cb, sb, sa * cb};                                                // BEF rgen:57
    return;
  }
  // pinhole, REFL/shaders/raytrace.rgen:42-48
  const float u = px / (float)W, v = py / (float)H;
  const float dx = u * 2.0f - 1.0f, dy = v * 2.0f - 1.0f;
  origin       = mat4_mul(g.viewInverse, 0.0f, 0.0f, 0.0f, 1.0f);
  const v3 tgt = mat4_mul(g.projInverse, dx, dy, 1.0f, 1.0f);
  const v3 tn  = normalize3(tgt);
  dir          = mat4_mul(g.viewInverse, tn.x, tn.y, tn.z, 0.0f);
}

// The primary ray of pixel (x, y): through the pixel centre.
__device__ __forceinline__ void raygen(const trt_globals& g, const ToroCam& tc, uint32_t W, uint32_t H,
                                       int camera, uint32_t x, uint32_t y, v3& origin, v3& dir)
{
  raygen_at(g, tc, W, H, camera, x, y, (float)x + 0.5f, (float)y + 0.5f, origin, dir);
}

// The ray of a sub-pixel sample (trt_camera_rays*, trt_shade_camera*; include/trt.h states the arithmetic).  Pinhole: the
// film position is the pixel centre plus (jx, jy).  Toroidal: the offset is in the tables — `tc` holds the tables of
// THIS sample, built on the host from d_alfa·((float)x + jx) and d_beta·((float)y + jy) — and jx, jy are not read.
// With jx = jy = 0 (and the render's tables) this is raygen(), bit for bit: t + 0.0f == t for every t that is not -0.
__device__ __forceinline__ void raygen_offset(const trt_globals& g, const ToroCam& tc, uint32_t W, uint32_t H,
                                              int camera, uint32_t x, uint32_t y, float jx, float jy, v3& origin, v3& dir)
{
  raygen_at(g, tc, W, H, camera, x, y, ((float)x + 0.5f) + jx, ((float)y + 0.5f) + jy, origin, dir);
}

// ------------------------------------------------------------------------------------------
// post pass: pow(c, 1/2.2) with exact-operation log2 / exp2 (REFL/shaders/post.frag:33-37)
// ------------------------------------------------------------------------------------------
// log2(x), x a positive normal float: x = 2^e·m, m ∈ [√½, √2); ln(m) = 2·atanh(s), s = (m-1)/(m+1),
// odd series to s⁹ (|s| <= 0.172: truncation < 5e-10); only + - * / fma and integer bit moves.
__device__ __forceinline__ float log2_poly(float x)
{
  int   bits = __float_as_int(x);
  int   e    = (bits >> 23) - 127;
  float m    = __int_as_float((bits & 0x007fffff) | 0x3f800000);
  if(m > 1.41421354f) { m *= 0.5f; e += 1; }
  const float s  = (m - 1.0f) / (m + 1.0f);
  const float s2 = s * s;
  float p = fma_(s2, 0.222222222f, 0.285714286f);   // 2/9, 2/7
  p = fma_(s2, p, 0.4f);                             // 2/5
  p = fma_(s2, p, 0.666666667f);                     // 2/3
  p = fma_(s2, p, 2.0f);
  return fma_(p * s, 1.44269504f, (float)e);         // ln -> log2, plus the exponent
}
// 2^y for y in [-126, 127]: n = floor(y), 2^f = exp(f·ln2) by its Taylor polynomial to f⁹, then
// the exponent is added to the bit pattern.
__device__ __forceinline__ float exp2_poly(float y)
{
  y = min_(max_(y, -126.0f), 127.0f);
  const float n = floorf(y);
  const float z = (y - n) * 0.693147181f;
  float p = fma_(z, 2.75573192e-6f, 2.48015873e-5f);  // 1/9!, 1/8!
  p = fma_(z, p, 1.98412698e-4f);                     // 1/7!
  p = fma_(z, p, 1.38888889e-3f);                     // 1/6!
  p = fma_(z, p, 8.33333333e-3f);                     // 1/5!
  p = fma_(z, p, 4.16666667e-2f);                     // 1/4!
  p = fma_(z, p, 1.66666667e-1f);                     // 1/3!
  p = fma_(z, p, 0.5f);
  p = fma_(z, p, 1.0f);
  p = fma_(z, p, 1.0f);
  return __int_as_float(__float_as_int(p) + ((int)n << 23));
}
// pow(c, 1/2.2) as the post shader applies it; non-positive and NaN inputs give 0, +inf stays.
__device__ __forceinline__ float post_gamma(float c)
{
  if(!(c > 0.0f)) return 0.0f;
  if(c > 3.0e38f) return c;
  if(c < 1.17549435e-38f) return 0.0f;  // subnormal colours
  return exp2_poly(0.454545455f * log2_poly(c));
}

// ------------------------------------------------------------------------------------------
// the (u, v) of a point on a torus (trt_shade_textured*, trt_hit_uv*; include/trt.h states the rule)
// ------------------------------------------------------------------------------------------
// atan2(y, x) in (-pi, pi] with exact operations only — like log2_poly / exp2_poly it does not move with the ROCm release
// (OCML's atan2f may).  Octant reduction to mn / mx in [0, 1], folded once more at tan(pi/8) by
// atan(a) = pi/4 + atan((a - 1) / (a + 1)) BEFORE the division, so that there is one division and |q| <= tan(pi/8); then
// atan(q) = q + q·s·(c1 + s·(c2 + s·(c3 + s·c4))), s = q², a least-maximum fit on that interval (|error| < 5e-9 rad before
// rounding; with it, against FP64 atan2 over two million points: 2.6e-7 rad, 4.2e-8 of a turn — the roundings of the
// constants of pi).  (0, 0) gives 0 / 0 = NaN: a caller on a ring torus never passes it (rho >= R - r > 0, and
// (rho - R)² + y² = r²), and torus_uv() turns a NaN into 0.
__device__ __forceinline__ float atan2_poly(float y, float x)
{
  const float ax = abs_(x), ay = abs_(y);
  const float mx = max_(ax, ay), mn = min_(ax, ay);
  const bool  far = mn > 0.414213568f * mx;                  // tan(pi/8)
  const float q  = (far ? mn - mx : mn) / (far ? mn + mx : mx);
  const float s  = q * q;
  float p = fma_(s, 0.07902598f, -0.13824454f);
  p = fma_(s, p, 0.19971879f);
  p = fma_(s, p, -0.33332756f);
  float r = fma_(p * s, q, q);
  if(far) r += 0.785398163f;                                 // pi/4
  if(ay > ax) r = 1.57079633f - r;                           // pi/2
  if(x < 0.0f) r = 3.14159265f - r;                          // pi
  return y < 0.0f ? -r : r;
}
// An angle in radians as a fraction of a turn in [0, 1): one multiplication by 1/(2 pi), less its floor; a value that
// rounds up to 1 (a tiny negative angle) is 0, the same point of the circle — and so is a NaN.
__device__ __forceinline__ float angle_to_turn(float a)
{
  const float t = a * 0.159154943f;
  const float f = t - floorf(t);
  return f < 1.0f ? f : 0.0f;
}
// (u, v) of point P on torus i: q = P − C in the torus' frame (the rows (u, a, w) of TorusRot; the identity for +y),
// u the angle of (q.x, q.z) about the axis, v the angle of (rho − R, q.y) about the tube — rho exactly as torus_normal
// forms it.  ONE function for the shading kernels and trt_hit_uv.
template <bool ORIENT>
__device__ __forceinline__ void torus_uv(const SceneK& S, int i, v3 P, float& u, float& v)
{
  const TorusShade& T = S.shade[i];
  v3 q = sub3(P, v3{T.cx, T.cy, T.cz});
  if(ORIENT && is_oriented(S, i))
  {
    const v3 pw = q;
    rotate_to_local<float>(S.rot[i], pw.x, pw.y, pw.z, q.x, q.y, q.z);
  }
  const float rho = sqrt_(fma_(q.z, q.z, q.x * q.x));
  u = angle_to_turn(atan2_poly(q.z, q.x));
  v = angle_to_turn(atan2_poly(q.y, rho - T.R));
}

}  // namespace trt
