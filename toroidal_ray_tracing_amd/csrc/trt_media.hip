// trt_media.hip — media that fill the tubes, integrated along caller-supplied rays (trt_chords*, trt_glow*, trt_glow_profile*, trt_glow_weights*,
// trt_glow_weights_absorbed*, trt_glow_project*, trt_glow_backproject*, trt_glow_tangent*, trt_glow_adjoint*), gfx950.
//
// What the kernels share, each said once:
//   tube_frame, tube_rho2   the ray in torus j's frame, and the tube label of its point at t: the inside test and every
//                    profile lookup are this one expression
//   tube_intervals   the pairing rule: torus j's crossings and the two inside tests → at most two intervals
//   media_ray        ray i's window, and behind a window that is not empty its RayK and world length
//   for_each_ray     the grid-stride loop over the rays and the counted-tests epilogue
//   merged_pieces    the intervals of several tori merged in the lane's crossing column, walked piece by piece (merged_fill,
//                    then merged_walk: a kernel that walks a ray twice fills once)
//   knot_of, gauss_pair, glow_step_weight   a label's knot and fraction; the two points of a sub-step; E and the weight of a step
// The kernels, one lane per ray:
//   chords_kernel    the length of every ray inside every tube: the intervals summed, n_tori coalesced streams out.
//   glow_kernel      radiance and the transmittance left: the emission–absorption integral over the merged pieces of the
//                    tori with a medium, one float4 per ray out.
//   glow_profile_kernel   glow with a radial profile per torus: every piece cut into sub-steps, the tables (in LDS) read at
//                    the two Gauss–Legendre points of each.
//   glow_weights_kernel   the response of every ray to every knot of every torus' profile (sigma = 0): the sub-steps inside
//                    each interval of a torus, 17 accumulators per lane in LDS, 17 · n_tori streams out.
//   glow_weights_absorbed_kernel   the same response behind absorbing media: the merged pieces of ALL tori with a running T,
//                    the accumulators of all tori live at once, the block width chosen from n_tori.
//   glow_project_kernel, glow_backproject_kernel   that walk again, with the weights used on the chip: W · x per ray, and
//                    Wᵀ y in FP64 reduced over the rays (backproject_sum_kernel adds the blocks' rows).
//   glow_tangent_kernel, glow_sigma_adjoint_kernel   the derivative of glow_project_kernel's map with respect to all four
//                    channels of the tables: J · delta per ray in one sweep (store_tables_kernel puts the direction's tables
//                    where the walk finds them), and the sigma entries of Jᵀ y — two sweeps over the lane's stored column,
//                    reduced as the back-projection reduces (adjoint_sum_kernel adds the blocks' rows).
//   launch_chords, launch_glow, launch_glow_profile, launch_glow_weights, launch_glow_weights_absorbed, launch_glow_project,
//                    launch_glow_backproject, launch_glow_tangent, launch_glow_adjoint   their grid and launch wrappers.
//
// The crossings of torus j are trt_crossings' (torus_crossings, trt_device.hpp: every torus in S.order over the full
// window, no enclosure cull); include/trt.h states the arithmetic of everything on top of them, expression by expression.
// The media come in the kernel arguments (Media, trt_kernels.hpp); SceneK knows nothing of them and no material is read.
// Default solver only: instantiated for <float | double> × ORIENT.  Compiled with -ffp-contract=off like every unit.
#include <cstring>

#include "trt_render.hpp"

namespace trt {

// ------------------------------------------------------------------------------------------
// the tube label and the pairing rule
// ------------------------------------------------------------------------------------------
// The ray torus_crossings() hands the solver for torus j, and the torus it is tested against: the world ray and torus_k()'s
// centre, or — wave-uniform — the ray in the frame of an oriented torus and a centre of zero.
template <class Real, bool ORIENT>
__device__ __forceinline__ void tube_frame(const SceneK& S, int j, const RayK<Real>& r, LocalRay<Real>& l, TorusK<Real>& T)
{
  l = {(Real)r.ox, (Real)r.oy, (Real)r.oz, (Real)r.dx, (Real)r.dy, (Real)r.dz, r.dd, r.inv_dd};
  T = torus_k<Real>(S, j);
  if constexpr(ORIENT)
    if(is_oriented(S, j))
    {
      l.set(S, j, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
      T = centred(T);
    }
}
// The label of the ray's point at t, rho² — the squared distance from the tube's centre circle — in the solver precision:
// P = fma(t, d, o) − c per component, q = sqrt(fma(pz, pz, px·px)) − R, rho² = fma(q, q, py·py).  rho² < r² is inside,
// (float)rho² · inv_r2 is the x of a profile: the two agree on this expression to the bit (include/trt.h).
template <class Real>
__device__ __forceinline__ Real tube_rho2(const LocalRay<Real>& l, const TorusK<Real>& T, Real t)
{
  const Real px = fma_(t, l.dx, l.ox) - T.cx, py = fma_(t, l.dy, l.oy) - T.cy, pz = fma_(t, l.dz, l.oz) - T.cz;
  const Real q  = sqrt_(fma_(pz, pz, px * px)) - T.R;
  return fma_(q, q, py * py);
}
// Whether the point of ray r at t lies inside torus i's tube.  A non-finite point compares false: outside.
template <class Real, bool ORIENT>
__device__ __forceinline__ bool tube_inside(const SceneK& S, int i, const RayK<Real>& r, float t)
{
  LocalRay<Real> l;
  TorusK<Real>   T;
  tube_frame<Real, ORIENT>(S, i, r, l, T);
  return tube_rho2(l, T, (Real)t) < T.r2;
}

// emit(a, b, from_start, to_end) per interval of torus j inside the window (r.tmin, r.tmax) of ray r, left to right:
// from_start — a is r.tmin because the window starts inside the tube; to_end — b is r.tmax because it ends inside.
// The torus' at most four crossings are first put in trt_crossings' order — ascending t, a crossing behind every earlier
// one with t <= its own (column_insert's stable rule): the two roots of a grazing contact can come out of the solver's
// polish in descending order, and walked as found they would close an interval before it opens — in four registers and
// four flags, by select chains (nothing is indexed: no private array that could go to scratch).  Then the walk carries
// one open interval: an entering crossing opens one if none is open, a leaving one closes and emits it, both are ignored
// otherwise; what is still open behind the last crossing is emitted only if the window's end point lies inside, and
// dropped if not.  At most two intervals in exact arithmetic.
template <class Real, bool ORIENT, class Emit>
__device__ __forceinline__ void tube_intervals(const SceneK& S, int j, const RayK<Real>& r, WorkCount& wc, Emit&& emit)
{
  const bool  in0 = tube_inside<Real, ORIENT>(S, j, r, r.tmin), in1 = tube_inside<Real, ORIENT>(S, j, r, r.tmax);
  const float inf = __builtin_inff();
  float t0 = inf, t1 = inf, t2 = inf, t3 = inf;   // (a crossing has t < tmax: an unused slot never compares <= t)
  bool  e0 = false, e1 = false, e2 = false, e3 = false;
  int   n  = 0;
  torus_crossings<Real, ORIENT>(S, j, r, wc, [&](float t, bool entering) {
    const bool c0 = t0 <= t, c1 = t1 <= t, c2 = t2 <= t;   // sorted: c2 implies c1 implies c0
    t3 = c2 ? t : t2;   e3 = c2 ? entering : e2;
    t2 = c2 ? t2 : (c1 ? t : t1);   e2 = c2 ? e2 : (c1 ? entering : e1);
    t1 = c1 ? t1 : (c0 ? t : t0);   e1 = c1 ? e1 : (c0 ? entering : e0);
    t0 = c0 ? t0 : t;   e0 = c0 ? e0 : entering;
    ++n;
  });
  float open = r.tmin;
  bool  has = in0, first = in0;
  for(int k = 0; k < n && k < 4; ++k)
  {
    const float t        = k == 0 ? t0 : (k == 1 ? t1 : (k == 2 ? t2 : t3));
    const bool  entering = k == 0 ? e0 : (k == 1 ? e1 : (k == 2 ? e2 : e3));
    if(entering)
    {
      if(!has)
      {
        open = t;
        has  = true;
      }
    }
    else if(has)
    {
      emit(open, t, first, false);
      has   = false;
      first = false;
    }
  }
  if(has && in1)
    emit(open, r.tmax, first, true);
}

// ------------------------------------------------------------------------------------------
// the rays of a query
// ------------------------------------------------------------------------------------------
// Ray i of a query: whether its window (in.tmin, min(tmax_per_ray[i], in.tmax)) — the per-ray bound clipped by the scalar; a
// NaN bound stays NaN and empties it — is not empty.  Only then are the ray's streams read: r holds the ray and its window,
// len the world length per unit of t.
template <class Real>
__device__ __forceinline__ bool media_ray(const MediaRays& in, uint64_t i, RayK<Real>& r, float& len)
{
  const float b    = in.tmax_per_ray ? ((gptr<const float>)in.tmax_per_ray)[i] : in.tmax;
  const float tmax = b > in.tmax ? in.tmax : b;
  if(!(tmax > in.tmin))
    return false;
  const gptr<const float> ox = (gptr<const float>)in.rays.ox, oy = (gptr<const float>)in.rays.oy, oz = (gptr<const float>)in.rays.oz;
  const gptr<const float> dx = (gptr<const float>)in.rays.dx, dy = (gptr<const float>)in.rays.dy, dz = (gptr<const float>)in.rays.dz;
  const v3 o = {ox[i], oy[i], oz[i]};
  const v3 d = {dx[i], dy[i], dz[i]};
  r.set(o, d, in.tmin, tmax);
  len = sqrt_((d.x * d.x + d.y * d.y) + d.z * d.z);
  return true;
}
// body(i, tests, wc) for every ray i of the block's lanes (grid-stride), then the block's counts into `stats`.  A body counts
// the tori it tests in `tests`.
template <class Body>
__device__ __forceinline__ void for_each_ray(const MediaRays& in, unsigned long long* stats, Body&& body)
{
  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < in.rays.n; i += stride)
    body(i, tests, wc);
  if(stats)
    block_add_stats(stats, tests, 0u, 0u, wc);
}

// ------------------------------------------------------------------------------------------
// chords(rays_in → n_tori streams of lengths)
// ------------------------------------------------------------------------------------------
// No LDS beyond the scene.  The torus loop is wave-uniform, so the store of torus j is one instruction of 64 consecutive
// floats of stream j.  A ray whose window is empty executes no test and stores zeros.
template <class Real, bool ORIENT = false>
__global__ __launch_bounds__(256) void chords_kernel(const SceneK scene, const ChordsArgs a)
{
  __shared__ SceneK S;
  stage_scene<ORIENT>(&S, scene);

  for_each_ray(a.in, a.stats, [&](uint64_t i, uint32_t& tests, WorkCount& wc) {
    RayK<Real> r;
    float      len = 0.0f;
    const bool window = media_ray(a.in, i, r, len);
    for(int k = 0; k < S.n_tori; ++k)
    {
      const int j   = S.order[k];
      float     acc = 0.0f;
      if(window)
      {
        ++tests;
        tube_intervals<Real, ORIENT>(S, j, r, wc, [&](float u, float v, bool, bool) { acc = acc + (v - u) * len; });
      }
      st1(a.length, (uint64_t)j * a.in.rays.n + i, acc);
    }
  });
}

// ------------------------------------------------------------------------------------------
// glow(rays_in → radiance and transmittance)
// ------------------------------------------------------------------------------------------
// (1 − exp(−τ)) / τ for τ < kGlowSeries, where the quotient would cancel: its series Σ (−τ)^k / (k + 1)! to τ⁶ (the
// first term left out is below 1.6e-9 there), Horner with fma.
constexpr float kGlowSeries = 0.25f;
__device__ __forceinline__ float one_minus_exp_over(float tau)
{
  float p = fma_(tau, 1.98412698e-4f, -1.38888889e-3f);   // 1/7!, -1/6!
  p = fma_(tau, p, 8.33333333e-3f);                       // 1/5!
  p = fma_(tau, p, -4.16666667e-2f);                      // -1/4!
  p = fma_(tau, p, 1.66666667e-1f);                       // 1/3!
  p = fma_(tau, p, -0.5f);
  return fma_(tau, p, 1.0f);
}

// What a homogeneous step over the world length l with the absorption sg lets through, E = exp(−sg · l), and the weight
// wgt = (1 − E) / sg of what it emits (l where sg is 0; the series below kGlowSeries).
__device__ __forceinline__ void glow_step_weight(float sg, float l, float& E, float& wgt)
{
  const float tau = sg * l;
  E   = 1.0f;
  wgt = l;
  if(sg != 0.0f)
  {
    E   = exp2_poly(-tau * 1.44269504f);
    wgt = tau < kGlowSeries ? l * one_minus_exp_over(tau) : (1.0f - E) / sg;
  }
}

// The homogeneous step of trt_glow over the world length l, with the summed emission (e0, e1, e2) and absorption sg: a
// piece of glow_kernel, a sub-step of glow_profile_kernel.
__device__ __forceinline__ void glow_step(float e0, float e1, float e2, float sg, float l, float& Lr, float& Lg, float& Lb, float& T)
{
  float E, wgt;
  glow_step_weight(sg, l, E, wgt);
  Lr = fma_(e0 * wgt, T, Lr);
  Lg = fma_(e1 * wgt, T, Lg);
  Lb = fma_(e2 * wgt, T, Lb);
  T  = T * E;
}

// ------------------------------------------------------------------------------------------
// the merged pieces of a ray
// ------------------------------------------------------------------------------------------
// piece(u, v, active) for every non-empty piece (u, v) of ray r's window inside some tube, front to back; bit j of `active`:
// the piece lies inside torus j.  A torus with bit j of `present` goes through the pairing rule (and counts in `tests`);
// the ends of its intervals go into the lane's sorted column in dynamic LDS (column_insert: crossings_kernel's layout, K =
// 4 · n_tori slots — two intervals per torus at most, so nothing is ever truncated — at the stride LANES) with the byte
// id << 1 | 1 for a start and id << 1 for an end.  An interval that starts with the window is a bit of the initial
// active mask instead of a slot, and one that ends with the window has no end slot: the last piece closes it.  Then the
// pieces between consecutive break points are walked.  Equal break points give an empty piece, which is skipped: their
// order in the column does not matter.  (Parameters by reference, for column_insert's reason.)
// The two halves, for a kernel that walks the pieces of a ray more than once (the roots are solved once): merged_fill
// leaves the column, its length `count` and the initial mask `active`; merged_walk walks the pieces from them and leaves
// all three as they are.
template <class Real, bool ORIENT, uint32_t LANES>
__device__ __forceinline__ void merged_fill(const SceneK& S, const RayK<Real>& r, const uint32_t& present, float* const& ct, uint8_t* const& cw,
                                            const uint32_t& K, uint32_t& tests, WorkCount& wc, uint32_t& active, uint32_t& count)
{
  active = 0u;
  count  = 0u;
  for(int k = 0; k < S.n_tori; ++k)
  {
    const int j = S.order[k];
    if(!((present >> j) & 1u))
      continue;
    ++tests;
    tube_intervals<Real, ORIENT>(S, j, r, wc, [&](float u, float v, bool from_start, bool to_end) {
      if(from_start) active |= 1u << j;
      else column_insert<LANES>(ct, cw, K, count, u, j, true);
      if(!to_end) column_insert<LANES>(ct, cw, K, count, v, j, false);
    });
  }
}
template <class Real, uint32_t LANES, class Piece>
__device__ __forceinline__ void merged_walk(const RayK<Real>& r, float* const& ct, uint8_t* const& cw, uint32_t active,
                                            const uint32_t& count, Piece&& piece)
{
  float u = r.tmin;
  for(uint32_t k = 0; k <= count; ++k)
  {
    const bool     last = k == count;
    const float    v    = last ? r.tmax : ct[k * LANES];
    const uint32_t w    = last ? 0u : cw[k * LANES];
    if(active != 0u && v > u)
      piece(u, v, active);
    const uint32_t bit = 1u << (w >> 1);
    if(!last)
      active = (w & 1u) ? (active | bit) : (active & ~bit);
    u = v;
  }
}
template <class Real, bool ORIENT, uint32_t LANES, class Piece>
__device__ __forceinline__ void merged_pieces(const SceneK& S, const RayK<Real>& r, const uint32_t& present, float* const& ct, uint8_t* const& cw,
                                              const uint32_t& K, uint32_t& tests, WorkCount& wc, Piece&& piece)
{
  uint32_t active, count;
  merged_fill<Real, ORIENT, LANES>(S, r, present, ct, cw, K, tests, wc, active, count);
  merged_walk<Real, LANES>(r, ct, cw, active, count, piece);
}

// The pieces of the tori with a medium (bit j of media.present).  The sums over the active tori of a piece are a loop over
// the torus id that is uniform for the wave (its bound and the media come from the kernel arguments: scalar loads),
// predicated by the lane's mask.
template <class Real, bool ORIENT = false>
__global__ __launch_bounds__(256) void glow_kernel(const SceneK scene, const GlowArgs a)
{
  __shared__ SceneK S;
  extern __shared__ float crossing_lds[];   // [K][256] t, then [K][256] bytes
  stage_scene<ORIENT>(&S, scene);

  const uint32_t K  = 4u * (uint32_t)S.n_tori;
  float*         ct = crossing_lds + threadIdx.x;
  uint8_t*       cw = reinterpret_cast<uint8_t*>(crossing_lds + K * 256u) + threadIdx.x;

  for_each_ray(a.in, a.stats, [&](uint64_t i, uint32_t& tests, WorkCount& wc) {
    float      Lr = 0.0f, Lg = 0.0f, Lb = 0.0f, T = 1.0f, len;
    RayK<Real> r;
    if(media_ray(a.in, i, r, len))
      merged_pieces<Real, ORIENT, 256u>(S, r, a.media.present, ct, cw, K, tests, wc, [&](float u, float v, uint32_t active) {
        float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f, sg = 0.0f;
        for(int j = 0; j < scene.n_tori; ++j)
          if((active >> j) & 1u)
          {
            e0 = e0 + a.media.m[j].emission[0];
            e1 = e1 + a.media.m[j].emission[1];
            e2 = e2 + a.media.m[j].emission[2];
            sg = sg + a.media.m[j].sigma;
          }
        glow_step(e0, e1, e2, sg, (v - u) * len, Lr, Lg, Lb, T);
      });
    st4(a.rgba + 4 * i, make_float4(Lr, Lg, Lb, T));
  });
}

// ------------------------------------------------------------------------------------------
// glow_profile(rays_in → radiance and transmittance, the media varying across the tubes)
// ------------------------------------------------------------------------------------------
// SceneK without its materials, which no kernel of this unit reads: with the profiles (2176 B) beside it the whole
// struct would not fit the 4-KiB kernel-argument segment.  The members up to `shade` sit where SceneK has them.
struct SceneNoMat {
  uint32_t head[kSceneMat];   // SceneK's header, k32, k64 and shade
  TorusRot rot[TRT_MAX_TORI];
};
static_assert(offsetof(SceneK, mat) == 4 * kSceneMat && sizeof(SceneNoMat) == 4 * (kSceneMat + 72), "SceneNoMat layout");
static_assert(sizeof(SceneNoMat) + sizeof(GlowProfileArgs) <= 4096, "the kernel-argument segment of glow_profile_kernel");
// stage_scene for a SceneNoMat: the records in use, each to its place in the SceneK in LDS (n_mat is not read behind it).
template <bool ORIENT>
__device__ __forceinline__ void stage_scene_no_mat(SceneK* lds, const SceneNoMat& arg)
{
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&arg);
  uint32_t*       dst = reinterpret_cast<uint32_t*>(lds);
  const uint32_t  n = arg.head[0], f64 = arg.head[2];   // SceneK::n_tori, SceneK::f64
  const uint32_t  c0 = kSceneHdr, c1 = c0 + (f64 ? 0u : 10u * n), c2 = c1 + (f64 ? 20u * n : 0u), c3 = c2 + 5u * n;
  const uint32_t  c4 = c3 + (ORIENT ? 9u * n : 0u);
  for(uint32_t i = threadIdx.x; i < c4; i += blockDim.x)
  {
    if(i >= c3)
      dst[kSceneRot + (i - c3)] = src[kSceneMat + (i - c3)];
    else
    {
      const uint32_t off = i < c0 ? i : i < c1 ? kSceneK32 + (i - c0) : i < c2 ? kSceneK64 + (i - c1) : kSceneShade + (i - c2);
      dst[off] = src[off];
    }
  }
}
// What the launches of those kernels pass for the scene.
inline SceneNoMat scene_no_mat(const SceneK& scene)
{
  SceneNoMat sc;
  std::memcpy(sc.head, &scene, sizeof sc.head);
  std::memcpy(sc.rot, scene.rot, sizeof sc.rot);
  return sc;
}

// The knot k and the fraction f of a label x = rho² / r²: y = min(x, 1) · 16 (a NaN x goes to the wall), k = min((int)y, 15),
// f = y − k.  knot_of returns y, from which knot_split gives k and f again.
__device__ __forceinline__ void knot_split(float y, int& k, float& f)
{
  k = min((int)y, 15);
  f = y - (float)k;
}
__device__ __forceinline__ float knot_of(float x, int& k, float& f)
{
  const float y = (x < 1.0f ? x : 1.0f) * 16.0f;
  knot_split(y, k, f);
  return y;
}
// The knots k and k + 1 of one profile, interpolated at x: channel c = fma(f, knot[k+1][c] − knot[k][c], knot[k][c]); added to acc.
__device__ __forceinline__ void profile_add(const float4* knots, float x, float4& acc)
{
  int   k;
  float f;
  knot_of(x, k, f);
  const float4 lo = knots[k], hi = knots[k + 1];
  acc.x = acc.x + fma_(f, hi.x - lo.x, lo.x);
  acc.y = acc.y + fma_(f, hi.y - lo.y, lo.y);
  acc.z = acc.z + fma_(f, hi.z - lo.z, lo.z);
  acc.w = acc.w + fma_(f, hi.w - lo.w, lo.w);
}
// The two Gauss–Legendre parameters of sub-step s of a piece that starts at u, h being the sub-step's length in t:
// its middle m = fma(s + 0.5, h, u), and m ∓ h / (2 √3).
__device__ __forceinline__ void gauss_pair(uint32_t s, float h, float u, float& ta, float& tb)
{
  const float m = fma_((float)s + 0.5f, h, u);
  ta = fma_(-0.288675135f, h, m);
  tb = fma_(0.288675135f, h, m);
}

// The pieces of the tori with a profile (bit j of prof.present), each cut into a.sub.steps equal sub-steps; at the two
// Gauss–Legendre points of a sub-step every active torus is asked for x = rho² / r² at the point — in the solver's frame
// and precision — and its table for the four channels there; the two sums are averaged and go through
// glow_step.  The sub-step loop and the torus loop are uniform for the wave (their bounds come from the arguments) and
// predicated by the lane's mask.  The knot index differs from lane to lane, so the tables are staged into LDS once per
// block: a knot is one 16-byte read.  The ray in an oriented torus' frame depends on the ray and the torus alone, but
// holding it for n_tori tori would take a private array or as much LDS again as the columns: it is formed once per
// sub-step and torus, for both points.
template <class Real, bool ORIENT = false>
__global__ __launch_bounds__(256) void glow_profile_kernel(const SceneNoMat scene, const GlowProfileArgs a)
{
  __shared__ SceneK S;
  __shared__ float4 knots[TRT_MAX_TORI * TRT_PROFILE_KNOTS];
  extern __shared__ float crossing_lds[];   // [K][256] t, then [K][256] bytes
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&a.prof.p[0]);
    uint32_t*       dst = reinterpret_cast<uint32_t*>(knots);
    for(uint32_t i = threadIdx.x; i < 4u * TRT_PROFILE_KNOTS * scene.head[0]; i += blockDim.x)
      dst[i] = src[i];
  }
  stage_scene_no_mat<ORIENT>(&S, scene);
  __syncthreads();   // publishes the tables and the scene

  const uint32_t K  = 4u * (uint32_t)S.n_tori;
  float*         ct = crossing_lds + threadIdx.x;
  uint8_t*       cw = reinterpret_cast<uint8_t*>(crossing_lds + K * 256u) + threadIdx.x;

  const int n_tori = (int)scene.head[0];
  for_each_ray(a.in, a.stats, [&](uint64_t i, uint32_t& tests, WorkCount& wc) {
    float      Lr = 0.0f, Lg = 0.0f, Lb = 0.0f, T = 1.0f, len;
    RayK<Real> r;
    if(media_ray(a.in, i, r, len))
      merged_pieces<Real, ORIENT, 256u>(S, r, a.prof.present, ct, cw, K, tests, wc, [&](float u, float v, uint32_t active) {
        const float h = (v - u) * a.sub.inv_steps;
        const float l = h * len;
        for(uint32_t s = 0; s < a.sub.steps; ++s)
        {
          float ta, tb;
          gauss_pair(s, h, u, ta, tb);
          float4 A = make_float4(0.0f, 0.0f, 0.0f, 0.0f), B = A;
          for(int j = 0; j < n_tori; ++j)
            if((active >> j) & 1u)
            {
              LocalRay<Real> lr;
              TorusK<Real>   Tk;
              tube_frame<Real, ORIENT>(S, j, r, lr, Tk);
              const float ir = a.prof.inv_r2[j];
              profile_add(knots + j * TRT_PROFILE_KNOTS, (float)tube_rho2(lr, Tk, (Real)ta) * ir, A);
              profile_add(knots + j * TRT_PROFILE_KNOTS, (float)tube_rho2(lr, Tk, (Real)tb) * ir, B);
            }
          glow_step((A.x + B.x) * 0.5f, (A.y + B.y) * 0.5f, (A.z + B.z) * 0.5f, (A.w + B.w) * 0.5f, l, Lr, Lg, Lb, T);
        }
      });
    st4(a.rgba + 4 * i, make_float4(Lr, Lg, Lb, T));
  });
}

// ------------------------------------------------------------------------------------------
// glow_weights(rays_in → 17 · n_tori streams: the hat-weighted length of every ray per knot and torus)
// ------------------------------------------------------------------------------------------
// The sub-steps inside every interval of a torus: no column, no merge — torus j's intervals are trt_chords', whatever the
// other tori do.  At each of the two Gauss–Legendre points of a sub-step the label x = rho² / r² picks the knot kn and the
// fraction f, and half the sub-step's world length goes to the accumulators kn and kn + 1 as g · (1 − f) and g · f.
// kn differs from lane to lane, so the 17 accumulators are not registers (a private array indexed by kn would go to
// scratch) but a column of LDS: acc[k][256], the lane's slot k at acc[k * 256 + threadIdx.x].  Within a wave the 64 lanes
// of one access sit on 64 different banks whatever their k is (k * 256 words is a multiple of 64): no conflict.  A lane
// touches its own column only, so nothing but the scene staging needs a barrier.  Per torus: zero the column, walk, store
// the 17 values to their 17 streams (one instruction of 64 consecutive floats each).  The ray in an oriented torus' frame
// is formed once per torus.  The sub-step loop and the torus loop are uniform for the wave.
constexpr uint32_t kWeightLanes = 256;
template <class Real, bool ORIENT = false>
__global__ __launch_bounds__(256) void glow_weights_kernel(const SceneK scene, const GlowWeightsArgs a)
{
  __shared__ SceneK S;
  __shared__ float  acc[TRT_PROFILE_KNOTS * kWeightLanes];
  stage_scene<ORIENT>(&S, scene);
  float* const W = acc + threadIdx.x;

  for_each_ray(a.in, a.stats, [&](uint64_t i, uint32_t& tests, WorkCount& wc) {
    RayK<Real> r;
    float      len = 0.0f;
    const bool window = media_ray(a.in, i, r, len);
    for(int k = 0; k < scene.n_tori; ++k)
    {
      const int j = S.order[k];
      for(uint32_t c = 0; c < TRT_PROFILE_KNOTS; ++c)
        W[c * kWeightLanes] = 0.0f;
      if(window)
      {
        ++tests;
        LocalRay<Real> lr;
        TorusK<Real>   Tk;
        tube_frame<Real, ORIENT>(S, j, r, lr, Tk);
        const float ir = a.inv_r2[j];
        tube_intervals<Real, ORIENT>(S, j, r, wc, [&](float u, float v, bool, bool) {
          const float h = (v - u) * a.sub.inv_steps;
          const float l = h * len;
          const float g = l * 0.5f;
          for(uint32_t s = 0; s < a.sub.steps; ++s)
          {
            float t[2];
            gauss_pair(s, h, u, t[0], t[1]);
            for(int side = 0; side < 2; ++side)
            {
              int   kn;
              float f;
              knot_of((float)tube_rho2(lr, Tk, (Real)t[side]) * ir, kn, f);
              float* const w = W + (uint32_t)kn * kWeightLanes;
              w[0]            = fma_(g, 1.0f - f, w[0]);
              w[kWeightLanes] = fma_(g, f, w[kWeightLanes]);
            }
          }
        });
      }
      for(uint32_t c = 0; c < TRT_PROFILE_KNOTS; ++c)
        st1(a.weight, ((uint64_t)j * TRT_PROFILE_KNOTS + c) * a.in.rays.n + i, W[c * kWeightLanes]);
    }
  });
}

// ------------------------------------------------------------------------------------------
// glow_weights_absorbed(rays_in → 17 · n_tori streams and the transmittance: the weights behind absorbing media)
// ------------------------------------------------------------------------------------------
// The merged pieces with EVERY torus present, cut into sub-steps, and the deposit of glow_weights_kernel: in every
// sub-step the sigma of the active tori is summed at the two Gauss–Legendre points as profile_add sums channel 3, the step
// gives E and the weight w (glow_step_weight), and g = (w · 0.5) · T — T in front of the sub-step — goes to the knots kn
// and kn + 1 of every active torus at both points.  A sub-step deposits into every active torus, so the accumulators of
// ALL tori are live at once: 17 · n_tori floats per lane, lane-minor in dynamic LDS (acc[(j · 17 + k) · LANES + lane]: the
// 64 lanes of an access sit on 64 different banks whatever their k is).  Behind them, per lane: y = min(x, 1) · 16 of the
// two points for every torus (2 · n_tori floats) — kn and f come from y alone, so the deposit reads them back instead of
// forming the point in the torus' frame a second time, and no private array indexed by j goes to scratch — and the 4 · n_tori
// slots of the crossing column.  96 · n_tori bytes per lane in all: the host picks LANES (256, 128 or 64) from n_tori so
// that a block stays below 64 KiB.  A lane touches its own columns only and the order of the additions into an
// accumulator is the walk's, so the result does not depend on LANES and nothing but the staging needs a barrier.
//
// Three kernels run this walk and differ in what leaves the chip behind it: glow_weights_absorbed_kernel stores the
// columns, glow_project_kernel their FP64 dot products with the emission tables, glow_backproject_kernel their products
// with an image, reduced over the rays.  What they share is said once: absorbed_stage (the sigma tables and the scene into
// LDS), AbsorbedLane (where a lane's columns are) and absorbed_ray (the walk of one ray into the lane's accumulators).
constexpr uint32_t kAbsorbedLaneBytes = 4u * (TRT_PROFILE_KNOTS + 2u) + 4u * (uint32_t)(sizeof(float) + sizeof(uint8_t));   // per torus: 96
static_assert(sizeof(SceneNoMat) + sizeof(GlowWeightsAbsorbedArgs) <= 4096, "the kernel-argument segment of glow_weights_absorbed_kernel");
static_assert(sizeof(SceneNoMat) + sizeof(GlowProfileArgs) <= 4096, "the kernel-argument segment of glow_project_kernel");
static_assert(sizeof(SceneNoMat) + sizeof(GlowBackprojectArgs) <= 4096, "the kernel-argument segment of glow_backproject_kernel");
// sigma[j * 17 + k] = src[(j * 17 + k) * step]: GlowWeightsAbsorbedArgs' packed tables (step 1), or channel 3 of
// trt_profile's knots (step 4, src at knot[0][3]).  Ends with the barrier that publishes the tables and the scene.
template <bool ORIENT, uint32_t LANES>
__device__ __forceinline__ void absorbed_stage(SceneK* S, float* sigma, const SceneNoMat& scene, const float* src, uint32_t step)
{
  for(uint32_t i = threadIdx.x; i < TRT_PROFILE_KNOTS * scene.head[0]; i += LANES)
    sigma[i] = src[i * step];
  stage_scene_no_mat<ORIENT>(S, scene);
  __syncthreads();
}
// The lane's columns in the block's dynamic LDS: [17 n_tori][LANES] acc, [2 n_tori][LANES] y, [K][LANES] t, [K][LANES] bytes.
template <uint32_t LANES>
struct AbsorbedLane {
  uint32_t K, n_acc;
  float*   W;
  float*   Y;
  float*   ct;
  uint8_t* cw;
  __device__ __forceinline__ AbsorbedLane(float* lane_lds, uint32_t n_tori)
    : K(4u * n_tori), n_acc(TRT_PROFILE_KNOTS * n_tori), W(lane_lds + threadIdx.x), Y(lane_lds + n_acc * LANES + threadIdx.x),
      ct(lane_lds + (n_acc + 2u * n_tori) * LANES + threadIdx.x),
      cw(reinterpret_cast<uint8_t*>(lane_lds + (n_acc + 2u * n_tori + K) * LANES) + threadIdx.x)
  {
  }
};
// g to the hats of a sub-step, for every active torus j from the y of its two points in Y: g · (1 − f) to the accumulator
// kn and g · f to kn + 1, at t-, then at t+.  The four accumulators are read at once — one LDS latency per torus, not four
// in a row — and where t+ falls on a slot of t- it adds to what t- left there: the same operations in the same order per
// accumulator.  The stores go out t- first, so that a shared slot keeps the value with both deposits.
template <uint32_t LANES>
__device__ __forceinline__ void hat_deposit(float* const& W, const float* const& Y, const uint32_t& n_tori, const uint32_t& active, const float g)
{
  for(uint32_t j = 0; j < n_tori; ++j)
    if((active >> j) & 1u)
    {
      int   ka, kb;
      float fa, fb;
      knot_split(Y[(2u * j) * LANES], ka, fa);
      knot_split(Y[(2u * j + 1u) * LANES], kb, fb);
      float* const wa = W + (j * TRT_PROFILE_KNOTS + (uint32_t)ka) * LANES;
      float* const wb = W + (j * TRT_PROFILE_KNOTS + (uint32_t)kb) * LANES;
      float a0 = wa[0], a1 = wa[LANES], b0 = wb[0], b1 = wb[LANES];
      a0 = fma_(g, 1.0f - fa, a0);
      a1 = fma_(g, fa, a1);
      b0 = kb == ka ? a0 : (kb == ka + 1 ? a1 : b0);
      b1 = kb == ka ? a1 : (kb + 1 == ka ? a0 : b1);
      b0 = fma_(g, 1.0f - fb, b0);
      b1 = fma_(g, fb, b1);
      wa[0]     = a0;
      wa[LANES] = a1;
      wb[0]     = b0;
      wb[LANES] = b1;
    }
}
// Ray i of `in` walked into the lane's accumulators (zeroed first; an empty window leaves them zero and executes no
// test); returns the transmittance left.  (Parameters by reference, for column_insert's reason.)
template <class Real, bool ORIENT, uint32_t LANES>
__device__ __forceinline__ float absorbed_ray(const SceneK& S, const float* const& sigma, const MediaRays& in, const MediaSteps& sub,
                                              const float (&inv_r2)[TRT_MAX_TORI], const uint32_t& n_tori, const uint64_t& i,
                                              const AbsorbedLane<LANES>& lane, uint32_t& tests, WorkCount& wc)
{
  float* const W = lane.W;
  float* const Y = lane.Y;
  {
    float      T = 1.0f, len;
    RayK<Real> r;
    const bool window = media_ray(in, i, r, len);
    for(uint32_t c = 0; c < lane.n_acc; ++c)
      W[c * LANES] = 0.0f;
    if(window)
      merged_pieces<Real, ORIENT, LANES>(S, r, ~0u, lane.ct, lane.cw, lane.K, tests, wc, [&](float u, float v, uint32_t active) {
        const float h = (v - u) * sub.inv_steps;
        const float l = h * len;
        for(uint32_t s = 0; s < sub.steps; ++s)
        {
          float ta, tb;
          gauss_pair(s, h, u, ta, tb);
          float A = 0.0f, B = 0.0f;
          for(uint32_t j = 0; j < n_tori; ++j)
            if((active >> j) & 1u)
            {
              LocalRay<Real> lr;
              TorusK<Real>   Tk;
              tube_frame<Real, ORIENT>(S, (int)j, r, lr, Tk);
              const float ir = inv_r2[j];
              int         ka, kb;
              float       fa, fb;
              const float ya = knot_of((float)tube_rho2(lr, Tk, (Real)ta) * ir, ka, fa);
              const float yb = knot_of((float)tube_rho2(lr, Tk, (Real)tb) * ir, kb, fb);
              const float* const sg = sigma + j * TRT_PROFILE_KNOTS;
              A = A + fma_(fa, sg[ka + 1] - sg[ka], sg[ka]);
              B = B + fma_(fb, sg[kb + 1] - sg[kb], sg[kb]);
              Y[(2u * j) * LANES]      = ya;
              Y[(2u * j + 1u) * LANES] = yb;
            }
          float E, wgt;
          glow_step_weight((A + B) * 0.5f, l, E, wgt);
          hat_deposit<LANES>(W, Y, n_tori, active, (wgt * 0.5f) * T);
          T = T * E;
        }
      });
    return T;
  }
}

template <class Real, bool ORIENT, uint32_t LANES>
__global__ __launch_bounds__(LANES) void glow_weights_absorbed_kernel(const SceneNoMat scene, const GlowWeightsAbsorbedArgs a)
{
  __shared__ SceneK S;
  __shared__ float  sigma[TRT_MAX_TORI * TRT_PROFILE_KNOTS];
  extern __shared__ float lane_lds[];
  const uint32_t n_tori = scene.head[0];
  absorbed_stage<ORIENT, LANES>(&S, sigma, scene, &a.sigma[0][0], 1u);
  const AbsorbedLane<LANES> lane(lane_lds, n_tori);

  // (for_each_ray's loop, written out: as a callback, this kernel's body has its scalar registers spilt to lanes — 18 more
  // v_writelane, 16 more v_readlane — and its 64-step rows measure 1.2 to 1.7 % slower; profiles/r29_media_one_walk.txt)
  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * LANES;
  for(uint64_t i = (uint64_t)blockIdx.x * LANES + threadIdx.x; i < a.in.rays.n; i += stride)
  {
    const float T = absorbed_ray<Real, ORIENT, LANES>(S, sigma, a.in, a.sub, a.inv_r2, n_tori, i, lane, tests, wc);
    for(uint32_t c = 0; c < lane.n_acc; ++c)
      st1(a.weight, (uint64_t)c * a.in.rays.n + i, lane.W[c * LANES]);
    if(a.trans)
      st1(a.trans, i, T);
  }
  if(a.stats)
    block_add_stats(a.stats, tests, 0u, 0u, wc);
}

// ------------------------------------------------------------------------------------------
// glow_project(rays_in → W · x and the transmittance): the forward product with exactly those weights
// ------------------------------------------------------------------------------------------
// Behind a ray's walk the lane reads its own column back, torus by torus and knot by knot, and forms the three dot products
// with the emission tables as include/trt.h states them: p = p + (double)W · (double)knot, the product exact, one rounded
// FP64 addition (the unit is compiled with -ffp-contract=off; a contracted fma would round the same sum once as well, the
// product being exact).  The tables stay in the kernel arguments: j and k are uniform for the wave, so a knot is a scalar
// load and costs no LDS.  One 16-byte store per ray; no weight leaves the chip.
template <class Real, bool ORIENT, uint32_t LANES>
__global__ __launch_bounds__(LANES) void glow_project_kernel(const SceneNoMat scene, const GlowProfileArgs a)
{
  __shared__ SceneK S;
  __shared__ float  sigma[TRT_MAX_TORI * TRT_PROFILE_KNOTS];
  extern __shared__ float lane_lds[];
  const uint32_t n_tori = scene.head[0];
  absorbed_stage<ORIENT, LANES>(&S, sigma, scene, &a.prof.p[0].knot[0][3], 4u);
  const AbsorbedLane<LANES> lane(lane_lds, n_tori);

  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * LANES;
  for(uint64_t i = (uint64_t)blockIdx.x * LANES + threadIdx.x; i < a.in.rays.n; i += stride)
  {
    const float T = absorbed_ray<Real, ORIENT, LANES>(S, sigma, a.in, a.sub, a.prof.inv_r2, n_tori, i, lane, tests, wc);
    double      pr = 0.0, pg = 0.0, pb = 0.0;
    for(uint32_t j = 0; j < n_tori; ++j)
      for(uint32_t k = 0; k < TRT_PROFILE_KNOTS; ++k)
      {
        const double w = (double)lane.W[(j * TRT_PROFILE_KNOTS + k) * LANES];
        pr = pr + w * (double)a.prof.p[j].knot[k][0];
        pg = pg + w * (double)a.prof.p[j].knot[k][1];
        pb = pb + w * (double)a.prof.p[j].knot[k][2];
      }
    st4(a.rgba + 4 * i, make_float4((float)pr, (float)pg, (float)pb, T));
  }
  if(a.stats)
    block_add_stats(a.stats, tests, 0u, 0u, wc);
}

// ------------------------------------------------------------------------------------------
// glow_backproject(rays_in, y → Wᵀ y and the column sums, in FP64): the adjoint with exactly those weights
// ------------------------------------------------------------------------------------------
// A block takes the rays in rounds of LANES (grid-stride; the loop is uniform for the block, a lane behind the last ray
// holds a zero column and a zero y).  Behind a round's walks the block holds W[c][lane] for its LANES rays in LDS, and
// reduces them against y over the lanes by a TRANSPOSED read: thread e of a pass owns the output (row c = e >> 2, channel
// ch = e & 3) and adds the LANES terms (double)W[c][l] · (double)y[l][ch] — each product exact in FP64 — one after the
// other into an FP64 accumulator.  Channel 3 of y is replaced by 1.0f on the way in: its output is the column sum.
//   Why not cross-lane operations: a wave-wide tree over DPP takes six FP64 additions and twelve register moves per lane
//   and output — 4 · 17 · n_tori outputs, so 3264 additions per lane and round for eight tori — where the transposed read
//   takes ONE addition per lane and output, and two LDS reads.
//   Banks: the four threads of a row read the same word of W (a broadcast), and the 16 rows of a wave start their walk over
//   the lanes rotated by c — l = (step + c) mod LANES — so that they sit on 16 different banks (c · LANES is a multiple of
//   64).  y lies lane-major, four floats per lane: the wave's 16 lanes times four channels are 64 consecutive words.  The
//   order of a row's additions is therefore rotated by its c, and fixed: the same bits from every launch.
//   Where y lies: in the lane's y and crossing columns, which are dead behind the walk (24 · n_tori bytes per lane; 16 are
//   needed) — a barrier in front (every walk of the round has ended) and one behind the reduction (the next round's walks
//   overwrite them).
//   The partials over the rounds: 4 · 17 · n_tori FP64 values per block.  They are the threads' REGISTERS, not LDS: a
//   block of 128 lanes for five tori has 1704 bytes of its 64 KiB left, and the 2720 that its partials take do not fit.
//   The pass loop is unrolled (PASSES = the outputs of the widest scene of this block width over LANES: 1, 3 or 9), so
//   acc[] is never indexed at run time and stays in 2 · PASSES registers.  An output belongs to one thread for the whole
//   kernel, so its additions are ordered without any atomic.
// At its end the block writes its row of 4 · 17 · n_tori doubles to partials[blockIdx.x]; backproject_sum_kernel adds the rows
// in index order.  No floating-point atomics anywhere: the bits depend on (n, the grid, LANES) alone.
static_assert(4u * sizeof(float) <= (2u + 4u) * sizeof(float), "a lane's y fits its dead y and t columns for one torus already: the reduction adds no LDS");
template <class Real, bool ORIENT, uint32_t LANES>
__global__ __launch_bounds__(LANES) void glow_backproject_kernel(const SceneNoMat scene, const GlowBackprojectArgs a)
{
  constexpr uint32_t kMaxTori = LANES == 256u ? 2u : LANES == 128u ? 5u : TRT_MAX_TORI;
  constexpr uint32_t PASSES   = (4u * TRT_PROFILE_KNOTS * kMaxTori + LANES - 1u) / LANES;
  __shared__ SceneK S;
  __shared__ float  sigma[TRT_MAX_TORI * TRT_PROFILE_KNOTS];
  extern __shared__ float lane_lds[];
  const uint32_t n_tori = scene.head[0];
  absorbed_stage<ORIENT, LANES>(&S, sigma, scene, &a.sigma[0][0], 1u);
  const AbsorbedLane<LANES> lane(lane_lds, n_tori);
  const uint32_t n_out = 4u * lane.n_acc;
  float* const   ys    = lane_lds + lane.n_acc * LANES;   // [LANES][4]

  double acc[PASSES];
#pragma unroll
  for(uint32_t p = 0; p < PASSES; ++p)
    acc[p] = 0.0;

  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * LANES;
  for(uint64_t base = (uint64_t)blockIdx.x * LANES; base < a.in.rays.n; base += stride)
  {
    const uint64_t i = base + threadIdx.x;
    float          y0 = 0.0f, y1 = 0.0f, y2 = 0.0f;
    if(i < a.in.rays.n)
    {
      absorbed_ray<Real, ORIENT, LANES>(S, sigma, a.in, a.sub, a.inv_r2, n_tori, i, lane, tests, wc);
      const f4v y = *((gptr<const f4v>)(a.y + 4 * i));
      y0 = y.x;
      y1 = y.y;
      y2 = y.z;
    }
    else
      for(uint32_t c = 0; c < lane.n_acc; ++c)
        lane.W[c * LANES] = 0.0f;
    __syncthreads();   // every walk of the round has ended: the columns are whole, the y and crossing columns dead
    ys[4u * threadIdx.x]      = y0;
    ys[4u * threadIdx.x + 1u] = y1;
    ys[4u * threadIdx.x + 2u] = y2;
    ys[4u * threadIdx.x + 3u] = 1.0f;
    __syncthreads();
#pragma unroll
    for(uint32_t p = 0; p < PASSES; ++p)
    {
      const uint32_t e = p * LANES + threadIdx.x;
      if(e < n_out)
      {
        const uint32_t     c = e >> 2, ch = e & 3u;
        const float* const w = lane_lds + c * LANES;
        double             s = acc[p];
#pragma unroll 4
        for(uint32_t step = 0; step < LANES; ++step)   // (unrolled by four: whole, the nine passes of 64 lanes spill)
        {
          const uint32_t l = (step + c) & (LANES - 1u);
          s = s + (double)w[l] * (double)ys[4u * l + ch];
        }
        acc[p] = s;
      }
    }
    __syncthreads();   // the next round's walks write where y lies
  }
#pragma unroll
  for(uint32_t p = 0; p < PASSES; ++p)
  {
    const uint32_t e = p * LANES + threadIdx.x;
    if(e < n_out)
      ((gptr<double>)a.partials)[(uint64_t)blockIdx.x * n_out + e] = acc[p];
  }
  if(a.stats)
    block_add_stats(a.stats, tests, 0u, 0u, wc);
}
// back[e] = 0.0 + partials[0][e] + partials[1][e] + … in row order, one thread per output: `rows` dependent FP64 additions
// (2048 at the most), the loads in front of them.  rows == 0 (no ray) writes zeros.
__global__ __launch_bounds__(256) void backproject_sum_kernel(const double* partials, uint32_t rows, uint32_t n_out, double* back)
{
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if(e >= n_out)
    return;
  double s = 0.0;
#pragma unroll 8
  for(uint32_t r = 0; r < rows; ++r)
    s = s + ((gptr<const double>)partials)[(uint64_t)r * n_out + e];
  ((gptr<double>)back)[e] = s;
}

// ------------------------------------------------------------------------------------------
// glow_tangent, glow_adjoint: J v and Jᵀ y of the forward rule with respect to all four channels of the tables
// ------------------------------------------------------------------------------------------
// F maps the tables to (L_r, L_g, L_b, T) of a ray by glow_project_kernel's rule in exact arithmetic; include/trt.h states
// its derivative.  Per sub-step s, with e and sg the tables at the hats of the sub-step, l its world length, E and w as
// glow_step_weight gives them, T_s the transmittance in front of it:
//   dL_c = Σ_s [ de_c · w · T_s + dsg · (e_c · w' · T_s − l · B_c) ]     B_c: what arrives from behind s;   dT = −T Σ_s l · dsg
// w' = ∂w/∂sg = (l · E − w) / sg.  The quotient cancels at small τ = sg · l (l · E and w both go to l), so below
// kGlowSlopeSeries it is the series l² · Q(τ), Q(τ) = Σ_m (−1)^(m+1) (m + 1) / (m + 2)! · τ^m = −1/2 + τ/3 − τ²/8 + τ³/30 − …
// to τ¹⁰, Horner with fma: the series alternates with falling terms, so what is left out is below the first term left
// out, 12/13! = 1.93e-9 at τ = 1 against |Q| >= 0.264 there — 7.3e-9 relative.  At τ >= 1 the quotient loses a factor
// 2 (1 + 1/τ) E / |E − (1 − E)/τ| <= 2.8 on E's rounding.  sg = 0 takes the series: −l²/2, the continuous limit.  The
// threshold is on τ alone and l enters by products only: a scene scaled by a power of two with the tables scaled the
// other way gives the same bits times that power.
constexpr float kGlowSlopeSeries = 1.0f;
__device__ __forceinline__ float glow_step_slope(float sg, float l, float E, float wgt)
{
  const float tau = sg * l;
  if(!(tau < kGlowSlopeSeries))
    return (l * E - wgt) / sg;
  float q = fma_(tau, -2.29644327e-8f, 2.50521084e-7f);   // -11/12!, 10/11!
  q = fma_(tau, q, -2.48015873e-6f);                      // -9/10!
  q = fma_(tau, q, 2.20458554e-5f);                       // 8/9!
  q = fma_(tau, q, -1.73611111e-4f);                      // -7/8!
  q = fma_(tau, q, 1.19047619e-3f);                       // 6/7!
  q = fma_(tau, q, -6.94444444e-3f);                      // -5/6!
  q = fma_(tau, q, 3.33333333e-2f);                       // 4/5!
  q = fma_(tau, q, -0.125f);                              // -3/4!
  q = fma_(tau, q, 3.33333333e-1f);                       // 2/3!
  q = fma_(tau, q, -0.5f);                                // -1/2!
  return l * (l * q);
}

// each(j, xa, xb) for every active torus j: the labels x = rho² / r² of the two Gauss points ta, tb of a sub-step, formed
// as glow_profile_kernel and absorbed_ray form them.
template <class Real, bool ORIENT, class Each>
__device__ __forceinline__ void substep_labels(const SceneK& S, const RayK<Real>& r, const float (&inv_r2)[TRT_MAX_TORI], const uint32_t& n_tori,
                                               const uint32_t& active, float ta, float tb, Each&& each)
{
  for(uint32_t j = 0; j < n_tori; ++j)
    if((active >> j) & 1u)
    {
      LocalRay<Real> lr;
      TorusK<Real>   Tk;
      tube_frame<Real, ORIENT>(S, (int)j, r, lr, Tk);
      const float ir = inv_r2[j];
      each(j, (float)tube_rho2(lr, Tk, (Real)ta) * ir, (float)tube_rho2(lr, Tk, (Real)tb) * ir);
    }
}
// `words` 32-bit words of tables into LDS, from the kernel arguments or from device memory.
__device__ __forceinline__ void stage_tables(float4* lds, const void* src, uint32_t words)
{
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t*       d = reinterpret_cast<uint32_t*>(lds);
  for(uint32_t i = threadIdx.x; i < words; i += blockDim.x)
    d[i] = s[i];
}

// The store kernel in front of glow_tangent_kernel: the direction's tables from its own arguments to the ctx's scratch.
struct ProfileTables {
  trt_profile p[TRT_MAX_TORI];
};
__global__ __launch_bounds__(256) void store_tables_kernel(const ProfileTables t, float* dst)
{
  const uint32_t  i   = blockIdx.x * 256u + threadIdx.x;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&t);
  if(i < sizeof(ProfileTables) / 4u)
    ((gptr<uint32_t>)reinterpret_cast<uint32_t*>(dst))[i] = src[i];
}

// glow_profile_kernel's layout — one lane per ray, 256 lanes, the crossing column in dynamic LDS — with every torus present
// and two tables in static LDS: the point of linearisation from the arguments, the direction from `delta` (device memory:
// both do not fit the argument segment).  Forward mode needs one sweep: with D = −Σ_{s'<s} l · dsg carried along, the term
// −dsg_{s'} · l_{s'} · B summed over s' is Σ_s e_c · w · T_s · D_s, and dT = T · D.  D is carried with its sign — fma(−l, dsg, D)
// stays +0 where no sigma moves — so that dT is +0 there, not −0.  No per-torus accumulator: 256 lanes at every n_tori.
static_assert(sizeof(SceneNoMat) + sizeof(GlowProfileArgs) + sizeof(float*) <= 4096, "the kernel-argument segment of glow_tangent_kernel");
static_assert(sizeof(ProfileTables) + sizeof(float*) <= 4096, "the kernel-argument segment of store_tables_kernel");
template <class Real, bool ORIENT = false>
__global__ __launch_bounds__(256) void glow_tangent_kernel(const SceneNoMat scene, const GlowProfileArgs a, const float* delta)
{
  __shared__ SceneK S;
  __shared__ float4 knots[TRT_MAX_TORI * TRT_PROFILE_KNOTS];
  __shared__ float4 dknots[TRT_MAX_TORI * TRT_PROFILE_KNOTS];
  extern __shared__ float crossing_lds[];   // [K][256] t, then [K][256] bytes
  const uint32_t n_tori = scene.head[0];
  stage_tables(knots, &a.prof.p[0], 4u * TRT_PROFILE_KNOTS * n_tori);
  {
    const gptr<const uint32_t> src = (gptr<const uint32_t>)reinterpret_cast<const uint32_t*>(delta);
    uint32_t*                  dst = reinterpret_cast<uint32_t*>(dknots);
    for(uint32_t i = threadIdx.x; i < 4u * TRT_PROFILE_KNOTS * n_tori; i += blockDim.x)
      dst[i] = src[i];
  }
  stage_scene_no_mat<ORIENT>(&S, scene);
  __syncthreads();   // publishes the tables and the scene

  const uint32_t K  = 4u * n_tori;
  float*         ct = crossing_lds + threadIdx.x;
  uint8_t*       cw = reinterpret_cast<uint8_t*>(crossing_lds + K * 256u) + threadIdx.x;

  for_each_ray(a.in, a.stats, [&](uint64_t i, uint32_t& tests, WorkCount& wc) {
    float      Lr = 0.0f, Lg = 0.0f, Lb = 0.0f, T = 1.0f, D = 0.0f, len;
    RayK<Real> r;
    if(media_ray(a.in, i, r, len))
      merged_pieces<Real, ORIENT, 256u>(S, r, ~0u, ct, cw, K, tests, wc, [&](float u, float v, uint32_t active) {
        const float h = (v - u) * a.sub.inv_steps;
        const float l = h * len;
        for(uint32_t s = 0; s < a.sub.steps; ++s)
        {
          float ta, tb;
          gauss_pair(s, h, u, ta, tb);
          float4 A = make_float4(0.0f, 0.0f, 0.0f, 0.0f), B = A, dA = A, dB = A;
          substep_labels<Real, ORIENT>(S, r, a.prof.inv_r2, n_tori, active, ta, tb, [&](uint32_t j, float xa, float xb) {
            profile_add(knots + j * TRT_PROFILE_KNOTS, xa, A);
            profile_add(knots + j * TRT_PROFILE_KNOTS, xb, B);
            profile_add(dknots + j * TRT_PROFILE_KNOTS, xa, dA);
            profile_add(dknots + j * TRT_PROFILE_KNOTS, xb, dB);
          });
          const float e0 = (A.x + B.x) * 0.5f, e1 = (A.y + B.y) * 0.5f, e2 = (A.z + B.z) * 0.5f, sg = (A.w + B.w) * 0.5f;
          const float d0 = (dA.x + dB.x) * 0.5f, d1 = (dA.y + dB.y) * 0.5f, d2 = (dA.z + dB.z) * 0.5f, dsg = (dA.w + dB.w) * 0.5f;
          float E, wgt;
          glow_step_weight(sg, l, E, wgt);
          const float k = dsg * glow_step_slope(sg, l, E, wgt);
          // (de · w + dsg · w' · e + e · w · D) · T: with dsg == 0 and D == 0 this is glow_step's e · w · T of de, to the bit
          Lr = fma_(fma_(e0 * wgt, D, fma_(d0, wgt, k * e0)), T, Lr);
          Lg = fma_(fma_(e1 * wgt, D, fma_(d1, wgt, k * e1)), T, Lg);
          Lb = fma_(fma_(e2 * wgt, D, fma_(d2, wgt, k * e2)), T, Lb);
          D  = fma_(-l, dsg, D);
          T  = T * E;
        }
      });
    st4(a.rgba + 4 * i, make_float4(Lr, Lg, Lb, T * D));
  });
}

// The sigma half of the adjoint: G[j][k] = Σ_s λ_s · hat_s[j][k] per ray in AbsorbedLane's layout (G where W is: 96 bytes
// per lane and torus, the same block widths), then Σ over the rays in FP64 as glow_backproject_kernel sums W.
//   λ_s = Σ_{c<3} y_c (e_c · w' · T_s − l · B_c) − y_3 · T · l          B_c = L_c − Σ_{s'<=s} e_c · w · T_{s'}
// B needs the ray's whole L_c and λ its final T, so the ray's stored crossing column is walked TWICE (merged_fill once,
// merged_walk twice: the roots are solved once): the first sweep is glow_profile_kernel's sub-step and leaves L_c and T;
// the second repeats it — the same operations, so its prefix ends on L_c to the bit and B >= 0 throughout, ending at 0 —
// and deposits λ_s / 2 at the hats of both points (hat_deposit).  All four channels of the tables are read: float4 knots
// in static LDS, 1632 B more than absorbed_stage's sigma[].
//   The reduction is glow_backproject_kernel's transposed read with the multiplier 1: thread e owns row c = e and adds the
//   LANES values (double)G[c][l], l = (step + c) mod LANES (64 rows of a wave on 64 banks), into an FP64 register; 17 ·
//   n_tori outputs, so one pass at 256 and 128 lanes and three at 64.  One row of partials per block, summed in row order
//   by adjoint_sum_kernel into slot 3 of every knot.  No floating-point atomics.
struct GlowSigmaAdjointArgs {
  MediaRays           in;
  MediaSteps          sub;
  Profiles            prof;
  const float*        y;
  double*             partials;
  unsigned long long* stats;
};
static_assert(sizeof(SceneNoMat) + sizeof(GlowSigmaAdjointArgs) <= 4096, "the kernel-argument segment of glow_sigma_adjoint_kernel");
template <class Real, bool ORIENT, uint32_t LANES>
__global__ __launch_bounds__(LANES) void glow_sigma_adjoint_kernel(const SceneNoMat scene, const GlowSigmaAdjointArgs a)
{
  constexpr uint32_t kMaxTori = LANES == 256u ? 2u : LANES == 128u ? 5u : TRT_MAX_TORI;
  constexpr uint32_t PASSES   = (TRT_PROFILE_KNOTS * kMaxTori + LANES - 1u) / LANES;
  __shared__ SceneK S;
  __shared__ float4 knots[TRT_MAX_TORI * TRT_PROFILE_KNOTS];
  extern __shared__ float lane_lds[];
  const uint32_t n_tori = scene.head[0];
  stage_tables(knots, &a.prof.p[0], 4u * TRT_PROFILE_KNOTS * n_tori);
  stage_scene_no_mat<ORIENT>(&S, scene);
  __syncthreads();   // publishes the tables and the scene
  const AbsorbedLane<LANES> lane(lane_lds, n_tori);
  float* const G = lane.W;
  float* const Y = lane.Y;

  double acc[PASSES];
#pragma unroll
  for(uint32_t p = 0; p < PASSES; ++p)
    acc[p] = 0.0;

  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * LANES;
  for(uint64_t base = (uint64_t)blockIdx.x * LANES; base < a.in.rays.n; base += stride)
  {
    const uint64_t i = base + threadIdx.x;
    for(uint32_t c = 0; c < lane.n_acc; ++c)
      G[c * LANES] = 0.0f;
    float      len;
    RayK<Real> r;
    if(i < a.in.rays.n && media_ray(a.in, i, r, len))
    {
      uint32_t active0, count;
      merged_fill<Real, ORIENT, LANES>(S, r, ~0u, lane.ct, lane.cw, lane.K, tests, wc, active0, count);
      const f4v y = *((gptr<const f4v>)(a.y + 4 * i));
      // e and sg of sub-step s of the piece (u, u + steps · h) at its two points, whose y go to Y for the deposit if `keep`
      const auto tables_at = [&](auto keep, uint32_t s, float h, float u, uint32_t active, float& e0, float& e1, float& e2, float& sg) {
        float ta, tb;
        gauss_pair(s, h, u, ta, tb);
        float4 A = make_float4(0.0f, 0.0f, 0.0f, 0.0f), B = A;
        substep_labels<Real, ORIENT>(S, r, a.prof.inv_r2, n_tori, active, ta, tb, [&](uint32_t j, float xa, float xb) {
          if constexpr(decltype(keep)::value)
          {
            int   k;
            float f;
            Y[(2u * j) * LANES]      = knot_of(xa, k, f);
            Y[(2u * j + 1u) * LANES] = knot_of(xb, k, f);
          }
          profile_add(knots + j * TRT_PROFILE_KNOTS, xa, A);
          profile_add(knots + j * TRT_PROFILE_KNOTS, xb, B);
        });
        e0 = (A.x + B.x) * 0.5f;
        e1 = (A.y + B.y) * 0.5f;
        e2 = (A.z + B.z) * 0.5f;
        sg = (A.w + B.w) * 0.5f;
      };
      float Lr = 0.0f, Lg = 0.0f, Lb = 0.0f, T = 1.0f;
      merged_walk<Real, LANES>(r, lane.ct, lane.cw, active0, count, [&](float u, float v, uint32_t active) {
        const float h = (v - u) * a.sub.inv_steps;
        const float l = h * len;
        for(uint32_t s = 0; s < a.sub.steps; ++s)
        {
          float e0, e1, e2, sg;
          tables_at(std::false_type{}, s, h, u, active, e0, e1, e2, sg);
          glow_step(e0, e1, e2, sg, l, Lr, Lg, Lb, T);
        }
      });
      const float yT = y.w * T;
      float       Pr = 0.0f, Pg = 0.0f, Pb = 0.0f;
      T = 1.0f;
      merged_walk<Real, LANES>(r, lane.ct, lane.cw, active0, count, [&](float u, float v, uint32_t active) {
        const float h = (v - u) * a.sub.inv_steps;
        const float l = h * len;
        for(uint32_t s = 0; s < a.sub.steps; ++s)
        {
          float e0, e1, e2, sg, E, wgt;
          tables_at(std::true_type{}, s, h, u, active, e0, e1, e2, sg);
          glow_step_weight(sg, l, E, wgt);
          const float k = glow_step_slope(sg, l, E, wgt) * T;
          Pr = fma_(e0 * wgt, T, Pr);   // glow_step's operations: the prefix through s
          Pg = fma_(e1 * wgt, T, Pg);
          Pb = fma_(e2 * wgt, T, Pb);
          float lam = y.x * fma_(-l, Lr - Pr, e0 * k);
          lam = fma_(y.y, fma_(-l, Lg - Pg, e1 * k), lam);
          lam = fma_(y.z, fma_(-l, Lb - Pb, e2 * k), lam);
          lam = fma_(-yT, l, lam);
          hat_deposit<LANES>(G, Y, n_tori, active, lam * 0.5f);
          T = T * E;
        }
      });
    }
    __syncthreads();   // every walk of the round has ended: the columns are whole
#pragma unroll
    for(uint32_t p = 0; p < PASSES; ++p)
    {
      const uint32_t c = p * LANES + threadIdx.x;
      if(c < lane.n_acc)
      {
        const float* const g = lane_lds + c * LANES;
        double             s = acc[p];
#pragma unroll 4
        for(uint32_t step = 0; step < LANES; ++step)
          s = s + (double)g[(step + c) & (LANES - 1u)];
        acc[p] = s;
      }
    }
    __syncthreads();   // the next round's walks zero the columns
  }
#pragma unroll
  for(uint32_t p = 0; p < PASSES; ++p)
  {
    const uint32_t c = p * LANES + threadIdx.x;
    if(c < lane.n_acc)
      ((gptr<double>)a.partials)[(uint64_t)blockIdx.x * lane.n_acc + c] = acc[p];
  }
  if(a.stats)
    block_add_stats(a.stats, tests, 0u, 0u, wc);
}
// grad[4 c + 3] = 0.0 + partials[0][c] + partials[1][c] + … in row order, one thread per knot: backproject_sum_kernel for
// the sigma slot.  rows == 0 (no ray) writes zeros.
__global__ __launch_bounds__(256) void adjoint_sum_kernel(const double* partials, uint32_t rows, uint32_t n_acc, double* grad)
{
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if(c >= n_acc)
    return;
  double s = 0.0;
#pragma unroll 8
  for(uint32_t r = 0; r < rows; ++r)
    s = s + ((gptr<const double>)partials)[(uint64_t)r * n_acc + c];
  ((gptr<double>)grad)[4u * c + 3u] = s;
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
// Default solver only (the enumeration is the walk's: trt_api.hip refuses the others before it gets here): launch(real, ori)
// with the scene's Real as a value and its ORIENT flag as a type, then the launch's error.
template <class Launch>
static hipError_t launch_default_solver(const SceneK& scene, Launch&& launch)
{
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    if constexpr(decltype(alt)::value)
      return hipErrorInvalidValue;
    else
    {
      launch(real, ori);
      return hipGetLastError();
    }
  });
}

hipError_t launch_chords(const SceneK& scene, const ChordsArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.in.rays.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.in.rays.n, tn);
  return launch_default_solver(scene, [&](auto real, auto ori) {
    hipLaunchKernelGGL((chords_kernel<decltype(real), decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
  });
}

// 4 · n_tori slots per lane: 5 KiB of columns for one torus, 40 KiB for eight (shade_through_kernel's).
hipError_t launch_glow(const SceneK& scene, const GlowArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.in.rays.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.in.rays.n, tn);
  const uint32_t lds  = 4u * (uint32_t)scene.n_tori * kCrossingSlotBytes;
  return launch_default_solver(scene, [&](auto real, auto ori) {
    hipLaunchKernelGGL((glow_kernel<decltype(real), decltype(ori)::value>), dim3(grid), dim3(256), lds, stream, scene, a);
  });
}

// glow_kernel's columns; the tables are static LDS (2176 B).  The scene travels without its materials (SceneNoMat).
hipError_t launch_glow_profile(const SceneK& scene, const GlowProfileArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.in.rays.n == 0)
    return hipSuccess;
  const uint32_t   grid = stream_grid(a.in.rays.n, tn);
  const uint32_t   lds  = 4u * (uint32_t)scene.n_tori * kCrossingSlotBytes;
  const SceneNoMat sc   = scene_no_mat(scene);
  return launch_default_solver(scene, [&](auto real, auto ori) {
    hipLaunchKernelGGL((glow_profile_kernel<decltype(real), decltype(ori)::value>), dim3(grid), dim3(256), lds, stream, sc, a);
  });
}

// 17 KiB of static LDS for the accumulators beside the scene; no dynamic LDS.
static_assert(sizeof(SceneK) + sizeof(GlowWeightsArgs) <= 4096, "the kernel-argument segment of glow_weights_kernel");
hipError_t launch_glow_weights(const SceneK& scene, const GlowWeightsArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.in.rays.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.in.rays.n, tn);
  return launch_default_solver(scene, [&](auto real, auto ori) {
    hipLaunchKernelGGL((glow_weights_kernel<decltype(real), decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
  });
}

// The block width from n_tori: 96 · n_tori bytes of dynamic LDS per lane beside 2.4 KiB of static LDS (the scene, the
// sigma tables), every block at or below 64 KiB — no function attribute is needed and at least two blocks share a CU.
// 256 lanes up to two tori (48 KiB), 128 up to five (60 KiB), 64 beyond (48 KiB for eight).  TRT_ABSORBED_LANES (64, 128
// or 256, for measurements: tools/bench_weights_absorbed.py) overrides the choice where the block still fits 64 KiB.
uint32_t glow_weights_absorbed_lanes(int n_tori, const Tuning& tn)
{
  const uint32_t pick = n_tori <= 2 ? 256u : n_tori <= 5 ? 128u : 64u, want = tn.absorbed_lanes;
  if((want == 64u || want == 128u || want == 256u) && want * kAbsorbedLaneBytes * (uint32_t)n_tori + 4096u <= 65536u)
    return want;
  return pick;
}
template <class Real, bool ORIENT, uint32_t LANES>
static void launch_absorbed_width(const SceneNoMat& sc, const GlowWeightsAbsorbedArgs& a, uint32_t n_tori, const Tuning& tn, hipStream_t stream)
{
  static_assert(LANES * kAbsorbedLaneBytes * (LANES == 256u ? 2u : LANES == 128u ? 5u : TRT_MAX_TORI) + sizeof(SceneK) + 1024u <= 65536u,
                "a block of glow_weights_absorbed_kernel stays at or below 64 KiB of LDS");
  hipLaunchKernelGGL((glow_weights_absorbed_kernel<Real, ORIENT, LANES>), dim3(stream_grid_lanes(a.in.rays.n, LANES, tn)), dim3(LANES),
                     LANES * kAbsorbedLaneBytes * n_tori, stream, sc, a);
}
hipError_t launch_glow_weights_absorbed(const SceneK& scene, const GlowWeightsAbsorbedArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.in.rays.n == 0)
    return hipSuccess;
  const uint32_t   lanes = glow_weights_absorbed_lanes(scene.n_tori, tn);
  const SceneNoMat sc    = scene_no_mat(scene);
  return launch_default_solver(scene, [&](auto real, auto ori) {
    using Real          = decltype(real);
    constexpr bool kOri = decltype(ori)::value;
    const uint32_t nt   = (uint32_t)scene.n_tori;
    if(lanes == 256u) launch_absorbed_width<Real, kOri, 256u>(sc, a, nt, tn, stream);
    else if(lanes == 128u) launch_absorbed_width<Real, kOri, 128u>(sc, a, nt, tn, stream);
    else launch_absorbed_width<Real, kOri, 64u>(sc, a, nt, tn, stream);
  });
}

// trt_glow_project*: the same blocks and the same grid; the emission tables ride in the arguments beside the scene.
template <class Real, bool ORIENT, uint32_t LANES>
static void launch_project_width(const SceneNoMat& sc, const GlowProfileArgs& a, uint32_t n_tori, const Tuning& tn, hipStream_t stream)
{
  hipLaunchKernelGGL((glow_project_kernel<Real, ORIENT, LANES>), dim3(stream_grid_lanes(a.in.rays.n, LANES, tn)), dim3(LANES),
                     LANES * kAbsorbedLaneBytes * n_tori, stream, sc, a);
}
hipError_t launch_glow_project(const SceneK& scene, const GlowProfileArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.in.rays.n == 0)
    return hipSuccess;
  const uint32_t   lanes = glow_weights_absorbed_lanes(scene.n_tori, tn);
  const SceneNoMat sc    = scene_no_mat(scene);
  return launch_default_solver(scene, [&](auto real, auto ori) {
    using Real          = decltype(real);
    constexpr bool kOri = decltype(ori)::value;
    const uint32_t nt   = (uint32_t)scene.n_tori;
    if(lanes == 256u) launch_project_width<Real, kOri, 256u>(sc, a, nt, tn, stream);
    else if(lanes == 128u) launch_project_width<Real, kOri, 128u>(sc, a, nt, tn, stream);
    else launch_project_width<Real, kOri, 64u>(sc, a, nt, tn, stream);
  });
}

// trt_glow_backproject*: the same blocks on an eighth of the grid — every block leaves a row of partials, so the grid is
// what fills the device (131072 lanes: two blocks of 256 or eight of 64 per CU) and the rows stay at 2048 at the most;
// the blocks go round their rays instead.  glow_backproject_rows is that grid: the host sizes the partials by it.
uint32_t glow_backproject_rows(int n_tori, uint64_t n, const Tuning& tn)
{
  const uint32_t lanes = glow_weights_absorbed_lanes(n_tori, tn);
  const uint64_t want = (n + lanes - 1) / lanes, cap = (uint64_t)(tn.trace_blocks ? tn.trace_blocks : 512u) * (256u / lanes);
  return (uint32_t)(want < cap ? want : cap);
}
template <class Real, bool ORIENT, uint32_t LANES>
static void launch_backproject_width(const SceneNoMat& sc, const GlowBackprojectArgs& a, uint32_t n_tori, hipStream_t stream)
{
  hipLaunchKernelGGL((glow_backproject_kernel<Real, ORIENT, LANES>), dim3(a.rows), dim3(LANES), LANES * kAbsorbedLaneBytes * n_tori, stream, sc, a);
}
hipError_t launch_glow_backproject(const SceneK& scene, const GlowBackprojectArgs& a, const Tuning& tn, hipStream_t stream)
{
  const uint32_t nt = (uint32_t)scene.n_tori, n_out = 4u * TRT_PROFILE_KNOTS * nt;
  if(a.rows != glow_backproject_rows(scene.n_tori, a.in.rays.n, tn))
    return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if(a.rows)
  {
    const uint32_t   lanes = glow_weights_absorbed_lanes(scene.n_tori, tn);
    const SceneNoMat sc    = scene_no_mat(scene);
    e = launch_default_solver(scene, [&](auto real, auto ori) {
      using Real          = decltype(real);
      constexpr bool kOri = decltype(ori)::value;
      if(lanes == 256u) launch_backproject_width<Real, kOri, 256u>(sc, a, nt, stream);
      else if(lanes == 128u) launch_backproject_width<Real, kOri, 128u>(sc, a, nt, stream);
      else launch_backproject_width<Real, kOri, 64u>(sc, a, nt, stream);
    });
  }
  if(e != hipSuccess)
    return e;
  hipLaunchKernelGGL(backproject_sum_kernel, dim3((n_out + 255u) / 256u), dim3(256), 0, stream, a.partials, a.rows, n_out, a.back);
  return hipGetLastError();
}

// trt_glow_tangent*: the store kernel (the direction's tables to a.delta_dev), then glow_profile_kernel's grid and columns.
hipError_t launch_glow_tangent(const SceneK& scene, const GlowTangentArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.in.rays.n == 0)
    return hipSuccess;
  ProfileTables t;
  std::memcpy(t.p, a.delta, sizeof t.p);
  hipLaunchKernelGGL(store_tables_kernel, dim3((uint32_t)(sizeof t / 4u + 255u) / 256u), dim3(256), 0, stream, t, a.delta_dev);
  if(const hipError_t e = hipGetLastError(); e != hipSuccess)
    return e;
  GlowProfileArgs p;
  p.in    = a.in;
  p.sub   = a.sub;
  p.prof  = a.prof;
  p.rgba  = a.rgba;
  p.stats = a.stats;
  const uint32_t     grid  = stream_grid(a.in.rays.n, tn);
  const uint32_t     lds   = 4u * (uint32_t)scene.n_tori * kCrossingSlotBytes;
  const SceneNoMat   sc    = scene_no_mat(scene);
  const float* const delta = a.delta_dev;
  return launch_default_solver(scene, [&](auto real, auto ori) {
    hipLaunchKernelGGL((glow_tangent_kernel<decltype(real), decltype(ori)::value>), dim3(grid), dim3(256), lds, stream, sc, p, delta);
  });
}

// trt_glow_adjoint*: launch_glow_backproject as it stands for channels 0..2 (its column sums land in slot 3 and its walk
// is not counted: the statistics are one walk's), then the sigma kernel on the same grid and its sum, which overwrites slot 3.
template <class Real, bool ORIENT, uint32_t LANES>
static void launch_sigma_adjoint_width(const SceneNoMat& sc, const GlowSigmaAdjointArgs& a, uint32_t rows, uint32_t n_tori, hipStream_t stream)
{
  static_assert(LANES * kAbsorbedLaneBytes * (LANES == 256u ? 2u : LANES == 128u ? 5u : TRT_MAX_TORI) + sizeof(SceneK) +
                        sizeof(float4) * TRT_MAX_TORI * TRT_PROFILE_KNOTS + 64u <= 65536u,
                "a block of glow_sigma_adjoint_kernel stays at or below 64 KiB of LDS");
  hipLaunchKernelGGL((glow_sigma_adjoint_kernel<Real, ORIENT, LANES>), dim3(rows), dim3(LANES), LANES * kAbsorbedLaneBytes * n_tori, stream, sc, a);
}
hipError_t launch_glow_adjoint(const SceneK& scene, const GlowAdjointArgs& a, const Tuning& tn, hipStream_t stream)
{
  const uint32_t      nt = (uint32_t)scene.n_tori;
  GlowBackprojectArgs w;
  w.in  = a.in;
  w.sub = a.sub;
  std::memset(w.sigma, 0, sizeof w.sigma);
  for(uint32_t j = 0; j < nt; ++j)
    for(uint32_t k = 0; k < TRT_PROFILE_KNOTS; ++k)
      w.sigma[j][k] = a.prof.p[j].knot[k][3];
  std::memcpy(w.inv_r2, a.prof.inv_r2, sizeof w.inv_r2);
  w.y        = a.y;
  w.partials = a.partials_w;
  w.rows     = a.rows;
  w.back     = a.grad;
  w.stats    = nullptr;
  if(const hipError_t e = launch_glow_backproject(scene, w, tn, stream); e != hipSuccess)
    return e;
  if(a.rows)
  {
    GlowSigmaAdjointArgs g;
    g.in       = a.in;
    g.sub      = a.sub;
    g.prof     = a.prof;
    g.y        = a.y;
    g.partials = a.partials_g;
    g.stats    = a.stats;
    const uint32_t   lanes = glow_weights_absorbed_lanes(scene.n_tori, tn);
    const SceneNoMat sc    = scene_no_mat(scene);
    const hipError_t e     = launch_default_solver(scene, [&](auto real, auto ori) {
      using Real          = decltype(real);
      constexpr bool kOri = decltype(ori)::value;
      if(lanes == 256u) launch_sigma_adjoint_width<Real, kOri, 256u>(sc, g, a.rows, nt, stream);
      else if(lanes == 128u) launch_sigma_adjoint_width<Real, kOri, 128u>(sc, g, a.rows, nt, stream);
      else launch_sigma_adjoint_width<Real, kOri, 64u>(sc, g, a.rows, nt, stream);
    });
    if(e != hipSuccess)
      return e;
  }
  const uint32_t n_acc = TRT_PROFILE_KNOTS * nt;
  hipLaunchKernelGGL(adjoint_sum_kernel, dim3((n_acc + 255u) / 256u), dim3(256), 0, stream, a.partials_g, a.rows, n_acc, a.grad);
  return hipGetLastError();
}

}  // namespace trt
