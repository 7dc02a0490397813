// trt_through.hip — translucent surfaces along caller-supplied rays (trt_transmittance*, trt_shade_through*), gfx950.
//
//   transmittance        the soft shadow query of one ray: the product of the pass factors of every wall it crosses
//   transmittance_kernel transmittance(rays_in → T_out): SoA rays in, one float per ray out.
//   through_loop         the payload loop of one ray with front-to-back "over" compositing of its crossings
//   shade_through_kernel shade_through(rays_in → colours_out): shade_stream_walk around through_loop.  A kernel of its own and
//                        not a form of shade_kernel (trt_render.hpp): it has no camera kernel, sizes its dynamic LDS by the
//                        scene and runs with the default solver only — three things a form would have to say for it alone,
//                        and the shared kernel and launch to ask.  It shares the argument template (StreamShade<Opacity>).
//   launch_transmittance, launch_shade_through   their grid and launch wrappers.
//
// The crossings of a segment are trt_crossings' (torus_crossings, trt_device.hpp: every torus in S.order over the full
// window, no enclosure cull), the shading is the render's (hit_begin, compute_specular, miss_colour: trt_render.hpp).
// The opacities come in the kernel arguments (Opacity, trt_kernels.hpp), indexed by torus id; SceneK knows nothing of them.
// Default solver only: instantiated for <float | double> × ORIENT.  Compiled with -ffp-contract=off like every unit.
#include "trt_render.hpp"

namespace trt {

// ------------------------------------------------------------------------------------------
// transmittance(rays_in → one float per ray): the soft any-hit query
// ------------------------------------------------------------------------------------------
// T = 1, then torus by torus in S.order and root by root T = T * p[id]; the query stops after the torus at which T
// becomes 0 — with every p in {0, 1} that is any_hit()'s walk, test for test: (T == 0) == any_hit() and `tests` counts
// the same.  `p` is indexed by torus id, which is wave-uniform here (every lane of a query loop is at the same torus).
// No window check: the callers own it (transmittance_kernel, as occluded_kernel does for any_hit).
template <class Real, bool ORIENT, class Pass>
__device__ __forceinline__ float transmittance(const SceneK& S, const Pass& p, v3 o, v3 d, float tmin, float tmax,
                                               uint32_t& tests, WorkCount& wc)
{
  RayK<Real> r;
  r.set(o, d, tmin, tmax);
  float T = 1.0f;
  for(int k = 0; k < S.n_tori; ++k)
  {
    const int   j  = S.order[k];
    const float pj = p[j];
    ++tests;
    torus_crossings<Real, ORIENT>(S, j, r, wc, [&](float, bool) { T = T * pj; });
    if(T == 0.0f)
      break;
  }
  return T;
}

// One lane per ray, no LDS beyond the scene.  A ray whose window is empty — !(tmax_i > tmin), a NaN bound included —
// executes no test and gets T = 1.
template <class Real, bool ORIENT = false>
__global__ __launch_bounds__(256) void transmittance_kernel(const SceneK scene, const TransmittanceArgs a)
{
  __shared__ SceneK S;
  stage_scene<ORIENT>(&S, scene);

  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.rays.n; i += stride)
  {
    const float tmax = a.tmax_per_ray ? a.tmax_per_ray[i] : a.tmax;
    float       T    = 1.0f;
    if(tmax > a.tmin)
    {
      const v3 o = {a.rays.ox[i], a.rays.oy[i], a.rays.oz[i]};
      const v3 d = {a.rays.dx[i], a.rays.dy[i], a.rays.dz[i]};
      T = transmittance<Real, ORIENT>(S, a.op.p, o, d, a.tmin, tmax, tests, wc);
    }
    a.T[i] = T;
  }
  if(a.stats)
    block_add_stats(a.stats, 0u, 0u, tests, wc);
}

// ------------------------------------------------------------------------------------------
// shade_through(rays_in → one colour per output): the payload loop with translucent walls
// ------------------------------------------------------------------------------------------
// bounce_loop() (trt_render.hpp) with the closest hit of a segment replaced by the segment's whole sorted list of
// crossings — the lane's column in dynamic LDS (column_insert: crossings_kernel's layout, K = 4 · n_tori slots, so nothing
// is ever truncated) — walked front to back.  The path carries the throughput A (the payload's attenuation) and acc (its
// hitValue).  A crossing of opacity a == 0 is skipped unshaded; any other one is shaded as the closest-hit shader shades
// it, with the shadow bit replaced by the transmittance T of the shadow ray, and added with the weight A · a; behind a
// translucent wall (a < 1) the walk goes on with A · p, an opaque one ends the segment as hit_end() ends it: a mirror
// (illum 3) scales A by Ks BEFORE its own colour is added (rchit:149 runs before rgen:76) and starts the next segment at
// (P, reflect(d, N)), anything else ends the path.  A segment that runs out of crossings adds the miss colour.
// With every a in {0, 1} each expression below is bit for bit hit_end()'s and bounce_loop()'s: fma(0.3, 1 - T, T) is 1
// at T = 1 and 0.3f at T = 0, spec · 1, A · 1.
// `oa` / `op`: the opacities and pass factors by torus id, in LDS (the id of a crossing differs from lane to lane).
// The shadow query runs in registers alone; the column is read again only after it.
template <class Real, bool ORIENT>
__device__ __forceinline__ v3 through_loop(const SceneK& S, const trt_push& pc, const float* oa, const float* op,
                                           float* ct, uint8_t* cw, uint32_t K, v3 origin, v3 direction,
                                           uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc)
{
  int depth = 0;
  v3  A   = {1.0f, 1.0f, 1.0f};                                           // rgen:56
  v3  acc = {0.0f, 0.0f, 0.0f};                                           // rgen:61
  for(;;)                                                                  // rgen:62
  {
    uint32_t count = 0;
    {
      RayK<Real> r;
      r.set(origin, direction, kTMin, kTMax);
      uint32_t& tests = depth == 0 ? n_primary : n_bounce;
      for(int k = 0; k < S.n_tori; ++k)
      {
        const int j = S.order[k];
        ++tests;
        torus_crossings<Real, ORIENT>(S, j, r, wc, [&](float t, bool entering) { column_insert(ct, cw, K, count, t, j, entering); });
      }
    }
    const uint32_t kept = umin(count, K);
    bool next = false, ended = false;
    v3   nextO = origin, nextD = direction;
    for(uint32_t k = 0; k < kept; ++k)
    {
      const int   id = (int)(cw[k * 256u] >> 1);
      const float a  = oa[id];
      if(a == 0.0f)
        continue;
      HitState h;
      hit_begin<ORIENT>(S, pc, id, ct[k * 256u], origin, direction, h);
      float T = 1.0f;
      if(h.wantShadow)                                                     // rchit:112-131, a fraction for the bit
        T = transmittance<Real, ORIENT>(S, op, h.P, h.L, kTMin, h.lightDistance, n_shadow, wc);
      const MaterialK& mat = S.mat[h.matId];
      const float att = fma_(0.3f, 1.0f - T, T);                           // rchit:135
      v3 spec = {0.0f, 0.0f, 0.0f};
      if(T > 0.0f && h.wantShadow)
        spec = scale3(compute_specular(mat, direction, h.L, h.N), T);      // rchit:140
      const float kl = att * h.lightIntensity;                             // rchit:155
      const v3    c  = {kl * (h.diffuse.x + spec.x), kl * (h.diffuse.y + spec.y), kl * (h.diffuse.z + spec.z)};
      const bool opaque = !(a < 1.0f);
      const bool mirror = opaque && mat.illum == 3;                        // rchit:145
      if(mirror)
      {
        A.x *= mat.specular[0];
        A.y *= mat.specular[1];
        A.z *= mat.specular[2];
      }
      acc.x = fma_(c.x, A.x * a, acc.x);                                   // rgen:76
      acc.y = fma_(c.y, A.y * a, acc.y);
      acc.z = fma_(c.z, A.z * a, acc.z);
      if(!opaque)
      {
        const float p = op[id];
        A = {A.x * p, A.y * p, A.z * p};
        continue;
      }
      if(mirror)
      {
        next  = true;
        nextO = h.P;
        nextD = reflect3(direction, h.N);
      }
      ended = true;
      break;
    }
    if(!ended)
    {
      const v3 m = miss_colour(pc);                                        // rmiss:37
      acc.x = fma_(m.x, A.x, acc.x);
      acc.y = fma_(m.y, A.y, acc.y);
      acc.z = fma_(m.z, A.z, acc.z);
    }
    depth++;                                                               // rgen:78
    if(!next || depth >= pc.maxDepth)                                      // rgen:79
      break;
    origin    = nextO;                                                     // rgen:82
    direction = nextD;                                                     // rgen:83
  }
  return acc;
}

// shade_stream_walk (trt_render.hpp) around through_loop.  LDS: the scene, 16 opacity words, and
// the block's columns (K · kCrossingSlotBytes).
template <class Real, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_through_kernel(const SceneK scene, const ShadeThroughArgs a)
{
  __shared__ SceneK  S;
  __shared__ Opacity O;
  extern __shared__ float crossing_lds[];   // [K][256] t, then [K][256] bytes
  stage_words(&O, a.table);
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes both)

  const uint32_t K  = 4u * (uint32_t)S.n_tori;
  float*         ct = crossing_lds + threadIdx.x;
  uint8_t*       cw = reinterpret_cast<uint8_t*>(crossing_lds + K * 256u) + threadIdx.x;

  shade_stream_walk(a.rays, a.n_out, a.samples, a.rgba, a.stats, [&](v3 o, v3 d, uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc) {
    return through_loop<Real, ORIENT>(S, a.pc, O.a, O.p, ct, cw, K, o, d, n_primary, n_bounce, n_shadow, wc);
  });
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
// Default solver only (the enumeration is the walk's: trt_api.hip refuses the others before it gets here).
hipError_t launch_transmittance(const SceneK& scene, const TransmittanceArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.rays.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.rays.n, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    if constexpr(decltype(alt)::value)
      return hipErrorInvalidValue;
    else
    {
      hipLaunchKernelGGL((transmittance_kernel<decltype(real), decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
      return hipGetLastError();
    }
  });
}

// One lane per output (a.n_out = a.rays.n / a.samples); 4 · n_tori slots per lane: 5 KiB of columns for one torus, 40 KiB for eight.
hipError_t launch_shade_through(const SceneK& scene, const ShadeThroughArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.n_out == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.n_out, tn);
  const uint32_t lds  = 4u * (uint32_t)scene.n_tori * kCrossingSlotBytes;
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    if constexpr(decltype(alt)::value)
      return hipErrorInvalidValue;
    else
    {
      hipLaunchKernelGGL((shade_through_kernel<decltype(real), decltype(ori)::value>), dim3(grid), dim3(256), lds, stream, scene, a);
      return hipGetLastError();
    }
  });
}

}  // namespace trt
