// trt_lights.hip — several lights and area lights along caller and camera rays (trt_shade_lit*, trt_shade_lit_camera*), gfx950.
//
//   lit_hit                  the colour of one hit under the light table: per light the light half of hit_begin, the shadow
//                            stage — one any-hit ray, or K towards a disc about the light — and the colour half of hit_end
//   lit_loop                 bounce_loop (trt_render.hpp) with lit_hit in the place of hit_begin / the shadow query / hit_end
//   shade_lit_kernel         shade_kernel (trt_rays.hip) with lit_loop
//   shade_lit_camera_kernel  shade_camera_kernel (trt_rays.hip) with lit_loop
//   launch_shade_lit, launch_shade_lit_camera   their grid and launch wrappers.
//
// Only the closest hit of a segment and any-hit queries are needed, so every solver and the oriented tori apply —
// instantiated for <float | double> × ALT × ORIENT like shade_kernel.  The lights come in the kernel arguments (Lights,
// trt_kernels.hpp) and stay there: the loops over lights and samples have kernel-uniform trip counts and indices, so every
// table read is a scalar load from the argument segment, as in fan_occluded_kernel.  SceneK and trt_push know nothing of them.
// Compiled with -ffp-contract=off like every unit: each operation below is one FP32 rounding, in the order written.
#include "trt_render.hpp"

namespace trt {

// SceneK and the larger of the two argument structs travel in one kernel-argument segment.
static_assert(sizeof(SceneK) + sizeof(ShadeLitCameraArgs) <= 4096 && sizeof(SceneK) + sizeof(ShadeLitArgs) <= 4096,
              "the kernel-argument segment of the shade_lit kernels: lower TRT_MAX_LIGHT_SAMPLES rather than move the tables");
static_assert(sizeof(trt_light) == 36, "trt_light: include/trt.h");

// ------------------------------------------------------------------------------------------
// the colour of one hit under the light table (include/trt.h states the rule operation for operation)
// ------------------------------------------------------------------------------------------
// prd of rchit:155, summed over the lights.  The shadow stage is ONE any-hit call site inside a flat loop over (light,
// sample): a light of radius 0 is the one ray (P, L) over (kTMin, dist), an area light K rays towards the disc of its
// radius about its centre, in the plane across L; lanes whose N·L <= 0 are predicated off, and no sample ends the loop
// early — v is a count.  `skip` is the path's enclosure mask, `inside` the tubes inside the torus hit: a ray that leaves the
// surface outwards cannot hit those first (bounce_loop has the argument); a sample below the horizon enters the tube.
template <class Real, bool ALT, bool ORIENT>
__device__ __forceinline__ v3 lit_hit(const SceneK& S, const Lights& lt, const HitState& h, v3 d, uint32_t skip, uint32_t inside,
                                      uint32_t& n_shadow, WorkCount& wc)
{
  const MaterialK& mat = S.mat[h.matId];
  v3 prd = {0.0f, 0.0f, 0.0f};
  for(uint32_t l = 0; l < lt.n; ++l)
  {
    const trt_light& q  = lt.l[l];
    const v3         lp = {q.position[0], q.position[1], q.position[2]};
    v3    L;
    float dist = 100000.0f, I = q.intensity;                                 // rchit:79-80
    if(q.type == 0)                                                          // rchit:82
    {
      const v3 lDir = sub3(lp, h.P);
      dist = sqrt_(dot3(lDir, lDir));
      I    = q.intensity / (dist * dist);
      L    = scale3(lDir, 1.0f / dist);
    }
    else
      L = normalize3(lp);                                                    // rchit:91 (lDir = L)
    const bool     want = dot3(h.N, L) > 0.0f;                               // rchit:112
    const bool     area = q.radius > 0.0f;
    const uint32_t rays = area ? lt.K : 1u;
    uint32_t       occ  = 0;
    for(uint32_t s = 0; s < rays; ++s)
    {
      v3       Ls   = L;
      float    tmax = dist;
      uint32_t mask = skip | inside;
      if(area)
      {
        // The basis and lDir are formed again for every sample, from an opaque copy of L: the same bits, a dozen operations
        // beside a query of hundreds — hoisted out of the loop they are nine more VGPRs live across the solve.
        v3 Lo = L;
        asm volatile("" : "+v"(Lo.x), "+v"(Lo.y), "+v"(Lo.z));
        const FanBasis tb = fan_basis(Lo);
        const v3       lD = q.type == 0 ? sub3(lp, h.P) : Lo;
        const float a = q.radius * lt.u[s], b = q.radius * lt.v[s];
        const v3    e = {lD.x + ((a * tb.T.x) + (b * tb.B.x)), lD.y + ((a * tb.T.y) + (b * tb.B.y)), lD.z + ((a * tb.T.z) + (b * tb.B.z))};
        const float len = sqrt_(dot3(e, e));
        Ls   = scale3(e, 1.0f / len);
        tmax = q.type == 0 ? len : 100000.0f;
        if(!(dot3(h.N, Ls) > 0.0f))
          mask = skip;
      }
      if(want && any_hit<Real, ALT, ORIENT>(S, h.P, Ls, kTMin, tmax, n_shadow, wc, mask))   // rchit:114-131
        ++occ;
    }
    const float v    = (float)(rays - occ) / (float)rays;                    // 1 for a lane without a shadow ray
    const float att  = fma_(0.3f, 1.0f - v, v);                              // rchit:135
    v3          spec = {0.0f, 0.0f, 0.0f};
    if(v > 0.0f && want)
      spec = scale3(compute_specular(mat, d, L, h.N), v);                    // rchit:140
    const v3    diffuse = compute_diffuse(mat, L, h.N);                      // rchit:100
    const float kl = att * I;                                                // rchit:155
    const v3    c  = {kl * (diffuse.x + spec.x), kl * (diffuse.y + spec.y), kl * (diffuse.z + spec.z)};
    if(l == 0u)
      prd = {c.x * q.color[0], c.y * q.color[1], c.z * q.color[2]};
    else
      prd = {fma_(c.x, q.color[0], prd.x), fma_(c.y, q.color[1], prd.y), fma_(c.z, q.color[2], prd.z)};
  }
  return prd;
}

// ------------------------------------------------------------------------------------------
// the payload loop of one ray under the light table
// ------------------------------------------------------------------------------------------
// bounce_loop() (trt_render.hpp) — the raygen loop rgen:54-87, the miss shader, the enclosure mask that starts
// empty and grows at a hit from outside when `grow`, the mirror step (hit_mirror: stated once, there) — with the light of
// pc replaced by the table: hit_point, lit_hit, hit_mirror where bounce_loop has hit_begin, any_hit, hit_end.
template <class Real, bool ALT, bool ORIENT>
__device__ __forceinline__ v3 lit_loop(const SceneK& S, const trt_push& pc, const Lights& lt, v3 origin, v3 direction, bool grow,
                                       uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc)
{
  int      depth = 0, done = 1;                                            // rgen:54,57
  uint32_t skip = 0u;
  v3       attenuation = {1.0f, 1.0f, 1.0f};                               // rgen:56
  v3       hitValue = {0.0f, 0.0f, 0.0f};                                  // rgen:61
  for(;;)                                                                  // rgen:62
  {
    v3    prdHit, nextO = origin, nextD = direction;
    float t;
    const int id = closest_hit<Real, ALT, kRenderWalk, ORIENT>(S, origin, direction, kTMin, kTMax, t, depth == 0 ? n_primary : n_bounce, wc, skip);
    if(id < 0)
      prdHit = miss_colour(pc);                                            // rmiss:37
    else
    {
      HitState h;
      hit_point<ORIENT>(S, id, t, origin, direction, h);
      const uint32_t inside = S.inside[id];
      prdHit = lit_hit<Real, ALT, ORIENT>(S, lt, h, direction, skip, inside, n_shadow, wc);
      if(grow && dot3(h.N, direction) < 0.0f)   // hit from outside: reflect(D, N) leaves outwards
        skip |= inside;
      hit_mirror(S.mat[h.matId], h, direction, attenuation, done, nextO, nextD);
    }
    hitValue.x = fma_(prdHit.x, attenuation.x, hitValue.x);                // rgen:76
    hitValue.y = fma_(prdHit.y, attenuation.y, hitValue.y);
    hitValue.z = fma_(prdHit.z, attenuation.z, hitValue.z);
    depth++;                                                               // rgen:78
    if(done == 1 || depth >= pc.maxDepth)                                  // rgen:79
      break;
    origin    = nextO;                                                     // rgen:82
    direction = nextD;                                                     // rgen:83
    done      = 1;                                                         // rgen:84
  }
  return hitValue;
}

// ------------------------------------------------------------------------------------------
// shade_lit(rays_in → one colour per output), shade_lit_camera(camera → the band of an image)
// ------------------------------------------------------------------------------------------
// shade_kernel and shade_camera_kernel (trt_rays.hip) with lit_loop: the two walks of trt_render.hpp, so the camera form's
// image is, bit for bit, camera_rays_kernel's rays put through shade_lit_kernel.  LDS: the scene and, in the camera form,
// the camera.
template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_lit_kernel(const SceneK scene, const ShadeLitArgs a)
{
  __shared__ SceneK S;
  stage_scene<ORIENT>(&S, scene);

  shade_stream_walk(a.rays, a.n_out, a.samples, a.rgba, a.stats, [&](v3 o, v3 d, uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc) {
    return lit_loop<Real, ALT, ORIENT>(S, a.pc, a.lights, o, d, dot3(d, d) <= kCullUnitDD, n_primary, n_bounce, n_shadow, wc);
  });
}

template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_lit_camera_kernel(const SceneK scene, const ShadeLitCameraArgs a)
{
  __shared__ SceneK     S;
  __shared__ CameraArgs cam;
  stage_words(&cam, a.cam);
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes both)

  shade_camera_walk(cam, a.rgba, a.stats, [&](v3 o, v3 d, uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc) {
    return lit_loop<Real, ALT, ORIENT>(S, a.pc, a.lights, o, d, dot3(d, d) <= kCullUnitDD, n_primary, n_bounce, n_shadow, wc);
  });
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
// One lane per output (a.n_out = a.rays.n / a.samples); every solver, like launch_shade.
hipError_t launch_shade_lit(const SceneK& scene, const ShadeLitArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.n_out == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.n_out, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((shade_lit_kernel<decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

// One wave per 8×8 tile of the band, four to a block; every solver, like launch_shade_camera.
hipError_t launch_shade_lit_camera(const SceneK& scene, const ShadeLitCameraArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.cam.n_px == 0)
    return hipSuccess;
  const uint32_t grid = camera_grid(a.cam, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((shade_lit_camera_kernel<decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

}  // namespace trt
