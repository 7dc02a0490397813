// trt_lights.hip — several lights and area lights along caller and camera rays (trt_shade_lit*, trt_shade_lit_camera*), gfx950.
//
//   lit_hit                  the colour of one hit under the light table: per light the light half of hit_begin, the shadow
//                            stage — one any-hit ray, or K towards a disc about the light — and the colour half of hit_end
//   LitHit                   the hit step of bounce_loop (trt_render.hpp) with hit_point / lit_hit / hit_mirror in the place of
//                            hit_begin / the shadow query / hit_end
//   ShadeLit                 the form: shade_kernel / shade_camera_kernel (trt_render.hpp) with LitHit, nothing staged
//   launch_shade_lit, launch_shade_lit_camera   the two shared launches with that form.
//
// Only the closest hit of a segment and any-hit queries are needed, so every solver and the oriented tori apply —
// instantiated for <float | double> × ALT × ORIENT like the plain form.  The lights come in the kernel arguments (Lights,
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
// shade_lit(rays_in → one colour per output), shade_lit_camera(camera → the band of an image)
// ------------------------------------------------------------------------------------------
// The hit step under the light table: the light of pc replaced by the table — hit_point, lit_hit, hit_mirror where
// PcLightHit (trt_render.hpp) has hit_begin, any_hit, hit_end; the mirror step is stated once, there.
template <class Real, bool ALT, bool ORIENT>
struct LitHit : PcLightHit<Real, ALT, ORIENT> {
  const Lights& lt;
  __device__ __forceinline__ explicit LitHit(const Lights& lights) : lt(lights) {}
  __device__ __forceinline__ void begin(const SceneK& S, const trt_push&, int id, float t, v3 o, v3 d, HitState& h) const
  {
    hit_point<ORIENT>(S, id, t, o, d, h);
  }
  __device__ __forceinline__ v3 light(const SceneK& S, const HitState& h, v3 d, uint32_t skip, uint32_t inside, uint32_t& n_shadow, WorkCount& wc) const
  {
    return lit_hit<Real, ALT, ORIENT>(S, lt, h, d, skip, inside, n_shadow, wc);
  }
  __device__ __forceinline__ v3 end(const SceneK& S, const HitState& h, v3 d, v3 prd, v3& attenuation, int& done, v3& nextO, v3& nextD) const
  {
    hit_mirror(S.mat[h.matId], h, d, attenuation, done, nextO, nextD);
    return prd;
  }
};

// The form: nothing staged — the table stays in the argument segment (above) — and LitHit on it.
struct ShadeLit {
  using Table  = Lights;
  using Staged = NotStaged;
  template <class Args> static __device__ __forceinline__ void stage(Staged*, const Args&) {}
  template <class Real, bool ALT, bool ORIENT, class Args>
  static __device__ __forceinline__ LitHit<Real, ALT, ORIENT> hit(const Args& a, const Staged&) { return LitHit<Real, ALT, ORIENT>{a.table}; }
};

hipError_t launch_shade_lit(const SceneK& scene, const ShadeLitArgs& a, const Tuning& tn, hipStream_t stream) { return launch_stream_form<ShadeLit>(scene, a, tn, stream); }
hipError_t launch_shade_lit_camera(const SceneK& scene, const ShadeLitCameraArgs& a, const Tuning& tn, hipStream_t stream) { return launch_camera_form<ShadeLit>(scene, a, tn, stream); }

}  // namespace trt
