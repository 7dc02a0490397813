// trt_lights.hip — several lights and area lights along caller and camera rays (trt_shade_lit*, trt_shade_lit_camera*), gfx950.
//
//   lit_hit, LitHit          (trt_hits.hpp) the colour of one hit under the light table: per light the light half of hit_begin,
//                            the shadow stage — one any-hit ray, or K towards a disc about the light — and the colour half of
//                            hit_end; the hit step of bounce_loop (trt_render.hpp) with hit_point / lit_hit / hit_mirror in
//                            the place of hit_begin / the shadow query / hit_end
//   ShadeLit                 the form: shade_kernel / shade_camera_kernel (trt_render.hpp) with LitHit, nothing staged
//   launch_shade_lit, launch_shade_lit_camera   the two shared launches with that form.
//
// Only the closest hit of a segment and any-hit queries are needed, so every solver and the oriented tori apply —
// instantiated for <float | double> × ALT × ORIENT like the plain form.  The lights come in the kernel arguments (Lights,
// trt_kernels.hpp) and stay there: the loops over lights and samples have kernel-uniform trip counts and indices, so every
// table read is a scalar load from the argument segment, as in fan_occluded_kernel.  SceneK and trt_push know nothing of them.
// Compiled with -ffp-contract=off like every unit: each operation below is one FP32 rounding, in the order written.
#include "trt_hits.hpp"

namespace trt {

// SceneK and the larger of the two argument structs travel in one kernel-argument segment.
static_assert(sizeof(SceneK) + sizeof(ShadeLitCameraArgs) <= 4096 && sizeof(SceneK) + sizeof(ShadeLitArgs) <= 4096,
              "the kernel-argument segment of the shade_lit kernels: lower TRT_MAX_LIGHT_SAMPLES rather than move the tables");

// ------------------------------------------------------------------------------------------
// shade_lit(rays_in → one colour per output), shade_lit_camera(camera → the band of an image)
// ------------------------------------------------------------------------------------------
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
