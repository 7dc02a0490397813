// trt_glass.hip — glass tori: refraction along caller and camera rays (trt_shade_refract*, trt_shade_refract_camera*), gfx950.
//
//   GlassHit       the render's hit step with what bounce_loop() asks at every hit answered: is this torus a dielectric, and
//                  if so the refracted (or totally reflected) successor ray and the filtered attenuation
//   ShadeRefract   the form: shade_kernel / shade_camera_kernel (trt_render.hpp) with Glass staged into LDS and GlassHit
//   launch_shade_refract, launch_shade_refract_camera   the two shared launches with that form.
//
// The loop is the render's (bounce_loop, trt_render.hpp): only the closest hit of a segment is needed, so every solver
// and the oriented tori apply — instantiated for <float | double> × ALT × ORIENT like the plain form.  The dielectrics come
// in the kernel arguments (Glass, trt_kernels.hpp), indexed by torus id; SceneK knows nothing of them.
// F32 and F64 are separate instantiations, as everywhere: the FP64 solve needs about twice the VGPRs of the FP32 one, and
// a kernel that held both would run the FP32 scenes at the FP64 kernel's occupancy.
// Compiled with -ffp-contract=off like every unit: each operation below is one FP32 rounding, in the order written.
#include "trt_hits.hpp"

namespace trt {

// The render's hit step with the dielectric (glass_step, trt_hits.hpp) as the glass() of bounce_loop().
template <class Real, bool ALT, bool ORIENT>
struct GlassHit : PcLightHit<Real, ALT, ORIENT> {
  const Glass& g;
  __device__ __forceinline__ explicit GlassHit(const Glass& glass) : g(glass) {}
  __device__ __forceinline__ bool glass(int id, const HitState& h, v3 d, v3& attenuation, int& done, v3& nextO, v3& nextD) const
  {
    return glass_step(g, id, h, d, attenuation, done, nextO, nextD);
  }
};

// ------------------------------------------------------------------------------------------
// shade_refract(rays_in → one colour per output), shade_refract_camera(camera → the band of an image)
// ------------------------------------------------------------------------------------------
// The form: the 41 words of Glass staged into LDS, the render's hit step with the dielectric asked after it.
struct ShadeRefract {
  using Table  = Glass;
  using Staged = Glass;
  template <class Args> static __device__ __forceinline__ void stage(Staged* G, const Args& a) { stage_words(G, a.table); }
  template <class Real, bool ALT, bool ORIENT, class Args>
  static __device__ __forceinline__ GlassHit<Real, ALT, ORIENT> hit(const Args&, const Staged& G) { return GlassHit<Real, ALT, ORIENT>{G}; }
};

hipError_t launch_shade_refract(const SceneK& scene, const ShadeRefractArgs& a, const Tuning& tn, hipStream_t stream) { return launch_stream_form<ShadeRefract>(scene, a, tn, stream); }
hipError_t launch_shade_refract_camera(const SceneK& scene, const ShadeRefractCameraArgs& a, const Tuning& tn, hipStream_t stream) { return launch_camera_form<ShadeRefract>(scene, a, tn, stream); }

}  // namespace trt
