// trt_glass.hip — glass tori: refraction along caller and camera rays (trt_shade_refract*, trt_shade_refract_camera*), gfx950.
//
//   GlassPath                    what bounce_loop() asks at every hit: is this torus a dielectric, and if so the refracted
//                                (or totally reflected) successor ray and the filtered attenuation
//   shade_refract_kernel         shade_kernel (trt_rays.hip) with GlassPath handed to the loop
//   shade_refract_camera_kernel  shade_camera_kernel (trt_rays.hip) with GlassPath handed to the loop
//   launch_shade_refract, launch_shade_refract_camera   their grid and launch wrappers.
//
// The loop is the render's (bounce_loop, trt_render.hpp): only the closest hit of a segment is needed, so every solver
// and the oriented tori apply — instantiated for <float | double> × ALT × ORIENT like shade_kernel.  The dielectrics come
// in the kernel arguments (Glass, trt_kernels.hpp), indexed by torus id; SceneK knows nothing of them.
// F32 and F64 are separate instantiations, as everywhere: the FP64 solve needs about twice the VGPRs of the FP32 one, and
// a kernel that held both would run the FP32 scenes at the FP64 kernel's occupancy.
// Compiled with -ffp-contract=off like every unit: each operation below is one FP32 rounding, in the order written.
#include "trt_render.hpp"

namespace trt {

// ------------------------------------------------------------------------------------------
// the dielectric: GLSL refract() at a glass hit, stateless
// ------------------------------------------------------------------------------------------
// Called by bounce_loop() after hit_end() — the hit is shaded as any non-mirror hit — and before the fma of rgen:76, as
// the mirror scales the attenuation by Ks before its own colour is added (rchit:149 before rgen:76).  Only the sign of
// N·I decides between entering and leaving: the path carries no "inside" flag, and the far side of a wall is vacuum.
// `g` lives in LDS: the id of a hit differs from lane to lane.
struct GlassPath {
  const Glass& g;
  __device__ __forceinline__ bool hit(int id, const HitState& h, v3 d, v3& attenuation, int& done, v3& nextO, v3& nextD) const
  {
    if(((g.mask >> id) & 1u) == 0u)
      return false;
    const v3    I        = normalize3(d);
    const float c        = dot3(h.N, I);
    const bool  entering = c < 0.0f;
    const v3    Nf       = entering ? h.N : neg3(h.N);
    const float eta      = entering ? g.inv_n[id] : g.n[id];
    const float cosi     = -dot3(Nf, I);
    const float k        = 1.0f - (eta * eta) * (1.0f - cosi * cosi);
    if(k < 0.0f)   // total internal reflection: the attenuation is untouched
      nextD = reflect3(I, Nf);
    else
    {
      const float m = eta * cosi - sqrt_(k);
      nextD = {fma_(m, Nf.x, eta * I.x), fma_(m, Nf.y, eta * I.y), fma_(m, Nf.z, eta * I.z)};
      if(entering)   // the filter, once per passage, on the way in
      {
        attenuation.x *= g.tf[id][0];
        attenuation.y *= g.tf[id][1];
        attenuation.z *= g.tf[id][2];
      }
    }
    nextO = h.P;
    done  = 0;
    return true;
  }
};

// ------------------------------------------------------------------------------------------
// shade_refract(rays_in → one colour per output), shade_refract_camera(camera → the band of an image)
// ------------------------------------------------------------------------------------------
// shade_kernel and shade_camera_kernel (trt_rays.hip) with GlassPath handed to the loop: the two walks of trt_render.hpp,
// so the camera form's image is, bit for bit, camera_rays_kernel's rays put through shade_refract_kernel.
// LDS: the scene, the 41 words of Glass and, in the camera form, the camera.
template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_refract_kernel(const SceneK scene, const ShadeRefractArgs a)
{
  __shared__ SceneK S;
  __shared__ Glass  G;
  stage_words(&G, a.glass);
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes both)

  shade_stream_walk(a.rays, a.n_out, a.samples, a.rgba, a.stats, [&](v3 o, v3 d, uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc) {
    return shade_ray<Real, ALT, ORIENT>(S, a.pc, o, d, n_primary, n_bounce, n_shadow, wc, GlassPath{G});
  });
}

template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_refract_camera_kernel(const SceneK scene, const ShadeRefractCameraArgs a)
{
  __shared__ SceneK     S;
  __shared__ CameraArgs cam;
  __shared__ Glass      G;
  stage_words(&cam, a.cam);
  stage_words(&G, a.glass);
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes all three)

  shade_camera_walk(cam, a.rgba, a.stats, [&](v3 o, v3 d, uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc) {
    return shade_ray<Real, ALT, ORIENT>(S, a.pc, o, d, n_primary, n_bounce, n_shadow, wc, GlassPath{G});
  });
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
// One lane per output (a.n_out = a.rays.n / a.samples); every solver, like launch_shade.
hipError_t launch_shade_refract(const SceneK& scene, const ShadeRefractArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.n_out == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.n_out, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((shade_refract_kernel<decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

// One wave per 8×8 tile of the band, four to a block; every solver, like launch_shade_camera.
hipError_t launch_shade_refract_camera(const SceneK& scene, const ShadeRefractCameraArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.cam.n_px == 0)
    return hipSuccess;
  const uint32_t grid = camera_grid(a.cam, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((shade_refract_camera_kernel<decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

}  // namespace trt
