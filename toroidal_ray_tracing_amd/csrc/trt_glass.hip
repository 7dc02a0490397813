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

__device__ __forceinline__ void stage_glass(Glass* lds, const Glass& arg)   // no barrier: the caller's stage_scene has one
{
  static_assert(sizeof(Glass) % 4 == 0 && sizeof(Glass) / 4 <= 256, "one dword per thread of a 256-thread block");
  if(threadIdx.x < sizeof(Glass) / 4)
    reinterpret_cast<uint32_t*>(lds)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&arg)[threadIdx.x];
}

// ------------------------------------------------------------------------------------------
// shade_refract(rays_in → one colour per output)
// ------------------------------------------------------------------------------------------
// shade_kernel, line for line: one lane owns one OUTPUT and walks its samples in order — the same layout, the same
// accumulation, the same division.  LDS: the scene and the 41 words of Glass.
template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_refract_kernel(const SceneK scene, const ShadeRefractArgs a)
{
  __shared__ SceneK S;
  __shared__ Glass  G;
  stage_glass(&G, a.glass);
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes both)

  const gptr<const float> ox = (gptr<const float>)a.rays.ox, oy = (gptr<const float>)a.rays.oy, oz = (gptr<const float>)a.rays.oz;
  const gptr<const float> dx = (gptr<const float>)a.rays.dx, dy = (gptr<const float>)a.rays.dy, dz = (gptr<const float>)a.rays.dz;
  const GlassPath glass = {G};
  uint32_t       n_primary = 0, n_bounce = 0, n_shadow = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_out; i += stride)
  {
    v3 acc = {0.0f, 0.0f, 0.0f};
    for(uint32_t s = 0; s < a.samples; ++s)
    {
      const uint64_t r = (uint64_t)s * a.n_out + i;
      const v3 o = {ox[r], oy[r], oz[r]};
      const v3 d = {dx[r], dy[r], dz[r]};
      const v3 c = bounce_loop<Real, ALT, ORIENT>(S, a.pc, o, d, 0u, dot3(d, d) <= kCullUnitDD, {1.0f, 1.0f, 1.0f}, [](float) {}, [](float, const HitState&, int) {},
                                                  n_primary, n_bounce, n_shadow, wc, glass);
      if(s == 0u) acc = c;
      else acc = {acc.x + c.x, acc.y + c.y, acc.z + c.z};
    }
    if(a.samples != 1u)
    {
      const float k = (float)a.samples;
      acc = {acc.x / k, acc.y / k, acc.z / k};
    }
    st4(a.rgba + 4 * i, make_float4(acc.x, acc.y, acc.z, 1.0f));           // rgen:87
  }
  if(a.stats)
    block_add_stats(a.stats, n_primary, n_bounce, n_shadow, wc);
}

// ------------------------------------------------------------------------------------------
// shade_refract_camera(camera → the band of an image)
// ------------------------------------------------------------------------------------------
// shade_camera_kernel, line for line: a wave owns one 8×8 tile of the band, a lane one pixel and its samples; the ray of
// (sample, pixel) is raygen_offset()'s — the image is, bit for bit, camera_rays_kernel's rays put through
// shade_refract_kernel.  LDS: the scene, the camera and Glass.
template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_refract_camera_kernel(const SceneK scene, const ShadeRefractCameraArgs a)
{
  __shared__ SceneK     S;
  __shared__ CameraArgs cam;
  __shared__ Glass      G;
  stage_camera(&cam, a.cam);
  stage_glass(&G, a.glass);
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes all three)

  const CameraArgs& c = cam;
  const GlassPath glass = {G};
  const uint32_t rows = c.row_end - c.row_begin, tiles_x = camera_tiles(c.W);
  const uint64_t n_tiles = (uint64_t)tiles_x * camera_tiles(rows);
  const uint32_t lane = threadIdx.x & 63u, xl = lane % kTile, yl = lane / kTile;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  static_assert(kTile * kTile == 64, "one tile per wave");
  uint32_t       n_primary = 0, n_bounce = 0, n_shadow = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * 4u;
  for(uint64_t t = (uint64_t)blockIdx.x * 4u + wave; t < n_tiles; t += stride)
  {
    uint32_t tx, ty;
    if(n_tiles <= 0xffffffffull)   // (kernel-uniform) one 32-bit division per tile
    {
      ty = (uint32_t)t / tiles_x;
      tx = (uint32_t)t - ty * tiles_x;
    }
    else
    {
      ty = (uint32_t)(t / tiles_x);
      tx = (uint32_t)(t - (uint64_t)ty * tiles_x);
    }
    const uint32_t x = tx * kTile + xl, ly = ty * kTile + yl, y = c.row_begin + ly;
    if(x >= c.W || ly >= rows)
      continue;
    v3 acc = {0.0f, 0.0f, 0.0f};
    for(uint32_t s = 0; s < c.samples; ++s)
    {
      const CameraArgs* cs = &cam;   // read through an opaque pointer, once per sample (shade_camera_kernel has the reason)
      asm volatile("" : "+v"(cs));
      v3 o, d;
      raygen_offset(cs->g, camera_sample(*cs, s), cs->W, cs->H, cs->camera, x, y, cs->jx[s], cs->jy[s], o, d);
      const v3 col = bounce_loop<Real, ALT, ORIENT>(S, a.pc, o, d, 0u, dot3(d, d) <= kCullUnitDD, {1.0f, 1.0f, 1.0f}, [](float) {}, [](float, const HitState&, int) {},
                                                    n_primary, n_bounce, n_shadow, wc, glass);
      if(s == 0u) acc = col;
      else acc = {acc.x + col.x, acc.y + col.y, acc.z + col.z};
    }
    if(c.samples != 1u)
    {
      const float k = (float)c.samples;
      acc = {acc.x / k, acc.y / k, acc.z / k};
    }
    st4(a.rgba + 4 * ((size_t)y * c.W + x), make_float4(acc.x, acc.y, acc.z, 1.0f));   // rgen:87
  }
  if(a.stats)
    block_add_stats(a.stats, n_primary, n_bounce, n_shadow, wc);
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
  const uint64_t n_tiles = (uint64_t)camera_tiles(a.cam.W) * camera_tiles(a.cam.row_end - a.cam.row_begin);
  const uint32_t grid = stream_grid(n_tiles * 64u, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((shade_refract_camera_kernel<decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

}  // namespace trt
