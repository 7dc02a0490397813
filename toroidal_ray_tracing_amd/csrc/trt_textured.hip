// trt_textured.hip — textures on tori along caller and camera rays (trt_shade_textured*, trt_shade_textured_camera*), and the
// (u, v) of surface points (trt_hit_uv*), gfx950.
//
//   texture_fetch                 the bilinear texel of one hit: four 4-byte loads, repeat addressing in integers
//   textured_loop                 bounce_loop (trt_render.hpp) with the texel multiplied into the hit's diffuse term between
//                                 hit_begin and the shadow query, where REFL/shaders/raytrace.rchit:101-106 has it
//   shade_textured_kernel         shade_kernel (trt_rays.hip) with textured_loop
//   shade_textured_camera_kernel  shade_camera_kernel (trt_rays.hip) with textured_loop
//   hit_uv_kernel                 torus_uv (trt_device.hpp) on a stream of points
//   launch_shade_textured, launch_shade_textured_camera, launch_hit_uv   their grid and launch wrappers.
//
// The first kernels of the shade family that read memory inside the hit.  The descriptor table (Textures, trt_kernels.hpp)
// comes in the kernel arguments and is indexed by the material of the hit, which differs from lane to lane: it is staged into
// LDS beside the scene (indexed by a VGPR in the argument segment it would go to the stack), and so is the 1-KB sRGB decode
// table of the ctx — only when some bound texture is sRGB.  No hardware sampler: its filter weights are fixed-point and
// unspecified, and the contract here is one FP32 rounding per written operation (include/trt.h states them).
// Compiled with -ffp-contract=off like every unit: each operation below is one FP32 rounding, in the order written.
#include "trt_render.hpp"

namespace trt {

// SceneK and the larger of the two argument structs travel in one kernel-argument segment.
static_assert(sizeof(SceneK) + sizeof(ShadeTexturedCameraArgs) <= 4096 && sizeof(SceneK) + sizeof(ShadeTexturedArgs) <= 4096,
              "the kernel-argument segment of the shade_textured kernels");
static_assert(sizeof(trt_texture) == 32, "trt_texture: include/trt.h");

// ------------------------------------------------------------------------------------------
// the texel of one hit (include/trt.h states the rule operation for operation)
// ------------------------------------------------------------------------------------------
// `i` reduced into [0, n) for ANY i: the remainder in integers, after the conversion — no u, v or repeat addresses outside
// the image.
__device__ __forceinline__ int wrap_texel(int i, int n)
{
  const int r = i % n;
  return r < 0 ? r + n : r;
}
// One channel of an RGBA8 texel (byte `k` of the little-endian word): through the decode table, or scaled.
__device__ __forceinline__ float texel_channel(uint32_t t, uint32_t k, bool srgb, const float* lut)
{
  const uint32_t c = (t >> (8u * k)) & 255u;
  return srgb ? lut[c] : (float)c * (1.0f / 255.0f);
}
__device__ __forceinline__ float lerp_(float a, float b, float f) { return fma_(f, b - a, a); }

// Bilinear, repeat addressing, texel centres at (i + 0.5) / W; `lut` is the sRGB decode table in LDS.
__device__ __forceinline__ v3 texture_fetch(const TextureK& T, const float* lut, float u, float v)
{
  const int   W = (int)T.W, H = (int)T.H;
  const float x = (u * T.ru) * (float)W - 0.5f, y = (v * T.rv) * (float)H - 0.5f;
  const float xf = floorf(x), yf = floorf(y);
  const float fx = x - xf, fy = y - yf;
  const int   i0 = wrap_texel((int)xf, W), j0 = wrap_texel((int)yf, H);
  const int   i1 = i0 + 1 == W ? 0 : i0 + 1, j1 = j0 + 1 == H ? 0 : j0 + 1;
  const gptr<const uint32_t> img = (gptr<const uint32_t>)(const void*)T.texels;
  const size_t   r0 = (size_t)j0 * (size_t)W, r1 = (size_t)j1 * (size_t)W;
  const uint32_t t00 = img[r0 + i0], t10 = img[r0 + i1], t01 = img[r1 + i0], t11 = img[r1 + i1];
  const bool     srgb = T.srgb != 0;
  float c[3];
#pragma unroll
  for(uint32_t k = 0; k < 3; ++k)
  {
    const float top = lerp_(texel_channel(t00, k, srgb, lut), texel_channel(t10, k, srgb, lut), fx);
    const float bot = lerp_(texel_channel(t01, k, srgb, lut), texel_channel(t11, k, srgb, lut), fx);
    c[k] = lerp_(top, bot, fy);
  }
  return {c[0], c[1], c[2]};
}

// ------------------------------------------------------------------------------------------
// the payload loop of one ray with textures
// ------------------------------------------------------------------------------------------
// bounce_loop() (trt_render.hpp) as shade_ray() runs it — the raygen loop rgen:54-87, the miss shader, the light of pc, the
// opaque shadow query, the mirror, the enclosure mask that starts empty and grows at a hit from outside when `grow` — with
// one step more between hit_begin and the shadow query: diffuse *= texel (rchit:101-106) for a material that names a
// texture.  A material without one runs trt_shade's arithmetic, so its colours are trt_shade's bit for bit; so does a
// texture whose every texel decodes to 1.  The texel is fetched BEFORE the solve of the shadow ray: nothing of it but the
// three products is live across it.
template <class Real, bool ALT, bool ORIENT>
__device__ __forceinline__ v3 textured_loop(const SceneK& S, const trt_push& pc, const Textures& tx, const float* lut, v3 origin, v3 direction,
                                            bool grow, uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc)
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
      hit_begin<ORIENT>(S, pc, id, t, origin, direction, h);
      const int k = tx.of_mat[h.matId];
      if(k >= 0)                                                           // rchit:101
      {
        float u, v;
        torus_uv<ORIENT>(S, id, h.P, u, v);
        const v3 texel = texture_fetch(tx.t[k], lut, u, v);
        h.diffuse = {h.diffuse.x * texel.x, h.diffuse.y * texel.y, h.diffuse.z * texel.z};   // rchit:105
        // The products are pinned HERE: nothing reads them before hit_end, so hipcc is free to sink the filter — four texel
        // words and two weights instead of three floats — below the shadow ray's solve.
        asm volatile("" : "+v"(h.diffuse.x), "+v"(h.diffuse.y), "+v"(h.diffuse.z));
      }
      bool shadowed = false;
      const uint32_t inside = S.inside[id];
      if(h.wantShadow)   // (N·L > 0: the shadow ray leaves the surface outwards)
        shadowed = any_hit<Real, ALT, ORIENT>(S, h.P, h.L, kTMin, h.lightDistance, n_shadow, wc, skip | inside);  // rchit:114-131
      if(grow && dot3(h.N, direction) < 0.0f)   // hit from outside: reflect(D, N) leaves outwards
        skip |= inside;
      prdHit = hit_end(S, h, direction, shadowed, attenuation, done, nextO, nextD);
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

// The descriptor table and, when a bound texture is sRGB, the decode table into LDS: one dword per thread of the
// 256-thread block each.  No barrier: the caller's stage_scene, which follows, has one and publishes everything.
__device__ __forceinline__ void stage_textures(Textures* tx, float* lut, const Textures& arg)
{
  static_assert(sizeof(float) * 256 == 1024, "one decode entry per thread of a 256-thread block");
  stage_words(tx, arg);
  if(arg.any_srgb)
    lut[threadIdx.x] = ((gptr<const float>)arg.decode)[threadIdx.x];
}

// ------------------------------------------------------------------------------------------
// shade_textured(rays_in → one colour per output), shade_textured_camera(camera → the band of an image)
// ------------------------------------------------------------------------------------------
// shade_kernel and shade_camera_kernel (trt_rays.hip) with textured_loop: the two walks of trt_render.hpp, so the camera
// form's image is, bit for bit, camera_rays_kernel's rays put through shade_textured_kernel.  LDS: the scene, the
// descriptors, the decode table and, in the camera form, the camera.
template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_textured_kernel(const SceneK scene, const ShadeTexturedArgs a)
{
  __shared__ SceneK   S;
  __shared__ Textures tx;
  __shared__ float    lut[256];
  stage_textures(&tx, lut, a.tex);
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes all three)

  shade_stream_walk(a.rays, a.n_out, a.samples, a.rgba, a.stats, [&](v3 o, v3 d, uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc) {
    return textured_loop<Real, ALT, ORIENT>(S, a.pc, tx, lut, o, d, dot3(d, d) <= kCullUnitDD, n_primary, n_bounce, n_shadow, wc);
  });
}

template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void shade_textured_camera_kernel(const SceneK scene, const ShadeTexturedCameraArgs a)
{
  __shared__ SceneK     S;
  __shared__ CameraArgs cam;
  __shared__ Textures   tx;
  __shared__ float      lut[256];
  stage_words(&cam, a.cam);
  stage_textures(&tx, lut, a.tex);
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes all four)

  shade_camera_walk(cam, a.rgba, a.stats, [&](v3 o, v3 d, uint32_t& n_primary, uint32_t& n_bounce, uint32_t& n_shadow, WorkCount& wc) {
    return textured_loop<Real, ALT, ORIENT>(S, a.pc, tx, lut, o, d, dot3(d, d) <= kCullUnitDD, n_primary, n_bounce, n_shadow, wc);
  });
}

// ------------------------------------------------------------------------------------------
// hit_uv(points → (u, v))
// ------------------------------------------------------------------------------------------
// A plain stream kernel: one lane per point, grid-stride.  The id comes from device memory and is never trusted as an
// index: outside [0, n_tori) — a miss record, or anything else — the point gets u = v = 0.
template <bool ORIENT>
__global__ __launch_bounds__(256) void hit_uv_kernel(const SceneK scene, const HitUvArgs a)
{
  __shared__ SceneK S;
  stage_scene<ORIENT>(&S, scene);

  const gptr<const float>   px = (gptr<const float>)a.px, py = (gptr<const float>)a.py, pz = (gptr<const float>)a.pz;
  const gptr<const int32_t> ids = (gptr<const int32_t>)a.id;
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for(uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < a.n; i += stride)
  {
    const int id = ids[i];
    float u = 0.0f, v = 0.0f;
    if(id >= 0 && id < S.n_tori)
      torus_uv<ORIENT>(S, id, v3{px[i], py[i], pz[i]}, u, v);
    if(a.u) st1(a.u, i, u);
    if(a.v) st1(a.v, i, v);
  }
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
// One lane per output (a.n_out = a.rays.n / a.samples); every solver, like launch_shade.
hipError_t launch_shade_textured(const SceneK& scene, const ShadeTexturedArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.n_out == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.n_out, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((shade_textured_kernel<decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

// One wave per 8×8 tile of the band, four to a block; every solver, like launch_shade_camera.
hipError_t launch_shade_textured_camera(const SceneK& scene, const ShadeTexturedCameraArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.cam.n_px == 0)
    return hipSuccess;
  const uint32_t grid = camera_grid(a.cam, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((shade_textured_camera_kernel<decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

// One lane per point; no solver runs.
hipError_t launch_hit_uv(const SceneK& scene, const HitUvArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.n, tn);
  return with_orient(scene, [&](auto ori) {
    hipLaunchKernelGGL((hit_uv_kernel<decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

}  // namespace trt
