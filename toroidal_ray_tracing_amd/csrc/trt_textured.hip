// trt_textured.hip — textures on tori along caller and camera rays (trt_shade_textured*, trt_shade_textured_camera*), and the
// (u, v) of surface points (trt_hit_uv*), gfx950.
//
//   texture_fetch, with_texel     (trt_hits.hpp) the bilinear texel of one hit: four 4-byte loads, repeat addressing in integers
//   TexturedHit                   the render's hit step with the texel multiplied into the hit's diffuse term between
//                                 hit_begin and the shadow query (the tint() of bounce_loop, trt_render.hpp), where
//                                 REFL/shaders/raytrace.rchit:101-106 has it
//   ShadeTextured                 the form: shade_kernel / shade_camera_kernel (trt_render.hpp) with the tables staged into
//                                 LDS and TexturedHit
//   hit_uv_kernel                 torus_uv (trt_device.hpp) on a stream of points
//   launch_shade_textured, launch_shade_textured_camera   the two shared launches with that form;  launch_hit_uv.
//
// The first kernels of the shade family that read memory inside the hit.  The descriptor table (Textures, trt_kernels.hpp)
// comes in the kernel arguments and is indexed by the material of the hit, which differs from lane to lane: it is staged into
// LDS beside the scene (indexed by a VGPR in the argument segment it would go to the stack), and so is the 1-KB sRGB decode
// table of the ctx — only when some bound texture is sRGB.  No hardware sampler: its filter weights are fixed-point and
// unspecified, and the contract here is one FP32 rounding per written operation (include/trt.h states them).
// Compiled with -ffp-contract=off like every unit: each operation below is one FP32 rounding, in the order written.
#include "trt_hits.hpp"

namespace trt {

// SceneK and the larger of the two argument structs travel in one kernel-argument segment.
static_assert(sizeof(SceneK) + sizeof(ShadeTexturedCameraArgs) <= 4096 && sizeof(SceneK) + sizeof(ShadeTexturedArgs) <= 4096,
              "the kernel-argument segment of the shade_textured kernels");

// ------------------------------------------------------------------------------------------
// shade_textured(rays_in → one colour per output), shade_textured_camera(camera → the band of an image)
// ------------------------------------------------------------------------------------------
// The hit step with textures: the render's (PcLightHit, trt_render.hpp — the light of pc, the opaque shadow query, the
// mirror) with one step more between hit_begin and the shadow query, the loop's tint(): diffuse *= texel (rchit:101-106)
// for a material that names a texture.  A material without one runs trt_shade's arithmetic, so its colours are trt_shade's
// bit for bit; so does a texture whose every texel decodes to 1.  The texel is fetched BEFORE the solve of the shadow ray:
// nothing of it but the three products is live across it.
template <class Real, bool ALT, bool ORIENT>
struct TexturedHit : PcLightHit<Real, ALT, ORIENT> {
  const TexturesLds& T;
  __device__ __forceinline__ explicit TexturedHit(const TexturesLds& t) : T(t) {}
  __device__ __forceinline__ void tint(const SceneK& S, int id, HitState& h) const
  {
    with_texel<ORIENT>(S, T, id, h, [&](v3 texel) {
      h.diffuse = {h.diffuse.x * texel.x, h.diffuse.y * texel.y, h.diffuse.z * texel.z};   // rchit:105
      // The products are pinned HERE: nothing reads them before hit_end, so hipcc is free to sink the filter — four texel
      // words and two weights instead of three floats — below the shadow ray's solve.
      asm volatile("" : "+v"(h.diffuse.x), "+v"(h.diffuse.y), "+v"(h.diffuse.z));
    });
  }
};

// The form: the descriptor table and, when a bound texture is sRGB, the decode table into LDS — one dword per thread of
// the 256-thread block each — and TexturedHit on them.
struct ShadeTextured {
  using Table  = Textures;
  using Staged = TexturesLds;
  template <class Args> static __device__ __forceinline__ void stage(Staged* T, const Args& a)
  {
    stage_textures(T, a.table);
  }
  template <class Real, bool ALT, bool ORIENT, class Args>
  static __device__ __forceinline__ TexturedHit<Real, ALT, ORIENT> hit(const Args&, const Staged& T) { return TexturedHit<Real, ALT, ORIENT>{T}; }
};

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
// The textured form of the two shade launches (trt_render.hpp).
hipError_t launch_shade_textured(const SceneK& scene, const ShadeTexturedArgs& a, const Tuning& tn, hipStream_t stream) { return launch_stream_form<ShadeTextured>(scene, a, tn, stream); }
hipError_t launch_shade_textured_camera(const SceneK& scene, const ShadeTexturedCameraArgs& a, const Tuning& tn, hipStream_t stream) { return launch_camera_form<ShadeTextured>(scene, a, tn, stream); }

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
