// trt_rays.hip — the ray-stream kernels of the toroidal ray tracer (trt_trace*, trt_occluded*, trt_crossings*, trt_shade*,
// trt_camera_rays*, trt_shade_camera*), gfx950.
//
//   trace_kernel       trace(rays_in → hits_out): SoA rays in, closest hit out.
//   occluded_kernel    occluded(rays_in → bits_out): SoA rays in, any hit out as a bit mask and / or flag bytes.
//   crossings_kernel   crossings(rays_in → slots_out): SoA rays in, every surface crossing out, in order, slot-major.
//   ShadePlain         shade(rays_in → colours_out): SoA rays in, bounce_loop()'s colour out, samples averaged — the plain form
//                      of the shade family, whose two kernels (shade_kernel, shade_camera_kernel) are in trt_render.hpp.
//   camera_rays_kernel   camera(frame → rays_out): the two cameras' rays with sub-pixel offsets, SoA and sample-major, out.
//   launch_trace, launch_occluded, launch_crossings, launch_shade, launch_camera_rays, launch_shade_camera
//                        their grid and launch wrappers; launch_shade and launch_shade_camera (the supersampled frame:
//                        shade_kernel with the rays made in registers by the camera) are the two shared launches with ShadePlain.
//   zero_words_kernel, launch_zero_words         zeroes the query counters of a counted launch.
//
// One lane = one ray; the scene is staged into LDS once per block.  Compiled with -ffp-contract=off (see trt_device.hpp
// for the arithmetic contract); each kernel is instantiated for the FP32 and the FP64 root solve.
#include "trt_render.hpp"

namespace trt {

// ------------------------------------------------------------------------------------------
// trace(rays_in → hits_out)
// ------------------------------------------------------------------------------------------
template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void trace_kernel(const SceneK scene, const TraceArgs a)
{
  __shared__ SceneK S;
  stage_scene<ORIENT>(&S, scene);

  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.rays.n; i += stride)
  {
    const v3 o = {a.rays.ox[i], a.rays.oy[i], a.rays.oz[i]};
    const v3 d = {a.rays.dx[i], a.rays.dy[i], a.rays.dz[i]};
    float     t;
    const int id = closest_hit<Real, ALT, kWalkTable, ORIENT>(S, o, d, a.tmin, a.tmax, t, tests, wc);   // incoherent rays: trt_device.hpp
    v3 P = {0.0f, 0.0f, 0.0f}, N = {0.0f, 0.0f, 0.0f};
    if(id >= 0)
    {
      P = {fma_(t, d.x, o.x), fma_(t, d.y, o.y), fma_(t, d.z, o.z)};
      N = torus_normal<ORIENT>(S, id, P);
    }
    if(a.hits.t) a.hits.t[i] = t;
    if(a.hits.px) a.hits.px[i] = P.x;
    if(a.hits.py) a.hits.py[i] = P.y;
    if(a.hits.pz) a.hits.pz[i] = P.z;
    if(a.hits.nx) a.hits.nx[i] = N.x;
    if(a.hits.ny) a.hits.ny[i] = N.y;
    if(a.hits.nz) a.hits.nz[i] = N.z;
    if(a.hits.id) a.hits.id[i] = id;
  }
  if(a.stats)
    block_add_stats(a.stats, tests, 0u, 0u, wc);
}

// ------------------------------------------------------------------------------------------
// occluded(rays_in → one bit per ray): the any-hit query
// ------------------------------------------------------------------------------------------
// A wave owns the 64 consecutive rays from a multiple of 64 on, so its mask word is one __ballot.  The grid-stride loop
// therefore runs on the WAVE's base index (a scalar: every lane of the wave makes the same trips and meets the ballot
// with the whole wave converged); the lanes at or beyond n load nothing and vote 0, which also zeroes the unused high
// bits of the last word.  A ray whose window is empty — !(tmax_i > tmin), a NaN bound included — executes no test.
template <class Real, bool ALT, bool ORIENT = false, int WALK = kOccludedWalk>
__global__ __launch_bounds__(256) void occluded_kernel(const SceneK scene, const OccludedArgs a)
{
  __shared__ SceneK S;
  stage_scene<ORIENT>(&S, scene);

  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint32_t lane   = threadIdx.x & 63u;
  const uint32_t wave   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for(uint64_t base = (uint64_t)blockIdx.x * 256u + wave * 64u; base < a.rays.n; base += stride)
  {
    const uint64_t i   = base + lane;
    bool           hit = false;
    if(i < a.rays.n)
    {
      const float tmax = a.tmax_per_ray ? a.tmax_per_ray[i] : a.tmax;
      if(tmax > a.tmin)
      {
        const v3 o = {a.rays.ox[i], a.rays.oy[i], a.rays.oz[i]};
        const v3 d = {a.rays.dx[i], a.rays.dy[i], a.rays.dz[i]};
        hit = any_hit<Real, ALT, ORIENT, WALK>(S, o, d, a.tmin, tmax, tests, wc);
      }
      if(a.flag) a.flag[i] = hit ? 1 : 0;
    }
    const unsigned long long word = __ballot(hit);
    if(a.mask && lane == 0u) a.mask[base >> 6] = word;
  }
  if(a.stats)
    block_add_stats(a.stats, 0u, 0u, tests, wc);
}

// ------------------------------------------------------------------------------------------
// crossings(rays_in → every surface crossing, in order)
// ------------------------------------------------------------------------------------------
// A lane enumerates its ray's crossings torus by torus (S.order, every torus over the full window: torus_crossings) and
// inserts each into a sorted column of its own in LDS — slot k of lane `tid` at [k * 256 + tid], so a wave's access to
// one slot is 64 consecutive words, and no indexed private array exists that could go to scratch
// memory.  The column is dynamic shared memory sized by max_per_ray: 5 B per slot and lane (t, then a byte id << 1 |
// entering), 1.25 KiB per slot and block — K = 4 keeps the block at 7 KiB with the scene, K = 32 at 42 KiB (3 blocks per
// CU).  Insertion is stable: a crossing goes behind every kept one with t <= its own, which is the tie rule (torus
// tested first, then earlier root); once the column is full only a crossing strictly below the last kept one gets in,
// so the kept slots are the first slots of the untruncated answer.  Nobody but the lane reads its column: the only
// barrier is stage_scene's, the only atomics the stats block add.  Stores are slot-major: one instruction, 64
// consecutive elements of slot k.  The window test !(tmax > tmin) is kernel-uniform.
// (kCrossingSlotBytes, column_insert: trt_render.hpp — shade_through_kernel fills the same column)
template <class Real, bool ORIENT = false>
__global__ __launch_bounds__(256) void crossings_kernel(const SceneK scene, const CrossingsArgs a)
{
  __shared__ SceneK S;
  extern __shared__ float crossing_lds[];   // [K][256] t, then [K][256] bytes
  stage_scene<ORIENT>(&S, scene);

  const uint32_t K   = a.max_per_ray;
  float*         ct  = crossing_lds + threadIdx.x;
  uint8_t*       cw  = reinterpret_cast<uint8_t*>(crossing_lds + K * 256u) + threadIdx.x;
  const bool     window = a.tmax > a.tmin;
  const float    inf = __builtin_inff();

  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.rays.n; i += stride)
  {
    uint32_t count = 0;
    if(window)
    {
      const v3 o = {a.rays.ox[i], a.rays.oy[i], a.rays.oz[i]};
      const v3 d = {a.rays.dx[i], a.rays.dy[i], a.rays.dz[i]};
      RayK<Real> r;
      r.set(o, d, a.tmin, a.tmax);
      for(int k = 0; k < S.n_tori; ++k)
      {
        const int j = S.order[k];
        ++tests;
        torus_crossings<Real, ORIENT>(S, j, r, wc, [&](float t, bool entering) { column_insert(ct, cw, K, count, t, j, entering); });
      }
    }
    const uint32_t kept = umin(count, K);
    for(uint32_t k = 0; k < K; ++k)
    {
      const bool     used = k < kept;
      const uint64_t at   = (uint64_t)k * a.rays.n + i;
      const uint32_t w    = used ? cw[k * 256u] : 0u;
      if(a.out.t) a.out.t[at] = used ? ct[k * 256u] : inf;
      if(a.out.id) a.out.id[at] = used ? (int32_t)(w >> 1) : -1;
      if(a.out.entering) a.out.entering[at] = (uint8_t)(w & 1u);
    }
    if(a.out.count) a.out.count[i] = count;
  }
  if(a.stats)
    block_add_stats(a.stats, tests, 0u, 0u, wc);
}

// ------------------------------------------------------------------------------------------
// shade(rays_in → one colour per output): the payload loop on caller-supplied rays
// ------------------------------------------------------------------------------------------
// The plain form of the shade family (trt_render.hpp has the two kernels, the walks and the colour of a caller's ray):
// no table, nothing staged, the render's own hit step.
struct ShadePlain {
  using Table  = void;
  using Staged = NotStaged;
  template <class Args> static __device__ __forceinline__ void stage(Staged*, const Args&) {}
  template <class Real, bool ALT, bool ORIENT, class Args>
  static __device__ __forceinline__ PcLightHit<Real, ALT, ORIENT> hit(const Args&, const Staged&) { return {}; }
};

// ------------------------------------------------------------------------------------------
// camera rays: the cameras of the render as ray streams, and shade_kernel fed by them
// ------------------------------------------------------------------------------------------
// Pixel i of the band → column x and image row y (camera_rays_kernel).  Linear rows, the simplest mapping: lane k of a
// wave is pixel base + k, so every stream store is contiguous over the wave.
// One division per pixel — by 32-bit arithmetic as long as the band has fewer than 2^32 pixels (kernel-uniform).
__device__ __forceinline__ void camera_pixel(const CameraArgs& c, uint64_t i, uint32_t& x, uint32_t& y)
{
  if(c.n_px <= 0xffffffffull)
  {
    const uint32_t i32 = (uint32_t)i, ly = i32 / c.W;
    x = i32 - ly * c.W;
    y = c.row_begin + ly;
  }
  else
  {
    const uint64_t ly = i / c.W;
    x = (uint32_t)(i - ly * c.W);
    y = c.row_begin + (uint32_t)ly;
  }
}
// One lane per (sample, pixel): blockIdx.y is the sample — block-uniform, so its offsets and table pointers are scalar
// loads from the kernel arguments and the pinhole origin is computed from scalars alone — blockIdx.x and the grid-stride
// loop run over the pixels of the band.  No loads but the four table entries of the toroidal camera (W + H floats per
// sample: cache-resident), 24 B of stores per ray, each stream 256 B contiguous per wave.
__global__ __launch_bounds__(256) void camera_rays_kernel(const CameraRaysArgs a)
{
  const CameraArgs& c = a.cam;
  const uint32_t s  = blockIdx.y;
  const ToroCam  tc = camera_sample(c, s);
  const float    jx = c.jx[s], jy = c.jy[s];
  const gptr<float> ox = (gptr<float>)a.out.ox, oy = (gptr<float>)a.out.oy, oz = (gptr<float>)a.out.oz;
  const gptr<float> dx = (gptr<float>)a.out.dx, dy = (gptr<float>)a.out.dy, dz = (gptr<float>)a.out.dz;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.n_px; i += stride)
  {
    uint32_t x, y;
    camera_pixel(c, i, x, y);
    v3 o, d;
    raygen_offset(c.g, tc, c.W, c.H, c.camera, x, y, jx, jy, o, d);
    const uint64_t r = (uint64_t)s * c.n_px + i;
    if(ox) ox[r] = o.x;
    if(oy) oy[r] = o.y;
    if(oz) oz[r] = o.z;
    if(dx) dx[r] = d.x;
    if(dy) dy[r] = d.y;
    if(dz) dz[r] = d.z;
  }
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
// (stream_grid and camera_grid, the grids of these kernels: trt_kernels.hpp)
hipError_t launch_trace(const SceneK& scene, const TraceArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.rays.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.rays.n, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    hipLaunchKernelGGL((trace_kernel<decltype(real), decltype(alt)::value, decltype(ori)::value>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

hipError_t launch_occluded(const SceneK& scene, const OccludedArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.rays.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.rays.n, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    using Real = decltype(real);
    constexpr bool ALT = decltype(alt)::value, ORIENT = decltype(ori)::value;
#ifdef TRT_TUNING   // TRT_OCCLUDED_WALK: the other form of the walk (bit-identical; tools/bench_occluded.py times both)
    if constexpr(!ALT)
      if(tn.occluded_walk != kOccludedWalk)
      {
        hipLaunchKernelGGL((occluded_kernel<Real, ALT, ORIENT, kOccludedWalk == kWalkTable ? kWalkNested : kWalkTable>), dim3(grid), dim3(256), 0, stream, scene, a);
        return hipGetLastError();
      }
#endif
    hipLaunchKernelGGL((occluded_kernel<Real, ALT, ORIENT>), dim3(grid), dim3(256), 0, stream, scene, a);
    return hipGetLastError();
  });
}

// Default solver only (the enumeration is the walk's: trt_api.hip refuses the others before it gets here).
hipError_t launch_crossings(const SceneK& scene, const CrossingsArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.rays.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.rays.n, tn);
  const uint32_t lds  = a.max_per_ray * kCrossingSlotBytes;
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    if constexpr(decltype(alt)::value)
      return hipErrorInvalidValue;
    else
    {
      hipLaunchKernelGGL((crossings_kernel<decltype(real), decltype(ori)::value>), dim3(grid), dim3(256), lds, stream, scene, a);
      return hipGetLastError();
    }
  });
}

// The plain form of the two shade launches (trt_render.hpp).
hipError_t launch_shade(const SceneK& scene, const ShadeArgs& a, const Tuning& tn, hipStream_t stream) { return launch_stream_form<ShadePlain>(scene, a, tn, stream); }
hipError_t launch_shade_camera(const SceneK& scene, const ShadeCameraArgs& a, const Tuning& tn, hipStream_t stream) { return launch_camera_form<ShadePlain>(scene, a, tn, stream); }

// One block per 256 pixels of the band (at most 4096: grid-stride) times one grid row per sample; no scene, no solver.
hipError_t launch_camera_rays(const CameraRaysArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.cam.n_px == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.cam.n_px, tn);
  hipLaunchKernelGGL(camera_rays_kernel, dim3(grid, a.cam.samples), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// Zeroes up to 64 words (the query counters of a counted launch) with a one-wave kernel: a kernel
// node when the stream is being captured — the *_dev entry points put no memset node into a graph
// (32 memset nodes between 64 kernel nodes faulted on replay under ROCm 7.2).
__global__ void zero_words_kernel(unsigned int* q, uint32_t n)
{
  for(uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) q[i] = 0u;
}

hipError_t launch_zero_words(unsigned int* words, uint32_t n, hipStream_t stream)
{
  if(n <= 64u) hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(64), 0, stream, words, n);
  else hipLaunchKernelGGL(zero_words_kernel, dim3((n + 1023u) / 1024u < 64u ? (n + 1023u) / 1024u : 64u), dim3(1024), 0, stream, words, n);
  return hipGetLastError();
}

}  // namespace trt
