// trt_rays.hip — the ray-stream kernels of the toroidal ray tracer (trt_trace*, trt_occluded*), gfx950.
//
//   trace_kernel       trace(rays_in → hits_out): SoA rays in, closest hit out.
//   occluded_kernel    occluded(rays_in → bits_out): SoA rays in, any hit out as a bit mask and / or flag bytes.
//   stream_grid, launch_trace, launch_occluded   their grid and launch wrappers.
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
// launch wrappers
// ------------------------------------------------------------------------------------------
namespace {
// The grid of the ray-stream kernels (trace_kernel, occluded_kernel; grid-stride loops): one block per 256 rays, at
// most 4096 blocks (TRT_TRACE_BLOCKS).
uint32_t stream_grid(uint64_t n, const Tuning& tn)
{
  const uint64_t want = (n + 255) / 256, cap = tn.trace_blocks ? tn.trace_blocks : 256u * 16u;
  return (uint32_t)(want < cap ? want : cap);
}
}  // namespace

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
