// trt_cloud.hip — gfx950 (MI355X / CDNA4) capture → point cloud (trt_cloud_dev): the step between the toroidal capture
// (RenderedData, 64 B per pixel) and its re-projection (Point, 32 B), which the reference takes through text files
// (BEF writeRenderedPosition / writeColorImage → SEC loadPoints + createCloudDataBuffer, SEC/hello_vulkan.cpp:496-660).
//
//   cloud_plan_kernel      one block: where the call's first point goes (0, or counts_dev[0]: append), the two count words,
//                          and — COMPACT — the chunk counts turned into their exclusive prefix.
//   cloud_stream_kernel    KEEP_ALL / MARK_MISSES: one record per lane and trip, the first 32 B of the 64-B record in as
//                          two dwordx4, one 32-B point out.
//   cloud_count_kernel     COMPACT, pass 1: kept records per chunk → table[chunk] (position half of the record only).
//   cloud_scatter_kernel   COMPACT, pass 2: rank inside the chunk (ballot + mbcnt per wave, LDS over the waves and the
//                          lane's trips), base from the table, kept points out in record order.
//
// No block waits for another one: the passes are separate launches and the kernel boundary orders them.  Nothing is
// written at or beyond `capacity`.  No arithmetic: a record's bits are copied, except the rules of include/trt.h
// (NaN → -FLT_MAX, .w = 0, a marked miss).
#include "trt_cloud.hpp"

#include <cfloat>

namespace trt {

namespace {

template <class T> using gptr = __attribute__((address_space(1))) T*;
typedef float f4v __attribute__((ext_vector_type(4)));

// The capture is read once by the pass that turns it into points and the cloud is written once: non-temporal, like the
// constant fills of the render path (st4c, trt_render.hpp) — the re-projection that follows reads the cloud from HBM
// whatever the policy (268 MB at 4096×2048), and the lines would only displace what the neighbouring passes keep.
// The count pass reads with the default policy: the scatter pass wants the same lines next.
__device__ __forceinline__ f4v  ld4(const float* p) { return *(gptr<const f4v>)p; }
__device__ __forceinline__ f4v  ld4s(const float* p) { return __builtin_nontemporal_load((gptr<const f4v>)p); }
__device__ __forceinline__ void st4s(float* p, f4v v) { __builtin_nontemporal_store(v, (gptr<f4v>)p); }

// The miss rule: what BEF/shaders/raytrace.rmiss:21 leaves in pos.xyz (-0 counts; a NaN never compares equal).
__device__ __forceinline__ bool  is_miss(f4v pos) { return pos.x == 0.0f && pos.y == 0.0f && pos.z == 0.0f; }
// loadPoints' "-nan → lowest()", for either sign of NaN; any other value keeps its bits (a select, no arithmetic)
__device__ __forceinline__ float no_nan(float v) { return v != v ? -FLT_MAX : v; }

__device__ __forceinline__ void store_point(trt_point* out, uint64_t at, f4v pos, f4v col, bool mark)
{
  const bool miss = mark && is_miss(pos);
  f4v p = {no_nan(pos.x), no_nan(pos.y), no_nan(pos.z), 0.0f};            // vec4(…, 0), SEC :646-647
  if(miss) p = f4v{-FLT_MAX, -FLT_MAX, -FLT_MAX, 0.0f};                   // outside every clip volume: the splat drops it
  st4s(out[at].pos, p);
  st4s(out[at].color, f4v{no_nan(col.x), no_nan(col.y), no_nan(col.z), 0.0f});
}

// Record k of lane `threadIdx.x` in the chunk of block `blockIdx.x`: consecutive lanes, consecutive records.
__device__ __forceinline__ uint64_t chunk_record(uint32_t k)
{
  return (uint64_t)blockIdx.x * kCloudChunk + k * kCloudThreads + threadIdx.x;
}

__global__ __launch_bounds__(kCloudThreads) void cloud_stream_kernel(const trt_rendered_data* __restrict__ in, uint64_t n,
                                                                     trt_point* __restrict__ out, uint64_t capacity,
                                                                     const uint64_t* __restrict__ header, int mark)
{
  const uint64_t start = header[kCloudStart];
  const uint64_t room  = capacity > start ? capacity - start : 0;
  f4v pos[kCloudPerLane], col[kCloudPerLane];
  // the trips' loads issued together: one 16-B load in flight per lane leaves a streaming pass bound by latency (post_kernel)
#pragma unroll
  for(uint32_t k = 0; k < kCloudPerLane; ++k)
  {
    const uint64_t i = chunk_record(k);
    if(i < n)
    {
      pos[k] = ld4s(in[i].pos);
      col[k] = ld4s(in[i].color);
    }
  }
#pragma unroll
  for(uint32_t k = 0; k < kCloudPerLane; ++k)
  {
    const uint64_t i = chunk_record(k);
    if(i < n && i < room) store_point(out, start + i, pos[k], col[k], mark != 0);
  }
}

__global__ __launch_bounds__(kCloudThreads) void cloud_count_kernel(const trt_rendered_data* __restrict__ in, uint64_t n,
                                                                    uint32_t* __restrict__ table)
{
  __shared__ uint32_t wave_cnt[kCloudThreads / 64];
  f4v pos[kCloudPerLane];
#pragma unroll
  for(uint32_t k = 0; k < kCloudPerLane; ++k)
  {
    const uint64_t i = chunk_record(k);
    if(i < n) pos[k] = ld4(in[i].pos);
  }
  uint32_t kept = 0;   // of the wave, over its trips
#pragma unroll
  for(uint32_t k = 0; k < kCloudPerLane; ++k)
    kept += (uint32_t)__popcll(__ballot(chunk_record(k) < n && !is_miss(pos[k])));
  if((threadIdx.x & 63u) == 0) wave_cnt[threadIdx.x >> 6] = kept;
  __syncthreads();
  if(threadIdx.x == 0)
  {
    uint32_t sum = 0;
    for(uint32_t w = 0; w < kCloudThreads / 64; ++w) sum += wave_cnt[w];
    table[blockIdx.x] = sum;
  }
}

// One block.  COMPACT: table[c] (kept records of chunk c) becomes the kept records of the chunks before c, a tile of
// kPlanThreads words per trip with the running total carried in a register; the total is what the call wants to add.
// The other modes want every record.  Then thread 0 fixes the call's first point and publishes the two count words — the
// kernels behind this one read `header`, never `counts`, so nothing races with the publication.
constexpr uint32_t kPlanThreads = 1024;
__global__ __launch_bounds__(kPlanThreads) void cloud_plan_kernel(uint64_t n_records, uint32_t n_chunks, int compact, int append,
                                                                  uint64_t capacity, uint64_t* __restrict__ counts,
                                                                  uint64_t* __restrict__ header, uint32_t* __restrict__ table)
{
  __shared__ uint32_t wave_sum[kPlanThreads / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t carry = 0;   // kept records of the tiles before this one (block-uniform; < 2^32 as n_records is)
  for(uint32_t base = 0; compact && base < n_chunks; base += kPlanThreads)
  {
    const uint32_t c = base + threadIdx.x;
    const uint32_t v = c < n_chunks ? table[c] : 0u;
    uint32_t incl = v;   // inclusive scan over the wave
#pragma unroll
    for(uint32_t d = 1; d < 64; d <<= 1)
    {
      const uint32_t up = __shfl_up(incl, d, 64);
      if(lane >= d) incl += up;
    }
    if(lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, tile = 0;
    for(uint32_t w = 0; w < kPlanThreads / 64; ++w)
    {
      const uint32_t s = wave_sum[w];
      if(w < wave) before += s;
      tile += s;
    }
    if(c < n_chunks) table[c] = carry + before + incl - v;
    carry += tile;
    __syncthreads();   // wave_sum is written again by the next trip
  }
  if(threadIdx.x == 0)
  {
    const uint64_t wanted = compact ? (uint64_t)carry : n_records;
    const uint64_t start  = append ? counts[0] : 0, wanted_before = append ? counts[1] : 0;
    header[kCloudStart] = start;
    const uint64_t end = start + wanted;
    counts[0] = end < capacity ? end : capacity;
    counts[1] = wanted_before + wanted;
  }
}

__global__ __launch_bounds__(kCloudThreads) void cloud_scatter_kernel(const trt_rendered_data* __restrict__ in, uint64_t n,
                                                                      trt_point* __restrict__ out, uint64_t capacity,
                                                                      const uint64_t* __restrict__ header,
                                                                      const uint32_t* __restrict__ table)
{
  constexpr uint32_t kWaves = kCloudThreads / 64;
  __shared__ uint32_t wave_cnt[kCloudPerLane][kWaves];
  const uint32_t wave = threadIdx.x >> 6;
  f4v pos[kCloudPerLane], col[kCloudPerLane];
#pragma unroll
  for(uint32_t k = 0; k < kCloudPerLane; ++k)
  {
    const uint64_t i = chunk_record(k);
    if(i < n)
    {
      pos[k] = ld4s(in[i].pos);
      col[k] = ld4s(in[i].color);
    }
  }
  // first point of the chunk: the call's first point + the kept records of the chunks before (cloud_plan_kernel)
  const uint64_t first = header[kCloudStart] + table[blockIdx.x];
  bool     keep[kCloudPerLane];
  uint32_t rank[kCloudPerLane];   // kept records of the same wave and trip on lower lanes
#pragma unroll
  for(uint32_t k = 0; k < kCloudPerLane; ++k)
  {
    keep[k] = chunk_record(k) < n && !is_miss(pos[k]);
    const unsigned long long b = __ballot(keep[k]);
    rank[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if((threadIdx.x & 63u) == 0) wave_cnt[k][wave] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  // record order inside the chunk is (trip, wave, lane): a running sum over the kCloudPerLane × kWaves counts in that order
  uint32_t run = 0;
#pragma unroll
  for(uint32_t k = 0; k < kCloudPerLane; ++k)
  {
    uint32_t mine = 0;
#pragma unroll
    for(uint32_t w = 0; w < kWaves; ++w)
    {
      if(w == wave) mine = run;
      run += wave_cnt[k][w];
    }
    const uint64_t at = first + mine + rank[k];
    if(keep[k] && at < capacity) store_point(out, at, pos[k], col[k], false);
  }
}

}  // namespace

hipError_t launch_cloud(const CloudArgs& a, hipStream_t stream)
{
  const bool     compact  = a.mode == TRT_CLOUD_COMPACT;
  const uint32_t n_chunks = (uint32_t)cloud_chunks(a.n_records);   // one block per chunk: many short blocks (launch_post)
  if(compact && n_chunks)
  {
    hipLaunchKernelGGL(cloud_count_kernel, dim3(n_chunks), dim3(kCloudThreads), 0, stream, a.rendered, a.n_records, a.table);
    if(hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(cloud_plan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, a.n_records, n_chunks, compact ? 1 : 0,
                     a.append ? 1 : 0, a.capacity, a.counts, a.header, a.table);
  if(hipError_t e = hipGetLastError()) return e;
  if(n_chunks == 0) return hipSuccess;
  if(compact)
    hipLaunchKernelGGL(cloud_scatter_kernel, dim3(n_chunks), dim3(kCloudThreads), 0, stream, a.rendered, a.n_records, a.points,
                       a.capacity, a.header, a.table);
  else
    hipLaunchKernelGGL(cloud_stream_kernel, dim3(n_chunks), dim3(kCloudThreads), 0, stream, a.rendered, a.n_records, a.points,
                       a.capacity, a.header, a.mode == TRT_CLOUD_MARK_MISSES ? 1 : 0);
  return hipGetLastError();
}

}  // namespace trt
