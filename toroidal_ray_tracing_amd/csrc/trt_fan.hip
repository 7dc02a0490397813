// trt_fan.hip — the ray-fan kernels of the toroidal ray tracer (trt_fan_rays*, trt_fan_occluded*), gfx950.
//
//   fan_dir                     the arithmetic contract of include/trt.h: one sample's direction in Duff et al.'s basis about N (fan_basis, trt_render.hpp).
//   fan_sample_dir              the choice between the table entry and fan_dir, for the two kernels with one lane per point.
//   fan_rays_kernel             fan(points → rays_out): `samples` rays per surface point, SoA and sample-major, out.
//   fan_occluded_kernel         form kFanLane of fan(points → bits, open): one lane owns a point and walks its samples.
//   fan_occluded_block_kernel   form kFanBlock: a block compacts the live points of 256 and deals (point, sample) pairs out.
//   launch_fan_rays, launch_fan_occluded   their launch wrappers (grid: stream_grid, trt_kernels.hpp).
//
// The rays are never stored by the fused kernels: a point is 28 B read (px, py, pz, nx, ny, nz, id), 12 B written.
// Compiled with -ffp-contract=off like every unit here: the products and sums below are the roundings the header lists.
#include "trt_render.hpp"

namespace trt {

// (FanBasis, fan_basis: trt_render.hpp — the area lights of trt_lights.hip build the same basis about L.)
// d.k = ((lx * T.k) + (ly * B.k)) + (lz * N.k)
__device__ __forceinline__ v3 fan_dir(const FanBasis& f, v3 N, float lx, float ly, float lz)
{
  return {((lx * f.T.x) + (ly * f.B.x)) + (lz * N.x), ((lx * f.T.y) + (ly * f.B.y)) + (lz * N.y), ((lx * f.T.z) + (ly * f.B.z)) + (lz * N.z)};
}
// One sample's direction: the table entry as it is (TRT_FAN_WORLD) or about N (`local`).  fan_occluded_block_kernel keeps
// its own text of this choice: it loads N and the basis from LDS inside it, and its machine code moves with the helper.
__device__ __forceinline__ v3 fan_sample_dir(bool local, const FanBasis& f, v3 N, float lx, float ly, float lz)
{
  return local ? fan_dir(f, N, lx, ly, lz) : v3{lx, ly, lz};
}

// A point is dead when the caller gave an id stream and its id is negative (the miss record).
__device__ __forceinline__ bool fan_live(const FanArgs& f, uint64_t i) { return !f.at.id || ((gptr<const int32_t>)f.at.id)[i] >= 0; }
__device__ __forceinline__ v3 fan_point(const FanArgs& f, uint64_t i)
{
  return {((gptr<const float>)f.at.px)[i], ((gptr<const float>)f.at.py)[i], ((gptr<const float>)f.at.pz)[i]};
}
__device__ __forceinline__ v3 fan_normal(const FanArgs& f, uint64_t i)   // TRT_FAN_LOCAL only: the streams may be NULL otherwise
{
  return {((gptr<const float>)f.at.nx)[i], ((gptr<const float>)f.at.ny)[i], ((gptr<const float>)f.at.nz)[i]};
}

// ------------------------------------------------------------------------------------------
// fan(points → rays_out)
// ------------------------------------------------------------------------------------------
// One lane per point: P, N and id loaded once, the basis computed once, then a loop over the samples whose trip count and
// table index are kernel-uniform — the table entries are scalar loads from the kernel arguments — storing 6 x samples
// elements, each store 256 B contiguous per wave (sample s of point i at s * n + i).  A dead point gets o = P, d = 0.
__global__ __launch_bounds__(256) void fan_rays_kernel(const FanRaysArgs a)
{
  const FanArgs& f = a.fan;
  const bool local = f.frame == TRT_FAN_LOCAL;
  const gptr<float> ox = (gptr<float>)a.out.ox, oy = (gptr<float>)a.out.oy, oz = (gptr<float>)a.out.oz;
  const gptr<float> dx = (gptr<float>)a.out.dx, dy = (gptr<float>)a.out.dy, dz = (gptr<float>)a.out.dz;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < f.n; i += stride)
  {
    const bool live = fan_live(f, i);
    const v3   P = fan_point(f, i);
    v3         N = {0.0f, 0.0f, 1.0f};
    if(local && live) N = fan_normal(f, i);
    const FanBasis tb = fan_basis(N);
    for(uint32_t s = 0; s < f.samples; ++s)
    {
      v3 d = fan_sample_dir(local, tb, N, f.lx[s], f.ly[s], f.lz[s]);
      if(!live) d = {0.0f, 0.0f, 0.0f};
      const uint64_t r = (uint64_t)s * f.n + i;
      if(ox) ox[r] = P.x;
      if(oy) oy[r] = P.y;
      if(oz) oz[r] = P.z;
      if(dx) dx[r] = d.x;
      if(dy) dy[r] = d.y;
      if(dz) dz[r] = d.z;
    }
  }
}

// ------------------------------------------------------------------------------------------
// fan(points → bits, open): the fused any-hit query
// ------------------------------------------------------------------------------------------
// What both forms store for a point: its word, and open = (samples − popcount) / samples, one correctly rounded division.
__device__ __forceinline__ void fan_store(const FanOccludedArgs& a, uint64_t i, unsigned long long bits)
{
  if(a.bits) ((gptr<unsigned long long>)a.bits)[i] = bits;
  if(a.open) ((gptr<float>)a.open)[i] = (float)(a.fan.samples - (uint32_t)__popcll(bits)) / (float)a.fan.samples;
}

// Form kFanLane.  One lane owns one point: it loads P, N and id once, computes the basis once and walks the samples with a
// kernel-uniform trip count — the table is read from the kernel arguments by the uniform index (scalar loads, no
// runtime-indexed private array) — setting bits in a 64-bit register; one 8-byte and one 4-byte store per point.  The
// grid-stride loop runs on the WAVE's base index, as occluded_kernel's does, so that the vote "does this wave hold a live
// point" is taken by the whole wave: a wave without one (the CLEAR part of a frame's first-hit record) skips the sample
// loop.  The window test !(tmax > tmin) is kernel-uniform and makes every point dead.  No atomics but the stats add.
template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void fan_occluded_kernel(const SceneK scene, const FanOccludedArgs a)
{
  __shared__ SceneK S;
  stage_scene<ORIENT>(&S, scene);

  const FanArgs& f = a.fan;
  const bool     local  = f.frame == TRT_FAN_LOCAL, window = a.tmax > a.tmin;
  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint32_t lane   = threadIdx.x & 63u;
  const uint32_t wave   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for(uint64_t base = (uint64_t)blockIdx.x * 256u + wave * 64u; base < f.n; base += stride)
  {
    const uint64_t i    = base + lane;
    const bool     live = i < f.n && window && fan_live(f, i);
    unsigned long long bits = 0ull;
    if(__ballot(live) != 0ull)
    {
      v3 P = {0.0f, 0.0f, 0.0f}, N = {0.0f, 0.0f, 1.0f};
      if(live)
      {
        P = fan_point(f, i);
        if(local) N = fan_normal(f, i);
      }
      const FanBasis tb = fan_basis(N);
      for(uint32_t s = 0; s < f.samples; ++s)
      {
        const v3 d = fan_sample_dir(local, tb, N, f.lx[s], f.ly[s], f.lz[s]);
        if(live && any_hit<Real, ALT, ORIENT, kOccludedWalk>(S, P, d, a.tmin, a.tmax, tests, wc))
          bits |= 1ull << s;
      }
    }
    if(i < f.n) fan_store(a, i, bits);
  }
  if(a.stats)
    block_add_stats(a.stats, 0u, 0u, tests, wc);
}

// Form kFanBlock.  On a frame's first-hit record most points are dead, and form kFanLane idles their lanes in every wave a
// silhouette crosses.  Here a block takes 256 points at a time:
//   1. every lane votes "live"; ballot + prefix over the four waves give a live point its slot j < L, and it stages P, N and
//      its basis at slot j of LDS (12 floats) and zeroes the slot's word;
//   2. the L x samples (point, sample) pairs are dealt to the lanes in the order q = s * L + j — neighbouring lanes share the
//      sample and sit on neighbouring points — in trips of 256 whose count is block-uniform; a lane whose ray is occluded
//      ORs its bit into the slot's word (an LDS atomic on the word's half: several lanes own samples of one point);
//   3. after one barrier the lane that owns point i reads the word of its slot and stores bits / open.
// Every barrier is reached by the whole block (the trip counts depend on the block's base and on L alone); lanes at or
// beyond n vote dead, take part in the barriers and store nothing.  The table is staged into LDS beside the scene (the
// sample index of a pair is not uniform).  A ray is the same arithmetic whoever runs it, and its test count does not depend
// on the lane: words, open and stats are those of form kFanLane bit for bit.
// LDS besides the scene: 12 KiB of points, 2 KiB of words, 768 B of table.
template <class Real, bool ALT, bool ORIENT = false>
__global__ __launch_bounds__(256) void fan_occluded_block_kernel(const SceneK scene, const FanOccludedArgs a)
{
  __shared__ SceneK   S;
  __shared__ float    tab[3][TRT_MAX_FAN_SAMPLES];
  __shared__ float    pt[12][256];    // px py pz nx ny nz Tx Ty Tz Bx By Bz, by slot
  __shared__ uint32_t word[256][2];   // low / high half of the slot's bits
  __shared__ uint32_t wave_live[4];
  static_assert(TRT_MAX_FAN_SAMPLES == 64, "a slot's word is two 32-bit halves; the table is staged by 192 threads");
  if(threadIdx.x < 3u * TRT_MAX_FAN_SAMPLES)   // lx, ly, lz lie behind one another in FanArgs: one dword per thread, as stage_camera reads its arguments
    reinterpret_cast<uint32_t*>(&tab[0][0])[threadIdx.x] = reinterpret_cast<const uint32_t*>(&a.fan)[offsetof(FanArgs, lx) / 4 + threadIdx.x];
  static_assert(offsetof(FanArgs, ly) == offsetof(FanArgs, lx) + sizeof(float) * TRT_MAX_FAN_SAMPLES &&
                offsetof(FanArgs, lz) == offsetof(FanArgs, ly) + sizeof(float) * TRT_MAX_FAN_SAMPLES, "FanArgs: one table of 3 x 64 floats");
  stage_scene<ORIENT>(&S, scene);   // (its barrier publishes the table too)

  const FanArgs& f = a.fan;
  const bool     local  = f.frame == TRT_FAN_LOCAL, window = a.tmax > a.tmin;
  const uint32_t samples = f.samples;
  uint32_t       tests  = 0;
  WorkCount      wc;
  const uint32_t tid    = threadIdx.x, lane = tid & 63u;
  const uint32_t wave   = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for(uint64_t base = (uint64_t)blockIdx.x * 256u; base < f.n; base += stride)
  {
    const uint64_t i    = base + tid;
    const bool     live = i < f.n && window && fan_live(f, i);
    const unsigned long long vote = __ballot(live);
    if(lane == 0u) wave_live[wave] = (uint32_t)__popcll(vote);
    __syncthreads();
    uint32_t first = 0, L = 0;   // slots of the waves in front of this one; live points of the block
    for(uint32_t w = 0; w < 4u; ++w)
    {
      const uint32_t c = wave_live[w];
      if(w < wave) first += c;
      L += c;
    }
    const uint32_t j = first + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));   // this lane's slot, if it is live
    if(live)
    {
      const v3 P = fan_point(f, i);
      v3       N = {0.0f, 0.0f, 1.0f};
      if(local) N = fan_normal(f, i);
      const FanBasis tb = fan_basis(N);
      pt[0][j] = P.x; pt[1][j] = P.y; pt[2][j] = P.z;
      pt[3][j] = N.x; pt[4][j] = N.y; pt[5][j] = N.z;
      pt[6][j] = tb.T.x; pt[7][j] = tb.T.y; pt[8][j] = tb.T.z;
      pt[9][j] = tb.B.x; pt[10][j] = tb.B.y; pt[11][j] = tb.B.z;
      word[j][0] = 0u;
      word[j][1] = 0u;
    }
    __syncthreads();
    const uint32_t pairs = L * samples;   // <= 256 * 64
    for(uint32_t q0 = 0; q0 < pairs; q0 += 256u)
    {
      const uint32_t q = q0 + tid;
      if(q < pairs)
      {
        const uint32_t s = q / L, k = q - s * L;
        const v3 P = {pt[0][k], pt[1][k], pt[2][k]};
        const float lx = tab[0][s], ly = tab[1][s], lz = tab[2][s];
        v3 d = {lx, ly, lz};
        if(local)
        {
          const v3       N  = {pt[3][k], pt[4][k], pt[5][k]};
          const FanBasis tb = {{pt[6][k], pt[7][k], pt[8][k]}, {pt[9][k], pt[10][k], pt[11][k]}};
          d = fan_dir(tb, N, lx, ly, lz);
        }
        if(any_hit<Real, ALT, ORIENT, kOccludedWalk>(S, P, d, a.tmin, a.tmax, tests, wc))
          atomicOr(&word[k][s >> 5], 1u << (s & 31u));
      }
    }
    __syncthreads();
    if(i < f.n)
      fan_store(a, i, live ? ((unsigned long long)word[j][1] << 32) | word[j][0] : 0ull);
    // (the next trip writes wave_live first and meets a barrier before anybody writes pt / word again)
  }
  if(a.stats)
    block_add_stats(a.stats, 0u, 0u, tests, wc);
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
// One block per 256 points (at most 4096: grid-stride); no scene, no solver.
hipError_t launch_fan_rays(const FanRaysArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.fan.n == 0)
    return hipSuccess;
  hipLaunchKernelGGL(fan_rays_kernel, dim3(stream_grid(a.fan.n, tn)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// Every solver and oriented tori, through the dispatch of launch_occluded.  The release library launches form kFanForm and
// compiles no other; a -DTRT_TUNING build has both and takes TRT_FAN_FORM (tools/bench_fan.py times them).
namespace {
template <int FORM, class Real, bool ALT, bool ORIENT>
hipError_t launch_fan_form(const SceneK& scene, const FanOccludedArgs& a, uint32_t grid, hipStream_t stream)
{
  if constexpr(FORM == kFanBlock)
    hipLaunchKernelGGL((fan_occluded_block_kernel<Real, ALT, ORIENT>), dim3(grid), dim3(256), 0, stream, scene, a);
  else
    hipLaunchKernelGGL((fan_occluded_kernel<Real, ALT, ORIENT>), dim3(grid), dim3(256), 0, stream, scene, a);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_fan_occluded(const SceneK& scene, const FanOccludedArgs& a, const Tuning& tn, hipStream_t stream)
{
  if(a.fan.n == 0)
    return hipSuccess;
  const uint32_t grid = stream_grid(a.fan.n, tn);
  return with_solver(scene, [&](auto real, auto alt, auto ori) {
    using Real = decltype(real);
    constexpr bool ALT = decltype(alt)::value, ORIENT = decltype(ori)::value;
#ifdef TRT_TUNING   // TRT_FAN_FORM: the other form (bit-identical words, open and counts)
    constexpr int kOther = kFanForm == kFanLane ? kFanBlock : kFanLane;
    if(tn.fan_form == kOther)
      return launch_fan_form<kOther, Real, ALT, ORIENT>(scene, a, grid, stream);
#endif
    return launch_fan_form<kFanForm, Real, ALT, ORIENT>(scene, a, grid, stream);
  });
}

}  // namespace trt
