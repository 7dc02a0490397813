// trt_splat.hip — gfx950 (MI355X / CDNA4) point-cloud re-projection of the toroidal ray tracer (trt_splat_dev): the
// z-buffered point splatting of SEC/, in the form splat_plan picks (SplatMode, trt_splat.hpp).
//
//   splat_bin_kernel          paged (the default up to kSortBins bins): projects the points and scatters their 12-B
//                             records by bin into pages, one sweep;
//   splat_count_kernel        the two-pass forms: projects the points and counts them per bin, then
//   splat_scatter[_sorted]_kernel  writes the records of each bin into its range — direct: images of more than kSortBins
//                             bins; sorted: clouds the page scheme cannot address (splat_plan's fallback).  By splat_plan's
//                             arithmetic (derived on the host, not measured) the release build first takes the sorted form
//                             at 33.6 M points on a 4096² image (2,048 bins), 44.7 M at 4096x2048 (1,024), 67.1 M at 2048²
//                             (512), 134 M at 1024² (128), never on an image of a dozen bins; from 153 M points (8 GiB of
//                             scratch) every image takes the one-pass form;
//   splat_resolve_bins_kernel one block per bin: the depth test in LDS, then every pixel of the bin written once;
//   splat_clear/points/resolve_kernel  the one-pass form (global atomicMin on per-pixel keys): points wider than 32
//                             pixels, images beyond 16,383 pixels a side or kSplatMaxBins bins, clouds whose records
//                             would take more than 8 GiB.
//
// The paged and the sorted scatter sort a chunk of points by bin in LDS, each in its own words: one set of helpers for both
// compiled to other code in all four instantiations and measured slower (profiles/r12_splat_sort.txt), so only the
// encoding of a staged record's bin (splat_stage_rec) is shared — a fix to one chunk sort belongs in the other too.
// Every form produces the same image bit for bit (test_splat_bit_exact: paged, direct, one-pass;
// tests/test_gpu_splat_forms.py: sorted).  Compiled with -ffp-contract=off (see trt_device.hpp for the arithmetic contract).
#include "trt_splat.hpp"

#include <cstdlib>
#include <type_traits>

namespace trt {

// ------------------------------------------------------------------------------------------
// point-cloud re-projection (SEC/): z-buffered point splatting with 64-bit atomic keys
// ------------------------------------------------------------------------------------------
// key = depth24 << 32 | point index.  atomicMin over the keys of a pixel yields the smallest
// depth and, among equal depths, the smallest index — exactly what in-order rasterisation
// with depth test LESS produces.  A cleared pixel holds 0x00FFFFFF'00000000, which no fragment
// can beat unless its depth is < 1.0 (LESS).  HBM-bound integer work: 32 B read per point,
// 8-B atomics on its ≈6 pixels, one 8-B read + 16-B write per pixel in the resolve.
constexpr unsigned long long kSplatClear = 0x00FFFFFFull << 32;

__global__ __launch_bounds__(256) void splat_clear_kernel(unsigned long long* keys, uint64_t n)
{
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    keys[i] = kSplatClear;
}

struct SplatArgs {
  float    vp[16];
  uint32_t W, H;
  float    half;   // point_size / 2
};

// Vertex stage + point rasterisation set-up of one point: false when the vertex is clipped or the point
// covers no pixel centre; else its 24-bit depth and the pixel rectangle [x0,x1) × [y0,y1) it covers.
__device__ __forceinline__ bool splat_project(float4 p, const SplatArgs& a, uint32_t& z24, int& x0, int& x1, int& y0, int& y1)
{
  // gl_Position = uni.viewProj * vec4(position, 1.0)   (SEC vert_shader.vert:51)
  const float cx = fma_(a.vp[12], 1.0f, fma_(a.vp[8], p.z, fma_(a.vp[4], p.y, a.vp[0] * p.x)));
  const float cy = fma_(a.vp[13], 1.0f, fma_(a.vp[9], p.z, fma_(a.vp[5], p.y, a.vp[1] * p.x)));
  const float cz = fma_(a.vp[14], 1.0f, fma_(a.vp[10], p.z, fma_(a.vp[6], p.y, a.vp[2] * p.x)));
  const float cw = fma_(a.vp[15], 1.0f, fma_(a.vp[11], p.z, fma_(a.vp[7], p.y, a.vp[3] * p.x)));
  if(!(cw > 0.0f && cx >= -cw && cx <= cw && cy >= -cw && cy <= cw && cz >= 0.0f && cz <= cw))
    return false;  // point clipping: the vertex is outside the view volume (NaN lands here too)
  const float iw = 1.0f / cw;
  const float xf = fma_(cx * iw, 0.5f, 0.5f) * (float)a.W;
  const float yf = fma_(cy * iw, 0.5f, 0.5f) * (float)a.H;
  z24 = (uint32_t)rintf((cz * iw) * 16777215.0f);
  // pixel centres c = j + 0.5 with lo <= c < hi  ⇔  j in [ceil(lo - 0.5), ceil(hi - 0.5))
  x0 = max((int)ceilf(xf - a.half - 0.5f), 0); x1 = min((int)ceilf(xf + a.half - 0.5f), (int)a.W);
  y0 = max((int)ceilf(yf - a.half - 0.5f), 0); y1 = min((int)ceilf(yf + a.half - 0.5f), (int)a.H);
  return x0 < x1 && y0 < y1;
}

__global__ __launch_bounds__(256) void splat_points_kernel(const trt_point* __restrict__ pts, uint64_t n, const SplatArgs a,
                                                           unsigned long long* keys)
{
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
  {
    uint32_t z24;
    int x0, x1, y0, y1;
    if(!splat_project(reinterpret_cast<const float4*>(pts)[2 * i], a, z24, x0, x1, y0, y1))
      continue;
    const unsigned long long key = ((unsigned long long)z24 << 32) | (unsigned long long)(uint32_t)i;
    for(int y = y0; y < y1; ++y)
      for(int x = x0; x < x1; ++x)
        atomicMin(&keys[(size_t)y * a.W + x], key);
  }
}

// ---- binned re-projection: the depth test in LDS -------------------------------------------------
// The one-pass form above sends ≈6 64-bit atomicMin per point to the memory side (≈26 G atomics/s chip-wide:
// 2 ms for 8.4 M random points).  Here the screen is cut into bins of 128 × 64 pixels — 8,192 keys = 64 KB, one
// LDS image — and the points are first sorted by bin:
//   count    every block projects its chunk of points ONCE — the 8-B result {depth24, pixel rectangle} goes to a
//            side array — and histograms it over the bins in LDS, one global add per non-empty bin; the block that
//            finishes LAST (a ticket) turns the bin counts into their exclusive prefix (no scan launch);
//   scatter  the chunks again, from the side array, ONE sweep: a block histograms its 4,096 points in LDS, reserves
//            one range per bin (one global add), SORTS its records by bin in an LDS staging area and writes them out
//            in sorted order — a wave's store instruction covers 768 contiguous bytes of a few bin runs instead of
//            64 records at 64 unrelated addresses (round 2: 16-B records written one by one, each 32-B sector of
//            HBM written twice — 273 MB of writes for 134 MB of records);
//   resolve  ONE block per bin: atomicMin of the keys in LDS (ds_min_u64), then every pixel of the bin is written
//            once — colour of the winning point, or the clear colour.
// Records are 12 B: {point index, depth24, rectangle inside the bin (4 × 7 bits)}.
// The keys, and so the image, are those of the one-pass form bit for bit (a minimum does not depend on the
// order of its operands).  A point wider than a bin edge would need more than 4 records: such sizes, and images
// with more than kSplatMaxBins bins, take the one-pass form.
constexpr uint32_t kBinW = 128, kBinH = 64, kSplatChunk = 8192, kSplatMaxDim = 16383;   // (kSplatMaxBins: trt_splat.hpp)

struct SplatRec { uint32_t idx, z, rect; };   // rect = rx0 | rx1 << 7 | ry0 << 15 | ry1 << 21  (bin-relative, half-open)

struct SplatBins {
  uint32_t  bins_x, bins_y, n_bins;
  uint32_t* count;    // [n_bins]   points per bin: accumulated by `count`, zeroed again by `resolve`
  uint32_t* offset;   // [n_bins]   first record of the bin (written by the last block of `count`)
  uint32_t* cursor;   // [n_bins]   records handed out so far (zeroed with the offsets)
  uint32_t* ticket;   // blocks of `count` that have finished
  uint32_t* table;    // [chunks of 4,096 points][n_bins] (sorted scatter only): where in its bin's range a chunk's records start —
                      // what `count`'s returning add on the bin's count word returned; nullptr: `scatter` draws from `cursor`
  SplatRec* records;  // [<= 4 · n_points]
  uint2*    proj;     // [n_points] the projected points (count → scatter)
  uint32_t  debug_skip;   // -DTRT_TUNING builds only (timing ablations of `resolve`: 16 no colour gather, 32 no depth test, 64 no record loads)
  // paged scatter (splat_bin_kernel): `records` is cut into pages of 1 << page_shift records; page k < n_bins is bin k's
  // first page, the pages behind them are handed out from a pool as bins fill up
  unsigned long long* state;  // [n_bins] fill (24 bits) | epoch (12) | handle of the current page (14) | handle of the next one (14): the bin's two-page window (splat_bin_kernel); handle 0 = the bin's own page, h > 0 = pool page h - 1; zero between calls
  uint32_t* pool;             // pool pages handed out (zero between calls)
  uint32_t* page_bin;         // [pool_pages] the bin a pool page belongs to
  uint32_t* rticket;          // blocks of `resolve` that have finished (zero between calls)
  uint32_t* page_seq;         // [pool_pages] … and which of that bin's pages it is (abstract page number, 12 bits)
  uint32_t  page_shift, pool_pages;   // a page holds 1 << page_shift records; pages 0 .. 2·n_bins-1 are the bins' own two
};

// projected point in 64 bits: x0 (14) | y0 (14) | width low 4 bits ; depth24 | width high 2 bits | height (6).
// W, H <= 16383 and point_size <= 32 (width, height <= 33) on this path; width 0 = the point draws nothing.
__device__ __forceinline__ uint2 splat_pack(uint32_t z24, int x0, int x1, int y0, int y1)
{
  const uint32_t w = (uint32_t)(x1 - x0), h = (uint32_t)(y1 - y0);
  return make_uint2((uint32_t)x0 | ((uint32_t)y0 << 14) | ((w & 15u) << 28), z24 | ((w >> 4) << 24) | (h << 26));
}
__device__ __forceinline__ bool splat_unpack(uint2 p, uint32_t& z24, int& x0, int& x1, int& y0, int& y1)
{
  const uint32_t w = (p.x >> 28) | (((p.y >> 24) & 3u) << 4), h = p.y >> 26;
  x0 = (int)(p.x & 16383u); y0 = (int)((p.x >> 14) & 16383u); x1 = x0 + (int)w; y1 = y0 + (int)h;
  z24 = p.y & 0xffffffu;
  return w != 0u;
}
__device__ __forceinline__ uint32_t splat_rect(int rx0, int rx1, int ry0, int ry1)
{
  return (uint32_t)rx0 | ((uint32_t)rx1 << 7) | ((uint32_t)ry0 << 15) | ((uint32_t)ry1 << 21);
}

// calls f(bin, x0r, x1r, y0r, y1r) for every bin the rectangle touches, rectangle clipped to the bin, bin-relative
template <class F>
__device__ __forceinline__ void splat_for_bins(const SplatBins& b, int x0, int x1, int y0, int y1, F f)
{
  const int bx0 = x0 / (int)kBinW, bx1 = (x1 - 1) / (int)kBinW, by0 = y0 / (int)kBinH, by1 = (y1 - 1) / (int)kBinH;
  for(int by = by0; by <= by1; ++by)
    for(int bx = bx0; bx <= bx1; ++bx)
    {
      const int ox = bx * (int)kBinW, oy = by * (int)kBinH;
      f((uint32_t)by * b.bins_x + (uint32_t)bx, max(x0 - ox, 0), min(x1 - ox, (int)kBinW), max(y0 - oy, 0), min(y1 - oy, (int)kBinH));
    }
}

// M sub-chunks of SUB points per block, 256 threads each (blockDim.x = M·256).  The direct scatter (M = 1, SUB = kSplatChunk)
// only needs the bins' totals.  The sorted scatter (TABLE: SUB = its chunk of 4,096 points, M = 4) also needs to know where in
// a bin's range each of ITS chunks starts: the block keeps one histogram per sub-chunk, adds their sum to the bin's count word
// with ONE returning atomic — what comes back is the number of records earlier blocks have claimed — and writes the sub-chunks'
// starts to table[chunk][bin]; the scatter then draws from no cursor at all (one million returning atomics less per call).
template <uint32_t SUB, uint32_t M, bool TABLE>
__global__ __launch_bounds__(M * 256) void splat_count_kernel(const trt_point* __restrict__ pts, uint64_t n, const SplatArgs a, const SplatBins b)
{
  extern __shared__ uint32_t hist_all[];   // [M][n_bins]
  __shared__ uint32_t part[256];
  __shared__ int      is_last;
  for(uint32_t k = threadIdx.x; k < M * b.n_bins; k += M * 256u) hist_all[k] = 0u;
  __syncthreads();
  const uint32_t m = threadIdx.x >> 8, t = threadIdx.x & 255u;
  uint32_t* hist = hist_all + m * b.n_bins;
  const uint64_t i0 = ((uint64_t)blockIdx.x * M + m) * SUB, i1 = min(n, i0 + SUB);
  // four points per lane and trip, their loads issued together (one 16-B load in flight per lane was latency-bound)
  constexpr uint32_t U = 4;
  for(uint64_t ib = i0 + t; ib < i1; ib += U * 256u)
  {
    float4 p[U];
#pragma unroll
    for(uint32_t u = 0; u < U; ++u)
    {
      const uint64_t i = ib + u * 256u;
      p[u] = i < i1 ? reinterpret_cast<const float4*>(pts)[2 * i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for(uint32_t u = 0; u < U; ++u)
    {
      const uint64_t i = ib + u * 256u;
      if(i >= i1) continue;
      uint32_t z24;
      int x0, x1, y0, y1;
      uint2 pk = make_uint2(0u, 0u);
      if(splat_project(p[u], a, z24, x0, x1, y0, y1))
      {
        pk = splat_pack(z24, x0, x1, y0, y1);
        splat_for_bins(b, x0, x1, y0, y1, [&](uint32_t bin, int, int, int, int) { atomicAdd(&hist[bin], 1u); });
      }
      b.proj[i] = pk;
    }
  }
  __syncthreads();
  // RETURNING adds: their results are back — the additions performed, at device scope — before the barrier in front of the
  // block's ticket.  (No __threadfence(): an agent-scope release writes back the XCD's whole L2, the chunk's freshly written
  // side array included — measured: the call 0.32 → 0.43 ms.)
  uint32_t sink = 0;
  for(uint32_t k = threadIdx.x; k < b.n_bins; k += M * 256u)
  {
    uint32_t c[M], total = 0;
#pragma unroll
    for(uint32_t j = 0; j < M; ++j) { c[j] = hist_all[j * b.n_bins + k]; total += c[j]; }
    uint32_t run = total ? atomicAdd(&b.count[k], total) : 0u;
    sink |= run;
    if(TABLE)
    {
#pragma unroll
      for(uint32_t j = 0; j < M; ++j)
      {
        b.table[((size_t)blockIdx.x * M + j) * b.n_bins + k] = run;
        run += c[j];
      }
    }
  }
  if(sink == 0xffffffffu) part[threadIdx.x & 255u] = sink;   // (never true: a bin holds fewer than 2^32 records) keeps the results live
  // the block that finishes last — every other block's additions are then performed — turns the counts into offsets
  __syncthreads();
  if(threadIdx.x == 0)
    is_last = atomicAdd(b.ticket, 1u) == gridDim.x - 1 ? 1 : 0;
  __syncthreads();
  if(!is_last || threadIdx.x >= 256u)
    return;
  const uint32_t per = (b.n_bins + 255u) / 256u, k0 = threadIdx.x * per, k1 = min(b.n_bins, k0 + per);
  uint32_t sum = 0;
  for(uint32_t k = k0; k < k1; ++k) sum += __hip_atomic_load(&b.count[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  part[threadIdx.x] = sum;
  __syncthreads();   // (only the block's first 256 threads are left: four whole waves)
  if(threadIdx.x == 0)
  {
    uint32_t run = 0;
    for(uint32_t q = 0; q < 256u; ++q) { const uint32_t c = part[q]; part[q] = run; run += c; }
    *b.ticket = 0u;   // the next call counts its blocks from zero
  }
  __syncthreads();
  uint32_t run = part[threadIdx.x];
  for(uint32_t k = k0; k < k1; ++k)
  {
    b.offset[k] = run;
    b.cursor[k] = 0u;
    run += __hip_atomic_load(&b.count[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// scatter, sorted: up to kSortBins bins (2048: images up to 4096² and beyond), 4,096 points per block of 512 threads,
// 12-B records staged in LDS in bin order.  LDS: 3 words per bin + 12 B per staged record = 78 KB: two blocks per CU.
constexpr uint32_t kSortBins = 2048, kSortChunk = 4096, kSortThreads = 512, kSortPer = kSortChunk / kSortThreads, kSortStage = 4608;
// A staged record of the sorted and of the paged scatter carries its bin in its spare bits: z is a depth24 (splat_project: at
// most 16777215) and rect ends with ry1 <= 64 at bit 21, below 2^28 — bits 31..24 of z take the bin's low byte, bits 30..28
// of rect its three high bits.
static_assert(kSortBins <= (1u << 11) && kBinW <= 128u && kBinH <= 64u, "8 + 3 spare bits for the bin; rect = 7 + 8 + 6 + 7 bits");
__device__ __forceinline__ SplatRec splat_stage_rec(uint32_t idx, uint32_t z24, uint32_t rect, uint32_t bin)
{
  return SplatRec{idx, z24 | (bin << 24), rect | ((bin >> 8) << 28)};
}
__device__ __forceinline__ uint32_t splat_staged_bin(SplatRec r) { return (r.z >> 24) | ((r.rect >> 28) << 8); }
__device__ __forceinline__ SplatRec splat_unstage_rec(SplatRec r) { return SplatRec{r.idx, r.z & 0xffffffu, r.rect & 0x0fffffffu}; }
template <uint32_t NB>   // bins the block's LDS arrays hold: 512 (images up to 2048²: 61 KB of LDS) or kSortBins (79 KB)
__global__ __launch_bounds__(kSortThreads) void splat_scatter_sorted_kernel(uint64_t n, const SplatBins b)
{
  __shared__ uint32_t hist[NB];    // points of this block per bin, then the rank counter
  __shared__ uint32_t lbase[NB];   // first staged record of the bin
  __shared__ uint32_t gbase[NB];   // first global record of this block's range in the bin
  __shared__ SplatRec stage[kSortStage];  // records in bin order (splat_stage_rec)
  __shared__ uint32_t wsum[kSortThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for(uint32_t k = tid; k < b.n_bins; k += kSortThreads) hist[k] = 0u;
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * kSortChunk, i1 = min(n, i0 + kSortChunk);
  uint2 pk[kSortPer];
#pragma unroll
  for(uint32_t u = 0; u < kSortPer; ++u)
  {
    const uint64_t i = i0 + u * kSortThreads + tid;
    pk[u] = i < i1 ? b.proj[i] : make_uint2(0u, 0u);
  }
#pragma unroll
  for(uint32_t u = 0; u < kSortPer; ++u)
  {
    uint32_t z24;
    int x0, x1, y0, y1;
    if(splat_unpack(pk[u], z24, x0, x1, y0, y1))
      splat_for_bins(b, x0, x1, y0, y1, [&](uint32_t bin, int, int, int, int) { atomicAdd(&hist[bin], 1u); });
  }
  __syncthreads();
  // exclusive prefix of the block's bin counts (the staging order) + one global reservation per non-empty bin
  constexpr uint32_t kPerT = NB / kSortThreads;   // 1 or 4 consecutive bins per thread
  uint32_t c[kPerT], mine = 0;
#pragma unroll
  for(uint32_t j = 0; j < kPerT; ++j)
  {
    const uint32_t k = tid * kPerT + j;
    c[j] = k < b.n_bins ? hist[k] : 0u;
    mine += c[j];
  }
  uint32_t inc = mine;
#pragma unroll
  for(int off = 1; off < 64; off <<= 1)
  {
    const uint32_t v = __shfl_up(inc, off, 64);
    if(lane >= (uint32_t)off) inc += v;
  }
  if(lane == 63u) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = inc - mine;
  for(uint32_t w = 0; w < wave; ++w) before += wsum[w];
  uint32_t total = 0;
  for(uint32_t w = 0; w < kSortThreads / 64; ++w) total += wsum[w];
#pragma unroll
  for(uint32_t j = 0; j < kPerT; ++j)
  {
    const uint32_t k = tid * kPerT + j;
    if(k < b.n_bins)
    {
      lbase[k] = before;
      gbase[k] = c[j] ? b.offset[k] + b.table[(size_t)blockIdx.x * b.n_bins + k] : 0u;   // (this chunk's start in the bin: `count`)
      hist[k]  = 0u;
      before += c[j];
    }
  }
  __syncthreads();
  // place: rank inside the bin from the LDS counter; records beyond the staging area (a chunk whose points straddle
  // many bins) go straight to their place in global memory
#pragma unroll
  for(uint32_t u = 0; u < kSortPer; ++u)
  {
    uint32_t z24;
    int x0, x1, y0, y1;
    if(splat_unpack(pk[u], z24, x0, x1, y0, y1))
    {
      const uint32_t idx = (uint32_t)(i0 + u * kSortThreads + tid);
      splat_for_bins(b, x0, x1, y0, y1, [&](uint32_t bin, int rx0, int rx1, int ry0, int ry1) {
        const uint32_t rank = atomicAdd(&hist[bin], 1u), slot = lbase[bin] + rank, rect = splat_rect(rx0, rx1, ry0, ry1);
        if(slot < kSortStage)
          stage[slot] = splat_stage_rec(idx, z24, rect, bin);
        else
          b.records[gbase[bin] + rank] = SplatRec{idx, z24, rect};
      });
    }
  }
  __syncthreads();
  const uint32_t n_staged = umin(total, kSortStage);
  for(uint32_t j = tid; j < n_staged; j += kSortThreads)
  {
    const SplatRec r = stage[j];
    const uint32_t bin = splat_staged_bin(r);
    b.records[gbase[bin] + (j - lbase[bin])] = splat_unstage_rec(r);
  }
}

// ---- paged scatter: count + scatter in ONE sweep over the points (default for up to kSortBins bins) -----------------
// The two-pass form reads the cloud to count (268 MB for 8.4 M points), writes the 8-B projections, reads them back and
// only then knows where a bin's records go.  Here nobody needs to know: the record area is cut into PAGES of S records,
// every bin owns two of them and takes more from a pool as it fills up, and a 64-bit word per bin says where the next
// record goes (the two-page window, in the kernel).  A block projects its 4,096 points, sorts their records by bin in LDS
// (as the sorted scatter does) and reserves a bin's run with ONE returning 64-bit add of its length.  Every page of a bin
// except the last two is completely filled and a pool page carries a note {bin, which page of the bin}, so `resolve`
// needs no page table: it picks its bin's pages out of the notes (a few thousand words) and reads the fill of the last
// two from the bin's word.  One launch less, no side array, no table: 8.4 M random points 0.215 -> 0.19 ms, a captured
// cloud in capture order 0.134 -> 0.095 ms, 873 -> 728 MB per call.
constexpr uint32_t kPageSpins = 1u << 22;
constexpr unsigned long long kPagePoison = (0x3fffull << 50) | (0x3fffull << 36) | (0xfffull << 24);   // both handles all ones: adds to `fill` leave it recognisable
template <uint32_t NB>   // bins the block's LDS arrays hold: 512 (images up to 2048²) or kSortBins
__global__ __launch_bounds__(kSortThreads, 4) void splat_bin_kernel(const trt_point* __restrict__ pts, uint64_t n, const SplatArgs a, const SplatBins b)
{
  constexpr uint32_t kStage = NB <= 512u ? 4608u : 3968u;   // 65 KB / 79 KB of LDS: two blocks per CU either way
  __shared__ uint32_t hist[NB];     // points of this block per bin, then the rank counter
  __shared__ uint32_t lfirst[NB];   // first staged record of the bin (bits 0..15) | records of its run in the first page (16..28)
  __shared__ uint32_t g0[NB];       // where the run starts (record index); ~0: the run is dropped
  __shared__ uint32_t g1[NB];       // where it goes on behind the page end
  __shared__ SplatRec stage[kStage];
  __shared__ uint32_t wsum[kSortThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // The block walks the chunks blockIdx, blockIdx + gridDim, …; the points of its NEXT chunk are loaded (8 x 16 B per
  // lane) before the current one is sorted, so that the reads run behind the LDS phases — two blocks per CU leave too few
  // waves to hide them otherwise (one chunk per block: 110 µs for the 8.4 M-point cloud).
  const uint64_t n_chunks = (n + kSortChunk - 1) / kSortChunk;
  float4 pn[kSortPer];
  auto fetch = [&](uint64_t chunk) {
    const uint64_t f0 = chunk * kSortChunk, f1 = min(n, f0 + kSortChunk);
#pragma unroll
    for(uint32_t u = 0; u < kSortPer; ++u)
    {
      const uint64_t i = f0 + u * kSortThreads + tid;
      pn[u] = chunk < n_chunks && i < f1 ? reinterpret_cast<const float4*>(pts)[2 * i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
  };
  constexpr bool kPrefetch = NB <= 512u;   // (the wider instantiation has four bins per thread to keep: prefetching would spill)
  if(kPrefetch) fetch(blockIdx.x);
  for(uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
  {
  if(!kPrefetch) fetch(chunk);
  for(uint32_t k = tid; k < b.n_bins; k += kSortThreads) hist[k] = 0u;
  __syncthreads();   // (also: the previous chunk's write-out has read the staging area and the bins' places)
  const uint64_t i0 = chunk * kSortChunk, i1 = min(n, i0 + kSortChunk);
  uint2 pk[kSortPer];
  {
    float4 p[kSortPer];
#pragma unroll
    for(uint32_t u = 0; u < kSortPer; ++u) p[u] = pn[u];
    if(kPrefetch) fetch(chunk + gridDim.x);
#pragma unroll
    for(uint32_t u = 0; u < kSortPer; ++u)
    {
      uint32_t z24;
      int x0, x1, y0, y1;
      pk[u] = make_uint2(0u, 0u);
      if(i0 + u * kSortThreads + tid < i1 && splat_project(p[u], a, z24, x0, x1, y0, y1))
      {
        pk[u] = splat_pack(z24, x0, x1, y0, y1);
        splat_for_bins(b, x0, x1, y0, y1, [&](uint32_t bin, int, int, int, int) { atomicAdd(&hist[bin], 1u); });
      }
    }
  }
  __syncthreads();
  // exclusive prefix of the block's bin counts (the staging order)
  constexpr uint32_t kPerT = NB / kSortThreads;   // 1 or 4 consecutive bins per thread
  uint32_t c[kPerT], mine = 0;
#pragma unroll
  for(uint32_t j = 0; j < kPerT; ++j)
  {
    const uint32_t k = tid * kPerT + j;
    c[j] = k < b.n_bins ? hist[k] : 0u;
    mine += c[j];
  }
  // one reservation per non-empty bin, ISSUED here and looked at after the prefix: the round trip of the returning add
  // runs behind it
  unsigned long long got[kPerT];
#pragma unroll
  for(uint32_t j = 0; j < kPerT; ++j)
    got[j] = c[j] ? atomicAdd(&b.state[tid * kPerT + j], (unsigned long long)c[j]) : 0ull;
  uint32_t inc = mine;
#pragma unroll
  for(int off = 1; off < 64; off <<= 1)
  {
    const uint32_t v = __shfl_up(inc, off, 64);
    if(lane >= (uint32_t)off) inc += v;
  }
  if(lane == 63u) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = inc - mine;
  for(uint32_t w = 0; w < wave; ++w) before += wsum[w];
  uint32_t total = 0;
  for(uint32_t w = 0; w < kSortThreads / 64; ++w) total += wsum[w];
#pragma unroll
  for(uint32_t j = 0; j < kPerT; ++j)
  {
    const uint32_t k = tid * kPerT + j;
    if(k >= b.n_bins) continue;
    lfirst[k] = before;
    hist[k]   = 0u;
    before += c[j];
  }
  __syncthreads();
  // Where a bin's run goes — the two-page WINDOW.  A bin's records fill pages of S records one after the other: abstract
  // page 0 and 1 are the bin's own (static), the following ones come from the pool.  The bin's 64-bit word holds
  // {fill, epoch e, handle of the CURRENT page (abstract page e), handle of the NEXT one (e + 1)}; `fill` counts from the
  // start of the current page, so the word describes a window of 2·S slots whose pages are both known.  An add of c returns
  // where the run starts (f) and in which pages: nobody waits for a page to be handed out while its run fits the window.
  // The adder whose run contains the next page's FIRST slot (f <= S < f + c) ROTATES the window once its add is back: it
  // takes a page from the pool, notes {bin, abstract page} for `resolve`, and adds ONE delta to the word that makes
  // {fill - S, e + 1, next, new page} of it — an add, so the adds of others commute with it and what they got back still
  // means the same slots.  Only a run that ends beyond the window (more than S records arrived at this bin within one
  // rotation: a crowded bin) waits — re-reading the word once per loop trip, so that lanes of the same wave that rotate for
  // other bins are never held up — until the epoch has advanced far enough; the rotation it waits for is made by an adder
  // inside the window, who waits for nothing.  Should the window have moved PAST a waiter's slots before it looks again, it
  // finds its pages by their abstract number in the pool's notes (slow, and never seen).  A bound on the re-reads
  // (kPageSpins) ends a wait that would not end: the bin is poisoned and stays empty, the grid drains.
  const uint32_t S = 1u << b.page_shift;
  auto page_at = [&](uint32_t k, uint32_t handle, uint32_t P) -> uint32_t {   // first record of abstract page P, handle as in the word
    return handle ? (2u * b.n_bins + (handle - 1u)) << b.page_shift : (((P & 1u) ? b.n_bins : 0u) + k) << b.page_shift;   // (handle 0: P is 0 or 1, the bin's own)
  };
  auto find_page = [&](uint32_t k, uint32_t P) -> uint32_t {   // abstract page P of bin k (the slow way)
    if(P < 2u) return ((P ? b.n_bins : 0u) + k) << b.page_shift;
    // the page exists (the window has been there); its notes were stored before the rotation's add but may become
    // visible after it: look again until they are (bounded)
    for(uint32_t tries = 0; tries < 4096u; ++tries)
    {
      const uint32_t used = umin(__hip_atomic_load(b.pool, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), b.pool_pages);
      for(uint32_t q = 0; q < used; ++q)
        if(__hip_atomic_load(&b.page_bin[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == k
           && __hip_atomic_load(&b.page_seq[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (P & 0xfffu))
          return (2u * b.n_bins + q) << b.page_shift;
      __builtin_amdgcn_s_sleep(64);
    }
    return ~0u;
  };
  auto resolve = [&]() {
#pragma unroll
  for(uint32_t j = 0; j < kPerT; ++j)
  {
    const uint32_t k = tid * kPerT + j, cj = c[j];
    if(k >= b.n_bins) continue;
    uint32_t first = cj, at0 = 0u, at1 = 0u, spins = 0u;
    bool done = cj == 0u;
    const unsigned long long mine = got[j];
    const uint32_t f0 = (uint32_t)mine & 0xffffffu, e0 = (uint32_t)(mine >> 24) & 0xfffu;
    unsigned long long w = mine;   // the word as last seen: the add's result first, re-read while the run lies beyond the window
    while(!done)
    {
      const uint32_t e = (uint32_t)(w >> 24) & 0xfffu, cur = (uint32_t)(w >> 36) & 0x3fffu, nxt = (uint32_t)(w >> 50);
      const uint32_t de = (e - e0) & 0xfffu;                       // rotations since the add
      const long long f = (long long)f0 - (long long)de * (long long)S;   // the run's start, counted from the current page
      if(cur == 0x3fffu && nxt == 0x3fffu) { at0 = ~0u; done = true; }   // poisoned
      else if(f < 0 && f + (long long)cj <= 0)
      {
        // the window has moved past the whole run (never seen): its page by its abstract number
        const uint32_t P = e0 + f0 / S, r0 = f0 % S;
        const uint32_t a0 = find_page(k, P), a1 = r0 + cj > S ? find_page(k, P + 1u) : 0u;
        first = umin(cj, S - r0);
        at0 = a0 == ~0u || a1 == ~0u ? ~0u : a0 + r0;
        at1 = a1;
        done = true;
      }
      else if(f + (long long)cj <= 2ll * S)
      {
        // inside the window (or straddling its start: never seen either)
        const long long g = f < 0 ? 0 : f;   // (f < 0: the run began in the page before the current one)
        if(f < 0)
        {
          const uint32_t a0 = find_page(k, e0 + f0 / S);
          first = (uint32_t)(-f);
          at0 = a0 == ~0u ? ~0u : a0 + f0 % S;
          at1 = page_at(k, cur, e);
        }
        else if(g >= (long long)S) { at0 = page_at(k, nxt, e + 1u) + (uint32_t)(g - S); }
        else
        {
          first = umin(cj, S - (uint32_t)g);
          at0 = page_at(k, cur, e) + (uint32_t)g;
          at1 = page_at(k, nxt, e + 1u);
        }
        if(f <= (long long)S && f + (long long)cj > (long long)S)
        {
          // this run holds the NEXT page's first slot (the current page is reserved to its end): rotate the window.  (Not
          // "the current page's last slot": a run that ends exactly there would have to rotate later, when it no longer looks.)
          const uint32_t q = atomicAdd(b.pool, 1u);
          if(q < b.pool_pages)
          {
            __hip_atomic_store(&b.page_bin[q], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&b.page_seq[q], ((e + 2u) & 0xfffu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // (modular 64-bit arithmetic: the word + delta = {fill - S, e + 1, nxt, q + 1} whatever others have added to fill)
            const unsigned long long delta = (1ull << 24) + (((unsigned long long)nxt - (unsigned long long)cur) << 36)
                                             + (((unsigned long long)(q + 1u) - (unsigned long long)nxt) << 50) - (unsigned long long)S;
            atomicAdd(&b.state[k], delta);
          }
          else   // (cannot happen: the pool holds more pages than the bins can fill)
            atomicExch(&b.state[k], kPagePoison);
        }
        done = true;
      }
      else
      {
        __builtin_amdgcn_s_sleep(8);
        if(TRT_SKIP(b, 128u))   // tuning build: waiters that look again only after ~50 µs — the window moves past them (find_page)
          for(int z = 0; z < 64; ++z) __builtin_amdgcn_s_sleep(127);
        w = __hip_atomic_load(&b.state[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if(++spins > kPageSpins)
        {
          at0 = ~0u;
          atomicExch(&b.state[k], kPagePoison);
          done = true;
        }
      }
    }
    // (belt and braces: a word that adds have pushed out of its poison pattern could name pages that do not exist —
    // nothing is ever written outside the record area)
    const uint32_t limit = (2u * b.n_bins + b.pool_pages) << b.page_shift;
    if(at0 != ~0u && (at0 > limit - first || (first < cj && at1 > limit - (cj - first)))) at0 = ~0u;
    lfirst[k] |= first << 16;
    g0[k]      = at0;
    g1[k]      = at1;
  }
  };
  // The reservations are looked at BEFORE the records are sorted — the add's round trip has run behind the prefix — because a
  // run that has to rotate its bin's window should do so at once: others may be waiting for it (measured: resolving after
  // the sort gains nothing on spread clouds and costs 20 % on a cloud that fills a third of the view).
  resolve();
  __syncthreads();
  // place: rank inside the bin from the LDS counter; records beyond the staging area (a chunk whose points straddle
  // many bins) go straight to their place in global memory
  auto place = [&](uint32_t bin, uint32_t rank) -> uint32_t {
    const uint32_t fr = lfirst[bin] >> 16;
    return rank < fr ? g0[bin] + rank : g1[bin] + (rank - fr);
  };
#pragma unroll
  for(uint32_t u = 0; u < kSortPer; ++u)
  {
    uint32_t z24;
    int x0, x1, y0, y1;
    if(splat_unpack(pk[u], z24, x0, x1, y0, y1))
    {
      const uint32_t idx = (uint32_t)(i0 + u * kSortThreads + tid);
      splat_for_bins(b, x0, x1, y0, y1, [&](uint32_t bin, int rx0, int rx1, int ry0, int ry1) {
        const uint32_t rank = atomicAdd(&hist[bin], 1u), slot = (lfirst[bin] & 0xffffu) + rank, rect = splat_rect(rx0, rx1, ry0, ry1);
        if(slot < kStage)
          stage[slot] = splat_stage_rec(idx, z24, rect, bin);
        else if(g0[bin] != ~0u)
          b.records[place(bin, rank)] = SplatRec{idx, z24, rect};
      });
    }
  }
  __syncthreads();
  const uint32_t n_staged = umin(total, kStage);
  for(uint32_t j = tid; j < n_staged; j += kSortThreads)
  {
    const SplatRec r = stage[j];
    const uint32_t bin = splat_staged_bin(r);
    if(g0[bin] != ~0u)
      b.records[place(bin, j - (lfirst[bin] & 0xffffu))] = splat_unstage_rec(r);
  }
  }   // chunks
}

// scatter, direct (images of more than kSortBins bins): every record written at its place.  ONE sweep over the side array:
// the block's 8,192 projected points stay in registers (16 per lane of 512, loaded together) between the counting and the
// placing pass.
constexpr uint32_t kDirectThreads = 512, kDirectPer = kSplatChunk / kDirectThreads;
__global__ __launch_bounds__(kDirectThreads) void splat_scatter_kernel(uint64_t n, const SplatBins b)
{
  extern __shared__ uint32_t lds[];
  uint32_t* hist = lds;             // [n_bins] points of this block per bin, then the rank counter
  uint32_t* base = lds + b.n_bins;  // [n_bins] first record of this block's range in the bin
  for(uint32_t k = threadIdx.x; k < b.n_bins; k += kDirectThreads) hist[k] = 0u;
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * kSplatChunk, i1 = min(n, i0 + kSplatChunk);
  uint2 pk[kDirectPer];
#pragma unroll
  for(uint32_t u = 0; u < kDirectPer; ++u)
  {
    const uint64_t i = i0 + u * kDirectThreads + threadIdx.x;
    pk[u] = i < i1 ? b.proj[i] : make_uint2(0u, 0u);
  }
#pragma unroll
  for(uint32_t u = 0; u < kDirectPer; ++u)
  {
    uint32_t z24;
    int x0, x1, y0, y1;
    if(splat_unpack(pk[u], z24, x0, x1, y0, y1))
      splat_for_bins(b, x0, x1, y0, y1, [&](uint32_t bin, int, int, int, int) { atomicAdd(&hist[bin], 1u); });
  }
  __syncthreads();
  for(uint32_t k = threadIdx.x; k < b.n_bins; k += kDirectThreads)
  {
    base[k] = hist[k] ? b.offset[k] + atomicAdd(&b.cursor[k], hist[k]) : 0u;
    hist[k] = 0u;
  }
  __syncthreads();
#pragma unroll
  for(uint32_t u = 0; u < kDirectPer; ++u)
  {
    uint32_t z24;
    int x0, x1, y0, y1;
    if(splat_unpack(pk[u], z24, x0, x1, y0, y1))
      splat_for_bins(b, x0, x1, y0, y1, [&](uint32_t bin, int rx0, int rx1, int ry0, int ry1) {
        const uint32_t rank = atomicAdd(&hist[bin], 1u);
        b.records[base[bin] + rank] = SplatRec{(uint32_t)(i0 + u * kDirectThreads + threadIdx.x), z24, splat_rect(rx0, rx1, ry0, ry1)};
      });
  }
}

constexpr int kSplatResolveThreads = 1024;   // 2 blocks of 64 KB LDS per CU: 32 waves, all the CU holds
constexpr uint32_t kPageList = 2056;         // pages a bin can hold (PAGED; see the kernel)
// the depth test of a batch of records: ds_min_u64 on the pixels of their rectangles.  (A plain LDS read in front of the
// atomic, to keep the three quarters of the fragments that lose away from the atomic unit, makes it SLOWER — 104.6 against
// 81.6 µs: the read is a round trip, the atomic is not.)
template <uint32_t kR>
__device__ __forceinline__ void splat_depth_test(unsigned long long* keys, const SplatRec (&rec)[kR])
{
#pragma unroll
  for(uint32_t u = 0; u < kR; ++u)
  {
    const unsigned long long key = ((unsigned long long)rec[u].z << 32) | (unsigned long long)rec[u].idx;
    const uint32_t x0 = rec[u].rect & 127u, x1 = (rec[u].rect >> 7) & 255u, y0 = (rec[u].rect >> 15) & 63u, y1 = (rec[u].rect >> 21) & 127u;
    for(uint32_t y = y0; y < y1; ++y)
      for(uint32_t x = x0; x < x1; ++x)
        atomicMin(&keys[y * kBinW + x], key);
  }
}

// the records of slots 0 .. n_slots-1 through the depth test: four records per lane and trip, their loads issued together
// (eight: +2 %); rec_at(v) is the record of slot v, or the empty record SplatRec{0, 0, 0} (an empty rectangle)
template <class RecAt>
__device__ __forceinline__ void splat_gather_test(const SplatBins& b, unsigned long long* keys, uint32_t n_slots, RecAt rec_at)
{
  constexpr uint32_t kR = 4;
  for(uint32_t rb = threadIdx.x; rb < n_slots; rb += kR * blockDim.x)
  {
    SplatRec rec[kR];
#pragma unroll
    for(uint32_t u = 0; u < kR; ++u)
      rec[u] = TRT_SKIP(b, 64u) ? SplatRec{0u, 0u, 0u} : rec_at(rb + u * blockDim.x);
    if(TRT_SKIP(b, 32u)) continue;
    splat_depth_test<kR>(keys, rec);
  }
}

template <bool PAGED>
__global__ __launch_bounds__(kSplatResolveThreads) void splat_resolve_bins_kernel(const trt_point* __restrict__ pts, const SplatArgs a, const SplatBins b,
                                                                                  float4 clear, float4* rgba)
{
  __shared__ unsigned long long keys[kBinW * kBinH];
  __shared__ uint32_t plist[PAGED ? kPageList : 1], n_list;
  for(uint32_t k = threadIdx.x; k < kBinW * kBinH; k += blockDim.x) keys[k] = kSplatClear;
  const uint32_t bin = blockIdx.x;
  if(PAGED)
  {
    // the bin's pages: its own two (abstract pages 0 and 1) and the pool pages whose notes name it; how many records a
    // page holds follows from its abstract number P and the bin's word {fill, epoch e, …}: every page before the current
    // one (P < e) is full, the current one holds min(fill, S), the next one what is left of fill.  The page size
    // (splat_plan) makes n_points / S < 2,049, and a bin holds at most one record per point: the list cannot overflow.
    const unsigned long long st = b.state[bin];
    const uint32_t S = 1u << b.page_shift, fill = (uint32_t)st & 0xffffffu, e = (uint32_t)(st >> 24) & 0xfffu;
    const bool     poisoned = ((uint32_t)(st >> 36) & 0x3fffu) == 0x3fffu && (uint32_t)(st >> 50) == 0x3fffu;   // (a reservation gave up, splat_bin_kernel: the bin stays empty)
    const uint32_t used = umin(__hip_atomic_load(b.pool, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), b.pool_pages);
    if(threadIdx.x == 0)
    {
      n_list   = 2u;
      plist[0] = bin;                      // page index | abstract number << 16
      plist[1] = (b.n_bins + bin) | (1u << 16);
    }
    __syncthreads();   // (also: the keys are initialised)
    for(uint32_t q = threadIdx.x; q < used && !poisoned; q += blockDim.x)
      if(b.page_bin[q] == bin)
      {
        const uint32_t en = atomicAdd(&n_list, 1u);
        if(en < kPageList) plist[en] = (2u * b.n_bins + q) | (b.page_seq[q] << 16);
      }
    __syncthreads();
    const uint32_t slots = poisoned ? 0u : umin(n_list, kPageList) << b.page_shift;
    splat_gather_test(b, keys, slots, [&](uint32_t v) {
      const uint32_t r = v & (S - 1u), en = v < slots ? plist[v >> b.page_shift] : 0u, page = en & 0xffffu, P = en >> 16;
      const uint32_t have = P < e ? S : (P == e ? umin(fill, S) : (P == e + 1u && fill > S ? umin(fill - S, S) : 0u));
      return v < slots && r < have ? b.records[((size_t)page << b.page_shift) + r] : SplatRec{0u, 0u, 0u};
    });
    __syncthreads();
    if(threadIdx.x == 0)
    {
      // the next call starts from zero: this bin's state word, and — once every block has read it — the pool counter
      b.state[bin] = 0ull;
      if(atomicAdd(b.rticket, 1u) == gridDim.x - 1u)
      {
        __hip_atomic_store(b.pool, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(b.rticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  else
  {
    __syncthreads();
    const uint32_t cnt = b.count[bin], off = b.offset[bin];
    splat_gather_test(b, keys, cnt, [&](uint32_t r) { return r < cnt ? b.records[off + r] : SplatRec{0u, 0u, 0u}; });
    __syncthreads();
    if(threadIdx.x == 0) b.count[bin] = 0u;   // the next call counts from zero
  }
  const uint32_t ox = (bin % b.bins_x) * kBinW, oy = (bin / b.bins_x) * kBinH;
  // the colour gather is a dependent random 16-B read per covered pixel: four of them in flight per lane
  constexpr uint32_t kU = 4;
  for(uint32_t k0 = threadIdx.x; k0 < kBinW * kBinH; k0 += kU * blockDim.x)
  {
    unsigned long long key[kU];
    float4 c[kU];
#pragma unroll
    for(uint32_t u = 0; u < kU; ++u)
    {
      const uint32_t k = k0 + u * blockDim.x;
      key[u] = k < kBinW * kBinH ? keys[k] : kSplatClear;
    }
#pragma unroll
    for(uint32_t u = 0; u < kU; ++u)
    {
      c[u] = clear;
      if(key[u] != kSplatClear && !TRT_SKIP(b, 16u))
      {
        const float4 pc = reinterpret_cast<const float4*>(pts)[2 * (size_t)(uint32_t)key[u] + 1];
        c[u] = make_float4(pc.x, pc.y, pc.z, 1.0f);   // o_color = vec4(current.color.xyz, 1.0)  (frag_shader.frag:44)
      }
    }
#pragma unroll
    for(uint32_t u = 0; u < kU; ++u)
    {
      const uint32_t k = k0 + u * blockDim.x;
      const uint32_t x = ox + (k % kBinW), y = oy + (k / kBinW);
      if(k < kBinW * kBinH && x < a.W && y < a.H)
        rgba[(size_t)y * a.W + x] = c[u];
    }
  }
}

__global__ __launch_bounds__(256) void splat_resolve_kernel(const unsigned long long* __restrict__ keys, uint64_t n,
                                                            const trt_point* __restrict__ pts, float4 clear, float4* rgba)
{
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
  {
    const unsigned long long k = keys[i];
    float4 c = clear;
    if(k != kSplatClear)
    {
      const float4 pc = reinterpret_cast<const float4*>(pts)[2 * (size_t)(uint32_t)k + 1];
      c = make_float4(pc.x, pc.y, pc.z, 1.0f);   // o_color = vec4(current.color.xyz, 1.0)  (frag_shader.frag:44)
    }
    rgba[i] = c;
  }
}

SplatPlan splat_plan(uint32_t W, uint32_t H, float point_size, uint64_t n_points, const Tuning& tn)
{
  SplatPlan pl{};
  const uint64_t nb = (uint64_t)((W + kBinW - 1) / kBinW) * ((H + kBinH - 1) / kBinH), np = n_points ? n_points : 1;
  auto al = [](uint64_t v) { return (size_t)((v + 15) & ~(uint64_t)15); };
  // the one-pass form: images or points beyond what a record can say, or more than 8 GiB of records
  if(tn.splat_variant == kSplatOnePass || nb > kSplatMaxBins || W > kSplatMaxDim || H > kSplatMaxDim || !(point_size <= 32.0f) ||
     4 * n_points > 0xffffffffull || np * (4 * kSplatRecordSize + 8) > ((uint64_t)8 << 30))
    return pl;
  pl.n_bins = (uint32_t)nb;
  pl.mode   = nb <= kSortBins ? kSplatPaged : kSplatDirect;
  if(tn.splat_variant == kSplatSorted && nb <= kSortBins) pl.mode = kSplatSorted;
  if(tn.splat_variant == kSplatDirect) pl.mode = kSplatDirect;
  if(pl.mode == kSplatPaged)
  {
    // Page size S: at least 4,096 records (a chunk's run for a bin is at most 4,096 long: it spans at most two pages, the
    // window of splat_bin_kernel) and large enough that the worst case (4 records per point) fills at most 2,048 pool pages:
    // an evenly spread cloud then leaves a bin in its own two pages or one rotation beyond (8.4 M points, 512 bins: S =
    // 16,384 against 16 k records per bin), and `resolve` picks a bin's pages out of a few thousand notes.  Every bin owns
    // two pages; a bin leaves less than one pool page unfilled and holds one more handed out ahead, so the pool never runs
    // dry with 4n/S + 2·n_bins + 2 pages.  (S = 4,096 for that cloud: the same on spread clouds, 4-5x slower on one that
    // fills a third of the view — a page end every 16 µs per bin is more than the rotations keep up with.)
    uint32_t shift = 12;
    while(shift < 19 && ((4 * np) >> shift) > 2048u) ++shift;
    // … and a window (2·S) that takes what one round of resident blocks (512 x 4,096 points) brings a bin four times
    // more crowded than the average in one burst: below that the adders of a moderately crowded bin wait for rotations
    // (2 M points over a third of the view, S = 4,096: 0.138 against 0.082 ms)
    const uint64_t burst = np < ((uint64_t)1 << 21) ? np : ((uint64_t)1 << 21);
    while(shift < 19 && ((uint64_t)1 << shift) * nb < 4 * burst) ++shift;
#ifdef TRT_TUNING
    if(const char* e = getenv("TRT_SPLAT_PAGE_SHIFT")) shift = (uint32_t)atoi(e);
#endif
    const uint64_t pool = ((4 * np) >> shift) + 2 * nb + 2, slots = (2 * nb + pool) << shift;
    if(slots <= 0xffffffffull && ((4 * np) >> shift) <= 2048u && 2 * nb + pool < 65536u && slots * kSplatRecordSize <= ((uint64_t)8 << 30))
    {
      pl.page_shift = shift; pl.pool_pages = (uint32_t)pool;
      pl.rec_bytes = al(slots * kSplatRecordSize); pl.pagebin_bytes = al(pool * sizeof(uint32_t)) * 2;   // page_bin + page_seq
      return pl;
    }
    pl.mode = kSplatSorted;   // (clouds beyond what the page scheme addresses, or whose pages would take more than 8 GiB: the two-pass form)
  }
  pl.rec_bytes  = al(np * 4 * kSplatRecordSize);
  pl.proj_bytes = al(np * 8);
  if(pl.mode == kSplatSorted) pl.table_bytes = al((np / kSortChunk + 4) * nb * sizeof(uint32_t));
  return pl;
}

namespace {
// The bins the LDS arrays of a splat_bin_kernel / splat_scatter_sorted_kernel block hold: f(integral_constant<NB>).
template <class F>
void with_sort_bins(uint32_t n_bins, F&& f)
{
  if(n_bins <= 512u) f(std::integral_constant<uint32_t, 512>{});
  else f(std::integral_constant<uint32_t, kSortBins>{});
}
}  // namespace

hipError_t launch_splat(const trt_point* pts, uint64_t n_points, const float* vp, uint32_t W, uint32_t H,
                        const float* clear, float point_size, const SplatScratch& sc, float* rgba, int n_cus,
                        const Tuning& tn, hipStream_t stream)
{
  SplatArgs a;
  for(int i = 0; i < 16; ++i) a.vp[i] = vp[i];
  a.W = W; a.H = H; a.half = point_size * 0.5f;
  const SplatPlan& pl = sc.plan;
  if(pl.mode != kSplatOnePass)
  {
    SplatBins b{};
    b.bins_x = (W + kBinW - 1) / kBinW; b.bins_y = (H + kBinH - 1) / kBinH; b.n_bins = pl.n_bins;
    // fixed layout whatever n_bins is: the count words of one call never alias another call's offsets
    b.count   = sc.bin_words + kSplatCountWord;
    b.offset  = sc.bin_words + kSplatOffsetWord;
    b.cursor  = sc.bin_words + kSplatCursorWord;
    b.state   = reinterpret_cast<unsigned long long*>(sc.bin_words + kSplatStateWord);
    b.ticket  = sc.bin_words + kSplatTicketWord;
    b.pool    = sc.bin_words + kSplatPoolWord;
    b.rticket = sc.bin_words + kSplatRTicketWord;
    char* base = static_cast<char*>(sc.records);
    b.records  = reinterpret_cast<SplatRec*>(base);
    b.proj     = reinterpret_cast<uint2*>(base + pl.proj_at());
    b.table    = pl.mode == kSplatSorted ? reinterpret_cast<uint32_t*>(base + pl.table_at()) : nullptr;
    b.page_bin = reinterpret_cast<uint32_t*>(base + pl.pagebin_at());
    b.page_seq = b.page_bin + pl.pagebin_bytes / 2 / sizeof(uint32_t);
    b.page_shift = pl.page_shift; b.pool_pages = pl.pool_pages;
    b.debug_skip = tn.debug_skip;   // always 0 in the release build
    const dim3 rgrid(pl.n_bins), rblock(kSplatResolveThreads);
    const float4 cl = make_float4(clear[0], clear[1], clear[2], clear[3]);
    if(pl.mode == kSplatPaged)
    {
      if(n_points)
      {
        const uint32_t schunks = (uint32_t)((n_points + kSortChunk - 1) / kSortChunk);
        // two blocks per CU are resident (64-80 KB of LDS each): that many blocks, each walking its share of the chunks
        uint32_t bgrid = (uint32_t)n_cus * 2u;
        if(tn.splat_blocks_per_cu) bgrid = (uint32_t)(n_cus * tn.splat_blocks_per_cu);
        if(bgrid == 0u || bgrid > schunks) bgrid = schunks;
        with_sort_bins(pl.n_bins, [&](auto nb) {
          hipLaunchKernelGGL(splat_bin_kernel<decltype(nb)::value>, dim3(bgrid), dim3(kSortThreads), 0, stream, pts, n_points, a, b);
        });
      }
      hipLaunchKernelGGL(splat_resolve_bins_kernel<true>, rgrid, rblock, 0, stream, pts, a, b, cl, reinterpret_cast<float4*>(rgba));
      return hipGetLastError();
    }
    if(n_points)
    {
      const uint32_t chunks = (uint32_t)((n_points + kSplatChunk - 1) / kSplatChunk), schunks = (uint32_t)((n_points + kSortChunk - 1) / kSortChunk);
      if(b.table)   // sorted scatter, two passes (-DTRT_TUNING builds: TRT_SPLAT_VARIANT=1)
      {
        hipLaunchKernelGGL((splat_count_kernel<kSortChunk, 4, true>), dim3((schunks + 3) / 4), dim3(1024), 4 * pl.n_bins * sizeof(uint32_t), stream, pts, n_points, a, b);
        with_sort_bins(pl.n_bins, [&](auto nb) {
          hipLaunchKernelGGL(splat_scatter_sorted_kernel<decltype(nb)::value>, dim3(schunks), dim3(kSortThreads), 0, stream, n_points, b);
        });
      }
      else
      {
        hipLaunchKernelGGL((splat_count_kernel<kSplatChunk, 1, false>), dim3(chunks), dim3(256), pl.n_bins * sizeof(uint32_t), stream, pts, n_points, a, b);
        hipLaunchKernelGGL(splat_scatter_kernel, dim3(chunks), dim3(kDirectThreads), 2 * pl.n_bins * sizeof(uint32_t), stream, n_points, b);
      }
    }
    hipLaunchKernelGGL(splat_resolve_bins_kernel<false>, rgrid, rblock, 0, stream, pts, a, b, cl, reinterpret_cast<float4*>(rgba));
    return hipGetLastError();
  }
  unsigned long long* keys = sc.keys;
  uint64_t npx = (uint64_t)W * H, cap = (uint64_t)n_cus * 16;
  if(tn.splat_blocks_per_cu) cap = (uint64_t)n_cus * tn.splat_blocks_per_cu;
  if(cap == 0) cap = 1;
  auto grid = [&](uint64_t n) { const uint64_t w = (n + 255) / 256; return dim3((uint32_t)(w < cap ? (w ? w : 1) : cap)); };
  hipLaunchKernelGGL(splat_clear_kernel, grid(npx), dim3(256), 0, stream, keys, npx);
  if(n_points)
    hipLaunchKernelGGL(splat_points_kernel, grid(n_points), dim3(256), 0, stream, pts, n_points, a, keys);
  hipLaunchKernelGGL(splat_resolve_kernel, grid(npx), dim3(256), 0, stream, keys, npx, pts,
                     make_float4(clear[0], clear[1], clear[2], clear[3]), reinterpret_cast<float4*>(rgba));
  return hipGetLastError();
}

}  // namespace trt
