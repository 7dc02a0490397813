// trt_splat.hpp — launch interface between the C ABI (trt_api.hip) and the point-cloud re-projection (trt_splat.hip).
// Host-side only types, as in trt_kernels.hpp.
#pragma once

#include "trt_kernels.hpp"

namespace trt {

// ---- The contract between the host (trt_api.hip) and the re-projection kernels (trt_splat.hip) ------------------------
// Every layout both sides index is stated here once.

// The re-projection's bin words (SplatScratch::bin_words), laid out for the largest bin count whatever a call uses.
constexpr uint32_t kSplatMaxBins     = 8192;
constexpr size_t   kSplatCountWord   = 0;                  // per bin: records (zero between calls)
constexpr size_t   kSplatOffsetWord  = kSplatMaxBins;      // per bin: first record
constexpr size_t   kSplatCursorWord  = 2 * kSplatMaxBins;  // per bin: scatter cursor
constexpr size_t   kSplatStateWord   = 3 * kSplatMaxBins;  // per bin: 64-bit page state (two words)
constexpr size_t   kSplatTicketWord  = 5 * kSplatMaxBins;  // blocks of `count` that have finished (zero between calls)
constexpr size_t   kSplatPoolWord    = kSplatTicketWord + 1;
constexpr size_t   kSplatRTicketWord = kSplatTicketWord + 2;
constexpr size_t   kSplatBinWords    = kSplatTicketWord + 64;   // + the ticket, pool and rticket words and a reserved tail
static_assert(kSplatStateWord % 2 == 0, "the page state is 64-bit");

// Scratch of the re-projection: the binned form (mode != 0: kSplatBinWords zero-initialised words + the 12-B records of
// the mode, splat_plan) or the one-pass form (keys: W·H 64-bit words).
constexpr size_t kSplatRecordSize = 12;
enum SplatMode { kSplatOnePass = 0, kSplatSorted = 1, kSplatDirect = 2, kSplatPaged = 3 };
// What a call needs (splat_plan): the form it takes and the bytes of ctx scratch behind `records`, laid out as
// [records | proj | table | page_bin], every part 16-byte aligned.
struct SplatPlan {
  int      mode;        // SplatMode
  uint32_t n_bins;
  uint32_t page_shift;  // paged: a page holds 1 << page_shift records
  uint32_t pool_pages;  // paged: pages behind the bins' first pages
  size_t   rec_bytes, proj_bytes, table_bytes, pagebin_bytes;
  size_t   proj_at() const { return rec_bytes; }   // byte offsets of the parts behind `records`, in the order above
  size_t   table_at() const { return proj_at() + proj_bytes; }
  size_t   pagebin_at() const { return table_at() + table_bytes; }   // page_bin, then page_seq: half of pagebin_bytes each
  size_t   total() const { return pagebin_at() + pagebin_bytes; }
};
struct SplatScratch {
  SplatPlan           plan;
  uint32_t*           bin_words;
  void*               records;   // plan.total() bytes
  unsigned long long* keys;
};
SplatPlan  splat_plan(uint32_t W, uint32_t H, float point_size, uint64_t n_points, const Tuning& tn);
hipError_t launch_splat(const trt_point* pts, uint64_t n_points, const float* vp, uint32_t W, uint32_t H,
                        const float* clear, float point_size, const SplatScratch& sc, float* rgba, int n_cus,
                        const Tuning& tn, hipStream_t stream);

}  // namespace trt
