// trt_cloud.hpp — launch interface between the C ABI (trt_api.hip) and the capture → point-cloud kernels (trt_cloud.hip).
// Host-side only types, as in trt_kernels.hpp.
#pragma once

#include "trt_kernels.hpp"

namespace trt {

// ---- The contract between the host (trt_api.hip) and the cloud kernels (trt_cloud.hip) -------------------------------
// Every layout both sides index is stated here once.

// A chunk: the records one block of the count and of the scatter pass owns (kCloudThreads lanes × kCloudPerLane records,
// record i of the chunk on lane i % kCloudThreads).  The Python side states the same number (abi.TRT_CLOUD_CHUNK): the
// tests straddle it.
constexpr uint32_t kCloudThreads = 256;
constexpr uint32_t kCloudPerLane = 4;
constexpr uint32_t kCloudChunk   = kCloudThreads * kCloudPerLane;   // 1024 records
constexpr uint64_t cloud_chunks(uint64_t n_records) { return (n_records + kCloudChunk - 1) / kCloudChunk; }

// ctx scratch of trt_cloud_dev (trt_ctx::d_cloud): a header of 64-bit words, then one 32-bit word per chunk.  No word
// carries anything from one call to the next — every call writes what it reads — so eager calls and graph replays mix.
//   header[kCloudStart]  first point this call writes (0, or counts_dev[0] as cloud_plan_kernel found it: append)
//   table[c]             COMPACT only: after the count pass the records of chunk c that are kept; after cloud_plan_kernel
//                        the kept records of the chunks before c (exclusive prefix; < 2^32 as n_records is)
enum CloudWord : uint32_t { kCloudStart = 0, kCloudHeaderWords = 8 };
constexpr size_t cloud_scratch_bytes(uint64_t n_records, int mode)
{
  return kCloudHeaderWords * sizeof(uint64_t) + (mode == TRT_CLOUD_COMPACT ? (size_t)cloud_chunks(n_records) * sizeof(uint32_t) : 0);
}

struct CloudArgs {
  const trt_rendered_data* rendered;   // n_records records, buffer order
  uint64_t                 n_records;  // <= 0xffffffff
  int                      mode;       // TRT_CLOUD_*
  int                      append;
  trt_point*               points;     // capacity points: nothing is written at or beyond it
  uint64_t                 capacity;
  uint64_t*                counts;     // counts_dev of the ABI: [0] points in the buffer, [1] points wanted
  uint64_t*                header;     // scratch, CloudWord
  uint32_t*                table;      // scratch behind the header: cloud_chunks(n_records) words (COMPACT)
};
// Kernel nodes only: [count pass (COMPACT)] → plan (one block) → stream (KEEP_ALL / MARK_MISSES) or scatter (COMPACT).
hipError_t launch_cloud(const CloudArgs& a, hipStream_t stream);

}  // namespace trt
