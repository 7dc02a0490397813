// trt_post.hip — gfx950 (MI355X / CDNA4) tonemap pass of the toroidal ray tracer (trt_post_dev).
//
//   post_kernel               pow(c, 1/2.2) of REFL/shaders/post.frag:33-37 on a rendered frame, one pixel per lane:
//                             float4 in, float4 and/or UNORM8 out.
//
// Compiled with -ffp-contract=off (see trt_device.hpp for the arithmetic contract).
#include "trt_kernels.hpp"

namespace trt {

// ------------------------------------------------------------------------------------------
// post pass (tonemap): streaming, one pixel per lane, 16 B in, 16 B and/or 4 B out
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void post_pixel(float4 c, uint64_t i, float4* __restrict__ f32_out, uint32_t* __restrict__ u8_out)
{
  // the framebuffer's alpha is 1 (rgen:87) and post_gamma(1) is exactly 1 (log2_poly(1) = 0,
  // exp2_poly(0) = 1): when the whole wave sees alpha 1 the fourth pow is skipped
  const float ow = __all(c.w == 1.0f) ? 1.0f : post_gamma(c.w);
  // a wave whose 64 pixels are all grey (r = g = b: the clear colour of the baseline frame, 85 % of its pixels) computes ONE
  // pow per pixel instead of three — the same bits, post_gamma being a function of its argument alone
  const bool  grey = __all(c.x == c.y && c.y == c.z);
  const float ox = post_gamma(c.x);
  float oy = ox, oz = ox;
  if(!grey)
  {
    oy = post_gamma(c.y);
    oz = post_gamma(c.z);
  }
  const float4 o = make_float4(ox, oy, oz, ow);
  if(f32_out) f32_out[i] = o;
  if(u8_out)
  {
    // UNORM8: round-to-nearest-even of clamp(o, 0, 1)·255 (v_rndne via rintf), R in the low byte
    const uint32_t r = (uint32_t)rintf(min_(max_(o.x, 0.0f), 1.0f) * 255.0f);
    const uint32_t g = (uint32_t)rintf(min_(max_(o.y, 0.0f), 1.0f) * 255.0f);
    const uint32_t b = (uint32_t)rintf(min_(max_(o.z, 0.0f), 1.0f) * 255.0f);
    const uint32_t a = (uint32_t)rintf(min_(max_(o.w, 0.0f), 1.0f) * 255.0f);
    u8_out[i] = r | (g << 8) | (b << 16) | (a << 24);
  }
}

// (Non-temporal loads and stores here: within noise, 0.088 against 0.089 ms — the → rgba8 pass is bound by the ≈200
// VALU instructions per pixel of the exact-operation pow, → f32 takes the same time with 1.6× the bytes.)
// Four pixels per lane and trip, their loads issued together: with one 16-B load in flight per
// lane the pass was bound by memory latency (32 KB in flight per CU ≈ 2.8 TB/s of reads), not by
// the ≈55 VALU instructions per channel.
__global__ __launch_bounds__(256) void post_kernel(const float4* __restrict__ in, uint64_t n, float4* __restrict__ f32_out,
                                                   uint32_t* __restrict__ u8_out)
{
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for(; i + 3 * stride < n; i += 4 * stride)
  {
    const float4 c0 = in[i], c1 = in[i + stride], c2 = in[i + 2 * stride], c3 = in[i + 3 * stride];
    post_pixel(c0, i, f32_out, u8_out);
    post_pixel(c1, i + stride, f32_out, u8_out);
    post_pixel(c2, i + 2 * stride, f32_out, u8_out);
    post_pixel(c3, i + 3 * stride, f32_out, u8_out);
  }
  for(; i < n; i += stride)
    post_pixel(in[i], i, f32_out, u8_out);
}

hipError_t launch_post(const float* in, uint64_t n, float* f32_out, uint8_t* u8_out, int n_cus, const Tuning& tn,
                       hipStream_t stream)
{
  if(n == 0) return hipSuccess;
  // many short blocks (one pixel per lane up to 16.8 M pixels): measured 0.074 / 0.087 ms for
  // → rgba8 / → f32 at 4096² against 0.097 / 0.112 ms with 4–16 long-running blocks per CU
  uint64_t want = (n + 255) / 256, cap = (uint64_t)n_cus * 256;
  if(tn.post_blocks_per_cu) cap = (uint64_t)n_cus * tn.post_blocks_per_cu;
  if(cap == 0) cap = 1;
  hipLaunchKernelGGL(post_kernel, dim3((uint32_t)(want < cap ? want : cap)), dim3(256), 0, stream,
                     reinterpret_cast<const float4*>(in), n, reinterpret_cast<float4*>(f32_out),
                     reinterpret_cast<uint32_t*>(u8_out));
  return hipGetLastError();
}

}  // namespace trt
