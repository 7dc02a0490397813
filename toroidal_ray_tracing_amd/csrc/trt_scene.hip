// trt_scene.hip — lights, textures and glass in one payload loop (trt_shade_scene*, trt_shade_scene_camera*), gfx950.
//
//   FilteredShadow   the shadow stage of lit_hit (trt_hits.hpp) whose rays pass through the tori of `clear` — the glass
//                    tori under TRT_SCENE_GLASS_SHADOWS, none without it — filtered by their transmittance: the visibility
//                    is a sum of filters per channel where OpaqueShadow's is a count
//   SceneHit         the hit step: LitHit's begin / light / end with the texel of the hit (with_texel) in every light's
//                    diffuse term, and the dielectric (glass_step) as its glass()
//   ShadeScene       the form: shade_kernel / shade_camera_kernel (trt_render.hpp) with Glass and the textures staged into
//                    LDS — they are indexed per lane, by the torus and the material of a hit — and SceneHit
//   launch_shade_scene, launch_shade_scene_camera   the two shared launches with that form.
//
// One kernel per <float | double> × ALT × ORIENT, as for every form; what a call does not use costs it a kernel-uniform
// branch: a light table of one entry (the host writes pc's light as one, trt_kernels.hpp SceneMix), an empty Glass::mask,
// an of_mat[] of -1, clear == 0.  The lights stay in the kernel-argument segment (every index into them is kernel-uniform:
// scalar loads), and so does `clear`.
// Compiled with -ffp-contract=off like every unit: each operation below is one FP32 rounding, in the order written.
#include "trt_hits.hpp"

namespace trt {

// SceneK and the larger of the two argument structs travel in one kernel-argument segment.
static_assert(sizeof(SceneK) + sizeof(ShadeSceneCameraArgs) <= 4096 && sizeof(SceneK) + sizeof(ShadeSceneArgs) <= 4096,
              "the kernel-argument segment of the shade_scene kernels: move the disc table out of the arguments for this form only");

// ------------------------------------------------------------------------------------------
// the shadow stage that lets light through glass (include/trt.h states the rule operation for operation)
// ------------------------------------------------------------------------------------------
// One shadow ray: the filter f starts at (1, 1, 1); the tori are tested as any_hit tests them (blocked_hit, trt_device.hpp);
// one that is hit and is not in `clear` makes f = 0 and ends the query, one that is in `clear` multiplies f by its Tf, once,
// and the query goes on.  The tori passed are collected as a mask over torus ids and multiplied in afterwards, in the test
// order: one VGPR live across the solves instead of three.  With `clear` != 0 the query runs without the enclosure mask:
// "cannot be hit first" holds for the opaque tubes inside a host tube, and a clear host lets the ray on to them.
// The visibility of a light: acc = f_0, acc += f_s in table order, v = acc / (float)rays per channel — for rays == 1 that
// is f itself, and with nothing passed every f is 0 or 1, acc the integer rays - occ and v OpaqueShadow's, bit for bit.
template <class Real, bool ALT, bool ORIENT>
struct FilteredShadow {
  using Seen = v3;         // acc: the sum of the filters of a light's samples
  const Glass&   g;        // (LDS)
  const uint32_t clear;    // kernel-uniform
  __device__ __forceinline__ Seen ray(const SceneK& S, v3 P, v3 Ls, float tmax, uint32_t mask, uint32_t s, bool want, uint32_t& n_shadow,
                                      WorkCount& wc, Seen acc) const
  {
    uint32_t passed = 0u;
    const bool blocked = want && blocked_hit<Real, ALT, ORIENT>(S, P, Ls, kTMin, tmax, n_shadow, wc, clear ? 0u : mask, [&](int i) {
      const uint32_t bit = (clear >> i) & 1u;
      passed |= bit << i;
      return bit != 0u;
    });
    v3 f = {1.0f, 1.0f, 1.0f};
    if(blocked)
      f = {0.0f, 0.0f, 0.0f};
    else if(passed)
      for(int k = 0; k < S.n_tori; ++k)
      {
        const int i = S.order[k];
        if((passed >> i) & 1u)
          f = {f.x * g.tf[i][0], f.y * g.tf[i][1], f.z * g.tf[i][2]};
      }
    return s == 0u ? f : v3{acc.x + f.x, acc.y + f.y, acc.z + f.z};
  }
  __device__ __forceinline__ v3 visible(Seen acc, uint32_t rays) const
  {
    const float K = (float)rays;
    return {acc.x / K, acc.y / K, acc.z / K};
  }
};

// ------------------------------------------------------------------------------------------
// shade_scene(rays_in → one colour per output), shade_scene_camera(camera → the band of an image)
// ------------------------------------------------------------------------------------------
// What the block stages: the tables a hit indexes per lane.
struct SceneMixLds {
  Glass       g;
  TexturesLds T;
};

// The hit step: LitHit — hit_point, the table's lights, hit_mirror — with the other two forms' one step each.  The texel
// is fetched once, in tint(), BEFORE the light loop, and waits in h.diffuse, which a hit under a light table does not
// otherwise use (every light forms its own diffuse term): (1, 1, 1) for a material without a texture, whose products are
// then the factors themselves.  It is pinned there for TexturedHit's reason: nothing of the fetch but three floats is
// live across the solves of the shadow rays.
template <class Real, bool ALT, bool ORIENT>
struct SceneHit : LitHit<Real, ALT, ORIENT> {
  const SceneMixLds& M;
  const uint32_t     clear;
  __device__ __forceinline__ SceneHit(const Lights& lights, const SceneMixLds& staged, uint32_t clear_) : LitHit<Real, ALT, ORIENT>(lights), M(staged), clear(clear_) {}
  __device__ __forceinline__ void tint(const SceneK& S, int id, HitState& h) const
  {
    v3 texel = {1.0f, 1.0f, 1.0f};
    with_texel<ORIENT>(S, M.T, id, h, [&](v3 t) { texel = t; });
    asm volatile("" : "+v"(texel.x), "+v"(texel.y), "+v"(texel.z));
    h.diffuse = texel;
  }
  __device__ __forceinline__ v3 light(const SceneK& S, const HitState& h, v3 d, uint32_t skip, uint32_t inside, uint32_t& n_shadow, WorkCount& wc) const
  {
    return lit_hit<Real, ALT, ORIENT>(S, this->lt, h, d, skip, inside, n_shadow, wc, h.diffuse, FilteredShadow<Real, ALT, ORIENT>{M.g, clear});
  }
  __device__ __forceinline__ bool glass(int id, const HitState& h, v3 d, v3& attenuation, int& done, v3& nextO, v3& nextD) const
  {
    return glass_step(M.g, id, h, d, attenuation, done, nextO, nextD);
  }
};

// The form: Glass (41 words) and the textures (stage_textures) into LDS, SceneHit on them and on the lights in the arguments.
struct ShadeScene {
  using Table  = SceneMix;
  using Staged = SceneMixLds;
  template <class Args> static __device__ __forceinline__ void stage(Staged* M, const Args& a)
  {
    stage_words(&M->g, a.table.glass);
    stage_textures(&M->T, a.table.tx);
  }
  template <class Real, bool ALT, bool ORIENT, class Args>
  static __device__ __forceinline__ SceneHit<Real, ALT, ORIENT> hit(const Args& a, const Staged& M)
  {
    return SceneHit<Real, ALT, ORIENT>{a.table.lights, M, a.table.clear};
  }
};

hipError_t launch_shade_scene(const SceneK& scene, const ShadeSceneArgs& a, const Tuning& tn, hipStream_t stream) { return launch_stream_form<ShadeScene>(scene, a, tn, stream); }
hipError_t launch_shade_scene_camera(const SceneK& scene, const ShadeSceneCameraArgs& a, const Tuning& tn, hipStream_t stream) { return launch_camera_form<ShadeScene>(scene, a, tn, stream); }

}  // namespace trt
