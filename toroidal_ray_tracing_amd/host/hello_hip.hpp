// hello_hip.hpp — C++ host-side mirror of the reference's sample class for the ray-tracing path.
//
// The reference drives its ray tracer through `class HelloVulkan`
// (vk_raytracing_tutorial_KHR/ray_tracing_reflections/hello_vulkan.h:37-163,
//  ray_tracing__before/hello_vulkan.h): main() calls updateUniformBuffer(), raytrace(cmdBuf,
// clearColor) and — when saving — copyRenderedPosition()/copyColorImage() followed by
// writeRenderedPosition()/writeRenderedRays()/writeColorImage().  `HelloHip` keeps those
// names, argument meanings and member names (m_pcRaster, m_pcRay, m_size) for exactly that
// subset, with the Vulkan objects replaced by a trt_ctx and HIP buffers; a command buffer
// becomes a HIP stream.  Everything else of HelloVulkan (swapchain, raster pipeline, OBJ
// loading, BLAS/TLAS, SBT, post pass, ImGui) is out of scope.
//
// Scene: the TLAS of triangle instances is replaced by analytic tori (`addTorus`), materials
// keep the WaveFrontMaterial layout (`addMaterial`).
#pragma once

#include <array>
#include <string>
#include <vector>

#include "../../include/trt.h"

struct PushConstantRaster  // ray_tracing__before/shaders/host_device.h:78-86 (light state only)
{
  float lightPosition[3]{10.f, 15.f, 8.f};  // hello_vulkan.h:74-80
  float lightIntensity{100.f};
  int   lightType{0};
};

class HelloHip
{
public:
  struct Extent { uint32_t width{0}, height{0}; };

  // --- set-up (replaces setup()/createOffscreenRender()/createRtDescriptorSet()) ----------
  void setup(int device = 0);                          // creates the trt_ctx; throws std::runtime_error
  void createOffscreenRender(uint32_t w, uint32_t h);  // rgba32f image + RenderedData buffer on the device
  int  addMaterial(const trt_material& m);             // returns the material index
  void addTorus(const float center[3], float R, float r, int matId);
  // Axis of symmetry of every torus added so far (trt_set_torus_axes): 3 floats per torus in addTorus order, any
  // non-zero length — the rotation part of the instance transform loadModel(filename, transform) takes in the
  // reference.  nullptr: every torus turns about +y again.  Call it after the last addTorus.
  void setTorusAxes(const float* axes);
  void destroyResources();
  ~HelloHip() { destroyResources(); }

  // --- camera (CameraManip.setLookat + updateUniformBuffer, hello_vulkan.cpp:57-98) --------
  void setLookat(const std::array<float, 3>& eye, const std::array<float, 3>& center,
                 const std::array<float, 3>& up, float fovDegrees = 60.f);
  void updateUniformBuffer();  // viewProj / viewInverse / projInverse / center → m_globals

  // --- the path ------------------------------------------------------------------------------
  // HelloVulkan::raytrace(cmdBuf, clearColor), hello_vulkan.cpp:913-935 / 936-958: refresh the
  // push constants from m_pcRaster and clearColor, then launch width × height rays.
  void raytrace(void* stream, const std::array<float, 4>& clearColor);

  // The shadow query on its own (traceRayEXT with gl_RayFlagsTerminateOnFirstHitEXT, REFL/shaders/raytrace.rchit:114-131)
  // against the tori added so far: device streams in, one byte and / or one mask bit per ray out (trt_occluded_dev).
  void occluded(void* stream, const trt_rays& raysDev, const float* tmaxPerRayDev, float tmin, float tmax,
                uint8_t* flagDev, uint64_t* maskDev);

  // The payload loop on caller-supplied rays with translucent surfaces (trt_shade_through_dev): the push constants are
  // refreshed as raytrace() refreshes them, then every ray of raysDev (sample-major, `samples` per output) is composited
  // front to back through the tori added so far, a material's `dissolve` being its opacity — a material added with
  // dissolve 0 is invisible here.  rgbaDev: (raysDev.n / samples) * 4 floats, 16-byte aligned.
  void shadeThrough(void* stream, const std::array<float, 4>& clearColor, const trt_rays& raysDev, uint32_t samples, float* rgbaDev);

  // Glass tori (trt_shade_refract_dev, trt_shade_refract_camera_dev): a material added with illum 6 or 7 refracts by its
  // `ior` and filters by its `transmittance` — give it an ior > 0, a zero-initialised glass material is refused.  The push
  // constants are refreshed as raytrace() refreshes them.  shadeRefract: every ray of raysDev (sample-major, `samples` per
  // output) into rgbaDev ((raysDev.n / samples) * 4 floats, 16-byte aligned).  raytraceRefract: the frame of m_camera into
  // the colour image raytrace() writes, `samples` rays per pixel at the sub-pixel offsets (2 floats per sample; nullptr:
  // the pixel centres); no RenderedData is written.
  void shadeRefract(void* stream, const std::array<float, 4>& clearColor, const trt_rays& raysDev, uint32_t samples, float* rgbaDev);
  void raytraceRefract(void* stream, const std::array<float, 4>& clearColor, uint32_t samples = 1, const float* offsets = nullptr);

  // Several lights and area lights (trt_shade_lit_dev, trt_shade_lit_camera_dev): the light of the push constants is
  // replaced by `lights` (host memory: the table, K = shadow_samples and the K x 2 disc positions of the area lights; see
  // include/trt.h).  Only the clear colour of the push constants is refreshed.  shadeLit: every ray of raysDev
  // (sample-major, `samples` per output) into rgbaDev ((raysDev.n / samples) * 4 floats, 16-byte aligned).  raytraceLit:
  // the frame of m_camera into the colour image raytrace() writes, `samples` rays per pixel at the sub-pixel offsets
  // (2 floats per sample; nullptr: the pixel centres); no RenderedData is written.
  void shadeLit(void* stream, const std::array<float, 4>& clearColor, const trt_lights& lights, const trt_rays& raysDev, uint32_t samples,
                float* rgbaDev);
  void raytraceLit(void* stream, const std::array<float, 4>& clearColor, const trt_lights& lights, uint32_t samples = 1,
                   const float* offsets = nullptr);

  // Textures on the tori (trt_set_textures, trt_shade_textured_dev, trt_shade_textured_camera_dev): the role of
  // createTextureImages() and of `diffuse *= texture(...)` in the closest-hit shader (REFL/shaders/raytrace.rchit:101-106).
  // setTextures: n host images (RGBA8, copied to the device; nullptr / 0 unbinds); a material added with textureId = k >= 0
  // then takes texture k at the (u, v) of a hit — the angle about the torus' axis, the angle about its tube.  The push
  // constants are refreshed as raytrace() refreshes them.  shadeTextured: every ray of raysDev (sample-major, `samples` per
  // output) into rgbaDev ((raysDev.n / samples) * 4 floats, 16-byte aligned).  raytraceTextured: the frame of m_camera into
  // the colour image raytrace() writes, `samples` rays per pixel at the sub-pixel offsets (2 floats per sample; nullptr:
  // the pixel centres), which filter the texture as they do edges; no RenderedData is written.  raytrace() itself refuses
  // a scene with a textured material.
  void setTextures(const trt_texture* textures, uint32_t n);
  void shadeTextured(void* stream, const std::array<float, 4>& clearColor, const trt_rays& raysDev, uint32_t samples, float* rgbaDev);
  void raytraceTextured(void* stream, const std::array<float, 4>& clearColor, uint32_t samples = 1, const float* offsets = nullptr);

  // Lights, textures and glass at once (trt_shade_scene_dev, trt_shade_scene_camera_dev): the table of shadeLit — or
  // nullptr for the light of the push constants, refreshed as raytrace() refreshes it —, the textures of setTextures and
  // the glass materials of shadeRefract in one call; flags: 0, or TRT_SCENE_GLASS_SHADOWS to let light through glass in
  // the shadow query, filtered by the glass' transmittance (include/trt.h).  shadeScene: every ray of raysDev
  // (sample-major, `samples` per output) into rgbaDev ((raysDev.n / samples) * 4 floats, 16-byte aligned).  raytraceScene:
  // the frame of m_camera into the colour image raytrace() writes, `samples` rays per pixel at the sub-pixel offsets
  // (2 floats per sample; nullptr: the pixel centres); no RenderedData is written.
  void shadeScene(void* stream, const std::array<float, 4>& clearColor, const trt_lights* lights, uint32_t flags, const trt_rays& raysDev,
                  uint32_t samples, float* rgbaDev);
  void raytraceScene(void* stream, const std::array<float, 4>& clearColor, const trt_lights* lights, uint32_t flags, uint32_t samples = 1,
                     const float* offsets = nullptr);

  // Media inside the tubes of the tori added so far (trt_chords_dev, trt_glow_dev; materials are not read).  chords: the
  // length of every ray of raysDev inside every tube, lengthDev[j * raysDev.n + i] for torus j (the order of the
  // addTorus calls).  glow: emission and absorption of media (one trt_medium per torus, host memory) integrated along
  // every ray; rgbaDev: raysDev.n * 4 floats, 16-byte aligned, (radiance rgb, transmittance left) per ray — composite
  // L + T * behind.  Ray i ends at min(tmaxPerRayDev[i], tmax), or at tmax if tmaxPerRayDev is null.
  void chords(void* stream, const trt_rays& raysDev, const float* tmaxPerRayDev, float tmin, float tmax, float* lengthDev);
  void glow(void* stream, const trt_rays& raysDev, const float* tmaxPerRayDev, const trt_medium* media, float tmin, float tmax,
            float* rgbaDev);
  // glow with media that vary across the tubes (trt_glow_profile_dev): one trt_profile per torus (host memory), a table of
  // emission and sigma over x = rho^2 / r^2 (0: the tube's axis, 1: its wall); every piece of a ray inside the tubes is
  // integrated in `steps` sub-steps (1..TRT_MAX_GLOW_STEPS).  rgbaDev as glow's.
  void glowProfile(void* stream, const trt_rays& raysDev, const float* tmaxPerRayDev, const trt_profile* profiles, uint32_t steps,
                   float tmin, float tmax, float* rgbaDev);
  // The response of every ray to every knot of such a table (trt_glow_weights_dev): weightDev holds n_tori * 17 * n floats,
  // the weight of knot k of torus j on ray i at [(j * TRT_PROFILE_KNOTS + k) * n + i]; without absorption glowProfile's
  // L_c is the sum of weight * knot[k][c].  Every interval of chords() is integrated in `steps` sub-steps.
  void glowWeights(void* stream, const trt_rays& raysDev, const float* tmaxPerRayDev, uint32_t steps, float tmin, float tmax,
                   float* weightDev);
  // The same response behind media that absorb (trt_glow_weights_absorbed_dev): glowProfile's tables, of which only sigma is
  // read; every deposit is weighted by the transmittance in front of it, so that glowProfile's L_c is the sum of
  // weight * knot[k][c] over tori and knots with any sigma.  transDev: the transmittance left per ray, or nullptr.
  void glowWeightsAbsorbed(void* stream, const trt_rays& raysDev, const float* tmaxPerRayDev, const trt_profile* profiles,
                           uint32_t steps, float tmin, float tmax, float* weightDev, float* transDev);
  // That matrix applied on the device, never stored (trt_glow_project_dev, trt_glow_backproject_dev).  glowProject: W x
  // with the emission channels of `profiles` as x, summed in FP64 and rounded once; rgbaDev as glow's, its T the
  // transmittance left.  glowBackproject: yDev (n * 4 floats, the layout of rgbaDev; channel 3 is not read) to backDev,
  // n_tori * 17 * 4 doubles: W^T y in channels 0..2 and the column sums in channel 3; profiles may be nullptr (no absorption).
  // The adjoint keeps partial sums in scratch of the context: make one eager call before capturing it.
  void glowProject(void* stream, const trt_rays& raysDev, const float* tmaxPerRayDev, const trt_profile* profiles, uint32_t steps,
                   float tmin, float tmax, float* rgbaDev);
  void glowBackproject(void* stream, const trt_rays& raysDev, const float* tmaxPerRayDev, const trt_profile* profiles, uint32_t steps,
                       float tmin, float tmax, const float* yDev, double* backDev);
  // The derivative of glowProject's map with respect to all four channels of the tables, at `profiles`
  // (trt_glow_tangent_dev, trt_glow_adjoint_dev).  glowTangent: J delta per ray, (dL_r, dL_g, dL_b, dT) in rgbaDev; delta of
  // any sign.  glowAdjoint: J^T y in gradDev, n_tori * 17 * 4 doubles in the layout of the tables; ALL four channels of yDev
  // are read (glowBackproject ignores the fourth).  Both use scratch of the context: make one eager call before capturing.
  void glowTangent(void* stream, const trt_rays& raysDev, const float* tmaxPerRayDev, const trt_profile* profiles, const trt_profile* delta,
                   uint32_t steps, float tmin, float tmax, float* rgbaDev);
  void glowAdjoint(void* stream, const trt_rays& raysDev, const float* tmaxPerRayDev, const trt_profile* profiles, uint32_t steps,
                   float tmin, float tmax, const float* yDev, double* gradDev);

  // Ambient occlusion on the record raytrace-style calls leave on the device (trt_fan_occluded_dev): from each of the n points
  // of atDev, `samples` any-hit rays with the directions dirs (samples x 3 host floats; frame TRT_FAN_LOCAL: about the
  // point's normal) against the tori added so far; one word of bits and / or the share of clear samples per point out.
  void fanOccluded(void* stream, const trt_hits& atDev, uint64_t n, int frame, uint32_t samples, const float* dirs, float tmin,
                   float tmax, uint64_t* bitsDev, float* openDev);

  // --- readback + text dumps (ray_tracing__before/hello_vulkan.cpp:991-1259) ----------------
  void copyRenderedPosition(void* stream);  // RenderedData device → host
  void copyColorImage(void* stream);        // rgba32f image device → host
  void writeRenderedPosition(const char* dir);  // dir + "data/renderedPosition<rho>.txt": "x y z\n", index x*H+y
  void writeRenderedRays(const char* dir);      // dir + "data/origins.txt", "data/directions.txt"
  void writeColorImage(const char* dir);        // dir + "data/renderedColor<rho>.txt": row-major "r g b\n"
  // the same dump under an explicit name — ray_tracing__before_second/hello_vulkan.cpp:781-825 writes the
  // re-projected image to dir + "data/<scene>ptCloudImage_10.txt", ray_tracing_reflections/…:1065-1110 the
  // ground truth to dir + "data/<scene>gTruth.txt": one "r g b\n" line per pixel, row-major
  void writeColorImageAs(const std::string& path);

  // --- post pass (drawPost, ray_tracing_reflections/hello_vulkan.cpp:560-579 + post.frag) ------
  void drawPost(void* stream);              // tonemap m_dColor -> 8-bit image (pow(c, 1/2.2))
  void copyPostImage(void* stream);         // device -> host
  const std::vector<uint8_t>& postImage() const { return m_hostPost; }
  // The presented image as a file: binary PPM (P6, 8-bit RGB) of the tonemapped frame — what the swapchain
  // shows after post.frag (REFL/shaders/post.frag:33-37); call drawPost() + copyPostImage() first.
  void writePostImagePPM(const std::string& path) const;

  // --- point-cloud re-projection (ray_tracing__before_second) -------------------------------
  // loadPoints (SEC/hello_vulkan.cpp:496-628): "x y z" per line, "-nan" -> numeric_limits<float>::lowest()
  void loadPoints(const std::string& positionFile, const std::string& colorFile);
  void createCloudDataBuffer();             // :633-660 — throws if the two files disagree in length
  void rasterize(void* stream, const std::array<float, 4>& clearColor);  // :313-330, POINT_LIST draw into m_dColor
  // The same cloud built on the device from the capture raytrace() left in the RenderedData buffer (trt_cloud_dev): no
  // text files, no host round trip, any width and height.  mode: TRT_CLOUD_KEEP_ALL (what the text path builds, exactly
  // instead of to six digits) | TRT_CLOUD_MARK_MISSES | TRT_CLOUD_COMPACT.  append: behind the points already there, so
  // the captures of a rho sweep make one cloud — call reserveCloud() first with room for all of them (without it the
  // cloud holds one capture; what does not fit is dropped and wantedPoints() tells).  Only enqueues on `stream`.
  void   reserveCloud(size_t capacity);
  void   createCloudDataBufferFromCapture(int mode = TRT_CLOUD_COMPACT, bool append = false, void* stream = nullptr);
  size_t numPoints() const;      // either path; after the device path it waits for the stream and reads the count back
  size_t wantedPoints() const;   // device path: points the calls wanted to store (> numPoints(): the reserve was too small)

  // --- state, named as in the reference -----------------------------------------------------
  PushConstantRaster m_pcRaster;
  trt_push           m_pcRay{{0, 0, 0, 0}, {0, 0, 0}, 0.f, 0, 10, 0.f};  // maxDepth 10 (hello_vulkan.h:157)
  Extent             m_size;
  int                m_camera{TRT_CAMERA_PINHOLE};  // REFL: pinhole; BEF: TRT_CAMERA_TOROIDAL
  trt_globals        m_globals{};

  const std::vector<float>&             colorImage() const { return m_hostColor; }
  const std::vector<trt_rendered_data>& renderedData() const { return m_hostRendered; }
  trt_ctx*                              ctx() const { return m_ctx; }

private:
  void check(int rc, const char* what) const;
  // m_pcRay with the clear colour and — withLight — the light state of m_pcRaster (hello_vulkan.cpp:917-920)
  const trt_push* pushFor(const std::array<float, 4>& clearColor, bool withLight);
  trt_scene       scene() const;   // the tori and materials added so far

  trt_ctx*                   m_ctx{nullptr};
  int                        m_device{0};
  std::vector<trt_torus>     m_tori;
  std::vector<trt_material>  m_materials;
  std::array<float, 3>       m_eye{0, 0, 0}, m_center{10, 0, 0}, m_up{0, 1, 0};  // main.cpp:95
  float                      m_fov{60.f};
  float*                     m_dColor{nullptr};
  trt_rendered_data*         m_dRendered{nullptr};
  std::vector<float>             m_hostColor;
  std::vector<trt_rendered_data> m_hostRendered;
  uint8_t*                       m_dPost{nullptr};
  std::vector<uint8_t>           m_hostPost;
  std::vector<std::array<float, 3>> m_positions, m_colors;   // SEC: m_positions / m_colors
  std::vector<trt_point>         m_cloudData;                // SEC: m_cloudData
  trt_point*                     m_dCloud{nullptr};
  size_t                         m_cloudCapacity{0};         // points m_dCloud has room for
  uint64_t*                      m_dCloudCounts{nullptr};    // counts_dev of trt_cloud_dev
  bool                           m_cloudFromCapture{false};  // m_dCloud was built by createCloudDataBufferFromCapture
  void*                          m_cloudStream{nullptr};     // … on this stream
};
