// scene_mix_main.cpp — a checker-textured plastic ring under a soft key light and a coloured fill light, seen through a
// glass ring that hovers above it, through the host mirror (HelloHip::setTextures / raytraceScene: trt_set_textures,
// trt_shade_scene_camera_dev).  The picture the textured, the soft-shadow and the glass example each stop short of.
// The plastic ring (R = 1, r = 0.35, about +y) carries the 8 x 4 checker of textured_ring; the glass ring (R = 1, r = 0.125,
// ior 1.5, an amber filter) lies 0.75 above it, between it and the key light — an area light of radius 0.5 with eight shadow
// rays per hit — so its shadow falls along the crest of the plastic ring; a blue point light fills in from the side.
//   1. flags = 0: glass casts the opaque shadow every other call gives it — a dark band behind a clear ring;
//   2. TRT_SCENE_GLASS_SHADOWS: the shadow rays pass the glass, filtered by its transmittance — an amber band.
// Prints both colours for every pixel of one scanline, with nine significant digits: the text holds every bit of the floats.
// Usage: scene_mix
#include <cstdio>
#include <vector>

#include "../toroidal_ray_tracing_amd/host/hello_hip.hpp"

static const uint32_t W = 48, H = 36, ROW = 15;

int main()
{
  try
  {
    HelloHip helloVk;
    helloVk.setup(0);
    helloVk.createOffscreenRender(W, H);
    trt_material plastic{}, glass{};
    plastic.ambient[0] = plastic.ambient[1] = plastic.ambient[2] = 0.05f;
    plastic.diffuse[0] = 0.75f; plastic.diffuse[1] = 0.75f; plastic.diffuse[2] = 0.75f;
    plastic.specular[0] = plastic.specular[1] = plastic.specular[2] = 0.5f;
    plastic.shininess = 24.f; plastic.ior = 1.f; plastic.dissolve = 1.f; plastic.illum = 2;
    plastic.textureId = 0;   // texture 0 of setTextures
    glass.diffuse[0] = glass.diffuse[1] = glass.diffuse[2] = 0.05f;
    glass.specular[0] = glass.specular[1] = glass.specular[2] = 0.5f;
    glass.shininess = 64.f; glass.dissolve = 1.f; glass.illum = 7; glass.textureId = -1;
    glass.ior = 1.5f;        // (a zero-initialised material has ior == 0, which the call refuses)
    glass.transmittance[0] = 0.95f; glass.transmittance[1] = 0.8f; glass.transmittance[2] = 0.6f;
    const int   mats[2] = {helloVk.addMaterial(plastic), helloVk.addMaterial(glass)};
    const float low[3] = {0.f, 0.f, 0.f}, high[3] = {0.f, 0.75f, 0.f};
    helloVk.addTorus(low, 1.0f, 0.35f, mats[0]);
    helloVk.addTorus(high, 1.0f, 0.125f, mats[1]);

    // the checker: 8 x 4 RGBA8 texels, warm white and slate, linear bytes
    std::vector<uint8_t> texels(8 * 4 * 4);
    for(uint32_t j = 0; j < 4; ++j)
      for(uint32_t i = 0; i < 8; ++i)
      {
        const bool    light = (i + j) % 2 == 0;
        const uint8_t c[4] = {(uint8_t)(light ? 255 : 96), (uint8_t)(light ? 240 : 112), (uint8_t)(light ? 208 : 160), 255};
        for(uint32_t k = 0; k < 4; ++k) texels[(j * 8 + i) * 4 + k] = c[k];
      }
    const trt_texture checker = {texels.data(), 8, 4, 4.f, 2.f, TRT_TEX_LINEAR};
    helloVk.setTextures(&checker, 1);

    // the lights: a soft white key light above, a blue fill from the side; eight positions on the unit disc, in binary
    // fractions so that every binding holds the same bits
    const trt_light table[2] = {
        {{0.5f, 6.f, -0.5f}, 40.f, {1.f, 1.f, 1.f}, 0, 0.5f},
        {{-4.f, 2.f, -3.f}, 10.f, {0.25f, 0.5f, 1.f}, 0, 0.f},
    };
    const float disc[16] = {0.25f, 0.f, -0.25f, 0.f, 0.f, 0.25f, 0.f, -0.25f, 0.625f, 0.625f, -0.625f, 0.625f, 0.625f, -0.625f, -0.625f, -0.625f};
    const trt_lights lights = {table, 2, 8, disc};

    // the pinhole camera of textured_ring: from the eye (0, 3, -4) at the origin
    trt_globals& g = helloVk.m_globals;
    g = trt_globals{};
    g.viewProj[0] = g.viewProj[5] = g.viewProj[10] = g.viewProj[15] = 1.f;   // (not read by the ray calls)
    g.projInverse[0] = 0.6f; g.projInverse[5] = 0.45f; g.projInverse[10] = 1.f; g.projInverse[15] = 1.f;
    g.viewInverse[0] = 1.f;
    g.viewInverse[5] = 0.8f;  g.viewInverse[6] = 0.6f;
    g.viewInverse[9] = -0.6f; g.viewInverse[10] = 0.8f;
    g.viewInverse[12] = 0.f;  g.viewInverse[13] = 3.f; g.viewInverse[14] = -4.f; g.viewInverse[15] = 1.f;
    helloVk.m_camera = TRT_CAMERA_PINHOLE;
    helloVk.m_pcRay.maxDepth = 6;

    const std::array<float, 4> clearColor = {0.1f, 0.2f, 0.4f, 1.f};
    helloVk.raytraceScene(nullptr, clearColor, &lights, 0);
    helloVk.copyColorImage(nullptr);
    const std::vector<float> opaque = helloVk.colorImage();
    helloVk.raytraceScene(nullptr, clearColor, &lights, TRT_SCENE_GLASS_SHADOWS);
    helloVk.copyColorImage(nullptr);
    const std::vector<float>& through = helloVk.colorImage();

    std::printf("scene mix, pinhole %ux%u, scanline %u\n", W, H, ROW);
    for(uint32_t x = 0; x < W; ++x)
    {
      const float *a = &opaque[((size_t)ROW * W + x) * 4], *b = &through[((size_t)ROW * W + x) * 4];
      std::printf("pixel %2u: opaque %.9g %.9g %.9g  through %.9g %.9g %.9g\n", x, a[0], a[1], a[2], b[0], b[1], b[2]);
    }
  }
  catch(const std::exception& e)
  {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
