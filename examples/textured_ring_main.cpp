// textured_ring_main.cpp — a checker-textured plastic ring beside a mirror ring that reflects it, through the host mirror
// (HelloHip::setTextures / raytraceTextured: trt_set_textures, trt_shade_textured_camera_dev).
// The plastic ring (R = 1, r = 0.35, about +y) carries an 8 x 4 checker that repeats four times about the axis and twice
// about the tube; the mirror ring (R = 0.75, r = 0.25) stands upright next to it, about +x, and shows the checker again.
// The texture coordinates are the torus' own two angles: no UV streams, no mesh.
//   1. one ray per pixel, through the pixel centres;
//   2. four rays per pixel on a 2 x 2 grid of sub-pixel offsets: the samples filter the texture as they filter edges
//      (no mip levels are built).
// Prints both colours for every pixel of one scanline, with nine significant digits: the text holds every bit of the floats.
// Usage: textured_ring
#include <cstdio>
#include <vector>

#include "../toroidal_ray_tracing_amd/host/hello_hip.hpp"

static const uint32_t W = 48, H = 36;

int main()
{
  try
  {
    HelloHip helloVk;
    helloVk.setup(0);
    helloVk.createOffscreenRender(W, H);
    trt_material plastic{}, mirror{};
    plastic.ambient[0] = plastic.ambient[1] = plastic.ambient[2] = 0.05f;
    plastic.diffuse[0] = 0.75f; plastic.diffuse[1] = 0.75f; plastic.diffuse[2] = 0.75f;
    plastic.specular[0] = plastic.specular[1] = plastic.specular[2] = 0.5f;
    plastic.shininess = 24.f; plastic.ior = 1.f; plastic.dissolve = 1.f; plastic.illum = 2;
    plastic.textureId = 0;   // texture 0 of setTextures (the reference: textureId + txtOffset)
    mirror.specular[0] = mirror.specular[1] = mirror.specular[2] = 0.95f;
    mirror.shininess = 32.f; mirror.ior = 1.f; mirror.dissolve = 1.f; mirror.illum = 3; mirror.textureId = -1;
    const int   mats[2] = {helloVk.addMaterial(plastic), helloVk.addMaterial(mirror)};
    const float left[3] = {-0.75f, 0.f, 0.f}, right[3] = {1.25f, 0.25f, 0.f};
    helloVk.addTorus(left, 1.0f, 0.35f, mats[0]);
    helloVk.addTorus(right, 0.75f, 0.25f, mats[1]);
    const float axes[6] = {0.f, 1.f, 0.f, 1.f, 0.f, 0.f};
    helloVk.setTorusAxes(axes);

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

    // pinhole camera (REFL/shaders/raytrace.rgen:42-48), written out in binary fractions so that every binding holds the
    // same bits: the film point (dx, dy) in [-1, 1]² becomes the camera-space target (0.6·dx, 0.45·dy, 1) through
    // projInverse; viewInverse (column-major) turns camera x, y, z into the world's (1, 0, 0), (0, 0.8, 0.6),
    // (0, -0.6, 0.8) — looking from the eye (0, 3, -4) at the origin — and carries the eye in its last column
    trt_globals& g = helloVk.m_globals;
    g = trt_globals{};
    g.viewProj[0] = g.viewProj[5] = g.viewProj[10] = g.viewProj[15] = 1.f;   // (not read by the ray calls)
    g.projInverse[0] = 0.6f; g.projInverse[5] = 0.45f; g.projInverse[10] = 1.f; g.projInverse[15] = 1.f;
    g.viewInverse[0] = 1.f;
    g.viewInverse[5] = 0.8f;  g.viewInverse[6] = 0.6f;
    g.viewInverse[9] = -0.6f; g.viewInverse[10] = 0.8f;
    g.viewInverse[12] = 0.f;  g.viewInverse[13] = 3.f; g.viewInverse[14] = -4.f; g.viewInverse[15] = 1.f;
    helloVk.m_camera = TRT_CAMERA_PINHOLE;
    helloVk.m_pcRay.maxDepth = 4;

    const std::array<float, 4> clearColor = {0.1f, 0.2f, 0.4f, 1.f};
    helloVk.raytraceTextured(nullptr, clearColor);
    helloVk.copyColorImage(nullptr);
    const std::vector<float> one = helloVk.colorImage();
    const float grid[8] = {-0.25f, -0.25f, 0.25f, -0.25f, -0.25f, 0.25f, 0.25f, 0.25f};
    helloVk.raytraceTextured(nullptr, clearColor, 4, grid);
    helloVk.copyColorImage(nullptr);
    const std::vector<float>& four = helloVk.colorImage();

    const uint32_t y = H / 2;
    std::printf("textured ring, pinhole %ux%u, scanline %u\n", W, H, y);
    for(uint32_t x = 0; x < W; ++x)
    {
      const float *a = &one[((size_t)y * W + x) * 4], *b = &four[((size_t)y * W + x) * 4];
      std::printf("pixel %2u: one %.9g %.9g %.9g  four %.9g %.9g %.9g\n", x, a[0], a[1], a[2], b[0], b[1], b[2]);
    }
  }
  catch(const std::exception& e)
  {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
