// linked_rings_main.cpp — eight interlocking rings: a chain along x whose rings turn about axes of their own
// (HelloHip::setTorusAxes / trt_set_torus_axes), the instance rotations loadModel(filename, transform) takes in the
// reference.  Renders one frame and writes the presented image as a PPM.
// Usage: linked_rings [width height maxDepth out.ppm]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../toroidal_ray_tracing_amd/host/hello_hip.hpp"

int main(int argc, char** argv)
{
  const uint32_t W = argc > 1 ? atoi(argv[1]) : 1920, H = argc > 2 ? atoi(argv[2]) : 1080;
  const int      depth = argc > 3 ? atoi(argv[3]) : 5;
  const std::string out = argc > 4 ? argv[4] : "linked_rings.ppm";
  try
  {
    HelloHip helloVk;
    helloVk.setup(0);
    helloVk.createOffscreenRender(W, H);
    trt_material mirror{}, plastic{};
    mirror.specular[0] = mirror.specular[1] = mirror.specular[2] = 0.95f;
    mirror.shininess = 32.f; mirror.ior = 1.f; mirror.dissolve = 1.f; mirror.illum = 3; mirror.textureId = -1;
    plastic.ambient[0] = plastic.ambient[1] = plastic.ambient[2] = 0.05f;
    plastic.diffuse[0] = 0.7f; plastic.diffuse[1] = 0.2f; plastic.diffuse[2] = 0.2f;
    plastic.specular[0] = plastic.specular[1] = plastic.specular[2] = 0.5f;
    plastic.shininess = 24.f; plastic.ior = 1.f; plastic.dissolve = 1.f; plastic.illum = 2; plastic.textureId = -1;
    const int mats[2] = {helloVk.addMaterial(mirror), helloVk.addMaterial(plastic)};
    // Centres 1.2 apart, R = 1, r = 0.2: a ring passes through its neighbour's hole 0.2 from the neighbour's centre,
    // 0.8 from its centre circle.  Axes alternately (0,1,1) and (0,-1,1): perpendicular to the chain and to each other.
    constexpr int kRings = 8;
    std::vector<float> axes;
    for(int i = 0; i < kRings; ++i)
    {
      const float c[3] = {(i - 0.5f * (kRings - 1)) * 1.2f, 0.f, 0.f};
      helloVk.addTorus(c, 1.0f, 0.2f, mats[(i / 2) % 2]);
      axes.insert(axes.end(), {0.f, i % 2 == 0 ? 1.f : -1.f, 1.f});   // any length: the library normalises
    }
    helloVk.setTorusAxes(axes.data());
    helloVk.setLookat({0.f, 3.f, -11.f}, {0.f, 0.f, 0.f}, {0.f, 1.f, 0.f});
    helloVk.m_pcRay.maxDepth = depth;
    helloVk.updateUniformBuffer();
    helloVk.raytrace(nullptr, {1, 1, 1, 1});
    helloVk.drawPost(nullptr);
    helloVk.copyPostImage(nullptr);
    helloVk.writePostImagePPM(out);
    std::printf("%ux%u, maxDepth %d, %d linked rings -> %s\n", W, H, depth, kRings, out.c_str());
  }
  catch(const std::exception& e)
  {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
