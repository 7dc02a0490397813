// capture_reproject_main.cpp — the capture loop of ray_tracing__before/main.cpp (toroidal camera, rho swept 4.5 → 10.0 in
// steps of 0.5, main.cpp:236-258) and the re-projection of ray_tracing__before_second/main.cpp in ONE program with no
// file in between: every capture stays in the RenderedData buffer on the device, its hits are appended to one compacted
// point cloud (trt_cloud_dev, TRT_CLOUD_COMPACT: exact, in the capture's x*H+y order, any width and height), and the
// cloud of all twelve captures is rasterised from a pinhole viewpoint, tonemapped and written as a PPM.
// Usage: capture_reproject [capture_width capture_height [width height [out.ppm]]]
#include <cstdio>
#include <cstdlib>

#include "../toroidal_ray_tracing_amd/host/hello_hip.hpp"

int main(int argc, char** argv)
{
  const uint32_t cw = argc > 1 ? atoi(argv[1]) : 512, ch = argc > 2 ? atoi(argv[2]) : 256;
  const uint32_t W = argc > 3 ? atoi(argv[3]) : 512, H = argc > 4 ? atoi(argv[4]) : 512;
  try
  {
    HelloHip helloVk;
    helloVk.setup(0);
    helloVk.createOffscreenRender(cw, ch);
    helloVk.m_camera = TRT_CAMERA_TOROIDAL;
    trt_material plastic{};
    plastic.ambient[0] = plastic.ambient[1] = plastic.ambient[2] = 0.05f;
    plastic.diffuse[0] = 0.7f; plastic.diffuse[1] = 0.2f; plastic.diffuse[2] = 0.2f;
    plastic.specular[0] = plastic.specular[1] = plastic.specular[2] = 0.5f;
    plastic.shininess = 24.f; plastic.ior = 1.f; plastic.dissolve = 1.f; plastic.illum = 2; plastic.textureId = -1;
    const float c[3] = {0, 0, 0};
    helloVk.addTorus(c, 14.0f, 3.0f, helloVk.addMaterial(plastic));  // the scene of toroidal_sweep
    helloVk.setLookat({0.f, 0.f, 0.f}, {10.f, 0.f, 0.f}, {0.f, 1.f, 0.f});  // main.cpp:124
    helloVk.updateUniformBuffer();
    const std::array<float, 4> clearColor{1, 1, 1, 1};
    size_t captures = 0;
    for(float rho = 4.5f; rho <= 10.0f; rho += 0.5f) ++captures;
    helloVk.reserveCloud(captures * (size_t)cw * ch);   // room for every record: nothing can be dropped
    // capture and append, capture and append: all on one stream, nothing waits for the host
    for(float rho = 4.5f; rho <= 10.0f; rho += 0.5f)
    {
      helloVk.m_pcRay.rho = rho;
      helloVk.raytrace(nullptr, clearColor);
      helloVk.createCloudDataBufferFromCapture(TRT_CLOUD_COMPACT, true, nullptr);
    }
    const size_t kept = helloVk.numPoints(), wanted = helloVk.wantedPoints();   // the one read-back
    std::printf("%zu captures of %ux%u: %zu records, %zu points kept (%zu wanted), %zu misses dropped\n", captures, cw, ch,
                captures * (size_t)cw * ch, kept, wanted, captures * (size_t)cw * ch - wanted);
    // the re-projection of SEC/main.cpp on its own image size
    helloVk.createOffscreenRender(W, H);
    helloVk.m_camera = TRT_CAMERA_PINHOLE;
    helloVk.setLookat({0.f, 0.f, 0.f}, {10.f, 0.f, 0.f}, {0.f, 1.f, 0.f});   // SEC main.cpp camera
    helloVk.updateUniformBuffer();
    helloVk.rasterize(nullptr, {0.8f, 0.8f, 0.8f, 1.0f});                    // SEC main.cpp:178
    helloVk.drawPost(nullptr);
    helloVk.copyColorImage(nullptr);
    helloVk.copyPostImage(nullptr);
    if(argc > 5) helloVk.writePostImagePPM(argv[5]);
    size_t drawn = 0;
    for(size_t i = 0; i < (size_t)W * H; ++i)
      drawn += helloVk.colorImage()[4 * i] != 0.8f || helloVk.colorImage()[4 * i + 1] != 0.8f;
    std::printf("%zu points -> %ux%u, %zu pixels covered, centre byte %u\n", kept, W, H, drawn,
                (unsigned)helloVk.postImage()[((size_t)(H / 2) * W + W / 2) * 4]);
  }
  catch(const std::exception& e)
  {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
