// include/superslam_hip/place_recognizer.hpp: the batch methods of EigenPlaces.  Without a GPU: their error conventions.  With a weights path
// (GPU): compute_global_descriptors on images that live in buffers of their own, with padded rows, in chunks of max_batch(), against
// compute_global_descriptor on every image - bit for bit.
#include <cstdio>
#include <cstring>

#include "superslam_hip/place_recognizer.hpp"

using namespace superslam_hip;
static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++g_fail; } } while (0)

int main(int argc, char** argv) {
  {  // not initialised: nothing reserved, nothing computed
    EigenPlaces ep("/nonexistent/eigenplaces.safetensors", 130, 100);
    CHECK(!ep.initialize());
    CHECK(ep.max_batch() == 0);
    CHECK(!ep.reserve_batch(4));
    CHECK(!ep.last_error().empty());
    std::vector<uint8_t> px(64 * 64, 7);
    std::vector<Image> two(2, Image{px.data(), 64, 64, 1, 0});
    CHECK(ep.compute_global_descriptors(two).empty());
    CHECK(ep.compute_global_descriptors(std::vector<Image>()).empty());
  }
  if (argc >= 2) {
    EigenPlaces ep(argv[1], 130, 100);
    CHECK(ep.initialize());
    CHECK(ep.max_batch() == 1);
    const int H = 60, W = 90, C = 3, N = 5, stride = W * C + 7;
    std::vector<std::vector<uint8_t>> bufs;
    std::vector<Image> images;
    for (int i = 0; i < N; ++i) {
      bufs.emplace_back(static_cast<size_t>(H) * stride, static_cast<uint8_t>(200 + i));   // the padding holds another value than any pixel row
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W * C; ++x) bufs.back()[static_cast<size_t>(y) * stride + x] = static_cast<uint8_t>((x * (7 + i) + y * 13 + ((x / 40 + y / 30 + i) % 5) * 37) & 255);
    }
    for (int i = 0; i < N; ++i) images.push_back(Image{bufs[i].data(), H, W, C, stride});
    std::vector<GlobalDescriptor> single;
    for (const Image& im : images) single.push_back(ep.compute_global_descriptor(im));
    for (int reserve : {1, 2, 8}) {   // chunks of 1; of 2, 2, 1; one chunk
      CHECK(ep.reserve_batch(reserve));
      CHECK(ep.max_batch() == reserve);
      const std::vector<GlobalDescriptor> got = ep.compute_global_descriptors(images);
      CHECK(got.size() == static_cast<size_t>(N));
      for (size_t i = 0; i < got.size(); ++i) {
        CHECK(got[i].size() == 512 && single[i].size() == 512);
        CHECK(std::memcmp(got[i].data(), single[i].data(), 512 * sizeof(float)) == 0);
      }
    }
    CHECK(std::memcmp(single[0].data(), single[1].data(), 512 * sizeof(float)) != 0);
    CHECK(!ep.reserve_batch(0) && !ep.reserve_batch(1025) && ep.max_batch() == 8);
    CHECK(ep.reserve_batch(3) && ep.max_batch() == 8);   // never shrinks
    std::vector<Image> mixed = images;
    mixed[2].rows = H - 1;
    CHECK(ep.compute_global_descriptors(mixed).empty());
    CHECK(ep.last_error().find("one size") != std::string::npos);
  }
  if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
  std::printf("place recognizer batch: all checks passed\n");
  return 0;
}
