// The C++ host layer's device-resident descriptor index (include/superslam_hip/place_index.hpp: superslam_hip::DescriptorIndex).
//   no arguments : CPU - the mirror's argument validation (empty results, last_error, nothing thrown) and the C ABI's argument checks
//                  (refused before any device is touched)
//   <in.bin> <out.bin> <exclude_recent> <top_k> <min_score> : GPU - rows added one at a time, then every query through query()
//       in.bin  = int32 M, dim, Q | int64 ids [M] | rows f32 [M][dim] | queries f32 [Q][dim]
//       out.bin = per query: int32 count | count x (int64 id, f32 score)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "superslam_hip/place_index.hpp"

using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static int run_cpu() {
  std::vector<float> d(512, 0.25f);
  {
    DescriptorIndex ix(100);
    EXPECT(ix.size() == 0 && ix.dim() == 0 && ix.capacity() == 100 && ix.last_error().empty());
    EXPECT(ix.query(d, 0, 5, 0.75f).empty() && ix.last_error().empty());             // nothing added yet: empty, as the reference
    EXPECT(ix.query(d, 0, 0, 0.75f).empty() && !ix.last_error().empty());            // topK <= 0 ("all" in the reference) is refused
    EXPECT(ix.query(d, 0, 51, 0.75f).empty());                                       // above max_top_k
    EXPECT(ix.query(d, 0, 5, std::nanf("")).empty());
    EXPECT(ix.query(nullptr, 512, 0, 5, 0.75f).empty());
    EXPECT(ix.query_device(nullptr, 512, 0, 5, 0.75f).empty());
    EXPECT(!ix.add(1, nullptr, 512) && !ix.add_device(1, nullptr, 512));
    std::vector<float> odd(510, 1.f);
    EXPECT(!ix.add(1, odd) && ix.size() == 0 && ix.handle() == nullptr);             // dim not a multiple of 4: refused without a device
    EXPECT(ix.last_error().find("dim") != std::string::npos);
    EXPECT(!ix.add(1, d.data(), 0) && !ix.add(1, d.data(), 4100));
    ix.clear();
  }
  {
    DescriptorIndex none(0);
    EXPECT(!none.add(1, d) && none.last_error().find("capacity") != std::string::npos);
    DescriptorIndex wide(10, 129);
    EXPECT(!wide.add(1, d) && wide.last_error().find("max_top_k") != std::string::npos);
  }
  sship_index* out = nullptr;
  EXPECT(sship_index_create(510, 10, 1, 5, &out) == SSHIP_ERR_INVALID && out == nullptr);
  EXPECT(sship_index_create(512, 10, 1, 5, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_index_create(512, 10, 0, 5, &out) == SSHIP_ERR_INVALID && sship_index_create(512, 10, 1025, 5, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_index_create(512, 10, 1, 0, &out) == SSHIP_ERR_INVALID && sship_index_create(512, 10, 1, 129, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_index_create(4096, 1 << 20, 1, 5, &out) == SSHIP_ERR_INVALID);       // 16 GiB of rows
  EXPECT(sship_index_dim(nullptr) == 0 && sship_index_capacity(nullptr) == 0 && sship_index_size(nullptr) == 0);
  EXPECT(sship_index_clear(nullptr) == SSHIP_ERR_INVALID);
  int64_t id = 0; float s = 0.f; int n = 0;
  EXPECT(sship_index_add_host(nullptr, &id, d.data(), 1, 512) == SSHIP_ERR_INVALID);
  EXPECT(sship_index_add_device(nullptr, &id, d.data(), 1, 512, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_index_read(nullptr, 0, 0, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_index_query_host(nullptr, d.data(), 0, 1, 0.f, &id, &s, &n) == SSHIP_ERR_INVALID);
  EXPECT(sship_index_query_device(nullptr, d.data(), 0, 1, 0.f, &id, &s, &n) == SSHIP_ERR_INVALID);
  EXPECT(sship_index_query_batch_device(nullptr, d.data(), 1, 512, nullptr, 0, 1, 0.f, nullptr, nullptr, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_index_bench(nullptr, 1, nullptr) == SSHIP_ERR_INVALID);
  sship_index_destroy(nullptr);
  std::printf(g_fail ? "place index host layer: %d check(s) failed (cpu)\n" : "place index host layer: all checks passed (cpu)\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 6) return run_cpu();
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int32_t hdr[3] = {0, 0, 0};
  if (std::fread(hdr, 4, 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] <= 0) return 2;
  const int M = hdr[0], dim = hdr[1], Q = hdr[2];
  std::vector<int64_t> ids(static_cast<size_t>(M));
  std::vector<float> rows(static_cast<size_t>(M) * dim), qs(static_cast<size_t>(Q) * dim);
  if (std::fread(ids.data(), 8, ids.size(), f) != ids.size() || std::fread(rows.data(), 4, rows.size(), f) != rows.size() ||
      std::fread(qs.data(), 4, qs.size(), f) != qs.size())
    return 2;
  std::fclose(f);
  const int exclude = std::atoi(argv[3]), top_k = std::atoi(argv[4]);
  const float min_score = static_cast<float>(std::atof(argv[5]));
  DescriptorIndex ix(M + 3);
  for (int i = 0; i < M; ++i) EXPECT(ix.add(static_cast<size_t>(ids[i]), rows.data() + static_cast<size_t>(i) * dim, dim));
  if (g_fail) { std::printf("%s\n", ix.last_error().c_str()); return 1; }
  EXPECT(ix.size() == static_cast<size_t>(M) && ix.dim() == dim);
  EXPECT(!ix.add(1, rows.data(), dim + 4) && ix.size() == static_cast<size_t>(M));        // the dimension is fixed by the first add
  for (int i = 0; i < 3; ++i) EXPECT(ix.add(static_cast<size_t>(900000 + i), rows.data(), dim));
  EXPECT(!ix.add(7, rows.data(), dim) && ix.size() == static_cast<size_t>(M) + 3);        // full: refused, content unchanged
  EXPECT(ix.query(qs.data(), dim, 0, 0, min_score).empty());                              // topK <= 0 refused on a live index too
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  int total = 0;
  for (int j = 0; j < Q; ++j) {
    // the three extra rows are the newest: exclude them on top of the caller's window
    const std::vector<DescriptorIndex::Candidate> c = ix.query(qs.data() + static_cast<size_t>(j) * dim, dim, static_cast<size_t>(exclude) + 3, top_k, min_score);
    const int32_t k = static_cast<int32_t>(c.size());
    std::fwrite(&k, 4, 1, o);
    for (const auto& e : c) { const int64_t id = static_cast<int64_t>(e.keyframe_id); std::fwrite(&id, 8, 1, o); std::fwrite(&e.score, 4, 1, o); }
    total += k;
  }
  std::fclose(o);
  std::printf("place index host layer: %d candidates for %d queries over %d rows\n", total, Q, M);
  return g_fail ? 1 : 0;
}
