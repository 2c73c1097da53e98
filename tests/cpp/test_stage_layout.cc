// csrc/stage_layout.h alone, as a program: every layout at small sizes and at the API maxima, and every pack / unpack on heap blocks of
// exactly in_bytes / out_bytes (so AddressSanitizer sees an overrun), compared byte for byte with expectations written out here.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../superslam_amd/csrc/stage_layout.h"

using namespace sship;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

struct Slot { size_t off, need; };
// multiples of 256, in declaration order, disjoint, and the region ends where the last slot does
static void check_region(const std::vector<Slot>& slots, size_t bytes) {
  size_t prev_end = 0;
  for (const Slot& s : slots) {
    CHECK(s.off % 256 == 0);
    CHECK(s.off >= prev_end);
    prev_end = s.off + s.need;
  }
  CHECK(bytes == prev_end);
}

constexpr unsigned char kFill = 0xCD;    // what a block holds before a pack
constexpr unsigned char kKeep = 0xA5;    // what the caller's outputs hold before an unpack
struct Block {
  char* p; size_t n;
  Block(size_t bytes, unsigned char fill) : p(static_cast<char*>(malloc(bytes ? bytes : 1))), n(bytes) { memset(p, fill, bytes); }
  ~Block() { free(p); }
  Block(const Block&) = delete;
};
static bool same(const Block& a, const std::vector<unsigned char>& want) { return a.n == want.size() && (a.n == 0 || memcmp(a.p, want.data(), a.n) == 0); }
template <class T> static std::vector<T> ramp(size_t n, int seed) {
  std::vector<T> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (T)((i * 7 + seed) % 251 + 1);
  return v;
}
template <class T> static void put(std::vector<unsigned char>& want, size_t off, const T* src, size_t count) {
  if (count) memcpy(want.data() + off, src, count * sizeof(T));
}
template <class T> static bool all_keep(const std::vector<T>& v, size_t from) {
  const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = from * sizeof(T); i < v.size() * sizeof(T); ++i) if (b[i] != kKeep) return false;
  return true;
}
template <class T> static std::vector<T> kept(size_t n) {
  std::vector<T> v(n ? n : 1);
  memset(v.data(), kKeep, v.size() * sizeof(T));
  return v;
}

// ---- pose / ransac -----------------------------------------------------------------------------------------------------------------------
static void obs_case(bool ransac, int max_obs) {
  const ObsStage st = ransac ? ransac_stage(max_obs) : pose_stage(max_obs);
  const size_t n = (size_t)max_obs, cost_bytes = ransac ? 8 : 16;
  check_region({{st.points, n * 12}, {st.meas, n * 12}, {st.pose0, ransac ? 0u : 96u}, {st.valid, n}}, st.in_bytes);
  check_region({{st.pose, 96}, {st.cost, cost_bytes}, {st.stats, 16}, {st.inlier, n}}, st.out_bytes);
  const std::vector<float> points = ramp<float>(n * 3, 1), meas = ramp<float>(n * 3, 2);
  std::vector<uint8_t> valid(n);
  for (size_t i = 0; i < n; ++i) valid[i] = (uint8_t)(i % 3 == 0 ? 0 : i % 3 == 1 ? 1 : 200);   // any non-zero byte counts as 1
  const std::vector<double> pose0 = ramp<double>(12, 3);
  const int counts[4] = {0, 1, max_obs - 1, max_obs};
  for (int m : counts) {
    if (m < 0) continue;
    for (int has_valid = 0; has_valid < 2; ++has_valid)
      for (int has_pose0 = 0; has_pose0 < (ransac ? 1 : 2); ++has_pose0) {
        Block in(st.in_bytes, kFill);
        obs_pack(in.p, st, m ? points.data() : nullptr, m ? meas.data() : nullptr, has_valid ? valid.data() : nullptr, m, has_pose0 ? pose0.data() : nullptr);
        std::vector<unsigned char> want(st.in_bytes, 0);   // zeros past the count and between the slots
        put(want, st.points, points.data(), (size_t)m * 3);
        put(want, st.meas, meas.data(), (size_t)m * 3);
        for (int i = 0; i < m; ++i) want[st.valid + i] = has_valid ? (valid[i] ? 1 : 0) : 1;
        if (has_pose0) put(want, st.pose0, pose0.data(), 12);
        CHECK(same(in, want));
      }
    for (int has_inlier = 0; has_inlier < 2; ++has_inlier) {
      Block out(st.out_bytes, 0);
      for (size_t i = 0; i < st.out_bytes; ++i) out.p[i] = (char)(i * 13 + 5);
      std::vector<double> pose = kept<double>(13), cost = kept<double>(3);
      std::vector<int32_t> stats = kept<int32_t>(5);
      std::vector<uint8_t> inlier = kept<uint8_t>(n + 1);
      obs_unpack(out.p, st, m, pose.data(), stats.data(), cost.data(), has_inlier ? inlier.data() : nullptr);
      CHECK(memcmp(pose.data(), out.p + st.pose, 96) == 0 && all_keep(pose, 12));
      CHECK(memcmp(cost.data(), out.p + st.cost, cost_bytes) == 0 && all_keep(cost, cost_bytes / 8));
      CHECK(memcmp(stats.data(), out.p + st.stats, 16) == 0 && all_keep(stats, 4));
      if (has_inlier) CHECK(memcmp(inlier.data(), out.p + st.inlier, (size_t)m) == 0 && all_keep(inlier, (size_t)m));
      else CHECK(all_keep(inlier, 0));
    }
  }
}

// ---- window smoother ---------------------------------------------------------------------------------------------------------------------
static void ba_case(int K, int N, int L) {
  const BaStage st = ba_stage(K, N, L);
  const size_t kn = (size_t)K * N, k12 = (size_t)K * 12, l3 = (size_t)L * 3;
  check_region({{st.pose0, k12 * 8}, {st.meas, kn * 12}, {st.track, kn * 4}, {st.n_kf, 4}}, st.in_bytes);
  check_region({{st.pose, k12 * 8}, {st.cost, 16}, {st.stats, 16}, {st.landmarks, l3 * 4}}, st.out_bytes);
  const std::vector<float> meas = ramp<float>(kn * 3, 4);
  const std::vector<int32_t> track = ramp<int32_t>(kn, 5);
  const std::vector<double> pose0 = ramp<double>(k12, 6);
  const int counts[4] = {0, 1, K - 1, K};
  for (int n_kf : counts) {
    Block in(st.in_bytes, kFill);
    ba_pack(in.p, st, meas.data(), track.data(), n_kf, pose0.data());
    std::vector<unsigned char> want(st.in_bytes, kFill);   // whole arrays are copied; nothing else is written
    put(want, st.pose0, pose0.data(), k12);
    put(want, st.meas, meas.data(), kn * 3);
    put(want, st.track, track.data(), kn);
    const int32_t nk = n_kf;
    put(want, st.n_kf, &nk, 1);
    CHECK(same(in, want));
  }
  for (int has_lm = 0; has_lm < 2; ++has_lm) {
    Block out(st.out_bytes, 0);
    for (size_t i = 0; i < st.out_bytes; ++i) out.p[i] = (char)(i * 11 + 3);
    std::vector<double> pose = kept<double>(k12 + 1), cost = kept<double>(3);
    std::vector<int32_t> stats = kept<int32_t>(5);
    std::vector<float> lm = kept<float>(l3 + 1);
    ba_unpack(out.p, st, pose.data(), stats.data(), cost.data(), has_lm ? lm.data() : nullptr);
    CHECK(memcmp(pose.data(), out.p + st.pose, k12 * 8) == 0 && all_keep(pose, k12));
    CHECK(memcmp(cost.data(), out.p + st.cost, 16) == 0 && all_keep(cost, 2));
    CHECK(memcmp(stats.data(), out.p + st.stats, 16) == 0 && all_keep(stats, 4));
    if (has_lm) CHECK(memcmp(lm.data(), out.p + st.landmarks, l3 * 4) == 0 && all_keep(lm, l3));
    else CHECK(all_keep(lm, 0));
  }
}

// ---- pose graph --------------------------------------------------------------------------------------------------------------------------
static void pg_case(int N, int L) {
  const PgStage st = pg_stage(N, L);
  const size_t n = (size_t)N, l = (size_t)L;
  check_region({{st.pose0, n * 96}, {st.oz, (n - 1) * 96}, {st.osg, (n - 1) * 48}, {st.lz, l * 96}, {st.lsg, l * 48}, {st.lk2, l * 8}, {st.lij, l * 8},
                {st.nn, 4}, {st.len, l}}, st.in_bytes);
  check_region({{st.pose, n * 96}, {st.cost, 16}, {st.chi2, l * 8}, {st.stats, 16}}, st.out_bytes);
  const std::vector<double> pose0 = ramp<double>(n * 12, 1), oz = ramp<double>(n * 12, 2), osg = ramp<double>(n * 6, 3), lz = ramp<double>(l * 12 + 1, 4),
                            lsg = ramp<double>(l * 6 + 1, 5), lk2 = ramp<double>(l + 1, 6);
  const std::vector<int32_t> lij = ramp<int32_t>(l * 2 + 1, 7);
  const int nodes[4] = {0, 1, N - 1, N}, loops[4] = {0, 1, L - 1, L};
  for (int nn : nodes)
    for (int nl : loops) {
      if (nl < 0 || nl > L) continue;
      for (int has_sigma = 0; has_sigma < 2; ++has_sigma) {
        Block in(st.in_bytes, kFill);
        pg_pack(in.p, st, nn, pose0.data(), oz.data(), has_sigma ? osg.data() : nullptr, nl, lij.data(), lz.data(), lsg.data(), lk2.data());
        std::vector<unsigned char> want(st.in_bytes, 0);
        put(want, st.pose0, pose0.data(), (size_t)nn * 12);
        if (nn > 1) put(want, st.oz, oz.data(), (size_t)(nn - 1) * 12);
        if (nn > 1 && has_sigma) put(want, st.osg, osg.data(), (size_t)(nn - 1) * 6);
        put(want, st.lz, lz.data(), (size_t)nl * 12);
        put(want, st.lsg, lsg.data(), (size_t)nl * 6);
        put(want, st.lk2, lk2.data(), (size_t)nl);
        put(want, st.lij, lij.data(), (size_t)nl * 2);
        for (int i = 0; i < nl; ++i) want[st.len + i] = 1;   // enable: the leading n_loops only
        const int32_t n32 = nn;
        put(want, st.nn, &n32, 1);
        CHECK(same(in, want));
      }
      for (int has_chi2 = 0; has_chi2 < 2; ++has_chi2) {
        Block out(st.out_bytes, 0);
        for (size_t i = 0; i < st.out_bytes; ++i) out.p[i] = (char)(i * 17 + 1);
        std::vector<double> pose = kept<double>(n * 12 + 1), cost = kept<double>(3), chi2 = kept<double>(l + 1);
        std::vector<int32_t> stats = kept<int32_t>(5);
        pg_unpack(out.p, st, nn, nl, pose.data(), stats.data(), cost.data(), has_chi2 ? chi2.data() : nullptr);
        CHECK(memcmp(pose.data(), out.p + st.pose, (size_t)nn * 96) == 0 && all_keep(pose, (size_t)nn * 12));
        CHECK(memcmp(cost.data(), out.p + st.cost, 16) == 0 && all_keep(cost, 2));
        CHECK(memcmp(stats.data(), out.p + st.stats, 16) == 0 && all_keep(stats, 4));
        if (has_chi2) CHECK(memcmp(chi2.data(), out.p + st.chi2, (size_t)nl * 8) == 0 && all_keep(chi2, (size_t)nl));
        else CHECK(all_keep(chi2, 0));
      }
    }
}

// ---- nearest-neighbour matcher -----------------------------------------------------------------------------------------------------------
static void nn_case(int max_kp) {
  const NnStage st = nn_stage(max_kp);
  const size_t n = (size_t)max_kp;
  check_region({{st.lens, 8}, {st.desc, 2 * n * 512}, {st.kp, 2 * n * 12}}, st.in_bytes);
  CHECK(st.desc1 == st.desc + n * 512 && st.kp1 == st.kp + n * 12);   // [2][max_kp][...]: the second image follows the first without a gap
  check_region({{st.m0, n * 4}, {st.ms0, n * 4}}, st.out_bytes);
  std::vector<float> d0(n * 256), d1(n * 256);
  for (size_t i = 0; i < d0.size(); ++i) { d0[i] = (float)((int)(i % 97) - 48) / 64.f; d1[i] = (float)((int)(i % 89) - 44) / 1024.f + 1e-5f; }
  const int s0 = 3, s1 = 5;
  const std::vector<float> k0 = ramp<float>(n * s0, 8), k1 = ramp<float>(n * s1, 9);
  const int counts[4] = {0, 1, max_kp - 1, max_kp};
  for (int n0 : counts)
    for (int n1 : counts) {
      Block in(st.in_bytes, kFill);
      nn_pack_lens(in.p, st, n0, n1);
      nn_pack_desc(in.p, st, n0, d0.data(), n1, d1.data());
      nn_pack_kp(in.p, st, k0.data(), s0, n0, k1.data(), s1, n1);
      std::vector<unsigned char> want(st.in_bytes, kFill);   // only the rows in use are written
      const int32_t lens[2] = {n0, n1};
      put(want, st.lens, lens, 2);
      for (int img = 0; img < 2; ++img) {
        const int cnt = img ? n1 : n0, stride = img ? s1 : s0;
        const std::vector<float>& d = img ? d1 : d0;
        const std::vector<float>& k = img ? k1 : k0;
        for (size_t i = 0; i < (size_t)cnt * 256; ++i) { const _Float16 h = (_Float16)d[i]; put(want, st.desc + img * n * 512 + i * 2, &h, 1); }
        for (int i = 0; i < cnt; ++i) {
          const float row[3] = {k[(size_t)i * stride], k[(size_t)i * stride + 1], 0.f};   // the third component is 0
          put(want, st.kp + img * n * 12 + (size_t)i * 12, row, 3);
        }
      }
      CHECK(same(in, want));
      Block out(st.out_bytes, 0);
      for (size_t i = 0; i < st.out_bytes; ++i) out.p[i] = (char)(i * 19 + 7);
      std::vector<int32_t> m0 = kept<int32_t>(n + 1);
      std::vector<float> ms0 = kept<float>(n + 1);
      nn_unpack(out.p, st, n0, m0.data(), ms0.data());
      CHECK(memcmp(m0.data(), out.p + st.m0, (size_t)n0 * 4) == 0 && all_keep(m0, (size_t)n0));
      CHECK(memcmp(ms0.data(), out.p + st.ms0, (size_t)n0 * 4) == 0 && all_keep(ms0, (size_t)n0));
    }
}

// ---- place index -------------------------------------------------------------------------------------------------------------------------
static void index_case(int dim, int max_top_k) {
  const IndexStage st = index_stage(dim, max_top_k);
  const size_t k = (size_t)max_top_k;
  check_region({{st.q, (size_t)dim * 4}}, st.in_bytes);
  check_region({{st.rows, k * 4}, {st.scores, k * 4}, {st.count, 4}}, st.out_bytes);
  const std::vector<float> q = ramp<float>((size_t)dim, 10);
  Block in(st.in_bytes, kFill);
  index_pack(in.p, st, dim, q.data());
  std::vector<unsigned char> want(st.in_bytes, kFill);
  put(want, st.q, q.data(), (size_t)dim);
  CHECK(same(in, want));
  const int size = max_top_k + 3;
  std::vector<int64_t> ids((size_t)size);
  for (int i = 0; i < size; ++i) ids[i] = 1000 + 3 * (int64_t)i;
  const int counts[4] = {0, 1, max_top_k - 1, max_top_k};
  for (int top_k : {1, max_top_k})
    for (int cnt : counts) {
      if (cnt > top_k) continue;
      Block out(st.out_bytes, 0);
      std::vector<int32_t> rows(k);
      std::vector<float> scores(k);
      for (size_t i = 0; i < k; ++i) { rows[i] = (int32_t)((i * 5 + 2) % size); scores[i] = 1.f - 0.001f * (float)i; }
      memcpy(out.p + st.rows, rows.data(), k * 4); memcpy(out.p + st.scores, scores.data(), k * 4); memcpy(out.p + st.count, &cnt, 4);
      std::vector<int64_t> ids_out = kept<int64_t>(k + 1);
      std::vector<float> sc_out = kept<float>(k + 1);
      int got = -7;
      CHECK(index_unpack(out.p, st, top_k, ids.data(), size, ids_out.data(), sc_out.data(), &got) == 0 && got == cnt);
      for (int i = 0; i < cnt; ++i) CHECK(ids_out[i] == ids[rows[i]] && sc_out[i] == scores[i]);
      CHECK(all_keep(ids_out, (size_t)cnt) && all_keep(sc_out, (size_t)cnt));
      // what the device must never return is refused, not read past
      const int over = top_k + 1, under = -1;
      memcpy(out.p + st.count, &over, 4);
      CHECK(index_unpack(out.p, st, top_k, ids.data(), size, ids_out.data(), sc_out.data(), &got) == 1);
      memcpy(out.p + st.count, &under, 4);
      CHECK(index_unpack(out.p, st, top_k, ids.data(), size, ids_out.data(), sc_out.data(), &got) == 1);
      if (cnt > 0) {
        memcpy(out.p + st.count, &cnt, 4);
        memcpy(out.p + st.rows + (size_t)(cnt - 1) * 4, &size, 4);
        CHECK(index_unpack(out.p, st, top_k, ids.data(), size, ids_out.data(), sc_out.data(), &got) == 2);
      }
    }
}

// ---- one image pair and its keypoints -----------------------------------------------------------------------------------------------------
static void pair_case(int h, int w, int n) {
  const PairStage st = pair_stage(h, w, n);
  const size_t px = (size_t)h * w, m = (size_t)n;
  check_region({{st.img, 2 * px}, {st.n, 4}, {st.kp, m * 12}, {st.pred, m * 12}}, st.in_bytes);
  CHECK(st.img1 == st.img + px);                        // [2][h][w]: the second image follows the first without a gap
  CHECK(st.tail_bytes == st.in_bytes - st.n && st.rows_bytes == m * 12);
  check_region({{st.rows, m * 12}, {st.flag, m * 4}, {st.status, m}, {st.cost, m * 8}, {st.levels, m}}, st.out_bytes);
  const size_t o_kp = st.kp - st.n, o_pred = st.pred - st.n;   // in the tail, which starts at the count
  const int32_t n32 = n;
  for (int kp_stride : {2, 3, 5})
    for (int score = 0; score < 2; ++score)
      for (int pred_stride : {0, 2, 7}) {               // 0: no pred
        // caller's arrays of exactly n strided rows (the last row ends with its stride: what the API documents)
        const std::vector<float> kp = ramp<float>(m * kp_stride, 11 + kp_stride), pr = ramp<float>(m * pred_stride, 12 + pred_stride);
        Block tail(st.tail_bytes, kFill);
        pair_pack_n(tail.p, n);
        pair_pack_kp(tail.p, st, kp.data(), kp_stride, n, score != 0);
        if (pred_stride) pair_pack_pred(tail.p, st, pr.data(), pred_stride, n);
        std::vector<unsigned char> want(st.tail_bytes, kFill);   // only the slots packed are written: whole, so nothing stale is uploaded from them
        put(want, 0, &n32, 1);
        for (int i = 0; i < n; ++i) {
          const float row[3] = {kp[(size_t)i * kp_stride], kp[(size_t)i * kp_stride + 1], score && kp_stride >= 3 ? kp[(size_t)i * kp_stride + 2] : 0.f};
          put(want, o_kp + (size_t)i * 12, row, 3);
          if (pred_stride) {
            const float prow[3] = {pr[(size_t)i * pred_stride], pr[(size_t)i * pred_stride + 1], 0.f};
            put(want, o_pred + (size_t)i * 12, prow, 3);
          }
        }
        CHECK(same(tail, want));
      }
  // the score travels as bits: a signalling-NaN pattern survives the pack
  if (n > 0) {
    const uint32_t bits[3] = {0x40000000u, 0x40400000u, 0x7fa00001u};
    float row[3];
    memcpy(row, bits, 12);
    const PairStage one = pair_stage(h, w, 1);
    Block t1(one.tail_bytes, kFill);
    pair_pack_kp(t1.p, one, row, 3, 1, true);
    CHECK(memcmp(t1.p + (one.kp - one.n), bits, 12) == 0);
  }
}

int main() {
  StageLayout lay;
  CHECK(lay.add(1) == 0 && lay.end == 1 && lay.add(255) == 256 && lay.end == 511 && lay.add(0) == 512 && lay.end == 512 && lay.add(7) == 512);
  for (int max_obs : {1, 5, 33, 2048}) { obs_case(false, max_obs); obs_case(true, max_obs); }
  for (auto c : {std::vector<int>{2, 1, 1}, {3, 5, 7}, {4, 33, 40}, {16, 2048, 32768}}) ba_case(c[0], c[1], c[2]);
  for (auto c : {std::vector<int>{2, 0}, {3, 1}, {5, 3}, {4096, 128}}) pg_case(c[0], c[1]);
  for (int max_kp : {1, 33, 4096}) nn_case(max_kp);
  for (auto c : {std::vector<int>{4, 1}, {36, 3}, {4, 3}, {36, 1}, {4096, 128}}) index_case(c[0], c[1]);
  for (auto c : {std::vector<int>{1, 1, 1}, {3, 5, 1}, {5, 5, 5}, {11, 21, 33}, {16384, 16384, 4096}}) pair_case(c[0], c[1], c[2]);
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("all checks passed (stage layout)\n");
  return 0;
}
