// Staging layouts of the single-item entries (sship_*_solve_host, sship_nn_match_*, sship_index_query_*, and the image-pair entries
// sship_stereo_refine_host, sship_stereo_search_host, sship_patch_track_host, sship_patch_track_pyramid_host, and the one-image / one-pair
// entries sship_fast_detect_host, sship_brief_describe_host, sship_hm_match_host): where each field of one staged
// item lies in the handle's (or, for an image pair, the call's) arena, and the host-side pack / unpack of that block.  Plain C++17, no HIP: api.hip includes it, and
// tests/cpp/test_stage_layout.cc builds it alone (also under the host sanitizers).  A block has an input region and an output region; each
// is contiguous, so one copy covers it, and every slot starts on a multiple of kStageAlign (what a hipMalloc of its own would give).
// Offsets of the output slots count from the start of the output region.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace sship {

constexpr size_t kStageAlign = 256;

// one region, bump-allocated: add(bytes) returns the slot's offset, `end` is the end of the last slot
struct StageLayout {
  size_t end = 0;
  size_t add(size_t bytes) {
    const size_t o = (end + kStageAlign - 1) / kStageAlign * kStageAlign;
    end = o + bytes;
    return o;
  }
};

// ---- pose-only solver and RANSAC seed: [max_obs] points | meas | pose0 (pose only) | valid -> pose | cost | stats | inlier --------------
struct ObsStage { size_t points, meas, pose0, valid, in_bytes, pose, cost, stats, inlier, out_bytes, cost_bytes; };
inline ObsStage obs_stage(int max_obs, size_t pose0_bytes, size_t cost_bytes) {
  const size_t n = (size_t)max_obs;
  StageLayout in, out;
  ObsStage s;
  s.points = in.add(n * 12); s.meas = in.add(n * 12); s.pose0 = in.add(pose0_bytes); s.valid = in.add(n); s.in_bytes = in.end;
  s.pose = out.add(96); s.cost = out.add(cost_bytes); s.stats = out.add(16); s.inlier = out.add(n); s.out_bytes = out.end;
  s.cost_bytes = cost_bytes;
  return s;
}
inline ObsStage pose_stage(int max_obs) { return obs_stage(max_obs, 96, 16); }
inline ObsStage ransac_stage(int max_obs) { return obs_stage(max_obs, 0, 8); }   // no prior pose; cost is one double
// rows >= n_obs absent (zeros, valid = 0); valid == NULL: every given row counts; pose0 == NULL: its slot stays zero
inline void obs_pack(char* in, const ObsStage& st, const float* points, const float* meas, const uint8_t* valid, int n_obs, const double* pose0) {
  const size_t m = (size_t)n_obs;
  memset(in, 0, st.in_bytes);
  if (m) { memcpy(in + st.points, points, m * 12); memcpy(in + st.meas, meas, m * 12); }
  uint8_t* hv = reinterpret_cast<uint8_t*>(in + st.valid);
  for (size_t i = 0; i < m; ++i) hv[i] = valid ? (valid[i] != 0) : 1;
  if (pose0) memcpy(in + st.pose0, pose0, 96);
}
inline void obs_unpack(const char* out, const ObsStage& st, int n_obs, double* pose, int32_t* stats, double* cost, uint8_t* inlier) {
  memcpy(pose, out + st.pose, 96);
  memcpy(cost, out + st.cost, st.cost_bytes);
  memcpy(stats, out + st.stats, 16);
  if (inlier && n_obs) memcpy(inlier, out + st.inlier, (size_t)n_obs);
}

// ---- window smoother: pose0 [K] | meas [K][N] | track [K][N] | n_kf -> pose [K] | cost | stats | landmarks [L] (last: optional) -----------
struct BaStage { size_t pose0, meas, track, n_kf, in_bytes, pose, cost, stats, landmarks, out_bytes, pose_bytes, obs, lm_bytes; };
inline BaStage ba_stage(int K, int N, int L) {
  StageLayout in, out;
  BaStage s;
  s.pose_bytes = (size_t)K * 96; s.obs = (size_t)K * N; s.lm_bytes = (size_t)L * 12;
  s.pose0 = in.add(s.pose_bytes); s.meas = in.add(s.obs * 12); s.track = in.add(s.obs * 4); s.n_kf = in.add(4); s.in_bytes = in.end;
  s.pose = out.add(s.pose_bytes); s.cost = out.add(16); s.stats = out.add(16); s.landmarks = out.add(s.lm_bytes); s.out_bytes = out.end;
  return s;
}
// the caller's arrays are whole windows: every row is copied, n_kf says how many keyframes count
inline void ba_pack(char* in, const BaStage& st, const float* meas, const int32_t* track, int n_kf, const double* pose0) {
  memcpy(in + st.pose0, pose0, st.pose_bytes);
  memcpy(in + st.meas, meas, st.obs * 12);
  memcpy(in + st.track, track, st.obs * 4);
  const int32_t nk = n_kf;
  memcpy(in + st.n_kf, &nk, 4);
}
inline void ba_unpack(const char* out, const BaStage& st, double* pose, int32_t* stats, double* cost, float* landmarks) {
  memcpy(pose, out + st.pose, st.pose_bytes);
  memcpy(cost, out + st.cost, 16);
  memcpy(stats, out + st.stats, 16);
  if (landmarks) memcpy(landmarks, out + st.landmarks, st.lm_bytes);
}

// ---- pose graph: pose0 [N] | odom_z | odom_sigma [N-1] | loop_z | loop_sigma | loop_k2 | loop_ij [L] | n_nodes | enable [L]
//                  -> pose [N] | cost | chi2 [L] | stats ---------------------------------------------------------------------------------
struct PgStage { size_t pose0, oz, osg, lz, lsg, lk2, lij, nn, len, in_bytes, pose, cost, chi2, stats, out_bytes; };
inline PgStage pg_stage(int N, int L) {
  const size_t n = (size_t)N, l = (size_t)L;
  StageLayout in, out;
  PgStage s;
  s.pose0 = in.add(n * 96); s.oz = in.add((n - 1) * 96); s.osg = in.add((n - 1) * 48);
  s.lz = in.add(l * 96); s.lsg = in.add(l * 48); s.lk2 = in.add(l * 8); s.lij = in.add(l * 8);
  s.nn = in.add(4); s.len = in.add(l); s.in_bytes = in.end;
  s.pose = out.add(n * 96); s.cost = out.add(16); s.chi2 = out.add(l * 8); s.stats = out.add(16); s.out_bytes = out.end;
  return s;
}
// rows past n_nodes / n_loops: zeros, and enable = 0; odom_sigma == NULL: its slot stays zero
inline void pg_pack(char* in, const PgStage& st, int n_nodes, const double* pose0, const double* odom_z, const double* odom_sigma, int n_loops,
                    const int32_t* loop_ij, const double* loop_z, const double* loop_sigma, const double* loop_k2) {
  memset(in, 0, st.in_bytes);
  if (n_nodes > 0) memcpy(in + st.pose0, pose0, (size_t)n_nodes * 96);
  if (n_nodes > 1) {
    memcpy(in + st.oz, odom_z, (size_t)(n_nodes - 1) * 96);
    if (odom_sigma) memcpy(in + st.osg, odom_sigma, (size_t)(n_nodes - 1) * 48);
  }
  if (n_loops > 0) {
    memcpy(in + st.lz, loop_z, (size_t)n_loops * 96);
    memcpy(in + st.lsg, loop_sigma, (size_t)n_loops * 48);
    memcpy(in + st.lk2, loop_k2, (size_t)n_loops * 8);
    memcpy(in + st.lij, loop_ij, (size_t)n_loops * 8);
    memset(in + st.len, 1, (size_t)n_loops);
  }
  const int32_t nn = n_nodes;
  memcpy(in + st.nn, &nn, 4);
}
inline void pg_unpack(const char* out, const PgStage& st, int n_nodes, int n_loops, double* pose, int32_t* stats, double* cost, double* chi2) {
  if (n_nodes > 0) memcpy(pose, out + st.pose, (size_t)n_nodes * 96);
  memcpy(cost, out + st.cost, 16);
  memcpy(stats, out + st.stats, 16);
  if (chi2 && n_loops > 0) memcpy(chi2, out + st.chi2, (size_t)n_loops * 8);
}

// ---- nearest-neighbour matcher, one pair: lens [2] | desc [2][max_kp][256] fp16 | kp [2][max_kp][3] -> matches0 | mscores0 [max_kp] -----
// `desc1` / `kp1`: where the second image's rows start.  Only the rows in use are packed and copied (n0 and n1 of them, not max_kp).
struct NnStage { size_t lens, desc, desc1, kp, kp1, in_bytes, m0, ms0, out_bytes; };
inline NnStage nn_stage(int max_kp) {
  const size_t n = (size_t)max_kp;
  StageLayout in, out;
  NnStage s;
  s.lens = in.add(8); s.desc = in.add(2 * n * 512); s.kp = in.add(2 * n * 12); s.in_bytes = in.end;
  s.desc1 = s.desc + n * 512; s.kp1 = s.kp + n * 12;
  s.m0 = out.add(n * 4); s.ms0 = out.add(n * 4); s.out_bytes = out.end;
  return s;
}
inline void nn_pack_lens(char* in, const NnStage& st, int n0, int n1) {
  const int32_t lens[2] = {n0, n1};
  memcpy(in + st.lens, lens, 8);
}
// CV_32F -> fp16 on the host, as sship_lg_match_host
inline void nn_pack_desc(char* in, const NnStage& st, int n0, const float* desc0, int n1, const float* desc1) {
  _Float16* h0 = reinterpret_cast<_Float16*>(in + st.desc);
  _Float16* h1 = reinterpret_cast<_Float16*>(in + st.desc1);
  for (size_t i = 0; i < (size_t)n0 * 256; ++i) h0[i] = (_Float16)desc0[i];
  for (size_t i = 0; i < (size_t)n1 * 256; ++i) h1[i] = (_Float16)desc1[i];
}
// the gate's keypoints as (x, y, 0) rows out of the caller's strided ones
inline void nn_pack_kp(char* in, const NnStage& st, const float* kp0, int st0, int n0, const float* kp1, int st1, int n1) {
  float* h0 = reinterpret_cast<float*>(in + st.kp);
  float* h1 = reinterpret_cast<float*>(in + st.kp1);
  for (int i = 0; i < n0; ++i) { h0[3 * i] = kp0[(size_t)i * st0]; h0[3 * i + 1] = kp0[(size_t)i * st0 + 1]; h0[3 * i + 2] = 0.f; }
  for (int i = 0; i < n1; ++i) { h1[3 * i] = kp1[(size_t)i * st1]; h1[3 * i + 1] = kp1[(size_t)i * st1 + 1]; h1[3 * i + 2] = 0.f; }
}
inline void nn_unpack(const char* out, const NnStage& st, int n0, int32_t* matches0, float* mscores0) {
  memcpy(matches0, out + st.m0, (size_t)n0 * 4);
  memcpy(mscores0, out + st.ms0, (size_t)n0 * 4);
}

// ---- place index, one query: q [dim] -> rows | scores [max_top_k] | count ------------------------------------------------------------------
struct IndexStage { size_t q, in_bytes, rows, scores, count, out_bytes; };
inline IndexStage index_stage(int dim, int max_top_k) {
  StageLayout in, out;
  IndexStage s;
  s.q = in.add((size_t)dim * 4); s.in_bytes = in.end;
  s.rows = out.add((size_t)max_top_k * 4); s.scores = out.add((size_t)max_top_k * 4); s.count = out.add(4); s.out_bytes = out.end;
  return s;
}
inline void index_pack(char* in, const IndexStage& st, int dim, const float* desc) { memcpy(in + st.q, desc, (size_t)dim * 4); }
// rows -> the caller's ids through `ids` [size].  Returns 0, 1 for a count outside [0, top_k], 2 for a row outside [0, size).
inline int index_unpack(const char* out, const IndexStage& st, int top_k, const int64_t* ids, int size, int64_t* ids_out, float* scores_out,
                        int* count_out) {
  int32_t n;
  memcpy(&n, out + st.count, 4);
  if (n < 0 || n > top_k) return 1;
  const int32_t* rows = reinterpret_cast<const int32_t*>(out + st.rows);
  const float* scores = reinterpret_cast<const float*>(out + st.scores);
  for (int i = 0; i < n; ++i) {
    if (rows[i] < 0 || rows[i] >= size) return 2;
    ids_out[i] = ids[rows[i]];
    scores_out[i] = scores[i];
  }
  *count_out = n;
  return 0;
}

// ---- one image pair and its keypoints (stereo refinement and search, patch and pyramid tracker):
//      img [2][h][w] | n | kp [n][3] | pred [n][3] -> rows [n][3] | flag [n] | status [n] | cost [n] i64 | levels [n] ---------------------------
// The images are packed to stride w, the second right behind the first (`img1`).  They are copied straight from the caller's strided
// memory, so the host block that the packs fill mirrors the input region from `n` on only (`tail_bytes` of it): pass its start as `tail`.
// `flag` holds matches0 (i32) for the trackers and has_depth (u8) for the stereo entries; the stereo refinement works in place on `rows`
// and `flag` and leaves `kp` and `pred` alone, as the stereo search does `pred`, and only the pyramid tracker writes `levels`.
struct PairStage { size_t img, img1, n, kp, pred, in_bytes, tail_bytes, rows, flag, status, cost, levels, out_bytes, rows_bytes; };
inline PairStage pair_stage(int h, int w, int n) {
  const size_t px = (size_t)h * w, m = (size_t)n;
  StageLayout in, out;
  PairStage s;
  s.rows_bytes = m * 12;
  s.img = in.add(2 * px); s.img1 = s.img + px; s.n = in.add(4); s.kp = in.add(s.rows_bytes); s.pred = in.add(s.rows_bytes); s.in_bytes = in.end;
  s.tail_bytes = s.in_bytes - s.n;
  s.rows = out.add(s.rows_bytes); s.flag = out.add(m * 4); s.status = out.add(m); s.cost = out.add(m * 8); s.levels = out.add(m); s.out_bytes = out.end;
  return s;
}
inline void pair_pack_n(char* tail, int n) {   // the tail starts with the count
  const int32_t n32 = n;
  memcpy(tail, &n32, 4);
}
// (x, y, third) rows out of the caller's strided ones: with `score`, the third float of a keypoint where kp_stride >= 3 (its bits are
// handed on), else 0
inline void pair_pack_kp(char* tail, const PairStage& st, const float* keypoints, int kp_stride, int n, bool score) {
  char* rows = tail + (st.kp - st.n);
  const size_t take = score && kp_stride >= 3 ? 12 : 8;
  memset(rows, 0, st.rows_bytes);
  for (int i = 0; i < n; ++i) memcpy(rows + (size_t)i * 12, keypoints + (size_t)i * kp_stride, take);
}
// (x, y, 0) rows out of pred_stride-strided ones
inline void pair_pack_pred(char* tail, const PairStage& st, const float* pred, int pred_stride, int n) {
  char* rows = tail + (st.pred - st.n);
  memset(rows, 0, st.rows_bytes);
  for (int i = 0; i < n; ++i) memcpy(rows + (size_t)i * 12, pred + (size_t)i * pred_stride, 8);
}

// ---- FAST corners, one image: img [h][w] | n_keep | keep [max_kp][3] -> kp [max_kp][3] | counts (n_out, n_candidates) | carry0 [max_kp] --------
// The image is packed to stride w and copied straight from the caller's strided memory; the host block mirrors the input region from
// `n` on (`tail_bytes` of it).
struct FastStage { size_t img, n, keep, in_bytes, tail_bytes, kp, counts, carry, out_bytes, rows; };
inline FastStage fast_stage(int h, int w, int max_kp) {
  StageLayout in, out;
  FastStage s;
  s.rows = (size_t)max_kp;
  s.img = in.add((size_t)h * w); s.n = in.add(4); s.keep = in.add(s.rows * 12); s.in_bytes = in.end;
  s.tail_bytes = s.in_bytes - s.n;
  s.kp = out.add(s.rows * 12); s.counts = out.add(8); s.carry = out.add(s.rows * 4); s.out_bytes = out.end;
  return s;
}
// the count, then (x, y, score) rows out of the caller's keep_stride-strided ones (keep_stride >= 3); rows from n_keep on stay zero
inline void fast_pack(char* tail, const FastStage& st, const float* keep, int keep_stride, int n_keep) {
  const int32_t n32 = n_keep;
  memcpy(tail, &n32, 4);
  char* rows = tail + (st.keep - st.n);
  for (int i = 0; i < n_keep; ++i) memcpy(rows + (size_t)i * 12, keep + (size_t)i * keep_stride, 12);
}
inline void fast_unpack(const char* out, const FastStage& st, float* kp_out, int32_t* n_out, int32_t* carry0, int32_t* n_candidates) {
  memcpy(kp_out, out + st.kp, st.rows * 12);
  memcpy(n_out, out + st.counts, 4);
  if (n_candidates) memcpy(n_candidates, out + st.counts + 4, 4);
  if (carry0) memcpy(carry0, out + st.carry, st.rows * 4);
}

// ---- binary descriptors, one image: img [h][w] | n | kp [rows][3] -> desc [rows][8] u32 | status [rows] | bin [rows] ---------------------
// rows = n (at least 1, so that no slot is empty); the image as for FAST; the host block mirrors the input region from `n` on.
struct BriefStage { size_t img, n, kp, in_bytes, tail_bytes, desc, status, bin, out_bytes, rows; };
inline BriefStage brief_stage(int h, int w, int n) {
  StageLayout in, out;
  BriefStage s;
  s.rows = (size_t)(n > 0 ? n : 1);
  s.img = in.add((size_t)h * w); s.n = in.add(4); s.kp = in.add(s.rows * 12); s.in_bytes = in.end;
  s.tail_bytes = s.in_bytes - s.n;
  s.desc = out.add(s.rows * 32); s.status = out.add(s.rows); s.bin = out.add(s.rows); s.out_bytes = out.end;
  return s;
}
// the count, then (x, y, 0) rows out of the caller's kp_stride-strided ones (kp_stride >= 2)
inline void brief_pack(char* tail, const BriefStage& st, const float* keypoints, int kp_stride, int n) {
  const int32_t n32 = n;
  memcpy(tail, &n32, 4);
  char* rows = tail + (st.kp - st.n);
  for (int i = 0; i < n; ++i) memcpy(rows + (size_t)i * 12, keypoints + (size_t)i * kp_stride, 8);
}
inline void brief_unpack(const char* out, const BriefStage& st, int n, uint32_t* desc, uint8_t* status, uint8_t* bin) {
  const size_t m = (size_t)n;
  if (!m) return;
  memcpy(desc, out + st.desc, m * 32);
  if (status) memcpy(status, out + st.status, m);
  if (bin) memcpy(bin, out + st.bin, m);
}

// ---- Hamming matcher, one pair: lens [2] | desc [2][max_kp][8] u32 | status [2][max_kp] | kp [2][max_kp][3] -> matches0 | dist0 | mscores0 [max_kp]
// `desc1` / `status1` / `kp1`: where the second set's rows start.  Only the rows in use are packed and copied.
struct HmStage { size_t lens, desc, desc1, status, status1, kp, kp1, in_bytes, m0, dist0, ms0, out_bytes; };
inline HmStage hm_stage(int max_kp) {
  const size_t n = (size_t)max_kp;
  StageLayout in, out;
  HmStage s;
  s.lens = in.add(8); s.desc = in.add(2 * n * 32); s.status = in.add(2 * n); s.kp = in.add(2 * n * 12); s.in_bytes = in.end;
  s.desc1 = s.desc + n * 32; s.status1 = s.status + n; s.kp1 = s.kp + n * 12;
  s.m0 = out.add(n * 4); s.dist0 = out.add(n * 4); s.ms0 = out.add(n * 4); s.out_bytes = out.end;
  return s;
}
// a NULL status array means "every row OK" (the value 1)
inline void hm_pack(char* in, const HmStage& st, int n0, const uint32_t* desc0, const uint8_t* status0, int n1, const uint32_t* desc1,
                    const uint8_t* status1) {
  const int32_t lens[2] = {n0, n1};
  memcpy(in + st.lens, lens, 8);
  if (n0) memcpy(in + st.desc, desc0, (size_t)n0 * 32);
  if (n1) memcpy(in + st.desc1, desc1, (size_t)n1 * 32);
  if (n0) { if (status0) memcpy(in + st.status, status0, (size_t)n0); else memset(in + st.status, 1, (size_t)n0); }
  if (n1) { if (status1) memcpy(in + st.status1, status1, (size_t)n1); else memset(in + st.status1, 1, (size_t)n1); }
}
// the gate's keypoints as (x, y, 0) rows out of the caller's strided ones
inline void hm_pack_kp(char* in, const HmStage& st, const float* kp0, int st0, int n0, const float* kp1, int st1, int n1) {
  char* h0 = in + st.kp;
  char* h1 = in + st.kp1;
  const float zero = 0.f;
  for (int i = 0; i < n0; ++i) { memcpy(h0 + (size_t)i * 12, kp0 + (size_t)i * st0, 8); memcpy(h0 + (size_t)i * 12 + 8, &zero, 4); }
  for (int i = 0; i < n1; ++i) { memcpy(h1 + (size_t)i * 12, kp1 + (size_t)i * st1, 8); memcpy(h1 + (size_t)i * 12 + 8, &zero, 4); }
}
inline void hm_unpack(const char* out, const HmStage& st, int n0, int32_t* matches0, int32_t* dist0, float* mscores0) {
  if (!n0) return;
  memcpy(matches0, out + st.m0, (size_t)n0 * 4);
  memcpy(dist0, out + st.dist0, (size_t)n0 * 4);
  if (mscores0) memcpy(mscores0, out + st.ms0, (size_t)n0 * 4);
}

}  // namespace sship
