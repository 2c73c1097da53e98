// Per-frame benchmark of the HIP front-end on a stereo sequence - the counterpart of the reference's
// examples/stereo/benchmark.cc:46-108 / examples/stereo/kitti.cc:70-129 for the part of SuperSLAM this library replaces
// (SURVEY 8(f) rows 1 and 3).  Per frame it runs exactly StereoFrontEnd's unit of work (src/StereoFrontEnd.cc:10-48):
// extract_stereo, the device LightGlue match, the consumer's disparity gate (uL - uR >= 1, |vL - vR| <= 2) - and, with
// --keyframe-match, the second LightGlue call of the tracker against the previous frame's left features
// (src/VoEstimator.cc:243-246).  Output mirrors the reference benchmark: frames, per-frame ms mean / p50 / p95 / max, fps over
// wall time, the real-time (>= 10 fps) verdict; timing brackets the front-end call only, as the reference times
// `track_stereo` after `cv::imread`.
//
// Input, as the reference's runners read it: <sequence>/times.txt (one timestamp per line; optional here - without it frames
// are read until one is missing), <sequence>/image_0/%06d.png and image_1/%06d.png (8/16-bit gray or RGB PNG, decoded by
// include/superslam_hip/image_io.hpp; .pgm is the fallback extension), or --synthetic N procedurally generated 1376x376 pairs.
//
// Decode runs AHEAD on a second thread, straight into the extractor's pinned upload ring (sship_sp_ring_*): the decoder
// writes pixels into pinned host memory and starts the H2D copy of frame i + 1..i + 3 on the ring's copy stream while the
// tracking thread is still computing frame i; --no-ring uses the copying host API (the reference's in-line staging) instead.
// What this runner does NOT link is the reference's GPU-free core (VoEstimator / WindowSmoother need GTSAM, absent here):
// it produces the StereoFrame inputs, not poses.
//
// build:  g++ -std=c++17 -O2 -Iinclude examples/frontend_benchmark.cc -o frontend_benchmark
//             -Lsuperslam_amd/lib -lsuperslam_hip -Wl,-rpath,$PWD/superslam_amd/lib -Wl,-rpath,/opt/rocm/lib -lpthread -lz
// run:    ./frontend_benchmark --sp sp.safetensors --lg lg.safetensors (--sequence DIR | --synthetic 200) [--keyframe-match]
//                              [--max-kp 600] [--threshold 0.005] [--border 4] [--no-ring] [--no-pipeline] [--bilinear] [--subpixel] [--balanced PX] [--matcher lightglue|nn]
//                              [--dump-keypoints FILE] [--stereo-gate MIN,MAX,ROW] [--track-window R] [--dump DIR] [--strict-ahead]
//
// --matcher nn: the mutual nearest-neighbour matcher (superslam_hip::NNMatcher, hloc's NN-mutual) in LightGlue's place - same
// IFeatureMatcher calls, no --lg needed.  Default: lightglue.
// --stereo-gate MIN,MAX,ROW (with --matcher nn): the stereo match searches the epipolar band only - MIN <= uL - uR <= MAX and
// |vL - vR| <= ROW (NNMatcher::set_stereo_gate) - instead of rejecting impossible partners after they have won a row or a column.  The
// temporal match of --keyframe-match then uses a second NNMatcher without a gate, or with --track-window R one gated (-R, R, -R, R).
// --bilinear: descriptors by upstream SuperPoint's bilinear sampling (SSHIP_DESC_BILINEAR) instead of the reference's nearest-cell gather.
// --subpixel: keypoints refined by the log-parabola peak fit (SSHIP_KP_SUBPIXEL) instead of the reference's integer score-map pixels.
// --balanced PX: keypoints spread over buckets of PX score-map pixels (SSHIP_SELECT_BALANCED) instead of the highest scores of the whole image.
// --dump-keypoints FILE: the first frame's keypoints as int32 n_left, n_right | f32 [n_left][3] (x, y, score) | f32 [n_right][3].
//
// Cross-frame pipelining (default with the ring; --no-pipeline turns it off): as soon as frame t's extraction has returned, frame
// t+1's extraction is ENQUEUED on the extractor's stream (sship_sp_ring_submit) - before frame t's LightGlue match - so the next
// frame's SuperPoint kernels share the GPU with this frame's matcher, whose launches cover a fraction of the CUs at one pair.
// --strict-ahead (ring + pipelining only): before deciding whether to submit frame t+1, the tracking thread waits until that frame
// is decoded or the source is exhausted, so every frame but the last is submitted ahead whatever the decode speed.  It changes
// when work is enqueued and nothing else.
//
// --dump DIR: what the consumer of every frame receives, written to DIR/frames.bin (DIR must exist and be writable) outside the
// timed bracket; no printed statistic changes.  Little-endian, no padding; tests/_runner_dump.py is the reader.
//   file header, 16 bytes : char[4] "SSRF" | u32 version = 1 | u32 descriptor dim (256) | u32 flags (bit 0: --keyframe-match)
//   then one record per frame, in frame order:
//     i32[8]              : frame index, n_left, n_right, n_stereo, n_temporal (-1: no temporal match was run for this frame - no
//                           --keyframe-match, frame 0, or a previous left image without keypoints), submitted_ahead (1: this frame's
//                           extraction had been enqueued by sship_sp_ring_submit before it was collected), 0, 0
//     f32[n_left][3]      : left keypoints (x, y, response)
//     f32[n_right][3]     : right keypoints
//     f32[n_left][256]    : left descriptors, as sship_desc_to_host returns them
//     f32[n_right][256]   : right descriptors
//     n_stereo x 12 bytes : the stereo matches as IFeatureMatcher::match returned them, (i32 queryIdx, i32 trainIdx, f32 distance)
//     u8[n_stereo]        : 1 where the runner's disparity gate (uL - uR >= 1, |vL - vR| <= 2) passed the match
//     n_temporal x 12 bytes (if n_temporal > 0): the temporal matches, query = this frame's left, train = the previous frame's left
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "superslam_hip/frontend.hpp"
#include "superslam_hip/image_io.hpp"
#include "superslam_hip/nn_matcher.hpp"

namespace sh = superslam_hip;

namespace {

// deterministic texture: two octaves of value noise plus filled rectangles (corners for the detector)
void synth_pair(int idx, int rows, int cols, uint8_t* left, uint8_t* right) {
  uint32_t s = 0x9E3779B9u * (uint32_t)(idx + 1);
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };
  const int gw = cols / 16 + 2, gh = rows / 16 + 2;
  std::vector<float> grid((size_t)gw * gh);
  for (auto& g : grid) g = (float)(rnd() & 0xffff) / 65535.f;
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      const float fx = x / 16.f, fy = y / 16.f;
      const int x0 = (int)fx, y0 = (int)fy;
      const float ax = fx - x0, ay = fy - y0;
      const float v = (grid[y0 * gw + x0] * (1 - ax) + grid[y0 * gw + x0 + 1] * ax) * (1 - ay) +
                      (grid[(y0 + 1) * gw + x0] * (1 - ax) + grid[(y0 + 1) * gw + x0 + 1] * ax) * ay;
      left[(size_t)y * cols + x] = (uint8_t)(40.f + 120.f * v);
    }
  for (int r = 0; r < 160; ++r) {
    const int w = 8 + (int)(rnd() % 40), h = 8 + (int)(rnd() % 40);
    const int x0 = (int)(rnd() % (uint32_t)(cols - w)), y0 = (int)(rnd() % (uint32_t)(rows - h));
    const uint8_t c = (uint8_t)(rnd() % 256);
    for (int y = y0; y < y0 + h; ++y) std::memset(&left[(size_t)y * cols + x0], c, (size_t)w);
  }
  const int d = 16 + (int)(rnd() % 3) * 16;  // SuperPoint on synthetic weights is shift-equivariant in 8-px steps
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) right[(size_t)y * cols + x] = left[(size_t)y * cols + std::min(cols - 1, x + d)];
}

float percentile(std::vector<float> v, double p) {  // same definition as the reference benchmark
  if (v.empty()) return 0.f;
  std::sort(v.begin(), v.end());
  return v[std::min(v.size() - 1, (size_t)(p * (v.size() - 1)))];
}

struct Source {
  std::string sequence, ext = "png";
  int synthetic = 0;
  size_t count = 0;  // frames announced by times.txt (0: until a file is missing)
  // frame ni into caller-provided memory of rows * cols bytes each; false at the end of the sequence
  bool load(int ni, int rows, int cols, uint8_t* left, uint8_t* right) const {
    if (synthetic > 0) {
      if (ni >= synthetic) return false;
      // eight distinct pairs, generated once and cycled: "decoding" a synthetic frame then costs a memcpy, like reading an
      // already-decoded image - the procedural generator itself (several ms per pair) would be the slowest stage of the run
      static std::vector<std::vector<uint8_t>> cache;
      static int crows = 0, ccols = 0;
      if (cache.empty() || crows != rows || ccols != cols) {
        cache.assign(16, std::vector<uint8_t>((size_t)rows * cols));
        for (int k = 0; k < 8; ++k) synth_pair(k, rows, cols, cache[2 * k].data(), cache[2 * k + 1].data());
        crows = rows; ccols = cols;
      }
      std::memcpy(left, cache[2 * (ni % 8)].data(), (size_t)rows * cols);
      std::memcpy(right, cache[2 * (ni % 8) + 1].data(), (size_t)rows * cols);
      return true;
    }
    if (count && (size_t)ni >= count) return false;
    char name[32];
    std::snprintf(name, sizeof name, "%06d.%s", ni, ext.c_str());
    int r = 0, c = 0;
    auto into = [&](uint8_t* dst) { return [=](int rr, int cc) -> uint8_t* { return (rr == rows && cc == cols) ? dst : nullptr; }; };
    return sh::read_gray_image(sequence + "/image_0/" + name, r, c, into(left)) &&
           sh::read_gray_image(sequence + "/image_1/" + name, r, c, into(right));
  }
};

}  // namespace

int main(int argc, char** argv) {
  std::string sp_path, lg_path, matcher_name = "lightglue", dump_path, dump_dir;
  Source src;
  int max_kp = 600, border = 4, balanced_px = 0;
  double thr = 0.005;
  bool keyframe = false, use_ring = true, pipeline = true, bilinear = false, subpixel = false, stereo_gate = false, strict_ahead = false, dump_frames = false;
  float gate_min = 0.f, gate_max = 0.f, gate_row = 0.f, track_window = -1.f;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
    if (a == "--sp") sp_path = next();
    else if (a == "--lg") lg_path = next();
    else if (a == "--sequence") src.sequence = next();
    else if (a == "--synthetic") src.synthetic = std::atoi(next());
    else if (a == "--max-kp") max_kp = std::atoi(next());
    else if (a == "--threshold") thr = std::atof(next());
    else if (a == "--border") border = std::atoi(next());
    else if (a == "--keyframe-match") keyframe = true;
    else if (a == "--no-ring") use_ring = false;
    else if (a == "--no-pipeline") pipeline = false;
    else if (a == "--bilinear") bilinear = true;
    else if (a == "--subpixel") subpixel = true;
    else if (a == "--balanced") {
      balanced_px = std::atoi(next());
      if (balanced_px < 8 || balanced_px > 65535) { std::fprintf(stderr, "--balanced needs a bucket size PX in [8, 65535]\n"); return 2; }
    }
    else if (a == "--dump-keypoints") dump_path = next();
    else if (a == "--dump") { dump_dir = next(); dump_frames = true; }
    else if (a == "--strict-ahead") strict_ahead = true;
    else if (a == "--matcher") matcher_name = next();
    else if (a == "--stereo-gate") {
      stereo_gate = std::sscanf(next(), "%f,%f,%f", &gate_min, &gate_max, &gate_row) == 3;
      if (!stereo_gate) { std::fprintf(stderr, "--stereo-gate needs MIN,MAX,ROW\n"); return 2; }
    }
    else if (a == "--track-window") track_window = (float)std::atof(next());
    else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
  }
  const bool use_nn = matcher_name == "nn";
  const bool gated = stereo_gate || track_window >= 0.f;  // the gates belong to the nn matcher
  bool bad_usage = sp_path.empty() || (!use_nn && (lg_path.empty() || matcher_name != "lightglue" || gated)) ||
                   (src.sequence.empty() && src.synthetic <= 0);
  if (strict_ahead && (!use_ring || !pipeline)) {
    std::fprintf(stderr, "--strict-ahead needs the ring and pipelining (not --no-ring / --no-pipeline)\n");
    bad_usage = true;
  }
  std::FILE* dump_file = nullptr;  // --dump DIR: opened before anything else starts, so that an unwritable DIR is bad usage
  if (!bad_usage && dump_frames) {
    dump_file = dump_dir.empty() ? nullptr : std::fopen((dump_dir + "/frames.bin").c_str(), "wb");
    if (!dump_file) { std::fprintf(stderr, "--dump: cannot write %s/frames.bin\n", dump_dir.c_str()); bad_usage = true; }
  }
  if (bad_usage) {
    std::fprintf(stderr, "usage: %s --sp W.safetensors --lg W.safetensors (--sequence DIR | --synthetic N) [--keyframe-match] "
                         "[--max-kp 600] [--threshold 0.005] [--border 4] [--no-ring] [--no-pipeline] [--bilinear] [--subpixel] [--balanced PX] [--matcher lightglue|nn] "
                         "[--dump-keypoints FILE] [--stereo-gate MIN,MAX,ROW] [--track-window R] [--dump DIR] [--strict-ahead] "
                         "(the gates need --matcher nn; --strict-ahead needs the ring and pipelining)\n", argv[0]);
    return 2;
  }
  if (dump_file) {
    const uint32_t hdr[3] = {1u, (uint32_t)sh::SuperPoint::descriptor_dim, keyframe ? 1u : 0u};
    std::fwrite("SSRF", 1, 4, dump_file);
    std::fwrite(hdr, 4, 3, dump_file);
  }

  // ---- frame geometry from the first frame; timestamps as the reference reads them ----
  int rows = 376, cols = 1376;
  std::vector<double> ts;
  if (src.synthetic <= 0) {
    ts = sh::read_times(src.sequence + "/times.txt");
    src.count = ts.size();
    std::vector<uint8_t> probe;
    if (!sh::read_gray_image(src.sequence + "/image_0/000000.png", probe, rows, cols)) {
      src.ext = "pgm";
      if (!sh::read_gray_image(src.sequence + "/image_0/000000.pgm", probe, rows, cols)) {
        std::fprintf(stderr, "Not a KITTI sequence dir (need image_0/000000.png or .pgm): %s\n", src.sequence.c_str());
        return 1;
      }
    }
  }
  sh::SuperPoint extractor(sp_path, max_kp, thr, border);
  sh::LightGlue lightglue(lg_path, cols, rows, max_kp);
  sh::NNMatcher nn(max_kp), nn_track(max_kp);  // nn_track: the temporal match of a gated run (its own window, or none)
  sh::IFeatureMatcher& matcher = use_nn ? static_cast<sh::IFeatureMatcher&>(nn) : lightglue;
  sh::IFeatureMatcher& track_matcher = gated ? static_cast<sh::IFeatureMatcher&>(nn_track) : matcher;
  if (stereo_gate && !nn.set_stereo_gate(gate_min, gate_max, gate_row)) { std::fprintf(stderr, "--stereo-gate: %s\n", nn.last_error().c_str()); return 2; }
  if (track_window >= 0.f && !nn_track.set_gate(-track_window, track_window, -track_window, track_window)) {
    std::fprintf(stderr, "--track-window: %s\n", nn_track.last_error().c_str());
    return 2;
  }
  if (bilinear) extractor.set_descriptor_sampling(SSHIP_DESC_BILINEAR);  // kept, applied by initialize()
  if (subpixel) extractor.set_keypoint_refinement(SSHIP_KP_SUBPIXEL);
  if (balanced_px) extractor.set_keypoint_selection(SSHIP_SELECT_BALANCED, balanced_px);
  if (!extractor.initialize() || !(use_nn ? nn.initialize() : lightglue.initialize()) || (gated && keyframe && !nn_track.initialize())) {
    std::fprintf(stderr, "initialisation failed: %s\n", sship_last_error());
    return 1;
  }
  constexpr int kDepth = 4;
  if (use_ring && !extractor.ring_create(kDepth, rows, cols, 1)) {
    std::fprintf(stderr, "upload ring: %s\n", extractor.last_error().c_str());
    return 1;
  }

  // ---- decode-ahead producer: frame ni -> ring slot ni % kDepth (pinned memory) -> asynchronous upload ----
  std::vector<std::vector<uint8_t>> plain(use_ring ? 0 : 2 * kDepth, std::vector<uint8_t>((size_t)rows * cols));
  std::mutex mu;
  std::condition_variable cv_free, cv_ready;
  int produced = 0, consumed = 0;  // frames decoded / frames whose slot has been handed back
  bool done = false;
  std::thread producer([&]() {
    for (int ni = 0;; ++ni) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_free.wait(lk, [&] { return ni - consumed < kDepth; });  // the slot's previous frame has been extracted
      }
      const int slot = ni % kDepth;
      uint8_t* l = use_ring ? extractor.ring_host(slot, 0) : plain[2 * slot].data();
      uint8_t* r = use_ring ? extractor.ring_host(slot, 1) : plain[2 * slot + 1].data();
      if (!src.load(ni, rows, cols, l, r)) break;
      if (use_ring) extractor.ring_upload(slot);
      std::lock_guard<std::mutex> lk(mu);
      produced = ni + 1;
      cv_ready.notify_one();
    }
    std::lock_guard<std::mutex> lk(mu);
    done = true;
    cv_ready.notify_one();
  });

  std::vector<float> ms;
  long stereo_points = 0, stereo_matches = 0, track_matches = 0, submitted_ahead = 0;
  sh::Features prev_left;
  bool was_submitted = false;         // this frame's extraction was enqueued ahead, during the previous frame
  std::vector<uint8_t> gate_passed;   // --dump: the gate's decision per stereo match
  const auto wall0 = std::chrono::steady_clock::now();
  for (int ni = 0;; ++ni) {
    {
      std::unique_lock<std::mutex> lk(mu);
      cv_ready.wait(lk, [&] { return produced > ni || done; });
      if (produced <= ni) break;
    }
    const int slot = ni % kDepth;
    const bool submitted_this = was_submitted;
    was_submitted = false;
    const auto t1 = std::chrono::steady_clock::now();
    std::pair<sh::Features, sh::Features> feats;
    if (use_ring) {
      feats = extractor.extract_stereo_ring(slot);   // a submitted slot: waits for its completion event only
      if (pipeline) {  // frame ni + 1 already decoded and uploading?  enqueue its extraction now, ahead of this frame's match
        bool have_next;
        {
          std::unique_lock<std::mutex> lk(mu);
          if (strict_ahead) cv_ready.wait(lk, [&] { return produced > ni + 1 || done; });  // the decoder is at most kDepth - 1 frames ahead: no deadlock
          have_next = produced > ni + 1;
        }
        if (have_next && extractor.ring_submit((ni + 1) % kDepth)) { ++submitted_ahead; was_submitted = true; }
      }
    } else feats = extractor.extract_stereo(sh::Image{plain[2 * slot].data(), rows, cols, 1, 0}, sh::Image{plain[2 * slot + 1].data(), rows, cols, 1, 0});
    if (ni == 0 && !dump_path.empty()) {
      std::FILE* o = std::fopen(dump_path.c_str(), "wb");
      if (!o) std::fprintf(stderr, "cannot write %s\n", dump_path.c_str());  // the run goes on: the decoder thread is live
      else {
        const int32_t n[2] = {(int32_t)feats.first.keypoints.size(), (int32_t)feats.second.keypoints.size()};
        std::fwrite(n, 4, 2, o);
        for (const sh::Features* ft : {&feats.first, &feats.second})
          for (const sh::KeyPoint& k : ft->keypoints) { const float v[3] = {k.x, k.y, k.response}; std::fwrite(v, 4, 3, o); }
        std::fclose(o);
      }
    }
    sh::MatchResult lr = matcher.match(feats.first.keypoints, feats.first.descriptors, feats.second.keypoints, feats.second.descriptors);
    if (dump_file) gate_passed.assign(lr.matches.size(), 0);
    for (size_t i = 0; i < lr.matches.size(); ++i) {  // StereoFrontEnd's gate
      const sh::DMatch& m = lr.matches[i];
      const sh::KeyPoint &kl = feats.first.keypoints[m.queryIdx], &kr = feats.second.keypoints[m.trainIdx];
      if (kl.x - kr.x >= 1.0f && std::abs(kl.y - kr.y) <= 2.0f) {
        ++stereo_points;
        if (dump_file) gate_passed[i] = 1;
      }
    }
    stereo_matches += (long)lr.matches.size();
    sh::MatchResult tr;
    const bool tracked = keyframe && !prev_left.descriptors.empty();
    if (tracked) {
      tr = track_matcher.match(feats.first.keypoints, feats.first.descriptors, prev_left.keypoints, prev_left.descriptors);
      track_matches += (long)tr.matches.size();
    }
    const auto t2 = std::chrono::steady_clock::now();
    ms.push_back((float)std::chrono::duration_cast<std::chrono::microseconds>(t2 - t1).count() / 1000.0f);
    if (dump_file) {  // outside the timed bracket; layout in the header comment
      const int32_t rec[8] = {ni, (int32_t)feats.first.keypoints.size(), (int32_t)feats.second.keypoints.size(), (int32_t)lr.matches.size(),
                              tracked ? (int32_t)tr.matches.size() : -1, submitted_this ? 1 : 0, 0, 0};
      std::fwrite(rec, 4, 8, dump_file);
      for (const sh::Features* ft : {&feats.first, &feats.second})
        for (const sh::KeyPoint& k : ft->keypoints) { const float v[3] = {k.x, k.y, k.response}; std::fwrite(v, 4, 3, dump_file); }
      for (const sh::Features* ft : {&feats.first, &feats.second}) {
        const sh::HostDescriptors hd = matcher.descriptors_to_host(ft->descriptors);
        std::fwrite(hd.data.data(), 4, hd.data.size(), dump_file);
      }
      auto write_matches = [&](const sh::MatchResult& r) {
        for (const sh::DMatch& m : r.matches) {
          const int32_t qt[2] = {m.queryIdx, m.trainIdx};
          std::fwrite(qt, 4, 2, dump_file);
          std::fwrite(&m.distance, 4, 1, dump_file);
        }
      };
      write_matches(lr);
      std::fwrite(gate_passed.data(), 1, gate_passed.size(), dump_file);
      write_matches(tr);
    }
    if (keyframe) prev_left = std::move(feats.first);  // holds its pool slot until the next frame replaces it
    {
      std::lock_guard<std::mutex> lk(mu);
      consumed = ni + 1;  // the extract call that read this slot has returned: the decoder may overwrite it
      cv_free.notify_one();
    }
  }
  const double wall = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - wall0).count() / 1000.0;
  producer.join();
  if (dump_file) {
    const bool failed = std::ferror(dump_file) != 0;
    if (std::fclose(dump_file) != 0 || failed) { std::fprintf(stderr, "--dump: writing %s/frames.bin failed\n", dump_dir.c_str()); return 1; }
  }
  if (ms.empty()) { std::fprintf(stderr, "no frames\n"); return 1; }

  const double mean = std::accumulate(ms.begin(), ms.end(), 0.0) / ms.size();
  std::printf("=========== SuperSLAM HIP front-end benchmark ===========\n");
  std::printf("source           : %s, %dx%d, %s%s\n", src.synthetic > 0 ? "synthetic" : (src.ext == "png" ? "PNG sequence" : "PGM sequence"), cols, rows,
              use_ring ? "pinned upload ring" : "copying host API", ts.empty() ? "" : ", times.txt");
  std::printf("frames           : %zu\n", ms.size());
  if (use_nn) std::printf("matcher          : nn (mutual nearest neighbour)\n");
  if (stereo_gate) std::printf("stereo gate      : %g <= uL - uR <= %g, |vL - vR| <= %g\n", gate_min, gate_max, gate_row);
  if (track_window >= 0.f) std::printf("track window     : +-%g px\n", track_window);
  if (subpixel) std::printf("keypoints        : sub-pixel (SSHIP_KP_SUBPIXEL)\n");
  if (balanced_px) std::printf("selection        : balanced over %d px buckets (SSHIP_SELECT_BALANCED)\n", balanced_px);
  if (use_ring) std::printf("pipelined        : %s (%ld of %zu extractions enqueued one frame ahead)\n", pipeline ? "yes" : "no", submitted_ahead, ms.size());
  std::printf("per-frame ms      mean=%.2f p50=%.2f p95=%.2f max=%.2f\n", mean, percentile(ms, 0.50), percentile(ms, 0.95), percentile(ms, 1.0));
  std::printf("throughput        : %.2f fps over %.1fs wall\n", wall > 0 ? ms.size() / wall : 0.0, wall);
  std::printf("real-time (>=10fps): %s\n", mean > 0 && (1000.0 / mean) >= 10.0 ? "YES" : "NO");
  if (!ts.empty() && ts.size() >= ms.size() && ms.size() > 1)
    std::printf("sequence rate     : %.2f fps (times.txt), processed at %.1fx real time\n", (ms.size() - 1) / (ts[ms.size() - 1] - ts[0]),
                (ts[ms.size() - 1] - ts[0]) / std::max(1e-9, wall));
  std::printf("stereo matches    : %.1f per frame, %.1f pass the disparity gate\n", (double)stereo_matches / ms.size(), (double)stereo_points / ms.size());
  if (keyframe) std::printf("keyframe matches  : %.1f per frame\n", ms.size() > 1 ? (double)track_matches / (ms.size() - 1) : 0.0);
  std::printf("=========================================================\n");
  return 0;
}
