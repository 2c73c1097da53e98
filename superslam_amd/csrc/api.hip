// C ABI of libsuperslam_hip.so (include/sship.h): weights, workspaces, streams and the launch sequences of
// the SuperPoint extractor, the LightGlue matcher and the fused front-end step.  gfx950 only; there is no CPU
// fallback anywhere in this library - without a GPU every entry point fails with SSHIP_ERR_NO_DEVICE.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/sship.h"
#include "../../include/superslam_hip/place_recognizer.hpp"
#include "brief_pattern.h"
#include "kernels.h"
#include "stage_layout.h"

namespace sship {

static thread_local std::string g_err;
static void (*g_log_cb)(int, const char*) = nullptr;
static int g_profiling = 0;  // 0 off, 1 stage marks, 2 stage marks + one mark per SuperPoint layer launch (sship_set_profiling)

void set_error(const std::string& msg) {
  g_err = msg;
  if (g_log_cb) g_log_cb(4, msg.c_str());
}
void log_msg(int level, const char* fmt, ...) {
  if (!g_log_cb) return;
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_log_cb(level, buf);
}
static int fail(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

// ------------------------------------------------------------------------------------------------
// device memory helper
// ------------------------------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; bytes = 0;
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};
struct PinBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~PinBuf() { if (p) (void)hipHostFree(p); }
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr; bytes = 0;
    hipError_t e = hipHostMalloc(&p, n, hipHostMallocDefault);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};
// One staged item (csrc/stage_layout.h): the layout's input region, then its output region from `out` on, in one device block.  A handle
// mirrors it slot for slot in one pinned block, so an offset names the same field on both sides; a per-call arena has no mirror.
struct StageArena {
  DevBuf d;
  PinBuf h;
  size_t out = 0;
  hipError_t create(size_t in_bytes, size_t out_bytes, bool pinned = true) {
    out = StageLayout{in_bytes}.add(0);
    hipError_t e = d.ensure(out + out_bytes);
    if (e == hipSuccess && pinned) e = h.ensure(out + out_bytes);
    return e;
  }
  template <class T> T* dev(size_t off) const { return reinterpret_cast<T*>(d.as<char>() + off); }
  template <class T> T* host(size_t off) const { return reinterpret_cast<T*>(h.as<char>() + off); }
  hipError_t upload(size_t off, size_t bytes, hipStream_t s) const { return hipMemcpyAsync(dev<char>(off), host<char>(off), bytes, hipMemcpyHostToDevice, s); }
  hipError_t download(size_t off, size_t bytes, hipStream_t s) const { return hipMemcpyAsync(host<char>(off), dev<char>(off), bytes, hipMemcpyDeviceToHost, s); }
};

// ------------------------------------------------------------------------------------------------
// safetensors reader (8-byte LE header length, JSON header, raw little-endian tensor data)
// ------------------------------------------------------------------------------------------------
struct Tensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  size_t numel() const { size_t n = 1; for (auto d : shape) n *= (size_t)d; return n; }
};
typedef std::map<std::string, Tensor> StateDict;

static float half_bits_to_float(uint16_t h) {
  const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1f;
  uint32_t m = h & 0x3ffu, u;
  if (e == 0) {
    if (m == 0) u = s;
    else {
      int sh = 0;
      while (!(m & 0x400u)) { m <<= 1; ++sh; }
      u = s | ((uint32_t)(113 - sh) << 23) | ((m & 0x3ffu) << 13);
    }
  } else if (e == 31) u = s | 0x7f800000u | (m << 13);
  else u = s | ((e + 112) << 23) | (m << 13);
  float f; memcpy(&f, &u, 4); return f;
}

static bool load_safetensors(const std::string& path, StateDict& sd, std::string& err) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { err = "cannot open weights file '" + path + "'"; return false; }
  uint64_t hlen = 0;
  f.read(reinterpret_cast<char*>(&hlen), 8);
  if (!f || hlen == 0 || hlen > (1ull << 28)) { err = "bad safetensors header in '" + path + "'"; return false; }
  std::string js(hlen, '\0');
  f.read(&js[0], (std::streamsize)hlen);
  std::vector<char> blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  // Minimal parser for {"name": {"dtype": "F32", "shape": [..], "data_offsets": [a, b]}, ...}
  size_t i = 0;
  auto skip_ws = [&]() { while (i < js.size() && (js[i] == ' ' || js[i] == '\n' || js[i] == '\t' || js[i] == '\r')) ++i; };
  auto parse_str = [&](std::string& out) -> bool {
    skip_ws();
    if (i >= js.size() || js[i] != '"') return false;
    ++i; out.clear();
    while (i < js.size() && js[i] != '"') { if (js[i] == '\\' && i + 1 < js.size()) ++i; out.push_back(js[i++]); }
    ++i; return true;
  };
  auto skip_value = [&]() {  // skip a JSON value (used for __metadata__)
    skip_ws();
    int depth = 0; bool in_str = false;
    for (; i < js.size(); ++i) {
      const char c = js[i];
      if (in_str) { if (c == '\\') ++i; else if (c == '"') in_str = false; continue; }
      if (c == '"') in_str = true;
      else if (c == '{' || c == '[') ++depth;
      else if (c == '}' || c == ']') { if (--depth == 0) { ++i; return; } }
      else if ((c == ',') && depth == 0) return;
    }
  };
  skip_ws();
  if (i >= js.size() || js[i] != '{') { err = "safetensors header is not an object"; return false; }
  ++i;
  while (true) {
    skip_ws();
    if (i < js.size() && js[i] == '}') break;
    std::string name;
    if (!parse_str(name)) { err = "safetensors header parse error"; return false; }
    skip_ws();
    if (js[i] != ':') { err = "safetensors header parse error (:)"; return false; }
    ++i;
    if (name == "__metadata__") { skip_value(); }
    else {
      skip_ws();
      if (js[i] != '{') { err = "safetensors entry parse error"; return false; }
      ++i;
      std::string dtype; std::vector<int64_t> shape; uint64_t off0 = 0, off1 = 0;
      while (true) {
        skip_ws();
        if (js[i] == '}') { ++i; break; }
        std::string key;
        if (!parse_str(key)) { err = "safetensors entry key parse error"; return false; }
        skip_ws(); ++i;  // ':'
        skip_ws();
        if (key == "dtype") { parse_str(dtype); }
        else if (key == "shape" || key == "data_offsets") {
          ++i;  // '['
          std::vector<int64_t> vals;
          while (true) {
            skip_ws();
            if (js[i] == ']') { ++i; break; }
            if (js[i] == ',') { ++i; continue; }
            vals.push_back(strtoll(js.c_str() + i, nullptr, 10));
            while (i < js.size() && (isdigit((unsigned char)js[i]) || js[i] == '-')) ++i;
          }
          if (key == "shape") shape = vals;
          else if (vals.size() == 2) { off0 = (uint64_t)vals[0]; off1 = (uint64_t)vals[1]; }
        } else skip_value();
        skip_ws();
        if (js[i] == ',') ++i;
      }
      Tensor t; t.shape = shape;
      const size_t n = t.numel();
      if (off1 > blob.size() || off1 < off0) { err = "tensor '" + name + "' exceeds file"; return false; }
      t.data.resize(n);
      if (dtype == "F32" && off1 - off0 == n * 4) memcpy(t.data.data(), blob.data() + off0, n * 4);
      else if (dtype == "F16" && off1 - off0 == n * 2) {
        const uint16_t* h = reinterpret_cast<const uint16_t*>(blob.data() + off0);
        for (size_t k = 0; k < n; ++k) t.data[k] = half_bits_to_float(h[k]);
      } else if (dtype == "I64" || dtype == "I32" || dtype == "U8" || dtype == "BOOL" || dtype == "I16" || dtype == "I8") {
        skip_ws();
        if (i < js.size() && js[i] == ',') ++i;
        continue;  // bookkeeping tensors (BatchNorm.num_batches_tracked ...): not weights
      } else { err = "tensor '" + name + "': unsupported dtype " + dtype; return false; }
      sd[name] = std::move(t);
    }
    skip_ws();
    if (i < js.size() && js[i] == ',') ++i;
  }
  return true;
}

static const Tensor* find_tensor(const StateDict& sd, const std::string& name, std::initializer_list<int64_t> shape,
                                 std::string& err) {
  auto it = sd.find(name);
  if (it == sd.end()) { err = "missing tensor '" + name + "'"; return nullptr; }
  if (it->second.shape != std::vector<int64_t>(shape)) { err = "tensor '" + name + "' has the wrong shape"; return nullptr; }
  return &it->second;
}

// ------------------------------------------------------------------------------------------------
// weight packing into MFMA A-fragment order (igemm.h):
//   [cout_blk][cin_chunk][ky][kx][kstep][mtile][lane][8]  with
//   cout = cb*CT + mt*32 + (lane & 31),  cin = chunk*64 + ks*16 + (lane >> 5)*8 + e
// `w` is [cout][cin][ks][ks] row-major (PyTorch Conv2d / Linear); row_map/scale allow host-side row
// permutation and folding of constant factors.
// ------------------------------------------------------------------------------------------------
// tile_interleave: M-tile mt of row block cb holds logical rows (mt * nblocks + cb) * 32 .. + 31 instead of
// cb * ct + mt * 32 .. (the fused projection of the LightGlue FFN kernel: every wave then owns one 32-row tile of
// EACH of the q / k / v segments, so all waves have the same epilogue work).  The bias stays in logical order.
static std::vector<_Float16> pack_conv(const float* w, int cout, int cin, int ks, int ct, int chunk, const std::vector<int>* row_map,
                                       const std::vector<float>* row_scale, bool tile_interleave);
static int upload_conv(const float* w, const float* bias, int cout, int cin, int ks, int ct, ConvW& out,
                       const std::vector<int>* row_map = nullptr, const std::vector<float>* row_scale = nullptr,
                       bool tile_interleave = false) {
  const int cout_pad = (cout + ct - 1) / ct * ct, mt_n = ct / 32, nchunk = cin / 64;
  const int nblocks = cout_pad / ct;
  std::vector<_Float16> pk((size_t)cout_pad * cin * ks * ks);
  size_t o = 0;
  for (int cb = 0; cb < cout_pad / ct; ++cb)
    for (int ch = 0; ch < nchunk; ++ch)
      for (int ky = 0; ky < ks; ++ky)
        for (int kx = 0; kx < ks; ++kx)
          for (int kstep = 0; kstep < 4; ++kstep)
            for (int mt = 0; mt < mt_n; ++mt)
              for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                  const int co = tile_interleave ? (mt * nblocks + cb) * 32 + (lane & 31) : cb * ct + mt * 32 + (lane & 31);
                  const int ci = ch * 64 + kstep * 16 + (lane >> 5) * 8 + e;
                  float v = 0.f;
                  if (co < cout) {
                    const int src = row_map ? (*row_map)[co] : co;
                    v = w[(((size_t)src * cin + ci) * ks + ky) * ks + kx];
                    if (row_scale) v *= (*row_scale)[co];
                  }
                  pk[o++] = (_Float16)v;
                }
  std::vector<float> bp(cout_pad, 0.f);
  for (int co = 0; co < cout; ++co) {
    const int src = row_map ? (*row_map)[co] : co;
    bp[co] = bias ? bias[src] * (row_scale ? (*row_scale)[co] : 1.f) : 0.f;
  }
  // a failure part-way leaves nothing behind (the caller's error path only frees what `out` still points to)
  auto fail_free = [&](hipError_t e, const char* what) {
    if (out.w) (void)hipFree(out.w);
    if (out.bias) (void)hipFree(out.bias);
    out.w = nullptr; out.bias = nullptr;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return (int)SSHIP_ERR_HIP;
  };
  out.w = nullptr; out.bias = nullptr;
  hipError_t e;
  if ((e = hipMalloc(reinterpret_cast<void**>(&out.w), pk.size() * sizeof(_Float16))) != hipSuccess) return fail_free(e, "upload_conv: hipMalloc(weights)");
  if ((e = hipMalloc(reinterpret_cast<void**>(&out.bias), bp.size() * sizeof(float))) != hipSuccess) return fail_free(e, "upload_conv: hipMalloc(bias)");
  if ((e = hipMemcpy(out.w, pk.data(), pk.size() * sizeof(_Float16), hipMemcpyHostToDevice)) != hipSuccess) return fail_free(e, "upload_conv: hipMemcpy(weights)");
  if ((e = hipMemcpy(out.bias, bp.data(), bp.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return fail_free(e, "upload_conv: hipMemcpy(bias)");
  out.cin = cin; out.cout = cout; out.cout_pad = cout_pad; out.ks = ks; out.ct = ct;
  return SSHIP_OK;
}
static void free_conv(ConvW& c) {
  if (c.w) (void)hipFree(c.w);
  if (c.w_q) (void)hipFree(c.w_q);
  if (c.w_wino) (void)hipFree(c.w_wino);
  if (c.bias) (void)hipFree(c.bias);
  c.w = nullptr; c.w_q = nullptr; c.w_wino = nullptr; c.bias = nullptr;
}
// the same fragment order with a K chunk of `chunk` channels: [cout_blk][cin / chunk][ky][kx][k-step chunk / 16][m-tile][lane][8]
static std::vector<_Float16> pack_conv(const float* w, int cout, int cin, int ks, int ct, int chunk, const std::vector<int>* row_map,
                                       const std::vector<float>* row_scale, bool /*tile_interleave*/) {
  const int cout_pad = (cout + ct - 1) / ct * ct, mt_n = ct / 32;
  std::vector<_Float16> pk((size_t)cout_pad * cin * ks * ks);
  size_t o = 0;
  for (int cb = 0; cb < cout_pad / ct; ++cb)
    for (int ch = 0; ch < cin / chunk; ++ch)
      for (int ky = 0; ky < ks; ++ky)
        for (int kx = 0; kx < ks; ++kx)
          for (int kstep = 0; kstep < chunk / 16; ++kstep)
            for (int mt = 0; mt < mt_n; ++mt)
              for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                  const int co = cb * ct + mt * 32 + (lane & 31);
                  const int ci = ch * chunk + kstep * 16 + (lane >> 5) * 8 + e;
                  float v = 0.f;
                  if (co < cout) {
                    const int src = row_map ? (*row_map)[co] : co;
                    v = w[(((size_t)src * cin + ci) * ks + ky) * ks + kx];
                    if (row_scale) v *= (*row_scale)[co];
                  }
                  pk[o++] = (_Float16)v;
                }
  return pk;
}
// Winograd F(2x2, 3x3) weights of a 64 -> 64 layer for conv_wino.hip: U_p = (G g G^T)[xi][nu], p = 4 xi + nu, computed in fp32 and
// rounded to fp16, packed as MFMA A fragments [p 16][chunk 4][m 2][lane 64][8]: cout = 32 m + (lane & 31), cin = 16 chunk + 8 (lane >> 5) + e
[[maybe_unused]] static int upload_wino(const float* w, ConvW& out) {
  static const float G[4][3] = {{1.f, 0.f, 0.f}, {.5f, .5f, .5f}, {.5f, -.5f, .5f}, {0.f, 0.f, 1.f}};
  std::vector<_Float16> pk((size_t)16 * 4 * 2 * 512);
  for (int co = 0; co < 64; ++co)
    for (int ci = 0; ci < 64; ++ci) {
      const float* g = w + ((size_t)co * 64 + ci) * 9;
      float Gg[4][3], U[4][4];
      for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 3; ++k) Gg[i][k] = G[i][0] * g[0 * 3 + k] + G[i][1] * g[1 * 3 + k] + G[i][2] * g[2 * 3 + k];
      for (int i = 0; i < 4; ++i)
        for (int jn = 0; jn < 4; ++jn) U[i][jn] = Gg[i][0] * G[jn][0] + Gg[i][1] * G[jn][1] + Gg[i][2] * G[jn][2];
      const int m = co >> 5, chunk = ci >> 4, lane = (co & 31) + 32 * ((ci & 15) >> 3), e = ci & 7;
      for (int p = 0; p < 16; ++p) pk[(((size_t)p * 4 + chunk) * 2 + m) * 512 + lane * 8 + e] = (_Float16)U[p >> 2][p & 3];
    }
  SSHIP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&out.w_wino), pk.size() * sizeof(_Float16)));
  SSHIP_HIP_CHECK(hipMemcpy(out.w_wino, pk.data(), pk.size() * sizeof(_Float16), hipMemcpyHostToDevice));
  return SSHIP_OK;
}
// second packing of a 128-input-channel 3x3 layer for conv_pp128.hip (64-row cout tiles, 32-channel chunks)
static int upload_conv_q(const float* w, int cout, int cin, ConvW& out) {
  const std::vector<_Float16> pk = pack_conv(w, cout, cin, 3, 64, 32, nullptr, nullptr, false);
  SSHIP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&out.w_q), pk.size() * sizeof(_Float16)));
  SSHIP_HIP_CHECK(hipMemcpy(out.w_q, pk.data(), pk.size() * sizeof(_Float16), hipMemcpyHostToDevice));
  return SSHIP_OK;
}
static int upload_floats(const float* src, size_t n, float** dst) {
  *dst = nullptr;
  SSHIP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(dst), n * sizeof(float)));
  if (hipError_t e = hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice)) {
    (void)hipFree(*dst); *dst = nullptr;
    set_error(std::string("upload_floats: ") + hipGetErrorString(e));
    return SSHIP_ERR_HIP;
  }
  return SSHIP_OK;
}

static std::atomic<bool> g_inited{false};
static std::atomic<int> g_device{-1};  // the device sship_init selected; every API entry binds the calling thread to it
static std::mutex g_init_mu;           // sship_init may race between the tracking and the loop-closure thread
// HIP's current device is per thread and defaults to 0: a second caller thread (the reference's loop-closure worker,
// SuperSLAM.cc:129-133) on a rank that owns device != 0 would otherwise launch on the wrong GPU.
static inline void bind_thread() {
  static thread_local bool bound = false;
  const int dev = g_device.load(std::memory_order_acquire);
  if (!bound && dev >= 0) { (void)hipSetDevice(dev); bound = true; }
}
static int require_device() {
  if (g_inited.load(std::memory_order_acquire)) return SSHIP_OK;
  return sship_init(-1);
}

// the two events of a measurement hook: destroyed whichever way the hook returns
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

// The timing every measurement hook shares: `run` once to warm up, then `iters` times between two events; *avg_ms = elapsed / iters.
template <class Run>
static int bench_loop(hipStream_t s, int iters, Run run, float* avg_ms) {
  SSHIP_HIP_CHECK(run());  // warm
  EventPair ev;
  SSHIP_HIP_CHECK(hipEventCreate(&ev.e0));
  SSHIP_HIP_CHECK(hipEventCreate(&ev.e1));
  SSHIP_HIP_CHECK(hipEventRecord(ev.e0, s));
  for (int i = 0; i < iters; ++i) SSHIP_HIP_CHECK(run());
  SSHIP_HIP_CHECK(hipEventRecord(ev.e1, s));
  SSHIP_HIP_CHECK(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  SSHIP_HIP_CHECK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *avg_ms = ms / iters;
  return SSHIP_OK;
}

// The measurement hook of the handles that keep their last call's arguments in `last` (nn, index, pose, ransac, ba, pg): `run` holds the
// handle's only launch call and is re-run on the handle's stream.  `who` is the entry's name, `verb` what the caller has to run first.
template <class Handle>
static int bench_last(Handle* h, int iters, float* avg_ms, const char* who, const char* verb,
                      hipError_t (*run)(const Handle*, const typename Handle::Last&, hipStream_t)) {
  if (!h || !avg_ms || iters <= 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": bad arguments");
  if (h->last.items <= 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": run a " + verb + " on this handle first");
  bind_thread();
  SSHIP_HIP_CHECK(hipDeviceSynchronize());  // the last call may have run on the caller's stream
  return bench_loop(h->stream, iters, [&]() { return run(h, h->last, h->stream); }, avg_ms);
}
// the two parameter checks the iterative solvers (pose, ba, pg) word alike
static int check_lambda(const char* who, double lambda0, double lambda_max) {
  if (!(lambda0 > 0.0) || lambda_max < lambda0 || std::isinf(lambda_max))
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": lambda0 must be > 0 and lambda_max finite and >= lambda0");
  return SSHIP_OK;
}
static int check_max_iterations(const char* who, int max_iterations) {
  if (max_iterations < 1) return fail(SSHIP_ERR_INVALID, std::string(who) + ": max_iterations must be >= 1");
  return SSHIP_OK;
}

// What the handles with nothing but a stream and RAII members to release share (nn, index, pose, ransac, ba, pg, rect).
template <class Handle>
static void destroy_handle(Handle* h) {
  if (!h) return;
  bind_thread();
  (void)hipDeviceSynchronize();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// The rectified stereo camera of the pose-only solver and the window smoother; `who` is the entry's name in the messages.
struct StereoCamera {
  bool set = false;
  double fx = 0, fy = 0, cx = 0, cy = 0, baseline = 0;
};
static int camera_set(StereoCamera* cam, const char* who, double fx, double fy, double cx, double cy, double baseline) {
  if (!cam) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null handle");
  if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy) || !std::isfinite(baseline))
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": every camera value must be finite");
  if (!(fx > 0.0) || !(fy > 0.0) || !(baseline > 0.0)) return fail(SSHIP_ERR_INVALID, std::string(who) + ": fx, fy and baseline must be > 0");
  *cam = StereoCamera{true, fx, fy, cx, cy, baseline};
  return SSHIP_OK;
}
static int camera_get(const StereoCamera* cam, const char* who, double* fx, double* fy, double* cx, double* cy, double* baseline) {
  if (!cam) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null handle");
  if (!cam->set) return fail(SSHIP_ERR_INVALID, std::string(who) + ": no camera has been set");
  if (fx) *fx = cam->fx;
  if (fy) *fy = cam->fy;
  if (cx) *cx = cam->cx;
  if (cy) *cy = cam->cy;
  if (baseline) *baseline = cam->baseline;
  return SSHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// stage timers (off by default)
// ------------------------------------------------------------------------------------------------
// One timer per calling THREAD (thread_local): the tracking thread and the loop-closure thread each own a handle
//  and may both have profiling on; sship_get_stage_timings reports the calling thread's last sequence.
// Labels are "<reference profile scope>:<stage>" - the scopes are the reference's own SUPERSLAM_PROFILE labels
// (sp_gpu_infer src/SuperPoint.cc:639, sp_extract_stereo :904, fe_lg_stereo_match src/StereoFrontEnd.cc:32), the part
// after the colon is this library's finer split of that scope.
struct StageTimer {
  std::vector<std::pair<const char*, hipEvent_t>> marks;
  std::vector<std::pair<std::string, float>> last;
  // No destructor work: a thread_local's destructor can run after the HIP runtime has been torn down (process exit,
  // or a thread that outlives hipDeviceReset) and hipEventDestroy there is undefined; at most 64 events leak per thread.
  void begin(hipStream_t s) { if (!g_profiling) return; clear(); mark("start", s); }
  // a matcher entered on its own (no extractor call in front of it on this thread) opens its own sequence
  void begin_if_idle(hipStream_t s) { if (g_profiling && marks.empty()) mark("start", s); }
  void mark(const char* label, hipStream_t s) {
    if (!g_profiling) return;
    if (marks.size() >= 64) {  // nobody collected: do not accumulate events without bound; re-arm so the next interval
      clear();                 // is measured from here, not from an arbitrary earlier stage
      hipEvent_t e0;
      if (hipEventCreate(&e0) == hipSuccess) { (void)hipEventRecord(e0, s); marks.push_back({"start", e0}); }
    }
    hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, s); marks.push_back({label, e});
  }
  // per-layer marks (level 2 only)
  void mark_fine(const char* label, hipStream_t s) { if (g_profiling >= 2) mark(label, s); }
  void clear() { for (auto& m : marks) (void)hipEventDestroy(m.second); marks.clear(); }
  void collect() {
    if (marks.size() < 2) return;
    (void)hipEventSynchronize(marks.back().second);
    last.clear();
    for (size_t i = 1; i < marks.size(); ++i) {
      float ms = 0.f; (void)hipEventElapsedTime(&ms, marks[i - 1].second, marks[i].second);
      last.push_back({marks[i].first, ms});
    }
    clear();
  }
};
static thread_local StageTimer g_timer;

}  // namespace sship

using namespace sship;

// ====================================================================================================
// runtime
// ====================================================================================================
extern "C" int sship_version(void) { return SSHIP_VERSION; }
extern "C" const char* sship_last_error(void) { return g_err.c_str(); }
extern "C" void sship_set_log_callback(void (*cb)(int, const char*)) { g_log_cb = cb; }
extern "C" void sship_set_profiling(int level) { g_profiling = level < 0 ? 0 : level > 2 ? 2 : level; }
extern "C" int sship_get_stage_timings(const char** labels, float* ms, int max_stages) {
  bind_thread();
  g_timer.collect();
  int n = 0;
  for (auto& kv : g_timer.last) {
    if (n >= max_stages) break;
    labels[n] = kv.first.c_str(); ms[n] = kv.second; ++n;
  }
  return n;
}
extern "C" int sship_init(int device) {
  std::lock_guard<std::mutex> init_guard(g_init_mu);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(SSHIP_ERR_NO_DEVICE, "no HIP device visible: libsuperslam_hip has no CPU path");
  if (device < 0) {
    const char* env = getenv("SUPERSLAM_HIP_DEVICE");
    device = env ? atoi(env) : -1;
  }
  if (device >= 0) {
    if (device >= count) return fail(SSHIP_ERR_INVALID, "device index out of range");
    SSHIP_HIP_CHECK(hipSetDevice(device));
  }
  int cur = 0;
  SSHIP_HIP_CHECK(hipGetDevice(&cur));
  hipDeviceProp_t prop;
  SSHIP_HIP_CHECK(hipGetDeviceProperties(&prop, cur));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SSHIP_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  g_device.store(cur, std::memory_order_release);
  g_inited.store(true, std::memory_order_release);
  log_msg(2, "sship: device %d %s, %d CUs", cur, prop.gcnArchName, prop.multiProcessorCount);
  return SSHIP_OK;
}
extern "C" int sship_device_synchronize(void) {
  bind_thread();
  SSHIP_HIP_CHECK(hipDeviceSynchronize());
  return SSHIP_OK;
}

// ====================================================================================================
// descriptor pool  (include/DescriptorPool.h:13-91, src/DescriptorPool.cc:10-38)
// ====================================================================================================
// The bookkeeping (free-list + mutex) is reference counted separately from the device slots, like the reference's
// shared_ptr<FreeList> (DescriptorPool.h:71-75): a DeviceDescriptors handle may outlive the extractor that owns the pool.
// sship_pool_destroy frees the DEVICE memory (DescriptorPool.cc:27-32 - a surviving handle's data pointer dangles exactly
// as in the reference) and drops the owner's reference; the struct itself dies with the last handle reference, so a late
// sship_pool_release never touches freed host memory.
struct sship_pool {
  int max_keypoints = 0, dim = 0;
  size_t slot_bytes = 0;
  std::vector<void*> slots;     // nullptr once destroyed
  std::vector<int> free_slots;  // LIFO (FreeList)
  mutable std::mutex mu;        // handles may be released from another thread (async keyframe copies)
  std::atomic<int> refs{1};     // owner + one per live handle (sship_pool_retain)
};
extern "C" int sship_pool_create(int num_slots, int max_keypoints, int dim, sship_pool** out) {
  bind_thread();
  if (!out || num_slots <= 0 || max_keypoints <= 0 || dim <= 0) return fail(SSHIP_ERR_INVALID, "pool_create: bad arguments");
  if (int rc = require_device()) return rc;
  auto* p = new sship_pool();
  p->max_keypoints = max_keypoints; p->dim = dim;
  p->slot_bytes = (size_t)max_keypoints * dim * sizeof(_Float16);
  p->slots.assign(num_slots, nullptr);
  for (int i = num_slots - 1; i >= 0; --i) p->free_slots.push_back(i);  // DescriptorPool.h:27-29
  for (int i = 0; i < num_slots; ++i)
    if (hipMalloc(&p->slots[i], p->slot_bytes) != hipSuccess) {
      sship_pool_destroy(p);
      return fail(SSHIP_ERR_NOMEM, "pool_create: hipMalloc failed");
    }
  *out = p;
  return SSHIP_OK;
}
extern "C" void sship_pool_retain(sship_pool* pool) {
  if (pool) pool->refs.fetch_add(1, std::memory_order_relaxed);
}
extern "C" void sship_pool_release_ref(sship_pool* pool) {
  if (pool && pool->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete pool;
}
extern "C" void sship_pool_destroy(sship_pool* pool) {
  bind_thread();
  if (!pool) return;
  {
    std::lock_guard<std::mutex> g(pool->mu);
    for (void*& s : pool->slots) { if (s) (void)hipFree(s); s = nullptr; }
  }
  sship_pool_release_ref(pool);
}
extern "C" int sship_pool_acquire(sship_pool* pool) {
  bind_thread();
  if (!pool) return -1;
  std::lock_guard<std::mutex> g(pool->mu);
  if (pool->free_slots.empty()) return -1;
  const int s = pool->free_slots.back();
  pool->free_slots.pop_back();
  return s;
}
extern "C" void sship_pool_release(sship_pool* pool, int slot) {
  bind_thread();
  if (!pool || slot < 0 || slot >= (int)pool->slots.size()) return;
  std::lock_guard<std::mutex> g(pool->mu);
  pool->free_slots.push_back(slot);
}
extern "C" int sship_pool_in_use(const sship_pool* pool) {
  bind_thread();
  if (!pool) return 0;
  std::lock_guard<std::mutex> g(pool->mu);
  return (int)pool->slots.size() - (int)pool->free_slots.size();
}
extern "C" void* sship_pool_slot_ptr(const sship_pool* pool, int slot) {
  bind_thread();
  if (!pool || slot < 0 || slot >= (int)pool->slots.size()) return nullptr;
  std::lock_guard<std::mutex> g(pool->mu);
  return pool->slots[slot];
}

// ====================================================================================================
// gather / nms / select stage entry points
// ====================================================================================================
extern "C" int sship_gather_normalize(const void* grid, int channels, int gh, int gw, const int* cell_h,
                                      const int* cell_w, int n, void* out, void* stream) {
  bind_thread();
  if (n <= 0) return SSHIP_OK;  // DescriptorGather.cu:69
  if (!grid || !cell_h || !cell_w || !out || channels <= 0) return fail(SSHIP_ERR_INVALID, "gather_normalize: null argument");
  if (int rc = require_device()) return rc;
  launch_gather_chw(static_cast<const _Float16*>(grid), channels, gh, gw, cell_h, cell_w, n,
                    static_cast<_Float16*>(out), static_cast<hipStream_t>(stream));
  SSHIP_HIP_CHECK(hipGetLastError());
  return SSHIP_OK;
}
extern "C" int sship_gather_normalize_hwc(const void* grid, int channels, int gh, int gw, const int* cell_h,
                                          const int* cell_w, int n, void* out, void* stream) {
  bind_thread();
  if (n <= 0) return SSHIP_OK;
  if (!grid || !cell_h || !cell_w || !out) return fail(SSHIP_ERR_INVALID, "gather_normalize_hwc: null argument");
  if (channels <= 0 || channels > 256 || channels % 4) return fail(SSHIP_ERR_INVALID, "gather_normalize_hwc: channels must be <= 256 and a multiple of 4");
  if (int rc = require_device()) return rc;
  launch_gather_hwc(false, static_cast<const _Float16*>(grid), channels, gh, gw, 0, cell_h, cell_w, nullptr, n, n, 1,
                    static_cast<_Float16*>(out), static_cast<hipStream_t>(stream));
  SSHIP_HIP_CHECK(hipGetLastError());
  return SSHIP_OK;
}
static int sample_bilinear(bool hwc, const void* grid, int channels, int gh, int gw, const float* kp_xy, int n, void* out, void* stream) {
  bind_thread();
  if (n <= 0) return SSHIP_OK;
  if (!grid || !kp_xy || !out) return fail(SSHIP_ERR_INVALID, "sample_descriptors_bilinear: null argument");
  if (channels <= 0 || channels > 256 || (hwc && channels % 4)) return fail(SSHIP_ERR_INVALID, "sample_descriptors_bilinear: channels must be in [1, 256] (a multiple of 4 for the channels-last grid)");
  if (gh <= 0 || gw <= 0) return fail(SSHIP_ERR_INVALID, "sample_descriptors_bilinear: empty grid");
  if (int rc = require_device()) return rc;
  if (hwc) launch_sample_bilinear_hwc(static_cast<const _Float16*>(grid), channels, gh, gw, kp_xy, n, static_cast<_Float16*>(out), static_cast<hipStream_t>(stream));
  else launch_sample_bilinear_chw(static_cast<const _Float16*>(grid), channels, gh, gw, kp_xy, n, static_cast<_Float16*>(out), static_cast<hipStream_t>(stream));
  SSHIP_HIP_CHECK(hipGetLastError());
  return SSHIP_OK;
}
extern "C" int sship_sample_descriptors_bilinear(const void* grid, int channels, int gh, int gw, const float* kp_xy, int n, void* out,
                                                 void* stream) {
  return sample_bilinear(false, grid, channels, gh, gw, kp_xy, n, out, stream);
}
extern "C" int sship_sample_descriptors_bilinear_hwc(const void* grid, int channels, int gh, int gw, const float* kp_xy, int n, void* out,
                                                     void* stream) {
  return sample_bilinear(true, grid, channels, gh, gw, kp_xy, n, out, stream);
}
static int refine_stage(const float* logits, size_t cell_stride, size_t chan_stride, int Hc, int Wc, const int* pix, int n, float* offsets, void* stream) {
  bind_thread();
  if (n <= 0) return SSHIP_OK;
  if (!logits || !pix || !offsets) return fail(SSHIP_ERR_INVALID, "refine_keypoints: null argument");
  if (Hc < 1 || Wc < 1 || Hc > 8191 || Wc > 8191) return fail(SSHIP_ERR_INVALID, "refine_keypoints: the cell grid must be 1 .. 8191 cells a side");
  if (int rc = require_device()) return rc;
  KpRefineArgs a{};
  a.logits = logits; a.img_stride = 0; a.cell_stride = cell_stride; a.chan_stride = chan_stride; a.Hc = Hc; a.Wc = Wc;
  a.pix = pix; a.n_dev = nullptr; a.n_host = n; a.max_kp = n; a.offsets = offsets;
  launch_kp_refine(a, 1, static_cast<hipStream_t>(stream));
  SSHIP_HIP_CHECK(hipGetLastError());
  return SSHIP_OK;
}
extern "C" int sship_refine_keypoints(const float* logits_chw, int Hc, int Wc, const int* pix, int n, float* offsets, void* stream) {
  return refine_stage(logits_chw, 1, (size_t)(Hc > 0 ? Hc : 0) * (size_t)(Wc > 0 ? Wc : 0), Hc, Wc, pix, n, offsets, stream);
}
extern "C" int sship_refine_keypoints_hwc(const float* logits, int row_stride, int Hc, int Wc, const int* pix, int n, float* offsets,
                                          void* stream) {
  if (n > 0 && row_stride < 65) { bind_thread(); return fail(SSHIP_ERR_INVALID, "refine_keypoints_hwc: row_stride must be at least 65"); }
  return refine_stage(logits, (size_t)(row_stride > 0 ? row_stride : 0), 1, Hc, Wc, pix, n, offsets, stream);
}
extern "C" int sship_nms(const float* scores, int batch, int h, int w, int radius, float* out, void* stream) {
  bind_thread();
  if (!scores || !out || batch <= 0 || h <= 0 || w <= 0) return fail(SSHIP_ERR_INVALID, "nms: bad arguments");
  if (radius < 0 || radius > 8) return fail(SSHIP_ERR_INVALID, "nms: radius must be in [0, 8]");
  if (int rc = require_device()) return rc;
  NmsArgs a{};
  a.scores_in = scores; a.B = batch; a.H = h; a.W = w; a.radius = radius; a.scores_out = out;
  launch_nms_tile(1, a, static_cast<hipStream_t>(stream));
  SSHIP_HIP_CHECK(hipGetLastError());
  return SSHIP_OK;
}
extern "C" int sship_select_topk(const float* scores, int score_h, int score_w, int input_h, int input_w, double thr,
                                 int border, int max_kp, int desc_h, int desc_w, float* kp_xys, int* cell_h,
                                 int* cell_w, int* n_dev, int* n_cand_dev, void* stream) {
  bind_thread();
  if (!scores || !kp_xys || !cell_h || !cell_w || !n_dev || score_h <= 0 || score_w <= 0)
    return fail(SSHIP_ERR_INVALID, "select_topk: bad arguments");
  if (max_kp <= 0 || max_kp > kMaxKp) return fail(SSHIP_ERR_INVALID, "select_topk: max_kp must be in [1, 4096]");
  if (int rc = require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cap = score_h * score_w;
  DevBuf cand, cnt;
  SSHIP_HIP_CHECK(cand.ensure((size_t)cap * 8));
  SSHIP_HIP_CHECK(cnt.ensure(4));
  SSHIP_HIP_CHECK(hipMemsetAsync(cnt.p, 0, 4, s));
  launch_threshold_scan(scores, score_h, score_w, threshold_as_float(thr), border, cand.as<unsigned long long>(),
                        cnt.as<int>(), cap, s);
  TopkArgs t{};
  t.cand = cand.as<unsigned long long>(); t.cand_count = cnt.as<int>(); t.cap = cap; t.max_kp = max_kp;
  t.score_w = score_w;
  t.scale_x = static_cast<float>(input_w) / score_w;  // SuperPoint.cc:707-708
  t.scale_y = static_cast<float>(input_h) / score_h;
  t.desc_h = desc_h; t.desc_w = desc_w; t.kp_xys = kp_xys; t.cell_h = cell_h; t.cell_w = cell_w; t.n_out = n_dev;
  t.n_cand_out = n_cand_dev;
  launch_topk(t, 1, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));  // scratch buffers die with this scope
  return SSHIP_OK;
}

// ====================================================================================================
// SuperPoint
// ====================================================================================================
struct sship_sp {
  sship_sp_config cfg{};
  hipStream_t stream = nullptr;
  float* w1a = nullptr;  // [9][64] tap-major fp32 (fp16-rounded values)  (stand-alone conv1a kernel)
  float* b1a = nullptr;
  _Float16* w1a_frag = nullptr;   // conv1a as MFMA A fragments [2][64][8] (K = 9 taps zero-padded to 16)
  _Float16* w1a_fragb = nullptr;  // ping-pong kernel: taps 0..4 | taps 5..8 + the bias split into fp16 hi/lo parts (see sship_sp_create)
  ConvW c1b, c2a, c2b, c3a, c3b, c4a, c4b, cPa, cPb, cDa, cDb;
  ConvW cDb32;  // convDb packed in 32-row blocks (one per wave of k_desc_head_gather)
  sship_pool* pool = nullptr;
  // activations (channels-last fp16), sized for (B, H, W)
  int wsB = 0, wsH = 0, wsW = 0;
  DevBuf img, a1a, a1b, a2a, a2b, a3a, a3b, a4a, a4b, aPa, aDa, draw, logits, cand, cand_count;
  const void* cand_zero_ptr = nullptr; int cand_zero_n = 0;  // cand_count[0 .. cand_zero_n) of this allocation are known to be zero (sp_select) ...
  hipStream_t cand_zero_stream = nullptr;                      // ... for work ordered after the last k_topk on THIS stream
  DevBuf kp, cell_h, cell_w, n_dev, desc_stage, gray_in;
  int desc_sampling = SSHIP_DESC_NEAREST;  // sship_sp_set_descriptor_sampling
  int kp_refinement = SSHIP_KP_INTEGER;    // sship_sp_set_keypoint_refinement
  int kp_selection = SSHIP_SELECT_TOPK;    // sship_sp_set_keypoint_selection
  int bucket_px = 32;                      // G of the balanced mode (and of sship_sp_bench_layer 17 in either mode)
  DevBuf sel, sel_count, sel_ws;           // balanced mode only: [B, max_kp] selected keys, [B] their counts, k_select_balanced's workspace
  DevBuf pix;                              // [B, max_kp] score-map pixels of the keypoints (h << 16 | w): written by k_topk in bilinear / sub-pixel mode only
  PinBuf h_kp, h_n, h_img;
  int cap = 0;
  float thr_f = 0.f;
  bool img_valid = false;  // sp->img holds the pixels of the last call (host-image paths always; batch path under profiling)
  // decode-ahead upload ring (sship_sp_ring_*): `depth` stereo frames in pinned host memory + their device copies
  struct Ring {
    int depth = 0, h = 0, w = 0, ch = 0;
    size_t img_bytes = 0;
    std::vector<void*> host, dev;     // [depth]: left image then right image, contiguous
    std::vector<hipEvent_t> uploaded;  // [depth]
    hipStream_t copy_stream = nullptr;
    // sship_sp_ring_submit: an extraction enqueued ahead of the call that collects it
    struct Pending { bool active = false; int slots[2] = {-1, -1}; int rc_pool = 0; hipEvent_t done = nullptr; void* h_kp = nullptr; void* h_n = nullptr; };
    std::vector<Pending> pending;      // [depth]
  } ring;
};

static void ring_free(sship_sp* sp);
static void sp_shapes(int H, int W, int& H2, int& W2, int& H4, int& W4, int& Hc, int& Wc) {
  H2 = H / 2; W2 = W / 2; H4 = H2 / 2; W4 = W2 / 2; Hc = H4 / 2; Wc = W4 / 2;  // MaxPool2d(2,2) floors
}

// Balanced selection: the second key list, its counters and the kernel's workspace, for B images of a map of Hc x Wc cells.  The workspace is
// sized for the finest bucket (8 px: one bucket per cell), so a later change of bucket_px never allocates.  Grows only; the default mode never
// calls it, and a handle that never leaves the default mode never holds these buffers.
struct SelWs { unsigned long long* seg; unsigned long long* bnd; int* tab; };
static size_t sel_ws_layout(const DevBuf& ws, int B, int cap, int nb_max, SelWs* out) {
  const size_t seg = (size_t)B * cap * 8, bnd = (size_t)B * nb_max * 8, tab = (size_t)B * nb_max * 4;
  if (out) {
    char* p = static_cast<char*>(ws.p);
    out->seg = reinterpret_cast<unsigned long long*>(p);
    out->bnd = reinterpret_cast<unsigned long long*>(p + seg);
    out->tab = reinterpret_cast<int*>(p + seg + bnd);
  }
  return seg + bnd + tab;
}
static int sp_ensure_balanced(sship_sp* sp, int B, int Hc, int Wc) {
  const int mk = sp->cfg.max_keypoints;
  SSHIP_HIP_CHECK(sp->sel.ensure((size_t)B * mk * 8));
  SSHIP_HIP_CHECK(sp->sel_count.ensure((size_t)B * 4));
  SSHIP_HIP_CHECK(sp->sel_ws.ensure(sel_ws_layout(sp->sel_ws, B, Hc * 8 * Wc * 8, Hc * Wc, nullptr)));
  return SSHIP_OK;
}
static SelectBalancedArgs select_balanced_args(const unsigned long long* cand, const int* cand_count, int cap, int max_kp, int score_h, int score_w,
                                               int bucket_px, unsigned long long* sel, int* sel_count, const SelWs& ws) {
  SelectBalancedArgs q{};
  q.cand = cand; q.cand_count = cand_count; q.cap = cap; q.max_kp = max_kp; q.score_w = score_w; q.bucket_px = bucket_px;
  q.nbx = (score_w + bucket_px - 1) / bucket_px;
  q.nb = q.nbx * ((score_h + bucket_px - 1) / bucket_px);
  q.sel = sel; q.sel_count = sel_count; q.n_cand_out = nullptr;
  q.ws_seg = ws.seg; q.ws_bnd = ws.bnd; q.ws_tab = ws.tab;
  return q;
}

static int sp_ensure(sship_sp* sp, int B, int H, int W) {
  if (sp->kp_selection == SSHIP_SELECT_BALANCED) {
    int H2, W2, H4, W4, Hc, Wc;
    sp_shapes(H, W, H2, W2, H4, W4, Hc, Wc);
    if (Hc >= 1 && Wc >= 1)
      if (int rc = sp_ensure_balanced(sp, B > sp->wsB ? B : sp->wsB, Hc, Wc)) return rc;
  }
  if (B <= sp->wsB && H == sp->wsH && W == sp->wsW) return SSHIP_OK;
  int H2, W2, H4, W4, Hc, Wc;
  sp_shapes(H, W, H2, W2, H4, W4, Hc, Wc);
  if (Hc < 1 || Wc < 1) return fail(SSHIP_ERR_INVALID, "image too small for SuperPoint (needs >= 8x8)");
  const size_t px1 = (size_t)B * H * W, px2 = (size_t)B * H2 * W2, px4 = (size_t)B * H4 * W4, pxc = (size_t)B * Hc * Wc;
  const int mk = sp->cfg.max_keypoints;
  SSHIP_HIP_CHECK(sp->img.ensure(px1));
  SSHIP_HIP_CHECK(sp->gray_in.ensure(px1 * 3));
  SSHIP_HIP_CHECK(sp->a1a.ensure(px1 * 64 * 2));
  SSHIP_HIP_CHECK(sp->a1b.ensure(px2 * 64 * 2));
  SSHIP_HIP_CHECK(sp->a2a.ensure(px2 * 64 * 2));
  SSHIP_HIP_CHECK(sp->a2b.ensure(px4 * 64 * 2));
  SSHIP_HIP_CHECK(sp->a3a.ensure(px4 * 128 * 2));
  SSHIP_HIP_CHECK(sp->a3b.ensure(pxc * 128 * 2));
  SSHIP_HIP_CHECK(sp->a4a.ensure(pxc * 128 * 2));
  SSHIP_HIP_CHECK(sp->a4b.ensure(pxc * 128 * 2));
  SSHIP_HIP_CHECK(sp->aPa.ensure(pxc * 256 * 2));
  SSHIP_HIP_CHECK(sp->aDa.ensure(pxc * 256 * 2));
  SSHIP_HIP_CHECK(sp->draw.ensure(pxc * 256 * 2));
  SSHIP_HIP_CHECK(sp->logits.ensure(pxc * kLogitStride * 4));
  sp->cap = Hc * 8 * Wc * 8;
  SSHIP_HIP_CHECK(sp->cand.ensure((size_t)B * sp->cap * 8));
  SSHIP_HIP_CHECK(sp->cand_count.ensure((size_t)B * 4));
  SSHIP_HIP_CHECK(sp->kp.ensure((size_t)B * mk * 3 * 4));
  SSHIP_HIP_CHECK(sp->cell_h.ensure((size_t)B * mk * 4));
  SSHIP_HIP_CHECK(sp->cell_w.ensure((size_t)B * mk * 4));
  SSHIP_HIP_CHECK(sp->pix.ensure((size_t)B * mk * 4));
  SSHIP_HIP_CHECK(sp->n_dev.ensure((size_t)B * 4));
  SSHIP_HIP_CHECK(sp->h_kp.ensure((size_t)B * mk * 3 * 4));
  SSHIP_HIP_CHECK(sp->h_n.ensure((size_t)B * 4));
  SSHIP_HIP_CHECK(sp->h_img.ensure(px1 * 3));
  sp->wsB = B; sp->wsH = H; sp->wsW = W;
  return SSHIP_OK;
}

// 3x3 conv kernel selection.  Default: the ping-pong kernel (conv_pp.hip) for every layer; SUPERSLAM_HIP_CONV=strip
// runs the lock-step strip kernel instead (conv_strip.hip, kept for A/B runs: profiles/r01_pp_vs_strip.txt).
static int conv_mode() {  // 1 ping-pong (default), 2 strip (developer build only)
  static const int v = [] {
    const char* e = dev_env("SUPERSLAM_HIP_CONV");
    return (SSHIP_DEV_SWITCHES && e && std::string(e) == "strip") ? 2 : 1;
  }();
  return v;
}
static hipError_t conv3(const ConvW& w, const _Float16* in, _Float16* out, int B, int H, int W, bool pool, hipStream_t s) {
#if SSHIP_DEV_SWITCHES
  // SUPERSLAM_HIP_CONV64=wino: conv2a / conv2b as Winograd F(2x2, 3x3) (conv_wino.hip; A/B)
  static const bool wino = [] { const char* e = dev_env("SUPERSLAM_HIP_CONV64"); return e && std::string(e) == "wino"; }();
  if (wino && w.w_wino && sp_conv3x3_wino_fits(H, W, w.cin, w.cout)) return sp_conv3x3_wino(w.w_wino, w.bias, in, out, B, H, W, pool, s);
  return conv_mode() == 1 ? sp_conv3x3_pp(w, in, out, B, H, W, pool, s) : sp_conv3x3_strip(w, in, out, B, H, W, pool, s);
#else
  return sp_conv3x3_pp(w, in, out, B, H, W, pool, s);
#endif
}
// conv2a + conv2b + pool run as ONE launch (conv_fuse2.hip) at every batch size - the strips are cut into as many row segments as it takes to give
// every CU work, so a one-pair call gains as well (0.736 -> 0.710 ms) - unless the shape does not fit the kernel (maps under 8 pixels, images beyond
// 32-bit offsets): then, and in the developer build under SUPERSLAM_HIP_CONV2=split (A/B; tests/test_gpu_alt_paths.py), the two conv3x3_pp launches run.
// Both paths give the same bits.  (sship_sp_debug_activation layer 2 = conv2a's map exists only on the two-launch path, which the shipped
// library does take where the fused kernel does not fit: an 8x8 image, for one.)
static bool conv2_fused(int B, int H2, int W2) {
#if SSHIP_DEV_SWITCHES
  static const std::string mode = [] { const char* e = dev_env("SUPERSLAM_HIP_CONV2"); return std::string(e ? e : ""); }();
  static const bool other = [] { const char* e = dev_env("SUPERSLAM_HIP_CONV64"); return e != nullptr; }();
  if (mode == "split" || other || conv_mode() != 1) return false;
#endif
  return sp_conv2ab_fused_fits(B, H2, W2, true);
}
// conv3a (64 -> 128) runs on conv3x3_pp<64, 64> (two cout tiles).  The rolling-window kernel's one-layer form (conv_fuse2.hip: conv_roll<true>, all 128
// output channels in one launch, weights in registers) is bit-identical and draws the SAME joules (0.7276 vs 0.7274 J per 128-image launch,
// profiles/r06_l_*): it exists in the developer build only (SUPERSLAM_HIP_CONV3A=roll; A/B in tests/test_gpu_alt_paths.py).
static hipError_t conv3a_layer(const ConvW& w, const _Float16* in, _Float16* out, int B, int H, int W, hipStream_t s) {
#if SSHIP_DEV_SWITCHES
  static const bool roll = [] { const char* e = dev_env("SUPERSLAM_HIP_CONV3A"); return e && std::string(e) == "roll"; }();
  if (roll && conv_mode() == 1 && w.cin == 64 && w.cout == 128 && w.ct == 64 && sp_conv3a_roll_fits(B, H, W)) return sp_conv3a_roll(w, in, out, B, H, W, s);
#endif
  return conv3(w, in, out, B, H, W, false, s);
}
static hipError_t conv1ab(sship_sp* sp, const uint8_t* img, _Float16* out, int B, int H, int W, hipStream_t s);
static bool desc_dense_mode() {
  static const bool v = [] { const char* e = dev_env("SUPERSLAM_HIP_DESC"); return e && std::string(e) == "dense"; }();
  return v;
}
// descriptor rows of the selected keypoints of `B` images (cells / counts at the given pointers; the cells are the handle's, from image img0 on)
static hipError_t desc_head(sship_sp* sp, int img0, int Hc, int Wc, const int* cell_h, const int* cell_w, const int* n_dev, int B,
                            _Float16* out, size_t out_img_stride, hipStream_t s) {
  const int mk = sp->cfg.max_keypoints;
  if (sp->desc_sampling == SSHIP_DESC_BILINEAR)  // the corner variant of the sparse head, at the pixels the same k_topk launch left in sp->pix
    return launch_desc_head_sparse_bilinear(sp->cDa, sp->cDb32, sp->a4b.as<_Float16>() + (size_t)img0 * Hc * Wc * 128, Hc, Wc,
                                            sp->pix.as<int>() + (cell_h - sp->cell_h.as<int>()), n_dev, mk, B, out, out_img_stride, s);
  if (desc_dense_mode()) {
    launch_desc_head_gather(sp->cDb32, sp->aDa.as<_Float16>() + (size_t)img0 * Hc * Wc * 256, Hc, Wc, cell_h, cell_w, n_dev, mk, B, out,
                            out_img_stride, s);
    return hipGetLastError();
  }
  return launch_desc_head_sparse(sp->cDa, sp->cDb32, sp->a4b.as<_Float16>() + (size_t)img0 * Hc * Wc * 128, Hc, Wc, cell_h, cell_w, n_dev,
                                 mk, B, out, out_img_stride, s);
}

// encoder + both heads up to (logits, raw descriptor grid).  utils/convert_superpoint_to_onnx.py:51-64,77,88.
static int sp_network(sship_sp* sp, const uint8_t* imgs, int B, int H, int W, hipStream_t s, bool dense_desc) {
  int H2, W2, H4, W4, Hc, Wc;
  sp_shapes(H, W, H2, W2, H4, W4, Hc, Wc);
  // conv1a is evaluated inside conv1b's tile staging (conv_pp.hip): the 64-channel full-resolution activation
  // never exists in HBM.
  // level-2 profiling: one mark per launch, labelled "<level-1 label>/<layer>" ("sp_gpu_infer:encoder/conv2a", ...,
  // "sp_gpu_infer:encoder/conv4b", "sp_gpu_infer:heads/convPb", "sp_extract_stereo:select/topk").  At level 2 NO entry
  // carries the bare level-1 label: a stage's level-1 time is the SUM over its "<label>/..." entries (what bench.py does)
  SSHIP_HIP_CHECK(conv1ab(sp, imgs, sp->a1b.as<_Float16>(), B, H, W, s));
  g_timer.mark_fine("sp_gpu_infer:encoder/conv1a+conv1b+pool", s);
  if (conv2_fused(B, H2, W2)) {
    // conv2a -> conv2b -> pool in one launch, the map between them never leaves the CU (conv_fuse2.hip; bit-identical to the two launches below)
    SSHIP_HIP_CHECK(sp_conv2ab_fused(sp->c2a, sp->c2b, sp->a1b.as<_Float16>(), sp->a2b.as<_Float16>(), B, H2, W2, s));
    g_timer.mark_fine("sp_gpu_infer:encoder/conv2a+conv2b+pool", s);
  } else {
    SSHIP_HIP_CHECK(conv3(sp->c2a, sp->a1b.as<_Float16>(), sp->a2a.as<_Float16>(), B, H2, W2, false, s));
    g_timer.mark_fine("sp_gpu_infer:encoder/conv2a", s);
    SSHIP_HIP_CHECK(conv3(sp->c2b, sp->a2a.as<_Float16>(), sp->a2b.as<_Float16>(), B, H2, W2, true, s));
    g_timer.mark_fine("sp_gpu_infer:encoder/conv2b+pool", s);
  }
  SSHIP_HIP_CHECK(conv3a_layer(sp->c3a, sp->a2b.as<_Float16>(), sp->a3a.as<_Float16>(), B, H4, W4, s));
  g_timer.mark_fine("sp_gpu_infer:encoder/conv3a", s);
  SSHIP_HIP_CHECK(conv3(sp->c3b, sp->a3a.as<_Float16>(), sp->a3b.as<_Float16>(), B, H4, W4, true, s));
  g_timer.mark_fine("sp_gpu_infer:encoder/conv3b+pool", s);
  SSHIP_HIP_CHECK(conv3(sp->c4a, sp->a3b.as<_Float16>(), sp->a4a.as<_Float16>(), B, Hc, Wc, false, s));
  g_timer.mark_fine("sp_gpu_infer:encoder/conv4a", s);
  SSHIP_HIP_CHECK(conv3(sp->c4b, sp->a4a.as<_Float16>(), sp->a4b.as<_Float16>(), B, Hc, Wc, false, s));
  g_timer.mark(g_profiling >= 2 ? "sp_gpu_infer:encoder/conv4b" : "sp_gpu_infer:encoder", s);
  SSHIP_HIP_CHECK(conv3(sp->cPa, sp->a4b.as<_Float16>(), sp->aPa.as<_Float16>(), B, Hc, Wc, false, s));
  g_timer.mark_fine("sp_gpu_infer:heads/convPa", s);
  SSHIP_HIP_CHECK(sp_conv1x1_f32(sp->cPb, sp->aPa.as<_Float16>(), sp->logits.as<float>(), kLogitStride, B, Hc, Wc, s));
  // the dense descriptor branch (convDa, convDb) is only materialised for the dense API; extraction evaluates both
  // layers at the selected keypoints (k_desc_head_sparse).  SUPERSLAM_HIP_DESC=dense: dense convDa + gather (A/B runs).
  if (dense_desc || desc_dense_mode()) SSHIP_HIP_CHECK(conv3(sp->cDa, sp->a4b.as<_Float16>(), sp->aDa.as<_Float16>(), B, Hc, Wc, false, s));
  if (dense_desc) SSHIP_HIP_CHECK(sp_conv1x1_f16(sp->cDb, sp->aDa.as<_Float16>(), sp->draw.as<_Float16>(), B, Hc, Wc, s));
  g_timer.mark(g_profiling >= 2 ? "sp_gpu_infer:heads/convPb" : "sp_gpu_infer:heads", s);
  return SSHIP_OK;
}

// k_topk writes the packed score-map pixels only for the modes that read them
static bool sp_wants_pix(const sship_sp* sp) { return sp->desc_sampling == SSHIP_DESC_BILINEAR || sp->kp_refinement == SSHIP_KP_SUBPIXEL; }
// sub-pixel mode: overwrite x, y of the keypoints of `B` images (kp [B, max_kp, 3], counts on the device) - k_kp_refine
static hipError_t sp_refine(sship_sp* sp, int B, int Hc, int Wc, float* kp, const int* n_dev, float scale_x, float scale_y, hipStream_t s) {
  KpRefineArgs r{};
  r.logits = sp->logits.as<float>(); r.img_stride = (size_t)Hc * Wc * kLogitStride; r.cell_stride = kLogitStride; r.chan_stride = 1;
  r.Hc = Hc; r.Wc = Wc; r.pix = sp->pix.as<int>(); r.n_dev = n_dev; r.n_host = 0; r.max_kp = sp->cfg.max_keypoints;
  r.kp_xys = kp; r.scale_x = scale_x; r.scale_y = scale_y; r.offsets = nullptr;
  launch_kp_refine(r, B, s);
  return hipGetLastError();
}
// heatmap softmax + NMS + threshold -> candidates -> top-k keypoints/cells (all on device).
// The last three arguments are for sship_sp_debug_select alone (every product call leaves them null: its two launches get the arguments they
// always got): other logits than sp->logits [B][Hc][Wc][kLogitStride], the pre-NMS softmax map [B][8Hc][8Wc], the candidate counts [B].
static int sp_select(sship_sp* sp, int B, int H, int W, float* scores_out, float* kp_out, int* n_out, hipStream_t s,
                     const float* logits = nullptr, float* raw_out = nullptr, int* n_cand_out = nullptr) {
  int H2, W2, H4, W4, Hc, Wc;
  sp_shapes(H, W, H2, W2, H4, W4, Hc, Wc);
  // The candidate counters are zeroed by k_topk once it has read them (a 5-us memset launch per call in latency mode otherwise);
  // a memset is needed only for a fresh / regrown buffer or after a call that did not get as far as its k_topk launch.
  // the counters are zero for THIS call only if the k_topk that zeroed them ran on the same stream (a call on another stream is not
  // ordered behind it: it clears its own, as every call did before the reset moved into k_topk)
  if (sp->cand_zero_ptr != sp->cand_count.p || sp->cand_zero_n < B || sp->cand_zero_stream != s)
    SSHIP_HIP_CHECK(hipMemsetAsync(sp->cand_count.p, 0, (size_t)B * 4, s));
  sp->cand_zero_ptr = sp->cand_count.p; sp->cand_zero_n = 0; sp->cand_zero_stream = s;
  NmsArgs a{};
  a.logits = logits ? logits : sp->logits.as<float>(); a.ls = kLogitStride; a.B = B; a.H = Hc * 8; a.W = Wc * 8;
  a.radius = sp->cfg.nms_radius; a.thr_f = sp->thr_f; a.border = sp->cfg.remove_borders;
  a.cand = sp->cand.as<unsigned long long>(); a.cand_count = sp->cand_count.as<int>(); a.cap = sp->cap;
  a.scores_out = scores_out; a.scores_raw_out = raw_out;
  launch_nms_tile(0, a, s);
  g_timer.mark_fine("sp_extract_stereo:select/nms_tile", s);
  TopkArgs t{};
  t.cand = a.cand; t.cand_count = a.cand_count; t.cap = sp->cap; t.max_kp = sp->cfg.max_keypoints;
  t.score_w = Wc * 8;
  t.scale_x = static_cast<float>(W) / (Wc * 8);
  t.scale_y = static_cast<float>(H) / (Hc * 8);
  t.desc_h = Hc; t.desc_w = Wc; t.kp_xys = kp_out; t.cell_h = sp->cell_h.as<int>(); t.cell_w = sp->cell_w.as<int>();
  t.n_out = n_out; t.n_cand_out = n_cand_out; t.reset_count = a.cand_count;
  t.pix = sp_wants_pix(sp) ? sp->pix.as<int>() : nullptr;
  if (sp->kp_selection == SSHIP_SELECT_BALANCED) {
    // one more launch, in this mode only: k_select_balanced leaves the K keys the rule selects in sp->sel, and k_topk sorts and emits THAT
    // list.  It still clears the original counter (reset_count) for the next call; the candidate count M is reported by the new kernel.
    SelWs ws;
    if (sp->sel.bytes < (size_t)sp->wsB * t.max_kp * 8 || sp->sel_ws.bytes < sel_ws_layout(sp->sel_ws, sp->wsB, sp->cap, Hc * Wc, &ws))
      return fail(SSHIP_ERR_INVALID, "balanced selection: the workspace has not been sized for this shape");  // sp_ensure does; never taken
    SelectBalancedArgs q = select_balanced_args(a.cand, a.cand_count, sp->cap, t.max_kp, Hc * 8, Wc * 8, sp->bucket_px,
                                                sp->sel.as<unsigned long long>(), sp->sel_count.as<int>(), ws);
    q.n_cand_out = n_cand_out;
    SSHIP_HIP_CHECK(launch_select_balanced(q, B, s));
    g_timer.mark_fine("sp_extract_stereo:select/balanced", s);
    t.cand = q.sel; t.cand_count = q.sel_count; t.cap = t.max_kp; t.n_cand_out = nullptr;
  }
  launch_topk(t, B, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  sp->cand_zero_n = B;
  if (sp->kp_refinement == SSHIP_KP_SUBPIXEL) {
    // one more launch, in this mode only: x, y of every keypoint from the logits convPb left in sp->logits (nothing writes them before the
    // next call's network) at the pixels k_topk left in sp->pix.  Scores, cells and the descriptor head do not see it.
    g_timer.mark_fine("sp_extract_stereo:select/topk", s);
    SSHIP_HIP_CHECK(sp_refine(sp, B, Hc, Wc, kp_out, n_out, t.scale_x, t.scale_y, s));
    g_timer.mark(g_profiling >= 2 ? "sp_extract_stereo:select/kp_refine" : "sp_extract_stereo:select", s);
    return SSHIP_OK;
  }
  g_timer.mark(g_profiling >= 2 ? "sp_extract_stereo:select/topk" : "sp_extract_stereo:select", s);
  return SSHIP_OK;
}

static hipError_t conv1ab(sship_sp* sp, const uint8_t* img, _Float16* out, int B, int H, int W, hipStream_t s) {
#if SSHIP_DEV_SWITCHES
  if (conv_mode() == 2) return sp_conv1ab_fused(sp->c1b, sp->w1a_frag, sp->b1a, img, out, B, H, W, s);
#endif
  return sp_conv1ab_pp(sp->c1b, sp->w1a_fragb, sp->b1a, img, out, B, H, W, s);
}

extern "C" int sship_sp_create(const sship_sp_config* cfg, sship_sp** out) {
  bind_thread();
  if (!cfg || !out || !cfg->weights_path) return fail(SSHIP_ERR_INVALID, "sp_create: null argument");
  if (cfg->max_keypoints <= 0 || cfg->max_keypoints > kMaxKp) return fail(SSHIP_ERR_INVALID, "sp_create: max_keypoints must be in [1, 4096]");
  if (cfg->nms_radius < 0 || cfg->nms_radius > 8) return fail(SSHIP_ERR_INVALID, "sp_create: nms_radius must be in [0, 8]");
  if (int rc = require_device()) return rc;
  StateDict sd; std::string err;
  if (!load_safetensors(cfg->weights_path, sd, err)) return fail(SSHIP_ERR_IO, err);
  // every early return below releases what has been uploaded so far (weights, fragments, stream, pool)
  std::unique_ptr<sship_sp, void (*)(sship_sp*)> sp(new sship_sp(), sship_sp_destroy);
  sp->cfg = *cfg;
  if (sp->cfg.pool_slots <= 0) sp->cfg.pool_slots = 8;
  if (sp->cfg.max_batch <= 0) sp->cfg.max_batch = 2;
  sp->cfg.weights_path = nullptr;
  sp->thr_f = threshold_as_float(cfg->keypoint_threshold);
  struct L { const char* name; int cout, cin, ks, ct; ConvW* dst; };
  const L layers[] = {{"conv1b", 64, 64, 3, 64, &sp->c1b}, {"conv2a", 64, 64, 3, 64, &sp->c2a},
                      {"conv2b", 64, 64, 3, 64, &sp->c2b}, {"conv3a", 128, 64, 3, 64, &sp->c3a},
                      {"conv3b", 128, 128, 3, 32, &sp->c3b}, {"conv4a", 128, 128, 3, 32, &sp->c4a},
                      {"conv4b", 128, 128, 3, 32, &sp->c4b}, {"convPa", 256, 128, 3, 32, &sp->cPa},
                      {"convPb", 65, 256, 1, 96, &sp->cPb}, {"convDa", 256, 128, 3, 32, &sp->cDa},
                      {"convDb", 256, 256, 1, 128, &sp->cDb}};
  for (const L& l : layers) {
    const Tensor* w = find_tensor(sd, std::string(l.name) + ".weight", {l.cout, l.cin, l.ks, l.ks}, err);
    const Tensor* b = w ? find_tensor(sd, std::string(l.name) + ".bias", {l.cout}, err) : nullptr;
    if (!w || !b) return fail(SSHIP_ERR_IO, err);
    if (int rc = upload_conv(w->data.data(), b->data.data(), l.cout, l.cin, l.ks, l.ct, *l.dst)) return rc;
    // second packing (64-row cout tiles over 32-channel chunks) for the kernels of conv_pp128.hip; conv1b runs fused with conv1a
    // (conv_pp.hip), convDa keeps the k order the sparse descriptor head shares
    if (l.ks == 3 && std::string(l.name) != "convDa" && std::string(l.name) != "conv1b")
      if (int rc = upload_conv_q(w->data.data(), l.cout, l.cin, *l.dst)) return rc;
#if SSHIP_DEV_SWITCHES
    if (std::string(l.name) == "conv2a" || std::string(l.name) == "conv2b")
      if (int rc = upload_wino(w->data.data(), *l.dst)) return rc;
#endif
    if (std::string(l.name) == "convDb")
      if (int rc = upload_conv(w->data.data(), b->data.data(), l.cout, l.cin, 1, 32, sp->cDb32)) return rc;
    if (std::string(l.name) == "convPb") {  // the streaming kernel reads the plain matrix, [80][256] fp16 (sp_convs.hip: k_convpb_stream)
      std::vector<_Float16> plain((size_t)80 * 256, (_Float16)0.f);
      for (int co = 0; co < 65; ++co)
        for (int ci = 0; ci < 256; ++ci) plain[(size_t)co * 256 + ci] = (_Float16)w->data[(size_t)co * 256 + ci];
      SSHIP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&l.dst->w_q), plain.size() * sizeof(_Float16)));
      SSHIP_HIP_CHECK(hipMemcpy(l.dst->w_q, plain.data(), plain.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    }
  }
  {
    const Tensor* w = find_tensor(sd, "conv1a.weight", {64, 1, 3, 3}, err);
    const Tensor* b = w ? find_tensor(sd, "conv1a.bias", {64}, err) : nullptr;
    if (!w || !b) return fail(SSHIP_ERR_IO, err);
    std::vector<float> wt(576);
    for (int co = 0; co < 64; ++co)
      for (int t = 0; t < 9; ++t) wt[t * 64 + co] = (float)(_Float16)w->data[co * 9 + t];  // fp16 engine weights
    if (int rc = upload_floats(wt.data(), 576, &sp->w1a)) return rc;
    if (int rc = upload_floats(b->data.data(), 64, &sp->b1a)) return rc;
    std::vector<_Float16> fr(2 * 64 * 8);
    for (int mt = 0; mt < 2; ++mt)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int co = mt * 32 + (lane & 31), k = (lane >> 5) * 8 + e;
          fr[(mt * 64 + lane) * 8 + e] = (_Float16)(k < 9 ? w->data[co * 9 + k] : 0.f);
        }
    SSHIP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&sp->w1a_frag), fr.size() * sizeof(_Float16)));
    SSHIP_HIP_CHECK(hipMemcpy(sp->w1a_frag, fr.data(), fr.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    // ping-pong kernel (conv_pp.hip, stage_conv1a): balanced K layout - lanes hh = 0 hold taps 0..4 in slots 0..4, lanes hh = 1
    // taps 5..8 in slots 0..3 and the bias, split into fp16 hi / lo parts, in slots 4 and 5 (their B elements are 1.0)
    std::fill(fr.begin(), fr.end(), (_Float16)0.f);
    for (int mt = 0; mt < 2; ++mt)
      for (int lane = 0; lane < 64; ++lane) {
        const int co = mt * 32 + (lane & 31), hh = lane >> 5;
        _Float16* f = &fr[(mt * 64 + lane) * 8];
        if (hh == 0) {
          for (int e = 0; e < 5; ++e) f[e] = (_Float16)w->data[co * 9 + e];
        } else {
          for (int e = 0; e < 4; ++e) f[e] = (_Float16)w->data[co * 9 + 5 + e];
          const _Float16 hi = (_Float16)b->data[co];
          f[4] = hi;
          f[5] = (_Float16)(b->data[co] - (float)hi);
        }
      }
    SSHIP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&sp->w1a_fragb), fr.size() * sizeof(_Float16)));
    SSHIP_HIP_CHECK(hipMemcpy(sp->w1a_fragb, fr.data(), fr.size() * sizeof(_Float16), hipMemcpyHostToDevice));
  }
  // blocking stream: ordered with the legacy default stream, so a caller that passes stream = NULL (e.g. torch's default
  // stream, whose handle IS 0) still gets its work ordered against ours
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&sp->stream, hipStreamDefault));
  if (int rc = sship_pool_create(sp->cfg.pool_slots, sp->cfg.max_keypoints, SSHIP_DESC_DIM, &sp->pool)) return rc;
  *out = sp.release();
  return SSHIP_OK;
}
extern "C" void sship_sp_destroy(sship_sp* sp) {
  bind_thread();
  if (!sp) return;
  (void)hipDeviceSynchronize();
  for (ConvW* c : {&sp->c1b, &sp->c2a, &sp->c2b, &sp->c3a, &sp->c3b, &sp->c4a, &sp->c4b, &sp->cPa, &sp->cPb, &sp->cDa, &sp->cDb, &sp->cDb32})
    free_conv(*c);
  if (sp->w1a) (void)hipFree(sp->w1a);
  if (sp->b1a) (void)hipFree(sp->b1a);
  if (sp->w1a_frag) (void)hipFree(sp->w1a_frag);
  if (sp->w1a_fragb) (void)hipFree(sp->w1a_fragb);
  ring_free(sp);  // BEFORE the pool: an uncollected sship_sp_ring_submit hands its slots back to sp->pool
  if (sp->pool) sship_pool_destroy(sp->pool);
  sp->pool = nullptr;
  if (sp->stream) (void)hipStreamDestroy(sp->stream);
  delete sp;
}
extern "C" int sship_sp_debug_activation(sship_sp* sp, int layer, void* out_host, unsigned long long bytes) {
  bind_thread();
  if (!sp || !out_host) return fail(SSHIP_ERR_INVALID, "sp_debug_activation: null argument");
  // 8 convPa, 9 convDa, 10 convDb (raw) and 11 convPb's logits (fp32, kLogitStride floats a cell): the head activations
  DevBuf* bufs[12] = {nullptr, &sp->a1b, &sp->a2a, &sp->a2b, &sp->a3a, &sp->a3b, &sp->a4a, &sp->a4b, &sp->aPa, &sp->aDa, &sp->draw, &sp->logits};
  if (layer < 1 || layer > 11 || !bufs[layer]->p || bytes > bufs[layer]->bytes) return fail(SSHIP_ERR_INVALID, "sp_debug_activation: bad layer / size");
  SSHIP_HIP_CHECK(hipDeviceSynchronize());
  SSHIP_HIP_CHECK(hipMemcpy(out_host, bufs[layer]->p, bytes, hipMemcpyDeviceToHost));
  return SSHIP_OK;
}
// Test-only hooks, exported but NOT part of include/sship.h (tests/_tail_ab.py binds them by name; the product never calls them): the two
// kernels behind convPa alone, with this handle's weights on the caller's device buffers, device-synchronising.
//   sship_sp_debug_convpb:    convPb on `pixels` rows of 256 fp16 -> `pixels` rows of 68 fp32 (65 logits, 3 zeros)
//   sship_sp_debug_desc_head: the nearest-cell descriptor head on a conv4b map a4b [batch][Hc][Wc][128] fp16 at the cells cell_h / cell_w
//                             [batch][max_kp] (counts n_dev [batch]) -> desc [batch][max_kp][256] fp16; rows past an image's count are left as they are
extern "C" int sship_sp_debug_convpb(sship_sp* sp, const void* in_fp16_dev, int pixels, float* logits_dev) {
  bind_thread();
  if (!sp || !in_fp16_dev || !logits_dev || pixels <= 0) return fail(SSHIP_ERR_INVALID, "sp_debug_convpb: bad arguments");
  SSHIP_HIP_CHECK(sp_conv1x1_f32(sp->cPb, static_cast<const _Float16*>(in_fp16_dev), logits_dev, kLogitStride, 1, 1, pixels, sp->stream));
  SSHIP_HIP_CHECK(hipStreamSynchronize(sp->stream));
  return SSHIP_OK;
}
extern "C" int sship_sp_debug_desc_head(sship_sp* sp, const void* a4b_fp16_dev, int batch, int Hc, int Wc, const int* cell_h_dev,
                                        const int* cell_w_dev, const int* n_dev, int max_kp, void* desc_fp16_dev) {
  bind_thread();
  if (!sp || !a4b_fp16_dev || !cell_h_dev || !cell_w_dev || !n_dev || !desc_fp16_dev || batch <= 0 || Hc <= 0 || Wc <= 0 || max_kp <= 0)
    return fail(SSHIP_ERR_INVALID, "sp_debug_desc_head: bad arguments");
  SSHIP_HIP_CHECK(launch_desc_head_sparse(sp->cDa, sp->cDb32, static_cast<const _Float16*>(a4b_fp16_dev), Hc, Wc, cell_h_dev, cell_w_dev, n_dev,
                                          max_kp, batch, static_cast<_Float16*>(desc_fp16_dev), (size_t)max_kp * 256, sp->stream));
  SSHIP_HIP_CHECK(hipStreamSynchronize(sp->stream));
  return SSHIP_OK;
}
//   sship_sp_debug_select:    the selection of an extraction - sp_select itself, with the handle's radius, threshold, border and max_keypoints - on
//                             logits [batch][Hc][Wc][68] fp32 on the device, or (logits_dev NULL) on the ones the handle's last network call at
//                             this batch and size left behind.  h, w: the image size (Hc = h / 8, Wc = w / 8).  kp [batch][max_kp][3], cells
//                             [batch][max_kp] and counts [batch] as an extraction produces them (kp rows past an image's count are left as they are, cell
//                             rows past it are the handle's buffers, copied whole), n_cand [batch] = candidates before the top-k.
//                             raw / nms NULL: the NMS launch has exactly an extraction's arguments (candidates only, no map is written);
//                             otherwise it also writes the softmax map before NMS and / or the map after it, [batch][8Hc][8Wc] fp32.
extern "C" int sship_sp_debug_select(sship_sp* sp, const float* logits_dev, int batch, int h, int w, float* kp_dev, int* cell_h_dev,
                                     int* cell_w_dev, int* n_dev, int* n_cand_dev, float* raw_dev, float* nms_dev) {
  bind_thread();
  if (!sp || !kp_dev || !n_dev || batch <= 0 || h < 8 || w < 8) return fail(SSHIP_ERR_INVALID, "sp_debug_select: bad arguments");
  if (logits_dev) {
    if (sp->kp_refinement == SSHIP_KP_SUBPIXEL) return fail(SSHIP_ERR_INVALID, "sp_debug_select: sub-pixel refinement reads the handle's own logits");
    if (int rc = sp_ensure(sp, batch, h, w)) return rc;
  } else if (!sp->logits.p || batch > sp->wsB || h != sp->wsH || w != sp->wsW) {
    return fail(SSHIP_ERR_INVALID, "sp_debug_select: run the network at this shape first");
  } else if (sp->kp_selection == SSHIP_SELECT_BALANCED) {  // the mode may have been set after that network call
    if (int rc = sp_ensure_balanced(sp, sp->wsB, h / 8, w / 8)) return rc;
  }
  SSHIP_HIP_CHECK(hipDeviceSynchronize());  // the logits may come from any stream
  hipStream_t s = sp->stream;
  if (int rc = sp_select(sp, batch, h, w, nms_dev, kp_dev, n_dev, s, logits_dev, raw_dev, n_cand_dev)) return rc;
  const size_t cells = (size_t)batch * sp->cfg.max_keypoints * sizeof(int);
  if (cell_h_dev) SSHIP_HIP_CHECK(hipMemcpyAsync(cell_h_dev, sp->cell_h.p, cells, hipMemcpyDeviceToDevice, s));
  if (cell_w_dev) SSHIP_HIP_CHECK(hipMemcpyAsync(cell_w_dev, sp->cell_w.p, cells, hipMemcpyDeviceToDevice, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  return SSHIP_OK;
}
extern "C" sship_pool* sship_sp_pool(sship_sp* sp) {
  bind_thread(); return sp ? sp->pool : nullptr; }
extern "C" int sship_sp_max_keypoints(const sship_sp* sp) { return sp ? sp->cfg.max_keypoints : 0; }
extern "C" int sship_sp_set_descriptor_sampling(sship_sp* sp, int mode) {
  if (!sp) return fail(SSHIP_ERR_INVALID, "sp_set_descriptor_sampling: null handle");
  if (mode != SSHIP_DESC_NEAREST && mode != SSHIP_DESC_BILINEAR)
    return fail(SSHIP_ERR_INVALID, "sp_set_descriptor_sampling: mode must be 0 (nearest) or 1 (bilinear)");
  for (const auto& pd : sp->ring.pending)
    if (pd.active) return fail(SSHIP_ERR_INVALID, "sp_set_descriptor_sampling: a ring submission is pending (collect it with sship_sp_extract_stereo_ring first)");
#if SSHIP_DEV_SWITCHES
  // developer build: the dense-branch A/B path (SUPERSLAM_HIP_DESC=dense) has no bilinear form
  if (mode == SSHIP_DESC_BILINEAR && desc_dense_mode()) return fail(SSHIP_ERR_INVALID, "sp_set_descriptor_sampling: bilinear sampling is not available under SUPERSLAM_HIP_DESC=dense");
#endif
  sp->desc_sampling = mode;
  return SSHIP_OK;
}
extern "C" int sship_sp_descriptor_sampling(const sship_sp* sp) { return sp ? sp->desc_sampling : SSHIP_DESC_NEAREST; }
extern "C" int sship_sp_set_keypoint_refinement(sship_sp* sp, int mode) {
  if (!sp) return fail(SSHIP_ERR_INVALID, "sp_set_keypoint_refinement: null handle");
  if (mode != SSHIP_KP_INTEGER && mode != SSHIP_KP_SUBPIXEL)
    return fail(SSHIP_ERR_INVALID, "sp_set_keypoint_refinement: mode must be 0 (integer) or 1 (sub-pixel)");
  for (const auto& pd : sp->ring.pending)
    if (pd.active) return fail(SSHIP_ERR_INVALID, "sp_set_keypoint_refinement: a ring submission is pending (collect it with sship_sp_extract_stereo_ring first)");
  // developer build: every detector-head switch (SUPERSLAM_HIP_CONVPB=igemm, the SUPERSLAM_HIP_CONV* encoder kernels) still writes the
  // fp32 logits as 68-float rows into sp->logits, so none of them has to refuse SSHIP_KP_SUBPIXEL; a switch that keeps the logits on chip must.
  sp->kp_refinement = mode;
  return SSHIP_OK;
}
extern "C" int sship_sp_keypoint_refinement(const sship_sp* sp) { return sp ? sp->kp_refinement : SSHIP_KP_INTEGER; }
extern "C" int sship_sp_set_keypoint_selection(sship_sp* sp, int mode, int bucket_px) {
  if (!sp) return fail(SSHIP_ERR_INVALID, "sp_set_keypoint_selection: null handle");
  if (mode != SSHIP_SELECT_TOPK && mode != SSHIP_SELECT_BALANCED)
    return fail(SSHIP_ERR_INVALID, "sp_set_keypoint_selection: mode must be 0 (top-k) or 1 (balanced)");
  if (mode == SSHIP_SELECT_BALANCED && (bucket_px < 8 || bucket_px > 65535))
    return fail(SSHIP_ERR_INVALID, "sp_set_keypoint_selection: bucket_px must be in [8, 65535]");
  for (const auto& pd : sp->ring.pending)
    if (pd.active) return fail(SSHIP_ERR_INVALID, "sp_set_keypoint_selection: a ring submission is pending (collect it with sship_sp_extract_stereo_ring first)");
  // no allocation here: the next call's sp_ensure sizes the mode's buffers where it sizes the other selection buffers
  sp->kp_selection = mode;
  if (mode == SSHIP_SELECT_BALANCED) sp->bucket_px = bucket_px;
  return SSHIP_OK;
}
extern "C" int sship_sp_keypoint_selection(const sship_sp* sp, int* bucket_px_out) {
  if (bucket_px_out) *bucket_px_out = sp ? sp->bucket_px : 0;
  return sp ? sp->kp_selection : SSHIP_SELECT_TOPK;
}
// stage twin of sship_select_topk: threshold scan -> k_select_balanced -> k_topk on the selected list
extern "C" int sship_select_topk_balanced(const float* scores, int score_h, int score_w, int input_h, int input_w, double thr, int border,
                                          int max_kp, int bucket_px, int desc_h, int desc_w, float* kp_xys, int* cell_h, int* cell_w,
                                          int* n_dev, int* n_cand_dev, void* stream) {
  bind_thread();
  if (!scores || !kp_xys || !cell_h || !cell_w || !n_dev || score_h <= 0 || score_w <= 0)
    return fail(SSHIP_ERR_INVALID, "select_topk_balanced: bad arguments");
  if (max_kp <= 0 || max_kp > kMaxKp) return fail(SSHIP_ERR_INVALID, "select_topk_balanced: max_kp must be in [1, 4096]");
  if (bucket_px < 8 || bucket_px > 65535) return fail(SSHIP_ERR_INVALID, "select_topk_balanced: bucket_px must be in [8, 65535]");
  if (int rc = require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cap = score_h * score_w;
  DevBuf cand, cnt, sel, ws_buf;  // cnt: the candidate counter, then the selected count
  SSHIP_HIP_CHECK(cand.ensure((size_t)cap * 8));
  SSHIP_HIP_CHECK(cnt.ensure(8));
  SSHIP_HIP_CHECK(sel.ensure((size_t)max_kp * 8));
  const int nb_max = ((score_h + 7) / 8) * ((score_w + 7) / 8);
  SSHIP_HIP_CHECK(ws_buf.ensure(sel_ws_layout(ws_buf, 1, cap, nb_max, nullptr)));
  SelWs ws;
  sel_ws_layout(ws_buf, 1, cap, nb_max, &ws);
  SSHIP_HIP_CHECK(hipMemsetAsync(cnt.p, 0, 8, s));
  launch_threshold_scan(scores, score_h, score_w, threshold_as_float(thr), border, cand.as<unsigned long long>(), cnt.as<int>(), cap, s);
  SelectBalancedArgs q = select_balanced_args(cand.as<unsigned long long>(), cnt.as<int>(), cap, max_kp, score_h, score_w, bucket_px,
                                              sel.as<unsigned long long>(), cnt.as<int>() + 1, ws);
  q.n_cand_out = n_cand_dev;
  SSHIP_HIP_CHECK(launch_select_balanced(q, 1, s));
  TopkArgs t{};
  t.cand = q.sel; t.cand_count = q.sel_count; t.cap = max_kp; t.max_kp = max_kp;
  t.score_w = score_w;
  t.scale_x = static_cast<float>(input_w) / score_w;
  t.scale_y = static_cast<float>(input_h) / score_h;
  t.desc_h = desc_h; t.desc_w = desc_w; t.kp_xys = kp_xys; t.cell_h = cell_h; t.cell_w = cell_w; t.n_out = n_dev;
  launch_topk(t, 1, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));  // scratch buffers die with this scope
  return SSHIP_OK;
}

extern "C" int sship_sp_extract_batch_device(sship_sp* sp, const uint8_t* imgs, int batch, int h, int w, void* desc_out,
                                             float* kp_out, int* n_out, void* stream) {
  bind_thread();
  if (!sp || !imgs || !desc_out || !kp_out || !n_out || batch <= 0) return fail(SSHIP_ERR_INVALID, "sp_extract_batch_device: bad arguments");
  // stream == NULL is the legacy default stream itself (torch's default stream): back-to-back extractor / matcher calls
  // made with NULL are then ordered with each other and with the caller's own NULL-stream work.  (They used to fall back
  // to each handle's private stream, which are ordered with the NULL stream but not with one another.)
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = sp_ensure(sp, batch, h, w)) return rc;
  // a profiled call keeps a copy of its input in the handle: sship_sp_bench_layer re-launches layers on the buffers this
  // call leaves behind, and a conv1a+conv1b launch on an all-zero image clocks ~7 % higher than on real pixels (the chip
  // runs at its power limit; low-toggle operands draw less) - the figure would flatter the kernel
  if (g_profiling && imgs != sp->img.as<uint8_t>())
    SSHIP_HIP_CHECK(hipMemcpyAsync(sp->img.p, imgs, (size_t)batch * h * w, hipMemcpyDeviceToDevice, s));
  sp->img_valid = g_profiling != 0 || imgs == sp->img.as<uint8_t>();
  g_timer.begin(s);
  if (int rc = sp_network(sp, imgs, batch, h, w, s, false)) return rc;
  if (int rc = sp_select(sp, batch, h, w, nullptr, kp_out, n_out, s)) return rc;
  int H2, W2, H4, W4, Hc, Wc;
  sp_shapes(h, w, H2, W2, H4, W4, Hc, Wc);
  SSHIP_HIP_CHECK(desc_head(sp, 0, Hc, Wc, sp->cell_h.as<int>(), sp->cell_w.as<int>(), n_out, batch, static_cast<_Float16*>(desc_out),
                            (size_t)sp->cfg.max_keypoints * 256, s));
  g_timer.mark("sp_extract_stereo:gather", s);
  return SSHIP_OK;
}

extern "C" int sship_sp_dense(sship_sp* sp, const uint8_t* imgs, int batch, int h, int w, float* scores, void* desc_grid,
                              float* logits, void* stream) {
  bind_thread();
  if (!sp || !imgs || batch <= 0) return fail(SSHIP_ERR_INVALID, "sp_dense: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = legacy default stream (see sship_sp_extract_batch_device)
  if (int rc = sp_ensure(sp, batch, h, w)) return rc;
  if (int rc = sp_network(sp, imgs, batch, h, w, s, desc_grid != nullptr)) return rc;
  int H2, W2, H4, W4, Hc, Wc;
  sp_shapes(h, w, H2, W2, H4, W4, Hc, Wc);
  if (scores) {
    NmsArgs a{};
    a.logits = sp->logits.as<float>(); a.ls = kLogitStride; a.B = batch; a.H = Hc * 8; a.W = Wc * 8;
    a.radius = sp->cfg.nms_radius; a.scores_out = scores;
    launch_nms_tile(0, a, s);
  }
  if (desc_grid) launch_desc_dense_chw(sp->draw.as<_Float16>(), Hc * Wc, batch, static_cast<_Float16*>(desc_grid), s);
  if (logits) launch_logits_chw(sp->logits.as<float>(), kLogitStride, Hc * Wc, batch, logits, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  return SSHIP_OK;
}

extern "C" int sship_mfma_probe(int random_operands, float* tflops) {
  bind_thread();
  if (!tflops) return fail(SSHIP_ERR_INVALID, "mfma_probe: null argument");
  if (int rc = require_device()) return rc;
  SSHIP_HIP_CHECK(mfma_probe(random_operands != 0, tflops));
  return SSHIP_OK;
}

extern "C" int sship_sp_bench_layer(sship_sp* sp, int layer, int batch, int h, int w, int iters, float* avg_ms,
                                    double* macs) {
  bind_thread();
  if (!sp || !avg_ms || iters <= 0 || layer < 0 || layer > 17) return fail(SSHIP_ERR_INVALID, "sp_bench_layer: bad arguments");
  if (batch > sp->wsB || h != sp->wsH || w != sp->wsW) return fail(SSHIP_ERR_INVALID, "sp_bench_layer: run the network at this shape first");
  if (layer <= 1 && !sp->img_valid)
    return fail(SSHIP_ERR_INVALID, "sp_bench_layer: the handle holds no copy of the last input - make one call with sship_set_profiling(1) first "
                                   "(a launch on stale / zero pixels runs at a higher clock than the real one)");
  int H2, W2, H4, W4, Hc, Wc;
  sp_shapes(h, w, H2, W2, H4, W4, Hc, Wc);
  hipStream_t s = sp->stream;
  _Float16 *a1a = sp->a1a.as<_Float16>(), *a1b = sp->a1b.as<_Float16>(), *a2a = sp->a2a.as<_Float16>(),
           *a2b = sp->a2b.as<_Float16>(), *a3a = sp->a3a.as<_Float16>(), *a3b = sp->a3b.as<_Float16>(),
           *a4a = sp->a4a.as<_Float16>(), *a4b = sp->a4b.as<_Float16>(), *aPa = sp->aPa.as<_Float16>(),
           *aDa = sp->aDa.as<_Float16>();
  const bool for_refine = layer == 16;  // its k_topk launch leaves the packed pixels whatever mode the handle is in
  auto run = [&]() -> hipError_t {
    switch (layer) {
      case 0: launch_conv1a(sp->img.as<uint8_t>(), sp->w1a, sp->b1a, a1a, batch, h, w, s); return hipGetLastError();  // stand-alone (not on the path)
      case 1: return conv1ab(sp, sp->img.as<uint8_t>(), a1b, batch, h, w, s);
      case 15:  // conv2a -> conv2b -> pool in one launch (conv_fuse2.hip): what a throughput batch runs instead of layers 2 and 3
        if (!sp_conv2ab_fused_fits(batch, H2, W2, true)) return hipErrorInvalidValue;
        return sp_conv2ab_fused(sp->c2a, sp->c2b, a1b, a2b, batch, H2, W2, s);
      case 2: return conv3(sp->c2a, a1b, a2a, batch, H2, W2, false, s);
      case 3: return conv3(sp->c2b, a2a, a2b, batch, H2, W2, true, s);
      case 4: return conv3a_layer(sp->c3a, a2b, a3a, batch, H4, W4, s);
      case 5: return conv3(sp->c3b, a3a, a3b, batch, H4, W4, true, s);
      case 6: return conv3(sp->c4a, a3b, a4a, batch, Hc, Wc, false, s);
      case 7: return conv3(sp->c4b, a4a, a4b, batch, Hc, Wc, false, s);
      case 8: return conv3(sp->cPa, a4b, aPa, batch, Hc, Wc, false, s);
      case 9: return sp_conv1x1_f32(sp->cPb, aPa, sp->logits.as<float>(), kLogitStride, batch, Hc, Wc, s);
      case 10: return conv3(sp->cDa, a4b, aDa, batch, Hc, Wc, false, s);
      case 11: return sp_conv1x1_f16(sp->cDb, aDa, sp->draw.as<_Float16>(), batch, Hc, Wc, s);
      case 12: {  // softmax + depth-to-space + NMS + threshold + candidate compaction (k_nms_tile) on the last logits
        if (hipError_t e = hipMemsetAsync(sp->cand_count.p, 0, (size_t)batch * 4, s)) return e;
        sp->cand_zero_n = 0;  // this stage leaves its counts behind (stage 13 reads them): the next extraction clears them itself
        NmsArgs a{};
        a.logits = sp->logits.as<float>(); a.ls = kLogitStride; a.B = batch; a.H = Hc * 8; a.W = Wc * 8;
        a.radius = sp->cfg.nms_radius; a.thr_f = sp->thr_f; a.border = sp->cfg.remove_borders;
        a.cand = sp->cand.as<unsigned long long>(); a.cand_count = sp->cand_count.as<int>(); a.cap = sp->cap;
        launch_nms_tile(0, a, s);
        return hipGetLastError();
      }
      case 13: {  // top-k over the candidates left by the last selection (k_topk)
        TopkArgs t{};
        t.cand = sp->cand.as<unsigned long long>(); t.cand_count = sp->cand_count.as<int>(); t.cap = sp->cap;
        t.max_kp = sp->cfg.max_keypoints; t.score_w = Wc * 8;
        t.scale_x = static_cast<float>(w) / (Wc * 8); t.scale_y = static_cast<float>(h) / (Hc * 8);
        t.desc_h = Hc; t.desc_w = Wc; t.kp_xys = sp->kp.as<float>(); t.cell_h = sp->cell_h.as<int>(); t.cell_w = sp->cell_w.as<int>();
        t.n_out = sp->n_dev.as<int>(); t.n_cand_out = nullptr;
        t.pix = (sp_wants_pix(sp) || for_refine) ? sp->pix.as<int>() : nullptr;
        launch_topk(t, batch, s);
        return hipGetLastError();
      }
      case 17: {  // balanced selection over the candidates left by the last selection (k_select_balanced alone), whatever mode the handle is in
        SelWs ws;
        sel_ws_layout(sp->sel_ws, sp->wsB, sp->cap, Hc * Wc, &ws);
        const SelectBalancedArgs q = select_balanced_args(sp->cand.as<unsigned long long>(), sp->cand_count.as<int>(), sp->cap, sp->cfg.max_keypoints,
                                                          Hc * 8, Wc * 8, sp->bucket_px, sp->sel.as<unsigned long long>(), sp->sel_count.as<int>(), ws);
        return launch_select_balanced(q, batch, s);
      }
      case 16:  // sub-pixel refinement of the selected keypoints (k_kp_refine), whatever mode the handle is in
        return sp_refine(sp, batch, Hc, Wc, sp->kp.as<float>(), sp->n_dev.as<int>(), static_cast<float>(w) / (Wc * 8), static_cast<float>(h) / (Hc * 8), s);
      default:  // 14: descriptor head at the selected keypoints (k_desc_head_sparse) into the staging rows
        if (hipError_t e = sp->desc_stage.ensure((size_t)batch * sp->cfg.max_keypoints * 512)) return e;
        return desc_head(sp, 0, Hc, Wc, sp->cell_h.as<int>(), sp->cell_w.as<int>(), sp->n_dev.as<int>(), batch, sp->desc_stage.as<_Float16>(),
                         (size_t)sp->cfg.max_keypoints * 256, s);
    }
  };
  if (layer == 17) {  // reads the candidates (layer 12 leaves them and their counts behind); its buffers exist only once the mode has been used
    if (int rc = sp_ensure_balanced(sp, sp->wsB, Hc, Wc)) return rc;
    layer = 12; SSHIP_HIP_CHECK(run());
    layer = 17;
  }
  if (layer == 13 || layer == 14 || layer == 16) {  // these read the selection's outputs: produce them once on this handle's own buffers
    const int keep = layer;
    layer = 12; SSHIP_HIP_CHECK(run());
    layer = 13; SSHIP_HIP_CHECK(run());
    layer = keep;
  }
  const double px[12] = {(double)h * w, (double)h * w, (double)H2 * W2, (double)H2 * W2, (double)H4 * W4, (double)H4 * W4,
                         (double)Hc * Wc, (double)Hc * Wc, (double)Hc * Wc, (double)Hc * Wc, (double)Hc * Wc, (double)Hc * Wc};
  const double mpp[12] = {9.0 * 64, 576.0 * 64 + 9.0 * 64 /* conv1a fused */, 576.0 * 64, 576.0 * 64, 576.0 * 128, 1152.0 * 128, 1152.0 * 128,
                          1152.0 * 128, 1152.0 * 256, 256.0 * 65, 1152.0 * 256, 256.0 * 256};
  if (macs) *macs = layer < 12 ? px[layer] * mpp[layer] * batch : layer == 15 ? (px[2] * mpp[2] + px[3] * mpp[3]) * batch : 0.0;
  return bench_loop(s, iters, run, avg_ms);
}

// host-image front: upload (pinned) -> gray -> batch path into pool slots -> D2H keypoints.
static int sp_extract_device(sship_sp* sp, const uint8_t* gray, int B, int h, int w, sship_features* const* outs);
static int sp_extract_host(sship_sp* sp, const uint8_t* const* imgs, int B, int h, int w, int stride, int channels,
                           sship_features* const* outs) {
  if (channels != 1 && channels != 3) return fail(SSHIP_ERR_INVALID, "image must have 1 or 3 channels");
  if (h <= 0 || w <= 0 || stride < w * channels) return fail(SSHIP_ERR_INVALID, "bad image geometry");
  if (int rc = sp_ensure(sp, B, h, w)) return rc;
  hipStream_t s = sp->stream;
  const size_t row = (size_t)w * channels, img_bytes = row * h;
  uint8_t* hp = sp->h_img.as<uint8_t>();
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < h; ++y) memcpy(hp + b * img_bytes + y * row, imgs[b] + (size_t)y * stride, row);
  if (channels == 1) {
    SSHIP_HIP_CHECK(hipMemcpyAsync(sp->img.p, hp, img_bytes * B, hipMemcpyHostToDevice, s));
  } else {
    SSHIP_HIP_CHECK(hipMemcpyAsync(sp->gray_in.p, hp, img_bytes * B, hipMemcpyHostToDevice, s));
    launch_bgr2gray(sp->gray_in.as<uint8_t>(), B * h * w, sp->img.as<uint8_t>(), s);
  }
  sp->img_valid = true;
  return sp_extract_device(sp, sp->img.as<uint8_t>(), B, h, w, outs);
}
// `gray`: B u8 images [h][w] resident on the device, ordered with sp->stream.
// Enqueue: network + selection + descriptor head into freshly acquired pool slots + D2H of keypoints / counts into the given
// pinned buffers - everything asynchronous on sp->stream.  slots[b] = -1 where the pool was exhausted (*rc_pool set).
static int sp_extract_enqueue(sship_sp* sp, const uint8_t* gray, int B, int h, int w, int* slots, int* rc_pool, float* h_kp, int* h_n) {
  hipStream_t s = sp->stream;
  g_timer.begin(s);
  *rc_pool = SSHIP_OK;
  for (int b = 0; b < B; ++b) slots[b] = -1;
  if (int rc = sp_network(sp, gray, B, h, w, s, false)) return rc;
  if (int rc = sp_select(sp, B, h, w, nullptr, sp->kp.as<float>(), sp->n_dev.as<int>(), s)) return rc;
  int H2, W2, H4, W4, Hc, Wc;
  sp_shapes(h, w, H2, W2, H4, W4, Hc, Wc);
  const int mk = sp->cfg.max_keypoints;
  // a HIP failure after slots were acquired hands them back: the 8-slot pool must not shrink with every error
  auto give_back = [&](hipError_t e, const char* what) {
    (void)hipStreamSynchronize(s);
    for (int b = 0; b < B; ++b)
      if (slots[b] >= 0) { sship_pool_release(sp->pool, slots[b]); slots[b] = -1; }
    return fail(SSHIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  for (int b = 0; b < B; ++b) {
    slots[b] = sship_pool_acquire(sp->pool);  // pool_->make(n), SuperPoint.cc:721
    if (slots[b] < 0) { *rc_pool = SSHIP_ERR_POOL_EXHAUSTED; continue; }
    if (hipError_t e = desc_head(sp, b, Hc, Wc, sp->cell_h.as<int>() + (size_t)b * mk, sp->cell_w.as<int>() + (size_t)b * mk,
                                 sp->n_dev.as<int>() + b, 1, static_cast<_Float16*>(sship_pool_slot_ptr(sp->pool, slots[b])), 0, s))
      return give_back(e, "sp_extract: descriptor head");
  }
  g_timer.mark("sp_extract_stereo:gather", s);
  if (hipError_t e = hipMemcpyAsync(h_kp, sp->kp.p, (size_t)B * mk * 12, hipMemcpyDeviceToHost, s)) return give_back(e, "sp_extract: D2H keypoints");
  if (hipError_t e = hipMemcpyAsync(h_n, sp->n_dev.p, (size_t)B * 4, hipMemcpyDeviceToHost, s)) return give_back(e, "sp_extract: D2H counts");
  return SSHIP_OK;
}
// Finish (after the stream / the completion event has been waited for): host copies into the caller's features.
static int sp_extract_finish(sship_sp* sp, int B, const int* slots, int rc_pool, const float* h_kp, const int* h_n, sship_features* const* outs) {
  const int mk = sp->cfg.max_keypoints;
  for (int b = 0; b < B; ++b) {
    const int n = h_n[b];
    outs[b]->n = n; outs[b]->slot = slots[b]; outs[b]->desc_dev = nullptr;
    if (outs[b]->kp_xys) memcpy(outs[b]->kp_xys, h_kp + (size_t)b * mk * 3, (size_t)n * 12);
    if (outs[b]->slot >= 0) {
      if (n == 0) { sship_pool_release(sp->pool, outs[b]->slot); outs[b]->slot = -1; }  // empty handle, SuperPoint.cc:722-723
      else outs[b]->desc_dev = sship_pool_slot_ptr(sp->pool, outs[b]->slot);
    }
  }
  if (rc_pool) return fail(rc_pool, "SuperPoint: descriptor pool exhausted (no free slot)");
  return SSHIP_OK;
}
static int sp_extract_device(sship_sp* sp, const uint8_t* gray, int B, int h, int w, sship_features* const* outs) {
  for (int b = 0; b < B; ++b) { outs[b]->n = 0; outs[b]->desc_dev = nullptr; outs[b]->slot = -1; }
  int slots[2] = {-1, -1}, rc_pool = 0;
  if (B > 2) return fail(SSHIP_ERR_INVALID, "sp_extract: at most two images per host call");
  if (int rc = sp_extract_enqueue(sp, gray, B, h, w, slots, &rc_pool, sp->h_kp.as<float>(), sp->h_n.as<int>())) return rc;
  if (hipError_t e = hipStreamSynchronize(sp->stream)) {
    for (int b = 0; b < B; ++b) if (slots[b] >= 0) sship_pool_release(sp->pool, slots[b]);
    return fail(SSHIP_ERR_HIP, std::string("sp_extract: stream synchronize: ") + hipGetErrorString(e));
  }
  return sp_extract_finish(sp, B, slots, rc_pool, sp->h_kp.as<float>(), sp->h_n.as<int>(), outs);
}

extern "C" int sship_sp_extract(sship_sp* sp, const uint8_t* img, int h, int w, int stride, int channels,
                                sship_features* out) {
  bind_thread();
  if (!sp || !img || !out) return fail(SSHIP_ERR_INVALID, "sp_extract: null argument");
  const uint8_t* imgs[1] = {img};
  sship_features* outs[1] = {out};
  return sp_extract_host(sp, imgs, 1, h, w, stride, channels, outs);
}
extern "C" int sship_sp_extract_stereo(sship_sp* sp, const uint8_t* left, const uint8_t* right, int h, int w, int stride,
                                       int channels, sship_features* out_left, sship_features* out_right) {
  bind_thread();
  if (!sp || !left || !right || !out_left || !out_right) return fail(SSHIP_ERR_INVALID, "sp_extract_stereo: null argument");
  const uint8_t* imgs[2] = {left, right};
  sship_features* outs[2] = {out_left, out_right};
  return sp_extract_host(sp, imgs, 2, h, w, stride, channels, outs);
}
// ---- decode-ahead upload ring (include/sship.h) ----
static void ring_free(sship_sp* sp) {
  auto& r = sp->ring;
  for (void* p : r.host) if (p) (void)hipHostFree(p);
  for (void* p : r.dev) if (p) (void)hipFree(p);
  for (hipEvent_t e : r.uploaded) if (e) (void)hipEventDestroy(e);
  for (auto& pd : r.pending) {
    if (pd.active) {  // submitted, never collected: hand the pool slots back
      if (pd.done) (void)hipEventSynchronize(pd.done);
      for (int b = 0; b < 2; ++b) if (pd.slots[b] >= 0 && sp->pool) sship_pool_release(sp->pool, pd.slots[b]);
    }
    if (pd.done) (void)hipEventDestroy(pd.done);
    if (pd.h_kp) (void)hipHostFree(pd.h_kp);
    if (pd.h_n) (void)hipHostFree(pd.h_n);
  }
  if (r.copy_stream) (void)hipStreamDestroy(r.copy_stream);
  r = sship_sp::Ring();
}
extern "C" int sship_sp_ring_create(sship_sp* sp, int depth, int h, int w, int channels) {
  bind_thread();
  if (!sp || depth < 1 || depth > 16 || h <= 0 || w <= 0 || (channels != 1 && channels != 3)) return fail(SSHIP_ERR_INVALID, "sp_ring_create: bad arguments");
  if (int rc = sp_ensure(sp, 2, h, w)) return rc;
  ring_free(sp);
  auto& r = sp->ring;
  r.depth = depth; r.h = h; r.w = w; r.ch = channels; r.img_bytes = (size_t)h * w * channels;
  r.host.assign(depth, nullptr); r.dev.assign(depth, nullptr); r.uploaded.assign(depth, nullptr);
  r.pending.assign(depth, sship_sp::Ring::Pending());
  auto bail = [&](const char* what, hipError_t e) { ring_free(sp); return fail(SSHIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); };
  if (hipError_t e = hipStreamCreateWithFlags(&r.copy_stream, hipStreamNonBlocking)) return bail("sp_ring_create: stream", e);
  for (int i = 0; i < depth; ++i) {
    if (hipError_t e = hipHostMalloc(&r.host[i], 2 * r.img_bytes, hipHostMallocDefault)) return bail("sp_ring_create: pinned host frame", e);
    if (hipError_t e = hipMalloc(&r.dev[i], 2 * r.img_bytes)) return bail("sp_ring_create: device frame", e);
    if (hipError_t e = hipEventCreateWithFlags(&r.uploaded[i], hipEventDisableTiming)) return bail("sp_ring_create: event", e);
    if (hipError_t e = hipEventCreateWithFlags(&r.pending[i].done, hipEventDisableTiming)) return bail("sp_ring_create: event", e);
    if (hipError_t e = hipHostMalloc(&r.pending[i].h_kp, (size_t)2 * sp->cfg.max_keypoints * 12, hipHostMallocDefault)) return bail("sp_ring_create: pinned keypoints", e);
    if (hipError_t e = hipHostMalloc(&r.pending[i].h_n, 8, hipHostMallocDefault)) return bail("sp_ring_create: pinned counts", e);
  }
  return SSHIP_OK;
}
extern "C" uint8_t* sship_sp_ring_host(sship_sp* sp, int slot, int image) {
  if (!sp || slot < 0 || slot >= sp->ring.depth || image < 0 || image > 1) return nullptr;
  return static_cast<uint8_t*>(sp->ring.host[slot]) + (size_t)image * sp->ring.img_bytes;
}
extern "C" int sship_sp_ring_upload(sship_sp* sp, int slot) {
  bind_thread();
  if (!sp || slot < 0 || slot >= sp->ring.depth) return fail(SSHIP_ERR_INVALID, "sp_ring_upload: bad slot");
  auto& r = sp->ring;
  // a submitted, uncollected extraction may still be reading r.dev[slot] on sp->stream (directly for 1 channel, through
  // bgr2gray for 3): re-uploading under it would race silently.  Collect first.
  if (r.pending[slot].active)
    return fail(SSHIP_ERR_INVALID, "sp_ring_upload: this slot has a submitted extraction that was not collected (sship_sp_extract_stereo_ring) yet");
  SSHIP_HIP_CHECK(hipMemcpyAsync(r.dev[slot], r.host[slot], 2 * r.img_bytes, hipMemcpyHostToDevice, r.copy_stream));
  SSHIP_HIP_CHECK(hipEventRecord(r.uploaded[slot], r.copy_stream));
  return SSHIP_OK;
}
// the slot's pair as grayscale on the device, ordered with sp->stream; a failed wait / launch is an error, not a partly uploaded frame
static int ring_gray(sship_sp* sp, int slot, const uint8_t** gray) {
  auto& r = sp->ring;
  SSHIP_HIP_CHECK(hipStreamWaitEvent(sp->stream, r.uploaded[slot], 0));
  if (r.ch == 3) {
    launch_bgr2gray(static_cast<const uint8_t*>(r.dev[slot]), 2 * r.h * r.w, sp->img.as<uint8_t>(), sp->stream);
    SSHIP_HIP_CHECK(hipGetLastError());
    *gray = sp->img.as<uint8_t>();
    return SSHIP_OK;
  }
  *gray = static_cast<const uint8_t*>(r.dev[slot]);
  return SSHIP_OK;
}
extern "C" int sship_sp_ring_submit(sship_sp* sp, int slot) {
  bind_thread();
  if (!sp || slot < 0 || slot >= sp->ring.depth) return fail(SSHIP_ERR_INVALID, "sp_ring_submit: bad slot");
  auto& r = sp->ring;
  auto& pd = r.pending[slot];
  if (pd.active) return fail(SSHIP_ERR_INVALID, "sp_ring_submit: this slot already has a submitted extraction (collect it with sship_sp_extract_stereo_ring)");
  if (int rc = sp_ensure(sp, 2, r.h, r.w)) return rc;
  const uint8_t* gray = nullptr;
  if (int rc = ring_gray(sp, slot, &gray)) return rc;
  if (int rc = sp_extract_enqueue(sp, gray, 2, r.h, r.w, pd.slots, &pd.rc_pool, static_cast<float*>(pd.h_kp), static_cast<int*>(pd.h_n))) return rc;
  SSHIP_HIP_CHECK(hipEventRecord(pd.done, sp->stream));
  pd.active = true;
  return SSHIP_OK;
}
extern "C" int sship_sp_extract_stereo_ring(sship_sp* sp, int slot, sship_features* out_left, sship_features* out_right) {
  bind_thread();
  if (!sp || !out_left || !out_right || slot < 0 || slot >= sp->ring.depth) return fail(SSHIP_ERR_INVALID, "sp_extract_stereo_ring: bad arguments");
  auto& r = sp->ring;
  sship_features* outs[2] = {out_left, out_right};
  auto& pd = r.pending[slot];
  if (pd.active) {  // submitted ahead (sship_sp_ring_submit): wait for its completion event only
    pd.active = false;
    for (int b = 0; b < 2; ++b) { outs[b]->n = 0; outs[b]->desc_dev = nullptr; outs[b]->slot = -1; }
    if (hipError_t e = hipEventSynchronize(pd.done)) {
      for (int b = 0; b < 2; ++b) if (pd.slots[b] >= 0) sship_pool_release(sp->pool, pd.slots[b]);
      return fail(SSHIP_ERR_HIP, std::string("sp_extract_stereo_ring: ") + hipGetErrorString(e));
    }
    return sp_extract_finish(sp, 2, pd.slots, pd.rc_pool, static_cast<const float*>(pd.h_kp), static_cast<const int*>(pd.h_n), outs);
  }
  if (int rc = sp_ensure(sp, 2, r.h, r.w)) return rc;
  const uint8_t* gray = nullptr;
  if (int rc = ring_gray(sp, slot, &gray)) return rc;
  return sp_extract_device(sp, gray, 2, r.h, r.w, outs);
}
extern "C" int sship_desc_to_host(const void* desc_dev, int count, int dim, float* out) {
  bind_thread();
  if (count <= 0 || !desc_dev) return SSHIP_OK;  // empty handle -> empty Mat (LightGlue.cc:461-462)
  if (!out || dim <= 0) return fail(SSHIP_ERR_INVALID, "desc_to_host: bad arguments");
  const size_t n = (size_t)count * dim;
  std::vector<uint16_t> tmp(n);
  SSHIP_HIP_CHECK(hipMemcpy(tmp.data(), desc_dev, n * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) out[i] = half_bits_to_float(tmp[i]);
  return SSHIP_OK;
}
extern "C" int sship_sp_infer_host(sship_sp* sp, const uint8_t* img, int h, int w, int stride, int channels, float* kp_xys,
                                   float* desc_f32, int* n) {
  bind_thread();
  if (!sp || !img || !kp_xys || !desc_f32 || !n) return fail(SSHIP_ERR_INVALID, "sp_infer_host: null argument");
  sship_features f{};
  f.kp_xys = kp_xys;
  if (int rc = sship_sp_extract(sp, img, h, w, stride, channels, &f)) return rc;
  *n = f.n;
  int rc = SSHIP_OK;
  if (f.n > 0) rc = sship_desc_to_host(f.desc_dev, f.n, SSHIP_DESC_DIM, desc_f32);
  if (f.slot >= 0) sship_pool_release(sp->pool, f.slot);
  return rc;
}

// ====================================================================================================
// LightGlue
// ====================================================================================================
constexpr int kLgLayers = 9;
struct sship_lg_weights {
  std::mutex mu;
  int refs = 1;
  ConvW qkv[kLgLayers], ffn0_s[kLgLayers], ffn3_s[kLgLayers];  // ffn0_*: out_proj / to_out folded in
  ConvW qkv_t[kLgLayers], cqkv_t[kLgLayers], final_t;            // same projections packed per wave for the FFN tail
  ConvW cqkv[kLgLayers], ffn0_c[kLgLayers], ffn3_c[kLgLayers];
  float *ln_g_s[kLgLayers] = {}, *ln_b_s[kLgLayers] = {}, *ln_g_c[kLgLayers] = {}, *ln_b_c[kLgLayers] = {};
  float* match_w = nullptr;
  float match_b = 0.f;
  float* wr = nullptr;
  // adaptive depth (sship_lg_set_depth_confidence): token_confidence[0..7] and log_assignment[0..7], when the file holds them.  The
  // nine assignment heads sit at a fixed stride (head h at h * 65536) so that a kernel selects one by index; head 8 is the packed final_t
  // above and is not used from here.
  bool has_depth = false;
  std::string depth_missing;   // the first missing tensor (the error text of sship_lg_set_depth_confidence)
  float* tc_w = nullptr;       // [8][256]
  float tc_b[8] = {};
  float* head_wt = nullptr;    // [9][256 in][256 out]: final_proj^T, scaled by 256^-0.25 like final_t
  float* head_b = nullptr;     // [9][256], scaled likewise
  float* head_mw = nullptr;    // [9][256] matchability weights
  float* head_mb = nullptr;    // [9]
  // adaptive width (sship_lg_set_width_confidence) needs log_assignment.{0..7}.matchability only: head_mw / head_mb are uploaded when the
  // file holds those, whether or not the rest of the depth heads is there
  bool has_width = false;
  std::string width_missing;
};
static void lg_weights_free(sship_lg_weights* w) {
  for (int i = 0; i < kLgLayers; ++i) {
    for (ConvW* c : {&w->qkv[i], &w->ffn0_s[i], &w->ffn3_s[i], &w->cqkv[i], &w->ffn0_c[i], &w->ffn3_c[i], &w->qkv_t[i], &w->cqkv_t[i]})
      free_conv(*c);
    for (float* p : {w->ln_g_s[i], w->ln_b_s[i], w->ln_g_c[i], w->ln_b_c[i]}) if (p) (void)hipFree(p);
  }
  free_conv(w->final_t);
  for (float* p : {w->tc_w, w->head_wt, w->head_b, w->head_mw, w->head_mb}) if (p) (void)hipFree(p);
  if (w->match_w) (void)hipFree(w->match_w);
  if (w->wr) (void)hipFree(w->wr);
  delete w;
}

extern "C" int sship_lg_weights_load(const char* path, sship_lg_weights** out) {
  bind_thread();
  if (!path || !out) return fail(SSHIP_ERR_INVALID, "lg_weights_load: null argument");
  if (int rc = require_device()) return rc;
  StateDict sd; std::string err;
  if (!load_safetensors(path, sd, err)) return fail(SSHIP_ERR_IO, err);
  // The published checkpoint (superpoint_lightglue.pth) names the blocks self_attn.{i}.* / cross_attn.{i}.*; upstream's
  // LightGlue.__init__ renames them to transformers.{i}.self_attn.* / .cross_attn.* at load time, which is also what
  // matcher.state_dict() (the module the reference exports, utils/convert_lightglue_to_onnx.py:64-74) holds.  Accept both,
  // and an optional "matcher." prefix (a state dict saved from a wrapper module).
  {
    StateDict renamed;
    for (auto& kv : sd) {
      std::string k = kv.first;
      if (k.compare(0, 8, "matcher.") == 0) k = k.substr(8);
      for (const char* blk : {"self_attn.", "cross_attn."}) {
        const size_t bl = strlen(blk);
        if (k.compare(0, bl, blk) == 0) {
          const size_t dot = k.find('.', bl);
          if (dot != std::string::npos && dot > bl && k.find_first_not_of("0123456789", bl) == dot)
            k = "transformers." + k.substr(bl, dot - bl) + "." + std::string(blk, bl - 1) + k.substr(dot);
        }
      }
      renamed[k] = std::move(kv.second);
    }
    sd.swap(renamed);
  }
  sship_lg_weights* w = new sship_lg_weights();
  auto bail = [&](int rc, const std::string& m) { lg_weights_free(w); return fail(rc, m); };
  auto lin = [&](const std::string& name, int cout, int cin, ConvW& dst, const std::vector<int>* map = nullptr,
                 const std::vector<float>* scale = nullptr) -> int {
    const Tensor* wt = find_tensor(sd, name + ".weight", {cout, cin}, err);
    const Tensor* bs = wt ? find_tensor(sd, name + ".bias", {cout}, err) : nullptr;
    if (!wt || !bs) return SSHIP_ERR_IO;
    // 256-row layers use 64-row workgroup tiles (more workgroups for the small token GEMMs), wider ones 128.
    return upload_conv(wt->data.data(), bs->data.data(), cout, cin, 1, cout <= 256 ? 64 : 128, dst, map, scale);
  };
  // FFN of a block with the attention output projection folded into ffn.0:
  //   ffn.0(cat[x, Wo c + bo]) = cat[x, c] [W0a | W0b Wo]^T + (b0 + W0b bo)      (fp64 accumulate on the host)
  // ffn.0' is packed in 64-row blocks and ffn.3 in 32-row blocks: one block per wave of k_lg_ffn.
  auto ffn = [&](const std::string& p, const char* proj, ConvW& d0, ConvW& d3) -> int {
    const Tensor* wo = find_tensor(sd, p + proj + ".weight", {256, 256}, err);
    const Tensor* bo = wo ? find_tensor(sd, p + proj + ".bias", {256}, err) : nullptr;
    const Tensor* w0 = bo ? find_tensor(sd, p + "ffn.0.weight", {512, 512}, err) : nullptr;
    const Tensor* b0 = w0 ? find_tensor(sd, p + "ffn.0.bias", {512}, err) : nullptr;
    const Tensor* w3 = b0 ? find_tensor(sd, p + "ffn.3.weight", {256, 512}, err) : nullptr;
    const Tensor* b3 = w3 ? find_tensor(sd, p + "ffn.3.bias", {256}, err) : nullptr;
    if (!b3) return SSHIP_ERR_IO;
    std::vector<float> wf(512 * 512), bf(512);
    for (int o = 0; o < 512; ++o) {
      const float* row = w0->data.data() + (size_t)o * 512;
      for (int i = 0; i < 256; ++i) wf[(size_t)o * 512 + i] = row[i];
      double bacc = b0->data[o];
      for (int k = 0; k < 256; ++k) bacc += (double)row[256 + k] * bo->data[k];
      bf[o] = (float)bacc;
      for (int i = 0; i < 256; ++i) {
        double a = 0.0;
        for (int k = 0; k < 256; ++k) a += (double)row[256 + k] * wo->data[(size_t)k * 256 + i];
        wf[(size_t)o * 512 + 256 + i] = (float)a;
      }
    }
    if (int rc = upload_conv(wf.data(), bf.data(), 512, 512, 1, 64, d0)) return rc;
    return upload_conv(w3->data.data(), b3->data.data(), 256, 512, 1, 32, d3);
  };
  auto vec = [&](const std::string& name, int n, float** dst) -> int {
    const Tensor* t = find_tensor(sd, name, {n}, err);
    if (!t) return SSHIP_ERR_IO;
    return upload_floats(t->data.data(), n, dst);
  };
  const float kLog2e = 1.4426950408889634f;
  // SelfBlock Wqkv: unflatten(-1, (4, 64, 3)) -> original row f = h*192 + d*3 + c ; new row R = c*256 + h*64 + d.
  std::vector<int> qkv_map(768);
  std::vector<float> qkv_scale(768, 1.f);
  for (int c = 0; c < 3; ++c)
    for (int h = 0; h < 4; ++h)
      for (int d = 0; d < 64; ++d) {
        const int R = c * 256 + h * 64 + d;
        qkv_map[R] = h * 192 + d * 3 + c;
        if (c == 0) qkv_scale[R] = 0.125f * kLog2e;  // softmax(q k^T / sqrt(64)) evaluated with exp2
      }
  // CrossBlock: both qk sides are scaled by 64^-0.25; sqrt(log2 e) on each side turns exp into exp2.
  std::vector<float> cq_scale(256, powf(64.f, -0.25f) * sqrtf(kLog2e));
  std::vector<float> fp_scale(256, powf(256.f, -0.25f));  // mdesc = final_proj(x) / d^0.25
  for (int i = 0; i < kLgLayers; ++i) {
    const std::string ps = "transformers." + std::to_string(i) + ".self_attn.";
    const std::string pc = "transformers." + std::to_string(i) + ".cross_attn.";
    int rc = 0;
    if ((rc = lin(ps + "Wqkv", 768, 256, w->qkv[i], &qkv_map, &qkv_scale))) return bail(rc, err);
    {
      const Tensor* wt = find_tensor(sd, ps + "Wqkv.weight", {768, 256}, err);
      const Tensor* bs = find_tensor(sd, ps + "Wqkv.bias", {768}, err);
      if ((rc = upload_conv(wt->data.data(), bs->data.data(), 768, 256, 1, 96, w->qkv_t[i], &qkv_map, &qkv_scale, true))) return bail(rc, g_err);
    }
    if ((rc = ffn(ps, "out_proj", w->ffn0_s[i], w->ffn3_s[i]))) return bail(rc, err.empty() ? g_err : err);
    if ((rc = vec(ps + "ffn.1.weight", 512, &w->ln_g_s[i]))) return bail(rc, err);
    if ((rc = vec(ps + "ffn.1.bias", 512, &w->ln_b_s[i]))) return bail(rc, err);
    // fused [to_qk ; to_v] -> one 512-row GEMM
    const Tensor* wqk = find_tensor(sd, pc + "to_qk.weight", {256, 256}, err);
    const Tensor* bqk = wqk ? find_tensor(sd, pc + "to_qk.bias", {256}, err) : nullptr;
    const Tensor* wv = bqk ? find_tensor(sd, pc + "to_v.weight", {256, 256}, err) : nullptr;
    const Tensor* bv = wv ? find_tensor(sd, pc + "to_v.bias", {256}, err) : nullptr;
    if (!bv) return bail(SSHIP_ERR_IO, err);
    std::vector<float> wcat(512 * 256), bcat(512), scat(512, 1.f);
    memcpy(wcat.data(), wqk->data.data(), 256 * 256 * 4);
    memcpy(wcat.data() + 256 * 256, wv->data.data(), 256 * 256 * 4);
    memcpy(bcat.data(), bqk->data.data(), 256 * 4);
    memcpy(bcat.data() + 256, bv->data.data(), 256 * 4);
    for (int r = 0; r < 256; ++r) scat[r] = cq_scale[r];
    if ((rc = upload_conv(wcat.data(), bcat.data(), 512, 256, 1, 128, w->cqkv[i], nullptr, &scat))) return bail(rc, g_err);
    if ((rc = upload_conv(wcat.data(), bcat.data(), 512, 256, 1, 64, w->cqkv_t[i], nullptr, &scat, true))) return bail(rc, g_err);
    if ((rc = ffn(pc, "to_out", w->ffn0_c[i], w->ffn3_c[i]))) return bail(rc, err.empty() ? g_err : err);
    if ((rc = vec(pc + "ffn.1.weight", 512, &w->ln_g_c[i]))) return bail(rc, err);
    if ((rc = vec(pc + "ffn.1.bias", 512, &w->ln_b_c[i]))) return bail(rc, err);
  }
  {
    // depth_confidence = -1 -> only log_assignment[n_layers - 1] is evaluated (convert_lightglue_to_onnx.py:71-74)
    const std::string pa = "log_assignment." + std::to_string(kLgLayers - 1) + ".";
    int rc = 0;
    {
      const Tensor* wt = find_tensor(sd, pa + "final_proj.weight", {256, 256}, err);
      const Tensor* bs = find_tensor(sd, pa + "final_proj.bias", {256}, err);
      if ((rc = upload_conv(wt->data.data(), bs->data.data(), 256, 256, 1, 32, w->final_t, nullptr, &fp_scale))) return bail(rc, g_err);
    }
    const Tensor* mw = find_tensor(sd, pa + "matchability.weight", {1, 256}, err);
    const Tensor* mb = mw ? find_tensor(sd, pa + "matchability.bias", {1}, err) : nullptr;
    if (!mb) return bail(SSHIP_ERR_IO, err);
    if ((rc = upload_floats(mw->data.data(), 256, &w->match_w))) return bail(rc, g_err);
    w->match_b = mb->data[0];
    const Tensor* wr = find_tensor(sd, "posenc.Wr.weight", {32, 2}, err);
    if (!wr) return bail(SSHIP_ERR_IO, err);
    if ((rc = upload_floats(wr->data.data(), 64, &w->wr))) return bail(rc, g_err);
  }
  {
    // adaptive depth's heads: optional (a file without them loads as before; sship_lg_set_depth_confidence refuses to turn it on)
    auto opt = [&](const std::string& name, std::initializer_list<int64_t> shape) -> const Tensor* {
      auto it = sd.find(name);
      if (it != sd.end() && it->second.shape == std::vector<int64_t>(shape)) return &it->second;
      if (w->depth_missing.empty()) w->depth_missing = name;
      return nullptr;
    };
    std::vector<float> tcw(8 * 256), hwt((size_t)9 * 65536, 0.f), hb(9 * 256, 0.f), hmw(9 * 256, 0.f), hmb(9, 0.f);
    const float sc = fp_scale[0];
    bool ok = true;
    for (int i = 0; i < kLgLayers - 1 && ok; ++i) {
      const std::string pt = "token_confidence." + std::to_string(i) + ".token.0.";
      const std::string pa = "log_assignment." + std::to_string(i) + ".";
      const Tensor* tw = opt(pt + "weight", {1, 256});
      const Tensor* tb = tw ? opt(pt + "bias", {1}) : nullptr;
      const Tensor* fw = tb ? opt(pa + "final_proj.weight", {256, 256}) : nullptr;
      const Tensor* fb = fw ? opt(pa + "final_proj.bias", {256}) : nullptr;
      const Tensor* mw = fb ? opt(pa + "matchability.weight", {1, 256}) : nullptr;
      const Tensor* mb = mw ? opt(pa + "matchability.bias", {1}) : nullptr;
      if (!mb) { ok = false; break; }
      memcpy(tcw.data() + i * 256, tw->data.data(), 256 * 4);
      w->tc_b[i] = tb->data[0];
      for (int o = 0; o < 256; ++o) {
        for (int k = 0; k < 256; ++k) hwt[(size_t)i * 65536 + (size_t)k * 256 + o] = fw->data[(size_t)o * 256 + k] * sc;
        hb[i * 256 + o] = fb->data[o] * sc;
      }
      memcpy(hmw.data() + i * 256, mw->data.data(), 256 * 4);
      hmb[i] = mb->data[0];
    }
    if (ok) {
      int rc = 0;
      if ((rc = upload_floats(tcw.data(), tcw.size(), &w->tc_w)) || (rc = upload_floats(hwt.data(), hwt.size(), &w->head_wt)) ||
          (rc = upload_floats(hb.data(), hb.size(), &w->head_b)) || (rc = upload_floats(hmw.data(), hmw.size(), &w->head_mw)) ||
          (rc = upload_floats(hmb.data(), hmb.size(), &w->head_mb)))
        return bail(rc, g_err);
      w->has_depth = true;
      w->has_width = true;
      w->depth_missing.clear();
    } else {
      // adaptive width alone: the eight matchability heads
      bool okw = true;
      for (int i = 0; i < kLgLayers - 1 && okw; ++i) {
        const std::string pa = "log_assignment." + std::to_string(i) + ".matchability.";
        auto iw = sd.find(pa + "weight"), ib = sd.find(pa + "bias");
        if (iw == sd.end() || iw->second.shape != std::vector<int64_t>({1, 256})) { w->width_missing = pa + "weight"; okw = false; break; }
        if (ib == sd.end() || ib->second.shape != std::vector<int64_t>({1})) { w->width_missing = pa + "bias"; okw = false; break; }
        memcpy(hmw.data() + i * 256, iw->second.data.data(), 256 * 4);
        hmb[i] = ib->second.data[0];
      }
      if (okw) {
        int rc = 0;
        if ((rc = upload_floats(hmw.data(), hmw.size(), &w->head_mw)) || (rc = upload_floats(hmb.data(), hmb.size(), &w->head_mb)))
          return bail(rc, g_err);
        w->has_width = true;
      }
    }
  }
  *out = w;
  return SSHIP_OK;
}
extern "C" void sship_lg_weights_retain(sship_lg_weights* w) {
  bind_thread();
  if (!w) return;
  std::lock_guard<std::mutex> g(w->mu);
  ++w->refs;
}
extern "C" void sship_lg_weights_release(sship_lg_weights* w) {
  bind_thread();
  if (!w) return;
  bool last;
  { std::lock_guard<std::mutex> g(w->mu); last = (--w->refs == 0); }
  if (last) lg_weights_free(w);
}

// Word offsets inside one slot of sship_lg::cap_ad: lens [9][2] | rope [9][2 NP][64] | ind [8][2 NP] | prune [8][2 NP] | wlen [8][2] | chg [8][2] |
// cnt [8] | layers_run [1] | mc [max_kp] | msc [max_kp]
struct LgCapAd {
  size_t lens, rope, ind, prune, wlen, chg, cnt, lr, mc, msc, words;
  LgCapAd() : LgCapAd(0, 0) {}
  LgCapAd(int NP, int max_kp) {
    const size_t np2 = (size_t)2 * NP;
    lens = 0;
    rope = lens + 9 * 2;
    ind = rope + 9 * np2 * 64;
    prune = ind + 8 * np2;
    wlen = prune + 8 * np2;
    chg = wlen + 8 * 2;
    cnt = chg + 8 * 2;
    lr = cnt + 8;
    mc = lr + 1;
    msc = mc + (size_t)max_kp;
    words = msc + (size_t)max_kp;
  }
};
struct sship_lg {
  sship_lg_weights* w = nullptr;
  int image_w = 0, image_h = 0, max_kp = 0, max_pairs = 0, NP = 0;
  hipStream_t stream = nullptr;
  DevBuf x, rope, q, k, vt, ctx, md, logsig, sim, ws;
  DevBuf kp_stage, desc_stage, lens, m0, ms0;
  DevBuf lens_c;  // per-sequence counts clamped to [0, max_kp] by k_lg_prep: what every later kernel of the call reads
  DevBuf kpn;     // normalised keypoints [S*NP][2] f32 (src/LightGlue.cc:241-251 on the device; read back by sship_lg_debug_read)
  int debug_layers = kLgLayers;  // sship_lg_debug_set_layers
  int last_pairs = 0;
  // adaptive depth (sship_lg_set_depth_confidence): <= 0 = off.  dep: the per-call state of include/.../kernels.h LgDepth for every pair
  float depth_conf = -1.f;
  bool last_adaptive = false;
  int last_layers = kLgLayers;
  DevBuf dep;
  // adaptive width (sship_lg_set_width_confidence): <= 0 = off.  wid: the per-call state of kernels.h LgWidth for every pair;
  // m0c / ms0c: the matches of the live sets before they are mapped back through ind
  float width_conf = -1.f;
  int width_min_kp = 0;
  bool last_width = false;
  DevBuf wid, m0c, ms0c;
  PinBuf h_kp, h_lens, h_m0, h_ms0, h_desc;
  // throughput batches run their transformer layers as two half-batches on two streams (lg_forward): the second stream and the
  // fork / join events
  static constexpr int kAux = 3;
  hipStream_t aux[kAux] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[kAux] = {nullptr, nullptr, nullptr};
  // test-only stage capture (include/sship.h: sship_lg_debug_capture): cap_n = 0 is off.  cap: fp16 [slot][layer][stage 0..9][2 NP][256],
  // cap_md: fp16 [slot][2 NP][256], cap_ls: f32 [slot][2 NP]; allocated when capture is first switched on
  static constexpr int kCapSlots = 8, kCapStages = 10;
  int cap_n = 0, cap_pairs[kCapSlots] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool captured = false;
  int cap_last_pairs = 0;
  DevBuf cap, cap_md, cap_ls;
  // the same capture with adaptive depth / width on (sship_lg_debug_adaptive): cap_ad holds, per slot, cap_lay.words 4-byte words
  // (layout: LgCapAd, set when capture is switched on), cap_amd / cap_als the md (fp16 [2 NP][256]) / logsig (f32 [2 NP]) the assignment read
  bool cap_last_adaptive = false, cap_last_width = false, cap_last_assigned = false;
  LgCapAd cap_lay;
  DevBuf cap_ad, cap_amd, cap_als;
};

// Adaptive depth state layout in sship_lg::dep (ints): cnt [P][8] | layers_run [P] | lens_live [2P] | live [P + kAux + 1] | tickets [kAux + 1]
static size_t lg_dep_ints(int P) { return (size_t)P * 8 + P + 2 * (size_t)P + P + sship_lg::kAux + 1 + sship_lg::kAux + 1; }
// Adaptive width state layout in sship_lg::wid (ints): wlen [2P] | chg [2P] | ind [2P][NP] | prune [2P][NP] | tiles | rtiles, the tile lists
// sized for 32-token tiles: [P * 2 NP / 32 + kAux + 1] each (a count in front of every launch group's list)
static size_t lg_wid_list_ints(int P, int NP) { return (size_t)P * (2 * NP / 32) + sship_lg::kAux + 1; }
static size_t lg_wid_ints(int P, int NP) { return 4 * (size_t)P + 4 * (size_t)P * NP + 2 * lg_wid_list_ints(P, NP); }
extern "C" int sship_lg_create(sship_lg_weights* w, int image_w, int image_h, int max_kp, int max_pairs, sship_lg** out) {
  bind_thread();
  if (!w || !out || image_w <= 0 || image_h <= 0) return fail(SSHIP_ERR_INVALID, "lg_create: bad arguments");
  if (max_kp <= 0 || max_kp > kMaxKp) return fail(SSHIP_ERR_INVALID, "lg_create: max_keypoints must be in [1, 4096]");
  if (max_pairs <= 0) max_pairs = 1;
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_lg> lg(new sship_lg());
  lg->image_w = image_w; lg->image_h = image_h; lg->max_kp = max_kp; lg->max_pairs = max_pairs;
  lg->NP = (max_kp + 31) / 32 * 32;  // 32-token granularity: 600 keypoints -> 608 tokens (128-granular padding was 6.7 % dead work)

  const size_t S = 2 * (size_t)max_pairs, T = S * lg->NP, NP = lg->NP;
  SSHIP_HIP_CHECK(lg->x.ensure(T * 256 * 2));
  SSHIP_HIP_CHECK(lg->rope.ensure(T * 64 * 4));
  SSHIP_HIP_CHECK(lg->q.ensure(T * 256 * 2));
  SSHIP_HIP_CHECK(lg->k.ensure(T * 256 * 2));
  SSHIP_HIP_CHECK(lg->vt.ensure(T * 256 * 2));
  SSHIP_HIP_CHECK(lg->ctx.ensure(T * 256 * 2));
  SSHIP_HIP_CHECK(lg->md.ensure(T * 256 * 2));
  SSHIP_HIP_CHECK(lg->logsig.ensure(T * 4));
  SSHIP_HIP_CHECK(lg->sim.ensure((size_t)max_pairs * NP * NP * 4));
  SSHIP_HIP_CHECK(lg->ws.ensure((size_t)max_pairs * 5 * NP * 4));
  SSHIP_HIP_CHECK(lg->kp_stage.ensure(S * max_kp * 3 * 4));
  SSHIP_HIP_CHECK(lg->desc_stage.ensure(S * max_kp * 256 * 2));
  SSHIP_HIP_CHECK(lg->lens.ensure(S * 4));
  SSHIP_HIP_CHECK(lg->lens_c.ensure(S * 4));
  SSHIP_HIP_CHECK(lg->kpn.ensure(T * 2 * 4));
  SSHIP_HIP_CHECK(lg->m0.ensure((size_t)max_pairs * max_kp * 4));
  SSHIP_HIP_CHECK(lg->ms0.ensure((size_t)max_pairs * max_kp * 4));
  SSHIP_HIP_CHECK(lg->h_kp.ensure(2 * (size_t)max_kp * 3 * 4));
  SSHIP_HIP_CHECK(lg->h_lens.ensure(2 * 4));
  SSHIP_HIP_CHECK(lg->h_m0.ensure((size_t)max_kp * 4));
  SSHIP_HIP_CHECK(lg->h_ms0.ensure((size_t)max_kp * 4));
  SSHIP_HIP_CHECK(lg->h_desc.ensure(2 * (size_t)max_kp * 256 * 2));
  SSHIP_HIP_CHECK(lg->dep.ensure(lg_dep_ints(max_pairs) * 4));
  SSHIP_HIP_CHECK(lg->wid.ensure(lg_wid_ints(max_pairs, lg->NP) * 4));
  SSHIP_HIP_CHECK(lg->m0c.ensure((size_t)max_pairs * max_kp * 4));
  SSHIP_HIP_CHECK(lg->ms0c.ensure((size_t)max_pairs * max_kp * 4));
  // q/k/vt/ctx of padded tokens must stay finite: start from zeros (prep rewrites x every call).
  SSHIP_HIP_CHECK(hipMemset(lg->q.p, 0, lg->q.bytes));
  SSHIP_HIP_CHECK(hipMemset(lg->k.p, 0, lg->k.bytes));
  SSHIP_HIP_CHECK(hipMemset(lg->vt.p, 0, lg->vt.bytes));
  SSHIP_HIP_CHECK(hipMemset(lg->ctx.p, 0, lg->ctx.bytes));
  // from here on the handle owns streams / events: hand it to sship_lg_destroy on any failure (w is still null: nothing to release)
  std::unique_ptr<sship_lg, void (*)(sship_lg*)> owned(lg.release(), sship_lg_destroy);
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&owned->stream, hipStreamDefault));
  for (int i = 0; i < sship_lg::kAux; ++i) {
    SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&owned->aux[i], hipStreamNonBlocking));
    SSHIP_HIP_CHECK(hipEventCreateWithFlags(&owned->ev_join[i], hipEventDisableTiming));
  }
  SSHIP_HIP_CHECK(hipEventCreateWithFlags(&owned->ev_fork, hipEventDisableTiming));
  sship_lg_weights_retain(w);
  owned->w = w;
  *out = owned.release();
  return SSHIP_OK;
}
extern "C" void sship_lg_destroy(sship_lg* lg) {
  bind_thread();
  if (!lg) return;
  (void)hipDeviceSynchronize();
  if (lg->stream) (void)hipStreamDestroy(lg->stream);
  for (int i = 0; i < sship_lg::kAux; ++i) {
    if (lg->aux[i]) (void)hipStreamDestroy(lg->aux[i]);
    if (lg->ev_join[i]) (void)hipEventDestroy(lg->ev_join[i]);
  }
  if (lg->ev_fork) (void)hipEventDestroy(lg->ev_fork);
  sship_lg_weights_release(lg->w);
  delete lg;
}
extern "C" int sship_lg_normalize_keypoints(const sship_lg* lg, const float* kp, int stride, int n, float* out) {
  if (!lg || !kp || !out || stride < 2) return fail(SSHIP_ERR_INVALID, "lg_normalize_keypoints: bad arguments");
  const float scale = std::max(lg->image_w, lg->image_h) / 2.0f;  // LightGlue.cc:242-244
  const float cx = lg->image_w / 2.0f, cy = lg->image_h / 2.0f;
  for (int i = 0; i < n; ++i) {
    out[2 * i + 0] = (kp[(size_t)i * stride + 0] - cx) / scale;
    out[2 * i + 1] = (kp[(size_t)i * stride + 1] - cy) / scale;
  }
  return SSHIP_OK;
}

// Test-only introspection (include/sship.h): truncate the matcher after n layers / read its internal state back.
extern "C" int sship_lg_debug_set_layers(sship_lg* lg, int n_layers) {
  if (!lg || n_layers < 1 || n_layers > kLgLayers) return fail(SSHIP_ERR_INVALID, "lg_debug_set_layers: n_layers must be in [1, 9]");
  lg->debug_layers = n_layers;
  return SSHIP_OK;
}
extern "C" int sship_lg_debug_read(sship_lg* lg, int what, int index, int rows, int cols, float* out) {
  bind_thread();
  if (!lg || !out || rows <= 0 || index < 0) return fail(SSHIP_ERR_INVALID, "lg_debug_read: bad arguments");
  const int NP = lg->NP, S = 2 * lg->last_pairs;
  if (rows > NP) return fail(SSHIP_ERR_INVALID, "lg_debug_read: rows exceeds the padded sequence length");
  SSHIP_HIP_CHECK(hipDeviceSynchronize());
  switch (what) {
    case SSHIP_LG_DEBUG_X: {  // residual stream of sequence `index`: fp16 [NP][256]
      if (index >= S || cols != 256) return fail(SSHIP_ERR_INVALID, "lg_debug_read(X): index/cols");
      std::vector<uint16_t> tmp((size_t)rows * 256);
      SSHIP_HIP_CHECK(hipMemcpy(tmp.data(), lg->x.as<_Float16>() + (size_t)index * NP * 256, tmp.size() * 2, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < tmp.size(); ++i) out[i] = half_bits_to_float(tmp[i]);
      return SSHIP_OK;
    }
    case SSHIP_LG_DEBUG_SIM: {  // assignment similarity of pair `index`: f32 [NP][NP]
      if (index >= S / 2 || cols <= 0 || cols > NP) return fail(SSHIP_ERR_INVALID, "lg_debug_read(SIM): index/cols");
      // the match itself never materialises the matrix: computed here, on demand, from the final projections of the last call
      launch_lg_sim(lg->md.as<_Float16>(), lg->lens_c.as<int>(), LgDims{S, NP}, lg->sim.as<float>(), lg->stream);
      SSHIP_HIP_CHECK(hipStreamSynchronize(lg->stream));
      SSHIP_HIP_CHECK(hipMemcpy2D(out, (size_t)cols * 4, lg->sim.as<float>() + (size_t)index * NP * NP, (size_t)NP * 4, (size_t)cols * 4, rows,
                                  hipMemcpyDeviceToHost));
      return SSHIP_OK;
    }
    case SSHIP_LG_DEBUG_KPTS: {  // normalised keypoints of sequence `index`: f32 [NP][2]
      if (index >= S || cols != 2) return fail(SSHIP_ERR_INVALID, "lg_debug_read(KPTS): index/cols");
      SSHIP_HIP_CHECK(hipMemcpy(out, lg->kpn.as<float>() + (size_t)index * NP * 2, (size_t)rows * 8, hipMemcpyDeviceToHost));
      return SSHIP_OK;
    }
    case SSHIP_LG_DEBUG_ROPE: {  // rotary table of sequence `index`: f32 [NP][32] (cos, sin) pairs
      if (index >= S || cols != 64) return fail(SSHIP_ERR_INVALID, "lg_debug_read(ROPE): index/cols");
      SSHIP_HIP_CHECK(hipMemcpy(out, lg->rope.as<float>() + (size_t)index * NP * 64, (size_t)rows * 256, hipMemcpyDeviceToHost));
      return SSHIP_OK;
    }
    case SSHIP_LG_DEBUG_IND: {  // original keypoint index of the rows of sequence `index` (identity when adaptive width was off)
      if (index >= S || cols != 1) return fail(SSHIP_ERR_INVALID, "lg_debug_read(IND): index/cols");
      if (!lg->last_width) {
        for (int i = 0; i < rows; ++i) out[i] = (float)i;
        return SSHIP_OK;
      }
      std::vector<int> tmp((size_t)rows);
      SSHIP_HIP_CHECK(hipMemcpy(tmp.data(), lg->wid.as<int>() + 4 * (size_t)lg->max_pairs + (size_t)index * NP, tmp.size() * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < rows; ++i) out[i] = (float)tmp[i];
      return SSHIP_OK;
    }
    default: return fail(SSHIP_ERR_INVALID, "lg_debug_read: unknown selector");
  }
}

// Test-only stage capture (include/sship.h).  A pair's slice of every token buffer is contiguous: sequences 2p, 2p + 1 = 2 NP rows of 256.
extern "C" int sship_lg_debug_capture(sship_lg* lg, const int* pairs, int count) {
  bind_thread();
  if (!lg || count < 0 || count > sship_lg::kCapSlots || (count > 0 && !pairs))
    return fail(SSHIP_ERR_INVALID, "lg_debug_capture: null handle, or count outside 0..8");
  for (int i = 0; i < count; ++i) {
    if (pairs[i] < 0) return fail(SSHIP_ERR_INVALID, "lg_debug_capture: negative pair index");
    for (int k = 0; k < i; ++k)
      if (pairs[k] == pairs[i]) return fail(SSHIP_ERR_INVALID, "lg_debug_capture: repeated pair index");
  }
  SSHIP_HIP_CHECK(hipDeviceSynchronize());  // copies of an earlier call may still be in flight
  if (count > 0) {
    const size_t pair_halfs = (size_t)2 * lg->NP * 256;
    SSHIP_HIP_CHECK(lg->cap.ensure((size_t)sship_lg::kCapSlots * kLgLayers * sship_lg::kCapStages * pair_halfs * 2));
    SSHIP_HIP_CHECK(lg->cap_md.ensure((size_t)sship_lg::kCapSlots * pair_halfs * 2));
    SSHIP_HIP_CHECK(lg->cap_ls.ensure((size_t)sship_lg::kCapSlots * 2 * lg->NP * 4));
    lg->cap_lay = LgCapAd(lg->NP, lg->max_kp);
    SSHIP_HIP_CHECK(lg->cap_ad.ensure((size_t)sship_lg::kCapSlots * lg->cap_lay.words * 4));
    SSHIP_HIP_CHECK(lg->cap_amd.ensure((size_t)sship_lg::kCapSlots * pair_halfs * 2));
    SSHIP_HIP_CHECK(lg->cap_als.ensure((size_t)sship_lg::kCapSlots * 2 * lg->NP * 4));
  }
  for (int i = 0; i < count; ++i) lg->cap_pairs[i] = pairs[i];
  lg->cap_n = count;
  lg->captured = false;
  return SSHIP_OK;
}
// The inverses of the fragment orders the projections store in, written from the consumer's side (what k_lg_attention's operand loads
// expect of a 32-token tile of 2048 halfs), not from the epilogues that write them:
//   Q / K  B fragment of K-step ks: lane (token j = lane % 32, half hh = lane / 32) holds channels d = 16 ks + 8 hh + e, e = 0 .. 7
//   V^T    A fragment of PV K-step kk, M-tile mt: lane (channel d = 32 mt + lane % 32, hh = lane / 32) holds the 8 keys of the swapped QK^T
//          C-layout, key = 16 kk + 4 hh + (e % 4) + 8 (e / 4)
static void lg_unpermute_qk(const uint16_t* src, int NP, float* out) {  // src [4 heads][NP / 32 tiles][2048] -> out [NP][256]
  const int nt32 = NP / 32;
  for (int h = 0; h < 4; ++h)
    for (int t = 0; t < nt32; ++t)
      for (int o = 0; o < 2048; ++o) {
        const int ks = o / 512, lane = (o % 512) / 8, e = o % 8;
        const int token = t * 32 + lane % 32, d = 16 * ks + 8 * (lane / 32) + e;
        out[(size_t)token * 256 + h * 64 + d] = half_bits_to_float(src[((size_t)h * nt32 + t) * 2048 + o]);
      }
}
static void lg_unpermute_vt(const uint16_t* src, int NP, float* out) {
  const int nt32 = NP / 32;
  for (int h = 0; h < 4; ++h)
    for (int t = 0; t < nt32; ++t)
      for (int o = 0; o < 2048; ++o) {
        const int kk = o / 1024, mt = (o / 512) % 2, lane = (o % 512) / 8, e = o % 8;
        const int token = t * 32 + 16 * kk + 4 * (lane / 32) + (e % 4) + 8 * (e / 4), d = 32 * mt + lane % 32;
        out[(size_t)token * 256 + h * 64 + d] = half_bits_to_float(src[((size_t)h * nt32 + t) * 2048 + o]);
      }
}
extern "C" int sship_lg_debug_stage(sship_lg* lg, int slot, int layer, int stage, float* out, unsigned long long floats) {
  bind_thread();
  if (!lg || !out) return fail(SSHIP_ERR_INVALID, "lg_debug_stage: null argument");
  if (lg->cap_n == 0 || !lg->captured) return fail(SSHIP_ERR_INVALID, "lg_debug_stage: capture is off or no call has run since it was switched on");
  if (slot < 0 || slot >= lg->cap_n || lg->cap_pairs[slot] >= lg->cap_last_pairs)
    return fail(SSHIP_ERR_INVALID, "lg_debug_stage: no such slot, or the last call did not hold its pair");
  if (layer < 0 || layer >= kLgLayers || stage < 0 || stage > SSHIP_LG_STAGE_LOGSIG || (stage >= SSHIP_LG_STAGE_MD && layer != kLgLayers - 1))
    return fail(SSHIP_ERR_INVALID, "lg_debug_stage: no such layer / stage");
  const int NP = lg->NP;
  const size_t pair_halfs = (size_t)2 * NP * 256;
  if (floats != (stage == SSHIP_LG_STAGE_LOGSIG ? (size_t)2 * NP : pair_halfs)) return fail(SSHIP_ERR_INVALID, "lg_debug_stage: bad size");
  SSHIP_HIP_CHECK(hipDeviceSynchronize());
  if (stage == SSHIP_LG_STAGE_LOGSIG) {
    SSHIP_HIP_CHECK(hipMemcpy(out, lg->cap_ls.as<float>() + (size_t)slot * 2 * NP, (size_t)2 * NP * 4, hipMemcpyDeviceToHost));
    return SSHIP_OK;
  }
  std::vector<uint16_t> tmp(pair_halfs);
  const _Float16* src = stage == SSHIP_LG_STAGE_MD
                            ? lg->cap_md.as<_Float16>() + (size_t)slot * pair_halfs
                            : lg->cap.as<_Float16>() + (((size_t)slot * kLgLayers + layer) * sship_lg::kCapStages + stage) * pair_halfs;
  SSHIP_HIP_CHECK(hipMemcpy(tmp.data(), src, pair_halfs * 2, hipMemcpyDeviceToHost));
  const bool qk = stage == SSHIP_LG_STAGE_Q_S || stage == SSHIP_LG_STAGE_K_S || stage == SSHIP_LG_STAGE_QK_C;
  const bool vt = stage == SSHIP_LG_STAGE_V_S || stage == SSHIP_LG_STAGE_V_C;
  for (int seq = 0; seq < 2; ++seq) {
    const uint16_t* s16 = tmp.data() + (size_t)seq * NP * 256;
    float* o = out + (size_t)seq * NP * 256;
    if (qk) lg_unpermute_qk(s16, NP, o);
    else if (vt) lg_unpermute_vt(s16, NP, o);
    else
      for (size_t i = 0; i < (size_t)NP * 256; ++i) o[i] = half_bits_to_float(s16[i]);
  }
  return SSHIP_OK;
}

// Test-only (include/sship.h): what the capture kept of the adaptive modes' state, as 4-byte values (int32 or f32 by item)
extern "C" int sship_lg_debug_adaptive(sship_lg* lg, int slot, int layer, int what, void* out, unsigned long long count) {
  bind_thread();
  if (!lg || !out) return fail(SSHIP_ERR_INVALID, "lg_debug_adaptive: null argument");
  if (lg->cap_n == 0 || !lg->captured || !lg->cap_last_adaptive)
    return fail(SSHIP_ERR_INVALID, "lg_debug_adaptive: capture is off, no call has run since it was switched on, or the last call ran with both adaptive modes off");
  if (slot < 0 || slot >= lg->cap_n || lg->cap_pairs[slot] >= lg->cap_last_pairs)
    return fail(SSHIP_ERR_INVALID, "lg_debug_adaptive: no such slot, or the last call did not hold its pair");
  const size_t NP = lg->NP, K = lg->max_kp;
  const LgCapAd& lay = lg->cap_lay;
  size_t off = 0, n = 0;
  int layers = 1;      // valid layers: [0, layers)
  bool need_width = false, need_assign = false;
  switch (what) {
    case SSHIP_LG_ADAPT_LENS: off = lay.lens + (size_t)layer * 2; n = 2; layers = kLgLayers; break;
    case SSHIP_LG_ADAPT_ROPE: off = lay.rope + (size_t)layer * 2 * NP * 64; n = 2 * NP * 64; layers = kLgLayers; break;
    case SSHIP_LG_ADAPT_IND: off = lay.ind + (size_t)layer * 2 * NP; n = 2 * NP; layers = kLgLayers - 1; need_width = true; break;
    case SSHIP_LG_ADAPT_PRUNE: off = lay.prune + (size_t)layer * 2 * NP; n = 2 * NP; layers = kLgLayers - 1; need_width = true; break;
    case SSHIP_LG_ADAPT_WLEN: off = lay.wlen + (size_t)layer * 2; n = 2; layers = kLgLayers - 1; need_width = true; break;
    case SSHIP_LG_ADAPT_CHG: off = lay.chg + (size_t)layer * 2; n = 2; layers = kLgLayers - 1; need_width = true; break;
    case SSHIP_LG_ADAPT_CNT: off = lay.cnt; n = 8; break;
    case SSHIP_LG_ADAPT_LAYERS_RUN: off = lay.lr; n = 1; break;
    case SSHIP_LG_ADAPT_MD: n = 2 * NP * 256; need_assign = true; break;
    case SSHIP_LG_ADAPT_LOGSIG: n = 2 * NP; need_assign = true; break;
    case SSHIP_LG_ADAPT_MATCHES_C: off = lay.mc; n = K; need_width = need_assign = true; break;
    case SSHIP_LG_ADAPT_MSCORES_C: off = lay.msc; n = K; need_width = need_assign = true; break;
    default: return fail(SSHIP_ERR_INVALID, "lg_debug_adaptive: unknown item");
  }
  if (layer < 0 || layer >= layers) return fail(SSHIP_ERR_INVALID, "lg_debug_adaptive: no such layer for this item");
  if ((need_width && !lg->cap_last_width) || (need_assign && !lg->cap_last_assigned))
    return fail(SSHIP_ERR_INVALID, "lg_debug_adaptive: the last call did not produce this item (adaptive width off, or a truncated run)");
  if (count != n) return fail(SSHIP_ERR_INVALID, "lg_debug_adaptive: bad size");
  SSHIP_HIP_CHECK(hipDeviceSynchronize());
  if (what == SSHIP_LG_ADAPT_MD) {
    std::vector<uint16_t> tmp(n);
    SSHIP_HIP_CHECK(hipMemcpy(tmp.data(), lg->cap_amd.as<_Float16>() + (size_t)slot * n, n * 2, hipMemcpyDeviceToHost));
    float* o = static_cast<float*>(out);
    for (size_t i = 0; i < n; ++i) o[i] = half_bits_to_float(tmp[i]);
    return SSHIP_OK;
  }
  const void* src = what == SSHIP_LG_ADAPT_LOGSIG ? static_cast<const void*>(lg->cap_als.as<float>() + (size_t)slot * n)
                                                  : static_cast<const void*>(lg->cap_ad.as<int>() + (size_t)slot * lay.words + off);
  SSHIP_HIP_CHECK(hipMemcpy(out, src, n * 4, hipMemcpyDeviceToHost));
  return SSHIP_OK;
}

// the state of launch group `part` (pairs [p0, p0 + np))
static LgDepth lg_depth_state(sship_lg* lg, int p0, int part) {
  const int P = lg->max_pairs;
  int* b = lg->dep.as<int>();
  int* cnt = b;
  int* lr = cnt + (size_t)P * 8;
  int* ll = lr + P;
  int* live = ll + 2 * (size_t)P;
  unsigned* tk = reinterpret_cast<unsigned*>(live + P + sship_lg::kAux + 1);
  // live lists of consecutive groups: [p0 + part, p0 + part + np + 1) never overlap (p0 grows by np, part by 1)
  return LgDepth{cnt + (size_t)p0 * 8, lr + p0, ll + 2 * (size_t)p0, live + p0 + part, tk + part};
}
// thr_i = clip(0.8 + 0.1 exp(-4 i / 9), 0, 1) (upstream LightGlue.confidence_threshold, n_layers = 9), rounded to fp32
static float lg_depth_threshold(int i) {
  const double t = 0.8 + 0.1 * std::exp(-4.0 * i / (double)kLgLayers);
  return (float)std::min(1.0, std::max(0.0, t));
}
extern "C" int sship_lg_set_depth_confidence(sship_lg* lg, float depth_confidence) {
  bind_thread();
  if (!lg) return fail(SSHIP_ERR_INVALID, "lg_set_depth_confidence: null handle");
  if (std::isnan(depth_confidence) || depth_confidence > 1.f)
    return fail(SSHIP_ERR_INVALID, "lg_set_depth_confidence: depth_confidence must be <= 1 (<= 0 turns adaptive depth off)");
  if (depth_confidence > 0.f && !lg->w->has_depth)
    return fail(SSHIP_ERR_INVALID, "lg_set_depth_confidence: the weights hold no token_confidence / early log_assignment heads (missing '" +
                                       lg->w->depth_missing + "'); adaptive depth needs token_confidence.{0..7} and log_assignment.{0..7}");
  lg->depth_conf = depth_confidence > 0.f ? depth_confidence : -1.f;
  return SSHIP_OK;
}
extern "C" int sship_lg_layers_run(sship_lg* lg, int* out_host, int pairs) {
  bind_thread();
  if (!lg || !out_host || pairs <= 0) return fail(SSHIP_ERR_INVALID, "lg_layers_run: bad arguments");
  if (pairs > lg->last_pairs) return fail(SSHIP_ERR_INVALID, "lg_layers_run: pairs exceeds the pairs of the last call");
  SSHIP_HIP_CHECK(hipDeviceSynchronize());
  if (!lg->last_adaptive) {
    for (int p = 0; p < pairs; ++p) out_host[p] = lg->last_layers;
    return SSHIP_OK;
  }
  SSHIP_HIP_CHECK(hipMemcpy(out_host, lg->dep.as<int>() + (size_t)lg->max_pairs * 8, (size_t)pairs * 4, hipMemcpyDeviceToHost));
  return SSHIP_OK;
}

// the width state of launch group `part` (pairs [p0, p0 + np))
static LgWidth lg_width_state(sship_lg* lg, int p0, int part) {
  const size_t P = lg->max_pairs, NP = lg->NP;
  int* b = lg->wid.as<int>();
  int* wlen = b;
  int* chg = wlen + 2 * P;
  int* ind = chg + 2 * P;
  int* prune = ind + 2 * P * NP;
  int* tiles = prune + 2 * P * NP;
  int* rtiles = tiles + lg_wid_list_ints((int)P, (int)NP);
  // tile lists of consecutive groups never overlap: a group's list holds at most np * 2 NP / 32 tiles behind its count
  const size_t lo = (size_t)p0 * (2 * NP / 32) + part;
  return LgWidth{wlen + 2 * (size_t)p0, chg + 2 * (size_t)p0, ind + 2 * (size_t)p0 * NP, prune + 2 * (size_t)p0 * NP, tiles + lo, rtiles + lo};
}
extern "C" int sship_lg_set_width_confidence(sship_lg* lg, float width_confidence, int min_keypoints) {
  bind_thread();
  if (!lg) return fail(SSHIP_ERR_INVALID, "lg_set_width_confidence: null handle");
  if (std::isnan(width_confidence) || width_confidence > 1.f || min_keypoints < 0)
    return fail(SSHIP_ERR_INVALID, "lg_set_width_confidence: width_confidence must be <= 1 (<= 0 turns adaptive width off) and min_keypoints >= 0");
  if (width_confidence > 0.f && !lg->w->has_width)
    return fail(SSHIP_ERR_INVALID, "lg_set_width_confidence: the weights hold no early matchability heads (missing '" +
                                       (lg->w->width_missing.empty() ? lg->w->depth_missing : lg->w->width_missing) +
                                       "'); adaptive width needs log_assignment.{0..7}.matchability");
  lg->width_conf = width_confidence > 0.f ? width_confidence : -1.f;
  lg->width_min_kp = min_keypoints;
  return SSHIP_OK;
}
extern "C" int sship_lg_prune_counts(sship_lg* lg, int pair, int32_t* prune0, int n0, int32_t* prune1, int n1) {
  bind_thread();
  if (!lg || pair < 0 || n0 < 0 || n1 < 0 || (n0 > 0 && !prune0) || (n1 > 0 && !prune1))
    return fail(SSHIP_ERR_INVALID, "lg_prune_counts: bad arguments");
  if (pair >= lg->last_pairs) return fail(SSHIP_ERR_INVALID, "lg_prune_counts: pair exceeds the pairs of the last call");
  if (n0 > lg->max_kp || n1 > lg->max_kp) return fail(SSHIP_ERR_INVALID, "lg_prune_counts: n exceeds max_keypoints");
  SSHIP_HIP_CHECK(hipDeviceSynchronize());
  if (!lg->last_width) {  // upstream reports n_layers for every keypoint when it does not prune
    for (int i = 0; i < n0; ++i) prune0[i] = kLgLayers;
    for (int i = 0; i < n1; ++i) prune1[i] = kLgLayers;
    return SSHIP_OK;
  }
  const size_t P = lg->max_pairs, NP = lg->NP;
  const int* pr = lg->wid.as<int>() + 4 * P + 2 * P * NP;
  if (n0 > 0) SSHIP_HIP_CHECK(hipMemcpy(prune0, pr + (size_t)(2 * pair) * NP, (size_t)n0 * 4, hipMemcpyDeviceToHost));
  if (n1 > 0) SSHIP_HIP_CHECK(hipMemcpy(prune1, pr + (size_t)(2 * pair + 1) * NP, (size_t)n1 * 4, hipMemcpyDeviceToHost));
  return SSHIP_OK;
}

// The matcher proper: `pairs` problems, everything on the device.  9 x (SelfBlock x2 images, CrossBlock), then
// log_assignment[8] + filter_matches.
static int lg_forward(sship_lg* lg, const float* kp, int kp_stride, int kp_seq_stride, const int* lens,
                      const _Float16* desc, size_t desc_seq_stride, int pairs, int32_t* m0, float* ms0, hipStream_t s) {
  const sship_lg_weights* w = lg->w;
  LgDims d{2 * pairs, lg->NP};
  const int T = d.S * d.NP;
  _Float16 *x = lg->x.as<_Float16>(), *q = lg->q.as<_Float16>(), *k = lg->k.as<_Float16>(), *vt = lg->vt.as<_Float16>();
  _Float16* ctx = lg->ctx.as<_Float16>();
  float* rope = lg->rope.as<float>();
  // prep also publishes the counts clamped to [0, max_kp] (a caller-supplied count above max_kp would otherwise read past
  // the descriptor / keypoint stride of its sequence): every kernel below reads the clamped copy.
  launch_lg_prep(kp, kp_stride, kp_seq_stride, lens, lg->max_kp, lg->lens_c.as<int>(), desc, desc_seq_stride, w->wr,
                 (float)lg->image_w, (float)lg->image_h, d, x, rope, lg->kpn.as<float>(), s);
  lens = lg->lens_c.as<int>();
  lg->last_pairs = pairs;
  // adaptive depth: layer i's token confidence after its CrossBlock, the running set for layers i + 1 ..; the exit head after the join
  const bool adaptive = lg->depth_conf > 0.f;
  // adaptive width: after the depth decision of layer i the running pairs drop their unmatchable tokens; layers i + 1 .. run on the rest
  const bool width = lg->width_conf > 0.f;
  const float keep_thr = 1.0f - lg->width_conf;
#if SSHIP_DEV_SWITCHES
  // the developer kernels that do not know the running set: refuse rather than ignore the setting
  if (adaptive && ((dev_env("SUPERSLAM_HIP_FFN") && atoi(dev_env("SUPERSLAM_HIP_FFN")) == 16) ||
                   (dev_env("SUPERSLAM_HIP_ATTN") && std::string(dev_env("SUPERSLAM_HIP_ATTN")) == "res")))
    return fail(SSHIP_ERR_INVALID, "lightglue: adaptive depth is not supported by the 16-wave FFN or the LDS-resident-key attention");
  if (width && ((dev_env("SUPERSLAM_HIP_FFN") && atoi(dev_env("SUPERSLAM_HIP_FFN")) == 16) ||
                (dev_env("SUPERSLAM_HIP_ATTN") && std::string(dev_env("SUPERSLAM_HIP_ATTN")) == "res")))
    return fail(SSHIP_ERR_INVALID, "lightglue: adaptive width is not supported by the 16-wave FFN or the LDS-resident-key attention");
#endif
  if (lg->cap_n) {  // test-only stage capture (sship_lg_debug_capture)
    lg->captured = true;
    lg->cap_last_pairs = pairs;
    lg->cap_last_adaptive = adaptive || width;
    lg->cap_last_width = width;
    lg->cap_last_assigned = false;
  }
  lg->last_adaptive = adaptive || width;  // layers_run comes from the device in both modes
  lg->last_width = width;
  lg->last_layers = lg->debug_layers;
  // 3 launches per block: [projection fused into the previous FFN's tail] -> attention -> FFN(+ next projection).
  static const bool igemm_qkv0 = dev_env("SUPERSLAM_HIP_LG_QKV0") && std::string(dev_env("SUPERSLAM_HIP_LG_QKV0")) == "igemm";  // A/B
  const int n_layers = lg->debug_layers;  // kLgLayers except under sship_lg_debug_set_layers (test-only)
  // the layer stack of pairs [p0, p0 + np) on stream st: every buffer is sequence-major, pairs are independent
  auto layers = [&](int p0, int np, hipStream_t st, bool shared_gpu, int part) -> int {
    const LgDims ds{2 * np, lg->NP};
    const LgDepth dep = lg_depth_state(lg, p0, part);
    const LgWidth wd = lg_width_state(lg, p0, part);
    const size_t tok = (size_t)2 * p0 * lg->NP;
    _Float16 *xs = x + tok * 256, *qs = q + tok * 256, *ks = k + tok * 256, *vs = vt + tok * 256, *cs = ctx + tok * 256;
    float* rs = rope + tok * 64;
    const int* ls = lens + 2 * p0;
    if (adaptive || width) launch_lg_depth_init(ls, np, dep, st);
    if (width) launch_lg_width_init(ls, lg->NP, np, wd, st);
    // test-only stage capture: the slices of the listed pairs of this launch group, copied on this group's stream right after the launch
    // that produced them (`buf` is the whole-call buffer; a pair's slice is contiguous)
    const size_t pair_halfs = (size_t)2 * lg->NP * 256;
    // (short names: SSHIP_HIP_CHECK spells its expression into the error text, and the shipped library holds no SSHIP_* name but the documented ones)
    constexpr int kCap_X_IN = SSHIP_LG_STAGE_X_IN, kCap_Q_S = SSHIP_LG_STAGE_Q_S, kCap_K_S = SSHIP_LG_STAGE_K_S, kCap_V_S = SSHIP_LG_STAGE_V_S,
                  kCap_CTX_S = SSHIP_LG_STAGE_CTX_S, kCap_X_MID = SSHIP_LG_STAGE_X_MID, kCap_QK_C = SSHIP_LG_STAGE_QK_C,
                  kCap_V_C = SSHIP_LG_STAGE_V_C, kCap_CTX_C = SSHIP_LG_STAGE_CTX_C, kCap_X_OUT = SSHIP_LG_STAGE_X_OUT, kCap_MD = SSHIP_LG_STAGE_MD;
    auto cap = [&](int layer, int stage, const _Float16* buf) -> hipError_t {
      for (int c = 0; c < lg->cap_n; ++c) {
        const int p = lg->cap_pairs[c];
        if (p < p0 || p >= p0 + np) continue;
        _Float16* dst = stage == SSHIP_LG_STAGE_MD
                            ? lg->cap_md.as<_Float16>() + (size_t)c * pair_halfs
                            : lg->cap.as<_Float16>() + (((size_t)c * kLgLayers + layer) * sship_lg::kCapStages + stage) * pair_halfs;
        if (hipError_t e = hipMemcpyAsync(dst, buf + (size_t)p * pair_halfs, pair_halfs * 2, hipMemcpyDeviceToDevice, st)) return e;
      }
      return hipSuccess;
    };
    // the same for the state of the adaptive modes (4-byte words; `src` is offset to this launch group, `per_pair` words per pair)
    const LgCapAd& lay = lg->cap_lay;
    auto cap_words = [&](size_t dst_word, const void* src, size_t per_pair) -> hipError_t {
      for (int c = 0; c < lg->cap_n; ++c) {
        const int p = lg->cap_pairs[c];
        if (p < p0 || p >= p0 + np) continue;
        if (hipError_t e = hipMemcpyAsync(lg->cap_ad.as<int>() + (size_t)c * lay.words + dst_word,
                                          static_cast<const int*>(src) + (size_t)(p - p0) * per_pair, per_pair * 4, hipMemcpyDeviceToDevice, st))
          return e;
      }
      return hipSuccess;
    };
    const int tile_tokens = lg_ffn_tile_tokens(ds.S * ds.NP);
    // what each FFN launch streams (w0, w3, the fused projection): handed to the launch BEFORE it as a prefetch hint (latency mode)
    auto self_w = [&](int i, const ConvW** o) { o[0] = &w->ffn0_s[i]; o[1] = &w->ffn3_s[i]; o[2] = &w->cqkv_t[i]; };
    auto cross_w = [&](int i, const ConvW** o) { o[0] = &w->ffn0_c[i]; o[1] = &w->ffn3_c[i]; o[2] = i + 1 < kLgLayers ? &w->qkv_t[i + 1] : &w->final_t; };
    const ConvW* pf[3];
    self_w(0, pf);
#if SSHIP_DEV_SWITCHES
    if (igemm_qkv0) SSHIP_HIP_CHECK(lg_linear_heads(w->qkv[0], xs, ds, /*rope_segs=*/2, /*t_seg=*/2, rs, qs, ks, vs, st));
    else
#endif
    SSHIP_HIP_CHECK(launch_lg_proj_heads(w->qkv_t[0], xs, ds, /*rope_segs=*/2, /*t_seg=*/2, rs, qs, ks, vs, st, pf));
    for (int i = 0; i < n_layers; ++i) {
      // adaptive depth, layers >= 1: the attention launches see the counts of running pairs only (0 for stopped ones: their
      // workgroups return at once), the FFN launches walk the tiles of running pairs only.  Layer 0 runs as without it.
      // adaptive width, layers >= 1: lens_live holds the LIVE counts of running pairs, and the FFN launches walk the list of live tiles
      const int* la = (adaptive || width) && i > 0 ? dep.lens_live : ls;
      const int* live = i > 0 ? (width ? wd.tiles : adaptive ? dep.live : nullptr) : nullptr;
      const int lm = width ? 2 : 1;
      if (lg->cap_n) {  // what the previous launch (the first projection, or layer i - 1's CrossBlock FFN) left for this layer
        SSHIP_HIP_CHECK(cap(i, kCap_X_IN, x));
        SSHIP_HIP_CHECK(cap(i, kCap_Q_S, q));
        SSHIP_HIP_CHECK(cap(i, kCap_K_S, k));
        SSHIP_HIP_CHECK(cap(i, kCap_V_S, vt));
        if (adaptive || width) {  // the counts and the rope table this layer's launches read
          SSHIP_HIP_CHECK(cap_words(lay.lens + (size_t)i * 2, la, 2));
          SSHIP_HIP_CHECK(cap_words(lay.rope + (size_t)i * 2 * lg->NP * 64, rs, (size_t)2 * lg->NP * 64));
        }
      }
      // SelfBlock (both images of every pair in one launch); its FFN also emits CrossBlock's [to_qk | to_v]
      launch_lg_attention(qs, ks, vs, la, ds, false, cs, st, shared_gpu);
      if (lg->cap_n) SSHIP_HIP_CHECK(cap(i, kCap_CTX_S, ctx));
      cross_w(i, pf);
      launch_lg_ffn(w->ffn0_s[i], w->ffn3_s[i], w->ln_g_s[i], w->ln_b_s[i], cs, xs, ds, &w->cqkv_t[i], true, /*rope_segs=*/0,
                    /*t_seg=*/1, rs, qs, ks, vs, nullptr, nullptr, 0.f, nullptr, st, pf, live, lm);
      if (lg->cap_n) {
        SSHIP_HIP_CHECK(cap(i, kCap_X_MID, x));
        SSHIP_HIP_CHECK(cap(i, kCap_QK_C, q));
        SSHIP_HIP_CHECK(cap(i, kCap_V_C, vt));
      }
      // CrossBlock (qk shared by both directions; sequence s attends to s^1); its FFN emits the next layer's Wqkv,
      // or final_proj + matchability after the last layer
      launch_lg_attention(qs, qs, vs, la, ds, true, cs, st, shared_gpu);
      if (lg->cap_n) SSHIP_HIP_CHECK(cap(i, kCap_CTX_C, ctx));
      if (i + 1 < kLgLayers) {
        self_w(i + 1, pf);
        launch_lg_ffn(w->ffn0_c[i], w->ffn3_c[i], w->ln_g_c[i], w->ln_b_c[i], cs, xs, ds, &w->qkv_t[i + 1], true, 2, 2, rs, qs, ks,
                      vs, nullptr, nullptr, 0.f, nullptr, st, pf, live, lm);
        if (lg->cap_n) SSHIP_HIP_CHECK(cap(i, kCap_X_OUT, x));  // before a pruning step compacts the rows
        if (adaptive)  // token confidence of layer i and the stop rule (reads x after layer i; with width on, of the live tokens)
          launch_lg_depth_conf(xs, width ? wd.wlen : ls, lg->NP, np, w->tc_w + i * 256, w->tc_b[i], lg_depth_threshold(i), lg->depth_conf, i, dep, st);
        if (width) {
          // the pruning step of layer i for the pairs still running, then the counts / tile lists of layer i + 1.  The FFN above
          // projected layer i + 1's Q / K / V from the rows as they were: the sequences that lost tokens are projected again.
          launch_lg_width_prune(xs, rs, lg->NP, np, w->head_mw + i * 256, w->head_mb + i, keep_thr, lg->width_min_kp,
                                adaptive ? w->tc_w + i * 256 : nullptr, w->tc_b[i], lg_depth_threshold(i), dep, wd, st);
          launch_lg_width_publish(lg->NP, np, tile_tokens, i, dep, wd, st);
          if (i + 1 < n_layers)
            SSHIP_HIP_CHECK(launch_lg_proj_heads(w->qkv_t[i + 1], xs, ds, 2, 2, rs, qs, ks, vs, st, nullptr, wd.rtiles));
          if (lg->cap_n) {  // the width state after the pruning step of layer i
            SSHIP_HIP_CHECK(cap_words(lay.ind + (size_t)i * 2 * lg->NP, wd.ind, (size_t)2 * lg->NP));
            SSHIP_HIP_CHECK(cap_words(lay.prune + (size_t)i * 2 * lg->NP, wd.prune, (size_t)2 * lg->NP));
            SSHIP_HIP_CHECK(cap_words(lay.wlen + (size_t)i * 2, wd.wlen, 2));
            SSHIP_HIP_CHECK(cap_words(lay.chg + (size_t)i * 2, wd.chg, 2));
          }
        }
      } else
        launch_lg_ffn(w->ffn0_c[i], w->ffn3_c[i], w->ln_g_c[i], w->ln_b_c[i], cs, xs, ds, &w->final_t, false, 0, 0, rs, qs, ks, vs,
                      lg->md.as<_Float16>() + tok * 256, w->match_w, w->match_b, lg->logsig.as<float>() + tok, st, nullptr, live, lm);
      if (lg->cap_n) {
        if (i + 1 == kLgLayers) {
          SSHIP_HIP_CHECK(cap(i, kCap_X_OUT, x));
          SSHIP_HIP_CHECK(cap(i, kCap_MD, lg->md.as<_Float16>()));
          for (int c = 0; c < lg->cap_n; ++c) {
            const int p = lg->cap_pairs[c];
            if (p < p0 || p >= p0 + np) continue;
            SSHIP_HIP_CHECK(hipMemcpyAsync(lg->cap_ls.as<float>() + (size_t)c * 2 * lg->NP, lg->logsig.as<float>() + (size_t)p * 2 * lg->NP,
                                           (size_t)2 * lg->NP * 4, hipMemcpyDeviceToDevice, st));
          }
        }
      }
    }
    if (lg->cap_n && (adaptive || width)) {  // test-only capture: the counters and the verdicts of the stop rule, as the layer stack left them
      SSHIP_HIP_CHECK(cap_words(lay.cnt, dep.cnt, 8));
      SSHIP_HIP_CHECK(cap_words(lay.lr, dep.layers_run, 1));
    }
    SSHIP_HIP_CHECK(hipGetLastError());
    return SSHIP_OK;
  };
  // Throughput batches: two half-batches on two streams.  Every LightGlue launch is a whole number of workgroup "rounds" over
  // the 512 workgroup slots plus a partly filled last one (FFN: 1216 tiles = 2.4 rounds at 64 pairs - a third of the launch
  // runs at 37 % occupancy); a second, independent stream of the same kernels fills those tails, and an attention workgroup
  // (70 KB LDS, transcendental-bound) can share a CU with an FFN workgroup (79 KB, matrix-bound) of the other half.
  // Only when each half still qualifies for the throughput kernels; SUPERSLAM_HIP_LG_SPLIT=1 turns it off (A/B runs).
  static const int split_env = dev_env("SUPERSLAM_HIP_LG_SPLIT") ? atoi(dev_env("SUPERSLAM_HIP_LG_SPLIT")) : 0;
  int parts = 1;
  if (split_env >= 1 && split_env <= 1 + sship_lg::kAux) parts = std::min(split_env, pairs);  // forced (1 = off)
  else if ((size_t)2 * (pairs / 2) * lg->NP / 64 >= (size_t)2 * cu_count()) parts = 2;
  if (parts > 1) {
    SSHIP_HIP_CHECK(hipEventRecord(lg->ev_fork, s));
    // Once an auxiliary stream has been forked, every exit - including an error part-way - joins it back into `s` first:
    // work already queued on the (non-blocking) auxiliary streams would otherwise be unordered with the caller's stream and
    // the next call's k_lg_prep could overwrite x / rope / lens_c while an auxiliary stream still reads them.
    int forked = 0, rc = SSHIP_OK;
    hipError_t he = hipSuccess;
    int p0 = pairs / parts;  // part 0 (on s) is launched last: the auxiliary streams are already busy by then
    for (int i = 1; i < parts && rc == SSHIP_OK && he == hipSuccess; ++i) {
      const int np = i + 1 < parts ? pairs / parts : pairs - p0;
      if ((he = hipStreamWaitEvent(lg->aux[i - 1], lg->ev_fork, 0)) != hipSuccess) break;
      forked = i;
      rc = layers(p0, np, lg->aux[i - 1], true, i);
      p0 += np;
    }
    if (rc == SSHIP_OK && he == hipSuccess) rc = layers(0, pairs / parts, s, true, 0);
    for (int i = 1; i <= forked; ++i) {  // join (also on the error path; best effort there)
      hipError_t e1 = hipEventRecord(lg->ev_join[i - 1], lg->aux[i - 1]);
      if (e1 == hipSuccess) e1 = hipStreamWaitEvent(s, lg->ev_join[i - 1], 0);
      if (e1 != hipSuccess) { (void)hipStreamSynchronize(lg->aux[i - 1]); if (he == hipSuccess) he = e1; }
    }
    if (rc != SSHIP_OK) return rc;
    SSHIP_HIP_CHECK(he);
  } else {
    if (int rc = layers(0, pairs, s, false, 0)) return rc;
  }
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("fe_lg_stereo_match:layers_x9", s);
  if (n_layers < kLgLayers) {  // truncated debug run: x after layer n_layers is the product; no assignment
    lg->debug_layers = kLgLayers;  // one-shot: a caller that forgets to reset it must not keep a matcher that matches nothing
    log_msg(3, "sship: LightGlue ran truncated to %d layer(s) (sship_lg_debug_set_layers, test-only); matches0 = -1", n_layers);
    SSHIP_HIP_CHECK(hipMemsetAsync(m0, 0xff, (size_t)pairs * lg->max_kp * 4, s));
    SSHIP_HIP_CHECK(hipMemsetAsync(ms0, 0, (size_t)pairs * lg->max_kp * 4, s));
    return SSHIP_OK;
  }
  if (adaptive)  // md / logsig of the pairs that stopped early, from the assignment head of the layer they stopped after
    launch_lg_exit_head(x, lg->NP, pairs, lg->dep.as<int>() + (size_t)lg->max_pairs * 8, w->head_wt, w->head_b, w->head_mw, w->head_mb,
                        lg->md.as<_Float16>(), lg->logsig.as<float>(), s);
  if (lg->cap_n && (adaptive || width)) {  // test-only capture: md / logsig as the assignment reads them (after the exit head)
    const size_t pair_halfs = (size_t)2 * lg->NP * 256;
    for (int c = 0; c < lg->cap_n; ++c) {
      const int p = lg->cap_pairs[c];
      if (p >= pairs) continue;
      SSHIP_HIP_CHECK(hipMemcpyAsync(lg->cap_amd.as<_Float16>() + (size_t)c * pair_halfs, lg->md.as<_Float16>() + (size_t)p * pair_halfs,
                                     pair_halfs * 2, hipMemcpyDeviceToDevice, s));
      SSHIP_HIP_CHECK(hipMemcpyAsync(lg->cap_als.as<float>() + (size_t)c * 2 * lg->NP, lg->logsig.as<float>() + (size_t)p * 2 * lg->NP,
                                     (size_t)2 * lg->NP * 4, hipMemcpyDeviceToDevice, s));
    }
    lg->cap_last_assigned = true;
  }
  if (width) {
    // the assignment of the live sets (row a = the a-th surviving keypoint), then back to keypoint indices through ind
    const int* wlen = lg->wid.as<int>();
    launch_lg_assign(lg->md.as<_Float16>(), lg->logsig.as<float>(), wlen, d, lg->ws.as<float>(), lg->sim.as<float>(), lg->max_kp,
                     lg->m0c.as<int32_t>(), lg->ms0c.as<float>(), 0.1f /* filter_threshold */, 0, s);
    SSHIP_HIP_CHECK(hipMemsetAsync(m0, 0xff, (size_t)pairs * lg->max_kp * 4, s));
    SSHIP_HIP_CHECK(hipMemsetAsync(ms0, 0, (size_t)pairs * lg->max_kp * 4, s));
    if (lg->cap_n) {  // test-only capture: the matches of the live sets, as the scatter reads them
      const LgCapAd& lay = lg->cap_lay;
      for (int c = 0; c < lg->cap_n; ++c) {
        const int p = lg->cap_pairs[c];
        if (p >= pairs) continue;
        int* dst = lg->cap_ad.as<int>() + (size_t)c * lay.words;
        SSHIP_HIP_CHECK(hipMemcpyAsync(dst + lay.mc, lg->m0c.as<int32_t>() + (size_t)p * lg->max_kp, (size_t)lg->max_kp * 4, hipMemcpyDeviceToDevice, s));
        SSHIP_HIP_CHECK(hipMemcpyAsync(dst + lay.msc, lg->ms0c.as<float>() + (size_t)p * lg->max_kp, (size_t)lg->max_kp * 4, hipMemcpyDeviceToDevice, s));
      }
    }
    launch_lg_width_scatter(wlen, wlen + 4 * (size_t)lg->max_pairs, lg->NP, pairs, lg->max_kp, lg->m0c.as<int32_t>(), lg->ms0c.as<float>(), m0, ms0, s);
    SSHIP_HIP_CHECK(hipGetLastError());
    g_timer.mark("fe_lg_stereo_match:assign_filter", s);
    return SSHIP_OK;
  }
  // log-assignment + mutual filter straight from md (lg_kernels.hip: k_assign_stream); lg->sim is the partials' scratch
  launch_lg_assign(lg->md.as<_Float16>(), lg->logsig.as<float>(), lens, d, lg->ws.as<float>(), lg->sim.as<float>(), lg->max_kp, m0, ms0,
                   0.1f /* filter_threshold */, 0, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("fe_lg_stereo_match:assign_filter", s);
  return SSHIP_OK;
}

extern "C" int sship_lg_match_batch_device(sship_lg* lg, const float* kp, const int* n, const void* desc, int pairs,
                                           int32_t* m0, float* ms0, void* stream) {
  bind_thread();
  if (!lg || !kp || !n || !desc || !m0 || !ms0) return fail(SSHIP_ERR_INVALID, "lg_match_batch_device: null argument");
  if (pairs <= 0 || pairs > lg->max_pairs) return fail(SSHIP_ERR_INVALID, "lg_match_batch_device: pairs exceeds max_pairs");
  hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = legacy default stream: ordered after an extractor call made with NULL
  g_timer.begin_if_idle(s);
  return lg_forward(lg, kp, 3, lg->max_kp * 3, n, static_cast<const _Float16*>(desc), (size_t)lg->max_kp * 256, pairs,
                    m0, ms0, s);
}

// Measurement hook (include/sship.h): one stage of the matcher re-launched `iters` times over the state of the last call.
extern "C" int sship_lg_bench_stage(sship_lg* lg, int stage, int iters, float* avg_ms) {
  bind_thread();
  if (!lg || !avg_ms || iters <= 0 || stage < 0 || stage > 7) return fail(SSHIP_ERR_INVALID, "lg_bench_stage: bad arguments");
  if (lg->last_pairs <= 0) return fail(SSHIP_ERR_INVALID, "lg_bench_stage: run a match on this handle first");
  const sship_lg_weights* w = lg->w;
  const int pairs = lg->last_pairs;
  LgDims d{2 * pairs, lg->NP};
  hipStream_t s = lg->stream;
  _Float16 *x = lg->x.as<_Float16>(), *q = lg->q.as<_Float16>(), *k = lg->k.as<_Float16>(), *vt = lg->vt.as<_Float16>();
  _Float16* ctx = lg->ctx.as<_Float16>();
  float* rope = lg->rope.as<float>();
  const int* lens = lg->lens_c.as<int>();
  const bool call_splits = (size_t)2 * (pairs / 2) * lg->NP / 64 >= (size_t)2 * cu_count();  // lg_forward's two-stream condition
  auto run = [&]() -> hipError_t {
    switch (stage) {
      case 0: return launch_lg_proj_heads(w->qkv_t[0], x, d, 2, 2, rope, q, k, vt, s);
      // the attention kernel the CALL launches: lg_forward runs a throughput batch as two half-batches on two streams and tells the launcher
      // so (shared_gpu: no key split, wave-granular query units).  Rounds 2-5 timed the key-split variant here - a kernel the call never runs.
      case 1: launch_lg_attention(q, k, vt, lens, d, false, ctx, s, call_splits); return hipGetLastError();
      case 2: launch_lg_attention(q, q, vt, lens, d, true, ctx, s, call_splits); return hipGetLastError();
      case 3: launch_lg_ffn(w->ffn0_s[0], w->ffn3_s[0], w->ln_g_s[0], w->ln_b_s[0], ctx, x, d, &w->cqkv_t[0], true, 0, 1, rope, q, k, vt,
                            nullptr, nullptr, 0.f, nullptr, s); return hipGetLastError();
      case 4: launch_lg_ffn(w->ffn0_c[0], w->ffn3_c[0], w->ln_g_c[0], w->ln_b_c[0], ctx, x, d, &w->qkv_t[1], true, 2, 2, rope, q, k, vt,
                            nullptr, nullptr, 0.f, nullptr, s); return hipGetLastError();
      case 5: launch_lg_ffn(w->ffn0_c[8], w->ffn3_c[8], w->ln_g_c[8], w->ln_b_c[8], ctx, x, d, &w->final_t, false, 0, 0, rope, q, k, vt,
                            lg->md.as<_Float16>(), w->match_w, w->match_b, lg->logsig.as<float>(), s); return hipGetLastError();
      case 6: launch_lg_assign(lg->md.as<_Float16>(), lg->logsig.as<float>(), lens, d, lg->ws.as<float>(), lg->sim.as<float>(), lg->max_kp,
                               lg->m0.as<int32_t>(), lg->ms0.as<float>(), 0.1f, 1, s); return hipGetLastError();  // log-sum-exp pass
      default: launch_lg_assign(lg->md.as<_Float16>(), lg->logsig.as<float>(), lens, d, lg->ws.as<float>(), lg->sim.as<float>(), lg->max_kp,
                                lg->m0.as<int32_t>(), lg->ms0.as<float>(), 0.1f, 2, s); return hipGetLastError();  // arg-max pass
    }
  };
  // stages 3 / 4 update the residual stream in place: keep a copy and put it back (the values do not affect the timing, but
  // the handle's state should be what the last match left)
  DevBuf keep;
  const size_t xbytes = (size_t)d.S * d.NP * 512;
  SSHIP_HIP_CHECK(keep.ensure(xbytes));
  SSHIP_HIP_CHECK(hipMemcpyAsync(keep.p, x, xbytes, hipMemcpyDeviceToDevice, s));
  if (int rc = bench_loop(s, iters, run, avg_ms)) return rc;
  SSHIP_HIP_CHECK(hipMemcpyAsync(x, keep.p, xbytes, hipMemcpyDeviceToDevice, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  return SSHIP_OK;
}

static int lg_match_common(sship_lg* lg, const float* kp0, int st0, int n0, const float* kp1, int st1, int n1,
                           int32_t* matches0, float* mscores0) {
  // kpts -> pinned [2, max_kp, 3] (x, y, 0) -> device; descriptors already staged in desc_stage.
  hipStream_t s = lg->stream;
  g_timer.begin_if_idle(s);
  float* hk = lg->h_kp.as<float>();
  const int mk = lg->max_kp;
  for (int i = 0; i < n0; ++i) { hk[3 * i] = kp0[(size_t)i * st0]; hk[3 * i + 1] = kp0[(size_t)i * st0 + 1]; hk[3 * i + 2] = 0.f; }
  for (int i = 0; i < n1; ++i) {
    hk[(size_t)mk * 3 + 3 * i] = kp1[(size_t)i * st1]; hk[(size_t)mk * 3 + 3 * i + 1] = kp1[(size_t)i * st1 + 1];
    hk[(size_t)mk * 3 + 3 * i + 2] = 0.f;
  }
  lg->h_lens.as<int>()[0] = n0; lg->h_lens.as<int>()[1] = n1;
  SSHIP_HIP_CHECK(hipMemcpyAsync(lg->kp_stage.p, hk, 2 * (size_t)mk * 12, hipMemcpyHostToDevice, s));
  SSHIP_HIP_CHECK(hipMemcpyAsync(lg->lens.p, lg->h_lens.p, 8, hipMemcpyHostToDevice, s));
  if (int rc = lg_forward(lg, lg->kp_stage.as<float>(), 3, mk * 3, lg->lens.as<int>(), lg->desc_stage.as<_Float16>(),
                          (size_t)mk * 256, 1, lg->m0.as<int32_t>(), lg->ms0.as<float>(), s))
    return rc;
  SSHIP_HIP_CHECK(hipMemcpyAsync(lg->h_m0.p, lg->m0.p, (size_t)n0 * 4, hipMemcpyDeviceToHost, s));
  SSHIP_HIP_CHECK(hipMemcpyAsync(lg->h_ms0.p, lg->ms0.p, (size_t)n0 * 4, hipMemcpyDeviceToHost, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  memcpy(matches0, lg->h_m0.p, (size_t)n0 * 4);
  memcpy(mscores0, lg->h_ms0.p, (size_t)n0 * 4);
  return SSHIP_OK;
}

extern "C" int sship_lg_match_device(sship_lg* lg, const float* kp0, int st0, int n0, const void* desc0, const float* kp1,
                                     int st1, int n1, const void* desc1, int32_t* matches0, float* mscores0) {
  bind_thread();
  if (!lg || !kp0 || !kp1 || !desc0 || !desc1 || !matches0 || !mscores0) return fail(SSHIP_ERR_INVALID, "lg_match_device: null argument");
  if (n0 <= 0 || n1 <= 0) return fail(SSHIP_ERR_INVALID, "lg_match_device: empty keypoint set");  // LightGlue.cc:381-385
  if (n0 > lg->max_kp || n1 > lg->max_kp || st0 < 2 || st1 < 2) return fail(SSHIP_ERR_INVALID, "lg_match_device: n exceeds max_keypoints");
  hipStream_t s = lg->stream;
  // D2D of exactly the slot bytes into the matcher's inputs (LightGlue.cc:425-441)
  SSHIP_HIP_CHECK(hipMemcpyAsync(lg->desc_stage.p, desc0, (size_t)n0 * 512, hipMemcpyDeviceToDevice, s));
  SSHIP_HIP_CHECK(hipMemcpyAsync(lg->desc_stage.as<_Float16>() + (size_t)lg->max_kp * 256, desc1, (size_t)n1 * 512,
                                 hipMemcpyDeviceToDevice, s));
  return lg_match_common(lg, kp0, st0, n0, kp1, st1, n1, matches0, mscores0);
}
extern "C" int sship_lg_match_host(sship_lg* lg, const float* kp0, int st0, int n0, const float* desc0, const float* kp1,
                                   int st1, int n1, const float* desc1, int32_t* matches0, float* mscores0) {
  bind_thread();
  if (!lg || !kp0 || !kp1 || !desc0 || !desc1 || !matches0 || !mscores0) return fail(SSHIP_ERR_INVALID, "lg_match_host: null argument");
  if (n0 <= 0 || n1 <= 0) return fail(SSHIP_ERR_INVALID, "lg_match_host: empty keypoint set");  // LightGlue.cc:294-295
  if (n0 > lg->max_kp || n1 > lg->max_kp || st0 < 2 || st1 < 2) return fail(SSHIP_ERR_INVALID, "lg_match_host: n exceeds max_keypoints");
  hipStream_t s = lg->stream;
  _Float16* hd = lg->h_desc.as<_Float16>();  // store_floats: CV_32F -> engine dtype on the host (LightGlue.cc:227-238)
  for (size_t i = 0; i < (size_t)n0 * 256; ++i) hd[i] = (_Float16)desc0[i];
  for (size_t i = 0; i < (size_t)n1 * 256; ++i) hd[(size_t)lg->max_kp * 256 + i] = (_Float16)desc1[i];
  SSHIP_HIP_CHECK(hipMemcpyAsync(lg->desc_stage.p, hd, (size_t)n0 * 512, hipMemcpyHostToDevice, s));
  SSHIP_HIP_CHECK(hipMemcpyAsync(lg->desc_stage.as<_Float16>() + (size_t)lg->max_kp * 256, hd + (size_t)lg->max_kp * 256,
                                 (size_t)n1 * 512, hipMemcpyHostToDevice, s));
  return lg_match_common(lg, kp0, st0, n0, kp1, st1, n1, matches0, mscores0);
}
extern "C" int sship_filter_matches(const int32_t* matches0, const float* mscores0, int n0, int* q, int* t, float* dist) {
  if (n0 <= 0) return 0;
  if (!matches0 || !q || !t || !dist) return -1;
  int k = 0;
  for (int i = 0; i < n0; ++i) {  // LightGlue.cc:351-361
    const int j = matches0[i];
    if (j < 0) continue;
    q[k] = i; t[k] = j; dist[k] = 1.0f - (mscores0 ? mscores0[i] : 1.0f);
    ++k;
  }
  return k;
}

// ====================================================================================================
// Mutual nearest-neighbour matcher (include/sship.h "Nearest-neighbour matcher"; csrc/nn_kernels.hip)
// ====================================================================================================
struct sship_nn {
  int max_kp = 0, max_pairs = 0;
  float ratio = 0.f, dist = 0.f;
  int mutual = 1;
  // the keypoint-window gate (include/sship.h "Keypoint-window gate"): off by default; (dx_lo, dx_hi, dy_lo, dy_hi)
  int gate_on = 0;
  float gate[4] = {-INFINITY, INFINITY, -INFINITY, INFINITY};
  hipStream_t stream = nullptr;
  DevBuf ws;
  StageArena one;   // the single-pair entries: one staged pair and its results (nn_stage)
  // the last call's launch arguments (sship_nn_bench re-runs them; the caller keeps a batch call's buffers alive until then)
  struct Last { const int* n = nullptr; const _Float16* desc = nullptr; const float* kp = nullptr;  // kp non-null: the last call was gated
                int items = 0; int32_t* m0 = nullptr; float* ms0 = nullptr; } last;
};
extern "C" int sship_nn_create(int max_kp, int max_pairs, sship_nn** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "nn_create: null argument");
  if (max_kp <= 0 || max_kp > kMaxKp) return fail(SSHIP_ERR_INVALID, "nn_create: max_keypoints must be in [1, 4096]");
  if (max_pairs <= 0) max_pairs = 1;  // as sship_lg_create
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_nn, void (*)(sship_nn*)> nn(new sship_nn(), sship_nn_destroy);
  nn->max_kp = max_kp; nn->max_pairs = max_pairs;
  SSHIP_HIP_CHECK(nn->ws.ensure(nn_workspace_floats(max_kp, max_pairs) * 4));
  const NnStage st = nn_stage(max_kp);
  SSHIP_HIP_CHECK(nn->one.create(st.in_bytes, st.out_bytes));
  SSHIP_HIP_CHECK(hipMemset(nn->one.dev<char>(st.desc), 0, st.in_bytes - st.desc));   // the descriptor and keypoint slots: rows never staged are zero
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&nn->stream, hipStreamDefault));
  *out = nn.release();
  return SSHIP_OK;
}
extern "C" void sship_nn_destroy(sship_nn* nn) { destroy_handle(nn); }
extern "C" int sship_nn_set_params(sship_nn* nn, float ratio_threshold, float distance_threshold, int mutual_check) {
  if (!nn) return fail(SSHIP_ERR_INVALID, "nn_set_params: null handle");
  if (std::isnan(ratio_threshold) || ratio_threshold > 1.f) return fail(SSHIP_ERR_INVALID, "nn_set_params: ratio_threshold must be <= 1");
  if (std::isnan(distance_threshold)) return fail(SSHIP_ERR_INVALID, "nn_set_params: distance_threshold is NaN");
  nn->ratio = ratio_threshold; nn->dist = distance_threshold; nn->mutual = mutual_check ? 1 : 0;
  return SSHIP_OK;
}
extern "C" int sship_nn_get_params(const sship_nn* nn, float* ratio_threshold, float* distance_threshold, int* mutual_check) {
  if (!nn) return fail(SSHIP_ERR_INVALID, "nn_get_params: null handle");
  if (ratio_threshold) *ratio_threshold = nn->ratio;
  if (distance_threshold) *distance_threshold = nn->dist;
  if (mutual_check) *mutual_check = nn->mutual;
  return SSHIP_OK;
}
extern "C" int sship_nn_set_gate(sship_nn* nn, int enabled, float dx_lo, float dx_hi, float dy_lo, float dy_hi) {
  if (!nn) return fail(SSHIP_ERR_INVALID, "nn_set_gate: null handle");
  if (std::isnan(dx_lo) || std::isnan(dx_hi) || std::isnan(dy_lo) || std::isnan(dy_hi)) return fail(SSHIP_ERR_INVALID, "nn_set_gate: a bound is NaN");
  if (dx_lo > dx_hi || dy_lo > dy_hi) return fail(SSHIP_ERR_INVALID, "nn_set_gate: lo > hi");
  nn->gate_on = enabled ? 1 : 0;
  nn->gate[0] = dx_lo; nn->gate[1] = dx_hi; nn->gate[2] = dy_lo; nn->gate[3] = dy_hi;
  return SSHIP_OK;
}
extern "C" int sship_nn_get_gate(const sship_nn* nn, int* enabled, float* dx_lo, float* dx_hi, float* dy_lo, float* dy_hi) {
  if (!nn) return fail(SSHIP_ERR_INVALID, "nn_get_gate: null handle");
  if (enabled) *enabled = nn->gate_on;
  if (dx_lo) *dx_lo = nn->gate[0];
  if (dx_hi) *dx_hi = nn->gate[1];
  if (dy_lo) *dy_lo = nn->gate[2];
  if (dy_hi) *dy_hi = nn->gate[3];
  return SSHIP_OK;
}
// kp == nullptr: the plain launches (a handle without a gate); otherwise the gated ones with the handle's window
static hipError_t nn_run(const sship_nn* nn, const sship_nn::Last& l, hipStream_t s) {
  if (l.kp) launch_nn_match_gated(l.desc, l.kp, l.n, nn->max_kp, l.items, nn->ws.as<float>(), nn->ratio, nn->dist, nn->mutual, nn->gate, l.m0, l.ms0, s);
  else launch_nn_match(l.desc, l.n, nn->max_kp, l.items, nn->ws.as<float>(), nn->ratio, nn->dist, nn->mutual, l.m0, l.ms0, s);
  return hipGetLastError();
}
static int nn_launch(sship_nn* nn, const int* n, const _Float16* desc, const float* kp, int pairs, int32_t* m0, float* ms0, hipStream_t s) {
  nn->last = {n, desc, kp, pairs, m0, ms0};
  SSHIP_HIP_CHECK(nn_run(nn, nn->last, s));
  return SSHIP_OK;
}
static const char kNnGatedMsg[] = ": the handle's gate is enabled - use the _gated entry point (keypoints are needed)";
extern "C" int sship_nn_match_batch_device(sship_nn* nn, const int* n, const void* desc, int pairs, int32_t* m0, float* ms0, void* stream) {
  if (!nn || !n || !desc || !m0 || !ms0) return fail(SSHIP_ERR_INVALID, "nn_match_batch_device: null argument");
  if (pairs <= 0 || pairs > nn->max_pairs) return fail(SSHIP_ERR_INVALID, "nn_match_batch_device: pairs exceeds max_pairs");
  if (nn->gate_on) return fail(SSHIP_ERR_INVALID, std::string("nn_match_batch_device") + kNnGatedMsg);
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = legacy default stream: ordered after an extractor call made with NULL
  g_timer.begin_if_idle(s);
  if (int rc = nn_launch(nn, n, static_cast<const _Float16*>(desc), nullptr, pairs, m0, ms0, s)) return rc;
  g_timer.mark("nn_match:stream_final", s);
  return SSHIP_OK;
}
extern "C" int sship_nn_match_gated_batch_device(sship_nn* nn, const int* n, const void* desc, const float* kp, int pairs, int32_t* m0,
                                                 float* ms0, void* stream) {
  if (!nn || !n || !desc || !m0 || !ms0) return fail(SSHIP_ERR_INVALID, "nn_match_gated_batch_device: null argument");
  if (pairs <= 0 || pairs > nn->max_pairs) return fail(SSHIP_ERR_INVALID, "nn_match_gated_batch_device: pairs exceeds max_pairs");
  if (nn->gate_on && !kp) return fail(SSHIP_ERR_INVALID, "nn_match_gated_batch_device: the gate is enabled and kp_dev is NULL");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  if (int rc = nn_launch(nn, n, static_cast<const _Float16*>(desc), nn->gate_on ? kp : nullptr, pairs, m0, ms0, s)) return rc;
  g_timer.mark(nn->gate_on ? "nn_match_gated:stream_final" : "nn_match:stream_final", s);
  return SSHIP_OK;
}
extern "C" int sship_stereo_associate_batch_device(const float* kp, const int* n, const int32_t* matches0, int pairs, int max_keypoints,
                                                   float min_disparity, float max_row_diff, float* stereo, uint8_t* has_depth, void* stream) {
  if (!kp || !n || !matches0 || !stereo || !has_depth) return fail(SSHIP_ERR_INVALID, "stereo_associate_batch_device: null argument");
  if (pairs <= 0 || max_keypoints <= 0 || max_keypoints > kMaxKp)
    return fail(SSHIP_ERR_INVALID, "stereo_associate_batch_device: pairs must be positive and max_keypoints in [1, 4096]");
  bind_thread();
  if (int rc = require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_stereo_associate(kp, n, matches0, max_keypoints, pairs, min_disparity, max_row_diff, stereo, has_depth, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("stereo_associate", s);
  return SSHIP_OK;
}
// one pair out of the handle's arena (descriptors already enqueued into its desc slot on the handle's stream)
// gated (kp0 != nullptr): the host keypoints go into the kp slot as [2][max_kp][3] (x, y, 0) first
static int nn_match_common(sship_nn* nn, int n0, int n1, int32_t* matches0, float* mscores0, const float* kp0 = nullptr, int st0 = 0,
                           const float* kp1 = nullptr, int st1 = 0) {
  hipStream_t s = nn->stream;
  const StageArena& a = nn->one;
  const NnStage st = nn_stage(nn->max_kp);
  nn_pack_lens(a.host<char>(0), st, n0, n1);
  SSHIP_HIP_CHECK(a.upload(st.lens, 2 * sizeof(int), s));
  if (kp0) {
    nn_pack_kp(a.host<char>(0), st, kp0, st0, n0, kp1, st1, n1);
    SSHIP_HIP_CHECK(a.upload(st.kp, (size_t)n0 * 3 * sizeof(float), s));
    SSHIP_HIP_CHECK(a.upload(st.kp1, (size_t)n1 * 3 * sizeof(float), s));
  }
  if (int rc = nn_launch(nn, a.dev<int>(st.lens), a.dev<_Float16>(st.desc), kp0 ? a.dev<float>(st.kp) : nullptr, 1, a.dev<int32_t>(a.out + st.m0),
                         a.dev<float>(a.out + st.ms0), s))
    return rc;
  SSHIP_HIP_CHECK(a.download(a.out + st.m0, (size_t)n0 * sizeof(int32_t), s));
  SSHIP_HIP_CHECK(a.download(a.out + st.ms0, (size_t)n0 * sizeof(float), s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  nn_unpack(a.host<char>(a.out), st, n0, matches0, mscores0);
  return SSHIP_OK;
}
static int nn_check_pair(const sship_nn* nn, int n0, const void* d0, int n1, const void* d1, const void* m0, const void* ms0, const char* who) {
  if (!nn || !d0 || !d1 || !m0 || !ms0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (n0 <= 0 || n1 <= 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": empty descriptor set");
  if (n0 > nn->max_kp || n1 > nn->max_kp) return fail(SSHIP_ERR_INVALID, std::string(who) + ": n exceeds max_keypoints");
  return SSHIP_OK;
}
// the gated calls' keypoint arguments: needed (and checked) only while the gate is enabled
static int nn_check_kp(const sship_nn* nn, const float* kp0, int st0, const float* kp1, int st1, const char* who) {
  if (!nn->gate_on) return SSHIP_OK;
  if (!kp0 || !kp1) return fail(SSHIP_ERR_INVALID, std::string(who) + ": the gate is enabled and a keypoint pointer is NULL");
  if (st0 < 2 || st1 < 2) return fail(SSHIP_ERR_INVALID, std::string(who) + ": kp_stride must be >= 2");
  return SSHIP_OK;
}
static int nn_stage_device(sship_nn* nn, int n0, const void* desc0, int n1, const void* desc1) {
  const NnStage st = nn_stage(nn->max_kp);
  SSHIP_HIP_CHECK(hipMemcpyAsync(nn->one.dev<char>(st.desc), desc0, (size_t)n0 * 256 * sizeof(_Float16), hipMemcpyDeviceToDevice, nn->stream));
  SSHIP_HIP_CHECK(hipMemcpyAsync(nn->one.dev<char>(st.desc1), desc1, (size_t)n1 * 256 * sizeof(_Float16), hipMemcpyDeviceToDevice, nn->stream));
  return SSHIP_OK;
}
static int nn_stage_host(sship_nn* nn, int n0, const float* desc0, int n1, const float* desc1);
extern "C" int sship_nn_match_device(sship_nn* nn, int n0, const void* desc0, int n1, const void* desc1, int32_t* matches0, float* mscores0) {
  if (int rc = nn_check_pair(nn, n0, desc0, n1, desc1, matches0, mscores0, "nn_match_device")) return rc;
  if (nn->gate_on) return fail(SSHIP_ERR_INVALID, std::string("nn_match_device") + kNnGatedMsg);
  bind_thread();
  if (int rc = nn_stage_device(nn, n0, desc0, n1, desc1)) return rc;
  return nn_match_common(nn, n0, n1, matches0, mscores0);
}
extern "C" int sship_nn_match_gated_device(sship_nn* nn, const float* kp0, int st0, int n0, const void* desc0, const float* kp1, int st1, int n1,
                                           const void* desc1, int32_t* matches0, float* mscores0) {
  if (int rc = nn_check_pair(nn, n0, desc0, n1, desc1, matches0, mscores0, "nn_match_gated_device")) return rc;
  if (int rc = nn_check_kp(nn, kp0, st0, kp1, st1, "nn_match_gated_device")) return rc;
  bind_thread();
  if (int rc = nn_stage_device(nn, n0, desc0, n1, desc1)) return rc;
  if (!nn->gate_on) return nn_match_common(nn, n0, n1, matches0, mscores0);
  return nn_match_common(nn, n0, n1, matches0, mscores0, kp0, st0, kp1, st1);
}
extern "C" int sship_nn_match_gated_host(sship_nn* nn, const float* kp0, int st0, int n0, const float* desc0, const float* kp1, int st1, int n1,
                                         const float* desc1, int32_t* matches0, float* mscores0) {
  if (int rc = nn_check_pair(nn, n0, desc0, n1, desc1, matches0, mscores0, "nn_match_gated_host")) return rc;
  if (int rc = nn_check_kp(nn, kp0, st0, kp1, st1, "nn_match_gated_host")) return rc;
  bind_thread();
  if (int rc = nn_stage_host(nn, n0, desc0, n1, desc1)) return rc;
  if (!nn->gate_on) return nn_match_common(nn, n0, n1, matches0, mscores0);
  return nn_match_common(nn, n0, n1, matches0, mscores0, kp0, st0, kp1, st1);
}
extern "C" int sship_nn_match_host(sship_nn* nn, int n0, const float* desc0, int n1, const float* desc1, int32_t* matches0, float* mscores0) {
  if (int rc = nn_check_pair(nn, n0, desc0, n1, desc1, matches0, mscores0, "nn_match_host")) return rc;
  if (nn->gate_on) return fail(SSHIP_ERR_INVALID, std::string("nn_match_host") + kNnGatedMsg);
  bind_thread();
  if (int rc = nn_stage_host(nn, n0, desc0, n1, desc1)) return rc;
  return nn_match_common(nn, n0, n1, matches0, mscores0);
}
static int nn_stage_host(sship_nn* nn, int n0, const float* desc0, int n1, const float* desc1) {
  const NnStage st = nn_stage(nn->max_kp);
  nn_pack_desc(nn->one.host<char>(0), st, n0, desc0, n1, desc1);
  SSHIP_HIP_CHECK(nn->one.upload(st.desc, (size_t)n0 * 256 * sizeof(_Float16), nn->stream));
  SSHIP_HIP_CHECK(nn->one.upload(st.desc1, (size_t)n1 * 256 * sizeof(_Float16), nn->stream));
  return SSHIP_OK;
}
// Measurement hook (include/sship.h): the last call's two launches (the gated ones after a gated call) re-run `iters` times on the handle's stream.
extern "C" int sship_nn_bench(sship_nn* nn, int iters, float* avg_ms) { return bench_last(nn, iters, avg_ms, "nn_bench", "match", nn_run); }

// ====================================================================================================
// EigenPlaces place recogniser: include/EigenPlaces.h:19-40, src/EigenPlaces.cc:47-174
// ====================================================================================================
struct sship_ep {
  int in_w = 0, in_h = 0;
  hipStream_t stream = nullptr;
  ConvW stem;
  struct Block { ConvW c1, c2, ds; bool has_ds = false; int stride = 1; } blocks[8];
  float* fc_wt = nullptr;   // [in 512][out 512] fp32 (transposed)
  float* fc_b = nullptr;
  float gem_p = 3.f;
  DevBuf d_in, patches, act[4], d_out;   // patches: the im2col matrix of the GEMM stem (developer build's A/B path only)
  DevBuf stem_frag, stem_bias;           // fused stem (round 6): [2][11][64][8] fp16 A fragments, fp32 bias [64]
  PinBuf h_out;
  DevBuf d_ws, d_tail;      // split-K partial sums; the tail's partial GeM sums, [512] pre-normalisation outputs + its arrival counter
  DevBuf d_img;             // u8 entry points: the uploaded image
  PinBuf h_img;
  // resize tables of (src_h, src_w) -> (in_h, in_w), one IMMUTABLE device buffer per source size seen (a dataset has one; a rig a few).
  // A set is written once, before its first use, and never touched again: no call on any stream can observe a table changing under it, so
  // the asynchronous entry point needs no device-wide synchronisation (round 5 re-used one buffer behind a hipDeviceSynchronize).
  struct Tables { int h = 0, w = 0; DevBuf d; };
  std::vector<std::unique_ptr<Tables>> tables;
  // test-only capture (include/sship.h: sship_ep_debug_capture): one buffer per stage, allocated when capture is first switched on
  static constexpr int kStages = 29;
  bool capture = false, captured = false, cap_ready = false;   // captured: a call has run since capture was switched on
  size_t cap_bytes[kStages] = {};           // 0: the stage does not exist (a block without a downsample)
  DevBuf cap[kStages];
  // batch entry points (sship_ep_reserve_batch): d_in, act, d_ws, d_tail and d_out / h_out hold max_batch images ([B][...] slices; the
  // single-image path uses slice 0 of the same buffers); cap_image = the image of a batch call the capture copies aside
  int max_batch = 1, cap_image = 0;
};
// words (4 bytes) between the tail slices of two images: [kTailPoolWg * 512 | 512] floats, the arrival counter, one pad word
static size_t ep_tail_slice() { return ep_tail_ws_floats() + 2; }
extern "C" void sship_ep_destroy(sship_ep* ep) {
  bind_thread();
  if (!ep) return;
  (void)hipDeviceSynchronize();
  free_conv(ep->stem);
  for (auto& b : ep->blocks) { free_conv(b.c1); free_conv(b.c2); free_conv(b.ds); }
  if (ep->fc_wt) (void)hipFree(ep->fc_wt);
  if (ep->fc_b) (void)hipFree(ep->fc_b);
  if (ep->stream) (void)hipStreamDestroy(ep->stream);
  delete ep;
}
extern "C" int sship_ep_create(const char* weights_path, int input_w, int input_h, sship_ep** out) {
  bind_thread();
  if (!weights_path || !out || input_w < 32 || input_h < 32) return fail(SSHIP_ERR_INVALID, "ep_create: bad arguments");
  if (int rc = require_device()) return rc;
  StateDict sd; std::string err;
  if (!load_safetensors(weights_path, sd, err)) return fail(SSHIP_ERR_IO, err);
  std::unique_ptr<sship_ep, void (*)(sship_ep*)> ep(new sship_ep(), sship_ep_destroy);
  ep->in_w = input_w; ep->in_h = input_h;
  // conv + BatchNorm (eval) folded: w' = w * g / sqrt(var + 1e-5), b' = beta - mean * g / sqrt(var + 1e-5)
  auto folded = [&](const std::string& conv, const std::string& bn, int cout, int cin, int ks, int cin_pad, ConvW& dst) -> int {
    const Tensor* w = find_tensor(sd, conv + ".weight", {cout, cin, ks, ks}, err);
    const Tensor* g = w ? find_tensor(sd, bn + ".weight", {cout}, err) : nullptr;
    const Tensor* be = g ? find_tensor(sd, bn + ".bias", {cout}, err) : nullptr;
    const Tensor* mu = be ? find_tensor(sd, bn + ".running_mean", {cout}, err) : nullptr;
    const Tensor* var = mu ? find_tensor(sd, bn + ".running_var", {cout}, err) : nullptr;
    if (!var) return fail(SSHIP_ERR_IO, err);
    const int kk = ks * ks;
    const bool flat = cin_pad != cin;  // the stem: [cout][cin*ks*ks] rows zero-padded to cin_pad, run as a 1x1 GEMM
    std::vector<float> wf((size_t)cout * (flat ? cin_pad : cin * kk), 0.f), bf(cout);
    for (int co = 0; co < cout; ++co) {
      const float sc = g->data[co] / sqrtf(var->data[co] + 1e-5f);
      bf[co] = be->data[co] - mu->data[co] * sc;
      for (int i = 0; i < cin * kk; ++i) wf[(size_t)co * (flat ? cin_pad : cin * kk) + i] = w->data[(size_t)co * cin * kk + i] * sc;
    }
    if (flat) {
      // the fused stem kernel's A fragments (ep_kernels.hip: k_ep_stem_pool): fragment (m, s), lane (row, kg) = W'[32 m + row][idx = 2 s + kg][kx 0..7],
      // idx = c * 7 + ky; idx = 21 and kx = 7 are zero padding of K
      std::vector<_Float16> fr((size_t)2 * 11 * 64 * 8);
      for (int m = 0; m < 2; ++m)
        for (int st = 0; st < 11; ++st)
          for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 8; ++e) {
              const int row = lane & 31, idx = 2 * st + (lane >> 5);
              float v = 0.f;
              if (idx < cin * ks && e < ks) v = wf[(size_t)(32 * m + row) * cin_pad + (idx / ks) * kk + (idx % ks) * ks + e];
              fr[((size_t)(m * 11 + st) * 64 + lane) * 8 + e] = (_Float16)v;
            }
      SSHIP_HIP_CHECK(ep->stem_frag.ensure(fr.size() * sizeof(_Float16)));
      SSHIP_HIP_CHECK(hipMemcpy(ep->stem_frag.p, fr.data(), fr.size() * sizeof(_Float16), hipMemcpyHostToDevice));
      SSHIP_HIP_CHECK(ep->stem_bias.ensure(bf.size() * sizeof(float)));
      SSHIP_HIP_CHECK(hipMemcpy(ep->stem_bias.p, bf.data(), bf.size() * sizeof(float), hipMemcpyHostToDevice));
      if (!SSHIP_DEV_SWITCHES) return SSHIP_OK;   // the GEMM form of the stem exists in the developer build only (A/B: SUPERSLAM_HIP_EP_STEM=gemm)
    }
    return upload_conv(wf.data(), bf.data(), cout, flat ? cin_pad : cin, flat ? 1 : ks, 64, dst);
  };
  if (int rc = folded("backbone.0", "backbone.1", 64, 3, 7, 192, ep->stem)) return rc;
  const int planes[4] = {64, 128, 256, 512};
  int cin = 64;
  for (int L = 0; L < 4; ++L)
    for (int b = 0; b < 2; ++b) {
      sship_ep::Block& blk = ep->blocks[L * 2 + b];
      const std::string p = "backbone." + std::to_string(4 + L) + "." + std::to_string(b);
      const int c_in = b == 0 ? cin : planes[L];
      blk.stride = (b == 0 && L > 0) ? 2 : 1;
      if (int rc = folded(p + ".conv1", p + ".bn1", planes[L], c_in, 3, c_in, blk.c1)) return rc;
      if (int rc = folded(p + ".conv2", p + ".bn2", planes[L], planes[L], 3, planes[L], blk.c2)) return rc;
      if (b == 0 && (blk.stride != 1 || c_in != planes[L])) {
        blk.has_ds = true;
        if (int rc = folded(p + ".downsample.0", p + ".downsample.1", planes[L], c_in, 1, c_in, blk.ds)) return rc;
      }
      if (b == 1) cin = planes[L];
    }
  {
    const Tensor* gp = find_tensor(sd, "aggregation.1.p", {1}, err);
    const Tensor* w = gp ? find_tensor(sd, "aggregation.3.weight", {512, 512}, err) : nullptr;
    const Tensor* bb = w ? find_tensor(sd, "aggregation.3.bias", {512}, err) : nullptr;
    if (!bb) return fail(SSHIP_ERR_IO, err);
    ep->gem_p = gp->data[0];
    std::vector<float> wt((size_t)512 * 512);
    for (int j = 0; j < 512; ++j)
      for (int c = 0; c < 512; ++c) wt[(size_t)c * 512 + j] = w->data[(size_t)j * 512 + c];
    if (int rc = upload_floats(wt.data(), wt.size(), &ep->fc_wt)) return rc;
    if (int rc = upload_floats(bb->data.data(), 512, &ep->fc_b)) return rc;
  }
  const int Ho = (input_h - 1) / 2 + 1, Wo = (input_w - 1) / 2 + 1;
  SSHIP_HIP_CHECK(ep->d_in.ensure((size_t)3 * input_h * input_w * 4));
  if (SSHIP_DEV_SWITCHES) SSHIP_HIP_CHECK(ep->patches.ensure((size_t)Ho * Wo * 192 * 2));
  for (auto& a : ep->act) SSHIP_HIP_CHECK(a.ensure((size_t)Ho * Wo * 64 * 2));
  SSHIP_HIP_CHECK(ep->d_out.ensure(512 * 4));
  SSHIP_HIP_CHECK(ep->h_out.ensure(512 * 4));
  SSHIP_HIP_CHECK(ep->d_ws.ensure(ep_splitk_workspace_bytes(input_h, input_w)));
  SSHIP_HIP_CHECK(ep->d_tail.ensure((ep_tail_ws_floats() + 2) * 4));
  SSHIP_HIP_CHECK(hipMemset(ep->d_tail.p, 0, (ep_tail_ws_floats() + 2) * 4));
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&ep->stream, hipStreamDefault));
  *out = ep.release();
  return SSHIP_OK;
}
extern "C" int sship_ep_descriptor_dim(const sship_ep* ep) { return ep ? 512 : 0; }
// host half of compute_global_descriptor (no GPU involved): include/superslam_hip/place_recognizer.hpp
extern "C" int sship_ep_preprocess(const uint8_t* img, int h, int w, int stride, int channels, int input_w, int input_h, float* chw_out) {
  if (!img || !chw_out || h <= 0 || w <= 0 || input_w <= 0 || input_h <= 0 || (channels != 1 && channels != 3) || stride < w * channels)
    return fail(SSHIP_ERR_INVALID, "ep_preprocess: bad arguments");
  superslam_hip::eigenplaces_preprocess(superslam_hip::Image{img, h, w, channels, stride}, input_w, input_h, chw_out);
  return SSHIP_OK;
}
constexpr int kEpMaxBatch = 1024;
// sizes of the capture stages of an engine (the numbering of include/sship.h), from the same ceil chain as ep_network
static void ep_stage_bytes(const sship_ep* ep, size_t (&bytes)[sship_ep::kStages]) {
  int h = (ep->in_h - 1) / 2 + 1, w = (ep->in_w - 1) / 2 + 1;
  h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1;
  bytes[0] = (size_t)3 * ep->in_h * ep->in_w * 4;
  bytes[1] = (size_t)h * w * 64 * 2;
  for (int i = 0; i < 8; ++i) {
    const auto& blk = ep->blocks[i];
    if (blk.stride == 2) { h = (h + 1) / 2; w = (w + 1) / 2; }
    const size_t n = (size_t)h * w * blk.c2.cout * 2;
    bytes[2 + 3 * i] = n; bytes[3 + 3 * i] = blk.has_ds ? n : 0; bytes[4 + 3 * i] = n;
  }
  bytes[26] = (size_t)ep_tail_pool_wgs(h * w) * 512 * 4;
  bytes[27] = 512 * 4;
  bytes[28] = 512 * 4;
}
// the network from the preprocessed fp32 [3, H, W] tensor in d_in to the descriptor in `desc_dev`, on stream s
static int ep_network(sship_ep* ep, float* desc_dev, hipStream_t s) {
  const int H = ep->in_h, W = ep->in_w;
  int h = (H - 1) / 2 + 1, w = (W - 1) / 2 + 1;
  // test-only capture: a stream-ordered device-to-device copy of a stage's output; off (the default) makes no call at all
  auto cap = [&](int stage, const void* src) -> hipError_t {
    if (!ep->capture) return hipSuccess;
    return hipMemcpyAsync(ep->cap[stage].p, src, ep->cap_bytes[stage], hipMemcpyDeviceToDevice, s);
  };
  SSHIP_HIP_CHECK(cap(0, ep->d_in.p));
  _Float16* a[4] = {ep->act[0].as<_Float16>(), ep->act[1].as<_Float16>(), ep->act[2].as<_Float16>(), ep->act[3].as<_Float16>()};
  const int hp = (h - 1) / 2 + 1, wp = (w - 1) / 2 + 1;  // MaxPool2d(3, 2, 1)
#if SSHIP_DEV_SWITCHES  // A/B: the stem of rounds 3-5 (im2col -> 1x1 GEMM -> max-pool, three launches)
  static const bool stem_gemm = [] { const char* e = dev_env("SUPERSLAM_HIP_EP_STEM"); return e && std::string(e) == "gemm"; }();
  if (stem_gemm) {
    launch_ep_im2col(ep->d_in.as<float>(), H, W, h, w, ep->patches.as<_Float16>(), s);
    SSHIP_HIP_CHECK(ep_conv(ep->stem, ep->patches.as<_Float16>(), a[0], nullptr, h, w, true, false, s));
    launch_ep_maxpool(a[0], h, w, hp, wp, a[1], s);
  } else
#endif
  launch_ep_stem_pool(ep->d_in.as<float>(), H, W, h, w, hp, wp, ep->stem_frag.as<_Float16>(), ep->stem_bias.as<float>(), a[1], s);
  h = hp; w = wp;
  SSHIP_HIP_CHECK(cap(1, a[1]));
  int cur = 1;  // index of the buffer holding the block input
  int stage = 2;  // capture stage of this block's conv1 (then its downsample, then its output)
  for (const auto& blk : ep->blocks) {
    int f[3], k = 0;
    for (int i = 0; i < 4; ++i) if (i != cur) f[k++] = i;  // three free buffers: t, ds, out
    const _Float16* res = a[cur];
    int ho = h, wo = w;
    if (blk.stride == 2) { ho = (h + 1) / 2; wo = (w + 1) / 2; }
    float* ws = ep->d_ws.as<float>();
    const size_t wsb = ep->d_ws.bytes;
    SSHIP_HIP_CHECK(ep_conv(blk.c1, a[cur], a[f[0]], nullptr, h, w, true, blk.stride == 2, s, ws, wsb));
    SSHIP_HIP_CHECK(cap(stage, a[f[0]]));
    if (blk.has_ds) {
      SSHIP_HIP_CHECK(ep_conv(blk.ds, a[cur], a[f[1]], nullptr, h, w, false, blk.stride == 2, s));
      SSHIP_HIP_CHECK(cap(stage + 1, a[f[1]]));
      res = a[f[1]];
    }
    SSHIP_HIP_CHECK(ep_conv(blk.c2, a[f[0]], a[f[2]], res, ho, wo, true, false, s, ws, wsb));
    SSHIP_HIP_CHECK(cap(stage + 2, a[f[2]]));
    cur = f[2]; h = ho; w = wo; stage += 3;
  }
  launch_ep_tail(a[cur], h * w, ep->gem_p, ep->fc_wt, ep->fc_b, ep->d_tail.as<float>(), ep->d_tail.as<int>() + ep_tail_ws_floats(), desc_dev, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  SSHIP_HIP_CHECK(cap(26, ep->d_tail.p));
  SSHIP_HIP_CHECK(cap(27, ep->d_tail.as<float>() + ep_tail_ws_floats() - 512));
  SSHIP_HIP_CHECK(cap(28, desc_dev));
  if (ep->capture) ep->captured = true;
  return SSHIP_OK;
}
// The same network for B images: the preprocessed [B][3][H][W] tensor in d_in -> row b of desc_dev (desc_stride floats apart).  Every map is
// [B][h][w][c]; per image the launches compute what ep_network computes, bit for bit (include/sship.h: the batch rule).  The capture copies
// image cap_image's slice of every stage (nothing when the batch does not hold that image).
static int ep_network_batch(sship_ep* ep, int B, float* desc_dev, int desc_stride, hipStream_t s) {
  const int H = ep->in_h, W = ep->in_w;
  int h = (H - 1) / 2 + 1, w = (W - 1) / 2 + 1;
  const bool capturing = ep->capture && ep->cap_image < B;
  const size_t ci = (size_t)ep->cap_image;
  auto cap = [&](int stage, const void* base, size_t image_bytes) -> hipError_t {
    if (!capturing) return hipSuccess;
    return hipMemcpyAsync(ep->cap[stage].p, static_cast<const char*>(base) + ci * image_bytes, ep->cap_bytes[stage], hipMemcpyDeviceToDevice, s);
  };
  auto cap_map = [&](int stage, const void* base) { return cap(stage, base, ep->cap_bytes[stage]); };
  SSHIP_HIP_CHECK(cap_map(0, ep->d_in.p));
  _Float16* a[4] = {ep->act[0].as<_Float16>(), ep->act[1].as<_Float16>(), ep->act[2].as<_Float16>(), ep->act[3].as<_Float16>()};
  const int hp = (h - 1) / 2 + 1, wp = (w - 1) / 2 + 1;
  launch_ep_stem_pool(ep->d_in.as<float>(), H, W, h, w, hp, wp, ep->stem_frag.as<_Float16>(), ep->stem_bias.as<float>(), a[1], s, B);
  h = hp; w = wp;
  SSHIP_HIP_CHECK(cap_map(1, a[1]));
  int cur = 1, stage = 2;
  float* ws = ep->d_ws.as<float>();
  const size_t wsb = ep->d_ws.bytes, ws1 = ep_splitk_workspace_bytes(H, W);
  for (const auto& blk : ep->blocks) {
    int f[3], k = 0;
    for (int i = 0; i < 4; ++i) if (i != cur) f[k++] = i;
    const _Float16* res = a[cur];
    int ho = h, wo = w;
    if (blk.stride == 2) { ho = (h + 1) / 2; wo = (w + 1) / 2; }
    SSHIP_HIP_CHECK(ep_conv_batch(blk.c1, a[cur], a[f[0]], nullptr, h, w, true, blk.stride == 2, B, s, ws, wsb, ws1));
    SSHIP_HIP_CHECK(cap_map(stage, a[f[0]]));
    if (blk.has_ds) {
      SSHIP_HIP_CHECK(ep_conv_batch(blk.ds, a[cur], a[f[1]], nullptr, h, w, false, blk.stride == 2, B, s, nullptr, 0, 0));
      SSHIP_HIP_CHECK(cap_map(stage + 1, a[f[1]]));
      res = a[f[1]];
    }
    SSHIP_HIP_CHECK(ep_conv_batch(blk.c2, a[f[0]], a[f[2]], res, ho, wo, true, false, B, s, ws, wsb, ws1));
    SSHIP_HIP_CHECK(cap_map(stage + 2, a[f[2]]));
    cur = f[2]; h = ho; w = wo; stage += 3;
  }
  const size_t slice = ep_tail_slice();
  launch_ep_tail(a[cur], h * w, ep->gem_p, ep->fc_wt, ep->fc_b, ep->d_tail.as<float>(), ep->d_tail.as<int>() + ep_tail_ws_floats(), desc_dev, s, B,
                 (int)slice, desc_stride);
  SSHIP_HIP_CHECK(hipGetLastError());
  SSHIP_HIP_CHECK(cap(26, ep->d_tail.p, slice * 4));
  SSHIP_HIP_CHECK(cap(27, ep->d_tail.as<float>() + ep_tail_ws_floats() - 512, slice * 4));
  SSHIP_HIP_CHECK(cap(28, desc_dev, (size_t)desc_stride * 4));
  if (ep->capture) ep->captured = capturing;
  return SSHIP_OK;
}
// Test-only (include/sship.h): per-stage capture of the network's activations
extern "C" int sship_ep_debug_capture(sship_ep* ep, int on) {
  bind_thread();
  if (!ep) return fail(SSHIP_ERR_INVALID, "ep_debug_capture: null handle");
  if (on && !ep->cap_ready) {
    ep_stage_bytes(ep, ep->cap_bytes);
    for (int i = 0; i < sship_ep::kStages; ++i)
      if (ep->cap_bytes[i]) SSHIP_HIP_CHECK(ep->cap[i].ensure(ep->cap_bytes[i]));
    ep->cap_ready = true;
  }
  ep->capture = on != 0;
  ep->captured = false;
  return SSHIP_OK;
}
extern "C" int sship_ep_debug_capture_image(sship_ep* ep, int image) {
  if (!ep || image < 0 || image >= kEpMaxBatch) return fail(SSHIP_ERR_INVALID, "ep_debug_capture_image: null handle or image outside 0..1023");
  ep->cap_image = image;
  ep->captured = false;
  return SSHIP_OK;
}
extern "C" int sship_ep_debug_activation(sship_ep* ep, int stage, void* out_host, unsigned long long bytes) {
  bind_thread();
  if (!ep || !out_host) return fail(SSHIP_ERR_INVALID, "ep_debug_activation: null argument");
  if (!ep->capture || !ep->captured) return fail(SSHIP_ERR_INVALID, "ep_debug_activation: capture is off or no call has run since it was switched on");
  if (stage < 0 || stage >= sship_ep::kStages || !ep->cap_bytes[stage] || bytes > ep->cap_bytes[stage])
    return fail(SSHIP_ERR_INVALID, "ep_debug_activation: bad stage / size");
  SSHIP_HIP_CHECK(hipDeviceSynchronize());
  SSHIP_HIP_CHECK(hipMemcpy(out_host, ep->cap[stage].p, bytes, hipMemcpyDeviceToHost));
  return SSHIP_OK;
}
extern "C" int sship_ep_infer(sship_ep* ep, const float* chw_host, float* desc_out) {
  bind_thread();
  if (!ep || !chw_host || !desc_out) return fail(SSHIP_ERR_INVALID, "ep_infer: null argument");
  hipStream_t s = ep->stream;
  SSHIP_HIP_CHECK(hipMemcpyAsync(ep->d_in.p, chw_host, (size_t)3 * ep->in_h * ep->in_w * 4, hipMemcpyHostToDevice, s));
  if (int rc = ep_network(ep, ep->d_out.as<float>(), s)) return rc;
  SSHIP_HIP_CHECK(hipMemcpyAsync(ep->h_out.p, ep->d_out.p, 512 * 4, hipMemcpyDeviceToHost, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  memcpy(desc_out, ep->h_out.p, 512 * 4);
  return SSHIP_OK;
}
// resize tables of (h, w) -> (in_h, in_w).  The first call with a new source size allocates and uploads its set (hipMalloc + a blocking copy of
// ~ 8 (in_w + in_h) ints: not legal under stream capture - run one call per source size before capturing); every later call only looks it up.
constexpr size_t kEpMaxTableSets = 16;
static int ep_tables(sship_ep* ep, int h, int w, const int** tab_out) {
  for (const auto& t : ep->tables)
    if (t->h == h && t->w == w) { *tab_out = t->d.as<int>(); return SSHIP_OK; }
  std::vector<int> t[8];
  superslam_hip::resize_bilinear_coeffs(ep->in_w, w, t[0], t[1], t[2], t[3]);
  superslam_hip::resize_bilinear_coeffs(ep->in_h, h, t[4], t[5], t[6], t[7]);
  std::vector<int> flat;
  for (auto& v : t) flat.insert(flat.end(), v.begin(), v.end());
  if (ep->tables.size() >= kEpMaxTableSets) {  // a stream of ever-changing sizes: drop the oldest set once nothing can still be reading it
    SSHIP_HIP_CHECK(hipDeviceSynchronize());
    ep->tables.erase(ep->tables.begin());
  }
  auto set = std::make_unique<sship_ep::Tables>();
  SSHIP_HIP_CHECK(set->d.ensure(flat.size() * 4));
  SSHIP_HIP_CHECK(hipMemcpy(set->d.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));  // a fresh buffer nobody reads yet
  set->h = h; set->w = w;
  *tab_out = set->d.as<int>();
  ep->tables.push_back(std::move(set));
  return SSHIP_OK;
}
static int ep_check_image(const void* img, int h, int w, int stride, int channels, const char* who) {
  if (!img || h <= 0 || w <= 0 || (channels != 1 && channels != 3) || stride < w * channels || h > 16384 || w > 16384)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": bad image arguments");
  return SSHIP_OK;
}
extern "C" int sship_ep_infer_u8_device(sship_ep* ep, const uint8_t* img_dev, int h, int w, int stride, int channels, float* desc_out_dev,
                                        void* stream) {
  bind_thread();
  if (!ep || !desc_out_dev) return fail(SSHIP_ERR_INVALID, "ep_infer_u8_device: null argument");
  if (int rc = ep_check_image(img_dev, h, w, stride, channels, "ep_infer_u8_device")) return rc;
  const int* tab = nullptr;
  if (int rc = ep_tables(ep, h, w, &tab)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_ep_resize_norm(img_dev, stride, channels, tab, ep->in_w, ep->in_h, ep->d_in.as<float>(), s);
  return ep_network(ep, desc_out_dev, s);
}
extern "C" int sship_ep_infer_u8(sship_ep* ep, const uint8_t* img, int h, int w, int stride, int channels, float* desc_out) {
  bind_thread();
  if (!ep || !desc_out) return fail(SSHIP_ERR_INVALID, "ep_infer_u8: null argument");
  if (int rc = ep_check_image(img, h, w, stride, channels, "ep_infer_u8")) return rc;
  hipStream_t s = ep->stream;
  const size_t row = (size_t)w * channels, bytes = row * h;
  SSHIP_HIP_CHECK(ep->h_img.ensure(bytes));
  SSHIP_HIP_CHECK(ep->d_img.ensure(bytes));
  for (int y = 0; y < h; ++y) memcpy(ep->h_img.as<uint8_t>() + (size_t)y * row, img + (size_t)y * stride, row);  // pinned, dense rows
  SSHIP_HIP_CHECK(hipMemcpyAsync(ep->d_img.p, ep->h_img.p, bytes, hipMemcpyHostToDevice, s));
  if (int rc = sship_ep_infer_u8_device(ep, ep->d_img.as<uint8_t>(), h, w, (int)row, channels, ep->d_out.as<float>(), s)) return rc;
  SSHIP_HIP_CHECK(hipMemcpyAsync(ep->h_out.p, ep->d_out.p, 512 * 4, hipMemcpyDeviceToHost, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  memcpy(desc_out, ep->h_out.p, 512 * 4);
  return SSHIP_OK;
}
extern "C" int sship_ep_bench(sship_ep* ep, const uint8_t* img_dev, int h, int w, int stride, int channels, int iters, float* avg_ms) {
  bind_thread();
  if (!ep || !avg_ms || iters <= 0) return fail(SSHIP_ERR_INVALID, "ep_bench: bad arguments");
  if (int rc = ep_check_image(img_dev, h, w, stride, channels, "ep_bench")) return rc;
  hipStream_t s = ep->stream;
  if (int rc = sship_ep_infer_u8_device(ep, img_dev, h, w, stride, channels, ep->d_out.as<float>(), s)) return rc;  // warm (also uploads the tables)
  EventPair ev;
  if (hipEventCreate(&ev.e0) != hipSuccess || hipEventCreate(&ev.e1) != hipSuccess) return fail(SSHIP_ERR_HIP, "ep_bench: hipEventCreate failed");
  if (hipEventRecord(ev.e0, s) != hipSuccess) return fail(SSHIP_ERR_HIP, "ep_bench: hipEventRecord failed");
  for (int i = 0; i < iters; ++i)
    if (int rc = sship_ep_infer_u8_device(ep, img_dev, h, w, stride, channels, ep->d_out.as<float>(), s)) return rc;
  float ms = 0.f;
  if (hipEventRecord(ev.e1, s) != hipSuccess || hipEventSynchronize(ev.e1) != hipSuccess || hipEventElapsedTime(&ms, ev.e0, ev.e1) != hipSuccess)
    return fail(SSHIP_ERR_HIP, "ep_bench: timing failed");
  *avg_ms = ms / iters;
  return SSHIP_OK;
}

// ---- batches (include/sship.h "EigenPlaces: batches") ----
extern "C" int sship_ep_max_batch(const sship_ep* ep) { return ep ? ep->max_batch : 0; }
extern "C" size_t sship_ep_batch_workspace_bytes(int input_w, int input_h, int batch) {
  if (input_w < 32 || input_h < 32 || input_w > 16384 || input_h > 16384 || batch < 1 || batch > kEpMaxBatch) return 0;
  return ep_batch_workspace_bytes(input_h, input_w, batch);
}
template <class Buf>
static void swap_buf(Buf& a, Buf& b) { std::swap(a.p, b.p); std::swap(a.bytes, b.bytes); }
extern "C" int sship_ep_reserve_batch(sship_ep* ep, int max_batch) {
  bind_thread();
  if (!ep || max_batch < 1 || max_batch > kEpMaxBatch) return fail(SSHIP_ERR_INVALID, "ep_reserve_batch: null handle or max_batch outside 1..1024");
  if (max_batch <= ep->max_batch) return SSHIP_OK;   // never shrinks
  SSHIP_HIP_CHECK(hipDeviceSynchronize());           // nothing may still read the buffers that are about to be replaced
  const size_t n = (size_t)max_batch;
  const int H = ep->in_h, W = ep->in_w;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, hp = (Ho - 1) / 2 + 1, wp = (Wo - 1) / 2 + 1;
  // the largest map of the batch path is the pooled one (the stem map never reaches HBM); slice 0 keeps the single-image path's size
  size_t map_elems = (size_t)hp * wp * 64;
  for (int L = 0, hh = hp, ww = wp; L < 3; ++L) {
    hh = (hh + 1) / 2; ww = (ww + 1) / 2;
    map_elems = std::max(map_elems, (size_t)hh * ww * (128u << L));
  }
  const size_t act_bytes = std::max((size_t)Ho * Wo * 64 * 2, n * map_elems * 2);
  size_t ws_bytes = ep_splitk_workspace_bytes(H, W);
  for (int b = 1; b <= max_batch; ++b) ws_bytes = std::max(ws_bytes, ep_batch_workspace_bytes(H, W, b));  // a layer's need drops to 0 where it turns grouped
  // everything into fresh buffers first: a failed allocation leaves the handle as it was
  DevBuf in, act[4], ws, tail, out;
  PinBuf hout;
  hipError_t e = in.ensure(n * 3 * H * W * 4);
  for (auto& a : act) if (e == hipSuccess) e = a.ensure(act_bytes);
  if (e == hipSuccess) e = ws.ensure(ws_bytes);
  if (e == hipSuccess) e = tail.ensure(n * ep_tail_slice() * 4);
  if (e == hipSuccess) e = out.ensure(n * 512 * 4);
  if (e == hipSuccess) e = hout.ensure(n * 512 * 4);
  if (e == hipSuccess) e = hipMemset(tail.p, 0, n * ep_tail_slice() * 4);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(SSHIP_ERR_NOMEM, std::string("ep_reserve_batch: ") + hipGetErrorString(e) + " (the handle keeps its reservation of " +
                                     std::to_string(ep->max_batch) + ")");
  }
  swap_buf(ep->d_in, in);
  for (int i = 0; i < 4; ++i) swap_buf(ep->act[i], act[i]);
  swap_buf(ep->d_ws, ws); swap_buf(ep->d_tail, tail); swap_buf(ep->d_out, out); swap_buf(ep->h_out, hout);
  ep->max_batch = max_batch;
  return SSHIP_OK;
}
// the argument checks every batch entry shares: nothing on the device is touched and the handle is unchanged when they fail
static int ep_check_batch(const sship_ep* ep, const void* imgs, int batch, int h, int w, int stride, long long image_stride, int channels,
                          const char* who) {
  if (!ep) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null handle");
  if (batch < 1 || batch > ep->max_batch)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": batch " + std::to_string(batch) + " outside 1.." + std::to_string(ep->max_batch) +
                                       " (sship_ep_reserve_batch grows the reservation; a call never does)");
  if (int rc = ep_check_image(imgs, h, w, stride, channels, who)) return rc;
  if (image_stride < (long long)h * stride) return fail(SSHIP_ERR_INVALID, std::string(who) + ": image_stride below h * stride");
  return SSHIP_OK;
}
extern "C" int sship_ep_infer_u8_batch_device(sship_ep* ep, const uint8_t* imgs_dev, int batch, int h, int w, int stride, long long image_stride,
                                              int channels, float* desc_out_dev, int desc_stride, void* stream) {
  bind_thread();
  if (int rc = ep_check_batch(ep, imgs_dev, batch, h, w, stride, image_stride, channels, "ep_infer_u8_batch_device")) return rc;
  if (!desc_out_dev || desc_stride < 512) return fail(SSHIP_ERR_INVALID, "ep_infer_u8_batch_device: null output or desc_stride below 512");
  const int* tab = nullptr;
  if (int rc = ep_tables(ep, h, w, &tab)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_ep_resize_norm(imgs_dev, stride, channels, tab, ep->in_w, ep->in_h, ep->d_in.as<float>(), s, batch, image_stride);
  return ep_network_batch(ep, batch, desc_out_dev, desc_stride, s);
}
extern "C" int sship_ep_infer_u8_batch(sship_ep* ep, const uint8_t* imgs, int batch, int h, int w, int stride, long long image_stride, int channels,
                                       float* desc_out) {
  bind_thread();
  if (int rc = ep_check_batch(ep, imgs, batch, h, w, stride, image_stride, channels, "ep_infer_u8_batch")) return rc;
  if (!desc_out) return fail(SSHIP_ERR_INVALID, "ep_infer_u8_batch: null output");
  hipStream_t s = ep->stream;
  const size_t row = (size_t)w * channels, img_bytes = row * h, bytes = img_bytes * batch;
  SSHIP_HIP_CHECK(ep->h_img.ensure(bytes));
  SSHIP_HIP_CHECK(ep->d_img.ensure(bytes));
  for (int b = 0; b < batch; ++b)
    for (int y = 0; y < h; ++y)   // pinned, dense rows, dense images
      memcpy(ep->h_img.as<uint8_t>() + b * img_bytes + (size_t)y * row, imgs + (long long)b * image_stride + (size_t)y * stride, row);
  SSHIP_HIP_CHECK(hipMemcpyAsync(ep->d_img.p, ep->h_img.p, bytes, hipMemcpyHostToDevice, s));
  if (int rc = sship_ep_infer_u8_batch_device(ep, ep->d_img.as<uint8_t>(), batch, h, w, (int)row, (long long)img_bytes, channels,
                                              ep->d_out.as<float>(), 512, s))
    return rc;
  SSHIP_HIP_CHECK(hipMemcpyAsync(ep->h_out.p, ep->d_out.p, (size_t)batch * 512 * 4, hipMemcpyDeviceToHost, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  memcpy(desc_out, ep->h_out.p, (size_t)batch * 512 * 4);
  return SSHIP_OK;
}
// Measurement hook: `iters` back-to-back batch calls on the handle's stream over resident images; *avg_ms = the mean duration of ONE batch call
extern "C" int sship_ep_bench_batch(sship_ep* ep, const uint8_t* imgs_dev, int batch, int h, int w, int stride, long long image_stride, int channels,
                                    int iters, float* avg_ms) {
  bind_thread();
  if (!avg_ms || iters <= 0) return fail(SSHIP_ERR_INVALID, "ep_bench_batch: bad arguments");
  if (int rc = ep_check_batch(ep, imgs_dev, batch, h, w, stride, image_stride, channels, "ep_bench_batch")) return rc;
  hipStream_t s = ep->stream;
  float* out = ep->d_out.as<float>();
  int rc = SSHIP_OK;
  auto run = [&]() -> hipError_t {
    rc = sship_ep_infer_u8_batch_device(ep, imgs_dev, batch, h, w, stride, image_stride, channels, out, 512, s);
    return rc == SSHIP_OK ? hipSuccess : hipErrorUnknown;
  };
  const int brc = bench_loop(s, iters, run, avg_ms);   // the first (warm) run also uploads the tables
  return rc != SSHIP_OK ? rc : brc;
}

// ====================================================================================================
// Place-recognition index (include/sship.h "Place-recognition index"; csrc/index_kernels.hip)
// ====================================================================================================
constexpr long long kIndexMaxBytes = 1ll << 31;  // capacity * dim * 4 (the header states it)
struct sship_index {
  int dim = 0, capacity = 0, max_queries = 0, max_top_k = 0;
  int size = 0;                 // host state, updated when an add is enqueued
  std::vector<int64_t> ids;     // [size] keyframe ids
  hipStream_t stream = nullptr;
  DevBuf db, qn, partial;       // [capacity][dim] stored rows; [ceil16(max_queries)][dim] normalised queries; chunk partials
  StageArena one;               // the per-query calls: one staged query and its results (index_stage)
  // the last query call's arguments (sship_index_bench re-runs its launches; the caller keeps a batch call's buffers alive until then)
  struct Last { const float* q = nullptr; long long q_stride = 0; int items = 0; const int* limits = nullptr; int limit_all = 0, top_k = 0, size = 0;
                float min_score = 0.f; int* rows = nullptr; float* scores = nullptr; int* counts = nullptr; } last;
};
extern "C" int sship_index_create(int dim, int capacity, int max_queries, int max_top_k, sship_index** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "index_create: null argument");
  *out = nullptr;
  if (dim < 4 || dim > 4096 || dim % 4) return fail(SSHIP_ERR_INVALID, "index_create: dim must be a multiple of 4 in [4, 4096]");
  if (capacity < 1 || (long long)capacity * dim * 4 > kIndexMaxBytes) return fail(SSHIP_ERR_INVALID, "index_create: capacity must be >= 1 and capacity * dim * 4 <= 2 GiB");
  if (max_queries < 1 || max_queries > 1024) return fail(SSHIP_ERR_INVALID, "index_create: max_queries must be in [1, 1024]");
  if (max_top_k < 1 || max_top_k > kIndexMaxTopK) return fail(SSHIP_ERR_INVALID, "index_create: max_top_k must be in [1, 128]");
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_index, void (*)(sship_index*)> ix(new sship_index(), sship_index_destroy);
  ix->dim = dim; ix->capacity = capacity; ix->max_queries = max_queries; ix->max_top_k = max_top_k;
  ix->ids.reserve(capacity);
  const size_t chunks = ((size_t)capacity + kIndexRows - 1) / kIndexRows;
  const size_t qpad = ((size_t)max_queries + kIndexTile - 1) / kIndexTile * kIndexTile;
  SSHIP_HIP_CHECK(ix->db.ensure((size_t)capacity * dim * 4));
  SSHIP_HIP_CHECK(ix->qn.ensure(qpad * dim * 4));
  SSHIP_HIP_CHECK(ix->partial.ensure(chunks * max_queries * max_top_k * 8));
  const IndexStage st = index_stage(dim, max_top_k);
  SSHIP_HIP_CHECK(ix->one.create(st.in_bytes, st.out_bytes));
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&ix->stream, hipStreamDefault));
  *out = ix.release();
  return SSHIP_OK;
}
extern "C" void sship_index_destroy(sship_index* ix) { destroy_handle(ix); }
extern "C" int sship_index_dim(const sship_index* ix) { return ix ? ix->dim : 0; }
extern "C" int sship_index_capacity(const sship_index* ix) { return ix ? ix->capacity : 0; }
extern "C" int sship_index_size(const sship_index* ix) { return ix ? ix->size : 0; }
extern "C" int sship_index_clear(sship_index* ix) {
  if (!ix) return fail(SSHIP_ERR_INVALID, "index_clear: null handle");
  ix->size = 0; ix->ids.clear(); ix->last = sship_index::Last();
  return SSHIP_OK;
}
static int index_check_add(const sship_index* ix, const int64_t* ids, const float* desc, int count, int row_stride, const char* who) {
  if (!ix || !ids || !desc) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (count < 1) return fail(SSHIP_ERR_INVALID, std::string(who) + ": count must be >= 1");
  if (row_stride < ix->dim) return fail(SSHIP_ERR_INVALID, std::string(who) + ": row_stride must be >= dim");
  if (count > ix->capacity - ix->size) return fail(SSHIP_ERR_INVALID, std::string(who) + ": the index is full (size + count exceeds capacity)");
  return SSHIP_OK;
}
static void index_commit_add(sship_index* ix, const int64_t* ids, int count) {
  ix->ids.insert(ix->ids.end(), ids, ids + count);
  ix->size += count;
}
extern "C" int sship_index_add_device(sship_index* ix, const int64_t* ids, const float* desc_dev, int count, int row_stride, void* stream) {
  if (int rc = index_check_add(ix, ids, desc_dev, count, row_stride, "index_add_device")) return rc;
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_index_normalize(desc_dev, row_stride, count, count, ix->dim, ix->db.as<float>() + (size_t)ix->size * ix->dim, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  index_commit_add(ix, ids, count);
  return SSHIP_OK;
}
// the raw rows go straight to their place in the database and are normalised there
extern "C" int sship_index_add_host(sship_index* ix, const int64_t* ids, const float* desc, int count, int row_stride) {
  if (int rc = index_check_add(ix, ids, desc, count, row_stride, "index_add_host")) return rc;
  bind_thread();
  hipStream_t s = ix->stream;
  float* dst = ix->db.as<float>() + (size_t)ix->size * ix->dim;
  SSHIP_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)ix->dim * 4, desc, (size_t)row_stride * 4, (size_t)ix->dim * 4, count, hipMemcpyHostToDevice, s));
  launch_index_normalize(dst, ix->dim, count, count, ix->dim, dst, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  index_commit_add(ix, ids, count);
  return SSHIP_OK;
}
extern "C" int sship_index_read(sship_index* ix, int first_row, int count, float* rows_out, int64_t* ids_out) {
  if (!ix) return fail(SSHIP_ERR_INVALID, "index_read: null handle");
  if (first_row < 0 || count < 0 || first_row > ix->size || count > ix->size - first_row)
    return fail(SSHIP_ERR_INVALID, "index_read: [first_row, first_row + count) must lie inside [0, size)");
  if (count == 0) return SSHIP_OK;
  if (ids_out) memcpy(ids_out, ix->ids.data() + first_row, (size_t)count * sizeof(int64_t));
  if (rows_out) {
    bind_thread();
    SSHIP_HIP_CHECK(hipDeviceSynchronize());  // an add may have been enqueued on the caller's stream
    SSHIP_HIP_CHECK(hipMemcpy(rows_out, ix->db.as<float>() + (size_t)first_row * ix->dim, (size_t)count * ix->dim * 4, hipMemcpyDeviceToHost));
  }
  return SSHIP_OK;
}
static int index_check_query(const sship_index* ix, int exclude_recent, int top_k, float min_score, const char* who) {
  if (exclude_recent < 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": exclude_recent must be >= 0");
  if (top_k < 1 || top_k > ix->max_top_k) return fail(SSHIP_ERR_INVALID, std::string(who) + ": top_k must be in [1, max_top_k] (there is no 'all')");
  if (std::isnan(min_score)) return fail(SSHIP_ERR_INVALID, std::string(who) + ": min_score is NaN");
  return SSHIP_OK;
}
static hipError_t index_run(const sship_index* ix, const sship_index::Last& l, hipStream_t s) {
  launch_index_query(ix->db.as<float>(), ix->dim, l.size, l.q, l.q_stride, l.items, l.limits, l.limit_all, l.top_k, l.min_score, ix->qn.as<float>(),
                     ix->partial.as<unsigned long long>(), l.rows, l.scores, l.counts, s);
  return hipGetLastError();
}
static int index_launch(sship_index* ix, const float* q, long long q_stride, int nq, const int* limits, int exclude_recent, int top_k, float min_score,
                        int* rows, float* scores, int* counts, hipStream_t s) {
  ix->last = {q, q_stride, nq, limits, exclude_recent >= ix->size ? 0 : ix->size - exclude_recent, top_k, ix->size, min_score, rows, scores, counts};
  SSHIP_HIP_CHECK(index_run(ix, ix->last, s));
  return SSHIP_OK;
}
extern "C" int sship_index_query_batch_device(sship_index* ix, const float* q_dev, int num_queries, int q_stride, const int32_t* limits_dev,
                                              int exclude_recent, int top_k, float min_score, int32_t* rows_dev, float* scores_dev,
                                              int32_t* counts_dev, void* stream) {
  if (!ix || !q_dev || !rows_dev || !scores_dev || !counts_dev) return fail(SSHIP_ERR_INVALID, "index_query_batch_device: null argument");
  if (num_queries < 1 || num_queries > ix->max_queries) return fail(SSHIP_ERR_INVALID, "index_query_batch_device: num_queries must be in [1, max_queries]");
  if (q_stride < ix->dim) return fail(SSHIP_ERR_INVALID, "index_query_batch_device: q_stride must be >= dim");
  if (int rc = index_check_query(ix, exclude_recent, top_k, min_score, "index_query_batch_device")) return rc;
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  if (int rc = index_launch(ix, q_dev, q_stride, num_queries, limits_dev, exclude_recent, top_k, min_score, rows_dev, scores_dev, counts_dev, s)) return rc;
  g_timer.mark("index_query:stream_final", s);
  return SSHIP_OK;
}
// one query, already enqueued into the arena's q slot on the handle's stream: the batch launches with Q = 1, results mapped to ids on the host
static int index_query_one(sship_index* ix, int exclude_recent, int top_k, float min_score, int64_t* ids_out, float* scores_out, int* count_out) {
  hipStream_t s = ix->stream;
  const StageArena& a = ix->one;
  const IndexStage st = index_stage(ix->dim, ix->max_top_k);
  if (int rc = index_launch(ix, a.dev<float>(st.q), ix->dim, 1, nullptr, exclude_recent, top_k, min_score, a.dev<int>(a.out + st.rows),
                            a.dev<float>(a.out + st.scores), a.dev<int>(a.out + st.count), s))
    return rc;
  SSHIP_HIP_CHECK(a.download(a.out, st.out_bytes, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  const int bad = index_unpack(a.host<char>(a.out), st, top_k, ix->ids.data(), ix->size, ids_out, scores_out, count_out);
  if (bad == 1) return fail(SSHIP_ERR_HIP, "index_query: the device returned an impossible count");
  if (bad == 2) return fail(SSHIP_ERR_HIP, "index_query: the device returned a row outside the index");
  return SSHIP_OK;
}
static int index_check_one(const sship_index* ix, const float* desc, int exclude_recent, int top_k, float min_score, const int64_t* ids_out,
                           const float* scores_out, const int* count_out, const char* who) {
  if (!ix || !desc || !ids_out || !scores_out || !count_out) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  return index_check_query(ix, exclude_recent, top_k, min_score, who);
}
extern "C" int sship_index_query_host(sship_index* ix, const float* desc, int exclude_recent, int top_k, float min_score, int64_t* ids_out,
                                      float* scores_out, int* count_out) {
  if (int rc = index_check_one(ix, desc, exclude_recent, top_k, min_score, ids_out, scores_out, count_out, "index_query_host")) return rc;
  bind_thread();
  const IndexStage st = index_stage(ix->dim, ix->max_top_k);
  index_pack(ix->one.host<char>(0), st, ix->dim, desc);
  SSHIP_HIP_CHECK(ix->one.upload(st.q, st.in_bytes - st.q, ix->stream));
  return index_query_one(ix, exclude_recent, top_k, min_score, ids_out, scores_out, count_out);
}
extern "C" int sship_index_query_device(sship_index* ix, const float* desc_dev, int exclude_recent, int top_k, float min_score, int64_t* ids_out,
                                        float* scores_out, int* count_out) {
  if (int rc = index_check_one(ix, desc_dev, exclude_recent, top_k, min_score, ids_out, scores_out, count_out, "index_query_device")) return rc;
  bind_thread();
  SSHIP_HIP_CHECK(hipMemcpyAsync(ix->one.dev<float>(index_stage(ix->dim, ix->max_top_k).q), desc_dev, (size_t)ix->dim * sizeof(float), hipMemcpyDeviceToDevice,
                                 ix->stream));
  return index_query_one(ix, exclude_recent, top_k, min_score, ids_out, scores_out, count_out);
}
// Measurement hook (include/sship.h): the last query call's launches (normalise, scan, merge) re-run `iters` times on the handle's stream.
extern "C" int sship_index_bench(sship_index* ix, int iters, float* avg_ms) { return bench_last(ix, iters, avg_ms, "index_bench", "query", index_run); }

// ====================================================================================================
// Pose-only stereo solver (include/sship.h "Pose-only stereo solver"; csrc/pose_kernels.hip)
// ====================================================================================================
constexpr int kPoseMaxPairs = 65535;
struct sship_pose {
  int max_obs = 0, max_pairs = 0;
  StereoCamera cam;
  sship_pose_params prm{10.0, 8.0, 40.0, 7.815, 1e-5, 1e5, 1e-5, 1e-5, 3.0, 100};
  hipStream_t stream = nullptr;
  StageArena one;   // sship_pose_solve_host: one staged pair and its results (pose_stage)
  // the last solve call's arguments (sship_pose_bench re-runs its launch; the caller keeps a batch call's buffers alive until then)
  struct Last { const float* points = nullptr; const float* meas = nullptr; const uint8_t* valid = nullptr; const double* pose0 = nullptr; int items = 0;
                double* pose = nullptr; int32_t* stats = nullptr; double* cost = nullptr; uint8_t* inlier = nullptr; } last;
};
static PoseK pose_constants(const sship_pose* ps) {
  PoseK k;
  k.fx = ps->cam.fx; k.fy = ps->cam.fy; k.cx = ps->cam.cx; k.cy = ps->cam.cy; k.baseline = ps->cam.baseline;
  k.inv_sigma_px = 1.0 / ps->prm.sigma_px; k.sigma_d0 = ps->prm.sigma_d0; k.d_cond = ps->cam.fx * ps->cam.baseline / ps->prm.cond_depth;
  k.k = std::sqrt(ps->prm.huber_k2); k.k2 = ps->prm.huber_k2;
  k.lambda0 = ps->prm.lambda0; k.lambda_max = ps->prm.lambda_max; k.abs_tol = ps->prm.abs_tol; k.rel_tol = ps->prm.rel_tol;
  k.inlier_px = ps->prm.inlier_px; k.max_iterations = ps->prm.max_iterations;
  return k;
}
extern "C" int sship_pose_create(int max_obs, int max_pairs, sship_pose** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "pose_create: null argument");
  *out = nullptr;
  if (max_obs < 1 || max_obs > kPoseMaxObs) return fail(SSHIP_ERR_INVALID, "pose_create: max_obs must be in [1, 2048]");
  if (max_pairs < 1 || max_pairs > kPoseMaxPairs) return fail(SSHIP_ERR_INVALID, "pose_create: max_pairs must be in [1, 65535]");
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_pose, void (*)(sship_pose*)> ps(new sship_pose(), sship_pose_destroy);
  ps->max_obs = max_obs; ps->max_pairs = max_pairs;
  const ObsStage st = pose_stage(max_obs);
  SSHIP_HIP_CHECK(ps->one.create(st.in_bytes, st.out_bytes));
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&ps->stream, hipStreamDefault));
  *out = ps.release();
  return SSHIP_OK;
}
extern "C" void sship_pose_destroy(sship_pose* ps) { destroy_handle(ps); }
extern "C" int sship_pose_set_camera(sship_pose* ps, double fx, double fy, double cx, double cy, double baseline) {
  return camera_set(ps ? &ps->cam : nullptr, "pose_set_camera", fx, fy, cx, cy, baseline);
}
extern "C" int sship_pose_get_camera(const sship_pose* ps, double* fx, double* fy, double* cx, double* cy, double* baseline) {
  return camera_get(ps ? &ps->cam : nullptr, "pose_get_camera", fx, fy, cx, cy, baseline);
}
extern "C" int sship_pose_set_params(sship_pose* ps, const sship_pose_params* p) {
  if (!ps || !p) return fail(SSHIP_ERR_INVALID, "pose_set_params: null argument");
  const double all[9] = {p->sigma_px, p->sigma_d0, p->cond_depth, p->huber_k2, p->lambda0, p->lambda_max, p->abs_tol, p->rel_tol, p->inlier_px};
  for (double v : all)
    if (std::isnan(v)) return fail(SSHIP_ERR_INVALID, "pose_set_params: a parameter is NaN");
  if (!(p->sigma_px > 0.0) || !(p->sigma_d0 > 0.0) || !(p->cond_depth > 0.0) || !(p->huber_k2 > 0.0) || std::isinf(p->sigma_px) ||
      std::isinf(p->sigma_d0) || std::isinf(p->cond_depth) || std::isinf(p->huber_k2))
    return fail(SSHIP_ERR_INVALID, "pose_set_params: sigma_px, sigma_d0, cond_depth and huber_k2 must be finite and > 0");
  if (int rc = check_lambda("pose_set_params", p->lambda0, p->lambda_max)) return rc;
  if (p->abs_tol < 0.0 || p->rel_tol < 0.0 || p->inlier_px < 0.0) return fail(SSHIP_ERR_INVALID, "pose_set_params: a tolerance or inlier_px is negative");
  if (int rc = check_max_iterations("pose_set_params", p->max_iterations)) return rc;
  ps->prm = *p;
  return SSHIP_OK;
}
extern "C" int sship_pose_get_params(const sship_pose* ps, sship_pose_params* p) {
  if (!ps || !p) return fail(SSHIP_ERR_INVALID, "pose_get_params: null argument");
  *p = ps->prm;
  return SSHIP_OK;
}
static hipError_t pose_run(const sship_pose* ps, const sship_pose::Last& l, hipStream_t s) {
  launch_pose_solve(l.points, l.meas, l.valid, l.pose0, ps->max_obs, l.items, pose_constants(ps), l.pose, l.stats, l.cost, l.inlier, s);
  return hipGetLastError();
}
static int pose_launch(sship_pose* ps, const float* points, const float* meas, const uint8_t* valid, const double* pose0, int pairs, double* pose,
                       int32_t* stats, double* cost, uint8_t* inlier, hipStream_t s) {
  ps->last = {points, meas, valid, pose0, pairs, pose, stats, cost, inlier};
  SSHIP_HIP_CHECK(pose_run(ps, ps->last, s));
  return SSHIP_OK;
}
extern "C" int sship_pose_solve_batch_device(sship_pose* ps, const float* points, const float* meas, const uint8_t* valid, const double* pose0,
                                             int pairs, double* pose, int32_t* stats, double* cost, uint8_t* inlier, void* stream) {
  if (!ps || !points || !meas || !valid || !pose || !stats || !cost) return fail(SSHIP_ERR_INVALID, "pose_solve_batch_device: null argument");
  if (pairs < 1 || pairs > ps->max_pairs) return fail(SSHIP_ERR_INVALID, "pose_solve_batch_device: pairs must be in [1, max_pairs]");
  if (!ps->cam.set) return fail(SSHIP_ERR_INVALID, "pose_solve_batch_device: set the camera first (sship_pose_set_camera)");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  if (int rc = pose_launch(ps, points, meas, valid, pose0, pairs, pose, stats, cost, inlier, s)) return rc;
  g_timer.mark("pose_solve", s);
  return SSHIP_OK;
}
extern "C" int sship_pose_solve_host(sship_pose* ps, const float* points, const float* meas, const uint8_t* valid, int n_obs, const double* pose0,
                                     double* pose_out, int32_t* stats_out, double* cost_out, uint8_t* inlier_out) {
  if (!ps || !pose_out || !stats_out || !cost_out) return fail(SSHIP_ERR_INVALID, "pose_solve_host: null argument");
  if (n_obs < 0 || n_obs > ps->max_obs) return fail(SSHIP_ERR_INVALID, "pose_solve_host: n_obs must be in [0, max_obs]");
  if (n_obs > 0 && (!points || !meas)) return fail(SSHIP_ERR_INVALID, "pose_solve_host: null argument");
  if (!ps->cam.set) return fail(SSHIP_ERR_INVALID, "pose_solve_host: set the camera first (sship_pose_set_camera)");
  bind_thread();
  hipStream_t s = ps->stream;
  const StageArena& a = ps->one;
  const ObsStage st = pose_stage(ps->max_obs);
  obs_pack(a.host<char>(0), st, points, meas, valid, n_obs, pose0);
  SSHIP_HIP_CHECK(a.upload(0, st.in_bytes, s));
  if (int rc = pose_launch(ps, a.dev<float>(st.points), a.dev<float>(st.meas), a.dev<uint8_t>(st.valid), pose0 ? a.dev<double>(st.pose0) : nullptr, 1,
                           a.dev<double>(a.out + st.pose), a.dev<int32_t>(a.out + st.stats), a.dev<double>(a.out + st.cost),
                           a.dev<uint8_t>(a.out + st.inlier), s))
    return rc;
  SSHIP_HIP_CHECK(a.download(a.out, st.out_bytes, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  obs_unpack(a.host<char>(a.out), st, n_obs, pose_out, stats_out, cost_out, inlier_out);
  return SSHIP_OK;
}
extern "C" int sship_pose_obs_from_matches_batch_device(const sship_pose* ps, const float* stereo0, const uint8_t* hd0, const float* stereo1,
                                                        const uint8_t* hd1, const int32_t* matches0, const int* n0, const int* n1, int n_stride,
                                                        int pairs, float* points, float* meas, uint8_t* valid, void* stream) {
  if (!ps || !stereo0 || !hd0 || !stereo1 || !hd1 || !matches0 || !n0 || !n1 || !points || !meas || !valid)
    return fail(SSHIP_ERR_INVALID, "pose_obs_from_matches_batch_device: null argument");
  if (pairs < 1 || pairs > ps->max_pairs) return fail(SSHIP_ERR_INVALID, "pose_obs_from_matches_batch_device: pairs must be in [1, max_pairs]");
  if (n_stride < 1) return fail(SSHIP_ERR_INVALID, "pose_obs_from_matches_batch_device: n_stride must be >= 1");
  if (!ps->cam.set) return fail(SSHIP_ERR_INVALID, "pose_obs_from_matches_batch_device: set the camera first (sship_pose_set_camera)");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_pose_gather(stereo0, hd0, stereo1, hd1, matches0, n0, n1, n_stride, ps->max_obs, pairs, pose_constants(ps), points, meas, valid, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("pose_gather", s);
  return SSHIP_OK;
}
// Measurement hook (include/sship.h): the last solve call's launch re-run `iters` times on the handle's stream.
extern "C" int sship_pose_bench(sship_pose* ps, int iters, float* avg_ms) { return bench_last(ps, iters, avg_ms, "pose_bench", "solve", pose_run); }

// ====================================================================================================
// RANSAC pose seed and inlier gate (include/sship.h "RANSAC pose seed and inlier gate"; csrc/ransac_kernels.hip)
// ====================================================================================================
struct sship_ransac {
  int max_obs = 0, max_pairs = 0;
  StereoCamera cam;
  sship_ransac_params prm{3.0, 1.0, 1e-8, 1u, 512};
  hipStream_t stream = nullptr;
  DevBuf workspace;                                            // [max_pairs, splits] records between the two launches
  StageArena one;                                              // sship_ransac_solve_host: one staged pair and its results (ransac_stage)
  // the last solve call's arguments (sship_ransac_bench re-runs its launches; the caller keeps a batch call's buffers alive until then)
  struct Last { const float* points = nullptr; const float* meas = nullptr; const uint8_t* valid = nullptr; int items = 0;
                double* pose = nullptr; int32_t* stats = nullptr; double* cost = nullptr; uint8_t* inlier = nullptr; } last;
};
static RansacK ransac_constants(const sship_ransac* rs) {
  RansacK k;
  k.fx = rs->cam.fx; k.fy = rs->cam.fy; k.cx = rs->cam.cx; k.cy = rs->cam.cy; k.baseline = rs->cam.baseline;
  k.thr2 = rs->prm.inlier_px * rs->prm.inlier_px; k.min_disparity = rs->prm.min_disparity; k.min_area2 = rs->prm.min_area2;
  k.seed = rs->prm.seed; k.num_hypotheses = rs->prm.num_hypotheses;
  return k;
}
extern "C" int sship_ransac_create(int max_obs, int max_pairs, sship_ransac** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "ransac_create: null argument");
  *out = nullptr;
  if (max_obs < 1 || max_obs > kPoseMaxObs) return fail(SSHIP_ERR_INVALID, "ransac_create: max_obs must be in [1, 2048]");
  if (max_pairs < 1 || max_pairs > kPoseMaxPairs) return fail(SSHIP_ERR_INVALID, "ransac_create: max_pairs must be in [1, 65535]");
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_ransac, void (*)(sship_ransac*)> rs(new sship_ransac(), sship_ransac_destroy);
  rs->max_obs = max_obs; rs->max_pairs = max_pairs;
  const ObsStage st = ransac_stage(max_obs);
  SSHIP_HIP_CHECK(rs->workspace.ensure(ransac_workspace_bytes(max_pairs, rs->prm.num_hypotheses)));
  SSHIP_HIP_CHECK(rs->one.create(st.in_bytes, st.out_bytes));
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&rs->stream, hipStreamDefault));
  *out = rs.release();
  return SSHIP_OK;
}
extern "C" void sship_ransac_destroy(sship_ransac* rs) { destroy_handle(rs); }
extern "C" int sship_ransac_set_camera(sship_ransac* rs, double fx, double fy, double cx, double cy, double baseline) {
  return camera_set(rs ? &rs->cam : nullptr, "ransac_set_camera", fx, fy, cx, cy, baseline);
}
extern "C" int sship_ransac_get_camera(const sship_ransac* rs, double* fx, double* fy, double* cx, double* cy, double* baseline) {
  return camera_get(rs ? &rs->cam : nullptr, "ransac_get_camera", fx, fy, cx, cy, baseline);
}
extern "C" int sship_ransac_set_params(sship_ransac* rs, const sship_ransac_params* p) {
  if (!rs || !p) return fail(SSHIP_ERR_INVALID, "ransac_set_params: null argument");
  const double all[3] = {p->inlier_px, p->min_disparity, p->min_area2};
  for (double v : all)
    if (!std::isfinite(v)) return fail(SSHIP_ERR_INVALID, "ransac_set_params: a parameter is NaN or infinite");
  if (p->inlier_px < 0.0 || p->min_disparity < 0.0 || p->min_area2 < 0.0)
    return fail(SSHIP_ERR_INVALID, "ransac_set_params: inlier_px, min_disparity or min_area2 is negative");
  if (p->num_hypotheses < 1 || p->num_hypotheses > 65536) return fail(SSHIP_ERR_INVALID, "ransac_set_params: num_hypotheses must be in [1, 65536]");
  const size_t need = ransac_workspace_bytes(rs->max_pairs, p->num_hypotheses);
  if (need > rs->workspace.bytes) {   // the old workspace may still be read by a launch in flight
    bind_thread();
    SSHIP_HIP_CHECK(hipDeviceSynchronize());
    SSHIP_HIP_CHECK(rs->workspace.ensure(need));
  }
  rs->prm = *p;
  return SSHIP_OK;
}
extern "C" int sship_ransac_get_params(const sship_ransac* rs, sship_ransac_params* p) {
  if (!rs || !p) return fail(SSHIP_ERR_INVALID, "ransac_get_params: null argument");
  *p = rs->prm;
  return SSHIP_OK;
}
static hipError_t ransac_run(const sship_ransac* rs, const sship_ransac::Last& l, hipStream_t s) {
  launch_ransac_solve(l.points, l.meas, l.valid, rs->max_obs, l.items, ransac_constants(rs), rs->workspace.p, l.pose, l.stats, l.cost, l.inlier, s);
  return hipGetLastError();
}
static int ransac_launch(sship_ransac* rs, const float* points, const float* meas, const uint8_t* valid, int pairs, double* pose, int32_t* stats,
                         double* cost, uint8_t* inlier, hipStream_t s) {
  rs->last = {points, meas, valid, pairs, pose, stats, cost, inlier};
  SSHIP_HIP_CHECK(ransac_run(rs, rs->last, s));
  return SSHIP_OK;
}
extern "C" int sship_ransac_solve_batch_device(sship_ransac* rs, const float* points, const float* meas, const uint8_t* valid, int pairs,
                                               double* pose, int32_t* stats, double* cost, uint8_t* inlier, void* stream) {
  if (!rs || !points || !meas || !valid || !pose || !stats || !cost) return fail(SSHIP_ERR_INVALID, "ransac_solve_batch_device: null argument");
  if (pairs < 1 || pairs > rs->max_pairs) return fail(SSHIP_ERR_INVALID, "ransac_solve_batch_device: pairs must be in [1, max_pairs]");
  if (!rs->cam.set) return fail(SSHIP_ERR_INVALID, "ransac_solve_batch_device: set the camera first (sship_ransac_set_camera)");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  if (int rc = ransac_launch(rs, points, meas, valid, pairs, pose, stats, cost, inlier, s)) return rc;
  g_timer.mark("ransac_solve", s);
  return SSHIP_OK;
}
extern "C" int sship_ransac_solve_host(sship_ransac* rs, const float* points, const float* meas, const uint8_t* valid, int n_obs, double* pose_out,
                                       int32_t* stats_out, double* cost_out, uint8_t* inlier_out) {
  if (!rs || !pose_out || !stats_out || !cost_out) return fail(SSHIP_ERR_INVALID, "ransac_solve_host: null argument");
  if (n_obs < 0 || n_obs > rs->max_obs) return fail(SSHIP_ERR_INVALID, "ransac_solve_host: n_obs must be in [0, max_obs]");
  if (n_obs > 0 && (!points || !meas)) return fail(SSHIP_ERR_INVALID, "ransac_solve_host: null argument");
  if (!rs->cam.set) return fail(SSHIP_ERR_INVALID, "ransac_solve_host: set the camera first (sship_ransac_set_camera)");
  bind_thread();
  hipStream_t s = rs->stream;
  const StageArena& a = rs->one;
  const ObsStage st = ransac_stage(rs->max_obs);
  obs_pack(a.host<char>(0), st, points, meas, valid, n_obs, nullptr);
  SSHIP_HIP_CHECK(a.upload(0, st.in_bytes, s));
  if (int rc = ransac_launch(rs, a.dev<float>(st.points), a.dev<float>(st.meas), a.dev<uint8_t>(st.valid), 1, a.dev<double>(a.out + st.pose),
                             a.dev<int32_t>(a.out + st.stats), a.dev<double>(a.out + st.cost), a.dev<uint8_t>(a.out + st.inlier), s))
    return rc;
  SSHIP_HIP_CHECK(a.download(a.out, st.out_bytes, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  obs_unpack(a.host<char>(a.out), st, n_obs, pose_out, stats_out, cost_out, inlier_out);
  return SSHIP_OK;
}
// Measurement hook (include/sship.h): the last solve call's two launches re-run `iters` times on the handle's stream.
extern "C" int sship_ransac_bench(sship_ransac* rs, int iters, float* avg_ms) { return bench_last(rs, iters, avg_ms, "ransac_bench", "solve", ransac_run); }

// ====================================================================================================
// Window smoother: sliding-window stereo bundle adjustment (include/sship.h "Window smoother"; csrc/ba_kernels.hip)
// ====================================================================================================
constexpr int kBaMaxWindows = 65535;
struct sship_ba {
  int K = 0, N = 0, L = 0, max_windows = 0;
  StereoCamera cam;
  sship_ba_params prm{1.0, 9.0, 1e-5, 1e5, 1e-3, 1e-3, 20};
  hipStream_t stream = nullptr;
  DevBuf workspace;
  StageArena one;   // sship_ba_solve_host: one staged window and its results (ba_stage)
  struct Last { const float* meas = nullptr; const int32_t* track = nullptr; const int32_t* n_kf = nullptr; const double* pose0 = nullptr; int items = 0;
                double* pose = nullptr; int32_t* stats = nullptr; double* cost = nullptr; float* landmarks = nullptr; } last;
};
static BaK ba_constants(const sship_ba* ba) {
  BaK k;
  k.fx = ba->cam.fx; k.fy = ba->cam.fy; k.cx = ba->cam.cx; k.cy = ba->cam.cy; k.baseline = ba->cam.baseline;
  k.inv_sigma = 1.0 / ba->prm.sigma_px; k.k = std::sqrt(ba->prm.huber_k2); k.k2 = ba->prm.huber_k2;
  k.lambda0 = ba->prm.lambda0; k.lambda_max = ba->prm.lambda_max; k.abs_tol = ba->prm.abs_tol; k.rel_tol = ba->prm.rel_tol;
  k.max_iterations = ba->prm.max_iterations;
  return k;
}
extern "C" int sship_ba_create(int max_keyframes, int max_obs, int max_landmarks, int max_windows, sship_ba** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "ba_create: null argument");
  *out = nullptr;
  if (max_keyframes < 2 || max_keyframes > kBaMaxKf) return fail(SSHIP_ERR_INVALID, "ba_create: max_keyframes must be in [2, 16]");
  if (max_obs < 1 || max_obs > kBaMaxObs) return fail(SSHIP_ERR_INVALID, "ba_create: max_obs must be in [1, 2048]");
  if (max_landmarks < 1 || max_landmarks > kBaMaxLandmarks) return fail(SSHIP_ERR_INVALID, "ba_create: max_landmarks must be in [1, 32768]");
  if (max_windows < 1 || max_windows > kBaMaxWindows) return fail(SSHIP_ERR_INVALID, "ba_create: max_windows must be in [1, 65535]");
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_ba, void (*)(sship_ba*)> ba(new sship_ba(), sship_ba_destroy);
  ba->K = max_keyframes; ba->N = max_obs; ba->L = max_landmarks; ba->max_windows = max_windows;
  const BaStage st = ba_stage(max_keyframes, max_obs, max_landmarks);
  SSHIP_HIP_CHECK(ba->workspace.ensure(ba_workspace_bytes(max_keyframes, max_obs, max_landmarks) * (size_t)std::min(max_windows, kBaResident)));
  SSHIP_HIP_CHECK(ba->one.create(st.in_bytes, st.out_bytes));
  SSHIP_HIP_CHECK(ba_solve_prepare());
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&ba->stream, hipStreamDefault));
  *out = ba.release();
  return SSHIP_OK;
}
extern "C" void sship_ba_destroy(sship_ba* ba) { destroy_handle(ba); }
extern "C" int sship_ba_set_camera(sship_ba* ba, double fx, double fy, double cx, double cy, double baseline) {
  return camera_set(ba ? &ba->cam : nullptr, "ba_set_camera", fx, fy, cx, cy, baseline);
}
extern "C" int sship_ba_get_camera(const sship_ba* ba, double* fx, double* fy, double* cx, double* cy, double* baseline) {
  return camera_get(ba ? &ba->cam : nullptr, "ba_get_camera", fx, fy, cx, cy, baseline);
}
extern "C" int sship_ba_set_params(sship_ba* ba, const sship_ba_params* p) {
  if (!ba || !p) return fail(SSHIP_ERR_INVALID, "ba_set_params: null argument");
  const double all[6] = {p->sigma_px, p->huber_k2, p->lambda0, p->lambda_max, p->abs_tol, p->rel_tol};
  for (double v : all)
    if (std::isnan(v)) return fail(SSHIP_ERR_INVALID, "ba_set_params: a parameter is NaN");
  if (!(p->sigma_px > 0.0) || !(p->huber_k2 > 0.0) || std::isinf(p->sigma_px) || std::isinf(p->huber_k2))
    return fail(SSHIP_ERR_INVALID, "ba_set_params: sigma_px and huber_k2 must be finite and > 0");
  if (int rc = check_lambda("ba_set_params", p->lambda0, p->lambda_max)) return rc;
  if (p->abs_tol < 0.0 || p->rel_tol < 0.0) return fail(SSHIP_ERR_INVALID, "ba_set_params: a tolerance is negative");
  if (int rc = check_max_iterations("ba_set_params", p->max_iterations)) return rc;
  ba->prm = *p;
  return SSHIP_OK;
}
extern "C" int sship_ba_get_params(const sship_ba* ba, sship_ba_params* p) {
  if (!ba || !p) return fail(SSHIP_ERR_INVALID, "ba_get_params: null argument");
  *p = ba->prm;
  return SSHIP_OK;
}
static hipError_t ba_run(const sship_ba* ba, const sship_ba::Last& l, hipStream_t s) {
  launch_ba_solve(l.meas, l.track, l.n_kf, l.pose0, ba->K, ba->N, ba->L, l.items, ba_constants(ba), ba->workspace.p, l.pose, l.stats, l.cost, l.landmarks, s);
  return hipGetLastError();
}
static int ba_launch(sship_ba* ba, const float* meas, const int32_t* track, const int32_t* n_kf, const double* pose0, int windows, double* pose,
                     int32_t* stats, double* cost, float* landmarks, hipStream_t s) {
  ba->last = {meas, track, n_kf, pose0, windows, pose, stats, cost, landmarks};
  SSHIP_HIP_CHECK(ba_run(ba, ba->last, s));
  return SSHIP_OK;
}
extern "C" int sship_ba_solve_batch_device(sship_ba* ba, const float* meas, const int32_t* track, const int32_t* n_kf, const double* pose0,
                                           int windows, double* pose, int32_t* stats, double* cost, float* landmarks, void* stream) {
  if (!ba || !meas || !track || !pose0 || !pose || !stats || !cost) return fail(SSHIP_ERR_INVALID, "ba_solve_batch_device: null argument");
  if (windows < 1 || windows > ba->max_windows) return fail(SSHIP_ERR_INVALID, "ba_solve_batch_device: windows must be in [1, max_windows]");
  if (!ba->cam.set) return fail(SSHIP_ERR_INVALID, "ba_solve_batch_device: set the camera first (sship_ba_set_camera)");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  if (int rc = ba_launch(ba, meas, track, n_kf, pose0, windows, pose, stats, cost, landmarks, s)) return rc;
  g_timer.mark("ba_solve", s);
  return SSHIP_OK;
}
extern "C" int sship_ba_solve_host(sship_ba* ba, const float* meas, const int32_t* track, int n_kf, const double* pose0, double* pose_out,
                                   int32_t* stats_out, double* cost_out, float* landmarks_out) {
  if (!ba || !meas || !track || !pose0 || !pose_out || !stats_out || !cost_out) return fail(SSHIP_ERR_INVALID, "ba_solve_host: null argument");
  if (n_kf < 0 || n_kf > ba->K) return fail(SSHIP_ERR_INVALID, "ba_solve_host: n_kf must be in [0, max_keyframes]");
  if (!ba->cam.set) return fail(SSHIP_ERR_INVALID, "ba_solve_host: set the camera first (sship_ba_set_camera)");
  bind_thread();
  hipStream_t s = ba->stream;
  const StageArena& a = ba->one;
  const BaStage st = ba_stage(ba->K, ba->N, ba->L);
  ba_pack(a.host<char>(0), st, meas, track, n_kf, pose0);
  SSHIP_HIP_CHECK(a.upload(0, st.in_bytes, s));
  if (int rc = ba_launch(ba, a.dev<float>(st.meas), a.dev<int32_t>(st.track), a.dev<int32_t>(st.n_kf), a.dev<double>(st.pose0), 1,
                         a.dev<double>(a.out + st.pose), a.dev<int32_t>(a.out + st.stats), a.dev<double>(a.out + st.cost),
                         a.dev<float>(a.out + st.landmarks), s))
    return rc;
  SSHIP_HIP_CHECK(a.download(a.out, landmarks_out ? st.out_bytes : st.landmarks, s));   // the landmarks are the last slot: not fetched unless asked for
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  ba_unpack(a.host<char>(a.out), st, pose_out, stats_out, cost_out, landmarks_out);
  return SSHIP_OK;
}
extern "C" int sship_ba_tracks_from_matches_batch_device(const sship_ba* ba, const uint8_t* has_depth, const int32_t* matches, const int32_t* n,
                                                         const int32_t* n_kf, int windows, int32_t* track, void* stream) {
  if (!ba || !has_depth || !matches || !n || !track) return fail(SSHIP_ERR_INVALID, "ba_tracks_from_matches_batch_device: null argument");
  if (windows < 1 || windows > ba->max_windows) return fail(SSHIP_ERR_INVALID, "ba_tracks_from_matches_batch_device: windows must be in [1, max_windows]");
  if ((long long)ba->L < (long long)ba->K * ba->N)
    return fail(SSHIP_ERR_INVALID, "ba_tracks_from_matches_batch_device: needs max_landmarks >= max_keyframes * max_obs");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_ba_tracks(has_depth, matches, n, n_kf, ba->K, ba->N, windows, track, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("ba_tracks", s);
  return SSHIP_OK;
}
// Measurement hook (include/sship.h): the last solve call's launch re-run `iters` times on the handle's stream.
extern "C" int sship_ba_bench(sship_ba* ba, int iters, float* avg_ms) { return bench_last(ba, iters, avg_ms, "ba_bench", "solve", ba_run); }

// ====================================================================================================
// Pose graph: batched pose-graph optimiser (include/sship.h "Pose graph"; csrc/pg_kernels.hip)
// ====================================================================================================
constexpr int kPgMaxGraphs = 65535;
struct sship_pg {
  int N = 0, L = 0, max_graphs = 0;
  sship_pg_params prm{0.02, 0.05, 1e-5, 1e5, 1e-5, 1e-5, 1e6, 100};
  hipStream_t stream = nullptr;
  DevBuf workspace;
  StageArena one;   // sship_pg_solve_host: one staged graph and its results (pg_stage)
  struct Last { const int32_t* n_nodes = nullptr; const double* pose0 = nullptr; const double* odom_z = nullptr; const double* odom_sigma = nullptr;
                const int32_t* loop_ij = nullptr; const double* loop_z = nullptr; const double* loop_sigma = nullptr; const double* loop_k2 = nullptr;
                const uint8_t* loop_enable = nullptr; int items = 0;
                double* pose = nullptr; int32_t* stats = nullptr; double* cost = nullptr; double* chi2 = nullptr; } last;
};
static PgK pg_constants(const sship_pg* pg) {
  PgK k;
  k.odom_sigma_rot = pg->prm.odom_sigma_rot; k.odom_sigma_trans = pg->prm.odom_sigma_trans;
  k.lambda0 = pg->prm.lambda0; k.lambda_max = pg->prm.lambda_max; k.abs_tol = pg->prm.abs_tol; k.rel_tol = pg->prm.rel_tol;
  k.max_translation = pg->prm.max_translation; k.max_iterations = pg->prm.max_iterations;
  return k;
}
extern "C" int sship_pg_create(int max_nodes, int max_loops, int max_graphs, sship_pg** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "pg_create: null argument");
  *out = nullptr;
  if (max_nodes < 2 || max_nodes > kPgMaxNodes) return fail(SSHIP_ERR_INVALID, "pg_create: max_nodes must be in [2, 4096]");
  if (max_loops < 0 || max_loops > kPgMaxLoops) return fail(SSHIP_ERR_INVALID, "pg_create: max_loops must be in [0, 128]");
  if (max_graphs < 1 || max_graphs > kPgMaxGraphs) return fail(SSHIP_ERR_INVALID, "pg_create: max_graphs must be in [1, 65535]");
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_pg, void (*)(sship_pg*)> pg(new sship_pg(), sship_pg_destroy);
  pg->N = max_nodes; pg->L = max_loops; pg->max_graphs = max_graphs;
  const PgStage st = pg_stage(max_nodes, max_loops);
  SSHIP_HIP_CHECK(pg->workspace.ensure(pg_workspace_bytes(max_nodes, max_loops) * (size_t)std::min(max_graphs, kPgResident)));
  SSHIP_HIP_CHECK(pg->one.create(st.in_bytes, st.out_bytes));
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&pg->stream, hipStreamDefault));
  *out = pg.release();
  return SSHIP_OK;
}
extern "C" size_t sship_pg_workspace_slice_bytes(int max_nodes, int max_loops) {
  if (max_nodes < 2 || max_nodes > kPgMaxNodes || max_loops < 0 || max_loops > kPgMaxLoops) return 0;
  return pg_workspace_bytes(max_nodes, max_loops);
}
extern "C" void sship_pg_destroy(sship_pg* pg) { destroy_handle(pg); }
extern "C" int sship_pg_set_params(sship_pg* pg, const sship_pg_params* p) {
  if (!pg || !p) return fail(SSHIP_ERR_INVALID, "pg_set_params: null argument");
  const double all[7] = {p->odom_sigma_rot, p->odom_sigma_trans, p->lambda0, p->lambda_max, p->abs_tol, p->rel_tol, p->max_translation};
  for (double v : all)
    if (std::isnan(v)) return fail(SSHIP_ERR_INVALID, "pg_set_params: a parameter is NaN");
  if (!(p->odom_sigma_rot > 0.0) || !(p->odom_sigma_trans > 0.0) || std::isinf(p->odom_sigma_rot) || std::isinf(p->odom_sigma_trans))
    return fail(SSHIP_ERR_INVALID, "pg_set_params: odom_sigma_rot and odom_sigma_trans must be finite and > 0");
  if (int rc = check_lambda("pg_set_params", p->lambda0, p->lambda_max)) return rc;
  if (p->abs_tol < 0.0 || p->rel_tol < 0.0) return fail(SSHIP_ERR_INVALID, "pg_set_params: a tolerance is negative");
  if (!(p->max_translation > 0.0) || std::isinf(p->max_translation))
    return fail(SSHIP_ERR_INVALID, "pg_set_params: max_translation must be finite and > 0");
  if (int rc = check_max_iterations("pg_set_params", p->max_iterations)) return rc;
  pg->prm = *p;
  return SSHIP_OK;
}
extern "C" int sship_pg_get_params(const sship_pg* pg, sship_pg_params* p) {
  if (!pg || !p) return fail(SSHIP_ERR_INVALID, "pg_get_params: null argument");
  *p = pg->prm;
  return SSHIP_OK;
}
static hipError_t pg_run(const sship_pg* pg, const sship_pg::Last& l, hipStream_t s) {
  launch_pg_solve(l.n_nodes, l.pose0, l.odom_z, l.odom_sigma, l.loop_ij, l.loop_z, l.loop_sigma, l.loop_k2, l.loop_enable, pg->N, pg->L, l.items,
                  pg_constants(pg), pg->workspace.p, l.pose, l.stats, l.cost, l.chi2, s);
  return hipGetLastError();
}
static int pg_launch(sship_pg* pg, const int32_t* n_nodes, const double* pose0, const double* odom_z, const double* odom_sigma,
                     const int32_t* loop_ij, const double* loop_z, const double* loop_sigma, const double* loop_k2, const uint8_t* loop_enable,
                     int graphs, double* pose, int32_t* stats, double* cost, double* chi2, hipStream_t s) {
  pg->last = {n_nodes, pose0, odom_z, odom_sigma, loop_ij, loop_z, loop_sigma, loop_k2, loop_enable, graphs, pose, stats, cost, chi2};
  SSHIP_HIP_CHECK(pg_run(pg, pg->last, s));
  return SSHIP_OK;
}
extern "C" int sship_pg_solve_batch_device(sship_pg* pg, const int32_t* n_nodes, const double* pose0, const double* odom_z,
                                           const double* odom_sigma, const int32_t* loop_ij, const double* loop_z, const double* loop_sigma,
                                           const double* loop_k2, const uint8_t* loop_enable, int graphs, double* pose, int32_t* stats,
                                           double* cost, double* loop_chi2, void* stream) {
  if (!pg || !pose0 || !odom_z || !pose || !stats || !cost) return fail(SSHIP_ERR_INVALID, "pg_solve_batch_device: null argument");
  const bool all_loops = loop_ij && loop_z && loop_sigma && loop_k2, no_loops = !loop_ij && !loop_z && !loop_sigma && !loop_k2 && !loop_enable;
  if (!(all_loops || (no_loops && pg->L == 0)))
    return fail(SSHIP_ERR_INVALID, "pg_solve_batch_device: the loop arrays may be NULL only when max_loops == 0, and then all of them");
  if (graphs < 1 || graphs > pg->max_graphs) return fail(SSHIP_ERR_INVALID, "pg_solve_batch_device: graphs must be in [1, max_graphs]");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  if (int rc = pg_launch(pg, n_nodes, pose0, odom_z, odom_sigma, loop_ij, loop_z, loop_sigma, loop_k2, loop_enable, graphs, pose, stats, cost,
                         loop_chi2, s))
    return rc;
  g_timer.mark("pg_solve", s);
  return SSHIP_OK;
}
extern "C" int sship_pg_solve_host(sship_pg* pg, int n_nodes, const double* pose0, const double* odom_z, const double* odom_sigma, int n_loops,
                                   const int32_t* loop_ij, const double* loop_z, const double* loop_sigma, const double* loop_k2,
                                   double* pose_out, int32_t* stats_out, double* cost_out, double* loop_chi2_out) {
  if (!pg || !stats_out || !cost_out) return fail(SSHIP_ERR_INVALID, "pg_solve_host: null argument");
  if (n_nodes < 0 || n_nodes > pg->N) return fail(SSHIP_ERR_INVALID, "pg_solve_host: n_nodes must be in [0, max_nodes]");
  if (n_loops < 0 || n_loops > pg->L) return fail(SSHIP_ERR_INVALID, "pg_solve_host: n_loops must be in [0, max_loops]");
  if (n_nodes > 0 && (!pose0 || !pose_out)) return fail(SSHIP_ERR_INVALID, "pg_solve_host: null argument");
  if (n_nodes > 1 && !odom_z) return fail(SSHIP_ERR_INVALID, "pg_solve_host: null argument");
  if (n_loops > 0 && (!loop_ij || !loop_z || !loop_sigma || !loop_k2)) return fail(SSHIP_ERR_INVALID, "pg_solve_host: null argument");
  bind_thread();
  hipStream_t s = pg->stream;
  const StageArena& a = pg->one;
  const PgStage st = pg_stage(pg->N, pg->L);
  const bool loops = pg->L > 0;   // a handle without loops passes null loop arrays
  pg_pack(a.host<char>(0), st, n_nodes, pose0, odom_z, odom_sigma, n_loops, loop_ij, loop_z, loop_sigma, loop_k2);
  SSHIP_HIP_CHECK(a.upload(0, st.in_bytes, s));
  if (int rc = pg_launch(pg, a.dev<int32_t>(st.nn), a.dev<double>(st.pose0), a.dev<double>(st.oz), odom_sigma ? a.dev<double>(st.osg) : nullptr,
                         loops ? a.dev<int32_t>(st.lij) : nullptr, loops ? a.dev<double>(st.lz) : nullptr, loops ? a.dev<double>(st.lsg) : nullptr,
                         loops ? a.dev<double>(st.lk2) : nullptr, loops ? a.dev<uint8_t>(st.len) : nullptr, 1, a.dev<double>(a.out + st.pose),
                         a.dev<int32_t>(a.out + st.stats), a.dev<double>(a.out + st.cost), a.dev<double>(a.out + st.chi2), s))
    return rc;
  SSHIP_HIP_CHECK(a.download(a.out, st.out_bytes, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  pg_unpack(a.host<char>(a.out), st, n_nodes, n_loops, pose_out, stats_out, cost_out, loop_chi2_out);
  return SSHIP_OK;
}
extern "C" int sship_pg_odometry_from_poses_batch_device(const sship_pg* pg, const double* pose, int graphs, double* odom_z, void* stream) {
  if (!pg || !pose || !odom_z) return fail(SSHIP_ERR_INVALID, "pg_odometry_from_poses_batch_device: null argument");
  if (graphs < 1 || graphs > pg->max_graphs) return fail(SSHIP_ERR_INVALID, "pg_odometry_from_poses_batch_device: graphs must be in [1, max_graphs]");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_pg_odometry(pose, pg->N, graphs, odom_z, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("pg_odometry", s);
  return SSHIP_OK;
}
extern "C" int sship_pg_loops_from_pose_batch_device(const sship_pg* pg, const int32_t* from, const int32_t* to, const double* pose,
                                                     const int32_t* stats, int graphs, int min_inliers, double noise_base, int32_t* loop_ij,
                                                     double* loop_z, double* loop_sigma, double* loop_k2, uint8_t* loop_enable, void* stream) {
  if (!pg || !from || !to || !pose || !stats || !loop_ij || !loop_z || !loop_sigma || !loop_k2 || !loop_enable)
    return fail(SSHIP_ERR_INVALID, "pg_loops_from_pose_batch_device: null argument");
  if (pg->L < 1) return fail(SSHIP_ERR_INVALID, "pg_loops_from_pose_batch_device: the handle has max_loops == 0");
  if (graphs < 1 || graphs > pg->max_graphs) return fail(SSHIP_ERR_INVALID, "pg_loops_from_pose_batch_device: graphs must be in [1, max_graphs]");
  if (min_inliers < 1) return fail(SSHIP_ERR_INVALID, "pg_loops_from_pose_batch_device: min_inliers must be >= 1");
  if (!std::isfinite(noise_base) || !(noise_base > 0.0)) return fail(SSHIP_ERR_INVALID, "pg_loops_from_pose_batch_device: noise_base must be finite and > 0");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_pg_loops(from, to, pose, stats, graphs * pg->L, min_inliers, noise_base, loop_ij, loop_z, loop_sigma, loop_k2, loop_enable, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("pg_loops", s);
  return SSHIP_OK;
}
// Measurement hook (include/sship.h): the last solve call's launch re-run `iters` times on the handle's stream.
extern "C" int sship_pg_bench(sship_pg* pg, int iters, float* avg_ms) { return bench_last(pg, iters, avg_ms, "pg_bench", "solve", pg_run); }

// ====================================================================================================
// rectification remap (sship_rect_*) and RGB-D association
// ====================================================================================================
struct sship_rect {
  int src_w = 0, src_h = 0, dst_w = 0, dst_h = 0, cameras = 0, tiles = 0;   // tiles per camera
  bool have[2] = {false, false};
  int n_staged[2] = {0, 0}, n_direct[2] = {0, 0};
  hipStream_t stream = nullptr;
  DevBuf table, tile_boxes;   // [cameras][dst_h * dst_w] RectEntry, [cameras][tiles] RectTile
  DevBuf src1, dst1;          // sship_rect_remap_host: one staged image and its result
  DevBuf bench_src, bench_dst;
  size_t px() const { return (size_t)dst_w * dst_h; }
};
static int rect_check_camera(const double* K, const double* D, int n_dist, const double* Pnew, const char* who) {
  if (!K || !Pnew) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (n_dist != 0 && n_dist != 4 && n_dist != 5 && n_dist != 8) return fail(SSHIP_ERR_INVALID, std::string(who) + ": n_dist must be 0, 4, 5 or 8");
  if (n_dist > 0 && !D) return fail(SSHIP_ERR_INVALID, std::string(who) + ": D is NULL with n_dist > 0");
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(K[i]) || !std::isfinite(Pnew[i])) return fail(SSHIP_ERR_INVALID, std::string(who) + ": K and Pnew must be finite");
  for (int i = 0; i < n_dist; ++i)
    if (!std::isfinite(D[i])) return fail(SSHIP_ERR_INVALID, std::string(who) + ": D must be finite");
  if (!(K[0] > 0.0) || !(K[4] > 0.0)) return fail(SSHIP_ERR_INVALID, std::string(who) + ": fx and fy of K must be > 0");
  return SSHIP_OK;
}
static bool rect_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= kRectMaxSize && h <= kRectMaxSize; }
extern "C" int sship_rect_build_maps(const double* K, const double* D, int n_dist, const double* R, const double* Pnew, int dst_w, int dst_h,
                                     float* map_x, float* map_y) {
  if (int rc = rect_check_camera(K, D, n_dist, Pnew, "rect_build_maps")) return rc;
  if (!map_x || !map_y) return fail(SSHIP_ERR_INVALID, "rect_build_maps: null argument");
  if (!rect_size_ok(dst_w, dst_h)) return fail(SSHIP_ERR_INVALID, "rect_build_maps: dst_w and dst_h must be in [1, 4096]");
  if (R)
    for (int i = 0; i < 9; ++i)
      if (!std::isfinite(R[i])) return fail(SSHIP_ERR_INVALID, "rect_build_maps: R must be finite");
  if (rect_build_maps(K, D, n_dist, R, Pnew, dst_w, dst_h, map_x, map_y)) return fail(SSHIP_ERR_INVALID, "rect_build_maps: Pnew * R is singular");
  return SSHIP_OK;
}
extern "C" int sship_rect_fixed_table(const float* map_x, const float* map_y, size_t count, int32_t* ix, int32_t* iy, uint16_t* frac) {
  if (!map_x || !map_y || !ix || !iy || !frac) return fail(SSHIP_ERR_INVALID, "rect_fixed_table: null argument");
  rect_fixed_table(map_x, map_y, count, ix, iy, frac);
  return SSHIP_OK;
}
extern "C" int sship_rect_create(int src_w, int src_h, int dst_w, int dst_h, int cameras, sship_rect** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "rect_create: null argument");
  *out = nullptr;
  if (!rect_size_ok(src_w, src_h)) return fail(SSHIP_ERR_INVALID, "rect_create: src_w and src_h must be in [1, 4096]");
  if (!rect_size_ok(dst_w, dst_h)) return fail(SSHIP_ERR_INVALID, "rect_create: dst_w and dst_h must be in [1, 4096]");
  if (cameras != 1 && cameras != 2) return fail(SSHIP_ERR_INVALID, "rect_create: cameras must be 1 or 2");
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_rect, void (*)(sship_rect*)> r(new sship_rect(), sship_rect_destroy);
  r->src_w = src_w; r->src_h = src_h; r->dst_w = dst_w; r->dst_h = dst_h; r->cameras = cameras;
  r->tiles = ((dst_w + kRectTileW - 1) / kRectTileW) * ((dst_h + kRectTileH - 1) / kRectTileH);
  SSHIP_HIP_CHECK(r->table.ensure(r->px() * cameras * sizeof(RectEntry)));
  SSHIP_HIP_CHECK(r->tile_boxes.ensure((size_t)r->tiles * cameras * sizeof(RectTile)));
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&r->stream, hipStreamDefault));
  *out = r.release();
  return SSHIP_OK;
}
extern "C" void sship_rect_destroy(sship_rect* rect) { destroy_handle(rect); }
extern "C" int sship_rect_set_maps(sship_rect* rect, int camera, const float* map_x, const float* map_y) {
  if (!rect || !map_x || !map_y) return fail(SSHIP_ERR_INVALID, "rect_set_maps: null argument");
  if (camera < 0 || camera >= rect->cameras) return fail(SSHIP_ERR_INVALID, "rect_set_maps: camera must be in [0, cameras)");
  bind_thread();
  std::vector<RectEntry> table;
  std::vector<RectTile> tiles;
  rect_device_table(map_x, map_y, rect->src_w, rect->src_h, rect->dst_w, rect->dst_h, table, tiles, &rect->n_staged[camera], &rect->n_direct[camera]);
  SSHIP_HIP_CHECK(hipDeviceSynchronize());   // a remap of an earlier table may still be running
  SSHIP_HIP_CHECK(hipMemcpy(rect->table.as<RectEntry>() + rect->px() * camera, table.data(), table.size() * sizeof(RectEntry), hipMemcpyHostToDevice));
  SSHIP_HIP_CHECK(hipMemcpy(rect->tile_boxes.as<RectTile>() + (size_t)rect->tiles * camera, tiles.data(), tiles.size() * sizeof(RectTile), hipMemcpyHostToDevice));
  rect->have[camera] = true;
  return SSHIP_OK;
}
extern "C" int sship_rect_set_camera(sship_rect* rect, int camera, const double* K, const double* D, int n_dist, const double* R, const double* Pnew) {
  if (!rect) return fail(SSHIP_ERR_INVALID, "rect_set_camera: null argument");
  if (camera < 0 || camera >= rect->cameras) return fail(SSHIP_ERR_INVALID, "rect_set_camera: camera must be in [0, cameras)");
  std::vector<float> mx(rect->px()), my(rect->px());
  if (int rc = sship_rect_build_maps(K, D, n_dist, R, Pnew, rect->dst_w, rect->dst_h, mx.data(), my.data())) return rc;
  return sship_rect_set_maps(rect, camera, mx.data(), my.data());
}
extern "C" int sship_rect_read_table(sship_rect* rect, int camera, int32_t* ix, int32_t* iy, uint16_t* frac) {
  if (!rect || !ix || !iy || !frac) return fail(SSHIP_ERR_INVALID, "rect_read_table: null argument");
  if (camera < 0 || camera >= rect->cameras) return fail(SSHIP_ERR_INVALID, "rect_read_table: camera must be in [0, cameras)");
  if (!rect->have[camera]) return fail(SSHIP_ERR_INVALID, "rect_read_table: the camera has no maps");
  bind_thread();
  std::vector<RectEntry> table(rect->px());
  SSHIP_HIP_CHECK(hipDeviceSynchronize());
  SSHIP_HIP_CHECK(hipMemcpy(table.data(), rect->table.as<RectEntry>() + rect->px() * camera, table.size() * sizeof(RectEntry), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < table.size(); ++i) { ix[i] = table[i].ix; iy[i] = table[i].iy; frac[i] = (uint16_t)(table[i].frac_mask & kRectFracMask); }
  return SSHIP_OK;
}
extern "C" int sship_rect_tile_paths(const sship_rect* rect, int camera, int* staged, int* direct) {
  if (!rect || !staged || !direct) return fail(SSHIP_ERR_INVALID, "rect_tile_paths: null argument");
  if (camera < 0 || camera >= rect->cameras) return fail(SSHIP_ERR_INVALID, "rect_tile_paths: camera must be in [0, cameras)");
  if (!rect->have[camera]) return fail(SSHIP_ERR_INVALID, "rect_tile_paths: the camera has no maps");
  *staged = rect->n_staged[camera]; *direct = rect->n_direct[camera];
  return SSHIP_OK;
}
// the cameras images [0, images) starting at camera cam0 use must all have maps
static int rect_check_maps(const sship_rect* rect, int cam0, int images, const char* who) {
  for (int i = 0; i < std::min(images, rect->cameras); ++i)
    if (!rect->have[(cam0 + i) % rect->cameras]) return fail(SSHIP_ERR_INVALID, std::string(who) + ": a camera the call uses has no maps (sship_rect_set_maps)");
  return SSHIP_OK;
}
extern "C" int sship_rect_remap_batch_device(sship_rect* rect, const uint8_t* src, int images, int src_stride, uint8_t* dst, void* stream) {
  if (!rect || !src || !dst) return fail(SSHIP_ERR_INVALID, "rect_remap_batch_device: null argument");
  if (images <= 0 || images > (1 << 20)) return fail(SSHIP_ERR_INVALID, "rect_remap_batch_device: images must be in [1, 1048576]");
  if (src_stride < rect->src_w || src_stride > (1 << 20)) return fail(SSHIP_ERR_INVALID, "rect_remap_batch_device: src_stride must be in [src_w, 1048576]");
  if (int rc = rect_check_maps(rect, 0, images, "rect_remap_batch_device")) return rc;
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_rect_remap(src, rect->src_h, src_stride, dst, rect->dst_w, rect->dst_h, rect->table.p, rect->tile_boxes.as<RectTile>(), rect->cameras, 0,
                    images, 0, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("rect_remap", s);
  return SSHIP_OK;
}
extern "C" int sship_rect_remap_host(sship_rect* rect, int camera, const uint8_t* src, int src_stride, uint8_t* dst) {
  if (!rect || !src || !dst) return fail(SSHIP_ERR_INVALID, "rect_remap_host: null argument");
  if (camera < 0 || camera >= rect->cameras) return fail(SSHIP_ERR_INVALID, "rect_remap_host: camera must be in [0, cameras)");
  if (src_stride < rect->src_w) return fail(SSHIP_ERR_INVALID, "rect_remap_host: src_stride must be >= src_w");
  if (int rc = rect_check_maps(rect, camera, 1, "rect_remap_host")) return rc;
  bind_thread();
  hipStream_t s = rect->stream;
  const int pitch = (rect->src_w + 3) & ~3;
  SSHIP_HIP_CHECK(rect->src1.ensure((size_t)pitch * rect->src_h));
  SSHIP_HIP_CHECK(rect->dst1.ensure(rect->px()));
  SSHIP_HIP_CHECK(hipMemcpy2DAsync(rect->src1.p, pitch, src, src_stride, rect->src_w, rect->src_h, hipMemcpyHostToDevice, s));
  launch_rect_remap(rect->src1.as<uint8_t>(), rect->src_h, pitch, rect->dst1.as<uint8_t>(), rect->dst_w, rect->dst_h, rect->table.p,
                    rect->tile_boxes.as<RectTile>(), rect->cameras, camera, 1, 0, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  SSHIP_HIP_CHECK(hipMemcpyAsync(dst, rect->dst1.p, rect->px(), hipMemcpyDeviceToHost, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  return SSHIP_OK;
}
extern "C" int sship_rect_bench(sship_rect* rect, int images, int path, int iters, float* avg_ms) {
  if (!rect || !avg_ms || iters <= 0) return fail(SSHIP_ERR_INVALID, "rect_bench: bad arguments");
  if (images <= 0 || images > 65536) return fail(SSHIP_ERR_INVALID, "rect_bench: images must be in [1, 65536]");
  if (path != SSHIP_RECT_PATH_TILE && path != SSHIP_RECT_PATH_DIRECT) return fail(SSHIP_ERR_INVALID, "rect_bench: path must be 0 (tile) or 1 (direct)");
  if (int rc = rect_check_maps(rect, 0, images, "rect_bench")) return rc;
  bind_thread();
  hipStream_t s = rect->stream;
  const size_t sb = (size_t)rect->src_w * rect->src_h * images, db = rect->px() * images;
  SSHIP_HIP_CHECK(rect->bench_src.ensure(sb));
  SSHIP_HIP_CHECK(rect->bench_dst.ensure(db));
  SSHIP_HIP_CHECK(hipDeviceSynchronize());
  SSHIP_HIP_CHECK(hipMemsetAsync(rect->bench_src.p, 0x5a, sb, s));
  auto run = [&]() -> hipError_t {
    launch_rect_remap(rect->bench_src.as<uint8_t>(), rect->src_h, rect->src_w, rect->bench_dst.as<uint8_t>(), rect->dst_w, rect->dst_h,
                      rect->table.p, rect->tile_boxes.as<RectTile>(), rect->cameras, 0, images, path == SSHIP_RECT_PATH_DIRECT ? 1 : 0, s);
    return hipGetLastError();
  };
  return bench_loop(s, iters, run, avg_ms);
}
// the checks both RGB-D entries share; fills the kernel's constants
static int rgbd_check(int depth_type, int h, int w, int depth_stride, const sship_rgbd_params* p, RgbdK* c, const char* who) {
  if (depth_type != SSHIP_DEPTH_U16 && depth_type != SSHIP_DEPTH_F32)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": depth_type must be 0 (u16) or 1 (f32)");
  const int es = depth_type == SSHIP_DEPTH_F32 ? 4 : 2;
  if (h < 1 || w < 1 || h > 16384 || w > 16384) return fail(SSHIP_ERR_INVALID, std::string(who) + ": h and w must be in [1, 16384]");
  if (depth_stride < w * es || depth_stride % es) return fail(SSHIP_ERR_INVALID, std::string(who) + ": depth_stride (bytes) must be >= the row and a multiple of the sample size");
  if (!(p->fx > 0.0) || !(p->fy > 0.0) || !std::isfinite(p->fx) || !std::isfinite(p->fy)) return fail(SSHIP_ERR_INVALID, std::string(who) + ": fx and fy must be finite and > 0");
  if (!(p->depth_factor > 0.0) || !std::isfinite(p->depth_factor)) return fail(SSHIP_ERR_INVALID, std::string(who) + ": depth_factor must be finite and > 0");
  if (!std::isfinite(p->cx) || !std::isfinite(p->cy) || !std::isfinite(p->bf) || std::isnan(p->max_depth))
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": cx, cy and bf must be finite and max_depth not NaN");
  c->fx = p->fx; c->fy = p->fy; c->cx = p->cx; c->cy = p->cy; c->bf = p->bf; c->depth_factor = p->depth_factor; c->max_depth = p->max_depth;
  c->has_dist = 0;
  for (int i = 0; i < 8; ++i) {
    if (!std::isfinite(p->dist[i])) return fail(SSHIP_ERR_INVALID, std::string(who) + ": dist must be finite");
    c->d[i] = p->dist[i];
    if (p->dist[i] != 0.0) c->has_dist = 1;
  }
  return SSHIP_OK;
}
extern "C" int sship_rgbd_associate_batch_device(const float* kp, const int* n, int frames, int max_keypoints, const void* depth, int depth_type,
                                                 int h, int w, int depth_stride, const sship_rgbd_params* p, float* kp_undist, float* stereo,
                                                 uint8_t* has_depth, void* stream) {
  if (!kp || !n || !depth || !p || !stereo || !has_depth) return fail(SSHIP_ERR_INVALID, "rgbd_associate_batch_device: null argument");
  if (frames <= 0 || max_keypoints <= 0 || max_keypoints > kMaxKp)
    return fail(SSHIP_ERR_INVALID, "rgbd_associate_batch_device: frames must be positive and max_keypoints in [1, 4096]");
  RgbdK c;
  if (int rc = rgbd_check(depth_type, h, w, depth_stride, p, &c, "rgbd_associate_batch_device")) return rc;
  bind_thread();
  if (int rc = require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_rgbd_associate(kp, n, frames, max_keypoints, depth, depth_type == SSHIP_DEPTH_F32, h, w, depth_stride, c, kp_undist, stereo, has_depth, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("rgbd_associate", s);
  return SSHIP_OK;
}
extern "C" int sship_rgbd_associate_host(const float* keypoints, int kp_stride, int n, const void* depth, int depth_type, int h, int w,
                                         int depth_stride, const sship_rgbd_params* p, float* kp_undist, float* stereo, uint8_t* has_depth) {
  if (n == 0) return SSHIP_OK;
  if (!keypoints || !kp_undist) return fail(SSHIP_ERR_INVALID, "rgbd_associate_host: null argument");
  if (n < 0 || n > kMaxKp || kp_stride < 2) return fail(SSHIP_ERR_INVALID, "rgbd_associate_host: n must be in [0, 4096] and kp_stride >= 2");
  if (!depth || !p || !stereo || !has_depth) return fail(SSHIP_ERR_INVALID, "rgbd_associate_host: null argument");
  RgbdK c;
  if (int rc = rgbd_check(depth_type, h, w, depth_stride, p, &c, "rgbd_associate_host")) return rc;
  bind_thread();
  std::vector<float> kp((size_t)n * 3, 0.f), und((size_t)n * 3);
  for (int i = 0; i < n; ++i) { kp[3 * i] = keypoints[(size_t)i * kp_stride]; kp[3 * i + 1] = keypoints[(size_t)i * kp_stride + 1]; }
  const size_t kb = kp.size() * sizeof(float), db = (size_t)h * depth_stride;
  if (int rc = require_device()) return rc;
  StageLayout lay;   // one device block for the call; the copies stay blocking and straight from / to the caller's memory
  const size_t o_kp = lay.add(kb), o_n = lay.add(sizeof(int)), o_depth = lay.add(db), o_und = lay.add(kb), o_st = lay.add(kb), o_hd = lay.add((size_t)n);
  StageArena a;
  SSHIP_HIP_CHECK(a.create(lay.end, 0, false));
  SSHIP_HIP_CHECK(hipMemcpy(a.dev<float>(o_kp), kp.data(), kb, hipMemcpyHostToDevice));
  SSHIP_HIP_CHECK(hipMemcpy(a.dev<int>(o_n), &n, sizeof(int), hipMemcpyHostToDevice));
  SSHIP_HIP_CHECK(hipMemcpy(a.dev<char>(o_depth), depth, db, hipMemcpyHostToDevice));
  if (int rc = sship_rgbd_associate_batch_device(a.dev<float>(o_kp), a.dev<int>(o_n), 1, n, a.dev<char>(o_depth), depth_type, h, w, depth_stride, p,
                                                 a.dev<float>(o_und), a.dev<float>(o_st), a.dev<uint8_t>(o_hd), nullptr)) return rc;
  SSHIP_HIP_CHECK(hipMemcpy(und.data(), a.dev<float>(o_und), kb, hipMemcpyDeviceToHost));   // a blocking copy on the NULL stream: ordered after the launch
  SSHIP_HIP_CHECK(hipMemcpy(stereo, a.dev<float>(o_st), kb, hipMemcpyDeviceToHost));
  SSHIP_HIP_CHECK(hipMemcpy(has_depth, a.dev<uint8_t>(o_hd), (size_t)n, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) { kp_undist[2 * i] = und[3 * i]; kp_undist[2 * i + 1] = und[3 * i + 1]; }
  return SSHIP_OK;
}

// ====================================================================================================
// what the patch-search entries share (stereo refinement and search, patch and pyramid tracker)
// ====================================================================================================
static int size_check(int h, int w, const char* who) {
  if (h < 1 || w < 1 || h > 16384 || w > 16384) return fail(SSHIP_ERR_INVALID, std::string(who) + ": h and w must be in [1, 16384]");
  return SSHIP_OK;
}
// a per-pixel threshold (min_texture, max_rms) as the kernels test it: on if > 0, and (value pw^2)^2
static void patch_threshold(float value, int pw, int* on, double* squared) {
  const double t = (double)value * (double)(pw * pw);
  *on = value > 0.f ? 1 : 0;
  *squared = t * t;
}
// One image pair per call, staged through one device block of the call's own (pair_stage in csrc/stage_layout.h).  The copies stay blocking
// and, for the images and the outputs, straight from / to the caller's memory.  `tail`: the packed input region from the count on.
static int pair_upload(StageArena& a, const PairStage& st, const uint8_t* img0, int stride0, const uint8_t* img1, int stride1, int h, int w,
                       const std::vector<char>& tail) {
  SSHIP_HIP_CHECK(a.create(st.in_bytes, st.out_bytes, false));
  SSHIP_HIP_CHECK(hipMemcpy2D(a.dev<uint8_t>(st.img), (size_t)w, img0, (size_t)stride0, (size_t)w, (size_t)h, hipMemcpyHostToDevice));
  SSHIP_HIP_CHECK(hipMemcpy2D(a.dev<uint8_t>(st.img1), (size_t)w, img1, (size_t)stride1, (size_t)w, (size_t)h, hipMemcpyHostToDevice));
  SSHIP_HIP_CHECK(hipMemcpy(a.dev<char>(st.n), tail.data(), st.tail_bytes, hipMemcpyHostToDevice));
  return SSHIP_OK;
}
// the outputs the caller asked for (dst != NULL): blocking copies on the NULL stream, so ordered after the launch
struct PairOut { void* dst; size_t off, bytes; };
static int pair_fetch(const StageArena& a, std::initializer_list<PairOut> outs) {
  for (const PairOut& o : outs)
    if (o.dst) { SSHIP_HIP_CHECK(hipMemcpy(o.dst, a.dev<char>(a.out + o.off), o.bytes, hipMemcpyDeviceToHost)); }
  return SSHIP_OK;
}

// ====================================================================================================
// sub-pixel disparity refinement by patch correlation (the rule is in include/sship.h)
// ====================================================================================================
// the checks both entries share; fills the kernel's constants
static int refine_check(int h, int w, const sship_stereo_refine_params* p, StereoRefineK* c, const char* who) {
  if (int rc = size_check(h, w, who)) return rc;
  if (p->half_window < 1 || p->half_window > 7) return fail(SSHIP_ERR_INVALID, std::string(who) + ": half_window must be in [1, 7]");
  if (p->search_radius < 1 || p->search_radius > 15) return fail(SSHIP_ERR_INVALID, std::string(who) + ": search_radius must be in [1, 15]");
  if (std::isnan(p->max_rms) || std::isnan(p->min_disparity)) return fail(SSHIP_ERR_INVALID, std::string(who) + ": max_rms and min_disparity must not be NaN");
  if (p->on_reject != SSHIP_REFINE_KEEP && p->on_reject != SSHIP_REFINE_DROP)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": on_reject must be 0 (keep) or 1 (drop)");
  patch_threshold(p->max_rms, 2 * p->half_window + 1, &c->gate, &c->gate2);
  c->min_disparity = p->min_disparity;
  c->half_window = p->half_window; c->search_radius = p->search_radius;
  c->drop = p->on_reject == SSHIP_REFINE_DROP ? 1 : 0;
  return SSHIP_OK;
}
extern "C" int sship_stereo_refine_batch_device(const uint8_t* imgs, int pairs, int h, int w, int stride, const float* stereo_in,
                                                const uint8_t* has_depth_in, const int* n, int n_stride, int max_keypoints,
                                                const sship_stereo_refine_params* p, float* stereo_out, uint8_t* has_depth_out,
                                                uint8_t* status, int64_t* cost, void* stream) {
  if (!imgs || !stereo_in || !has_depth_in || !n || !p || !stereo_out || !has_depth_out)
    return fail(SSHIP_ERR_INVALID, "stereo_refine_batch_device: null argument");
  if (pairs <= 0 || max_keypoints <= 0 || max_keypoints > kMaxKp)
    return fail(SSHIP_ERR_INVALID, "stereo_refine_batch_device: pairs must be positive and max_keypoints in [1, 4096]");
  if (n_stride != 1 && n_stride != 2) return fail(SSHIP_ERR_INVALID, "stereo_refine_batch_device: n_stride must be 1 or 2");
  StereoRefineK c;
  if (int rc = refine_check(h, w, p, &c, "stereo_refine_batch_device")) return rc;
  if (stride < w) return fail(SSHIP_ERR_INVALID, "stereo_refine_batch_device: stride (bytes) must be >= w");
  bind_thread();
  if (int rc = require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_stereo_refine(imgs, pairs, h, w, stride, stereo_in, has_depth_in, n, n_stride, max_keypoints, c, stereo_out, has_depth_out, status,
                       reinterpret_cast<long long*>(cost), s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("stereo_refine", s);
  return SSHIP_OK;
}
extern "C" int sship_stereo_refine_host(const uint8_t* left, int left_stride, const uint8_t* right, int right_stride, int h, int w,
                                        const float* stereo, const uint8_t* has_depth, int n, const sship_stereo_refine_params* p,
                                        float* stereo_out, uint8_t* has_depth_out, uint8_t* status, int64_t* cost) {
  if (!left || !right || !p) return fail(SSHIP_ERR_INVALID, "stereo_refine_host: null argument");
  if (n < 0 || n > kMaxKp) return fail(SSHIP_ERR_INVALID, "stereo_refine_host: n must be in [0, 4096]");
  StereoRefineK c;
  if (int rc = refine_check(h, w, p, &c, "stereo_refine_host")) return rc;
  if (left_stride < w || right_stride < w) return fail(SSHIP_ERR_INVALID, "stereo_refine_host: stride (bytes) must be >= w");
  if (n == 0) return SSHIP_OK;
  if (!stereo || !has_depth || !stereo_out || !has_depth_out) return fail(SSHIP_ERR_INVALID, "stereo_refine_host: null argument");
  bind_thread();
  if (int rc = require_device()) return rc;
  const PairStage st = pair_stage(h, w, n);
  const size_t m = (size_t)n;
  std::vector<char> tail(st.tail_bytes, 0);
  pair_pack_n(tail.data(), n);
  StageArena a;
  if (int rc = pair_upload(a, st, left, left_stride, right, right_stride, h, w, tail)) return rc;
  float* rows = a.dev<float>(a.out + st.rows);              // the caller's rows go straight into the output slots: refined in place
  uint8_t* hd = a.dev<uint8_t>(a.out + st.flag);
  SSHIP_HIP_CHECK(hipMemcpy(rows, stereo, st.rows_bytes, hipMemcpyHostToDevice));
  SSHIP_HIP_CHECK(hipMemcpy(hd, has_depth, m, hipMemcpyHostToDevice));
  if (int rc = sship_stereo_refine_batch_device(a.dev<uint8_t>(st.img), 1, h, w, w, rows, hd, a.dev<int>(st.n), 1, n, p, rows, hd,
                                                a.dev<uint8_t>(a.out + st.status), a.dev<int64_t>(a.out + st.cost), nullptr)) return rc;
  return pair_fetch(a, {{stereo_out, st.rows, st.rows_bytes}, {has_depth_out, st.flag, m}, {status, st.status, m}, {cost, st.cost, m * 8}});
}

// ====================================================================================================
// keypoint stereo depth by epipolar search (the rule is in include/sship.h)
// ====================================================================================================
// the checks both entries share; fills the kernel's constants
static int search_check(int h, int w, const sship_stereo_search_params* p, StereoSearchK* c, const char* who) {
  if (int rc = size_check(h, w, who)) return rc;
  if (p->half_window < 1 || p->half_window > 7) return fail(SSHIP_ERR_INVALID, std::string(who) + ": half_window must be in [1, 7]");
  if (p->min_disparity < 0 || p->max_disparity < p->min_disparity)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": 0 <= min_disparity <= max_disparity is required");
  const long long cand = (long long)p->max_disparity - p->min_disparity + 1;
  if (cand < 3 || cand > 512) return fail(SSHIP_ERR_INVALID, std::string(who) + ": max_disparity - min_disparity + 1 must be in [3, 512]");
  if (p->uniqueness < 0 || p->uniqueness > 99) return fail(SSHIP_ERR_INVALID, std::string(who) + ": uniqueness must be in [0, 99]");
  if (p->lr_check < -1 || p->lr_check > 16) return fail(SSHIP_ERR_INVALID, std::string(who) + ": lr_check must be in [-1, 16]");
  if (std::isnan(p->min_texture) || std::isnan(p->max_rms)) return fail(SSHIP_ERR_INVALID, std::string(who) + ": min_texture and max_rms must not be NaN");
  patch_threshold(p->min_texture, 2 * p->half_window + 1, &c->tex, &c->tex2);
  patch_threshold(p->max_rms, 2 * p->half_window + 1, &c->gate, &c->gate2);
  c->half_window = p->half_window; c->dlo = p->min_disparity; c->dhi = p->max_disparity;
  c->uniqueness = p->uniqueness; c->lr = p->lr_check;
  return SSHIP_OK;
}
extern "C" int sship_stereo_search_batch_device(const uint8_t* imgs, int pairs, int h, int w, int stride, const float* kp, const int* n,
                                                int unit_stride, int max_keypoints, const sship_stereo_search_params* p, float* stereo_out,
                                                uint8_t* has_depth_out, uint8_t* status, int64_t* cost, void* stream) {
  if (!imgs || !kp || !n || !p || !stereo_out || !has_depth_out) return fail(SSHIP_ERR_INVALID, "stereo_search_batch_device: null argument");
  if (pairs <= 0 || max_keypoints <= 0 || max_keypoints > kMaxKp)
    return fail(SSHIP_ERR_INVALID, "stereo_search_batch_device: pairs must be positive and max_keypoints in [1, 4096]");
  if (unit_stride != 1 && unit_stride != 2) return fail(SSHIP_ERR_INVALID, "stereo_search_batch_device: unit_stride must be 1 or 2");
  StereoSearchK c;
  if (int rc = search_check(h, w, p, &c, "stereo_search_batch_device")) return rc;
  if (stride < w) return fail(SSHIP_ERR_INVALID, "stereo_search_batch_device: stride (bytes) must be >= w");
  bind_thread();
  if (int rc = require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_stereo_search(imgs, pairs, h, w, stride, kp, n, unit_stride, max_keypoints, c, stereo_out, has_depth_out, status,
                       reinterpret_cast<long long*>(cost), s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("stereo_search", s);
  return SSHIP_OK;
}
extern "C" int sship_stereo_search_host(const uint8_t* left, int left_stride, const uint8_t* right, int right_stride, int h, int w,
                                        const float* keypoints, int kp_stride, int n, const sship_stereo_search_params* p, float* stereo_out,
                                        uint8_t* has_depth_out, uint8_t* status, int64_t* cost) {
  if (!left || !right || !p) return fail(SSHIP_ERR_INVALID, "stereo_search_host: null argument");
  if (n < 0 || n > kMaxKp || kp_stride < 2) return fail(SSHIP_ERR_INVALID, "stereo_search_host: n must be in [0, 4096] and kp_stride >= 2");
  StereoSearchK c;
  if (int rc = search_check(h, w, p, &c, "stereo_search_host")) return rc;
  if (left_stride < w || right_stride < w) return fail(SSHIP_ERR_INVALID, "stereo_search_host: stride (bytes) must be >= w");
  if (n == 0) return SSHIP_OK;
  if (!keypoints || !stereo_out || !has_depth_out) return fail(SSHIP_ERR_INVALID, "stereo_search_host: null argument");
  bind_thread();
  if (int rc = require_device()) return rc;
  const PairStage st = pair_stage(h, w, n);
  const size_t m = (size_t)n;
  std::vector<char> tail(st.tail_bytes, 0);
  pair_pack_n(tail.data(), n);
  pair_pack_kp(tail.data(), st, keypoints, kp_stride, n, false);
  StageArena a;
  if (int rc = pair_upload(a, st, left, left_stride, right, right_stride, h, w, tail)) return rc;
  if (int rc = sship_stereo_search_batch_device(a.dev<uint8_t>(st.img), 1, h, w, w, a.dev<float>(st.kp), a.dev<int>(st.n), 1, n, p,
                                                a.dev<float>(a.out + st.rows), a.dev<uint8_t>(a.out + st.flag), a.dev<uint8_t>(a.out + st.status),
                                                a.dev<int64_t>(a.out + st.cost), nullptr)) return rc;
  return pair_fetch(a, {{stereo_out, st.rows, st.rows_bytes}, {has_depth_out, st.flag, m}, {status, st.status, m}, {cost, st.cost, m * 8}});
}

// ====================================================================================================
// keypoint tracking by 2-D patch search (the rule is in include/sship.h)
// ====================================================================================================
// the checks both entries share; fills the kernel's constants
static int track_check(int h, int w, int stride0, int stride1, const sship_patch_track_params* p, PatchTrackK* c, const char* who) {
  if (int rc = size_check(h, w, who)) return rc;
  if (stride0 < w || stride1 < w) return fail(SSHIP_ERR_INVALID, std::string(who) + ": stride (bytes) must be >= w");
  if (p->half_window < 1 || p->half_window > 7) return fail(SSHIP_ERR_INVALID, std::string(who) + ": half_window must be in [1, 7]");
  if (p->search_radius < 1 || p->search_radius > 16) return fail(SSHIP_ERR_INVALID, std::string(who) + ": search_radius must be in [1, 16]");
  if (p->uniqueness < 0 || p->uniqueness > 99) return fail(SSHIP_ERR_INVALID, std::string(who) + ": uniqueness must be in [0, 99]");
  if (p->fb_check < -1 || p->fb_check > 16) return fail(SSHIP_ERR_INVALID, std::string(who) + ": fb_check must be in [-1, 16]");
  if (std::isnan(p->min_texture) || std::isnan(p->max_rms)) return fail(SSHIP_ERR_INVALID, std::string(who) + ": min_texture and max_rms must not be NaN");
  patch_threshold(p->min_texture, 2 * p->half_window + 1, &c->tex, &c->tex2);
  patch_threshold(p->max_rms, 2 * p->half_window + 1, &c->gate, &c->gate2);
  c->half_window = p->half_window; c->radius = p->search_radius; c->uniqueness = p->uniqueness; c->fb = p->fb_check;
  return SSHIP_OK;
}
extern "C" int sship_patch_track_batch_device(const uint8_t* imgs0, long long image_stride0, int stride0, const uint8_t* imgs1,
                                              long long image_stride1, int stride1, int pairs, int h, int w, const float* kp, const int* n,
                                              int unit_stride, const float* pred, int max_keypoints, const sship_patch_track_params* p,
                                              float* kp_out, int* n_out, int32_t* matches0, uint8_t* status, int64_t* cost, void* stream) {
  if (!imgs0 || !imgs1 || !kp || !n || !p || !kp_out || !matches0) return fail(SSHIP_ERR_INVALID, "patch_track_batch_device: null argument");
  if (pairs <= 0 || max_keypoints <= 0 || max_keypoints > kMaxKp)
    return fail(SSHIP_ERR_INVALID, "patch_track_batch_device: pairs must be positive and max_keypoints in [1, 4096]");
  if (unit_stride != 1 && unit_stride != 2) return fail(SSHIP_ERR_INVALID, "patch_track_batch_device: unit_stride must be 1 or 2");
  if (image_stride0 < 0 || image_stride1 < 0) return fail(SSHIP_ERR_INVALID, "patch_track_batch_device: image strides (bytes) must be >= 0");
  PatchTrackK c;
  if (int rc = track_check(h, w, stride0, stride1, p, &c, "patch_track_batch_device")) return rc;
  bind_thread();
  if (int rc = require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_patch_track(imgs0, image_stride0, stride0, imgs1, image_stride1, stride1, pairs, h, w, kp, n, unit_stride, pred, max_keypoints, c, kp_out,
                     n_out, matches0, status, reinterpret_cast<long long*>(cost), s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("patch_track", s);
  return SSHIP_OK;
}
extern "C" int sship_patch_track_host(const uint8_t* img0, int stride0, const uint8_t* img1, int stride1, int h, int w, const float* keypoints,
                                      int kp_stride, const float* pred, int pred_stride, int n, const sship_patch_track_params* p, float* kp_out,
                                      int32_t* matches0, uint8_t* status, int64_t* cost) {
  if (!img0 || !img1 || !p) return fail(SSHIP_ERR_INVALID, "patch_track_host: null argument");
  if (n < 0 || n > kMaxKp || kp_stride < 2 || (pred && pred_stride < 2))
    return fail(SSHIP_ERR_INVALID, "patch_track_host: n must be in [0, 4096], kp_stride >= 2 and, with pred, pred_stride >= 2");
  PatchTrackK c;
  if (int rc = track_check(h, w, stride0, stride1, p, &c, "patch_track_host")) return rc;
  if (n == 0) return SSHIP_OK;
  if (!keypoints || !kp_out || !matches0) return fail(SSHIP_ERR_INVALID, "patch_track_host: null argument");
  bind_thread();
  if (int rc = require_device()) return rc;
  const PairStage st = pair_stage(h, w, n);
  const size_t m = (size_t)n;
  std::vector<char> tail(st.tail_bytes, 0);
  pair_pack_n(tail.data(), n);
  pair_pack_kp(tail.data(), st, keypoints, kp_stride, n, true);
  if (pred) pair_pack_pred(tail.data(), st, pred, pred_stride, n);
  StageArena a;
  if (int rc = pair_upload(a, st, img0, stride0, img1, stride1, h, w, tail)) return rc;
  if (int rc = sship_patch_track_batch_device(a.dev<uint8_t>(st.img), 0, w, a.dev<uint8_t>(st.img1), 0, w, 1, h, w, a.dev<float>(st.kp), a.dev<int>(st.n),
                                              1, pred ? a.dev<float>(st.pred) : nullptr, n, p, a.dev<float>(a.out + st.rows), nullptr,
                                              a.dev<int32_t>(a.out + st.flag), a.dev<uint8_t>(a.out + st.status), a.dev<int64_t>(a.out + st.cost),
                                              nullptr)) return rc;
  return pair_fetch(a, {{kp_out, st.rows, st.rows_bytes}, {matches0, st.flag, m * 4}, {status, st.status, m}, {cost, st.cost, m * 8}});
}

// ====================================================================================================
// image pyramid (sship_pyr_*) and coarse-to-fine patch tracking (the rules are in include/sship.h)
// ====================================================================================================
struct sship_pyr {
  int h = 0, w = 0, levels = 0, max_images = 0;
  int lh[kPyrMaxLevels] = {}, lw[kPyrMaxLevels] = {}, pitch[kPyrMaxLevels] = {};
  size_t off[kPyrMaxLevels] = {};   // of level l >= 1 in `store`: max_images images of pitch[l] * lh[l] bytes each
  hipStream_t stream = nullptr;
  DevBuf store;
  // the last build; level 0 is the caller's memory
  const uint8_t* l0 = nullptr;
  long long l0_image_stride = 0;
  int l0_stride = 0, images = 0;
  size_t image_bytes(int l) const { return (size_t)pitch[l] * lh[l]; }
  uint8_t* level_ptr(int l) const { return store.as<uint8_t>() + off[l]; }
};
static int pyr_pitch(int w) { return (w + kPyrRowAlign - 1) / kPyrRowAlign * kPyrRowAlign; }
extern "C" int sship_pyr_create(int h, int w, int levels, int max_images, sship_pyr** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "pyr_create: null argument");
  *out = nullptr;
  if (h < 1 || w < 1 || h > 16384 || w > 16384) return fail(SSHIP_ERR_INVALID, "pyr_create: h and w must be in [1, 16384]");
  if (levels < 1 || levels > kPyrMaxLevels) return fail(SSHIP_ERR_INVALID, "pyr_create: levels must be in [1, 8]");
  if (max_images < 1 || max_images > 65535) return fail(SSHIP_ERR_INVALID, "pyr_create: max_images must be in [1, 65535]");
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_pyr, void (*)(sship_pyr*)> p(new sship_pyr(), sship_pyr_destroy);
  p->h = h; p->w = w; p->levels = levels; p->max_images = max_images;
  p->lh[0] = h; p->lw[0] = w;
  StageLayout lay;
  for (int l = 1; l < levels; ++l) {
    p->lh[l] = (p->lh[l - 1] + 1) / 2; p->lw[l] = (p->lw[l - 1] + 1) / 2; p->pitch[l] = pyr_pitch(p->lw[l]);
    p->off[l] = lay.add(p->image_bytes(l) * max_images);
  }
  SSHIP_HIP_CHECK(p->store.ensure(lay.end));
  if (lay.end) { SSHIP_HIP_CHECK(hipMemset(p->store.p, 0, lay.end)); }
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&p->stream, hipStreamDefault));
  *out = p.release();
  return SSHIP_OK;
}
extern "C" void sship_pyr_destroy(sship_pyr* pyr) { destroy_handle(pyr); }
// dword loads need every row of every image on a multiple of 4 bytes: always so in the handle's own levels, in the caller's level 0 where
// its pointer and strides happen to be
static bool pyr_dword_rows(const uint8_t* p, long long image_stride, long long stride) {
  return (reinterpret_cast<uintptr_t>(p) | (uintptr_t)image_stride | (uintptr_t)stride) % 4 == 0;
}
static void pyr_launch_levels(const sship_pyr* pyr, hipStream_t s) {
  for (int l = 1; l < pyr->levels; ++l) {
    const bool own = l > 1;
    const uint8_t* src = own ? pyr->level_ptr(l - 1) : pyr->l0;
    const long long is = own ? (long long)pyr->image_bytes(l - 1) : pyr->l0_image_stride, st = own ? pyr->pitch[l - 1] : pyr->l0_stride;
    launch_pyr_down(src, is, st, pyr->lh[l - 1], pyr->lw[l - 1], pyr_dword_rows(src, is, st) ? 1 : 0, pyr->level_ptr(l), (long long)pyr->image_bytes(l),
                    pyr->pitch[l], pyr->images, s);
  }
}
extern "C" int sship_pyr_build_batch_device(sship_pyr* pyr, const uint8_t* imgs, long long image_stride, int stride, int images, void* stream) {
  if (!pyr || !imgs) return fail(SSHIP_ERR_INVALID, "pyr_build_batch_device: null argument");
  if (images < 1 || images > pyr->max_images) return fail(SSHIP_ERR_INVALID, "pyr_build_batch_device: images must be in [1, max_images]");
  if (stride < pyr->w) return fail(SSHIP_ERR_INVALID, "pyr_build_batch_device: stride (bytes) must be >= w");
  if (image_stride < 0) return fail(SSHIP_ERR_INVALID, "pyr_build_batch_device: image_stride (bytes) must be >= 0");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  pyr->l0 = imgs; pyr->l0_image_stride = image_stride; pyr->l0_stride = stride; pyr->images = images;
  pyr_launch_levels(pyr, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("pyr_build", s);
  return SSHIP_OK;
}
static int pyr_check_level(const sship_pyr* pyr, int level, const char* who) {
  if (!pyr) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (level < 0 || level >= pyr->levels) return fail(SSHIP_ERR_INVALID, std::string(who) + ": level must be in [0, levels)");
  if (pyr->images <= 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": build the pyramid first");
  return SSHIP_OK;
}
extern "C" int sship_pyr_level(const sship_pyr* pyr, int level, const uint8_t** ptr, int* h, int* w, int* stride, long long* image_stride, int* images) {
  if (int rc = pyr_check_level(pyr, level, "pyr_level")) return rc;
  if (ptr) *ptr = level ? pyr->level_ptr(level) : pyr->l0;
  if (h) *h = pyr->lh[level];
  if (w) *w = pyr->lw[level];
  if (stride) *stride = level ? pyr->pitch[level] : pyr->l0_stride;
  if (image_stride) *image_stride = level ? (long long)pyr->image_bytes(level) : pyr->l0_image_stride;
  if (images) *images = pyr->images;
  return SSHIP_OK;
}
extern "C" int sship_pyr_read_level(const sship_pyr* pyr, int level, int first, int count, uint8_t* out, int out_stride) {
  if (int rc = pyr_check_level(pyr, level, "pyr_read_level")) return rc;
  if (!out) return fail(SSHIP_ERR_INVALID, "pyr_read_level: null argument");
  if (first < 0 || count < 1 || (long long)first + count > pyr->images)
    return fail(SSHIP_ERR_INVALID, "pyr_read_level: first and count must name images of the last build");
  if (out_stride < pyr->lw[level]) return fail(SSHIP_ERR_INVALID, "pyr_read_level: out_stride (bytes) must be >= the level's width");
  bind_thread();
  const uint8_t* ptr; int h, w, stride; long long is;
  (void)sship_pyr_level(pyr, level, &ptr, &h, &w, &stride, &is, nullptr);
  SSHIP_HIP_CHECK(hipDeviceSynchronize());   // the build may have run on the caller's stream
  for (int i = 0; i < count; ++i)
    SSHIP_HIP_CHECK(hipMemcpy2D(out + (size_t)i * h * out_stride, (size_t)out_stride, ptr + (size_t)(first + i) * is, (size_t)stride, (size_t)w, (size_t)h,
                                hipMemcpyDeviceToHost));
  return SSHIP_OK;
}
extern "C" int sship_pyr_down_host(const uint8_t* src, int src_stride, int h, int w, uint8_t* dst, int dst_stride) {
  if (!src || !dst) return fail(SSHIP_ERR_INVALID, "pyr_down_host: null argument");
  if (h < 1 || w < 1 || h > 16384 || w > 16384) return fail(SSHIP_ERR_INVALID, "pyr_down_host: h and w must be in [1, 16384]");
  const int h2 = (h + 1) / 2, w2 = (w + 1) / 2, pitch = pyr_pitch(w2);
  if (src_stride < w || dst_stride < w2) return fail(SSHIP_ERR_INVALID, "pyr_down_host: src_stride must be >= w and dst_stride >= (w + 1) / 2");
  bind_thread();
  if (int rc = require_device()) return rc;
  StageLayout lay;   // one device block for the call: the image packed to stride w, then the reduced image in padded rows
  const size_t o_src = lay.add((size_t)h * w), o_dst = lay.add((size_t)h2 * pitch);
  StageArena a;
  SSHIP_HIP_CHECK(a.create(lay.end, 0, false));
  SSHIP_HIP_CHECK(hipMemcpy2D(a.dev<uint8_t>(o_src), (size_t)w, src, (size_t)src_stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice));
  launch_pyr_down(a.dev<uint8_t>(o_src), 0, w, h, w, pyr_dword_rows(a.dev<uint8_t>(o_src), 0, w) ? 1 : 0, a.dev<uint8_t>(o_dst), 0, pitch, 1, nullptr);
  SSHIP_HIP_CHECK(hipGetLastError());
  SSHIP_HIP_CHECK(hipMemcpy2D(dst, (size_t)dst_stride, a.dev<uint8_t>(o_dst), (size_t)pitch, (size_t)w2, (size_t)h2, hipMemcpyDeviceToHost));   // blocking, on the NULL stream: after the launch
  return SSHIP_OK;
}
// Measurement hook (include/sship.h): the last build's launches re-run `iters` times on the handle's stream.
extern "C" int sship_pyr_bench(sship_pyr* pyr, int iters, float* avg_ms) {
  if (!pyr || !avg_ms || iters <= 0) return fail(SSHIP_ERR_INVALID, "pyr_bench: bad arguments");
  if (pyr->images <= 0) return fail(SSHIP_ERR_INVALID, "pyr_bench: build the pyramid first");
  bind_thread();
  SSHIP_HIP_CHECK(hipDeviceSynchronize());   // the last build may have run on the caller's stream
  return bench_loop(pyr->stream, iters, [&]() { pyr_launch_levels(pyr, pyr->stream); return hipGetLastError(); }, avg_ms);
}

// the checks both pyramid-tracker entries share; fills the kernel's constants
static int pyr_track_check(int h, int w, const sship_pyr_track_params* p, PyrTrackK* c, const char* who) {
  if (p->levels < 1 || p->levels > kPyrMaxLevels) return fail(SSHIP_ERR_INVALID, std::string(who) + ": levels must be in [1, 8]");
  if (p->coarse_radius < 1 || p->coarse_radius > 16) return fail(SSHIP_ERR_INVALID, std::string(who) + ": coarse_radius must be in [1, 16]");
  if (int rc = track_check(h, w, w, w, &p->fine, &c->fine, who)) return rc;
  c->levels = p->levels; c->coarse_radius = p->coarse_radius;
  c->slot_bytes = (int)pyr_track_slot_bytes(p->fine.half_window, p->levels > 1 ? std::max(p->fine.search_radius, p->coarse_radius) : p->fine.search_radius);
  return SSHIP_OK;
}
extern "C" int sship_patch_track_pyramid_batch_device(const sship_pyr* pyr0, int first0, int step0, const sship_pyr* pyr1, int first1, int step1,
                                                      int pairs, const float* kp, const int* n, int unit_stride, const float* pred,
                                                      int max_keypoints, const sship_pyr_track_params* p, float* kp_out, int* n_out,
                                                      int32_t* matches0, uint8_t* status, int64_t* cost, uint8_t* levels_tracked, void* stream) {
  const char* who = "patch_track_pyramid_batch_device";
  if (!pyr0 || !pyr1 || !kp || !n || !p || !kp_out || !matches0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (pairs <= 0 || max_keypoints <= 0 || max_keypoints > kMaxKp)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": pairs must be positive and max_keypoints in [1, 4096]");
  if (unit_stride != 1 && unit_stride != 2) return fail(SSHIP_ERR_INVALID, std::string(who) + ": unit_stride must be 1 or 2");
  if (pyr0->h != pyr1->h || pyr0->w != pyr1->w) return fail(SSHIP_ERR_INVALID, std::string(who) + ": the pyramids must have the same h and w");
  PyrTrackK c;
  if (int rc = pyr_track_check(pyr0->h, pyr0->w, p, &c, who)) return rc;
  if (pyr0->levels < p->levels || pyr1->levels < p->levels) return fail(SSHIP_ERR_INVALID, std::string(who) + ": a pyramid has fewer levels than params.levels");
  if (pyr0->images <= 0 || pyr1->images <= 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": build the pyramids first");
  if (first0 < 0 || step0 < 0 || first1 < 0 || step1 < 0 || (long long)first0 + (long long)(pairs - 1) * step0 >= pyr0->images ||
      (long long)first1 + (long long)(pairs - 1) * step1 >= pyr1->images)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": first + pair * step must name images of the last build, with first and step >= 0");
  bind_thread();
  if (int rc = require_device()) return rc;
  PyrTrackLevels tab = {};
  for (int l = 0; l < p->levels; ++l) {
    PyrTrackLevel& L = tab.l[l];
    const uint8_t *b0, *b1; int s0, s1; long long is0, is1;
    (void)sship_pyr_level(pyr0, l, &b0, &L.h, &L.w, &s0, &is0, nullptr);
    (void)sship_pyr_level(pyr1, l, &b1, nullptr, nullptr, &s1, &is1, nullptr);
    L.img0 = b0 + (size_t)first0 * is0; L.img1 = b1 + (size_t)first1 * is1;
    L.pair_stride0 = step0 * is0; L.pair_stride1 = step1 * is1; L.stride0 = s0; L.stride1 = s1;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_pyr_track(tab, pairs, kp, n, unit_stride, pred, max_keypoints, c, kp_out, n_out, matches0, status, reinterpret_cast<long long*>(cost),
                   levels_tracked, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("patch_track_pyramid", s);
  return SSHIP_OK;
}
extern "C" int sship_patch_track_pyramid_host(const uint8_t* img0, int stride0, const uint8_t* img1, int stride1, int h, int w, const float* keypoints,
                                              int kp_stride, const float* pred, int pred_stride, int n, const sship_pyr_track_params* p, float* kp_out,
                                              int32_t* matches0, uint8_t* status, int64_t* cost, uint8_t* levels_tracked) {
  const char* who = "patch_track_pyramid_host";
  if (!img0 || !img1 || !p) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (n < 0 || n > kMaxKp || kp_stride < 2 || (pred && pred_stride < 2))
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": n must be in [0, 4096], kp_stride >= 2 and, with pred, pred_stride >= 2");
  if (int rc = size_check(h, w, who)) return rc;
  if (stride0 < w || stride1 < w) return fail(SSHIP_ERR_INVALID, std::string(who) + ": stride (bytes) must be >= w");
  PyrTrackK c;
  if (int rc = pyr_track_check(h, w, p, &c, who)) return rc;
  if (n == 0) return SSHIP_OK;
  if (!keypoints || !kp_out || !matches0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  bind_thread();
  if (int rc = require_device()) return rc;
  const PairStage st = pair_stage(h, w, n);
  const size_t m = (size_t)n;
  std::vector<char> tail(st.tail_bytes, 0);
  pair_pack_n(tail.data(), n);
  pair_pack_kp(tail.data(), st, keypoints, kp_stride, n, true);
  if (pred) pair_pack_pred(tail.data(), st, pred, pred_stride, n);
  StageArena a;
  if (int rc = pair_upload(a, st, img0, stride0, img1, stride1, h, w, tail)) return rc;
  sship_pyr* raw = nullptr;   // a two-image pyramid reads the staged pair
  if (int rc = sship_pyr_create(h, w, p->levels, 2, &raw)) return rc;
  std::unique_ptr<sship_pyr, void (*)(sship_pyr*)> pyr(raw, sship_pyr_destroy);
  if (int rc = sship_pyr_build_batch_device(raw, a.dev<uint8_t>(st.img), (long long)(st.img1 - st.img), w, 2, nullptr)) return rc;
  if (int rc = sship_patch_track_pyramid_batch_device(raw, 0, 1, raw, 1, 1, 1, a.dev<float>(st.kp), a.dev<int>(st.n), 1,
                                                      pred ? a.dev<float>(st.pred) : nullptr, n, p, a.dev<float>(a.out + st.rows), nullptr,
                                                      a.dev<int32_t>(a.out + st.flag), a.dev<uint8_t>(a.out + st.status),
                                                      a.dev<int64_t>(a.out + st.cost), a.dev<uint8_t>(a.out + st.levels), nullptr)) return rc;
  return pair_fetch(a, {{kp_out, st.rows, st.rows_bytes}, {matches0, st.flag, m * 4}, {status, st.status, m}, {cost, st.cost, m * 8},
                        {levels_tracked, st.levels, m}});
}

// ====================================================================================================
// contrast-limited adaptive histogram equalisation (sship_clahe_*; the rule is in include/sship.h)
// ====================================================================================================
struct sship_clahe {
  int h = 0, w = 0, max_images = 0;
  double clip_limit = 0.0;
  ClaheK k = {};
  hipStream_t stream = nullptr;
  DevBuf luts;   // [max_images, tiles_y, tiles_x, 256] u8
  // the last call
  const uint8_t* src = nullptr;
  uint8_t* dst = nullptr;
  long long src_image_stride = 0, dst_image_stride = 0;
  int src_stride = 0, dst_stride = 0, images = 0;
  size_t image_luts() const { return (size_t)k.tiles_x * k.tiles_y * 256; }
};
static int clahe_check_clip(double clip_limit, const char* who) {
  if (!std::isfinite(clip_limit) || clip_limit < 0.0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": clip_limit must be finite and >= 0");
  return SSHIP_OK;
}
// L of the rule (0: no clipping): the product and the quotient in fp64, truncated
static int clahe_limit(double clip_limit, int area) {
  if (clip_limit == 0.0) return 0;
  const double q = (clip_limit * (double)area) / 256.0;
  if (q >= (double)area) return area;
  return std::max(1, (int)q);
}
// the size checks every entry shares; fills the kernels' constants
static int clahe_geometry(int h, int w, int tiles_x, int tiles_y, double clip_limit, ClaheK* k, const char* who) {
  if (h < 1 || w < 1 || h > 16384 || w > 16384) return fail(SSHIP_ERR_INVALID, std::string(who) + ": h and w must be in [1, 16384]");
  if (tiles_x < 1 || tiles_x > kClaheMaxTiles || tiles_y < 1 || tiles_y > kClaheMaxTiles)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": tiles_x and tiles_y must be in [1, 16]");
  if (int rc = clahe_check_clip(clip_limit, who)) return rc;
  int ew = w, eh = h;
  if (w % tiles_x != 0 || h % tiles_y != 0) { ew = w + (tiles_x - w % tiles_x); eh = h + (tiles_y - h % tiles_y); }
  if (ew - w > w - 1 || eh - h > h - 1)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": the image is too small for its extension (needs ew - w <= w - 1 and eh - h <= h - 1)");
  const int tw = ew / tiles_x, th = eh / tiles_y;
  if ((long long)tw * th > kClaheMaxArea) return fail(SSHIP_ERR_INVALID, std::string(who) + ": a tile must hold at most 2^24 pixels");
  const int area = tw * th;
  *k = ClaheK{tiles_x, tiles_y, tw, th, clahe_limit(clip_limit, area), 255.0f / (float)area, 1.0f / (float)tw, 1.0f / (float)th};
  return SSHIP_OK;
}
extern "C" int sship_clahe_create(int h, int w, int tiles_x, int tiles_y, double clip_limit, int max_images, sship_clahe** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "clahe_create: null argument");
  *out = nullptr;
  ClaheK k;
  if (int rc = clahe_geometry(h, w, tiles_x, tiles_y, clip_limit, &k, "clahe_create")) return rc;
  if (max_images < 1 || max_images > 65535) return fail(SSHIP_ERR_INVALID, "clahe_create: max_images must be in [1, 65535]");
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_clahe, void (*)(sship_clahe*)> p(new sship_clahe(), sship_clahe_destroy);
  p->h = h; p->w = w; p->max_images = max_images; p->clip_limit = clip_limit; p->k = k;
  SSHIP_HIP_CHECK(p->luts.ensure(p->image_luts() * max_images));
  SSHIP_HIP_CHECK(hipMemset(p->luts.p, 0, p->image_luts() * max_images));
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&p->stream, hipStreamDefault));
  *out = p.release();
  return SSHIP_OK;
}
extern "C" void sship_clahe_destroy(sship_clahe* clahe) { destroy_handle(clahe); }
extern "C" int sship_clahe_set_clip_limit(sship_clahe* clahe, double clip_limit) {
  if (!clahe) return fail(SSHIP_ERR_INVALID, "clahe_set_clip_limit: null argument");
  if (int rc = clahe_check_clip(clip_limit, "clahe_set_clip_limit")) return rc;
  clahe->clip_limit = clip_limit;
  clahe->k.limit = clahe_limit(clip_limit, clahe->k.tw * clahe->k.th);   // by value into the next call's launches
  return SSHIP_OK;
}
extern "C" int sship_clahe_get_params(const sship_clahe* clahe, int* h, int* w, int* tiles_x, int* tiles_y, double* clip_limit, int* max_images) {
  if (!clahe) return fail(SSHIP_ERR_INVALID, "clahe_get_params: null argument");
  if (h) *h = clahe->h;
  if (w) *w = clahe->w;
  if (tiles_x) *tiles_x = clahe->k.tiles_x;
  if (tiles_y) *tiles_y = clahe->k.tiles_y;
  if (clip_limit) *clip_limit = clahe->clip_limit;
  if (max_images) *max_images = clahe->max_images;
  return SSHIP_OK;
}
// the last call's launches: bit 0 the tables, bit 1 the pixels
static void clahe_launch(const sship_clahe* c, int kernels, hipStream_t s) {
  if (kernels & 1) launch_clahe_lut(c->src, c->src_image_stride, c->src_stride, c->h, c->w, c->k, c->luts.as<uint8_t>(), c->images, s);
  if (kernels & 2)
    launch_clahe_apply(c->src, c->src_image_stride, c->src_stride, c->dst, c->dst_image_stride, c->dst_stride, c->h, c->w, c->k, c->luts.as<uint8_t>(),
                       c->images, s);
}
extern "C" int sship_clahe_apply_batch_device(sship_clahe* clahe, const uint8_t* src, long long src_image_stride, int src_stride, uint8_t* dst,
                                              long long dst_image_stride, int dst_stride, int images, void* stream) {
  if (!clahe || !src || !dst) return fail(SSHIP_ERR_INVALID, "clahe_apply_batch_device: null argument");
  if (images < 1 || images > clahe->max_images) return fail(SSHIP_ERR_INVALID, "clahe_apply_batch_device: images must be in [1, max_images]");
  if (src_stride < clahe->w || dst_stride < clahe->w) return fail(SSHIP_ERR_INVALID, "clahe_apply_batch_device: stride (bytes) must be >= w");
  if (src_image_stride < 0 || dst_image_stride < 0) return fail(SSHIP_ERR_INVALID, "clahe_apply_batch_device: image_stride (bytes) must be >= 0");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  clahe->src = src; clahe->src_image_stride = src_image_stride; clahe->src_stride = src_stride;
  clahe->dst = dst; clahe->dst_image_stride = dst_image_stride; clahe->dst_stride = dst_stride; clahe->images = images;
  clahe_launch(clahe, 3, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("clahe", s);
  return SSHIP_OK;
}
extern "C" int sship_clahe_read_luts(const sship_clahe* clahe, int first, int count, uint8_t* out) {
  if (!clahe || !out) return fail(SSHIP_ERR_INVALID, "clahe_read_luts: null argument");
  if (clahe->images <= 0) return fail(SSHIP_ERR_INVALID, "clahe_read_luts: apply the handle first");
  if (first < 0 || count < 1 || (long long)first + count > clahe->images)
    return fail(SSHIP_ERR_INVALID, "clahe_read_luts: first and count must name images of the last call");
  bind_thread();
  SSHIP_HIP_CHECK(hipDeviceSynchronize());   // the call may have run on the caller's stream
  SSHIP_HIP_CHECK(hipMemcpy(out, clahe->luts.as<uint8_t>() + (size_t)first * clahe->image_luts(), (size_t)count * clahe->image_luts(), hipMemcpyDeviceToHost));
  return SSHIP_OK;
}
extern "C" int sship_clahe_apply_host(const uint8_t* src, int src_stride, int h, int w, int tiles_x, int tiles_y, double clip_limit, uint8_t* dst,
                                      int dst_stride) {
  if (!src || !dst) return fail(SSHIP_ERR_INVALID, "clahe_apply_host: null argument");
  ClaheK k;
  if (int rc = clahe_geometry(h, w, tiles_x, tiles_y, clip_limit, &k, "clahe_apply_host")) return rc;
  if (src_stride < w || dst_stride < w) return fail(SSHIP_ERR_INVALID, "clahe_apply_host: stride (bytes) must be >= w");
  bind_thread();
  if (int rc = require_device()) return rc;
  StageLayout lay;   // one device block for the call: the image packed to stride w, the result likewise, the tables
  const size_t o_src = lay.add((size_t)h * w), o_dst = lay.add((size_t)h * w), o_luts = lay.add((size_t)tiles_x * tiles_y * 256);
  StageArena a;
  SSHIP_HIP_CHECK(a.create(lay.end, 0, false));
  SSHIP_HIP_CHECK(hipMemcpy2D(a.dev<uint8_t>(o_src), (size_t)w, src, (size_t)src_stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice));
  launch_clahe_lut(a.dev<uint8_t>(o_src), 0, w, h, w, k, a.dev<uint8_t>(o_luts), 1, nullptr);
  launch_clahe_apply(a.dev<uint8_t>(o_src), 0, w, a.dev<uint8_t>(o_dst), 0, w, h, w, k, a.dev<uint8_t>(o_luts), 1, nullptr);
  SSHIP_HIP_CHECK(hipGetLastError());
  SSHIP_HIP_CHECK(hipMemcpy2D(dst, (size_t)dst_stride, a.dev<uint8_t>(o_dst), (size_t)w, (size_t)w, (size_t)h, hipMemcpyDeviceToHost));   // blocking, on the NULL stream: after the launches
  return SSHIP_OK;
}
// Measurement hooks (include/sship.h): the last call's launches re-run `iters` times on the handle's stream; kernels: 1 the tables, 2 the
// pixels, 3 both
extern "C" int sship_clahe_bench_kernels(sship_clahe* clahe, int kernels, int iters, float* avg_ms) {
  if (!clahe || !avg_ms || iters <= 0 || kernels < 1 || kernels > 3) return fail(SSHIP_ERR_INVALID, "clahe_bench: bad arguments");
  if (clahe->images <= 0) return fail(SSHIP_ERR_INVALID, "clahe_bench: apply the handle first");
  bind_thread();
  SSHIP_HIP_CHECK(hipDeviceSynchronize());   // the last call may have run on the caller's stream
  return bench_loop(clahe->stream, iters, [&]() { clahe_launch(clahe, kernels, clahe->stream); return hipGetLastError(); }, avg_ms);
}
extern "C" int sship_clahe_bench(sship_clahe* clahe, int iters, float* avg_ms) { return sship_clahe_bench_kernels(clahe, 3, iters, avg_ms); }

// ====================================================================================================
// FAST corners with track refill (sship_fast_*; the rule is in include/sship.h)
// ====================================================================================================
struct sship_fast {
  int h = 0, w = 0, max_kp = 0, max_images = 0, cap = 0, nb_max = 0;
  sship_fast_params p = {};
  hipStream_t stream = nullptr;
  DevBuf cand, counts, new_kp, cells, sel, sel_ws;   // counts: [3][max_images] candidates | selected by the balanced rule | new keypoints
  // the last call
  const uint8_t* imgs = nullptr;
  long long image_stride = 0;
  int stride = 0, images = 0, unit_stride = 1;
  const float* keep = nullptr;
  const int* keep_n = nullptr;
  float* kp_out = nullptr;
  int *n_out = nullptr, *carry0 = nullptr, *n_cand = nullptr;
};
static int fast_check_size(int h, int w, const char* who) {
  if (h < 7 || w < 7 || h > 16384 || w > 16384) return fail(SSHIP_ERR_INVALID, std::string(who) + ": h and w must be in [7, 16384]");
  return SSHIP_OK;
}
static int fast_check_params(const sship_fast_params* p, int max_kp, const char* who) {
  if (p->threshold < 0 || p->threshold > 254) return fail(SSHIP_ERR_INVALID, std::string(who) + ": threshold must be in [0, 254]");
  if (p->border < 3 || p->border > 64) return fail(SSHIP_ERR_INVALID, std::string(who) + ": border must be in [3, 64]");
  if (p->min_distance < 0 || p->min_distance > 32) return fail(SSHIP_ERR_INVALID, std::string(who) + ": min_distance must be in [0, 32]");
  if (p->selection != SSHIP_SELECT_TOPK && p->selection != SSHIP_SELECT_BALANCED)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": selection must be 0 (top-k) or 1 (balanced)");
  if (p->selection == SSHIP_SELECT_BALANCED && (p->bucket_px < 8 || p->bucket_px > 65535))
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": bucket_px must be in [8, 65535]");
  if (p->max_new < 1 || p->max_new > max_kp) return fail(SSHIP_ERR_INVALID, std::string(who) + ": max_new must be in [1, max_keypoints]");
  if (p->target < 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": target must be >= 0 (0: off)");
  return SSHIP_OK;
}
static sship_fast_params fast_default_params(int max_kp) { return sship_fast_params{20, 8, 10, SSHIP_SELECT_TOPK, 32, max_kp, 0}; }
extern "C" int sship_fast_create(int h, int w, int max_keypoints, int max_images, sship_fast** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "fast_create: null argument");
  *out = nullptr;
  if (int rc = fast_check_size(h, w, "fast_create")) return rc;
  if (max_keypoints < 1 || max_keypoints > kMaxKp) return fail(SSHIP_ERR_INVALID, "fast_create: max_keypoints must be in [1, 4096]");
  if (max_images < 1 || max_images > 65535) return fail(SSHIP_ERR_INVALID, "fast_create: max_images must be in [1, 65535]");
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_fast, void (*)(sship_fast*)> f(new sship_fast(), sship_fast_destroy);
  f->h = h; f->w = w; f->max_kp = max_keypoints; f->max_images = max_images; f->p = fast_default_params(max_keypoints);
  f->cap = ((h + 1) / 2) * ((w + 1) / 2);            // no two candidates are 8-neighbours: the list cannot overflow
  f->nb_max = ((h + 7) / 8) * ((w + 7) / 8);         // the buckets of the smallest bucket_px
  const size_t B = (size_t)max_images, mk = (size_t)max_keypoints;
  SSHIP_HIP_CHECK(f->cand.ensure(B * f->cap * 8));
  SSHIP_HIP_CHECK(f->counts.ensure(3 * B * 4));
  SSHIP_HIP_CHECK(f->new_kp.ensure(B * mk * 12));
  SSHIP_HIP_CHECK(f->cells.ensure(2 * B * mk * 4));
  SSHIP_HIP_CHECK(f->sel.ensure(B * mk * 8));
  SSHIP_HIP_CHECK(f->sel_ws.ensure(sel_ws_layout(f->sel_ws, max_images, f->cap, f->nb_max, nullptr)));
  SSHIP_HIP_CHECK(hipMemset(f->counts.p, 0, 3 * B * 4));
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&f->stream, hipStreamDefault));
  *out = f.release();
  return SSHIP_OK;
}
extern "C" void sship_fast_destroy(sship_fast* fast) { destroy_handle(fast); }
extern "C" int sship_fast_set_params(sship_fast* fast, const sship_fast_params* p) {
  if (!fast || !p) return fail(SSHIP_ERR_INVALID, "fast_set_params: null argument");
  if (int rc = fast_check_params(p, fast->max_kp, "fast_set_params")) return rc;
  fast->p = *p;   // by value into the next call's launches
  return SSHIP_OK;
}
extern "C" int sship_fast_get_params(const sship_fast* fast, sship_fast_params* p, int* h, int* w, int* max_keypoints, int* max_images) {
  if (!fast) return fail(SSHIP_ERR_INVALID, "fast_get_params: null argument");
  if (p) *p = fast->p;
  if (h) *h = fast->h;
  if (w) *w = fast->w;
  if (max_keypoints) *max_keypoints = fast->max_kp;
  if (max_images) *max_images = fast->max_images;
  return SSHIP_OK;
}
// the last call's launches: bit 0 k_fast_detect (and the clearing of its counters), bit 1 the selection (k_select_balanced in that mode,
// k_topk), bit 2 k_fast_merge
static hipError_t fast_launch(const sship_fast* f, int kernels, hipStream_t s) {
  const int B = f->images, mk = f->max_kp;
  const sship_fast_params& p = f->p;
  int* cand_count = f->counts.as<int>();
  int* sel_count = cand_count + f->max_images;
  int* n_new = sel_count + f->max_images;
  if (kernels & 1) {
    if (hipError_t e = hipMemsetAsync(cand_count, 0, (size_t)B * 4, s)) return e;
    const FastK c{f->h, f->w, (f->w + kFastTileW - 1) / kFastTileW, (f->h + kFastTileH - 1) / kFastTileH, p.threshold, p.border, f->cap,
                  p.min_distance, mk, f->unit_stride};
    launch_fast_detect(f->imgs, f->image_stride, f->stride, c, f->keep, f->keep_n, f->cand.as<unsigned long long>(), cand_count, B, s);
  }
  if (kernels & 2) {
    TopkArgs t{};
    t.cand = f->cand.as<unsigned long long>(); t.cand_count = cand_count; t.cap = f->cap; t.max_kp = p.max_new; t.score_w = f->w;
    t.scale_x = 1.f; t.scale_y = 1.f; t.desc_h = 1; t.desc_w = 1;
    t.kp_xys = f->new_kp.as<float>(); t.cell_h = f->cells.as<int>(); t.cell_w = f->cells.as<int>() + (size_t)f->max_images * mk;
    t.n_out = n_new; t.n_cand_out = f->n_cand; t.reset_count = nullptr; t.pix = nullptr;
    if (p.selection == SSHIP_SELECT_BALANCED) {
      SelWs ws;
      sel_ws_layout(f->sel_ws, f->max_images, f->cap, f->nb_max, &ws);
      SelectBalancedArgs q = select_balanced_args(t.cand, cand_count, f->cap, p.max_new, f->h, f->w, p.bucket_px, f->sel.as<unsigned long long>(),
                                                  sel_count, ws);
      q.n_cand_out = f->n_cand;
      if (hipError_t e = launch_select_balanced(q, B, s)) return e;
      t.cand = q.sel; t.cand_count = q.sel_count; t.cap = p.max_new; t.n_cand_out = nullptr;
    }
    launch_topk(t, B, s);
  }
  if (kernels & 4)
    launch_fast_merge(f->keep, f->keep_n, f->unit_stride, mk, f->new_kp.as<float>(), n_new, p.max_new, p.target, f->kp_out, f->n_out, f->carry0, B, s);
  return hipGetLastError();
}
extern "C" int sship_fast_detect_batch_device(sship_fast* fast, const uint8_t* imgs, long long image_stride, int stride, int images,
                                              const float* keep, const int* keep_n, int unit_stride, float* kp_out, int* n_out,
                                              int32_t* carry0, int* n_candidates, void* stream) {
  const char* who = "fast_detect_batch_device";
  if (!fast || !imgs || !kp_out || !n_out) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (images < 1 || images > fast->max_images) return fail(SSHIP_ERR_INVALID, std::string(who) + ": images must be in [1, max_images]");
  if (stride < fast->w) return fail(SSHIP_ERR_INVALID, std::string(who) + ": stride (bytes) must be >= w");
  if (image_stride < 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": image_stride (bytes) must be >= 0");
  if (keep) {
    if (!keep_n) return fail(SSHIP_ERR_INVALID, std::string(who) + ": keep needs keep_n");
    if (unit_stride != 1 && unit_stride != 2) return fail(SSHIP_ERR_INVALID, std::string(who) + ": unit_stride must be 1 or 2");
    // the merge of one image reads rows another image's merge may already have written: refused, not ordered
    const size_t unit = (size_t)fast->max_kp * 12;
    const char *k0 = reinterpret_cast<const char*>(keep), *k1 = k0 + ((size_t)(images - 1) * unit_stride + 1) * unit;
    const char *o0 = reinterpret_cast<const char*>(kp_out), *o1 = o0 + (size_t)images * unit;
    if (k0 < o1 && o0 < k1) return fail(SSHIP_ERR_INVALID, std::string(who) + ": keep must not overlap kp_out");
  }
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  fast->imgs = imgs; fast->image_stride = image_stride; fast->stride = stride; fast->images = images;
  fast->keep = keep; fast->keep_n = keep ? keep_n : nullptr; fast->unit_stride = keep ? unit_stride : 1;
  fast->kp_out = kp_out; fast->n_out = n_out; fast->carry0 = carry0; fast->n_cand = n_candidates;
  SSHIP_HIP_CHECK(fast_launch(fast, 7, s));
  g_timer.mark("fast_detect", s);
  return SSHIP_OK;
}
extern "C" int sship_fast_detect_host(const uint8_t* img, int stride, int h, int w, int max_keypoints, const sship_fast_params* p,
                                      const float* keep, int keep_stride, int n_keep, float* kp_out, int* n_out, int32_t* carry0,
                                      int* n_candidates) {
  const char* who = "fast_detect_host";
  if (!img || !p || !kp_out || !n_out) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (int rc = fast_check_size(h, w, who)) return rc;
  if (max_keypoints < 1 || max_keypoints > kMaxKp) return fail(SSHIP_ERR_INVALID, std::string(who) + ": max_keypoints must be in [1, 4096]");
  if (int rc = fast_check_params(p, max_keypoints, who)) return rc;
  if (stride < w) return fail(SSHIP_ERR_INVALID, std::string(who) + ": stride (bytes) must be >= w");
  if (keep && (n_keep < 0 || n_keep > max_keypoints || keep_stride < 3))
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": with keep, n_keep must be in [0, max_keypoints] and keep_stride >= 3");
  bind_thread();
  if (int rc = require_device()) return rc;
  sship_fast* raw = nullptr;
  if (int rc = sship_fast_create(h, w, max_keypoints, 1, &raw)) return rc;
  std::unique_ptr<sship_fast, void (*)(sship_fast*)> f(raw, sship_fast_destroy);
  raw->p = *p;
  const FastStage st = fast_stage(h, w, max_keypoints);
  std::vector<char> tail(st.tail_bytes, 0);
  fast_pack(tail.data(), st, keep, keep_stride, keep ? n_keep : 0);
  StageArena a;
  SSHIP_HIP_CHECK(a.create(st.in_bytes, st.out_bytes, false));
  SSHIP_HIP_CHECK(hipMemcpy2D(a.dev<uint8_t>(st.img), (size_t)w, img, (size_t)stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice));
  SSHIP_HIP_CHECK(hipMemcpy(a.dev<char>(st.n), tail.data(), st.tail_bytes, hipMemcpyHostToDevice));
  if (int rc = sship_fast_detect_batch_device(raw, a.dev<uint8_t>(st.img), 0, w, 1, keep ? a.dev<float>(st.keep) : nullptr, a.dev<int>(st.n), 1,
                                              a.dev<float>(a.out + st.kp), a.dev<int>(a.out + st.counts), a.dev<int32_t>(a.out + st.carry),
                                              a.dev<int>(a.out + st.counts) + 1, nullptr)) return rc;
  std::vector<char> back(st.out_bytes);
  SSHIP_HIP_CHECK(hipMemcpy(back.data(), a.dev<char>(a.out), st.out_bytes, hipMemcpyDeviceToHost));   // blocking, on the NULL stream: after the launches
  fast_unpack(back.data(), st, kp_out, n_out, carry0, n_candidates);
  return SSHIP_OK;
}
extern "C" int sship_fast_score_batch_device(const uint8_t* imgs, long long image_stride, int stride, int images, int h, int w, uint8_t* score,
                                             long long score_image_stride, int score_stride, void* stream) {
  const char* who = "fast_score_batch_device";
  if (!imgs || !score) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (int rc = fast_check_size(h, w, who)) return rc;
  if (images < 1 || images > 65535) return fail(SSHIP_ERR_INVALID, std::string(who) + ": images must be in [1, 65535]");
  if (stride < w || score_stride < w) return fail(SSHIP_ERR_INVALID, std::string(who) + ": stride (bytes) must be >= w");
  if (image_stride < 0 || score_image_stride < 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": image_stride (bytes) must be >= 0");
  bind_thread();
  if (int rc = require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_fast_score(imgs, image_stride, stride, h, w, score, score_image_stride, score_stride, images, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("fast_score", s);
  return SSHIP_OK;
}
// Measurement hooks (include/sship.h): the last call's launches re-run `iters` times on the handle's stream; kernels as at fast_launch
extern "C" int sship_fast_bench_kernels(sship_fast* fast, int kernels, int iters, float* avg_ms) {
  if (!fast || !avg_ms || iters <= 0 || kernels < 1 || kernels > 7) return fail(SSHIP_ERR_INVALID, "fast_bench: bad arguments");
  if (fast->images <= 0) return fail(SSHIP_ERR_INVALID, "fast_bench: detect with the handle first");
  bind_thread();
  SSHIP_HIP_CHECK(hipDeviceSynchronize());   // the last call may have run on the caller's stream
  return bench_loop(fast->stream, iters, [&]() { return fast_launch(fast, kernels, fast->stream); }, avg_ms);
}
extern "C" int sship_fast_bench(sship_fast* fast, int iters, float* avg_ms) { return sship_fast_bench_kernels(fast, 7, iters, avg_ms); }

// ====================================================================================================
// Steered BRIEF descriptors and the Hamming matcher (sship_brief_*, sship_hm_*; the rules are in include/sship.h)
// ====================================================================================================
extern "C" int sship_brief_pattern(int bin, int8_t* out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "brief_pattern: null argument");
  if (bin < 0 || bin >= kBriefBins) return fail(SSHIP_ERR_INVALID, "brief_pattern: bin must be in [0, 31]");
  memcpy(out, brief_table_host().v[bin], (size_t)kBriefBits * 4);
  return SSHIP_OK;
}
static int brief_check(int stride, int h, int w, int mode, const char* who) {
  if (h < 2 * kBriefReach + 1 || w < 2 * kBriefReach + 1 || h > 16384 || w > 16384)
    return fail(SSHIP_ERR_INVALID, std::string(who) + ": h and w must be in [33, 16384]");
  if (stride < w) return fail(SSHIP_ERR_INVALID, std::string(who) + ": stride (bytes) must be >= w");
  if (mode != SSHIP_BRIEF_STEERED && mode != SSHIP_BRIEF_UPRIGHT) return fail(SSHIP_ERR_INVALID, std::string(who) + ": mode must be 0 (steered) or 1 (upright)");
  return SSHIP_OK;
}
extern "C" int sship_brief_describe_batch_device(const uint8_t* imgs, long long image_stride, int stride, int images, int h, int w,
                                                 const float* kp, const int* n, int unit_stride, int max_keypoints, int mode, uint32_t* desc,
                                                 uint8_t* status, uint8_t* bin, void* stream) {
  const char* who = "brief_describe_batch_device";
  if (!imgs || !kp || !n || !desc) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (images < 1 || images > 65535) return fail(SSHIP_ERR_INVALID, std::string(who) + ": images must be in [1, 65535]");
  if (max_keypoints < 1 || max_keypoints > kMaxKp) return fail(SSHIP_ERR_INVALID, std::string(who) + ": max_keypoints must be in [1, 4096]");
  if (unit_stride != 1 && unit_stride != 2) return fail(SSHIP_ERR_INVALID, std::string(who) + ": unit_stride must be 1 or 2");
  if (image_stride < 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": image_stride (bytes) must be >= 0");
  if (int rc = brief_check(stride, h, w, mode, who)) return rc;
  bind_thread();
  if (int rc = require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  launch_brief_describe(imgs, image_stride, stride, images, h, w, kp, n, unit_stride, max_keypoints, mode, desc, status, bin, s);
  SSHIP_HIP_CHECK(hipGetLastError());
  g_timer.mark("brief_describe", s);
  return SSHIP_OK;
}
extern "C" int sship_brief_describe_host(const uint8_t* img, int stride, int h, int w, const float* keypoints, int kp_stride, int n, int mode,
                                         uint32_t* desc, uint8_t* status, uint8_t* bin) {
  const char* who = "brief_describe_host";
  if (!img) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (n < 0 || n > kMaxKp || kp_stride < 2) return fail(SSHIP_ERR_INVALID, std::string(who) + ": n must be in [0, 4096] and kp_stride >= 2");
  if (int rc = brief_check(stride, h, w, mode, who)) return rc;
  if (n == 0) return SSHIP_OK;
  if (!keypoints || !desc) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  bind_thread();
  if (int rc = require_device()) return rc;
  const BriefStage st = brief_stage(h, w, n);
  std::vector<char> tail(st.tail_bytes, 0);
  brief_pack(tail.data(), st, keypoints, kp_stride, n);
  StageArena a;
  SSHIP_HIP_CHECK(a.create(st.in_bytes, st.out_bytes, false));
  SSHIP_HIP_CHECK(hipMemcpy2D(a.dev<uint8_t>(st.img), (size_t)w, img, (size_t)stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice));
  SSHIP_HIP_CHECK(hipMemcpy(a.dev<char>(st.n), tail.data(), st.tail_bytes, hipMemcpyHostToDevice));
  if (int rc = sship_brief_describe_batch_device(a.dev<uint8_t>(st.img), 0, w, 1, h, w, a.dev<float>(st.kp), a.dev<int>(st.n), 1, n, mode,
                                                 a.dev<uint32_t>(a.out + st.desc), a.dev<uint8_t>(a.out + st.status),
                                                 a.dev<uint8_t>(a.out + st.bin), nullptr)) return rc;
  std::vector<char> back(st.out_bytes);
  SSHIP_HIP_CHECK(hipMemcpy(back.data(), a.dev<char>(a.out), st.out_bytes, hipMemcpyDeviceToHost));   // blocking, on the NULL stream: after the launch
  brief_unpack(back.data(), st, n, desc, status, bin);
  return SSHIP_OK;
}

struct sship_hm {
  int max_kp = 0, max_pairs = 0;
  int max_distance = 0, ratio_percent = 0, mutual = 1;
  int gate_on = 0;                                              // sship_nn's gate: (dx_lo, dx_hi, dy_lo, dy_hi)
  float gate[4] = {-INFINITY, INFINITY, -INFINITY, INFINITY};
  hipStream_t stream = nullptr;
  DevBuf ws;
  StageArena one;   // sship_hm_match_host: one staged pair and its results (hm_stage)
  // the last call's launch arguments (sship_hm_bench re-runs them; the caller keeps a batch call's buffers alive until then)
  struct Last { const int* n = nullptr; const uint32_t* desc = nullptr; const uint8_t* status = nullptr; const float* kp = nullptr;
                int first0 = 0, step0 = 0, first1 = 0, step1 = 0, items = 0; int32_t* m0 = nullptr; int32_t* dist0 = nullptr; float* ms0 = nullptr; } last;
};
extern "C" int sship_hm_create(int max_kp, int max_pairs, sship_hm** out) {
  if (!out) return fail(SSHIP_ERR_INVALID, "hm_create: null argument");
  *out = nullptr;
  if (max_kp < 1 || max_kp > kMaxKp) return fail(SSHIP_ERR_INVALID, "hm_create: max_keypoints must be in [1, 4096]");
  if (max_pairs < 1 || max_pairs > 65535) return fail(SSHIP_ERR_INVALID, "hm_create: max_pairs must be in [1, 65535]");
  bind_thread();
  if (int rc = require_device()) return rc;
  std::unique_ptr<sship_hm, void (*)(sship_hm*)> hm(new sship_hm(), sship_hm_destroy);
  hm->max_kp = max_kp; hm->max_pairs = max_pairs;
  SSHIP_HIP_CHECK(hm->ws.ensure(hm_workspace_ints(max_kp, max_pairs) * 4));
  const HmStage st = hm_stage(max_kp);
  SSHIP_HIP_CHECK(hm->one.create(st.in_bytes, st.out_bytes));
  SSHIP_HIP_CHECK(hipMemset(hm->one.dev<char>(0), 0, st.in_bytes));   // rows never staged are zero
  SSHIP_HIP_CHECK(hipStreamCreateWithFlags(&hm->stream, hipStreamDefault));
  *out = hm.release();
  return SSHIP_OK;
}
extern "C" void sship_hm_destroy(sship_hm* hm) { destroy_handle(hm); }
extern "C" int sship_hm_set_params(sship_hm* hm, int max_distance, int ratio_percent, int mutual_check) {
  if (!hm) return fail(SSHIP_ERR_INVALID, "hm_set_params: null handle");
  if (max_distance < 0 || max_distance > 256) return fail(SSHIP_ERR_INVALID, "hm_set_params: max_distance must be in [0, 256] (0: off)");
  if (ratio_percent < 0 || ratio_percent > 100) return fail(SSHIP_ERR_INVALID, "hm_set_params: ratio_percent must be in [0, 100] (0: off)");
  hm->max_distance = max_distance; hm->ratio_percent = ratio_percent; hm->mutual = mutual_check ? 1 : 0;
  return SSHIP_OK;
}
extern "C" int sship_hm_get_params(const sship_hm* hm, int* max_distance, int* ratio_percent, int* mutual_check, int* max_keypoints, int* max_pairs) {
  if (!hm) return fail(SSHIP_ERR_INVALID, "hm_get_params: null handle");
  if (max_distance) *max_distance = hm->max_distance;
  if (ratio_percent) *ratio_percent = hm->ratio_percent;
  if (mutual_check) *mutual_check = hm->mutual;
  if (max_keypoints) *max_keypoints = hm->max_kp;
  if (max_pairs) *max_pairs = hm->max_pairs;
  return SSHIP_OK;
}
extern "C" int sship_hm_set_gate(sship_hm* hm, int enabled, float dx_lo, float dx_hi, float dy_lo, float dy_hi) {
  if (!hm) return fail(SSHIP_ERR_INVALID, "hm_set_gate: null handle");
  if (std::isnan(dx_lo) || std::isnan(dx_hi) || std::isnan(dy_lo) || std::isnan(dy_hi)) return fail(SSHIP_ERR_INVALID, "hm_set_gate: a bound is NaN");
  if (dx_lo > dx_hi || dy_lo > dy_hi) return fail(SSHIP_ERR_INVALID, "hm_set_gate: lo > hi");
  hm->gate_on = enabled ? 1 : 0;
  hm->gate[0] = dx_lo; hm->gate[1] = dx_hi; hm->gate[2] = dy_lo; hm->gate[3] = dy_hi;
  return SSHIP_OK;
}
extern "C" int sship_hm_get_gate(const sship_hm* hm, int* enabled, float* dx_lo, float* dx_hi, float* dy_lo, float* dy_hi) {
  if (!hm) return fail(SSHIP_ERR_INVALID, "hm_get_gate: null handle");
  if (enabled) *enabled = hm->gate_on;
  if (dx_lo) *dx_lo = hm->gate[0];
  if (dx_hi) *dx_hi = hm->gate[1];
  if (dy_lo) *dy_lo = hm->gate[2];
  if (dy_hi) *dy_hi = hm->gate[3];
  return SSHIP_OK;
}
// kp == nullptr: the ungated launches; otherwise the gated ones with the handle's window
static hipError_t hm_run(const sship_hm* hm, const sship_hm::Last& l, hipStream_t s) {
  HmK c{hm->max_kp, hm->max_distance, hm->ratio_percent, hm->mutual, l.kp ? 1 : 0, {hm->gate[0], hm->gate[1], hm->gate[2], hm->gate[3]},
        l.first0, l.step0, l.first1, l.step1};
  launch_hm_match(l.n, l.desc, l.status, l.kp, c, l.items, hm->ws.as<int>(), l.m0, l.dist0, l.ms0, s);
  return hipGetLastError();
}
extern "C" int sship_hm_match_batch_device(sship_hm* hm, const int* n, const uint32_t* desc, const uint8_t* status, const float* kp, int first0,
                                           int step0, int first1, int step1, int pairs, int32_t* m0, int32_t* dist0, float* ms0, void* stream) {
  const char* who = "hm_match_batch_device";
  if (!hm || !n || !desc || !m0 || !dist0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (pairs < 1 || pairs > hm->max_pairs) return fail(SSHIP_ERR_INVALID, std::string(who) + ": pairs must be in [1, max_pairs]");
  if (first0 < 0 || step0 < 0 || first1 < 0 || step1 < 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": firsts and steps must be >= 0");
  if (reinterpret_cast<uintptr_t>(desc) % 16 != 0) return fail(SSHIP_ERR_INVALID, std::string(who) + ": desc_dev must be 16-byte aligned");
  if (hm->gate_on && !kp) return fail(SSHIP_ERR_INVALID, std::string(who) + ": the gate is enabled and kp_dev is NULL");
  bind_thread();
  hipStream_t s = static_cast<hipStream_t>(stream);
  g_timer.begin_if_idle(s);
  hm->last = {n, desc, status, hm->gate_on ? kp : nullptr, first0, step0, first1, step1, pairs, m0, dist0, ms0};
  SSHIP_HIP_CHECK(hm_run(hm, hm->last, s));
  g_timer.mark(hm->gate_on ? "hm_match_gated" : "hm_match", s);
  return SSHIP_OK;
}
extern "C" int sship_hm_match_host(sship_hm* hm, int n0, const uint32_t* desc0, const uint8_t* status0, const float* kp0, int kp_stride0, int n1,
                                   const uint32_t* desc1, const uint8_t* status1, const float* kp1, int kp_stride1, int32_t* matches0,
                                   int32_t* dist0, float* mscores0) {
  const char* who = "hm_match_host";
  if (!hm) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null handle");
  if (n0 < 0 || n1 < 0 || n0 > hm->max_kp || n1 > hm->max_kp) return fail(SSHIP_ERR_INVALID, std::string(who) + ": n0 and n1 must be in [0, max_keypoints]");
  if ((n0 && (!desc0 || !matches0 || !dist0)) || (n1 && !desc1)) return fail(SSHIP_ERR_INVALID, std::string(who) + ": null argument");
  if (hm->gate_on) {
    if ((n0 && !kp0) || (n1 && !kp1)) return fail(SSHIP_ERR_INVALID, std::string(who) + ": the gate is enabled and a keypoint pointer is NULL");
    if (kp_stride0 < 2 || kp_stride1 < 2) return fail(SSHIP_ERR_INVALID, std::string(who) + ": kp_stride must be >= 2");
  }
  if (n0 == 0) return SSHIP_OK;
  bind_thread();
  hipStream_t s = hm->stream;
  const StageArena& a = hm->one;
  const HmStage st = hm_stage(hm->max_kp);
  hm_pack(a.host<char>(0), st, n0, desc0, status0, n1, desc1, status1);
  SSHIP_HIP_CHECK(a.upload(st.lens, 8, s));
  SSHIP_HIP_CHECK(a.upload(st.desc, (size_t)n0 * 32, s));
  SSHIP_HIP_CHECK(a.upload(st.status, (size_t)n0, s));
  if (n1) { SSHIP_HIP_CHECK(a.upload(st.desc1, (size_t)n1 * 32, s)); SSHIP_HIP_CHECK(a.upload(st.status1, (size_t)n1, s)); }
  if (hm->gate_on) {
    hm_pack_kp(a.host<char>(0), st, kp0, kp_stride0, n0, kp1, kp_stride1, n1);
    SSHIP_HIP_CHECK(a.upload(st.kp, (size_t)n0 * 12, s));
    if (n1) SSHIP_HIP_CHECK(a.upload(st.kp1, (size_t)n1 * 12, s));
  }
  // the arena as two units of one array each: set 0 is unit 0, set 1 is unit 1
  if (int rc = sship_hm_match_batch_device(hm, a.dev<int>(st.lens), a.dev<uint32_t>(st.desc), a.dev<uint8_t>(st.status),
                                           hm->gate_on ? a.dev<float>(st.kp) : nullptr, 0, 0, 1, 0, 1, a.dev<int32_t>(a.out + st.m0),
                                           a.dev<int32_t>(a.out + st.dist0), a.dev<float>(a.out + st.ms0), s)) return rc;
  SSHIP_HIP_CHECK(a.download(a.out + st.m0, (size_t)n0 * 4, s));
  SSHIP_HIP_CHECK(a.download(a.out + st.dist0, (size_t)n0 * 4, s));
  SSHIP_HIP_CHECK(a.download(a.out + st.ms0, (size_t)n0 * 4, s));
  SSHIP_HIP_CHECK(hipStreamSynchronize(s));
  hm_unpack(a.host<char>(a.out), st, n0, matches0, dist0, mscores0);
  return SSHIP_OK;
}
// Measurement hook (include/sship.h): the last call's two launches re-run `iters` times on the handle's stream
extern "C" int sship_hm_bench(sship_hm* hm, int iters, float* avg_ms) { return bench_last(hm, iters, avg_ms, "hm_bench", "match", hm_run); }

// ====================================================================================================
// fused front-end step: SuperPoint(batch 2P) + select + gather + LightGlue(P)
// ====================================================================================================
extern "C" int sship_frontend_batch_device(sship_sp* sp, sship_lg* lg, const uint8_t* imgs, int pairs, int h, int w,
                                           void* desc_out, float* kp_out, int* n_out, int32_t* m0, float* ms0,
                                           void* stream) {
  bind_thread();
  if (!sp || !lg || !imgs || !desc_out || !kp_out || !n_out || !m0 || !ms0) return fail(SSHIP_ERR_INVALID, "frontend_batch_device: null argument");
  if (pairs <= 0 || pairs > lg->max_pairs) return fail(SSHIP_ERR_INVALID, "frontend_batch_device: pairs exceeds the matcher's max_pairs");
  if (sp->cfg.max_keypoints != lg->max_kp) return fail(SSHIP_ERR_INVALID, "frontend_batch_device: extractor and matcher disagree on max_keypoints");
  hipStream_t s = static_cast<hipStream_t>(stream);  // one stream for the extractor and the matcher; NULL = legacy default stream
  if (int rc = sship_sp_extract_batch_device(sp, imgs, 2 * pairs, h, w, desc_out, kp_out, n_out, s)) return rc;
  return lg_forward(lg, kp_out, 3, lg->max_kp * 3, n_out, static_cast<const _Float16*>(desc_out), (size_t)lg->max_kp * 256,
                    pairs, m0, ms0, s);
}
