// SuperPoint's 1x1 layers on the implicit-GEMM template (igemm.h) and the fused descriptor head.
// (The 3x3 layers live in conv_strip.hip / conv_pp.hip.)
//   convDb : 1x1 256->256, raw fp16 - dense grid only for sship_sp_dense; extraction uses k_desc_head_gather below
//   convPb : 1x1 256->65, fp32 logits in a 68-wide row (softmax happens in the heatmap kernel): k_convpb_stream below
// reference: utils/convert_superpoint_to_onnx.py:38-64,77,88.
#include <cstdlib>
#include <string>

#include "igemm.h"
#include "kernels.h"

namespace sship {

static IgemmArgs conv_args(const ConvW& w, const _Float16* in, int B, int H, int W) {
  IgemmArgs a{};
  a.in0 = in; a.in1 = in; a.cin0 = w.cin; a.cs0 = w.cin; a.cs1 = w.cin;
  a.wpack = w.w; a.bias = w.bias; a.B = B; a.H = H; a.W = W; a.cout = w.cout; a.ostride = w.cout;
  return a;
}

hipError_t sp_conv1x1_f16(const ConvW& w, const _Float16* in, _Float16* out, int B, int H, int W, hipStream_t s) {
  IgemmArgs a = conv_args(w, in, B, H, W);
  a.out0 = out;
  if (w.cin != 256) return hipErrorInvalidValue;
  return launch_igemm<1, 256, 128, 4, EpiF16<false, false>>(a, w.cout_pad, s);
}

// ---------------------------------------------------------------------------------------------------
// convPb as a streaming kernel: 1x1, 256 -> 65, fp32 logits.  The layer is HBM-bound (4.1 MB of fp16 in, 2.2 MB of fp32
// out per image, 1.06 GFLOP) and the implicit-GEMM template spent its time on two barriers per 64-channel stage and on
// re-staging 48 KB of weights per 128-pixel workgroup.  Here no operand goes through LDS but one weight M-tile:
//   * v_mfma_f32_16x16x32_f16 with the pixels as the N operand: lane l holds 8 consecutive channels (k-block l >> 4) of
//     pixel l & 15, i.e. a B fragment is a plain 16-byte global load and the four lanes of a pixel cover one 64-byte
//     sector per instruction; a 16-pixel tile is 8 loads per lane, prefetched one tile ahead into a second register set;
//   * the weights of output rows 0..63 live in registers for the whole kernel (4 M-tiles x 8 k-steps = 128 VGPRs,
//     read once per wave), the fifth M-tile (row 64 = the dustbin channel, rows 65..79 zero) comes from LDS (8 KiB);
//   * the accumulators start from the bias (LDS); a lane ends up with 4 consecutive channels of its pixel per M-tile;
//   * the 16 x 68 logits of a tile go through a wave-private LDS patch (4 352 B, no workgroup barrier) and leave as lane-linear
//     16-byte stores: with 68-float rows a tile is ONE contiguous block of 34 full 128-byte lines, 4.25 wave-stores.  (The
//     accumulator layout as it stands gives seventeen 64-byte pieces at a 272-byte stride per tile; that store path,
//     WHOLE = false, is kept in the developer build: SUPERSLAM_HIP_CONVPB=pieces.)  Floats 65..67 of a row are padding and
//     are written as zeros; nothing reads them (k_nms_tile, k_kp_refine and k_logits_chw read channels 0..64).
// 40 MFMAs (640 matrix-pipe clocks) per 16 pixels against ~1.3 KB of HBM traffic per pixel: memory-bound by design.
// ---------------------------------------------------------------------------------------------------
typedef float f4x_t __attribute__((ext_vector_type(4)));
// orders a wave's own LDS stores and loads across its lanes (a wave-private patch needs no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <bool WHOLE>
__global__ __launch_bounds__(256, 2) void k_convpb_stream(const _Float16* __restrict__ in, const _Float16* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ out, int P,
                                                          int ostride) {
  __shared__ __attribute__((aligned(16))) _Float16 s_a4[8 * 512];  // A fragments of M-tile 4, [k-step][lane][8]
  const int lane = threadIdx.x & 63, n = lane & 15, kb = lane >> 4;
  for (int u = threadIdx.x; u < 8 * 64; u += 256) {
    const int ks = u >> 6, l = u & 63;
    *reinterpret_cast<uint4*>(s_a4 + u * 8) = *reinterpret_cast<const uint4*>(w + (size_t)(64 + (l & 15)) * 256 + ks * 32 + (l >> 4) * 8);
  }
  h8_t a[4][8];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) a[m][ks] = *reinterpret_cast<const h8_t*>(w + (size_t)(16 * m + n) * 256 + ks * 32 + kb * 8);
  __shared__ __attribute__((aligned(16))) float s_b[80];  // bias, rows 65..79 zero: the accumulators start from it
  if (threadIdx.x < 80) s_b[threadIdx.x] = threadIdx.x < 65 ? bias[threadIdx.x] : 0.f;
  __shared__ __attribute__((aligned(16))) float s_o[WHOLE ? 4 * 16 * 68 : 4];  // per wave: the logits of one tile, [16][68]
  float* patch = s_o + (WHOLE ? (threadIdx.x >> 6) * (16 * 68) : 0);
  __syncthreads();
  const int ntiles = (P + 15) >> 4, nwaves = gridDim.x * 4;
  const _Float16* src = in + kb * 8;
  h8_t fA[8], fB[8];
  auto fetch = [&](h8_t (&f)[8], int t) __attribute__((always_inline)) {
    const int pix = min(min(t, ntiles - 1) * 16 + n, P - 1);  // clamped: a prefetch past the end re-reads a valid pixel
    const _Float16* p = src + (size_t)pix * 256;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) f[ks] = *reinterpret_cast<const h8_t*>(p + ks * 32);
  };
  auto tile = [&](const h8_t (&f)[8], int t) __attribute__((always_inline)) {
    f4x_t acc[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) acc[m] = *reinterpret_cast<const f4x_t*>(s_b + 16 * m + 4 * kb);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const h8_t a4 = *reinterpret_cast<const h8_t*>(s_a4 + (ks * 64 + lane) * 8);
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[m][ks], f[ks], acc[m], 0, 0, 0);
      acc[4] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a4, f[ks], acc[4], 0, 0, 0);
    }
    if constexpr (WHOLE) {
      wave_lds_sync();  // the previous tile's patch reads are done
#pragma unroll
      for (int m = 0; m < 4; ++m) *reinterpret_cast<f4x_t*>(patch + n * 68 + 16 * m + 4 * kb) = acc[m];
      if (kb == 0) *reinterpret_cast<f4x_t*>(patch + n * 68 + 64) = f4x_t{acc[4][0], 0.f, 0.f, 0.f};
      wave_lds_sync();
      const int units = 17 * min(16, P - t * 16);  // 16-byte units of the valid rows (ragged last tile: fewer than 16)
      float* o = out + (size_t)t * (16 * 68);      // ostride == 68 (the launcher): the tile is one block, laid out as the patch is
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int u = i * 64 + lane;
        if (u < units) *reinterpret_cast<f4x_t*>(o + 4 * u) = *reinterpret_cast<const f4x_t*>(patch + 4 * u);
      }
    } else {
      const int pix = t * 16 + n;
      if (pix < P) {
        float* o = out + (size_t)pix * ostride + 4 * kb;
#pragma unroll
        for (int m = 0; m < 4; ++m) *reinterpret_cast<f4x_t*>(o + 16 * m) = acc[m];
        if (kb == 0) o[64] = acc[4][0];
      }
    }
  };
  const int t0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  fetch(fA, t0);
  for (int t = t0; t < ntiles; t += 2 * nwaves) {
    fetch(fB, t + nwaves);
    __builtin_amdgcn_sched_barrier(0);  // the prefetch stays above this tile's MFMAs
    tile(fA, t);
    if (t + nwaves < ntiles) {
      fetch(fA, t + 2 * nwaves);
      __builtin_amdgcn_sched_barrier(0);
      tile(fB, t + nwaves);
    }
  }
}

// w.w_q: the plain fp16 weight matrix [80][256] (rows 65..79 zero), w.bias: [>= 80] floats
hipError_t sp_conv1x1_f32(const ConvW& w, const _Float16* in, float* out, int ostride, int B, int H, int W,
                          hipStream_t s) {
  if (w.cin != 256) return hipErrorInvalidValue;
  static const bool use_igemm = dev_env("SUPERSLAM_HIP_CONVPB") && std::string(dev_env("SUPERSLAM_HIP_CONVPB")) == "igemm";  // A/B (developer build)
  if (w.w_q && w.cout == 65 && ostride >= 68 && ostride % 4 == 0 && !use_igemm) {
    const int P = B * H * W;
    int wgs = 2 * cu_count();
    if (wgs * 4 > (P + 15) / 16) wgs = ((P + 15) / 16 + 3) / 4;
#if SSHIP_DEV_SWITCHES  // A/B and the bit-exact oracle of the whole-tile stores: one 64-byte piece per pixel and M-tile
    static const bool pieces = dev_env("SUPERSLAM_HIP_CONVPB") && std::string(dev_env("SUPERSLAM_HIP_CONVPB")) == "pieces";
    if (pieces) {
      hipLaunchKernelGGL(k_convpb_stream<false>, dim3(wgs), dim3(256), 0, s, in, w.w_q, w.bias, out, P, ostride);
      return hipGetLastError();
    }
#endif
    if (ostride != 68) return hipErrorInvalidValue;  // whole-tile stores: a tile's rows are contiguous (sship_sp_* passes kLogitStride = 68)
    hipLaunchKernelGGL(k_convpb_stream<true>, dim3(wgs), dim3(256), 0, s, in, w.w_q, w.bias, out, P, ostride);
    return hipGetLastError();
  }
#if SSHIP_DEV_SWITCHES
  IgemmArgs a = conv_args(w, in, B, H, W);
  a.out0 = out; a.ostride = ostride;
  return launch_igemm<1, 256, 96, 4, EpiF32>(a, w.cout_pad, s);  // 65 rows: three M-tiles, not four
#else
  return hipErrorInvalidValue;  // one path per layer: the detector's 1x1 is k_convpb_stream (sship_sp_create always uploads its matrix)
#endif
}

// ---------------------------------------------------------------------------------------------------
// Descriptor head at the selected keypoints only: convDb (1x1, 256 -> 256) + F.normalize + the gather's
// renormalisation, evaluated for the <= max_keypoints cells the top-k picked instead of all Hc*Wc cells
// (600 of 8084 at KITTI size: 13x less convDb work, and the dense 256-channel grid is never written).
// reference: convert_superpoint_to_onnx.py:88-89 (dense) + src/DescriptorGather.cu:14-56 (gather); per-cell
// arithmetic is unchanged (fp32 accumulate in the same k order as the dense igemm path, the raw value rounded to
// fp16 where the dense grid would hold it, F.normalize, fp16, rsqrt renormalise), so the staged API
// (sship_sp_dense + sship_gather_normalize) and this kernel agree to the last fp16 ulp.
// A workgroup (8 waves) owns 64 keypoints of one image; wave w owns output channels [32w, 32w+32).
// ---------------------------------------------------------------------------------------------------
constexpr int kDhLd = 264;  // halfs per LDS row (256 + 8: 33 sixteen-byte slots, odd)
__global__ __launch_bounds__(512) void k_desc_head_gather(const _Float16* __restrict__ da, int Hc, int Wc,
                                                          const int* __restrict__ cell_h, const int* __restrict__ cell_w,
                                                          const int* __restrict__ n_dev, int max_kp,
                                                          const _Float16* __restrict__ wp, const float* __restrict__ bias,
                                                          _Float16* __restrict__ out, size_t out_img_stride) {
  __shared__ __attribute__((aligned(16))) _Float16 s_x[64 * kDhLd];
  __shared__ float s_red[8][64];
  const int b = blockIdx.y, i0 = blockIdx.x * 64;
  const int n = n_dev[b];
  if (i0 >= n) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, hh = lane >> 5;
  const _Float16* img = da + (size_t)b * Hc * Wc * 256;
  for (int u = tid; u < 64 * 32; u += 512) {
    const int r = u >> 5, part = u & 31;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (i0 + r < n) {
      const int ch = cell_h[(size_t)b * max_kp + i0 + r], cw = cell_w[(size_t)b * max_kp + i0 + r];
      v = *reinterpret_cast<const uint4*>(img + ((size_t)ch * Wc + cw) * 256 + part * 8);
    }
    *reinterpret_cast<uint4*>(s_x + r * kDhLd + part * 8) = v;
  }
  h8_t a[16];
  {
    const _Float16* w = wp + (size_t)wave * (16 * 512) + lane * 8;  // packed [cb = wave][k16][lane][8] (ct = 32)
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) a[ks] = *reinterpret_cast<const h8_t*>(w + ks * 512);
  }
  __syncthreads();
  f16x_t acc[2];
#pragma unroll
  for (int nn = 0; nn < 2; ++nn)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nn][r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    const h8_t b0 = *reinterpret_cast<const h8_t*>(s_x + j * kDhLd + ks * 16 + hh * 8);
    const h8_t b1 = *reinterpret_cast<const h8_t*>(s_x + (32 + j) * kDhLd + ks * 16 + hh * 8);
    acc[0] = mfma32(a[ks], b0, acc[0]);
    acc[1] = mfma32(a[ks], b1, acc[1]);
  }
  // raw convDb value as the fp16 dense grid would hold it
  float v[2][16];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 bv = *reinterpret_cast<const float4*>(bias + wave * 32 + hh * 4 + g * 8);
    const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[nn][4 * g + e] = (float)(_Float16)(acc[nn][4 * g + e] + bb[e]);
  }
  auto row_sum_sq = [&](float (&tot)[2]) {
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
      float ss = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) ss += v[nn][r] * v[nn][r];
      ss += __shfl_xor(ss, 32, 64);
      if (hh == 0) s_red[wave][nn * 32 + j] = ss;
    }
    __syncthreads();
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) t += s_red[w][nn * 32 + j];
      tot[nn] = t;
    }
    __syncthreads();
  };
  float tot[2];
  row_sum_sq(tot);
#pragma unroll
  for (int nn = 0; nn < 2; ++nn) {
    const float denom = fmaxf(sqrtf(tot[nn]), 1e-12f);  // F.normalize(p=2, dim=1, eps=1e-12)
#pragma unroll
    for (int r = 0; r < 16; ++r) v[nn][r] = (float)(_Float16)(v[nn][r] / denom);  // the fp16 dense descriptor
  }
  row_sum_sq(tot);
#pragma unroll
  for (int nn = 0; nn < 2; ++nn) {
    const int i = i0 + nn * 32 + j;
    if (i >= n) continue;
    const float inv = rsqrtf(tot[nn] + 1e-12f);  // DescriptorGather.cu:46
    _Float16* orow = out + (size_t)b * out_img_stride + (size_t)i * 256 + wave * 32 + hh * 4;
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<h4_t*>(orow + g * 8) =
          to_h4(v[nn][4 * g] * inv, v[nn][4 * g + 1] * inv, v[nn][4 * g + 2] * inv, v[nn][4 * g + 3] * inv);
  }
}

// ---------------------------------------------------------------------------------------------------
// Whole descriptor head at the selected keypoints: convDa (3x3, 128 -> 256, ReLU) is ALSO evaluated only where a
// keypoint landed - its 3x3x128 input patch is gathered from the encoder output (a4b) - and feeds convDb + the two
// normalisations above without leaving the CU.  600 keypoints of 8084 cells at KITTI size: 13x less convDa work
// (it was the second most expensive head layer), and neither the 256-channel convDa map nor the descriptor grid is
// written to HBM.  Arithmetic per output is the dense kernel's: same fp16 operands, same k order (64-channel chunk, 32-channel
// half, kx, k-step, ky) into an fp32 accumulator that starts at the bias, ReLU, fp16.  reference: convert_superpoint_to_onnx.py:61-64,88-89.
// A workgroup (8 waves) owns 64 keypoints of one image; wave w owns output channels [32w, 32w+32) of both layers and
// streams its 72 KiB of convDa fragments from L2 (packed exactly as the dense conv kernels read them, ct = 32).
// ---------------------------------------------------------------------------------------------------
constexpr int kDsPatchLd = 584;  // halfs per keypoint and 64-channel chunk: 9 taps x 64 + 8 (1168 B: conflict-free b128 reads)
// NN = 32-keypoint N-tiles per workgroup: 2 for batches, 1 when that would leave most CUs without a workgroup (a stereo pair: 20 -> 40 workgroups,
// half the MFMAs and half the patch gather per workgroup; the per-keypoint arithmetic is the same, so the two are bit-identical)
//
// BIL (sship_sp_set_descriptor_sampling(SSHIP_DESC_BILINEAR)): upstream SuperPoint's bilinear sample_descriptors instead of the reference's
// nearest-cell gather.  The rows of the tile are CORNERS: row 4k + q is corner q = 2 dy + dx of keypoint k, so a workgroup serves 8 NN
// keypoints; `cell_h` holds k_topk's packed score-map pixels (h << 16 | w) and `cell_w` is unused.  Patch gather, both MFMA chains and
// F.normalize (the fp16 dense descriptor of the corner cell) are the code below, unchanged; a corner outside the grid is an empty row
// (cell -1, zero patch) with weight 0 - grid_sample's zero padding.  The four corner rows of a keypoint sit in four adjacent lanes of a
// half-wave, so the blend is two __shfl_xor steps on the weighted values ((c0 + c1) + (c2 + c3) in every lane: addition commutes, the
// four lanes hold the same bits, and NN does not enter), row_sum_sq gives |v|^2, and lane q stores channel group q of the row.
template <int NN, bool BIL>
__device__ __forceinline__ void desc_head_tail(f16x_t (&acc)[NN], _Float16* s_x, float (*s_red)[64], const float* s_wt,
                                               const _Float16* __restrict__ wdb, const float* __restrict__ bdb,
                                               _Float16* __restrict__ out_img, int i0, int n);
template <int NN, bool BIL = false>
__global__ __launch_bounds__(512) void k_desc_head_sparse(const _Float16* __restrict__ a4b, int Hc, int Wc,
                                                          const int* __restrict__ cell_h, const int* __restrict__ cell_w,
                                                          const int* __restrict__ n_dev, int max_kp,
                                                          const _Float16* __restrict__ wda, const float* __restrict__ bda,
                                                          const _Float16* __restrict__ wdb, const float* __restrict__ bdb,
                                                          _Float16* __restrict__ out, size_t out_img_stride) {
  extern __shared__ __attribute__((aligned(16))) char ds_smem[];
  _Float16* s_p = reinterpret_cast<_Float16*>(ds_smem);      // [64][kDsPatchLd] patch chunk
  constexpr int NK = 32 * NN;                                 // keypoints per workgroup
  _Float16* s_x = s_p + NK * kDsPatchLd;                      // [NK][kDhLd] convDa output (convDb input)
  float (*s_red)[64] = reinterpret_cast<float (*)[64]>(s_x + NK * kDhLd);
  int* s_cell = reinterpret_cast<int*>(s_red + 8);            // [64] (cell_h << 16 | cell_w), -1 = no keypoint
  float* s_wt = reinterpret_cast<float*>(s_cell + 64);        // [64] BIL: the corner's bilinear weight (the launch adds these 256 bytes)
  const int b = blockIdx.y, i0 = blockIdx.x * (BIL ? NK / 4 : NK);
  const int n = min(max(n_dev[b], 0), max_kp);
  if (i0 >= n) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, hh = lane >> 5;
  if constexpr (BIL) {
    if (tid < NK) {
      const int i = i0 + (tid >> 2), q = tid & 3;
      int c = -1;
      float wq = 0.f;
      if (i < n) {
        const int px = cell_h[(size_t)b * max_kp + i];
        int x0, y0;
        float fx, fy;
        bilinear_corner((float)(px & 0xffff), (float)(px >> 16), Hc, Wc, x0, y0, fx, fy);
        const int cy = y0 + (q >> 1), cx = x0 + (q & 1);
        if (cy >= 0 && cy < Hc && cx >= 0 && cx < Wc) { c = (cy << 16) | cx; wq = bilinear_weight(q, fx, fy); }
      }
      s_cell[tid] = c;
      s_wt[tid] = wq;
    }
  } else {
    if (tid < NK)
      s_cell[tid] = i0 + tid < n ? (cell_h[(size_t)b * max_kp + i0 + tid] << 16) | cell_w[(size_t)b * max_kp + i0 + tid] : -1;
  }
  const _Float16* img = a4b + (size_t)b * Hc * Wc * 128;
  // ---- convDa at the keypoints ----
  f16x_t acc[NN];  // start from the bias, as the dense ping-pong kernel does (conv_pp.hip: same fp32 summation order)
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 bv = *reinterpret_cast<const float4*>(bda + wave * 32 + hh * 4 + g * 8);
#pragma unroll
    for (int nn = 0; nn < NN; ++nn) { acc[nn][4 * g] = bv.x; acc[nn][4 * g + 1] = bv.y; acc[nn][4 * g + 2] = bv.z; acc[nn][4 * g + 3] = bv.w; }
  }
  const _Float16* wa = wda + (size_t)wave * (72 * 512) + lane * 8;  // [cb = wave][chunk][tap][kstep][lane][8]
  // k order inside a 64-channel chunk: the dense kernels' (conv_pp.hip CIN = 128 / conv_pp128.hip: 32-channel half, kx, k-step, ky)
  auto frag_of = [](int idx, int& tap, int& ks) __attribute__((always_inline)) {  // idx 0 .. 35 within the chunk
    const int h32 = idx / 18, r18 = idx - 18 * h32, t6 = r18 / 3, ky = r18 - 3 * t6;
    tap = ky * 3 + (t6 >> 1); ks = 2 * h32 + (t6 & 1);
  };
  auto wfrag = [&](int lin) __attribute__((always_inline)) {  // lin 0 .. 71 over both chunks
    int tap, ks;
    frag_of(lin % 36, tap, ks);
    return *reinterpret_cast<const h8_t*>(wa + (((lin / 36) * 9 + tap) * 4 + ks) * 512);
  };
  h8_t fa[2][12];  // two groups of 12 fragments in flight
#pragma unroll
  for (int i = 0; i < 12; ++i) fa[0][i] = wfrag(i);
  __syncthreads();  // s_cell
#pragma unroll
  for (int chunk = 0; chunk < 2; ++chunk) {  // unrolled: the fragment double buffer is indexed by the parity of g_lin
    if (chunk) __syncthreads();  // every wave is done reading the previous chunk's patches
    for (int u = tid; u < NK * 72; u += 512) {
      const int kp = u / 72, rem = u - kp * 72, tap = rem >> 3, part = rem & 7;
      const int ky = tap / 3, kx = tap - ky * 3;
      const int c = s_cell[kp];
      const int y = (c >> 16) + ky - 1, x = (c & 0xffff) + kx - 1;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (c >= 0 && y >= 0 && y < Hc && x >= 0 && x < Wc)  // conv padding = 1: taps outside the map are zero
        v = *reinterpret_cast<const uint4*>(img + ((size_t)y * Wc + x) * 128 + chunk * 64 + part * 8);
      *reinterpret_cast<uint4*>(s_p + kp * kDsPatchLd + tap * 64 + part * 8) = v;
    }
    __syncthreads();
#pragma unroll
    for (int grp = 0; grp < 3; ++grp) {
      const int g_lin = chunk * 3 + grp;  // 0..5 over the whole k range; buffers alternate across the chunk boundary
      if (g_lin + 1 < 6) {
#pragma unroll
        for (int i = 0; i < 12; ++i) fa[(g_lin + 1) & 1][i] = wfrag((g_lin + 1) * 12 + i);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        int tap, ks;
        frag_of(grp * 12 + i, tap, ks);
#pragma unroll
        for (int nn = 0; nn < NN; ++nn) {
          const h8_t bf = *reinterpret_cast<const h8_t*>(s_p + (nn * 32 + j) * kDsPatchLd + tap * 64 + ks * 16 + hh * 8);
          acc[nn] = mfma32(fa[g_lin & 1][i], bf, acc[nn]);
        }
      }
    }
  }
  desc_head_tail<NN, BIL>(acc, s_x, s_red, s_wt, wdb, bdb, out + (size_t)b * out_img_stride, i0, n);
}

// The part of the head behind convDa, shared by both forms of the kernel: ReLU + fp16 into s_x, convDb, both normalisations, the store.
// acc: this wave's convDa accumulators (bias included); s_x may alias LDS that no wave reads any more; out_img: row 0 of this image.
template <int NN, bool BIL>
__device__ __forceinline__ void desc_head_tail(f16x_t (&acc)[NN], _Float16* s_x, float (*s_red)[64], const float* s_wt,
                                               const _Float16* __restrict__ wdb, const float* __restrict__ bdb,
                                               _Float16* __restrict__ out_img, int i0, int n) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, hh = lane >> 5;
  // convDb fragments: requested now, they land while the convDa epilogue runs
  h8_t a[16];
  {
    const _Float16* w = wdb + (size_t)wave * (16 * 512) + lane * 8;  // packed [cb = wave][k16][lane][8] (ct = 32)
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) a[ks] = *reinterpret_cast<const h8_t*>(w + ks * 512);
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int nn = 0; nn < NN; ++nn)
      *reinterpret_cast<h4_t*>(s_x + (nn * 32 + j) * kDhLd + wave * 32 + hh * 4 + g * 8) =
          to_h4(fmaxf(acc[nn][4 * g], 0.f), fmaxf(acc[nn][4 * g + 1], 0.f), fmaxf(acc[nn][4 * g + 2], 0.f), fmaxf(acc[nn][4 * g + 3], 0.f));
  }
  __syncthreads();
  // ---- convDb + F.normalize + gather renormalisation (as k_desc_head_gather) ----
#pragma unroll
  for (int nn = 0; nn < NN; ++nn)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nn][r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
#pragma unroll
    for (int nn = 0; nn < NN; ++nn) {
      const h8_t bf = *reinterpret_cast<const h8_t*>(s_x + (nn * 32 + j) * kDhLd + ks * 16 + hh * 8);
      acc[nn] = mfma32(a[ks], bf, acc[nn]);
    }
  }
  float v[NN][16];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 bv = *reinterpret_cast<const float4*>(bdb + wave * 32 + hh * 4 + g * 8);
    const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int nn = 0; nn < NN; ++nn)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[nn][4 * g + e] = (float)(_Float16)(acc[nn][4 * g + e] + bb[e]);
  }
  auto row_sum_sq = [&](float (&tot)[NN]) {
#pragma unroll
    for (int nn = 0; nn < NN; ++nn) {
      float ss = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) ss += v[nn][r] * v[nn][r];
      ss += __shfl_xor(ss, 32, 64);
      if (hh == 0) s_red[wave][nn * 32 + j] = ss;
    }
    __syncthreads();
#pragma unroll
    for (int nn = 0; nn < NN; ++nn) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) t += s_red[w][nn * 32 + j];
      tot[nn] = t;
    }
    __syncthreads();
  };
  float tot[NN];
  row_sum_sq(tot);
#pragma unroll
  for (int nn = 0; nn < NN; ++nn) {
    const float denom = fmaxf(sqrtf(tot[nn]), 1e-12f);  // F.normalize(p=2, dim=1, eps=1e-12)
#pragma unroll
    for (int r = 0; r < 16; ++r) v[nn][r] = (float)(_Float16)(v[nn][r] / denom);  // the fp16 dense descriptor
  }
  if constexpr (BIL) {
    // blend the four corner rows of a keypoint (lanes j = 4k .. 4k + 3 of this half-wave), then F.normalize the blend
#pragma unroll
    for (int nn = 0; nn < NN; ++nn) {
      const float wq = s_wt[nn * 32 + j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float t = v[nn][r] * wq;
        t += __shfl_xor(t, 1, 64);
        t += __shfl_xor(t, 2, 64);
        v[nn][r] = t;
      }
    }
    row_sum_sq(tot);
#pragma unroll
    for (int nn = 0; nn < NN; ++nn) {
      const int i = i0 + ((nn * 32 + j) >> 2), q = j & 3;
      if (i >= n) continue;
      const float denom = fmaxf(sqrtf(tot[nn]), 1e-12f);  // F.normalize(p=2, dim=1, eps=1e-12)
      _Float16* orow = out_img + (size_t)i * 256 + wave * 32 + hh * 4;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (q == g)
          *reinterpret_cast<h4_t*>(orow + g * 8) =
              to_h4(v[nn][4 * g] / denom, v[nn][4 * g + 1] / denom, v[nn][4 * g + 2] / denom, v[nn][4 * g + 3] / denom);
    }
    return;
  }
  row_sum_sq(tot);
#pragma unroll
  for (int nn = 0; nn < NN; ++nn) {
    const int i = i0 + nn * 32 + j;
    if (i >= n) continue;
    const float inv = rsqrtf(tot[nn] + 1e-12f);  // DescriptorGather.cu:46
    _Float16* orow = out_img + (size_t)i * 256 + wave * 32 + hh * 4;
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<h4_t*>(orow + g * 8) =
          to_h4(v[nn][4 * g] * inv, v[nn][4 * g + 1] * inv, v[nn][4 * g + 2] * inv, v[nn][4 * g + 3] * inv);
  }
}

// ---------------------------------------------------------------------------------------------------
// The throughput form of the head above (NN = 2, nearest sampling; the launch of a batch): two workgroups per CU, so that one gathers while
// the other issues MFMAs.  What changes against k_desc_head_sparse<2> is the staging only:
//   * the patch is staged one 32-channel QUARTER at a time (the dense k order - 64-channel chunk, 32-channel half, kx, k-step, ky - makes a
//     quarter the 18 consecutive fragments 18 q .. 18 q + 17: same fragments at the same addresses of `wda`, same fp32 summation order),
//     into two buffers of 64 x (9 x 32 + 8) halfs: quarter q + 1 lands while quarter q feeds the MFMAs, one workgroup barrier per quarter;
//   * the gather is LDS-DMA through one buffer resource per image (base = the image's a4b, num_records = exactly Hc Wc 256 bytes): no
//     staging registers, no ds_write pass.  A buffer is 64 rows of 37 sixteen-byte slots = 37 lane-linear wave-instructions; slot 36 of a
//     row is the padding.  A lane's byte offset is formed ONCE (it is the same in all four quarters but for + 64 q) and only from a tap
//     that passed the map's bounds; every other slot - a tap outside the map (x = -1 and x = Wc are in range as linear offsets), a row
//     without a keypoint, the padding - gets kDqOob, which fails the range check in every quarter: the DMA writes zeros there;
//   * s_x (convDa's output) reuses buffer 0, which no wave reads after the barrier of quarter 3: 78 080 B of LDS per workgroup;
//   * 4 waves per SIMD = 128 VGPRs: the fragment ring is two groups of 6 (126 VGPRs, no scratch: profiles/desc_head_resource_usage.txt).
// ---------------------------------------------------------------------------------------------------
constexpr int kDqLd = 296;                 // halfs per keypoint and quarter: 9 taps x 32 + 8 (592 B = 37 slots, odd: conflict-free b128 reads)
constexpr int kDqBufBytes = 64 * kDqLd * 2;  // 37 888 = 37 x 1 024
constexpr unsigned kDqOob = 0x80000000u;   // + 64 q stays beyond every num_records (the launcher refuses maps of 2^31 bytes and more)
constexpr size_t kDqSmem = 2 * (size_t)kDqBufBytes + 8 * 64 * 4 + 64 * 4;
static_assert(kDqBufBytes == 37 * 1024 && 64 * kDhLd * 2 <= kDqBufBytes && 2 * kDqSmem <= 160 * 1024, "descriptor head LDS layout");
// (the second launch bound is waves per SIMD: two 8-wave workgroups on a CU are 4)
__global__ __launch_bounds__(512, 4) void k_desc_head_sparse_2wg(const _Float16* __restrict__ a4b, int Hc, int Wc,
                                                                 const int* __restrict__ cell_h, const int* __restrict__ cell_w,
                                                                 const int* __restrict__ n_dev, int max_kp,
                                                                 const _Float16* __restrict__ wda, const float* __restrict__ bda,
                                                                 const _Float16* __restrict__ wdb, const float* __restrict__ bdb,
                                                                 _Float16* __restrict__ out, size_t out_img_stride) {
  extern __shared__ __attribute__((aligned(16))) char ds_smem[];
  _Float16* s_p = reinterpret_cast<_Float16*>(ds_smem);       // [2][64][kDqLd] patch quarters
  float (*s_red)[64] = reinterpret_cast<float (*)[64]>(ds_smem + 2 * kDqBufBytes);
  int* s_cell = reinterpret_cast<int*>(s_red + 8);            // [64] (cell_h << 16 | cell_w), -1 = no keypoint
  const int b = blockIdx.y, i0 = blockIdx.x * 64;
  const int n = min(max(n_dev[b], 0), max_kp);
  if (i0 >= n) return;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, j = lane & 31, hh = lane >> 5;
  if (tid < 64)
    s_cell[tid] = i0 + tid < n ? (cell_h[(size_t)b * max_kp + i0 + tid] << 16) | cell_w[(size_t)b * max_kp + i0 + tid] : -1;
  f16x_t acc[2];  // start from the bias, as the dense ping-pong kernel does (conv_pp.hip: same fp32 summation order)
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 bv = *reinterpret_cast<const float4*>(bda + wave * 32 + hh * 4 + g * 8);
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) { acc[nn][4 * g] = bv.x; acc[nn][4 * g + 1] = bv.y; acc[nn][4 * g + 2] = bv.z; acc[nn][4 * g + 3] = bv.w; }
  }
  const _Float16* wa = wda + (size_t)wave * (72 * 512) + lane * 8;  // [cb = wave][chunk][tap][kstep][lane][8]
  // fragment r18 = 0 .. 17 of a quarter: (kx, k-step) pair r18 / 3, ky = r18 % 3 (k_desc_head_sparse: frag_of)
  auto wfrag = [&](int q, int r18) __attribute__((always_inline)) {
    const int t6 = r18 / 3, ky = r18 - 3 * t6, tap = ky * 3 + (t6 >> 1), ks = 2 * (q & 1) + (t6 & 1);
    return *reinterpret_cast<const h8_t*>(wa + (((q >> 1) * 9 + tap) * 4 + ks) * 512);
  };
  h8_t fa[2][6];  // two groups of 6 fragments in flight
#pragma unroll
  for (int i = 0; i < 6; ++i) fa[0][i] = wfrag(0, i);
  typedef int rsrc4_t __attribute__((ext_vector_type(4)));
  rsrc4_t rs;
  {
    const unsigned long long ba = (unsigned long long)(uintptr_t)(a4b + (size_t)b * Hc * Wc * 128);
    rs[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)ba);
    rs[1] = __builtin_amdgcn_readfirstlane((int)((unsigned)(ba >> 32) & 0xffffu));
    rs[2] = __builtin_amdgcn_readfirstlane(Hc * Wc * 256);
    rs[3] = 0x00020000;
  }
  __syncthreads();  // s_cell
  // wave-instruction wave + 8 k of a buffer (k = 0 .. 4, 37 in all) fills slots 64 (wave + 8 k) + lane
  unsigned voff[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int slot = (wave + 8 * k) * 64 + lane, kp = min(slot / 37, 63), within = slot - (slot / 37) * 37;
    const int tap = within >> 2, ky = tap / 3, kx = tap - ky * 3;
    const int c = s_cell[kp];
    const int y = (c >> 16) + ky - 1, x = (c & 0xffff) + kx - 1;
    const bool ok = within < 36 && c >= 0 && y >= 0 && y < Hc && x >= 0 && x < Wc;  // conv padding = 1: taps outside the map are zero
    voff[k] = ok ? (unsigned)(y * Wc + x) * 256u + (unsigned)(within & 3) * 16u : kDqOob;
  }
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)s_p);
  auto dma = [&](int q) __attribute__((always_inline)) {  // quarter q -> buffer q & 1
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      // instructions 37 .. 39 do not exist.  (Tested for every k, not only k = 4: a wave-uniform branch per instruction keeps the five
      // address adds apart - with one straight-line block the kernel needs 20 bytes of scratch under its 128 VGPRs.)
      if (wave + 8 * k >= 37) continue;
      const unsigned dst = lds0 + (unsigned)((q & 1) * kDqBufBytes + (wave + 8 * k) * 1024), v = voff[k] + 64u * q;
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(v), "s"(dst), "s"(rs) : "memory");
    }
  };
  dma(0);
#pragma unroll
  for (int q = 0; q < 4; ++q) {  // unrolled: the fragment double buffer is indexed by the parity of the group
    // this wave's share of quarter q has landed; behind the barrier all of it has, and every wave is done reading quarter q - 1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const _Float16* sq = s_p + (q & 1) * (64 * kDqLd);
#pragma unroll
    for (int grp = 0; grp < 3; ++grp) {
      const int g_lin = q * 3 + grp;  // 0..11 over the whole k range; the ring alternates across the quarter boundaries
      if (g_lin + 1 < 12) {
#pragma unroll
        for (int i = 0; i < 6; ++i) fa[(g_lin + 1) & 1][i] = wfrag((g_lin + 1) / 3, ((g_lin + 1) % 3) * 6 + i);
      }
      if (grp == 0 && q < 3) dma(q + 1);  // behind the fragments the next group waits for: two groups of MFMAs to land in
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const int r18 = grp * 6 + i, t6 = r18 / 3, ky = r18 - 3 * t6, tap = ky * 3 + (t6 >> 1);
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) {
          const h8_t bf = *reinterpret_cast<const h8_t*>(sq + (nn * 32 + j) * kDqLd + tap * 32 + (t6 & 1) * 16 + hh * 8);
          acc[nn] = mfma32(fa[g_lin & 1][i], bf, acc[nn]);
        }
      }
    }
  }
  // s_x = buffer 0: last read in quarter 2, and every wave has passed the barrier of quarter 3
  desc_head_tail<2, false>(acc, s_p, s_red, nullptr, wdb, bdb, out + (size_t)b * out_img_stride, i0, n);
}

// bilinear mode: four corner rows per keypoint, so a workgroup serves 8 NN keypoints and the grid is four times the nearest-cell one
hipError_t launch_desc_head_sparse_bilinear(const ConvW& da32, const ConvW& db32, const _Float16* a4b, int Hc, int Wc, const int* pix,
                                            const int* n_dev, int max_kp, int B, _Float16* out, size_t out_img_stride, hipStream_t s) {
  if (da32.cin != 128 || da32.cout != 256 || da32.ct != 32 || da32.ks != 3) return hipErrorInvalidValue;
  if (Hc > 4095 || Wc > 8191) return hipErrorInvalidValue;  // the packed (h << 16 | w) pixel word
  constexpr size_t smem = (size_t)64 * kDsPatchLd * 2 + (size_t)64 * kDhLd * 2 + 8 * 64 * 4 + 64 * 4 + 64 * 4;  // + the corner weights
  static const hipError_t attr_rc = [] {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_desc_head_sparse<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_desc_head_sparse<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  }();
  if (attr_rc != hipSuccess) return attr_rc;
  // latency mode by the nearest-cell launch's rule, on this launch's own workgroup count
  if (B * ((max_kp + 15) / 16) * 2 <= cu_count())
    hipLaunchKernelGGL((k_desc_head_sparse<1, true>), dim3((max_kp + 7) / 8, B), dim3(512), smem, s, a4b, Hc, Wc, pix, nullptr, n_dev,
                       max_kp, da32.w, da32.bias, db32.w, db32.bias, out, out_img_stride);
  else
    hipLaunchKernelGGL((k_desc_head_sparse<2, true>), dim3((max_kp + 15) / 16, B), dim3(512), smem, s, a4b, Hc, Wc, pix, nullptr, n_dev,
                       max_kp, da32.w, da32.bias, db32.w, db32.bias, out, out_img_stride);
  return hipGetLastError();
}

hipError_t launch_desc_head_sparse(const ConvW& da32, const ConvW& db32, const _Float16* a4b, int Hc, int Wc, const int* cell_h,
                                   const int* cell_w, const int* n_dev, int max_kp, int B, _Float16* out, size_t out_img_stride,
                                   hipStream_t s) {
  if (da32.cin != 128 || da32.cout != 256 || da32.ct != 32 || da32.ks != 3) return hipErrorInvalidValue;
  constexpr size_t smem = (size_t)64 * kDsPatchLd * 2 + (size_t)64 * kDhLd * 2 + 8 * 64 * 4 + 64 * 4;  // NN = 2 (NN = 1 uses half of the tile buffers)
  // thread-safe one-time opt-in to > 64 KiB of dynamic LDS (C++11 magic static; handles may be created on any thread)
  static const hipError_t attr_rc = [] {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_desc_head_sparse_2wg), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDqSmem);
    if (e != hipSuccess) return e;
#if SSHIP_DEV_SWITCHES
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_desc_head_sparse<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
#endif
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_desc_head_sparse<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  }();
  if (attr_rc != hipSuccess) return attr_rc;
  // developer build, SUPERSLAM_HIP_DESC_HEAD: "1wg" = k_desc_head_sparse<2> (one workgroup per CU, 64-channel chunks through registers: the A/B
  // and the bit-exact oracle of the two-workgroup form), "2wg" = the two-workgroup form; either one at EVERY batch size (tests reach them with few keypoints)
  static const std::string form = [] { const char* e = dev_env("SUPERSLAM_HIP_DESC_HEAD"); return std::string(e ? e : ""); }();
  // latency mode: 32-keypoint workgroups when the 64-keypoint grid would not give half of the CUs a workgroup
  if (B * ((max_kp + 63) / 64) * 2 <= cu_count() && form != "1wg" && form != "2wg") {
    hipLaunchKernelGGL(k_desc_head_sparse<1>, dim3((max_kp + 31) / 32, B), dim3(512), smem, s, a4b, Hc, Wc, cell_h, cell_w, n_dev,
                       max_kp, da32.w, da32.bias, db32.w, db32.bias, out, out_img_stride);
    return hipGetLastError();
  }
#if SSHIP_DEV_SWITCHES
  if (form == "1wg") {
    hipLaunchKernelGGL(k_desc_head_sparse<2>, dim3((max_kp + 63) / 64, B), dim3(512), smem, s, a4b, Hc, Wc, cell_h, cell_w, n_dev,
                       max_kp, da32.w, da32.bias, db32.w, db32.bias, out, out_img_stride);
    return hipGetLastError();
  }
#endif
  if ((long long)Hc * Wc * 256 >= (1ll << 31)) return hipErrorInvalidValue;  // the gather's 32-bit byte offsets (a map of 8 M cells)
  hipLaunchKernelGGL(k_desc_head_sparse_2wg, dim3((max_kp + 63) / 64, B), dim3(512), kDqSmem, s, a4b, Hc, Wc, cell_h, cell_w, n_dev,
                     max_kp, da32.w, da32.bias, db32.w, db32.bias, out, out_img_stride);
  return hipGetLastError();
}

void launch_desc_head_gather(const ConvW& db32, const _Float16* da, int Hc, int Wc, const int* cell_h, const int* cell_w,
                             const int* n_dev, int max_kp, int B, _Float16* out, size_t out_img_stride, hipStream_t s) {
  hipLaunchKernelGGL(k_desc_head_gather, dim3((max_kp + 63) / 64, B), dim3(512), 0, s, da, Hc, Wc, cell_h, cell_w, n_dev,
                     max_kp, db32.w, db32.bias, out, out_img_stride);
}

}  // namespace sship
