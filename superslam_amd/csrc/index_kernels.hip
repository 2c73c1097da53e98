// Place-recognition index (include/sship.h "Place-recognition index"): cosine top-k retrieval over a device-resident fp32
// database, the reference's CosineDescriptorIndex (src/PlaceRecognizer.cc:21-52) as three launches per query call:
//   k_index_normalize  the stored-row rule (fp64 norm, (float)((double)x / n)) for an add and for the queries of a call;
//   k_index_scan       one streaming pass over rows [0, max limit): scores = rows x a tile of 16 queries on the exact-f32 MFMA
//                      (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain), reduced per 256-row chunk to the chunk's best top_k keys;
//   k_index_merge      one workgroup per query: radix select of the top_k-th key over all chunk partials, then a rank sort of the winners.
// The [M, Q] score matrix never reaches HBM.  A key is 64 bits, (orderable score bits) << 32 | ~row: descending key order is the rule's
// total order (score descending, ties by ascending row), all keys of one query are distinct, and 0 is "no candidate".
// One path serves Q = 1 and Q = 1024: a score's summation order is a function of dim alone (the order is written at k_index_scan).
#include "kernels.h"

namespace sship {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

// (score, row) -> key.  -0 counts as +0 (the rule compares values); NaN never gets here.
__device__ __forceinline__ u64 index_key(float s, int row) {
  if (s == 0.f) s = 0.f;
  unsigned u = __float_as_uint(s);
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return (static_cast<u64>(u) << 32) | static_cast<u64>(0xffffffffu - static_cast<unsigned>(row));
}
__device__ __forceinline__ float index_key_score(u64 key) {
  unsigned u = static_cast<unsigned>(key >> 32);
  u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
  return __uint_as_float(u);
}
__device__ __forceinline__ int index_key_row(u64 key) { return static_cast<int>(0xffffffffu - static_cast<unsigned>(key)); }

// One workgroup per destination row.  src rows are `stride` floats apart and read as scalars (a caller's buffer has no alignment
// promise); dst is [rows_total][dim], 16-byte aligned, written as float4.  Rows >= count (the padding of a query tile) are zeroed.
// src == dst with stride == dim is allowed: every element is read and written by the same thread.
__global__ __launch_bounds__(256) void k_index_normalize(const float* src, long long stride, int count, int dim, float* dst) {
  __shared__ double red[256];
  const int row = blockIdx.x, tid = threadIdx.x;
  f32x4* out = reinterpret_cast<f32x4*>(dst + static_cast<size_t>(row) * dim);
  if (row >= count) {
    for (int k4 = tid; k4 < dim / 4; k4 += 256) out[k4] = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const float* x = src + static_cast<long long>(row) * stride;
  double acc = 0.0;
  for (int k = tid; k < dim; k += 256) { const double v = x[k]; acc += v * v; }
  red[tid] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  const double n = sqrt(red[0]);
  const bool scale = n > 1e-12;  // false for a NaN norm: the row stays as given
  for (int k4 = tid; k4 < dim / 4; k4 += 256) {
    f32x4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float xv = x[4 * k4 + c];
      v[c] = scale ? static_cast<float>(static_cast<double>(xv) / n) : xv;
    }
    out[k4] = v;
  }
}

// grid (chunks, query tiles), 256 threads.  Workgroup (c, t) scores rows [c R, c R + R) against queries [16 t, 16 t + 16) of qn
// ([16 * tiles][dim], normalised, padding rows zero).  Wave w owns rows c R + 64 w + 16 g + i (g = 0..3 independent accumulators,
// i = lane & 15 the MFMA's A row); the MFMA's B column is the query.  Per 32-wide k block a lane loads the 8 consecutive floats
// k0 + 8 h .. + 7 (h = lane >> 4) of its row - the four lane groups cover one 128-byte line of the row - and of its query, and issues 8
// MFMA steps; step e sums k0 + e, k0 + 8 + e, k0 + 16 + e, k0 + 24 + e in that order.  So a score is the fmaf chain over
//   k = 32 b + e + 8 h   for b = 0 .., e = 0..7, h = 0..3 (b outermost, h innermost), terms with k >= dim being (+0)(+0),
// the same for every row, query, index size and batch.  dim is a multiple of 4, so a float4 is wholly inside or wholly outside a row.
// Rows >= size are not read (their operand is 0) and rows >= limit_q are no candidates.
__global__ __launch_bounds__(256) void k_index_scan(const float* __restrict__ db, const float* __restrict__ qn, int dim, int size, int num_queries,
                                                    const int* __restrict__ limits, int limit_all, int top_k, float min_score, u64* partial) {
  __shared__ u64 keys[kIndexTile][kIndexRows + 1];
  __shared__ u64 best[kIndexTile][kIndexMaxTopK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x, q0 = blockIdx.y * kIndexTile;
  const int li = lane & 15, h = lane >> 4;
  const int row_base = chunk * kIndexRows + wave * 64;

  f32x4 acc[4];
  const float* ap[4];
  bool live[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int row = row_base + 16 * g + li;
    live[g] = row < size;
    ap[g] = db + static_cast<size_t>(live[g] ? row : 0) * dim;
  }
  const float* bp = qn + static_cast<size_t>(q0 + li) * dim;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < dim; k0 += 32) {
    const int kk = k0 + 8 * h;
    const bool in0 = kk < dim, in1 = kk + 4 < dim;
    const f32x4 b0 = in0 ? *reinterpret_cast<const f32x4*>(bp + kk) : zero;
    const f32x4 b1 = in1 ? *reinterpret_cast<const f32x4*>(bp + kk + 4) : zero;
    f32x4 a0[4], a1[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      a0[g] = (in0 && live[g]) ? *reinterpret_cast<const f32x4*>(ap[g] + kk) : zero;
      a1[g] = (in1 && live[g]) ? *reinterpret_cast<const f32x4*>(ap[g] + kk + 4) : zero;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[g][e], b0[e], acc[g], 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[g][e], b1[e], acc[g], 0, 0, 0);
  }
  // D[i = 4 h + r][j = li]: row i of the group, query j.  `s >= min_score` in this form: a NaN score is no candidate.
  const int q = q0 + li;
  int limit = 0;
  if (q < num_queries) {
    limit = limits ? limits[q] : limit_all;
    limit = limit < 0 ? 0 : limit > size ? size : limit;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int local = wave * 64 + 16 * g + 4 * h + r;
      const int row = chunk * kIndexRows + local;
      const float s = acc[g][r];
      keys[li][local] = (row < limit && s >= min_score) ? index_key(s, row) : 0ull;
    }
  for (int e = tid; e < kIndexTile * kIndexMaxTopK; e += 256) (&best[0][0])[e] = 0ull;
  __syncthreads();
  // rank sort of the chunk, per query: keys are distinct, so rank = the number of larger keys; the first top_k ranks are kept.
  // Right for min_score = -inf (every row a candidate) at R compares per row; a row that is no candidate costs nothing.
  const int nq = num_queries - q0 < kIndexTile ? num_queries - q0 : kIndexTile;
  for (int j = 0; j < nq; ++j) {
    const u64 mine = keys[j][tid];
    if (mine != 0ull) {
      int rank = 0;
      for (int i = 0; i < kIndexRows; ++i) rank += keys[j][i] > mine ? 1 : 0;
      if (rank < top_k) best[j][rank] = mine;
    }
  }
  __syncthreads();
  // partial [chunks][num_queries][top_k]
  for (int e = tid; e < nq * top_k; e += 256) {
    const int j = e / top_k, p = e - j * top_k;
    partial[(static_cast<size_t>(chunk) * num_queries + q0 + j) * top_k + p] = best[j][p];
  }
}

// One workgroup per query over its n = chunks * top_k partial keys (zeros are holes).  cnt = min(top_k, #keys).  The cnt-th largest
// key is found by an 8-bit radix select from the top byte down (8 passes, a 256-bin histogram each, integer LDS atomics only); the
// keys >= it are exactly the cnt winners (keys are distinct), collected in any order and placed by rank.  The output is a function of the
// key values alone.  Every entry of rows / scores [Q][top_k] and counts [Q] is written; the tail is -1 / 0.
__global__ __launch_bounds__(256) void k_index_merge(const u64* __restrict__ partial, int chunks, int num_queries, int top_k, int* rows,
                                                     float* scores, int* counts) {
  __shared__ int hist[256];
  __shared__ int suf[257];
  __shared__ u64 sel[kIndexMaxTopK];
  __shared__ u64 s_prefix;
  __shared__ int s_need, s_cnt, s_nsel;
  const int q = blockIdx.x, tid = threadIdx.x;
  const long long n = static_cast<long long>(chunks) * top_k;
  auto key_at = [&](long long e) -> u64 {
    const long long c = e / top_k;
    const int p = static_cast<int>(e - c * top_k);
    return partial[(static_cast<size_t>(c) * num_queries + q) * top_k + p];
  };
  if (tid == 0) { s_prefix = 0ull; s_need = 0; s_cnt = 0; s_nsel = 0; }
  for (int pass = 7; pass >= 0; --pass) {
    hist[tid] = 0;
    __syncthreads();
    const u64 prefix = s_prefix;
    const u64 mask = pass == 7 ? 0ull : ~0ull << (8 * (pass + 1));
    for (long long e = tid; e < n; e += 256) {
      const u64 k = key_at(e);
      if (k != 0ull && (k & mask) == prefix) atomicAdd(&hist[static_cast<int>(k >> (8 * pass)) & 255], 1);
    }
    __syncthreads();
    // suf[b] = keys of this pass with digit >= b
    suf[tid] = hist[tid];
    if (tid == 0) suf[256] = 0;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int add = tid + d < 256 ? suf[tid + d] : 0;
      __syncthreads();
      suf[tid] += add;
      __syncthreads();
    }
    if (pass == 7 && tid == 0) {
      s_cnt = suf[0] < top_k ? suf[0] : top_k;
      s_need = s_cnt;
    }
    __syncthreads();
    if (s_cnt == 0) break;  // uniform
    const int need = s_need;
    const bool pick = suf[tid] >= need && suf[tid + 1] < need;  // exactly one digit
    __syncthreads();
    if (pick) {
      s_prefix = prefix | (static_cast<u64>(tid) << (8 * pass));
      s_need = need - suf[tid + 1];
    }
    __syncthreads();
  }
  const int cnt = s_cnt;
  if (cnt > 0) {
    const u64 kth = s_prefix;
    for (long long e = tid; e < n; e += 256) {
      const u64 k = key_at(e);
      if (k >= kth && k != 0ull) {
        const int at = atomicAdd(&s_nsel, 1);
        if (at < kIndexMaxTopK) sel[at] = k;
      }
    }
    __syncthreads();
    if (tid < cnt) {
      const u64 mine = sel[tid];
      int rank = 0;
      for (int i = 0; i < cnt; ++i) rank += sel[i] > mine ? 1 : 0;
      rows[static_cast<size_t>(q) * top_k + rank] = index_key_row(mine);
      scores[static_cast<size_t>(q) * top_k + rank] = index_key_score(mine);
    }
  }
  for (int p = cnt + tid; p < top_k; p += 256) {
    rows[static_cast<size_t>(q) * top_k + p] = -1;
    scores[static_cast<size_t>(q) * top_k + p] = 0.f;
  }
  if (tid == 0) counts[q] = cnt;
}

void launch_index_normalize(const float* src, long long stride, int count, int rows_total, int dim, float* dst, hipStream_t s) {
  if (rows_total <= 0) return;
  hipLaunchKernelGGL(k_index_normalize, dim3(rows_total), dim3(256), 0, s, src, stride, count, dim, dst);
}

void launch_index_query(const float* db, int dim, int size, const float* q, long long q_stride, int num_queries, const int* limits, int limit_all,
                        int top_k, float min_score, float* qn, unsigned long long* partial, int* rows, float* scores, int* counts, hipStream_t s) {
  const int tiles = (num_queries + kIndexTile - 1) / kIndexTile;
  launch_index_normalize(q, q_stride, num_queries, tiles * kIndexTile, dim, qn, s);
  const int span = limits ? size : (limit_all < size ? limit_all : size);  // rows [0, span) can be candidates of some query
  const int chunks = span > 0 ? (span + kIndexRows - 1) / kIndexRows : 0;
  if (chunks > 0)
    hipLaunchKernelGGL(k_index_scan, dim3(chunks, tiles), dim3(256), 0, s, db, qn, dim, size, num_queries, limits, limit_all, top_k, min_score,
                       partial);
  hipLaunchKernelGGL(k_index_merge, dim3(num_queries), dim3(256), 0, s, partial, chunks, num_queries, top_k, rows, scores, counts);
}

}  // namespace sship
