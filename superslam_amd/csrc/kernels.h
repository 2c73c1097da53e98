// Internal kernel launch interface of libsuperslam_hip (not part of the C ABI).
#pragma once
#include "common.h"
#include "rect_host.h"

namespace sship {

constexpr int kMaxKp = 4096;   // upper bound on max_keypoints (top-k sorts in LDS)
constexpr int kLogitStride = 68;   // detector logits: 65 channels in a 68-wide fp32 row (272 B, 16-B aligned; was 80: 15 % fewer bytes through convPb -> k_nms_tile)

// ---- sp_kernels.hip ----
void launch_conv1a(const uint8_t* img, const float* w, const float* bias, _Float16* out, int B, int H, int W,
                   hipStream_t s);
struct NmsArgs {
  const float* logits;   // [B, Hc, Wc, ls] (loader 0)
  int ls;
  const float* scores_in;  // [B, H, W] (loader 1)
  int B, H, W;             // score-map shape
  int radius;
  float thr_f;             // smallest float f with (double)f > thr  ->  keep iff s >= thr_f
  int border;
  unsigned long long* cand;  // [B, cap] or null
  int* cand_count;           // [B]
  int cap;
  float* scores_out;         // [B, H, W] post-NMS or null
  float* scores_raw_out;     // [B, H, W] pre-NMS (softmax + depth-to-space) or null
};
float threshold_as_float(double thr);
void launch_nms_tile(int loader, const NmsArgs& a, hipStream_t s);

struct TopkArgs {
  const unsigned long long* cand;  // [B, cap]
  const int* cand_count;           // [B]
  int* reset_count;                // [B] or null: the kernel zeroes the image's candidate counter once it has read it (the next call's NMS starts from 0 without a memset launch)
  int cap, max_kp;
  int score_w;                     // W of the score map (key idx = h*W + w)
  float scale_x, scale_y;          // input_w / score_w, input_h / score_h (float division on the host)
  int desc_h, desc_w;
  float* kp_xys;                   // [B, max_kp, 3]
  int* cell_h;                     // [B, max_kp]
  int* cell_w;                     // [B, max_kp]
  int* n_out;                      // [B]
  int* n_cand_out;                 // [B] or null
  int* pix;                        // [B, max_kp] or null: the keypoint's score-map pixel (h << 16 | w), what the bilinear descriptor head samples at and k_kp_refine refines
};
void launch_topk(const TopkArgs& a, int B, hipStream_t s);
// Spatially balanced selection (include/sship.h, SSHIP_SELECT_BALANCED): from the M candidate keys of an image to the K = min(M, max_kp)
// keys the rule selects, in any order, as a second candidate list that k_topk then sorts and emits (k_select_balanced).
struct SelectBalancedArgs {
  const unsigned long long* cand;  // [B, cap]
  const int* cand_count;           // [B]; read, never written: k_topk's reset_count still clears it
  int cap, max_kp;
  int score_w;                     // W of the score map (key idx = h*W + w)
  int bucket_px, nbx, nb;          // G; buckets per row = ceil(W / G); buckets = nbx * ceil(H / G)
  unsigned long long* sel;         // [B, max_kp] the selected keys ...
  int* sel_count;                  // [B] ... and their number K (written, not accumulated: needs no clearing)
  int* n_cand_out;                 // [B] or null: M before the cap, what k_topk reports in the default mode
  unsigned long long* ws_seg;      // [B, cap] workspace: per-bucket segments, when the image does not fit the LDS path
  unsigned long long* ws_bnd;      // [B, nb]  boundary list
  int* ws_tab;                     // [B, nb]  bucket table
};
hipError_t launch_select_balanced(const SelectBalancedArgs& a, int B, hipStream_t s);
// Sub-pixel keypoint refinement (include/sship.h, sship_sp_set_keypoint_refinement): the three-point log-parabola fit per axis on the
// pre-NMS log-scores of the keypoint's pixel and its four neighbours.  Logit c of cell (cy, cx) of image b is
// logits[b * img_stride + (cy * Wc + cx) * cell_stride + c * chan_stride]; keypoint i of image b is pix[b * max_kp + i].
struct KpRefineArgs {
  const float* logits;
  size_t img_stride, cell_stride, chan_stride;  // in floats
  int Hc, Wc;
  const int* pix;        // [B, max_kp] score-map pixels (h << 16 | w), the packing k_topk writes; clamped into the map
  const int* n_dev;      // [B] device counts (clamped to [0, max_kp]) or null: n_host keypoints
  int n_host, max_kp;
  float* kp_xys;         // [B, max_kp, 3]: x = (w + dx) * scale_x and y = (h + dy) * scale_y overwrite kp[0], kp[1] ...
  float scale_x, scale_y;
  float* offsets;        // ... unless this is set: [B, max_kp, 2] = (dx, dy) (the stage form)
};
void launch_kp_refine(const KpRefineArgs& a, int B, hipStream_t s);
void launch_threshold_scan(const float* scores, int H, int W, float thr_f, int border, unsigned long long* cand,
                           int* cand_count, int cap, hipStream_t s);
void launch_gather_hwc(bool raw, const _Float16* grid, int C, int gh, int gw, size_t img_stride, const int* cell_h,
                       const int* cell_w, const int* n_dev, int n_host, int max_kp, int B, _Float16* out,
                       hipStream_t s);
void launch_gather_chw(const _Float16* grid, int C, int gh, int gw, const int* cell_h, const int* cell_w, int n,
                       _Float16* out, hipStream_t s);
// Bilinear descriptor sampling (include/sship.h, sship_sp_set_descriptor_sampling): upstream SuperPoint's sample_descriptors =
// grid_sample(align_corners = True, zero padding) at score-map pixel (x, y) of a gh x gw cell grid.  (x0, y0) = the top-left corner cell
// (-1 when the pixel lies left of / above the first cell centre), (fx, fy) the fractions; corner q = 2 dy + dx has weight
// bilinear_weight(q) and counts only where it lies inside the grid.  fp32; the coordinates are clamped so that no input can index outside.
__device__ __forceinline__ void bilinear_corner(float x, float y, int gh, int gw, int& x0, int& y0, float& fx, float& fy) {
  float gx = (x - 3.5f) / (8.f * (float)gw - 4.5f) * (float)(gw - 1);
  float gy = (y - 3.5f) / (8.f * (float)gh - 4.5f) * (float)(gh - 1);
  gx = fminf(fmaxf(gx, -1.f), (float)gw);
  gy = fminf(fmaxf(gy, -1.f), (float)gh);
  const float flx = floorf(gx), fly = floorf(gy);
  x0 = (int)flx; y0 = (int)fly; fx = gx - flx; fy = gy - fly;
}
__device__ __forceinline__ float bilinear_weight(int q, float fx, float fy) { return ((q & 2) ? fy : 1.f - fy) * ((q & 1) ? fx : 1.f - fx); }
// kp_xy [n][2] fp32 score-map pixels -> out [n][C] fp16, C <= 256 (hwc: a multiple of 4)
void launch_sample_bilinear_chw(const _Float16* grid, int C, int gh, int gw, const float* kp_xy, int n, _Float16* out, hipStream_t s);
void launch_sample_bilinear_hwc(const _Float16* grid, int C, int gh, int gw, const float* kp_xy, int n, _Float16* out, hipStream_t s);
void launch_desc_dense_chw(const _Float16* raw, int cells_per_img, int B, _Float16* out, hipStream_t s);
void launch_logits_chw(const float* in, int ls, int cells_per_img, int B, float* out, hipStream_t s);
void launch_bgr2gray(const uint8_t* in, int n, uint8_t* out, hipStream_t s);

// ---- sp_convs.hip : MFMA implicit-GEMM layers of SuperPoint ----
struct ConvW {          // one packed conv / linear layer on the device
  _Float16* w = nullptr;  // packed A-fragment order (igemm.h)
  _Float16* w_wino = nullptr;  // optional: Winograd F(2x2,3x3)-transformed weights of a 64 -> 64 3x3 layer (conv_wino.hip)
  _Float16* w_q = nullptr;  // optional second form: 64-row cout tiles over 32-channel chunks (conv_pp128.hip); convPb: the plain [80][256] matrix
  float* bias = nullptr;  // [cout_pad]
  int cin = 0, cout = 0, cout_pad = 0, ks = 1, ct = 64;
};
// in: channels-last fp16 [B,H,W,cin]; out: [B,Ho,Wo,cout] fp16 (pool: floor(/2)).
hipError_t sp_conv3x3_strip(const ConvW& w, const _Float16* in, _Float16* out, int B, int H, int W, bool pool,
                            hipStream_t s);
hipError_t sp_conv1ab_fused(const ConvW& w1b, const _Float16* w1a_frag, const float* b1a, const uint8_t* img,
                            _Float16* out, int B, int H, int W, hipStream_t s);
hipError_t sp_conv3x3_pp(const ConvW& w, const _Float16* in, _Float16* out, int B, int H, int W, bool pool, hipStream_t s);
bool sp_conv3x3_pp128_fits(int B, int H, int W, int cin);
hipError_t sp_conv3x3_pp128(const ConvW& w, const _Float16* in, _Float16* out, int B, int H, int W, bool pool, hipStream_t s);
// conv_fuse2.hip: conv2a -> conv2b -> max-pool in one launch (rolling window over 30-column strips, weights in registers); bit-identical to the
// two launches of sp_conv3x3_pp.  fits(): the shape is supported and (unless `any_batch`) the batch fills the chip with strip segments
bool sp_conv2ab_fused_fits(int B, int H, int W, bool any_batch);
hipError_t sp_conv2ab_fused(const ConvW& wa, const ConvW& wb, const _Float16* in, _Float16* out, int B, int H, int W, hipStream_t s);
// the same rolling-window kernel as ONE 64 -> 128 layer (conv3a): all 128 output channels in one launch, weights in registers; bit-identical to sp_conv3x3_pp
bool sp_conv3a_roll_fits(int B, int H, int W);
hipError_t sp_conv3a_roll(const ConvW& w, const _Float16* in, _Float16* out, int B, int H, int W, hipStream_t s);
hipError_t sp_conv1ab_pp(const ConvW& w1b, const _Float16* w1a_frag, const float* b1a, const uint8_t* img, _Float16* out,
                         int B, int H, int W, hipStream_t s);
// conv_wino.hip: Winograd F(2x2, 3x3) for 64 -> 64 channels (SUPERSLAM_HIP_CONV64=wino)
bool sp_conv3x3_wino_fits(int H, int W, int cin, int cout);
hipError_t sp_conv3x3_wino(const _Float16* upack, const float* bias, const _Float16* in, _Float16* out, int B, int H, int W, bool pool, hipStream_t s);
hipError_t sp_conv1x1_f16(const ConvW& w, const _Float16* in, _Float16* out, int B, int H, int W, hipStream_t s);
// compute units of the current device (cached; persistent kernels launch one workgroup per CU). probe.hip
int cu_count();

// probe.hip
hipError_t mfma_probe(bool random_operands, float* tflops);

hipError_t launch_desc_head_sparse(const ConvW& da32, const ConvW& db32, const _Float16* a4b, int Hc, int Wc, const int* cell_h,
                                   const int* cell_w, const int* n_dev, int max_kp, int B, _Float16* out, size_t out_img_stride,
                                   hipStream_t s);
// bilinear mode: rows are corners (four per keypoint), `pix` = k_topk's packed score-map pixels
hipError_t launch_desc_head_sparse_bilinear(const ConvW& da32, const ConvW& db32, const _Float16* a4b, int Hc, int Wc, const int* pix,
                                            const int* n_dev, int max_kp, int B, _Float16* out, size_t out_img_stride, hipStream_t s);
void launch_desc_head_gather(const ConvW& db32, const _Float16* da, int Hc, int Wc, const int* cell_h, const int* cell_w,
                             const int* n_dev, int max_kp, int B, _Float16* out, size_t out_img_stride, hipStream_t s);
hipError_t sp_conv1x1_f32(const ConvW& w, const _Float16* in, float* out, int ostride, int B, int H, int W,
                          hipStream_t s);

// ---- ep_kernels.hip : EigenPlaces (ResNet-18 + GeM) ----
// ws: split-K workspace of ws_bytes (ep_splitk_workspace_bytes) or null = never split; the split is clamped to what fits
hipError_t ep_conv(const ConvW& w, const _Float16* in, _Float16* out, const _Float16* res, int H, int W, bool relu, bool decim,
                   hipStream_t s, float* ws = nullptr, size_t ws_bytes = 0);
size_t ep_splitk_workspace_bytes(int in_h, int in_w);
// a batch of B images (maps [B][H][W][c]): per deep layer the single-image split k, run as batched split-K or as the grouped kernel
enum EpBatchForm { kEpDirect = 0, kEpSplit = 1, kEpGrouped = 2 };
struct EpBatchPlan { int form, k, th; };
EpBatchPlan ep_batch_plan(int ks, int cin, int cout, int cout_pad, int H, int W, bool decim, int batch, size_t ws1_bytes);
size_t ep_batch_workspace_bytes(int in_h, int in_w, int batch);
// ws_bytes: the batch workspace really held (too small for a split layer: hipErrorInvalidValue); ws1_bytes: ep_splitk_workspace_bytes of the engine
hipError_t ep_conv_batch(const ConvW& w, const _Float16* in, _Float16* out, const _Float16* res, int H, int W, bool relu, bool decim, int B,
                         hipStream_t s, float* ws, size_t ws_bytes, size_t ws1_bytes);
// B images image_stride bytes apart -> [B][3][out_h][out_w]
void launch_ep_resize_norm(const uint8_t* src, int stride, int ch, const int* tab, int out_w, int out_h, float* out, hipStream_t s, int B = 1,
                           long long image_stride = 0);
void launch_ep_im2col(const float* x, int H, int W, int Ho, int Wo, _Float16* out, hipStream_t s);
void launch_ep_maxpool(const _Float16* in, int H, int W, int Ho, int Wo, _Float16* out, hipStream_t s);
// fused stem + ReLU + max-pool (round 6): wfrag = [2][11][64][8] fp16 A fragments (k = (c, ky, kx padded to 8)), bias fp32 [64]
void launch_ep_stem_pool(const float* x, int H, int W, int Ho, int Wo, int Hp, int Wp, const _Float16* wfrag, const float* bias, _Float16* out,
                         hipStream_t s, int B = 1);
int ep_tail_pool_wgs(int npix);   // workgroups of the tail's pooling kernel = rows of partial sums it writes
size_t ep_tail_ws_floats();   // the tail's workspace: partial GeM sums of up to 32 workgroups + the [512] pre-normalisation outputs
void launch_ep_tail(const _Float16* feat, int npix, float p, const float* wt, const float* bias, float* ws, int* counters, float* out,
                    hipStream_t s, int B = 1, int slice = 0, int out_stride = 512);

// ---- lg_kernels.hip ----
struct LgDims {
  int S;    // sequences (2 * pairs)
  int NP;   // padded tokens per sequence (multiple of 32)
};
void launch_lg_prep(const float* kp, int kp_stride, int kp_seq_stride, const int* lens, int max_kp, int* lens_clamped,
                    const _Float16* desc, size_t desc_seq_stride, const float* wr, float img_w, float img_h, LgDims d,
                    _Float16* x, float* rope, float* kpn, hipStream_t s);
hipError_t lg_linear_heads(const ConvW& w, const _Float16* x, LgDims d, int rope_segs, int t_seg,
                           const float* rope, _Float16* q, _Float16* k, _Float16* vt, hipStream_t s);
void launch_lg_attention(const _Float16* q, const _Float16* k, const _Float16* vt, const int* lens, LgDims d,
                         bool cross, _Float16* ctx, hipStream_t s, bool shared_gpu = false);
// lg_attn_res.hip: throughput batches, the keys of a (sequence, head) resident in LDS
bool lg_attention_res_fits(LgDims d);
void launch_lg_attention_res(const _Float16* q, const _Float16* k, const _Float16* vt, const int* lens, LgDims d, bool cross,
                             _Float16* ctx, hipStream_t s);
// prefetch (both launches below): up to three packed layers the NEXT FFN launch streams; latency mode pulls them into L2 with surplus workgroups
hipError_t launch_lg_proj_heads(const ConvW& next, _Float16* x, LgDims d, int rope_segs, int t_seg, const float* rope, _Float16* q,
                                _Float16* k, _Float16* vt, hipStream_t s, const ConvW* const* prefetch = nullptr, const int* tiles = nullptr);
void launch_lg_ffn(const ConvW& w0, const ConvW& w3, const float* gamma, const float* beta, const _Float16* ctx,
                   _Float16* x, LgDims d, const ConvW* next, bool heads, int rope_segs, int t_seg, const float* rope,
                   _Float16* q, _Float16* k, _Float16* vt, _Float16* out, const float* match_w, float match_b,
                   float* logsig, hipStream_t s, const ConvW* const* prefetch = nullptr, const int* live = nullptr, int live_mode = 1);
// tokens per tile (32 | 64) of the FFN / projection launch over `tokens` tokens: the unit of a tile list handed to it (live_mode 2, `tiles`)
int lg_ffn_tile_tokens(int tokens);
// Adaptive depth (sship_lg_set_depth_confidence).  State of the pairs [p0, p0 + np) of one launch group, every pointer offset to p0:
struct LgDepth {
  int* cnt;         // [np][8]: valid tokens with confidence < thr_i after layer i (integer atomics: exact, order-independent)
  int* layers_run;  // [np]: 9 while running, i + 1 once stopped after layer i
  int* lens_live;   // [2 np]: the clamped counts of running pairs, 0 for stopped ones (what the attention launches of layers >= 1 read)
  int* live;        // [1 + np]: count, then the running pairs' indices (what the FFN launches of layers >= 1 walk)
  unsigned* ticket; // one counter: the last workgroup of a k_lg_depth_conf launch takes the decisions
};
void launch_lg_depth_init(const int* lens, int np, LgDepth dep, hipStream_t s);
// token confidence of layer i: counts, then (last workgroup) the stop rule for every pair of the group
void launch_lg_depth_conf(const _Float16* x, const int* lens, int NP, int np, const float* tw, float tb, float thr, float depth_conf,
                          int layer, LgDepth dep, hipStream_t s);
// the assignment inputs of every stopped pair from head layers_run - 1: md = final_proj(x) (scale folded in), logsig = logsigmoid(matchability . x)
// wt [9][256 in][256 out] fp32, bias [9][256], mw [9][256], mb [9]
void launch_lg_exit_head(const _Float16* x, int NP, int pairs, const int* layers_run, const float* wt, const float* bias, const float* mw,
                         const float* mb, _Float16* md, float* logsig, hipStream_t s);
// Adaptive width (sship_lg_set_width_confidence).  State of the pairs [p0, p0 + np) of one launch group, every pointer offset to p0:
struct LgWidth {
  int* wlen;    // [2 np]: live tokens of every sequence (a stopped or emptied pair keeps the counts it was matched on)
  int* chg;     // [2 np]: 1 if the sequence lost tokens at the last prune launch (its next-layer Q/K/V are projected again)
  int* ind;     // [2 np][NP]: original keypoint index of every live row
  int* prune;   // [2 np][NP], by original index: 1 + the pruning steps the keypoint survived (upstream's prune0 / prune1)
  int* tiles;   // [1 + tiles]: count, then the tiles that hold live tokens of running pairs (what the FFN launches walk)
  int* rtiles;  // [1 + tiles]: count, then the tiles of the sequences with chg = 1 (what the re-projection walks)
};
void launch_lg_width_init(const int* lens, int NP, int np, LgWidth wd, hipStream_t s);
// the pruning step of one layer for every running pair: one workgroup per sequence decides, compacts x / rope / ind in place (forward
// moves only) and zeroes the vacated rows.  keep = sigmoid(mw . x + mb) > keep_thr, or (tcw != null: depth on) sigmoid(tcw . x + tcb) <= thr
void launch_lg_width_prune(_Float16* x, float* rope, int NP, int np, const float* mw, const float* mb, float keep_thr, int min_kp,
                           const float* tcw, float tcb, float thr, LgDepth dep, LgWidth wd, hipStream_t s);
// after the prune launch of layer `layer`: a pair with an emptied image is finished (layers_run = layer + 1); lens_live (0 for pairs
// that are not running), the two tile lists in tiles of `tile_tokens` tokens
void launch_lg_width_publish(int NP, int np, int tile_tokens, int layer, LgDepth dep, LgWidth wd, hipStream_t s);
// matches of the live sets (mc / msc, [pairs][max_kp]) -> the caller's arrays through ind: pruned keypoints and rows >= n get -1 / 0
void launch_lg_width_scatter(const int* wlen, const int* ind, int NP, int pairs, int max_kp, const int32_t* mc, const float* msc,
                             int32_t* matches0, float* mscores0, hipStream_t s);
void launch_lg_sim(const _Float16* md, const int* lens, LgDims d, float* sim, hipStream_t s);
void launch_lg_assign(const _Float16* md, const float* logsig, const int* lens, LgDims d, float* ws, float* pcol, int max_kp,
                      int32_t* matches0, float* mscores0, float thr, int stage, hipStream_t s);

// ---- nn_kernels.hip : mutual nearest-neighbour matcher (sship_nn_*) ----
// desc [2 pairs][max_kp][256] fp16, lens [2 pairs] (device, clamped to [0, max_kp] by the kernels); ws: nn_workspace_floats(max_kp, max_pairs)
// floats of top-2 partials; ratio / dist <= 0 turn that test off; outputs [pairs][max_kp], every entry written
size_t nn_workspace_floats(int max_kp, int max_pairs);
void launch_nn_match(const _Float16* desc, const int* lens, int max_kp, int pairs, float* ws, float ratio, float dist, int mutual,
                     int32_t* matches0, float* mscores0, hipStream_t s);
// the same with the keypoint-window gate: kp [2 pairs][max_kp][3] fp32 (x, y, score), gate = (dx_lo, dx_hi, dy_lo, dy_hi); same workspace
void launch_nn_match_gated(const _Float16* desc, const float* kp, const int* lens, int max_kp, int pairs, float* ws, float ratio, float dist,
                           int mutual, const float gate[4], int32_t* matches0, float* mscores0, hipStream_t s);
// StereoFrontEnd::process's association on the device: stereo [pairs][max_kp][3] = (uL, uR or NaN, vL), has_depth [pairs][max_kp] u8
void launch_stereo_associate(const float* kp, const int* lens, const int32_t* matches0, int max_kp, int pairs, float min_disparity,
                             float max_row_diff, float* stereo, uint8_t* has_depth, hipStream_t s);

// ---- index_kernels.hip : place-recognition index (sship_index_*) ----
constexpr int kIndexRows = 256;     // database rows per scan workgroup (one chunk of partials)
constexpr int kIndexTile = 16;      // queries per scan workgroup (the MFMA's N)
constexpr int kIndexMaxTopK = 128;
// the stored-row rule: dst [rows_total][dim] (16-byte aligned) = normalised src rows (`stride` floats apart, any alignment); rows >= count
// are zeroed.  src == dst with stride == dim normalises in place.
void launch_index_normalize(const float* src, long long stride, int count, int rows_total, int dim, float* dst, hipStream_t s);
// one query call = normalise + scan + merge.  db [size][dim] stored rows; q: num_queries rows q_stride floats apart; limits: device [Q] or
// null (then limit_all for every query); qn: [ceil16(Q)][dim] floats; partial: ceil(size / kIndexRows) * Q * top_k keys;
// rows / scores [Q][top_k] and counts [Q] are written completely.
void launch_index_query(const float* db, int dim, int size, const float* q, long long q_stride, int num_queries, const int* limits, int limit_all,
                        int top_k, float min_score, float* qn, unsigned long long* partial, int* rows, float* scores, int* counts, hipStream_t s);

// ---- pose_kernels.hip : pose-only stereo solver (sship_pose_*) ----
constexpr int kPoseMaxObs = 2048;   // 8 observations per thread of a 256-thread workgroup, held in registers
struct PoseK {                      // the camera and the rule's constants, by value
  double fx, fy, cx, cy, baseline;
  double inv_sigma_px, sigma_d0, d_cond, k, k2;
  double lambda0, lambda_max, abs_tol, rel_tol, inlier_px;
  int max_iterations;
};
// one workgroup per pair, the whole LM loop in the launch.  pose0 / inlier may be null; every output entry is written.
void launch_pose_solve(const float* points, const float* meas, const uint8_t* valid, const double* pose0, int max_obs, int pairs,
                       const PoseK& k, double* pose, int32_t* stats, double* cost, uint8_t* inlier, hipStream_t s);
// the observation list from two frames' stereo points and matches0 (include/sship.h); every output entry is written.
void launch_pose_gather(const float* stereo0, const uint8_t* hd0, const float* stereo1, const uint8_t* hd1, const int32_t* matches0,
                        const int* n0, const int* n1, int n_stride, int max_obs, int pairs, const PoseK& k, float* points, float* meas,
                        uint8_t* valid, hipStream_t s);

// ---- ransac_kernels.hip : RANSAC pose seed and inlier gate (sship_ransac_*) ----
constexpr int kRansacMaxSplits = 32;   // workgroups that share one pair's hypotheses at most
constexpr int kRansacRecord = 14;      // doubles of a workgroup's partial result: cost, h, pose
struct RansacK {                       // the camera and the rule's constants, by value
  double fx, fy, cx, cy, baseline;
  double thr2, min_disparity, min_area2;
  uint32_t seed;
  int num_hypotheses;
};
int ransac_splits(int num_hypotheses);
size_t ransac_workspace_bytes(int max_pairs, int num_hypotheses);
// the score launch (splits x pairs workgroups) and the launch of the argmin and the winner's mask.  inlier may be null; every output
// entry is written.
void launch_ransac_solve(const float* points, const float* meas, const uint8_t* valid, int max_obs, int pairs, const RansacK& k,
                         void* workspace, double* pose, int32_t* stats, double* cost, uint8_t* inlier, hipStream_t s);

// ---- ba_kernels.hip : sliding-window stereo bundle adjustment (sship_ba_*) ----
constexpr int kBaMaxKf = 16;
constexpr int kBaMaxObs = 2048;
constexpr int kBaMaxLandmarks = 32768;
constexpr int kBaResident = 512;    // workgroups of a solve launch (they walk the windows), each with a workspace slice
struct BaK {                        // the camera and the rule's constants, by value
  double fx, fy, cx, cy, baseline;
  double inv_sigma, k, k2;
  double lambda0, lambda_max, abs_tol, rel_tol;
  int max_iterations;
};
// bytes of one workspace slice (include/sship.h states the formula); the handle holds min(max_windows, kBaResident) of them
size_t ba_workspace_bytes(int max_keyframes, int max_obs, int max_landmarks);
hipError_t ba_solve_prepare();
// one workgroup per window, the whole LM loop in the launch.  n_kf / landmarks may be null; every output entry is written.
void launch_ba_solve(const float* meas, const int32_t* track, const int32_t* n_kf, const double* pose0, int max_keyframes, int max_obs,
                     int max_landmarks, int windows, const BaK& k, void* workspace, double* pose, int32_t* stats, double* cost,
                     float* landmarks, hipStream_t s);
// the landmark bookkeeping from has_depth and matches0 chains (include/sship.h); every entry of track is written.
void launch_ba_tracks(const uint8_t* has_depth, const int32_t* matches, const int32_t* n, const int32_t* n_kf, int max_keyframes, int max_obs,
                      int windows, int32_t* track, hipStream_t s);

// ---- pg_kernels.hip : batched pose-graph optimiser (sship_pg_*) ----
constexpr int kPgMaxNodes = 4096;
constexpr int kPgMaxLoops = 128;
constexpr int kPgResident = 256;    // workgroups of a solve launch (they walk the graphs), each with a workspace slice
struct PgK {                        // the rule's constants, by value
  double odom_sigma_rot, odom_sigma_trans;
  double lambda0, lambda_max, abs_tol, rel_tol, max_translation;
  int max_iterations;
};
// bytes of one workspace slice (include/sship.h states the formula); the handle holds min(max_graphs, kPgResident) of them
size_t pg_workspace_bytes(int max_nodes, int max_loops);
// one workgroup per graph, the LM loop and the rejection loop in the launch.  n_nodes / odom_sigma / loop_enable / loop_chi2 may be null,
// and so may all loop arrays when max_loops == 0; every output entry is written.
void launch_pg_solve(const int32_t* n_nodes, const double* pose0, const double* odom_z, const double* odom_sigma, const int32_t* loop_ij,
                     const double* loop_z, const double* loop_sigma, const double* loop_k2, const uint8_t* loop_enable, int max_nodes,
                     int max_loops, int graphs, const PgK& k, void* workspace, double* pose, int32_t* stats, double* cost, double* loop_chi2,
                     hipStream_t s);
void launch_pg_odometry(const double* pose, int max_nodes, int graphs, double* odom_z, hipStream_t s);
void launch_pg_loops(const int32_t* from, const int32_t* to, const double* pose, const int32_t* stats, int pairs, int min_inliers,
                     double noise_base, int32_t* loop_ij, double* loop_z, double* loop_sigma, double* loop_k2, uint8_t* loop_enable,
                     hipStream_t s);

// rectification remap + RGB-D association (rect_kernels.hip; the host half - tables and tile boxes - is rect_host.h)
struct RgbdK { double fx, fy, cx, cy, d[8], bf, depth_factor, max_depth; int has_dist; };
void launch_rect_remap(const uint8_t* src, int src_h, int src_stride, uint8_t* dst, int dst_w, int dst_h, const void* table,
                       const RectTile* tiles, int cameras, int cam0, int images, int force_direct, hipStream_t s);
void launch_rgbd_associate(const float* kp, const int* lens, int frames, int max_kp, const void* depth, int depth_f32, int h, int w,
                           long long depth_stride, const RgbdK& c, float* kp_undist, float* stereo, uint8_t* has_depth, hipStream_t s);

// sub-pixel disparity refinement (stereo_refine_kernels.hip).  gate2 = (max_rms * N)^2, computed once on the host; gate = max_rms > 0.
struct StereoRefineK { double gate2; float min_disparity; int half_window, search_radius, gate, drop; };
// imgs [2 * pairs, h, stride bytes] u8; status / cost may be null; stereo_out / has_depth_out may alias their inputs
void launch_stereo_refine(const uint8_t* imgs, int pairs, int h, int w, long long stride, const float* stereo_in, const uint8_t* has_depth_in,
                          const int* lens, int n_stride, int max_kp, const StereoRefineK& c, float* stereo_out, uint8_t* has_depth_out,
                          uint8_t* status, long long* cost, hipStream_t s);

// keypoint stereo depth by epipolar search (stereo_search_kernels.hip).  tex2 = (min_texture * N)^2 and gate2 = (max_rms * N)^2, computed once
// on the host; tex / gate = the gate is on.
struct StereoSearchK { double tex2, gate2; int half_window, dlo, dhi, uniqueness, lr, tex, gate; };
// imgs [2 * pairs, h, stride bytes] u8; pair p reads kp / lens of unit p * unit_stride; status / cost may be null
void launch_stereo_search(const uint8_t* imgs, int pairs, int h, int w, long long stride, const float* kp, const int* lens, int unit_stride,
                          int max_kp, const StereoSearchK& c, float* stereo_out, uint8_t* has_depth_out, uint8_t* status, long long* cost,
                          hipStream_t s);

// keypoint tracking by 2-D patch search (patch_track_kernels.hip).  tex2 = (min_texture * N)^2 and gate2 = (max_rms * N)^2, computed once on
// the host; tex / gate = the gate is on; fb = fb_check.
struct PatchTrackK { double tex2, gate2; int half_window, radius, uniqueness, fb, tex, gate; };
// imgs0 / imgs1: image p at imgs + p * image_stride (bytes), rows of `stride` bytes; pair p reads kp / lens of unit p * unit_stride; pred
// [pairs, max_kp, 3] may be null and may be kp_out; n_out / status / cost may be null
void launch_patch_track(const uint8_t* imgs0, long long image_stride0, int stride0, const uint8_t* imgs1, long long image_stride1, int stride1,
                        int pairs, int h, int w, const float* kp, const int* lens, int unit_stride, const float* pred, int max_kp,
                        const PatchTrackK& c, float* kp_out, int* n_out, int* matches0, uint8_t* status, long long* cost, hipStream_t s);

// image pyramid and coarse-to-fine patch tracking (pyr_kernels.hip)
constexpr int kPyrMaxLevels = 8, kPyrTileW = 64, kPyrTileH = 16, kPyrRowAlign = 64;
// one reduction of `images` images: src image i at src + i * src_image_stride, rows of src_stride bytes, h x w; dst rows of dst_pitch bytes
// (a multiple of 4, >= (w + 1) / 2 rounded up to 4; dst and every dst row dword aligned).  aligned: src, src_image_stride and src_stride are multiples of 4 (rows are then read by dwords, else by bytes).
void launch_pyr_down(const uint8_t* src, long long src_image_stride, long long src_stride, int h, int w, int aligned, uint8_t* dst,
                     long long dst_image_stride, int dst_pitch, int images, hipStream_t s);
// one level of both pyramids as the tracker reads it: pair p reads the images at img + p * pair_stride (bytes)
struct PyrTrackLevel { const uint8_t* img0; const uint8_t* img1; long long pair_stride0, pair_stride1, stride0, stride1; int h, w; };
struct PyrTrackLevels { PyrTrackLevel l[kPyrMaxLevels]; };
// fine: level 0's constants; the levels above use its half_window and uniqueness with coarse_radius and no gate.  slot_bytes =
// pyr_track_slot_bytes(half_window, max(fine.radius, coarse_radius)): the LDS of one keypoint.
struct PyrTrackK { PatchTrackK fine; int levels, coarse_radius, slot_bytes; };
size_t pyr_track_slot_bytes(int half_window, int radius);
void launch_pyr_track(const PyrTrackLevels& tab, int pairs, const float* kp, const int* lens, int unit_stride, const float* pred, int max_kp,
                      const PyrTrackK& c, float* kp_out, int* n_out, int* matches0, uint8_t* status, long long* cost, uint8_t* levels_tracked,
                      hipStream_t s);

// contrast-limited adaptive histogram equalisation (clahe_kernels.hip)
constexpr int kClaheMaxTiles = 16, kClaheMaxArea = 1 << 24, kClaheBlockW = 256, kClaheBlockH = 32;
// the rule's constants, all formed on the host: tiles of tw x th pixels of the extended image, limit = L (0: no clipping),
// scale = 255.f / (float)(tw * th), inv_tw = 1.f / (float)tw, inv_th = 1.f / (float)th
struct ClaheK { int tiles_x, tiles_y, tw, th, limit; float scale, inv_tw, inv_th; };
// the two launches of one call: the tables of `images` images into luts [images, tiles_y, tiles_x, 256] (16-byte aligned), then every
// destination pixel from them.  Strides in bytes, no alignment asked; dst may be src with equal strides.
void launch_clahe_lut(const uint8_t* src, long long src_image_stride, long long src_stride, int h, int w, const ClaheK& c, uint8_t* luts,
                      int images, hipStream_t s);
void launch_clahe_apply(const uint8_t* src, long long src_image_stride, long long src_stride, uint8_t* dst, long long dst_image_stride,
                        long long dst_stride, int h, int w, const ClaheK& c, const uint8_t* luts, int images, hipStream_t s);

// FAST corners with track refill (fast_kernels.hip; the rule is in include/sship.h "FAST corners")
constexpr int kFastTileW = 64, kFastTileH = 32;
// cap = ceil(h / 2) * ceil(w / 2): the key list of an image cannot overflow (no two candidates are 8-neighbours);
// min_distance, max_kp and unit_stride describe the keep list of step 3
struct FastK { int h, w, tiles_x, tiles_y, threshold, border, cap, min_distance, max_kp, unit_stride; };
// step 1 alone: u8 scores [images, h, w] with caller strides (bytes), no alignment asked of either side
void launch_fast_score(const uint8_t* imgs, long long image_stride, long long stride, int h, int w, uint8_t* score,
                       long long score_image_stride, long long score_stride, int images, hipStream_t s);
// steps 1-3: the keys (bits((float)s) << 32) | (y * w + x) of the candidates into cand [images, cap], their number added to cand_count
// [images] (zeroed by the caller).  keep [units, max_kp, 3] with counts keep_n, image p reads unit p * unit_stride: the mask of step 3,
// applied when keep is given and min_distance > 0
void launch_fast_detect(const uint8_t* imgs, long long image_stride, long long stride, const FastK& c, const float* keep, const int* keep_n,
                        unsigned long long* cand, int* cand_count, int images, hipStream_t s);
// step 5: keep may be null (L = 0); new_kp [images, max_new, 3] and n_new [images] are what k_topk left; carry0 may be null
void launch_fast_merge(const float* keep, const int* keep_n, int unit_stride, int max_kp, const float* new_kp, const int* n_new, int max_new,
                       int target, float* kp_out, int* n_out, int* carry0, int images, hipStream_t s);

// Steered BRIEF descriptors and the Hamming matcher (brief_kernels.hip; the rules are in include/sship.h "Binary descriptors")
struct BriefTable;                               // csrc/brief_pattern.h
const BriefTable& brief_table_host();            // the object the device table is a copy of
constexpr int kBriefWaves = 4;                   // keypoints (one wave each) per workgroup of k_brief_describe
// image p reads unit p * unit_stride of kp [units, max_kp, 3] and lens [units]; status and bin may be null
void launch_brief_describe(const uint8_t* imgs, long long image_stride, int stride, int images, int h, int w, const float* kp, const int* lens,
                           int unit_stride, int max_kp, int mode, uint32_t* desc, uint8_t* status, uint8_t* bin, hipStream_t s);
constexpr int kHmRows = 128;                     // rows of one set per workgroup of k_hm_best, one per lane
constexpr int kHmTile = 64;                      // rows of the other set per LDS tile
struct HmK { int max_kp, max_distance, ratio_percent, mutual, gate_on; float gate[4]; int first0, step0, first1, step1; };
inline size_t hm_workspace_ints(int max_kp, int max_pairs) { return (size_t)max_pairs * 3 * max_kp; }   // fwd | bwd per pair, then e1
// status may be null; kp is read only with c.gate_on; mscores0 may be null.  Two launches: k_hm_best, k_hm_final.
void launch_hm_match(const int* lens, const uint32_t* desc, const uint8_t* status, const float* kp, const HmK& c, int pairs, int* ws,
                     int* matches0, int* dist0, float* mscores0, hipStream_t s);

}  // namespace sship
