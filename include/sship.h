/* sship.h - C ABI of libsuperslam_hip.so: the MI355X (gfx950) deep-feature front-end for SuperSLAM.
 *
 * This header is the drop-in boundary.  Every entry point replaces a piece of the reference's
 * TensorRT/CUDA inference layer (paths relative to /root/reference); the C++ adapter a maintainer adds
 * on the reference side (classes SuperPoint / LightGlue implementing IFeatureExtractor / IFeatureMatcher
 * over these calls) is shown in INTEGRATION.md and shipped as include/superslam_hip/.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch/OpenCV types cross the ABI;
 *   - every function returns an int status (0 = SSHIP_OK); nothing throws or longjmps across the ABI;
 *     sship_last_error() returns a thread-local message for the last non-zero status;
 *   - "_dev" pointers are HIP device pointers, all others host pointers;
 *   - `stream` is a hipStream_t passed as void*; NULL is the legacy default stream itself (= torch's default
 *     stream), so consecutive asynchronous calls made with NULL - extractor then matcher - are ordered with each
 *     other and with the caller's default-stream work.  The synchronous host-image / host-keypoint entry points
 *     use the handle's own (blocking) stream and return after synchronising it.  Multi-threaded callers: the legacy
 *     default stream synchronises with EVERY blocking stream of the process, i.e. a NULL-stream batch call on one
 *     thread serialises with another thread's handles (the loop-closure matcher / EigenPlaces).  The handle streams
 *     do not synchronise with each other, so threads that use the synchronous entry points (the reference's usage)
 *     run concurrently; a thread that drives the asynchronous batch API next to them should pass its own
 *     hipStreamNonBlocking stream (or hipStreamPerThread) instead of NULL;
 *   - external dtypes follow the reference engines (scripts/rebuild_engines.sh:85-92,108-115):
 *     image u8 (normalised to [0,1] on device), scores f32, descriptors f16, kpts f32,
 *     matches0 i32, mscores0 f32.  Internal accumulation is f32.
 *   - handles are single-threaded; sship_lg_weights is immutable and shareable across handles/threads
 *     (the LightGlueEngine / shared_engine() analogue, include/LightGlue.h:28-31,44).
 *
 * Environment
 *   The library reads exactly two environment variables, each once per process:
 *     SUPERSLAM_HIP_DEVICE=<n>   device ordinal sship_init(-1) / the first call of a thread binds (default 0; the multi-process
 *                                scripts set it from LOCAL_RANK);
 *     SSHIP_RCCL_LIBRARY=<path>  the RCCL library sship_comm_* binds at run time instead of the process's own / librccl.so.1.
 *   Nothing else: there is ONE kernel per layer and no run-time kernel selection, so a stray variable cannot move a SuperSLAM
 *   process onto a slower or looser path.  Profiling is an API (sship_set_profiling), not a variable.  The A/B switches of the
 *   development history (SUPERSLAM_HIP_CONV*, _ATTN*, _FFN*, _LG_*, SSHIP_*_TRACE) and the kernels they select exist only in the
 *   developer build superslam_amd/lib/variants/dev.so (`python -m superslam_amd.build --dev`, -DSSHIP_DEV_SWITCHES=1), which the
 *   A/B tests and scripts load explicitly.
 */
#ifndef SSHIP_H_
#define SSHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSHIP_VERSION 100
#define SSHIP_DESC_DIM 256 /* include/SuperPoint.h:76 descriptor_dim */

typedef enum {
  SSHIP_OK = 0,
  SSHIP_ERR_INVALID = 1,        /* bad argument */
  SSHIP_ERR_HIP = 2,            /* HIP runtime failure */
  SSHIP_ERR_IO = 3,             /* weights file missing / malformed */
  SSHIP_ERR_NOMEM = 4,
  SSHIP_ERR_POOL_EXHAUSTED = 5, /* src/SuperPoint.cc:724-727 */
  SSHIP_ERR_NO_DEVICE = 6       /* no gfx950 device: the library never falls back to the CPU */
} sship_status;

/* ------------------------------------------------------------------------------------------------
 * Runtime
 * ---------------------------------------------------------------------------------------------- */
/* Select the HIP device (replaces the implicit cudaSetDevice(0) of SuperPoint::initialize,
 * src/SuperPoint.cc:38-67).  Fails with SSHIP_ERR_NO_DEVICE when no GPU is visible. */
int sship_init(int device);
int sship_version(void);
const char* sship_last_error(void);
/* level: 0 trace .. 4 error; the adapter forwards to SLOG_* (include/Logging.h:21-26). */
void sship_set_log_callback(void (*cb)(int level, const char* msg));
int sship_device_synchronize(void);

/* ------------------------------------------------------------------------------------------------
 * Descriptor pool - include/DescriptorPool.h:13-91, src/DescriptorPool.cc:10-38
 * N device slots of max_keypoints*dim fp16; LIFO free-list (FreeList, DescriptorPool.h:25-44).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_pool sship_pool;
int sship_pool_create(int num_slots, int max_keypoints, int dim, sship_pool** out);
/* Frees the device slots and drops the creator's reference.  The bookkeeping (free-list, mutex) is reference counted
 * like the reference's shared_ptr<FreeList> (DescriptorPool.h:71-75): every DeviceDescriptors handle holds one
 * reference (sship_pool_retain when the handle is made, sship_pool_release + sship_pool_release_ref in its deleter),
 * so a handle may outlive the pool's owner; its data pointer then dangles exactly as in the reference
 * (DescriptorPool.cc:27-32) but releasing it is safe. */
void sship_pool_destroy(sship_pool* pool);
void sship_pool_retain(sship_pool* pool);
void sship_pool_release_ref(sship_pool* pool);
int sship_pool_acquire(sship_pool* pool);            /* FreeList::acquire: slot index or -1 when exhausted */
void sship_pool_release(sship_pool* pool, int slot); /* FreeList::release */
int sship_pool_in_use(const sship_pool* pool);       /* FreeList::in_use */
void* sship_pool_slot_ptr(const sship_pool* pool, int slot); /* DescriptorPool::slot_ptr (NULL if out of range) */

/* ------------------------------------------------------------------------------------------------
 * Descriptor gather - 1:1 with launch_gather_descriptors, include/DescriptorGather.h:12-20,
 * src/DescriptorGather.cu:14-82.  grid_fp16_dev is [channels, grid_h, grid_w] (CHW) fp16; cell_h/cell_w
 * are device int arrays; out is [num_keypoints, channels] fp16, each row L2-normalised
 * (fp32 sum of squares, rsqrt(sum + 1e-12), round-to-nearest fp16).  num_keypoints <= 0 is a no-op.
 * The _hwc variant reads a channels-last grid [grid_h, grid_w, channels] (one contiguous 512-B row per
 * keypoint - the layout the HIP SuperPoint produces internally).
 * ---------------------------------------------------------------------------------------------- */
int sship_gather_normalize(const void* grid_fp16_dev, int channels, int grid_h, int grid_w,
                           const int* cell_h_dev, const int* cell_w_dev, int num_keypoints,
                           void* out_fp16_dev, void* stream);
int sship_gather_normalize_hwc(const void* grid_fp16_dev, int channels, int grid_h, int grid_w,
                               const int* cell_h_dev, const int* cell_w_dev, int num_keypoints,
                               void* out_fp16_dev, void* stream);

/* Bilinear descriptor sampling at keypoint pixels: the stage twin of SSHIP_DESC_BILINEAR below (upstream cvg/LightGlue superpoint.py
 * sample_descriptors; the reference has no counterpart).  kp_xy_dev is a device array of num_keypoints x (x, y) fp32 SCORE-MAP pixels
 * (the grid covers 8*grid_w x 8*grid_h of them); out is [num_keypoints, channels] fp16.  For each keypoint, with D the grid:
 *   gx = (x - 3.5) / (8*grid_w - 4.5) * (grid_w - 1)        gy = (y - 3.5) / (8*grid_h - 4.5) * (grid_h - 1)
 *   x0 = floor(gx), fx = gx - x0                            y0 = floor(gy), fy = gy - y0
 *   v[c] = (1-fy)(1-fx) D[c,y0,x0] + (1-fy)fx D[c,y0,x0+1] + fy(1-fx) D[c,y0+1,x0] + fy fx D[c,y0+1,x0+1]
 *   out[c] = fp16( v[c] / max(||v||_2, 1e-12) )
 * i.e. grid_sample(mode = bilinear, align_corners = True, padding_mode = zeros) + F.normalize: a corner outside the grid contributes
 * zero (only for x < 3.5 or y < 3.5); grid_w == 1 or grid_h == 1 gives g = 0 on that axis.  Weights, blend, sum of squares and division
 * are fp32.  channels in [1, 256]; num_keypoints <= 0 is a no-op.  sship_sample_descriptors_bilinear reads a CHW grid
 * [channels, grid_h, grid_w] (the reference engine's layout, what sship_sp_dense returns), the _hwc variant a channels-last grid
 * [grid_h, grid_w, channels] (channels a multiple of 4). */
int sship_sample_descriptors_bilinear(const void* grid_fp16_dev, int channels, int grid_h, int grid_w,
                                      const float* kp_xy_dev, int num_keypoints, void* out_fp16_dev, void* stream);
int sship_sample_descriptors_bilinear_hwc(const void* grid_fp16_dev, int channels, int grid_h, int grid_w,
                                          const float* kp_xy_dev, int num_keypoints, void* out_fp16_dev, void* stream);

/* Sub-pixel keypoint refinement: the stage twin of SSHIP_KP_SUBPIXEL below (the reference has no counterpart).  The three-point
 * Gaussian (log-parabola) peak fit, per axis, on the PRE-NMS log-probabilities of a Hc x Wc grid of 65-logit cells:
 *   L[h, w] = logit[cell(h, w), pos(h, w)] - logsumexp(all 65 logits of that cell)      cell = (h / 8, w / 8), pos = 8 (h % 8) + (w % 8)
 * the log of the softmax score the NMS compared (the dustbin, logit 64, is part of the normaliser).  For a keypoint at the integer
 * score-map pixel (h, w), on the x axis:
 *   a = L[h, w-1], b = L[h, w], c = L[h, w+1], den = 2b - a - c
 *   dx = clamp(0.5 (c - a) / den, -0.5, 0.5)  if both neighbours are inside the 8Hc x 8Wc map and den > 0, else dx = 0
 * and dy the same with L[h-1, w] and L[h+1, w].  Neighbours inside an extractor's remove_borders band are inside the map and are used.
 * All of it is fp32 (log-scores as (v - max) - log(sum of exponentials)).
 *   - A keypoint is a 9x9 maximum of the score, so b >= a and b >= c and |dx| <= 0.5 holds without the clamp, which only guards rounding.
 *   - Refined keypoints therefore stay at least nms_radius pixels apart.
 *   - A neighbour may lie in another cell and have another normaliser: that is why L is used and not the raw logit.
 *   - Scores that are samples of a Gaussian inside one cell return its mean exactly.
 * pix_dev: num_keypoints packed pixels (h << 16) | w, the packing k_topk writes; a pixel outside the map is clamped into it.
 * offsets_dev: [num_keypoints, 2] fp32 = (dx, dy).  num_keypoints <= 0 is a no-op before any other check; otherwise NULL pointers or
 * Hc, Wc < 1 (or > 8191) -> SSHIP_ERR_INVALID.  No input can make a lane read outside the buffer.
 * sship_refine_keypoints reads CHW logits [65, Hc, Wc] (what sship_sp_dense returns), the _hwc variant cell-major rows
 * [Hc, Wc, row_stride] with row_stride >= 65 (the extractor's own buffer has 68: 16-byte aligned rows are read 16 bytes at a time). */
int sship_refine_keypoints(const float* logits_chw_dev, int Hc, int Wc, const int* pix_dev, int num_keypoints, float* offsets_dev,
                           void* stream);
int sship_refine_keypoints_hwc(const float* logits_dev, int row_stride, int Hc, int Wc, const int* pix_dev, int num_keypoints,
                               float* offsets_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Detector post-processing stages (exposed so each can be parity-tested bit-exactly)
 * ---------------------------------------------------------------------------------------------- */
/* utils/convert_superpoint_to_onnx.py:82-87: pooled = max_pool2d(s, 2r+1, 1, r); s = (s==pooled)?s:0. */
int sship_nms(const float* scores_dev, int batch, int h, int w, int radius, float* out_dev, void* stream);
/* src/SuperPoint.cc:696-719 on one device score map: strict `score > thr` (thr is a double) inside the
 * border, descending (score, h, w) order, first max_kp; kp (x = w*input_w/score_w, y = h*input_h/score_h,
 * score) triples, cells = min(h/8, desc_h-1), min(w/8, desc_w-1).  All outputs are device arrays
 * ([3*max_kp] f32, [max_kp] i32, [max_kp] i32, [1] i32); n_candidates_dev may be NULL.
 * Unlike the other entries that take a stream, this stage and its balanced twin below are NOT asynchronous: they own no handle, so the
 * candidate list is allocated per call, the launches go to `stream` in order, and the call returns after synchronising `stream` (the
 * scratch dies with the call).  They are parity-test stages; an extractor's own selection (sship_sp_extract_batch_device) is asynchronous. */
int sship_select_topk(const float* scores_dev, int score_h, int score_w, int input_h, int input_w,
                      double thr, int border, int max_kp, int desc_h, int desc_w, float* kp_xys_dev,
                      int* cell_h_dev, int* cell_w_dev, int* n_dev, int* n_candidates_dev, void* stream);
/* The same stage with the spatially balanced rule stated at sship_sp_set_keypoint_selection below (SSHIP_SELECT_BALANCED, G = bucket_px in
 * [8, 65535]): same candidates, same outputs and output order, n_candidates = M.  Bad arguments are refused before any device is touched. */
int sship_select_topk_balanced(const float* scores_dev, int score_h, int score_w, int input_h, int input_w,
                               double thr, int border, int max_kp, int bucket_px, int desc_h, int desc_w, float* kp_xys_dev,
                               int* cell_h_dev, int* cell_w_dev, int* n_dev, int* n_candidates_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SuperPoint extractor - include/SuperPoint.h:36-54, src/SuperPoint.cc
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_sp sship_sp;
typedef struct {
  const char* weights_path;  /* safetensors with the reference's state-dict keys (conv1a.weight ...).  Takes
                                the place of SuperPoint's engine_file (src/SuperSLAM.cc:72-78). */
  int max_keypoints;         /* superpoint.max_keypoints (600 in the KITTI YAML) */
  double keypoint_threshold; /* superpoint.keypoint_threshold (0.005) */
  int remove_borders;        /* superpoint.remove_borders (4) */
  int nms_radius;            /* exporter --nms-radius (4) */
  int pool_slots;            /* include/SuperPoint.h:77-78 descriptor_pool_slots (8); 0 -> 8 */
  int max_batch;             /* images per call the workspaces are sized for (2 = stereo); 0 -> 2 */
} sship_sp_config;

/* One image's extraction result.  kp_xys is caller-owned [3*max_keypoints] (x, y, score per keypoint -
 * cv::KeyPoint(x, y, 1, -1, score), src/SuperPoint.cc:715).  desc_dev points into pool slot `slot`
 * ([n, 256] fp16 row-major, L2-normalised); the caller owns the slot and returns it with
 * sship_pool_release(sship_sp_pool(sp), slot).  n == 0 -> slot = -1, desc_dev = NULL (success). */
typedef struct {
  float* kp_xys;
  int n;
  void* desc_dev;
  int slot;
} sship_features;

int sship_sp_create(const sship_sp_config* cfg, sship_sp** out); /* ctor + initialize() */
void sship_sp_destroy(sship_sp* sp);
sship_pool* sship_sp_pool(sship_sp* sp);
int sship_sp_max_keypoints(const sship_sp* sp);
/* How the descriptor of a keypoint is read from the descriptor map.  Per handle; it applies to every call made after it returns, through
 * every entry point that yields per-keypoint descriptors: sship_sp_extract, _extract_stereo, _extract_stereo_ring, _ring_submit,
 * _infer_host, _extract_batch_device and sship_frontend_batch_device (and sship_sp_bench_layer(14) times the head the mode selects).
 *   SSHIP_DESC_NEAREST (default): the reference's rule, the cell the keypoint falls in (cell = coord / 8, src/DescriptorGather.cu),
 *     renormalised - today's path, bit for bit, with the launches it always made.
 *   SSHIP_DESC_BILINEAR: upstream SuperPoint's sample_descriptors, which the reference's export replaced by the nearest-cell gather and
 *     which the published LightGlue weights were trained on: the rule stated at sship_sample_descriptors_bilinear above, with D = the
 *     fp16 dense descriptor map (what sship_sp_dense returns) and (x, y) = the keypoint's integer score-map pixel (w, h) BEFORE the
 *     rescale to input pixels.  The map is not materialised: convDa / convDb run at the four corner cells of every keypoint.
 * The mode changes descriptors ONLY: keypoints, scores and counts do not depend on it.
 * Any other mode or a NULL handle -> SSHIP_ERR_INVALID, the mode unchanged; also SSHIP_ERR_INVALID while a sship_sp_ring_submit is
 * pending (collect it first).  In the developer build, SUPERSLAM_HIP_DESC=dense has no bilinear form: the setter refuses
 * SSHIP_DESC_BILINEAR there with SSHIP_ERR_INVALID. */
enum { SSHIP_DESC_NEAREST = 0, SSHIP_DESC_BILINEAR = 1 };
int sship_sp_set_descriptor_sampling(sship_sp* sp, int mode);
int sship_sp_descriptor_sampling(const sship_sp* sp);
/* Where a keypoint is reported.  Per handle; it applies to every call made after it returns, through every entry point that yields
 * keypoints: sship_sp_extract, _extract_stereo, _extract_stereo_ring, _ring_submit, _infer_host, _extract_batch_device and
 * sship_frontend_batch_device (LightGlue then receives the refined coordinates).
 *   SSHIP_KP_INTEGER (default): the reference's rule, x = w * scale_x, y = h * scale_y at the integer score-map pixel (h, w)
 *     (src/SuperPoint.cc:711-719) - today's path, bit for bit, with the launches it always made.
 *   SSHIP_KP_SUBPIXEL: x = ((float)w + dx) * scale_x, y = ((float)h + dy) * scale_y with the same fp32 scales and (dx, dy) from the rule
 *     stated at sship_refine_keypoints below, evaluated on the detector logits of the same call.  One more launch (k_kp_refine), in
 *     this mode only.  The reference has no counterpart.
 * The mode changes x and y ONLY: counts, order, the score kp[2], the cells and the descriptors are the same bits as with the mode off.
 * In both descriptor-sampling modes the descriptors keep reading the integer pixel; the two modes are independent.
 * Any other mode or a NULL handle -> SSHIP_ERR_INVALID, the mode unchanged; also SSHIP_ERR_INVALID while a sship_sp_ring_submit is
 * pending (collect it first).  In the developer build the setter would refuse SSHIP_KP_SUBPIXEL under a SUPERSLAM_HIP_CONVPB* /
 * _CONV* switch that does not leave the fp32 logits in device memory; every switch there is today leaves them. */
enum { SSHIP_KP_INTEGER = 0, SSHIP_KP_SUBPIXEL = 1 };
int sship_sp_set_keypoint_refinement(sship_sp* sp, int mode);
int sship_sp_keypoint_refinement(const sship_sp* sp);   /* NULL -> SSHIP_KP_INTEGER */
/* Which candidates become keypoints.  Per handle; it applies to every call made after it returns, through every entry point that yields
 * keypoints: sship_sp_extract, _extract_stereo, _extract_stereo_ring, _ring_submit, _infer_host, _extract_batch_device and
 * sship_frontend_batch_device.
 *   SSHIP_SELECT_TOPK (default): the reference's rule, the max_keypoints highest scores of the whole image (src/SuperPoint.cc:696-719) -
 *     today's path, bit for bit, with the launches it always made.  bucket_px is ignored.
 *   SSHIP_SELECT_BALANCED: the keypoints are spread over square buckets of G = bucket_px score-map pixels.  One more launch
 *     (k_select_balanced, between the candidate compaction and the top-k), in this mode only.  The reference has no counterpart.
 * The rule.  The candidates of an image are exactly the default mode's: the pixels (h, w) of the H x W score map that survive NMS, lie
 * inside the border and have score > thr, each with the 64-bit key k = (bits(score) << 32) | (h * W + w); M is their number.
 *   Bucket:  the bucket of a candidate is (h / G, w / G) by integer division; the last row and column of buckets may be ragged.
 *   Rank:    r(c) = the number of candidates in the same bucket with a key greater than k(c); the best of every occupied bucket has rank 0.
 *   Selection order: c comes before c' if r(c) < r(c'), or if the ranks are equal and k(c) > k(c').  The selected set is the first
 *            K = min(M, max_keypoints) candidates in this order.
 *   Output order: the selected set is written in DESCENDING KEY ORDER, the default mode's order; keypoints, scores, cells and n have the
 *            layout and meaning they always had, and n_candidates stays M.
 * Everything is integer comparison of existing bits: there is no tolerance in this mode.  Three consequences:
 *   - n does not depend on the mode.
 *   - If M <= max_keypoints, the output is bit-identical to the default mode.
 *   - If G >= max(H, W), there is one bucket, and the output is bit-identical to the default mode.
 * The mode is independent of descriptor sampling and keypoint refinement: both act on the balanced set as they act on the default one.
 * bucket_px must be in [8, 65535] for SSHIP_SELECT_BALANCED (8 = one descriptor cell; nothing finer is useful behind a 9 x 9 NMS).
 * An unknown mode, a bucket_px out of range or a NULL handle -> SSHIP_ERR_INVALID, mode and bucket unchanged; also SSHIP_ERR_INVALID while
 * a sship_sp_ring_submit is pending (collect it first).  The setter allocates nothing: the mode's buffers (the selected keys, and a
 * workspace of 8 bytes per score-map pixel plus 12 per cell and image) are sized by the next call, where the handle's other selection
 * buffers are.  Cost: the kernel keeps an image's keys in LDS when it has at most 8192 candidates and 1024 buckets; beyond that it works in
 * the workspace, where a bucket of s candidates costs up to s^2 key comparisons. */
enum { SSHIP_SELECT_TOPK = 0, SSHIP_SELECT_BALANCED = 1 };
int sship_sp_set_keypoint_selection(sship_sp* sp, int mode, int bucket_px);
int sship_sp_keypoint_selection(const sship_sp* sp, int* bucket_px_out);   /* NULL handle -> SSHIP_SELECT_TOPK; bucket_px_out may be NULL */

/* SuperPoint::extract (src/SuperPoint.cc:895-899 -> infer_device :597-676): host u8 image, 1 or 3 (BGR)
 * channels, row stride in bytes.  Synchronous. */
int sship_sp_extract(sship_sp* sp, const uint8_t* img, int h, int w, int stride, int channels,
                     sship_features* out);
/* SuperPoint::extract_stereo (src/SuperPoint.cc:902-908 -> infer_device_stereo :754-892): one batch-2
 * pass; the pair must share resolution (:762-765). */
int sship_sp_extract_stereo(sship_sp* sp, const uint8_t* left, const uint8_t* right, int h, int w,
                            int stride, int channels, sship_features* out_left, sship_features* out_right);
/* Decode-ahead upload ring for dataset runners.  No reference counterpart: the reference stages every frame
 * in-line (clone + convertTo + memcpy into one pinned buffer + H2D, src/SuperPoint.cc:768-795); here `depth` stereo frames live in
 * pinned host memory, so a decoder thread writes pixels straight into a slot (sship_sp_ring_host), starts its H2D on the ring's
 * own copy stream (sship_sp_ring_upload - the one call that may run on another thread than the handle's owner), and the
 * tracking thread extracts from the uploaded slot (sship_sp_extract_stereo_ring = sship_sp_extract_stereo without the host
 * copy and with the upload already overlapped with the previous frame's compute).  Images are [h][w*channels] u8, 1 or 3 (BGR)
 * channels; the caller keeps slot reuse behind the extract call that consumes it. */
int sship_sp_ring_create(sship_sp* sp, int depth, int h, int w, int channels);
uint8_t* sship_sp_ring_host(sship_sp* sp, int slot, int image /* 0 left, 1 right */);
int sship_sp_ring_upload(sship_sp* sp, int slot);
int sship_sp_extract_stereo_ring(sship_sp* sp, int slot, sship_features* out_left, sship_features* out_right);
/* Cross-frame pipelining for the per-frame path (no reference counterpart: the reference runs extract -> match -> estimator
 * strictly in sequence, src/StereoFrontEnd.cc:10-48).  sship_sp_ring_submit ENQUEUES the whole extraction of an uploaded slot
 * (network, selection, descriptor head into two freshly acquired pool slots, D2H of keypoints / counts into the slot's own
 * pinned buffers) on the extractor's stream and returns at once; the later sship_sp_extract_stereo_ring(slot) only waits for
 * that work's completion event and hands the results out.  Called right after frame t's extraction has returned - before frame
 * t's LightGlue match - it lets frame t+1's SuperPoint kernels share the GPU with frame t's matcher (the matcher's launches
 * cover a fraction of the CUs at one pair).  Same thread as every other call on this handle; at most one submission per slot.
 * Pool budget: a submission acquires its two pool slots when it is ENQUEUED, not when it is collected.  The per-frame schedule of
 * examples/frontend_benchmark.cc (submit t+1 right after collecting t, keep the previous frame's left features for the temporal
 * match) therefore holds 2 slots in flight + 2 being matched + 1 held = 5 of the default 8 (cfg.pool_slots); a consumer that keeps
 * more than 3 further handles alive exhausts the pool at the next submission (tests/test_gpu_runner_frames.py asserts the 5).
 * Constraints while a submission is pending (submitted, not yet collected):
 *   - sship_sp_ring_upload(slot) on that slot returns SSHIP_ERR_INVALID: the queued network still reads the slot's device
 *     frame (collect first, then refill);
 *   - the synchronous extractor calls (sship_sp_extract*, sship_sp_extract_stereo_ring of another slot) run on the handle's
 *     own stream and are ordered behind the submission;
 *   - sship_sp_extract_batch_device / sship_frontend_batch_device on a caller-supplied NON-BLOCKING stream share the handle's
 *     activations with the submission and are NOT ordered with it: do not overlap them with a pending submission;
 *   - sship_sp_destroy with a submission pending waits for it and returns its pool slots.
 * Stage timings: sship_sp_ring_submit restarts the calling thread's stage marks, so under pipelining
 * sship_get_stage_timings mixes frame t+1's extraction stages with frame t's match stages - profile un-pipelined. */
int sship_sp_ring_submit(sship_sp* sp, int slot);
/* SuperPoint::infer host path (src/SuperPoint.cc:322-348,427-528): keypoints + CV_32F [n,256] descriptors
 * on the host.  kp_xys [3*max_kp], desc_f32 [max_kp*256]. */
int sship_sp_infer_host(sship_sp* sp, const uint8_t* img, int h, int w, int stride, int channels,
                        float* kp_xys, float* desc_f32, int* n);

/* Throughput path: `batch` grayscale u8 images already resident in HBM ([batch, h, w] contiguous); results
 * stay on the device: desc [batch, max_kp, 256] f16, kp [batch, max_kp, 3] f32, n [batch] i32.
 * Asynchronous on `stream`; no host synchronisation anywhere inside. */
int sship_sp_extract_batch_device(sship_sp* sp, const uint8_t* imgs_dev, int batch, int h, int w,
                                  void* desc_out_dev, float* kp_out_dev, int* n_out_dev, void* stream);

/* Dense outputs of the network, in the reference engine's layouts (scripts/rebuild_engines.sh:88-97):
 * scores f32 [batch, 8*(h/8), 8*(w/8)] after NMS, descriptors f16 [batch, 256, h/8, w/8] (CHW,
 * L2-normalised).  logits_dev (optional) receives the raw detector logits f32 [batch, 65, h/8, w/8].
 * Any output pointer may be NULL. */
int sship_sp_dense(sship_sp* sp, const uint8_t* imgs_dev, int batch, int h, int w, float* scores_dev,
                   void* desc_grid_dev, float* logits_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LightGlue matcher - include/LightGlue.h:28-63, src/LightGlue.cc
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_lg_weights sship_lg_weights; /* LightGlueEngine analogue (refcounted, immutable) */
typedef struct sship_lg sship_lg;

int sship_lg_weights_load(const char* safetensors_path, sship_lg_weights** out);
void sship_lg_weights_retain(sship_lg_weights* w);
void sship_lg_weights_release(sship_lg_weights* w);

/* LightGlue(engine, image_width, image_height) + initialize().  max_keypoints bounds n0/n1 (the reference
 * engine's profile max is 1024, scripts/rebuild_engines.sh:118); max_pairs sizes the batched workspaces. */
int sship_lg_create(sship_lg_weights* w, int image_width, int image_height, int max_keypoints,
                    int max_pairs, sship_lg** out);
void sship_lg_destroy(sship_lg* lg);

/* Keypoint normalisation, src/LightGlue.cc:241-251: (pt - (W/2,H/2)) / (max(W,H)/2).  kp_xy has `stride`
 * floats per keypoint (2 or 3); out is [n,2]. */
int sship_lg_normalize_keypoints(const sship_lg* lg, const float* kp_xy, int stride, int n, float* out);

/* Device match, src/LightGlue.cc:377-457: host keypoints (pixel coordinates, `kp_stride` floats apart),
 * descriptors resident in pool slots ([n,256] fp16).  Outputs on the host: matches0 [n0] (index into set 1
 * or -1), mscores0 [n0].  n0 == 0 or n1 == 0 -> SSHIP_ERR_INVALID (the reference returns an empty result). */
int sship_lg_match_device(sship_lg* lg, const float* kp0, int kp_stride0, int n0, const void* desc0_dev,
                          const float* kp1, int kp_stride1, int n1, const void* desc1_dev,
                          int32_t* matches0, float* mscores0);
/* Host-descriptor match, src/LightGlue.cc:285-324: CV_32F [n,256] descriptors, converted to fp16 and
 * uploaded internally (the loop-closure overload). */
int sship_lg_match_host(sship_lg* lg, const float* kp0, int kp_stride0, int n0, const float* desc0_f32,
                        const float* kp1, int kp_stride1, int n1, const float* desc1_f32,
                        int32_t* matches0, float* mscores0);
/* Throughput path: `pairs` independent problems, everything device-resident and asynchronous.
 * kp_dev [2*pairs, max_kp, 3] (pixel x, y, score), n_dev [2*pairs], desc_dev [2*pairs, max_kp, 256] f16,
 * image 2p is set 0 and image 2p+1 is set 1 of pair p.  Outputs matches0_dev / mscores0_dev
 * [pairs, max_kp]; rows >= n are -1 / 0. */
int sship_lg_match_batch_device(sship_lg* lg, const float* kp_dev, const int* n_dev, const void* desc_dev,
                                int pairs, int32_t* matches0_dev, float* mscores0_dev, void* stream);
/* Adaptive depth (upstream LightGlue's depth_confidence; the reference has no counterpart: its ONNX export turns it off).
 * Per handle, OFF by default; it applies to every call enqueued after it returns (one call in flight per handle, as everywhere here),
 * through every entry point: sship_lg_match_device / _match_host / _match_batch_device and sship_frontend_batch_device.
 * With depth_confidence = d in (0, 1] each pair p of a call is decided on its own:
 *   after layer i (i = 0..7, self and cross block of both images), c = sigmoid(w_i . x + b_i) for every valid token of both images,
 *   (w_i, b_i) = token_confidence.{i}.token.0.{weight,bias}, x = the residual stream after layer i; thr_i = fp32(clip(0.8 + 0.1 exp(-4 i / 9), 0, 1)).
 *   The pair stops after layer i if  1 - count(c < thr_i) / (n0 + n1) > d  (fp32, this form; n0 + n1 = 0 never stops) and is matched with
 *   log_assignment[i] (final_proj and matchability) on x after layer i; a pair that never stops runs nine layers and uses log_assignment[8].
 *   The filter (threshold 0.1, mutual check) is unchanged.  A pair's result does not depend on the other pairs of the call.
 * sship_lg_set_depth_confidence: d <= 0 turns it off (today's path, bit for bit); NaN or d > 1 -> SSHIP_ERR_INVALID; d > 0 with weights that
 *   lack any of token_confidence.{0..7} or log_assignment.{0..7} -> SSHIP_ERR_INVALID (the handle keeps its previous setting).
 * sship_lg_layers_run: layers run by each of the first `pairs` pairs of the last call (i + 1 for a pair that stopped after layer i, 9
 *   otherwise; upstream's `stop`), device-synchronising like sship_lg_debug_read.  With the option off every pair reports the layers run. */
int sship_lg_set_depth_confidence(sship_lg* lg, float depth_confidence);
int sship_lg_layers_run(sship_lg* lg, int* out_host, int pairs);
/* Adaptive width (upstream LightGlue's width_confidence / get_pruning_mask; the reference has no counterpart: its ONNX export turns it off).
 * Per handle, OFF by default; it applies to every call enqueued after it returns, through every entry point, like adaptive depth above.
 * With width_confidence = w in (0, 1] and min_keypoints = K >= 0, after layer i (i = 0..7, never after the last layer), for every pair
 * that is still running after the depth decision of layer i (a pair that stops at layer i is matched on the tokens it had during layer i),
 * and for each of its two images on its own:
 *   the image is pruned at this layer only if its live count is > K (upstream's pruning_th, an explicit argument here; 0 = always);
 *   s_t = sigmoid(log_assignment.{i}.matchability(x_t)) for every live token, x = the residual stream after layer i;
 *   keep_t = s_t > 1 - w (fp32, this form); with adaptive depth also on, keep_t |= c_t <= thr_i with the c and thr_i above (tokens of low
 *   confidence are never pruned); with depth off there is no second term;
 *   the kept tokens, in their original order, are the image's tokens for layers i + 1 ..; prune[t] += 1 for every kept token (prune
 *   starts at 1: upstream's prune0 / prune1);
 *   if either image of a pair has no token left the pair is finished: matches0 = -1, mscores0 = 0, layers_run = i + 1.
 * The assignment (log_assignment[layers_run - 1], the unchanged filter) runs on the live sets and is mapped back to keypoint indices;
 * pruned keypoints get -1 / 0, rows >= n stay -1 / 0.  A pair's result does not depend on the other pairs of the call.
 * sship_lg_set_width_confidence: w <= 0 turns it off (today's path, bit for bit); NaN, w > 1 or K < 0 -> SSHIP_ERR_INVALID; w > 0 with
 *   weights that lack any log_assignment.{0..7}.matchability -> SSHIP_ERR_INVALID (the handle keeps its previous setting).  The
 *   token-confidence heads are needed only when adaptive depth is on.
 * sship_lg_prune_counts: prune0[0 .. n0) / prune1[0 .. n1) of pair `pair` of the last call, device-synchronising like
 *   sship_lg_layers_run.  With the option off every keypoint reports 9 (as upstream does). */
int sship_lg_set_width_confidence(sship_lg* lg, float width_confidence, int min_keypoints);
int sship_lg_prune_counts(sship_lg* lg, int pair, int32_t* prune0, int n0, int32_t* prune1, int n1);
/* Test-only introspection of the matcher (no reference counterpart; used by the parity suite to compare the internals
 * with the oracle layer by layer - the product never calls these).
 * sship_lg_debug_set_layers: the NEXT match call on this handle (one-shot) runs only the first n_layers (1..9) transformer
 *   layers and skips the assignment (matches0 = -1, mscores0 = 0); the call after it is a full match again.
 * sship_lg_debug_read: after a match call, copy state of this handle to the host as f32 (device-synchronising):
 *   SSHIP_LG_DEBUG_X    residual stream of sequence `index` (2p = set 0, 2p+1 = set 1 of pair p): out[rows][256]
 *   SSHIP_LG_DEBUG_SIM  assignment similarity md0 md1^T of pair `index`: out[rows][cols]
 *   SSHIP_LG_DEBUG_KPTS normalised keypoints of sequence `index` (src/LightGlue.cc:241-251 on the device): out[rows][2]
 *   SSHIP_LG_DEBUG_ROPE rotary table of sequence `index`: out[rows][64] = 32 (cos, sin) pairs
 *   SSHIP_LG_DEBUG_IND  original keypoint index of each live row of sequence `index`: out[rows][1] (0, 1, 2 .. with adaptive width off)
 * With adaptive width on, SSHIP_LG_DEBUG_X and SSHIP_LG_DEBUG_ROPE return the COMPACTED stream: row a is keypoint IND[a], rows past the live count are padding. */
enum { SSHIP_LG_DEBUG_X = 0, SSHIP_LG_DEBUG_SIM = 1, SSHIP_LG_DEBUG_KPTS = 2, SSHIP_LG_DEBUG_ROPE = 3, SSHIP_LG_DEBUG_IND = 4 };
int sship_lg_debug_set_layers(sship_lg* lg, int n_layers);
int sship_lg_debug_read(sship_lg* lg, int what, int index, int rows, int cols, float* out);
/* Test-only: per-stage capture of the matcher (tests/test_gpu_lg_stages.py judges every launch from the inputs it read).  The residual
 * stream is updated in place and q / k / v^T / ctx are overwritten by every block, so nothing but the last state can be read after a call
 * unless it was copied aside while the call ran.
 * sship_lg_debug_capture(lg, pairs, count): count in 0 .. 8 pair indices of later calls; count = 0 (the default) turns capture off, and off
 *   costs one host branch per stage: no allocation, no launch, and no kernel knows about it.  On, every later match call of the handle (the
 *   batch-device and the single-pair entries alike) enqueues, right after the launch that produces a stage and on the stream that ran it (on
 *   the two-stream path each half copies its own pairs on its own stream), a device-to-device copy of that stage's slice of every listed pair
 *   that the call holds.  matches0 / mscores0 keep their bits.  With adaptive depth or adaptive width on the same stages are captured (X_OUT
 *   before the layer's pruning step, the next layer's X_IN / Q_S / K_S / V_S after it and after the re-projection), the state of the two modes
 *   in addition (sship_lg_debug_adaptive below), and layers_run / prune_counts keep their values too.  Negative or repeated pair indices ->
 *   SSHIP_ERR_INVALID.  Switching forgets what was captured.
 * sship_lg_debug_stage(lg, slot, layer, stage, out, floats): stage `stage` of layer `layer` (0 .. 8) of the pair listed at position `slot`,
 *   from the LAST call, as fp32 in natural order, device-synchronising: out[2][NP][256] (set 0, set 1 of the pair; NP = the handle's padded
 *   sequence length, max_keypoints rounded up to 32), out[2][NP] for LOGSIG; `floats` must be exactly that size.  Rows past a sequence's
 *   length are padding (whatever the buffers held).  SSHIP_ERR_INVALID for a stage, layer or slot that does not exist, for a slot whose pair
 *   the last call did not hold, and while capture is off or no call has run since it was switched on.
 * Stages (per layer, in launch order; `s` the softmax scale folded into the weights on the host, L = log2 e):
 *    0 X_IN    residual stream entering the layer (layer 0: the fp16 descriptors, zero rows for padding)
 *    1 Q_S     SelfBlock q [head h = c / 64][d = c % 64]: (Wq x + bq) * (L / 8), then rotary; the kernel stores it in MFMA B-fragment order
 *              [seq][h][token / 32][d / 16][lane = ((d % 16) / 8) * 32 + token % 32][d % 8], un-permuted here
 *    2 K_S     SelfBlock k, rotary, no scale; stored like Q_S
 *    3 V_S     SelfBlock v (no rotary, no scale); the kernel stores V^T in the PV A-fragment order
 *              [seq][h][token / 32][kk = (token % 32) / 16][d / 32][lane = hh * 32 + d % 32][e], r = token % 16, hh = (r % 8) / 4,
 *              e = r % 4 + 4 (r / 8), un-permuted here
 *    4 CTX_S   self-attention output softmax(q k^T) v per head, channels [h][d] (the output projection is folded into ffn.0)
 *    5 X_MID   residual stream after the SelfBlock FFN
 *    6 QK_C    CrossBlock to_qk(x) * (64^-1/4 * sqrt(L)) (shared by both directions, no rotary); stored like Q_S
 *    7 V_C     CrossBlock to_v(x); stored like V_S
 *    8 CTX_C   cross-attention output (sequence s attends to its partner s ^ 1)
 *    9 X_OUT   residual stream after the CrossBlock FFN
 *   10 MD      layer 8 only: final_proj(x) * 256^-1/4, fp16 [NP][256]
 *   11 LOGSIG  layer 8 only: logsigmoid(matchability(x)), fp32 [NP] */
enum { SSHIP_LG_STAGE_X_IN = 0, SSHIP_LG_STAGE_Q_S = 1, SSHIP_LG_STAGE_K_S = 2, SSHIP_LG_STAGE_V_S = 3, SSHIP_LG_STAGE_CTX_S = 4,
       SSHIP_LG_STAGE_X_MID = 5, SSHIP_LG_STAGE_QK_C = 6, SSHIP_LG_STAGE_V_C = 7, SSHIP_LG_STAGE_CTX_C = 8, SSHIP_LG_STAGE_X_OUT = 9,
       SSHIP_LG_STAGE_MD = 10, SSHIP_LG_STAGE_LOGSIG = 11 };
int sship_lg_debug_capture(sship_lg* lg, const int* pairs, int count);
int sship_lg_debug_stage(sship_lg* lg, int slot, int layer, int stage, float* out, unsigned long long floats);
/* Test-only: what the capture kept of the adaptive modes (tests/test_gpu_lg_adaptive_stages.py), for the pair listed at `slot`, from the LAST
 * call, device-synchronising.  Every item is an array of 4-byte values, int32 or f32 as listed; `count` must be exactly its length.  A stopped
 * pair's items of later layers are copied all the same (they show that nothing touched it).  SSHIP_ERR_INVALID as for sship_lg_debug_stage,
 * and when the last call ran with both modes off, for an item of adaptive width when width was off, and for the last four items after a
 * truncated run (sship_lg_debug_set_layers).  `layer` must be 0 for the items that have none.
 *    0 LENS        int32 [2]           layer 0 .. 8: the two counts the attention launches of the layer read (0, 0 for a pair that is not running)
 *    1 ROPE        f32 [2][NP][64]     layer 0 .. 8: the pair's rotary table as the layer read it
 *    2 IND         int32 [2][NP]       layer 0 .. 7, width: original keypoint index of every live row after the pruning step of the layer
 *    3 PRUNE       int32 [2][NP]       layer 0 .. 7, width: prune counts by original index after that step
 *    4 WLEN        int32 [2]           layer 0 .. 7, width: live tokens after that step
 *    5 CHG         int32 [2]           layer 0 .. 7, width: 1 where the sequence lost tokens at that step
 *    6 CNT         int32 [8]           tokens counted below the threshold after layer 0 .. 7 (0 where the pair was not running, or depth is off)
 *    7 LAYERS_RUN  int32 [1]           as sship_lg_layers_run
 *    8 MD          f32 [2][NP][256]    the fp16 rows the assignment read: the exit head's for a pair that stopped early
 *    9 LOGSIG      f32 [2][NP]         likewise
 *   10 MATCHES_C   int32 [max_kp]      width: matches of the live rows before they are mapped back through IND
 *   11 MSCORES_C   f32 [max_kp]        width: their scores */
enum { SSHIP_LG_ADAPT_LENS = 0, SSHIP_LG_ADAPT_ROPE = 1, SSHIP_LG_ADAPT_IND = 2, SSHIP_LG_ADAPT_PRUNE = 3, SSHIP_LG_ADAPT_WLEN = 4,
       SSHIP_LG_ADAPT_CHG = 5, SSHIP_LG_ADAPT_CNT = 6, SSHIP_LG_ADAPT_LAYERS_RUN = 7, SSHIP_LG_ADAPT_MD = 8, SSHIP_LG_ADAPT_LOGSIG = 9,
       SSHIP_LG_ADAPT_MATCHES_C = 10, SSHIP_LG_ADAPT_MSCORES_C = 11 };
int sship_lg_debug_adaptive(sship_lg* lg, int slot, int layer, int what, void* out, unsigned long long count);
/* Test-only: copy one activation of the extractor's LAST call to the host, raw (channels-last [batch][h_l][w_l][c_l]), device-synchronising.
 * layer: 1 conv1b (+pool), 2 conv2a, 3 conv2b (+pool), 4 conv3a, 5 conv3b (+pool), 6 conv4a, 7 conv4b (the ids of sship_sp_bench_layer), all fp16;
 * and the heads: 8 convPa, fp16 [B,Hc,Wc,256]; 9 convDa, the same layout, filled only by sship_sp_dense called with a descriptor grid;
 * 10 convDb's raw output before normalisation, fp16 [B,Hc,Wc,256], sship_sp_dense with a grid only; 11 convPb's logits, fp32 [B,Hc,Wc,68]:
 * 65 meaningful values at the head of every 68-float row.
 * Used by the parity suite to compare single layers with an fp64 convolution of the previous layer's activation (tests/test_gpu_sp_layers.py);
 * the product never calls it.  `bytes` must not exceed the activation's size.
 * Layer 2 (conv2a) is materialised only where conv2a and conv2b run as two launches: in the shipped library when the fused kernel
 * (csrc/conv_fuse2.hip, whose intermediate map never leaves the CU) does not fit - maps under 8 pixels, an 8x8 image for one - and in the developer
 * build under SUPERSLAM_HIP_CONV2=split / SUPERSLAM_HIP_CONV64=wino.  After a fused run its buffer holds an earlier run's map or nothing. */
int sship_sp_debug_activation(sship_sp* sp, int layer, void* out_host, unsigned long long bytes);
/* Match post-processing, src/LightGlue.cc:326-363: ascending i, skip -1, distance = 1 - score.
 * Returns the number of matches (>= 0). */
int sship_filter_matches(const int32_t* matches0, const float* mscores0, int n0, int* query_idx,
                         int* train_idx, float* distance);
/* LightGlue::descriptors_to_host, src/LightGlue.cc:460-475: fp16 [count, dim] device -> f32 host. */
int sship_desc_to_host(const void* desc_dev, int count, int dim, float* out_f32);

/* ------------------------------------------------------------------------------------------------
 * Nearest-neighbour matcher - a second superslam::IFeatureMatcher ("Pluggable feature matcher", include/InferenceInterfaces.h) next to
 * LightGlue: hloc's NN-mutual / NN-ratio / NN-superpoint (hloc/matchers/nearest_neighbor.py) and the reference's own cosineMatch
 * (tests/test_superpoint_cosine_matching.cc).  No weights, no image size.  About 200 times less arithmetic than the LightGlue stack: a
 * cheap pre-verification of loop candidates, a fallback without LightGlue weights, and the baseline LightGlue is judged against.
 * Inputs are two descriptor sets d0 [n0, 256] and d1 [n1, 256], fp16 row-major (the pool-slot layout).  Per handle: ratio_threshold r,
 * distance_threshold t, mutual_check.  The rule:
 *   sim_ij = sum_k d0[i,k] d1[j,k], fp16 operands, fp32 accumulation; rows are NOT renormalised.
 *   For row i over j < n1:  j1 = the smallest j attaining the maximum, s1 = that maximum, s2 = max_{j != j1} sim_ij (a duplicate of the best
 *     gives s2 == s1; s2 is absent when n1 == 1);  e1 = 2 (1 - s1), e2 = 2 (1 - s2) in fp32 (the squared L2 distances of unit rows).
 *   pass_i = (r <= 0 or s2 absent or e1 <= (r r) e2) and (t <= 0 or e1 <= t t);   fwd_i = pass_i ? j1 : -1.
 *   bwd_j is the same rule on columns, over i < n0 (n0 == 1 is the absent case).
 *   matches0_i = fwd_i if fwd_i >= 0 and (!mutual_check or bwd[fwd_i] == i), else -1;  mscores0_i = s1 when matched, else 0.
 *   Rows >= n are -1 / 0.  A pair's result does not depend on the other pairs of the call.
 * This is hloc's find_nn + mutual_check (ratio and distance tests on 2 (1 - sim), the backward direction filtered before the mutual
 * check) with two stated differences: the score is the cosine itself and zero for unmatched rows, so that sship_filter_matches yields
 * distance = 1 - cosine, what the reference's cosineMatch writes (hloc reports (sim + 1) / 2 and does not zero it); and n1 == 1 passes
 * the ratio test (hloc's topk(2) raises there).
 * Defaults: r = 0 (off), t = 0 (off), mutual_check on = hloc's NN-mutual.  (r = 0.8: NN-ratio; t = 0.7: NN-superpoint.)
 * sship_nn_set_params: r <= 0 / t <= 0 turn that test off; NaN r, r > 1 or NaN t -> SSHIP_ERR_INVALID (the handle keeps its setting).
 * Bad arguments are refused before any device is touched.  Workspaces are sized once at create (max_keypoints 1..4096; max_pairs <= 0 -> 1).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_nn sship_nn;
int sship_nn_create(int max_keypoints, int max_pairs, sship_nn** out);
void sship_nn_destroy(sship_nn* nn);
int sship_nn_set_params(sship_nn* nn, float ratio_threshold, float distance_threshold, int mutual_check);
int sship_nn_get_params(const sship_nn* nn, float* ratio_threshold, float* distance_threshold, int* mutual_check); /* any output may be NULL */
/* Per-frame calls, synchronous on the handle's own stream, outputs on the host (matches0 [n0], mscores0 [n0]) - like
 * sship_lg_match_device / _match_host without keypoints.  n0 == 0 or n1 == 0, or n > max_keypoints -> SSHIP_ERR_INVALID. */
int sship_nn_match_device(sship_nn* nn, int n0, const void* desc0_dev, int n1, const void* desc1_dev, int32_t* matches0, float* mscores0);
int sship_nn_match_host(sship_nn* nn, int n0, const float* desc0_f32, int n1, const float* desc1_f32, int32_t* matches0, float* mscores0);
/* Throughput path: the layouts of sship_lg_match_batch_device without kp - n_dev [2*pairs], desc_dev [2*pairs, max_kp, 256] f16 (image 2p
 * is set 0, 2p+1 set 1 of pair p: what sship_sp_extract_batch_device writes), outputs [pairs, max_kp].  Asynchronous on `stream`, no host
 * synchronisation inside.  Counts are read on the device and clamped to [0, max_keypoints]; a pair with a zero count is all -1 / 0.
 * Rows >= n of desc_dev are never used, whatever they hold (NaN, Inf), and every entry of the outputs is written. */
int sship_nn_match_batch_device(sship_nn* nn, const int* n_dev, const void* desc_dev, int pairs, int32_t* matches0_dev, float* mscores0_dev,
                                void* stream);
/* Measurement hook: re-run the launches of the last match call on this handle `iters` times (over the same buffers, which the caller of a
 * batch call keeps alive), timed with hipEvents on the handle's stream; *avg_ms = mean duration of one call's launches. */
int sship_nn_bench(sship_nn* nn, int iters, float* avg_ms);
/* Keypoint-window gate - per handle, off by default.  The matcher above reads descriptors only: every row of set 0 competes against every
 * row of set 1.  For rectified stereo (the partner lies in the epipolar band, src/StereoFrontEnd.cc:35-47 rejects the others AFTER matching)
 * and for frame-to-frame tracking (a square window around the previous position) the search space is restricted BEFORE the best and the
 * second best are chosen.  Gate g = (dx_lo, dx_hi, dy_lo, dy_hi); keypoints (x, y) in whatever pixel unit the caller uses.  The rule:
 *   For row i of set 0 and row j of set 1:  dx = x0_i - x1_j and dy = y0_i - y1_j, one fp32 subtraction each;
 *   in_ij = dx >= dx_lo && dx <= dx_hi && dy >= dy_lo && dy <= dy_hi, exactly this form: a NaN coordinate is in no window.
 *   An entry with !in_ij is absent, exactly like an index outside n0 x n1.  Everything else is the rule above over the PRESENT entries of
 *   a row or column: j1 = the smallest present index of the maximum, s2 = the maximum over the other present entries; s2 is absent when
 *   fewer than two entries are present (the generalisation of n1 == 1: the ratio test passes); a row with no present entry gives fwd_i = -1;
 *   columns follow the same rule; the mutual check and the scores are unchanged.
 *   Bounds may be +-INFINITY: the gate (-inf, inf, -inf, inf) with finite coordinates gives the ungated result bit for bit.
 *   Stereo use: (min_disparity, max_disparity, -row, +row).  A tracking window: (-r, r, -r, r).
 *   Swapping the sets with the gate (-dx_hi, -dx_lo, -dy_hi, -dy_lo) gives the inverse map under the mutual check.
 * sship_nn_set_gate: a NaN bound, lo > hi or a NULL handle -> SSHIP_ERR_INVALID (the handle keeps its setting); refused before any device is
 * touched.  sship_nn_get_gate: any output may be NULL.
 * The _gated entry points are the three above plus keypoints, and the handle's gate applies: the per-frame calls take HOST keypoints as
 * (kp, kp_stride) with 2 or 3 floats per keypoint, like sship_lg_match_device; the batch call takes kp_dev [2*pairs, max_kp, 3] f32 (x, y,
 * score), the layout sship_sp_extract_batch_device writes and sship_lg_match_batch_device reads.  Keypoint rows >= n are never used, whatever
 * they hold.  With the gate disabled they return the bits of the plain calls, and kp may be NULL.  On a handle whose gate is enabled the
 * PLAIN entry points return SSHIP_ERR_INVALID (a silent ungated match would be the worst outcome); on a handle without a gate they make
 * exactly the launches they made before the gate existed.  sship_nn_bench replays the gated launches after a gated call. */
int sship_nn_set_gate(sship_nn* nn, int enabled, float dx_lo, float dx_hi, float dy_lo, float dy_hi);
int sship_nn_get_gate(const sship_nn* nn, int* enabled, float* dx_lo, float* dx_hi, float* dy_lo, float* dy_hi);
int sship_nn_match_gated_device(sship_nn* nn, const float* kp0, int kp0_stride, int n0, const void* desc0_dev, const float* kp1, int kp1_stride,
                                int n1, const void* desc1_dev, int32_t* matches0, float* mscores0);
int sship_nn_match_gated_host(sship_nn* nn, const float* kp0, int kp0_stride, int n0, const float* desc0_f32, const float* kp1, int kp1_stride,
                              int n1, const float* desc1_f32, int32_t* matches0, float* mscores0);
int sship_nn_match_gated_batch_device(sship_nn* nn, const int* n_dev, const void* desc_dev, const float* kp_dev, int pairs,
                                      int32_t* matches0_dev, float* mscores0_dev, void* stream);
/* Stereo association - src/StereoFrontEnd.cc:35-47 as a device stage, on the output of either matcher: turns matches0 into the right
 * image's u coordinate (the disparity's other half) without going through the host.  kp_dev [2*pairs, max_kp, 3], n_dev [2*pairs]
 * (clamped to [0, max_keypoints] on the device), matches0_dev [pairs, max_kp].  For pair p and left keypoint i < n0, j = matches0[p, i]:
 *   has_depth = 0 <= j < n1 && (uL - uR >= min_disparity) && (|vL - vR| <= max_row_diff), in fp32, in this positive form: NaN gives no
 *   depth - the one stated difference from the reference's `continue` form, which lets NaN through.
 *   stereo_dev [pairs, max_kp, 3] f32 = (uL, has_depth ? uR : quiet NaN, vL);  has_depth_dev [pairs, max_kp] u8.
 *   Rows >= n0 are (0, NaN, 0) / 0, and every entry is written.
 * Asynchronous on `stream`, one launch.  The reference's defaults are min_disparity = 1, max_row_diff = 2. */
int sship_stereo_associate_batch_device(const float* kp_dev, const int* n_dev, const int32_t* matches0_dev, int pairs, int max_keypoints,
                                        float min_disparity, float max_row_diff, float* stereo_dev, uint8_t* has_depth_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * EigenPlaces place recogniser - include/EigenPlaces.h:19-40, src/EigenPlaces.cc
 * ResNet-18 trunk + L2Norm / GeM / Linear(512, 512) / L2Norm (utils/convert_eigenplaces_to_onnx.py:54-60), used once per
 * keyframe by the loop-closure thread.  weights_path: safetensors of the hub model's state_dict (keys backbone.*,
 * aggregation.*, what utils/convert_eigenplaces_to_onnx.py:99 saves) - it takes the place of the .engine file.
 * sship_ep_infer is the device half of EigenPlaces::compute_global_descriptor (src/EigenPlaces.cc:147-174): the caller hands
 * the HOST-preprocessed fp32 [3, input_h, input_w] tensor (src/EigenPlaces.cc:123-145 runs on the host in the reference too;
 * include/superslam_hip/place_recognizer.hpp restates it) and receives the L2-normalised 512-d descriptor.  Synchronous.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_ep sship_ep;
int sship_ep_create(const char* weights_path, int input_w, int input_h, sship_ep** out);
void sship_ep_destroy(sship_ep* ep);
int sship_ep_descriptor_dim(const sship_ep* ep);
int sship_ep_infer(sship_ep* ep, const float* chw_host, float* desc_out);
/* EigenPlaces::compute_global_descriptor for the image itself (src/EigenPlaces.cc:147-174 including :123-145): u8 image, 1 channel or
 * 3 = BGR, row stride in bytes, any size.  The image is uploaded as u8 and preprocessed ON THE DEVICE (fixed-point 8-bit bilinear resize to
 * input_w x input_h, x 1/255, ImageNet mean / std: bit-identical to sship_ep_preprocess), then the network runs as in sship_ep_infer -
 * the descriptor equals sship_ep_infer(sship_ep_preprocess(img)) bit for bit.
 *   sship_ep_infer_u8         host image, host descriptor; synchronous (returns after the handle's stream has drained);
 *   sship_ep_infer_u8_device  device image, device descriptor [512] f32, asynchronous on `stream` (NULL = legacy default stream).  One
 *                             call in flight per handle (the activations live in the handle: calls of one handle must be ordered, on one
 *                             stream or by events).  The FIRST call with a new source size (h, w) allocates and uploads that size's resize
 *                             tables (hipMalloc + a blocking copy; not legal under stream capture - warm each size up first); the tables
 *                             are immutable afterwards, so later calls are purely asynchronous.  The descriptor's bits do not depend on
 *                             the device's CU count or partition mode (the split-K factors are functions of the layer shapes only). */
int sship_ep_infer_u8(sship_ep* ep, const uint8_t* img, int h, int w, int stride, int channels, float* desc_out);
int sship_ep_infer_u8_device(sship_ep* ep, const uint8_t* img_dev, int h, int w, int stride, int channels, float* desc_out_dev, void* stream);
/* Measurement hook: `iters` back-to-back sship_ep_infer_u8_device calls on the handle's stream over a resident image; average ms. */
int sship_ep_bench(sship_ep* ep, const uint8_t* img_dev, int h, int w, int stride, int channels, int iters, float* avg_ms);
/* Test-only: per-stage capture of the network's activations.  The block activations live in four ping-pong buffers and are overwritten, so
 * nothing can be read back after a call unless it was copied aside while the call ran.  Used by the parity suite to compare every layer with
 * an fp64 convolution of the stage it read (tests/test_gpu_ep_layers.py); the product never calls it.
 * sship_ep_debug_capture(ep, on): off is the default and costs nothing (no allocation, no launch, no kernel knows about it).  Switched on,
 *   the per-stage buffers are allocated (once per handle) and every later call of the handle enqueues, on the call's own stream and right
 *   after the launch that produces it, a device-to-device copy of every stage's output; the descriptor's bits are unchanged.  Switching
 *   forgets what was captured.
 * sship_ep_debug_activation(ep, stage, out_host, bytes): copies one stage of the LAST call to the host, raw, device-synchronising.
 *   SSHIP_ERR_INVALID for a stage that does not exist, for bytes larger than the stage, and while capture is off or no call has run since it
 *   was switched on.
 * Stages (H x W the engine size; h1 = ceil(H / 4) by the chain h -> (h - 1) / 2 + 1 twice, h2 = ceil(h1 / 2), h3 = ceil(h2 / 2),
 * h4 = ceil(h3 / 2), likewise w; fp16 maps are channels-last [h][w][c]):
 *    0        the preprocessed input, fp32 [3][H][W]
 *    1        stem 7x7 / 2 + BatchNorm + ReLU + MaxPool2d(3, 2, 1), fp16 [h1][w1][64]
 *    2 + 3 b  block b's conv1 + bn1 + ReLU               (b = 0 .. 7: layer1.0, layer1.1, layer2.0, ... layer4.1)
 *    3 + 3 b  block b's downsample conv 1x1 + BatchNorm   (exists for b = 2, 4, 6 only: the first block of layer2 / 3 / 4)
 *    4 + 3 b  block b's output, ReLU(conv2 + bn2 + identity or downsample)
 *             all fp16, [h1][w1][64] for b = 0, 1; [h2][w2][128] for b = 2, 3; [h3][w3][256] for b = 4, 5; [h4][w4][512] for b = 6, 7
 *   26        the tail's partial sums of clamp(x / ||x||, 1e-6)^p over the locations, fp32 [G][512], G = min(32, ceil(h4 w4 / 8))
 *             workgroups (the GeM mean is their sum in ascending order, divided by h4 w4)
 *   27        the 512 outputs of the Linear, before the final L2 normalisation, fp32
 *   28        the descriptor, fp32 [512] */
int sship_ep_debug_capture(sship_ep* ep, int on);
int sship_ep_debug_activation(sship_ep* ep, int stage, void* out_host, unsigned long long bytes);
/* EigenPlaces: batches.  THE RULE: descriptor b of a batch call has exactly the bits sship_ep_infer_u8_device gives for image b alone - for
 * every batch size, at every position in the batch, on any stream, from the host or the device entry - and so has every captured stage.
 * The batch path keeps every rounding point of the single-image path, its fp32 summation orders (the split-K grouping of the deep layers, the
 * tail's partial sums per workgroup and per wave) and the non-contracted preprocessing; what changes with the batch is only how many images a
 * launch covers and whether a deep layer's group sums meet in a workspace (batched split-K) or in registers (the grouped kernel), chosen
 * from (layer shape, batch) alone - never from the device.
 * sship_ep_reserve_batch(ep, max_batch): max_batch in 1..1024, else SSHIP_ERR_INVALID.  Allocates the activations, the preprocessed input,
 *   the tail workspace and the split-K workspace for max_batch images (about 44 x input_w x input_h bytes per image: 11.5 MB at 512 x 512).
 *   Synchronises the device first; not legal under stream capture.  Never shrinks: a value <= sship_ep_max_batch is a no-op returning
 *   SSHIP_OK.  When an allocation fails (SSHIP_ERR_NOMEM) the handle keeps what it had and still works.
 * sship_ep_max_batch(ep): 1 after create, otherwise the reserved maximum; NULL -> 0.
 * sship_ep_batch_workspace_bytes(input_w, input_h, batch): pure host, no GPU.  The smallest byte count that holds
 *   ksplit x batch x output pixels x cout fp32 for every convolution that runs as batched split-K at this batch; 0 when none does; 0 on bad
 *   arguments (an engine below 32 x 32, batch outside 1..1024).
 * sship_ep_infer_u8_batch_device: image b starts at imgs_dev + b * image_stride BYTES; stride >= w * channels, image_stride >= h * stride, no
 *   alignment asked of either (image_stride = 2 * h * stride reads the left images of an interleaved L0, R0, L1, R1, ... buffer).  All images
 *   share one size and one channel count.  Row b of the output starts at desc_out_dev + b * desc_stride floats, desc_stride >= 512 - the
 *   layout sship_index_add_device and sship_index_query_batch_device take.  Asynchronous on `stream`; one call in flight per handle; the first
 *   call with a new source size uploads that size's tables exactly as the single-image entry does.  SSHIP_ERR_INVALID before any device is
 *   touched, the handle unchanged: batch outside 1..sship_ep_max_batch (a call never grows the reservation: no hidden allocation), a NULL
 *   pointer, bad image arguments, a stride below its minimum.
 * sship_ep_infer_u8_batch: the same from host images to host descriptors [batch][512]; synchronous (upload, the device entry, download) -
 *   the drop-in for a loop of sship_ep_infer_u8.
 * sship_ep_bench_batch: measurement hook, `iters` back-to-back batch calls on the handle's stream; *avg_ms = mean duration of ONE batch call.
 * sship_ep_debug_capture_image(ep, image): test-only, default 0: which image (0..1023) of later BATCH calls sship_ep_debug_capture copies
 *   aside; stage numbering and sizes unchanged, per image.  A batch call with batch <= image captures nothing and _debug_activation then
 *   returns SSHIP_ERR_INVALID.  Capture off still makes no call and no allocation. */
int sship_ep_reserve_batch(sship_ep* ep, int max_batch);
int sship_ep_max_batch(const sship_ep* ep);
size_t sship_ep_batch_workspace_bytes(int input_w, int input_h, int batch);
int sship_ep_infer_u8_batch_device(sship_ep* ep, const uint8_t* imgs_dev, int batch, int h, int w, int stride, long long image_stride,
                                   int channels, float* desc_out_dev, int desc_stride, void* stream);
int sship_ep_infer_u8_batch(sship_ep* ep, const uint8_t* imgs, int batch, int h, int w, int stride, long long image_stride, int channels,
                            float* desc_out);
int sship_ep_bench_batch(sship_ep* ep, const uint8_t* imgs_dev, int batch, int h, int w, int stride, long long image_stride, int channels,
                         int iters, float* avg_ms);
int sship_ep_debug_capture_image(sship_ep* ep, int image);
/* EigenPlaces::preprocess (src/EigenPlaces.cc:123-145) on the host, no GPU: u8 image (1 channel or 3 = BGR, row stride in bytes) ->
 * fp32 [3, input_h, input_w]: GRAY2RGB / BGR2RGB, cv::resize INTER_LINEAR (OpenCV's 8-bit fixed-point path), x 1/255,
 * ImageNet mean / std.  Exported so that every binding shares one implementation. */
int sship_ep_preprocess(const uint8_t* img, int h, int w, int stride, int channels, int input_w, int input_h, float* chw_out);

/* ------------------------------------------------------------------------------------------------
 * Place-recognition index - the reference's CosineDescriptorIndex (include/PlaceRecognizer.h, src/PlaceRecognizer.cc:21-52: add,
 * exclude-recent window, score gate, top-k) with the database resident on the device, so that the descriptor sship_ep_infer_u8_device
 * leaves in device memory is stored and searched without a host copy; and, with many queries per call, hloc's "pairs from retrieval"
 * over a whole sequence.  Any global descriptor: dim is a multiple of 4 in [4, 4096] (EigenPlaces: 512).  The rule:
 *   Stored row (normalizedRow, PlaceRecognizer.cc:10-18): n = sqrt(sum_k x_k x_k) accumulated in fp64; row_k = (float)((double)x_k / n) if
 *     n > 1e-12, else the row is stored unchanged - a NaN norm fails that comparison, so such a row stays as given.  Queries are
 *     normalised by the same rule inside the query call.
 *   Score: s_i = sum_k row_i[k] q[k], fp32 operands, fp32 accumulation; the database is never narrowed to fp16 / bf16.  A score's bits depend
 *     only on the row, the query and dim - not on the index size, the number of queries in the call, the query's position in the batch or
 *     the device's CU count: one query gives the same bits alone (_query_host / _query_device) and inside any batch.
 *   Candidates of query j: rows i < limit_j with s_i >= min_score, exactly this form: a NaN score is never a candidate, also with
 *     min_score = -INFINITY.  limit_j = size - exclude_recent (exclude_recent >= size: no candidates), or limits_dev[j] clamped to
 *     [0, size] when limits_dev is given (exclude_recent is then not used) - what a batch of consecutive keyframes or an all-against-all
 *     run needs.  Insertion order is recency.
 *   Order: descending score, ties by ascending row (the stable sort of oracle/eigenplaces_ref.py; the reference's std::sort leaves ties
 *     unspecified).  Output: the first min(top_k, #candidates) entries and that number as the count.  In the batch outputs entries at and
 *     beyond the count are -1 / 0.0f, and every entry is written.
 *   Stated difference from the reference: topK <= 0 means "all" there; here top_k must be in 1..max_top_k.
 * Handle: sship_index_create(dim, capacity, max_queries 1..1024, max_top_k 1..128); capacity >= 1 and capacity * dim * 4 <= 2 GiB.  All
 * storage and workspaces are allocated once at create: the fp32 database [capacity, dim], the normalised queries, and
 * ceil(capacity / 256) * max_queries * max_top_k 8-byte partial keys (one list per 256-row chunk and query).
 * Bad arguments are refused with SSHIP_ERR_INVALID before any device is touched, the handle unchanged: a bad create argument, a NULL
 * handle or pointer, count < 1, a stride below dim, an add beyond capacity, num_queries outside 1..max_queries, top_k outside
 * 1..max_top_k, exclude_recent < 0, a NaN min_score.  Valid create arguments without a GPU give SSHIP_ERR_NO_DEVICE.
 * State and ordering: keyframe ids (int64) and the size are HOST state, updated when an add is enqueued; device work is stream-ordered.
 * A handle is not thread-safe, and its calls must be ordered on one stream or by events (as for sship_ep_infer_u8_device): _add_device and
 * _query_batch_device run on `stream` (NULL = the legacy default stream); _add_host, _query_host and _query_device run on the handle's
 * own blocking stream and return after synchronising it; _read synchronises the device.  Device outputs of the batch call are ROW indices
 * (insertion positions); the per-query calls map them to ids.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_index sship_index;
int sship_index_create(int dim, int capacity, int max_queries, int max_top_k, sship_index** out);
void sship_index_destroy(sship_index* index);
int sship_index_dim(const sship_index* index);        /* NULL -> 0 */
int sship_index_capacity(const sship_index* index);   /* NULL -> 0 */
int sship_index_size(const sship_index* index);       /* NULL -> 0 */
int sship_index_clear(sship_index* index);            /* size = 0; the storage is kept */
/* Append `count` rows (row r at desc + r * row_stride floats, row_stride >= dim, no alignment needed) with their ids (host). */
int sship_index_add_host(sship_index* index, const int64_t* ids, const float* desc_f32, int count, int row_stride);
int sship_index_add_device(sship_index* index, const int64_t* ids, const float* desc_dev, int count, int row_stride, void* stream);
/* Stored rows [first_row, first_row + count) as they are on the device, and their ids; either output may be NULL. */
int sship_index_read(sship_index* index, int first_row, int count, float* rows_out, int64_t* ids_out);
/* One query, results on the host: ids_out / scores_out [top_k], *count_out entries are valid. */
int sship_index_query_host(sship_index* index, const float* desc_f32, int exclude_recent, int top_k, float min_score, int64_t* ids_out,
                           float* scores_out, int* count_out);
int sship_index_query_device(sship_index* index, const float* desc_dev, int exclude_recent, int top_k, float min_score, int64_t* ids_out,
                             float* scores_out, int* count_out);
/* num_queries queries (row j at q_dev + j * q_stride floats), everything device-resident and asynchronous on `stream`:
 * rows_dev i32 [num_queries, top_k], scores_dev f32 [num_queries, top_k], counts_dev i32 [num_queries].  limits_dev i32 [num_queries] or NULL. */
int sship_index_query_batch_device(sship_index* index, const float* q_dev, int num_queries, int q_stride, const int32_t* limits_dev,
                                   int exclude_recent, int top_k, float min_score, int32_t* rows_dev, float* scores_dev, int32_t* counts_dev,
                                   void* stream);
/* Measurement hook: re-run the launches of the last query call on this handle `iters` times (over the same buffers and the size of that
 * call, which the caller of a batch call keeps alive), timed with hipEvents on the handle's stream; *avg_ms = mean duration of one call. */
int sship_index_bench(sship_index* index, int iters, float* avg_ms);

/* ------------------------------------------------------------------------------------------------
 * Pose-only stereo solver - what both consumers of the front-end's output do with it: src/VoEstimator.cc:249-270 (FrameTracker::track on
 * PointObs {Xw, meas}) and src/LoopCloser.cc:55-89 (the same solve from identity, then an inlier count).  One 6x6 system per pair, `pairs`
 * pairs per call, device-resident, no GTSAM.  The objective is FrameTracker's (PoseOnlyStereoFactor under a Huber-robust diagonal noise,
 * include/PoseOptimizationFactors.h); the Levenberg-Marquardt schedule is this library's own and is stated here - the rule is NOT
 * "whatever GTSAM does".  Inputs are fp32 and are widened on load; all arithmetic is fp64.  The rule:
 *   Camera (fx, fy, cx, cy, baseline), no skew.  Pose Twc = [R | t], row-major 3x4, 12 doubles (superslam_hip::Pose3x4).
 *   Observation k = (X, (uL, uR, v), valid).  It is PRESENT iff its valid byte is non-zero and all six floats are finite; an absent
 *     observation contributes nothing, whatever it holds.
 *   q = R^T (X - t).  projection = (fx q.x / q.z + cx, fx (q.x - baseline) / q.z + cx, fy q.y / q.z + cy);  r = projection - (uL, uR, v).
 *   Whitened r~ = (r0 / sigma_px, r1 / sigma_uR, r2 / sigma_px) with sigma_uR = sigma_d0 sqrt(1 + (d_cond / d)^2), d = max(uL - uR, 1e-3)
 *     of the measurement, d_cond = fx baseline / cond_depth (stereo_diag_noise).
 *   Behind the camera, !(q.z > 0) in exactly this form: r = (2 fx, 2 fx, 2 fx) and the Jacobian is zero (the reference's cheirality branch).
 *   Huber on e = |r~| with k^2 = huber_k2: rho = e^2 / 2 for e <= k, k e - k^2 / 2 above;  IRLS weight w = min(1, k / e).
 *   Jacobian J~ = d r~ / d xi for the right perturbation T Exp(xi), xi = (omega, v), rotation first: dq/d omega = [q]x, dq/dv = -I.
 *   H = sum w J~^T J~,  g = sum w J~^T r~,  c = sum rho  over the present observations.
 *   Schedule:  (c, H, g) at T0, lambda = lambda0.  Repeat: if trials == max_iterations stop with ITER_CAP.  Solve (H + lambda I) delta = -g
 *     by Cholesky; a pivot that is not > 0 is a rejected trial (counted, nothing evaluated).  T' = T Exp(delta), the full SE(3) exponential
 *     (R' = R Exp(omega), t' = t + R V(omega) v; no re-orthonormalisation); (c', H', g') at T' in one pass; one trial.  Then, in this order:
 *     c' finite and |c - c'| <= max(abs_tol, rel_tol c): take T', CONVERGED, stop;  else c' < c: accept, lambda /= 10;  else reject,
 *     lambda *= 10, and lambda > lambda_max stops with STALLED at T.
 *   Fewer than 3 present observations: TOO_FEW.  A non-finite initial pose: BAD_INPUT.  In both the pose out is the pose in, and
 *     n_inliers, trials and both costs are 0.
 *   n_inliers (LoopCloser.cc:74-86): the present observations with q.z > 0 and hypot(r0, r2) < inlier_px at the final pose.
 *   Defaults (the reference's): sigma_px 10, sigma_d0 8, cond_depth 40, huber_k2 7.815, inlier_px 3 (LoopParams); the schedule's own:
 *     lambda0 1e-5, lambda_max 1e5, abs_tol = rel_tol = 1e-5, max_iterations 100.
 *   Sums run in one fixed order (per thread over its observations k = tid, tid + 256, ..., then lanes, then waves): a pair gives the same
 *     bits alone, inside any batch and at any batch position.
 * Handle: sship_pose_create(max_obs 1..2048, max_pairs 1..65535).  The camera must be set before a solve or a gather.
 * Bad arguments are refused with SSHIP_ERR_INVALID and a message before any device is touched, the handle unchanged: a NULL handle or
 * pointer, max_obs / max_pairs / pairs / n_obs out of range, fx, fy or baseline not > 0 (or any camera value not finite), a NaN in the
 * params, a sigma, cond_depth, huber_k2 or lambda0 not > 0, lambda_max < lambda0, a negative tolerance or inlier_px, max_iterations < 1.
 * Valid create arguments without a GPU give SSHIP_ERR_NO_DEVICE.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_pose sship_pose;
typedef struct sship_pose_params {
  double sigma_px, sigma_d0, cond_depth, huber_k2;
  double lambda0, lambda_max, abs_tol, rel_tol;
  double inlier_px;
  int max_iterations;
} sship_pose_params;
#define SSHIP_POSE_CONVERGED 0
#define SSHIP_POSE_ITER_CAP 1
#define SSHIP_POSE_STALLED 2
#define SSHIP_POSE_TOO_FEW 3
#define SSHIP_POSE_BAD_INPUT 4
int sship_pose_create(int max_obs, int max_pairs, sship_pose** out);
void sship_pose_destroy(sship_pose* ps);
int sship_pose_set_camera(sship_pose* ps, double fx, double fy, double cx, double cy, double baseline);
int sship_pose_get_camera(const sship_pose* ps, double* fx, double* fy, double* cx, double* cy, double* baseline); /* any output may be NULL */
int sship_pose_set_params(sship_pose* ps, const sship_pose_params* params);
int sship_pose_get_params(const sship_pose* ps, sship_pose_params* params);
/* Throughput path, one launch, asynchronous on `stream` (NULL = the legacy default stream), no host synchronisation inside:
 * points_dev [pairs, max_obs, 3] f32 (X in the frame the pose maps into), meas_dev [pairs, max_obs, 3] f32 (uL, uR, v),
 * valid_dev [pairs, max_obs] u8, pose0_dev [pairs, 12] f64 or NULL = identity;  pose_dev [pairs, 12] f64, stats_dev [pairs, 4] i32 =
 * (n_obs, n_inliers, trials, status), cost_dev [pairs, 2] f64 = (initial, final), inlier_dev [pairs, max_obs] u8 or NULL.  Every entry
 * of the outputs is written. */
int sship_pose_solve_batch_device(sship_pose* ps, const float* points_dev, const float* meas_dev, const uint8_t* valid_dev,
                                  const double* pose0_dev, int pairs, double* pose_dev, int32_t* stats_dev, double* cost_dev,
                                  uint8_t* inlier_dev, void* stream);
/* One pair from host arrays - the drop-in for one FrameTracker::track call: points / meas [n_obs, 3], valid [n_obs] or NULL = all,
 * pose0 [12] or NULL = identity; pose_out [12], stats_out [4], cost_out [2], inlier_out [n_obs] or NULL.  n_obs in 0..max_obs.
 * Synchronous on the handle's own stream; the same launch as the batch call with pairs = 1, hence the same bits. */
int sship_pose_solve_host(sship_pose* ps, const float* points, const float* meas, const uint8_t* valid, int n_obs, const double* pose0,
                          double* pose_out, int32_t* stats_out, double* cost_out, uint8_t* inlier_out);
/* The observation list from what the front-end leaves on the device (LoopCloser.cc:55-70), one launch, asynchronous on `stream`:
 * stereo0_dev / has_depth0_dev [pairs, max_obs, 3] / [pairs, max_obs] of the keyframe and stereo1_dev / has_depth1_dev of the frame (the
 * outputs of sship_stereo_associate_batch_device), matches0_dev [pairs, max_obs] from keyframe-left to frame-left keypoints, and the two
 * left-image counts of pair p at n0_dev[p * n_stride] and n1_dev[p * n_stride] (n_stride = 2 reads them out of an extractor's [2 * pairs]
 * array), clamped to [0, max_obs] on the device.  For keyframe keypoint i < n0 with j = matches0[p, i]:
 *   valid = 0 <= j < n1 && has_depth0[p, i] && has_depth1[p, j];
 *   X = backproject_cam(stereo0[p, i]) (LoopCloser.cc:19-24) in the keyframe's camera frame, in fp64 from the fp32 values and rounded
 *   once to fp32: Z = fx baseline / (uL - uR), X = (uL - cx) Z / fx, Y = (v - cy) Z / fy;   meas = stereo1[p, j].
 *   An invalid row, and every row >= n0, is (0, 0, 0) / (0, 0, 0) / 0.  Every entry is written. */
int sship_pose_obs_from_matches_batch_device(const sship_pose* ps, const float* stereo0_dev, const uint8_t* has_depth0_dev,
                                             const float* stereo1_dev, const uint8_t* has_depth1_dev, const int32_t* matches0_dev,
                                             const int* n0_dev, const int* n1_dev, int n_stride, int pairs, float* points_dev,
                                             float* meas_dev, uint8_t* valid_dev, void* stream);
/* Measurement hook: re-run the last solve call's launch on this handle `iters` times (over the same buffers, which the caller of a batch
 * call keeps alive), timed with hipEvents on the handle's stream; *avg_ms = mean duration of one launch. */
int sship_pose_bench(sship_pose* ps, int iters, float* avg_ms);

/* ------------------------------------------------------------------------------------------------
 * RANSAC pose seed and inlier gate - the hypothesise-and-verify stage between "matches" and "solve": the pose and the inlier set of
 * `pairs` pairs per call when the seed is unknown and many matches are wrong (a loop partner metres and tens of degrees away, which
 * src/LoopCloser.cc:72 hands to the local solve from the identity; the observations of sship_nn_*).  Device-resident, no early exit, no
 * adaptive count.  The reference has no such stage; the rule is this library's own and is stated here in full.  Camera, observation layout
 * and pose are the pose-only solver's: (fx, fy, cx, cy, baseline), observation k = (X, (uL, uR, v), valid), pose Twc = [R | t] row-major
 * 3x4 with X = R Y + t for a point Y in the frame's camera.  Inputs are fp32 and are widened on load; all arithmetic is fp64, every
 * product, quotient, square root and sum rounded once, in the order written below (no fused multiply-add).  The rule:
 *   PRESENT as in sship_pose_*: the valid byte is non-zero and all six floats are finite.  SAMPLEABLE: present and the measured disparity
 *     d = uL - uR >= min_disparity.  m = the number of sampleable observations; rank r is the r-th of them in ascending row order.
 *   Y_k, the measurement back-projected in the frame's camera, with the formula of sship_pose_obs_from_matches_batch_device but kept in
 *     fp64: Z = fx baseline / (uL - uR), Y_k = ((uL - cx) Z / fx, (v - cy) Z / fy, Z).
 *   Sampling is counter-based, on 32-bit unsigned values (all arithmetic mod 2^32):
 *     mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *     u(h, j) = mix(mix(seed + 0x9e3779b9 * (3 h + j + 1))).
 *     a = u(h, 0) % m;  b = u(h, 1) % (m - 1), b += (b >= a);  c = u(h, 2) % (m - 2), c += (c >= min(a, b)), then c += (c >= max(a, b)).
 *     Three distinct ranks, a function of (seed, h, m) only - never of the pair's position in the batch.
 *   Hypothesis h, from the observations of ranks (a, b, c) as (p0, p1, p2), once with p = X and once with p = Y:
 *     d1 = p1 - p0, d2 = p2 - p0, n = d1 x d2, e1 = d1 / |d1|, e3 = n / |n|, e2 = e3 x e1;  |v|^2 = (v.x^2 + v.y^2) + v.z^2.
 *     R = [e1 e2 e3]_X [e1 e2 e3]_Y^T, entry (i, j) = (e1X_i e1Y_j + e2X_i e2Y_j) + e3X_i e3Y_j.
 *     t = mean(X) - R mean(Y), mean = ((p0 + p1) + p2) / 3, (R v)_i = (R_i0 v_0 + R_i1 v_1) + R_i2 v_2.
 *     REJECTED (cost +Inf) unless |n|^2 > min_area2 for both triads and every entry of R and t is finite.
 *   Score (MSAC) of a hypothesis that is not rejected: one running fp64 sum, from 0, over the PRESENT observations in ascending row order.
 *     q = R^T (X - t), q_j = (R_0j d_0 + R_1j d_1) + R_2j d_2 with d = X - t.  thr2 = inlier_px^2.
 *     !(q.z > 0): the term is thr2.  Otherwise r0 = (fx q.x) (1 / q.z) + cx - uL, r2 = (fy q.y) (1 / q.z) + cy - v, e2 = r0^2 + r2^2, and the
 *     term is e2 if e2 < thr2, else thr2.  uR does not enter the score (as n_inliers of sship_pose_*, LoopCloser.cc:74-86).
 *   Winner: the lowest cost; the lower h wins a tie.  pose = the winner's (R, t); the inlier mask and n_inliers are the present
 *     observations with q.z > 0 && e2 < thr2 at the winner; stats = (n_present, n_inliers, best_h, status); cost = the winner's cost.
 *   Statuses: OK;  TOO_FEW when m < 3;  NO_MODEL when every hypothesis is rejected.  In the last two the pose is the identity, the mask is
 *     zero, n_inliers is 0, best_h is -1 and the cost is +Inf; n_present is still counted.
 *   Exactly num_hypotheses hypotheses, h = 0 .. num_hypotheses - 1, are evaluated.
 *   Defaults: inlier_px 3 (the reference's LoopParams); min_disparity 1, min_area2 1e-8 m^4, seed 1 and num_hypotheses 512 are this
 *     library's own choices.
 *   A hypothesis's cost depends on nothing but (the pair's observations, the camera, the parameters, h): a pair gives the same bits alone,
 *     at any position of any batch, and however the hypotheses are spread over workgroups; a winner below the smaller of two
 *     num_hypotheses that both keep it is the same for both.
 * Handle: sship_ransac_create(max_obs 1..2048, max_pairs 1..65535).  The camera must be set before a solve.
 * Bad arguments are refused with SSHIP_ERR_INVALID and a message before any device is touched, the handle unchanged: a NULL handle or
 * pointer, max_obs / max_pairs / pairs / n_obs out of range, fx, fy or baseline not > 0 (or any camera value not finite), a NaN or an
 * infinity in the params, a negative inlier_px, min_disparity or min_area2, num_hypotheses outside 1..65536.
 * Valid create arguments without a GPU give SSHIP_ERR_NO_DEVICE.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_ransac sship_ransac;
typedef struct sship_ransac_params {
  double inlier_px, min_disparity, min_area2;
  uint32_t seed;
  int num_hypotheses;
} sship_ransac_params;
#define SSHIP_RANSAC_OK 0
#define SSHIP_RANSAC_TOO_FEW 1
#define SSHIP_RANSAC_NO_MODEL 2
int sship_ransac_create(int max_obs, int max_pairs, sship_ransac** out);
void sship_ransac_destroy(sship_ransac* rs);
int sship_ransac_set_camera(sship_ransac* rs, double fx, double fy, double cx, double cy, double baseline);
int sship_ransac_get_camera(const sship_ransac* rs, double* fx, double* fy, double* cx, double* cy, double* baseline); /* any output may be NULL */
int sship_ransac_set_params(sship_ransac* rs, const sship_ransac_params* params);   /* may grow the handle's workspace: not during a solve */
int sship_ransac_get_params(const sship_ransac* rs, sship_ransac_params* params);
/* Throughput path, two launches (score, then argmin and mask), asynchronous on `stream` (NULL = the legacy default stream), no host
 * synchronisation inside: points_dev / meas_dev [pairs, max_obs, 3] f32 and valid_dev [pairs, max_obs] u8 as sship_pose_solve_batch_device
 * takes them;  pose_dev [pairs, 12] f64 and inlier_dev [pairs, max_obs] u8 (or NULL) in exactly the layouts that call takes as pose0_dev
 * and valid_dev, so the two chain without a kernel in between;  stats_dev [pairs, 4] i32 = (n_present, n_inliers, best_h, status),
 * cost_dev [pairs] f64.  Every entry of the outputs is written.  The handle's workspace carries the partial results between the two
 * launches: calls on one handle must be ordered on one stream. */
int sship_ransac_solve_batch_device(sship_ransac* rs, const float* points_dev, const float* meas_dev, const uint8_t* valid_dev, int pairs,
                                    double* pose_dev, int32_t* stats_dev, double* cost_dev, uint8_t* inlier_dev, void* stream);
/* One pair from host arrays: points / meas [n_obs, 3], valid [n_obs] or NULL = all; pose_out [12], stats_out [4], cost_out [1],
 * inlier_out [n_obs] or NULL.  n_obs in 0..max_obs.  Synchronous on the handle's own stream; the same launches as the batch call with
 * pairs = 1, hence the same bits. */
int sship_ransac_solve_host(sship_ransac* rs, const float* points, const float* meas, const uint8_t* valid, int n_obs, double* pose_out,
                            int32_t* stats_out, double* cost_out, uint8_t* inlier_out);
/* Measurement hook: re-run the last solve call's launches on this handle `iters` times (over the same buffers, which the caller of a batch
 * call keeps alive), timed with hipEvents on the handle's stream; *avg_ms = mean duration of one call's two launches. */
int sship_ransac_bench(sship_ransac* rs, int iters, float* avg_ms);

/* ------------------------------------------------------------------------------------------------
 * Window smoother - sliding-window stereo bundle adjustment: what VoEstimator::track does at every keyframe with smoother_.optimize()
 * (src/VoEstimator.cc:316-323, src/WindowSmoother.cc): a fixed-lag window of the last keyframe poses re-optimised against all stereo
 * observations of the landmarks they share, the landmarks eliminated.  `windows` windows per call, device-resident, no GTSAM.  The
 * objective follows the reference; the schedule is the pose-only solver's and is stated here - the rule is NOT "whatever GTSAM's smart
 * factors do".  Measurements are fp32 and are widened on load; all arithmetic is fp64.  The rule:
 *   Camera as in sship_pose_set_camera.  Poses are Twc = [R | t], row-major 3x4, 12 doubles.
 *   Window w has K = max_keyframes slots, the oldest first; n_kf = n_kf_dev[w] clamped to [0, K] (NULL: K).  Slot 0 is the gauge and is
 *     HELD FIXED (the reference pins it with a prior of sigma 1e-4, WindowSmoother.cc:58-60).
 *   Observation (k, i), k < n_kf, i < max_obs: meas[w, k, i] = (uL, uR, v) f32 and track[w, k, i] i32.  It is PRESENT iff
 *     0 <= track < max_landmarks, the three floats are finite (the (uL, NaN, vL) rows of stereo association are absent without a flag), and
 *     no lower row i' < i of the same keyframe is present with the same landmark (the lowest row wins).
 *   Landmark l is ACTIVE iff it has present observations in at least 2 keyframes (WindowSmoother.cc:85-87) and at least one of them has
 *     uL - uR > 0.  Only observations of active landmarks count: n_obs is their number, n_landmarks the number of active landmarks.
 *   Initial point: from the present observation with uL - uR > 0 in the lowest slot k: Xc = backproject_cam (LoopCloser.cc:19-24:
 *     Z = fx baseline / (uL - uR), X = (uL - cx) Z / fx, Y = (v - cy) Z / fy) in fp64, X_l = R_k Xc + t_k with pose0 of that slot; kept in fp64.
 *   Residual: q = R_k^T (X_l - t_k); r = projection(q) - meas with the pose-only rule's projection; whitened r~ = r / sigma_px on all three
 *     components (the smart factors need isotropic noise, WindowSmoother.cc:62-68).  Behind the camera, !(q.z > 0): the constant residual
 *     r = (2 fx, 2 fx, 2 fx) and zero Jacobians.
 *   Huber on e = |r~| with k^2 = huber_k2: rho = e^2 / 2 for e <= k, k e - k^2 / 2 above; IRLS weight w = min(1, k / e).  It stands where
 *     the reference's setDynamicOutlierRejectionThreshold(3.0) stands; the reference drops such observations, here they are down-weighted.
 *   Jacobians, whitened: Jp (3x6) for the right perturbation T Exp(xi), xi = (omega, v): dq/d omega = [q]x, dq/dv = -I;  Jl (3x3): dq/dX = R_k^T.
 *   Normal equations at a state: c = sum rho;  per slot k >= 1: A_k = sum w Jp^T Jp, a_k = sum w Jp^T r~;  per active landmark:
 *     C_l = sum w Jl^T Jl, c_l = sum w Jl^T r~;  per observation W_kl = w Jp^T Jl (6x3).  Slot 0's observations enter c, C_l and c_l only.
 *   One trial at damping lambda: C~_l = C_l + lambda I = L L^T by 3x3 Cholesky;  S = blockdiag(A_k + lambda I) - sum_l W_kl C~_l^-1 W_k'l^T
 *     over k, k' >= 1;  b = -a + sum_l W_kl C~_l^-1 c_l;  Cholesky of S, of order 6 (n_kf - 1) <= 90, gives delta_k (delta_0 = 0);
 *     delta_l = -C~_l^-1 (c_l + sum_k W_kl^T delta_k);  T_k' = T_k Exp(delta_k), the full SE(3) exponential without re-orthonormalisation;
 *     X_l' = X_l + delta_l.  A pivot that is not > 0, in any 3x3 or in S, makes the trial a rejected one: counted, nothing evaluated.
 *   Schedule: the pose-only rule's.  (c, normal equations) at the start, lambda = lambda0.  Repeat: trials == max_iterations stops with
 *     ITER_CAP; one trial; c' at the candidate; then, in this order: c' finite and |c - c'| <= max(abs_tol, rel_tol c): take it, CONVERGED,
 *     stop;  else c' < c: accept, lambda /= 10, new normal equations;  else reject, lambda *= 10, and lambda > lambda_max stops with STALLED.
 *   n_kf < 2 (the reference's "need parallax" return) or no active landmark: TOO_FEW.  A non-finite pose0 in a slot < n_kf: BAD_INPUT.  In
 *     both every pose out is the pose in, trials and both costs are 0, and every landmark out is NaN; n_obs and n_landmarks are still counted.
 *   A finite pose0 whose arithmetic overflows cannot be evaluated: the initial cost is NaN or Inf, every pivot fails, the trials are counted
 *     without an evaluation until lambda passes lambda_max, and the window ends STALLED with the pose in and both costs out non-finite.
 *   Defaults: sigma_px 1, huber_k2 9 (3 sigma), lambda0 1e-5, lambda_max 1e5, abs_tol = rel_tol = 1e-3 (the reference's,
 *     WindowSmoother.cc:96-97), max_iterations 20 (it counts trials; the reference caps GTSAM's outer iterations at 4).
 *   Two further differences from the smart factors: landmarks are variables eliminated by the Schur complement at their current estimate,
 *     not re-triangulated at every linearisation; a degenerate landmark is simply an ill-conditioned 3x3 that lambda regularises (no
 *     ZERO_ON_DEGENERACY mode).
 *   A consequence of down-weighting instead of dropping: a landmark seen in TWO keyframes of which one measurement is a gross mismatch has no
 *     point that fits both rays.  Its observations keep a Huber pull of k on the poses and its point drifts far away (finite, up to 1e7 m on
 *     the tests' scenes) while the window still ends CONVERGED or at ITER_CAP; with a fifth of the two-view tracks corrupted the poses were
 *     recovered to 0.01 - 0.12 m instead of 0.01 - 0.02 m (tests/test_ba_cpu.py pins this).  A caller whose matches carry such mismatches
 *     should gate them before the solve (the keypoint-window gate, the inlier mask of sship_ransac_* or of the pose-only solve) or leave
 *     two-view tracks out.
 *   Determinism: every sum runs in one fixed order - the blocks of a landmark over its slots in ascending k, the sums of a slot and of
 *     the cost per thread over its rows in index order, then lanes, then waves; every entry of S and b over the active landmarks in ascending
 *     l by one thread.  A window gives the same bits alone, inside any batch, at any batch position, and on a second call.
 * Handle: sship_ba_create(max_keyframes 2..16, max_obs 1..2048, max_landmarks 1..32768, max_windows 1..65535).  Workspace, allocated once
 * at create:  min(max_windows, 512) x ceil16(max_landmarks (4 max_keyframes + 204) + 288 max_keyframes max_obs) bytes (a launch runs at most
 * 512 workgroups, which walk the windows), plus the staging of sship_ba_solve_host, one window's inputs and outputs.
 * Bad arguments are refused with SSHIP_ERR_INVALID and a message before any device is touched, the handle unchanged: a NULL handle or
 * pointer, a create argument or `windows` out of range, a camera not set, fx, fy or baseline not > 0 (or any camera value not finite), a NaN
 * in the params, sigma_px, huber_k2 or lambda0 not > 0 (or not finite), lambda_max < lambda0 or infinite, a negative tolerance,
 * max_iterations < 1.  Valid create arguments without a GPU give SSHIP_ERR_NO_DEVICE.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_ba sship_ba;
typedef struct sship_ba_params {
  double sigma_px, huber_k2;
  double lambda0, lambda_max, abs_tol, rel_tol;
  int max_iterations;
} sship_ba_params;
#define SSHIP_BA_CONVERGED 0
#define SSHIP_BA_ITER_CAP 1
#define SSHIP_BA_STALLED 2
#define SSHIP_BA_TOO_FEW 3
#define SSHIP_BA_BAD_INPUT 4
int sship_ba_create(int max_keyframes, int max_obs, int max_landmarks, int max_windows, sship_ba** out);
void sship_ba_destroy(sship_ba* ba);
int sship_ba_set_camera(sship_ba* ba, double fx, double fy, double cx, double cy, double baseline);
int sship_ba_get_camera(const sship_ba* ba, double* fx, double* fy, double* cx, double* cy, double* baseline); /* any output may be NULL */
int sship_ba_set_params(sship_ba* ba, const sship_ba_params* params);
int sship_ba_get_params(const sship_ba* ba, sship_ba_params* params);
/* Throughput path, one launch, asynchronous on `stream` (NULL = the legacy default stream), no host synchronisation inside; calls on one
 * handle share its workspace and must be ordered by the caller.  meas_dev [windows, K, max_obs, 3] f32, track_dev [windows, K, max_obs] i32,
 * n_kf_dev [windows] i32 or NULL, pose0_dev [windows, K, 12] f64;  pose_dev [windows, K, 12] f64 (slot 0 and slots >= n_kf keep the bits of
 * pose0), stats_dev [windows, 4] i32 = (n_obs, n_landmarks, trials, status), cost_dev [windows, 2] f64 = (initial, final), landmarks_dev
 * [windows, max_landmarks, 3] f32 or NULL: the final X_l rounded once for active landmarks, quiet NaN elsewhere.  Every entry is written. */
int sship_ba_solve_batch_device(sship_ba* ba, const float* meas_dev, const int32_t* track_dev, const int32_t* n_kf_dev, const double* pose0_dev,
                                int windows, double* pose_dev, int32_t* stats_dev, double* cost_dev, float* landmarks_dev, void* stream);
/* One window from host arrays - the drop-in for one WindowSmoother::optimize: meas [K, max_obs, 3], track [K, max_obs], n_kf in 0..K,
 * pose0 [K, 12]; pose_out [K, 12], stats_out [4], cost_out [2], landmarks_out [max_landmarks, 3] or NULL.  Synchronous on the handle's own
 * stream; the same launch as the batch call with windows = 1, hence the same bits. */
int sship_ba_solve_host(sship_ba* ba, const float* meas, const int32_t* track, int n_kf, const double* pose0, double* pose_out,
                        int32_t* stats_out, double* cost_out, float* landmarks_out);
/* The landmark bookkeeping of VoEstimator.cc:208-214,252-266,306-315 as a device stage, one launch, asynchronous on `stream`:
 * has_depth_dev [windows, K, max_obs] u8 (of sship_stereo_associate_batch_device), matches_dev [windows, K - 1, max_obs] i32 where
 * matches_dev[w, k] is matches0 from keyframe k's to keyframe k + 1's left keypoints, n_dev [windows, K] i32 left-image counts (clamped to
 * [0, max_obs]), n_kf_dev [windows] or NULL;  track_dev [windows, K, max_obs] i32.
 *   track[0][i] = i for a row i < n_0 with has_depth.  For k >= 1 and a row j < n_k with has_depth: if some i < n_{k-1} has
 *   matches[k-1][i] == j and track[k-1][i] >= 0 then track[k][j] = track[k-1][i], the HIGHEST such i winning (the reference's map
 *   assignment in ascending match order); otherwise track[k][j] = k max_obs + j, a new landmark named by its first observation.
 *   Every other entry, slots >= n_kf included, is -1; every entry is written.  Needs max_landmarks >= max_keyframes max_obs. */
int sship_ba_tracks_from_matches_batch_device(const sship_ba* ba, const uint8_t* has_depth_dev, const int32_t* matches_dev, const int32_t* n_dev,
                                              const int32_t* n_kf_dev, int windows, int32_t* track_dev, void* stream);
/* Measurement hook: re-run the last solve call's launch on this handle `iters` times (over the same buffers, which the caller of a batch
 * call keeps alive), timed with hipEvents on the handle's stream; *avg_ms = mean duration of one launch. */
int sship_ba_bench(sship_ba* ba, int iters, float* avg_ms);

/* ------------------------------------------------------------------------------------------------
 * Pose graph - what GlobalPoseGraph::optimize_and_get_all does (src/GlobalPoseGraph.cc:56-98): the keyframe poses re-optimised against the
 * odometry chain and the accepted loop closures, with the reference's drop-the-last-loop retry inside the launch.  `graphs` independent
 * graphs per call, device-resident, fp64, no GTSAM.  The objective is the reference's (BetweenFactor<Pose3> under diagonal noise, Huber on
 * the loops); the schedule is the pose-only solver's and is stated here - the rule is NOT "whatever GTSAM does".  The rule:
 *   Graph g has n = n_nodes_dev[g] nodes clamped to [0, max_nodes] (NULL: max_nodes), in insertion order.  Poses are Twc = [R | t],
 *     row-major 3x4, 12 doubles.  Node 0 is the gauge and is HELD FIXED (the reference pins it with a prior of sigma 1e-4,
 *     GlobalPoseGraph.cc:29-30).
 *   Odometry slot k < n - 1 (backbone_): odom_z[g, k] is the measured T_k^-1 T_{k+1}, odom_sigma[g, k, 0..5] its sigmas (rotation x3,
 *     translation x3; a NULL array: (odom_sigma_rot x3, odom_sigma_trans x3) of the params, defaults 0.02 / 0.05, VoEstimator.cc:33-37).
 *     No robust kernel.  The slot is PRESENT iff its 12 + 6 values are finite and every sigma is > 0.
 *   Loop record l < max_loops (loops_): (i, j, Z, sigma[6], huber_k2).  PRESENT iff 0 <= i, j < n, i != j, all 12 + 6 + 1 values finite,
 *     every sigma > 0, its enable byte non-zero (NULL: all) and the rejection loop below has not dropped it.  huber_k2 <= 0: no robust
 *     kernel.  |i - j| == 1 is allowed and is still a loop record.  Anything absent contributes nothing, whatever it holds.
 *   Residual of an edge (i, j, Z): r = Log(Z^-1 T_i^-1 T_j) = (omega, v), rotation first.  Log of E = [R_E | t_E]:
 *     a = ((R21 - R12) / 2, (R02 - R20) / 2, (R10 - R01) / 2), s = |a|, c = (trace R_E - 1) / 2, theta = atan2(s, c);
 *     omega = a / A(theta) for theta^2 < 1e-2, a theta / s otherwise;  v = t_E - (omega x t_E) / 2 + D(theta) omega x (omega x t_E).
 *     (Within 1e-3 of theta = pi, s loses its digits and so does omega; no special branch.)
 *   Coefficients, x = theta^2.  For x >= 1e-2 the closed forms A = sin(theta) / theta, B = 2 sin^2(theta / 2) / x, C = (theta - sin) / theta^3,
 *     D = (1 - A / (2 B)) / x, C2 = (x + 2 cos - 2) / (2 x^2), C3 = (2 theta - 3 sin + theta cos) / (2 x^2 theta);  for x < 1e-2 the series
 *     A = 1 - x/6 (1 - x/20 (1 - x/42 (1 - x/72))),  B = (1 - x/12 (1 - x/30 (1 - x/56 (1 - x/90)))) / 2,
 *     C = (1 - x/20 (1 - x/42 (1 - x/72 (1 - x/110)))) / 6,  D = 1/12 + x/720 + x^2/30240 + x^3/1209600,
 *     C2 = (1 - x/30 (1 - x/56 (1 - x/90))) / 24,  C3 = 1/120 - x/2520 + x^2/120960 - x^3/9979200.
 *   Whitened r~ = r / sigma.  e = |r~|, k^2 = huber_k2: rho = e^2 / 2 for e <= k, k e - k^2 / 2 above; IRLS weight w = min(1, k / e).
 *   Jacobians for the right perturbation T Exp(xi), xi = (omega, v):  dr/dxi_j = Jr^-1(r),  dr/dxi_i = -Jr^-1(r) Ad(T_j^-1 T_i),
 *     Ad(T) = [[R, 0], [[t]x R, R]],  Jr^-1(r) = Jl(-r)^-1,  Jl(omega, v)^-1 = [[Ai, 0], [-Ai Q Ai, Ai]] with P = [omega]x, R = [v]x,
 *     Ai = I - P / 2 + D P^2 and Q = R / 2 + C (PR + RP + PRP) + C2 (PPR + RPP - 3 PRP) + C3 (PRPP + PPRP)  (Barfoot, eq. 7.86b).
 *     Whitened J~ = diag(1 / sigma) J.
 *   Normal equations over the free nodes 1 .. n-1:  H = sum w J~^T J~,  g = sum w J~^T r~,  c = sum rho.  The sums of a node run over its
 *     edges in the order odometry k-1, odometry k, loops in ascending record index; c per thread over the edges e = tid, tid + 256, ...
 *     (odometry slots, then loop records), then lanes, then waves.
 *   One trial at damping lambda solves (H + lambda I) delta = -g by Cholesky in this elimination order (nested dissection of the chain at
 *     the loop endpoints):  a free node that is the endpoint of no present loop is INTERIOR;  each maximal run of interior nodes (a
 *     SEGMENT) is eliminated from its lowest index upward - a block-tridiagonal Cholesky whose only fill is the block between the segment's
 *     two bounding nodes;  the loop endpoints (SEPARATORS) are then eliminated in ascending node index by a dense Cholesky of order
 *     6 x (number of separators) <= 12 max_loops.  A scalar pivot that is not > 0, anywhere, makes the trial a rejected one: counted,
 *     nothing evaluated.  Otherwise T_k' = T_k Exp(delta_k), the full SE(3) exponential of the pose-only rule, without
 *     re-orthonormalisation; delta_0 = 0.
 *   Schedule: the pose-only rule's.  (c, normal equations) at the start, lambda = lambda0.  Repeat: this attempt's trials == max_iterations
 *     stops with ITER_CAP; one trial; c' at the candidate; then, in this order: c' finite and |c - c'| <= max(abs_tol, rel_tol c): take it,
 *     CONVERGED, stop;  else c' < c: accept, lambda /= 10, new normal equations;  else reject, lambda *= 10 (the same normal equations are
 *     factorised again), and lambda > lambda_max stops with STALLED.
 *   The rejection loop (GlobalPoseGraph.cc:56-93): after the schedule ends the result is SANE iff every pose entry of a node < n is finite
 *     and every |t| <= max_translation.  Not sane and a present loop exists: the present loop with the highest record index is dropped,
 *     loops_dropped grows by one and the solve restarts from pose0 with lambda0 (a new attempt).  Not sane and no loop left: every pose out
 *     is the pose in, status DIVERGED.  `trials` counts over all attempts; the costs out are the first attempt's initial cost and the last
 *     attempt's final cost.  GTSAM's IndeterminantLinearSystemException has no counterpart: a failed pivot is a rejected trial.
 *     What the rejection loop catches is a loop that the solve FOLLOWS out of every sane range, such as a loop 1e9 m long from node 0 with
 *     tight sigmas.  The same loop between two free nodes defeats every step instead (the damping is lambda I with lambda <= lambda_max,
 *     nothing next to a Hessian of 1e24): the attempt ends STALLED at pose0, which is sane, nothing is dropped, and loop_chi2 names the loop
 *     (tests/test_pg_cpu.py pins both).
 *   n < 2 or no present edge: TOO_FEW.  A non-finite pose0 in a node < n: BAD_INPUT.  In both every pose out is the pose in, trials,
 *     loops_dropped and both costs are 0, and every loop_chi2 is NaN; n_edges is still counted.
 *   A node that no present edge connects to node 0 is held by lambda alone and stays where it is; it is not detected.
 *   Defaults: odom sigmas 0.02 / 0.05, max_translation 1e6, and GTSAM's, which the reference uses unchanged (GlobalPoseGraph.cc:77):
 *     lambda0 1e-5, lambda_max 1e5, abs_tol = rel_tol = 1e-5, max_iterations 100 (it counts trials).
 *   Determinism: every sum runs in one fixed order and there are no floating-point atomics: a graph gives the same bits alone, inside any
 *     batch, at any batch position and on a second call.
 * Handle: sship_pg_create(max_nodes 2..4096, max_loops 0..128, max_graphs 1..65535).  Workspace, allocated once at create:
 * min(max_graphs, 256) slices (a launch runs at most 256 workgroups, which walk the graphs) of
 *   ceil16(8 (80 (N - 1 + L) + 222 N + 120 (S + 1) + (6 S)^2) + 4 (3 N + 5 S + 2))  bytes,  N = max_nodes, L = max_loops,
 *   S = min(2 L, N - 1) the most separators a graph can have,
 * plus the staging of sship_pg_solve_host, one graph's inputs and outputs.
 * Bad arguments are refused with SSHIP_ERR_INVALID and a message before any device is touched, the handle unchanged: a NULL handle or
 * pointer (the loop arrays may all be NULL when max_loops == 0; they must be all NULL or all given), a create argument, `graphs`, `n_nodes`
 * or `n_loops` out of range, a NaN in the params, a sigma, lambda0 or max_translation not > 0 (or not finite), lambda_max < lambda0 or
 * infinite, a negative tolerance, max_iterations < 1, min_inliers < 1, noise_base not finite and > 0.  Valid create arguments without a GPU
 * give SSHIP_ERR_NO_DEVICE.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_pg sship_pg;
typedef struct sship_pg_params {
  double odom_sigma_rot, odom_sigma_trans;
  double lambda0, lambda_max, abs_tol, rel_tol;
  double max_translation;
  int max_iterations;
} sship_pg_params;
#define SSHIP_PG_CONVERGED 0
#define SSHIP_PG_ITER_CAP 1
#define SSHIP_PG_STALLED 2
#define SSHIP_PG_TOO_FEW 3
#define SSHIP_PG_BAD_INPUT 4
#define SSHIP_PG_DIVERGED 5
int sship_pg_create(int max_nodes, int max_loops, int max_graphs, sship_pg** out);
/* The bytes of one workspace slice as the library lays it out (the formula above); 0 for sizes that sship_pg_create refuses.  No device. */
size_t sship_pg_workspace_slice_bytes(int max_nodes, int max_loops);
void sship_pg_destroy(sship_pg* pg);
int sship_pg_set_params(sship_pg* pg, const sship_pg_params* params);
int sship_pg_get_params(const sship_pg* pg, sship_pg_params* params);
/* Throughput path, one launch, asynchronous on `stream` (NULL = the legacy default stream), no host synchronisation inside; calls on one
 * handle share its workspace and must be ordered by the caller.  With N = max_nodes and L = max_loops:  n_nodes_dev [graphs] i32 or NULL,
 * pose0_dev [graphs, N, 12] f64, odom_z_dev [graphs, N - 1, 12] f64, odom_sigma_dev [graphs, N - 1, 6] f64 or NULL, loop_ij_dev
 * [graphs, L, 2] i32, loop_z_dev [graphs, L, 12] f64, loop_sigma_dev [graphs, L, 6] f64, loop_k2_dev [graphs, L] f64, loop_enable_dev
 * [graphs, L] u8 or NULL;  pose_dev [graphs, N, 12] f64 (node 0 and nodes >= n keep the bits of pose0), stats_dev [graphs, 4] i32 =
 * (n_edges, loops_dropped, trials, status) with n_edges the present odometry slots plus the loops present in the last attempt, cost_dev
 * [graphs, 2] f64 = (initial, final), loop_chi2_dev [graphs, L] f64 or NULL: e^2 of each loop present in the last attempt at the final
 * poses, quiet NaN elsewhere.  Every entry of the outputs is written.  No output array may overlap an input array (pose_dev != pose0_dev:
 * the solve restarts from pose0 after a dropped loop, and the kernel reads it to the end).
 * Length of a launch: a graph is solved by ONE workgroup, a segment by one wave node after node, and the separator system is factorised
 * column by column in the workspace.  Measured on an MI355X: about 3 ms per trial for 256 graphs of 512 nodes and 16 loops,
 * 12 ms per trial for one graph of 4 096 nodes and 16 loops, and 0.55 s per trial with 128 loops (separator order 1 536) - so a launch
 * that runs into max_iterations = 100 there occupies its compute unit for about a minute.  A caller on a shared device bounds it with
 * max_iterations. */
int sship_pg_solve_batch_device(sship_pg* pg, const int32_t* n_nodes_dev, const double* pose0_dev, const double* odom_z_dev,
                                const double* odom_sigma_dev, const int32_t* loop_ij_dev, const double* loop_z_dev,
                                const double* loop_sigma_dev, const double* loop_k2_dev, const uint8_t* loop_enable_dev, int graphs,
                                double* pose_dev, int32_t* stats_dev, double* cost_dev, double* loop_chi2_dev, void* stream);
/* One graph from host arrays - the drop-in for one optimize_and_get_all: pose0 [n_nodes, 12], odom_z [n_nodes - 1, 12], odom_sigma
 * [n_nodes - 1, 6] or NULL, n_loops in 0..max_loops records loop_ij [n_loops, 2], loop_z [n_loops, 12], loop_sigma [n_loops, 6], loop_k2
 * [n_loops] (all enabled);  pose_out [n_nodes, 12], stats_out [4], cost_out [2], loop_chi2_out [n_loops] or NULL.  n_nodes in 0..max_nodes.
 * Synchronous on the handle's own stream; the same launch as the batch call with graphs = 1, hence the same bits. */
int sship_pg_solve_host(sship_pg* pg, int n_nodes, const double* pose0, const double* odom_z, const double* odom_sigma, int n_loops,
                        const int32_t* loop_ij, const double* loop_z, const double* loop_sigma, const double* loop_k2, double* pose_out,
                        int32_t* stats_out, double* cost_out, double* loop_chi2_out);
/* VoEstimator.cc:337-339 on the output of sship_ba_solve_batch_device, one launch, asynchronous on `stream`: from pose_dev [graphs, N, 12]
 * odom_z_dev[g, k] = T_k^-1 T_{k+1} = [R_k^T R_{k+1} | R_k^T (t_{k+1} - t_k)] for k < N - 1, every three-term sum as (a0 b0 + a1 b1) + a2 b2
 * with each product and sum rounded once (no fused multiply-add).  A non-finite pose gives a non-finite, hence absent, slot. */
int sship_pg_odometry_from_poses_batch_device(const sship_pg* pg, const double* pose_dev, int graphs, double* odom_z_dev, void* stream);
/* LoopCloser.cc:66-101 on the outputs of sship_pose_solve_batch_device, one launch, asynchronous on `stream`.  Pair p = g max_loops + l
 * fills loop record l of graph g: i = from_dev[p] (the candidate), j = to_dev[p] (the query), Z = pose_dev[p] (T_candidate_query), with
 * stats_dev [pairs, 4] the pose solver's (n_obs, n_inliers, trials, status).  Accepted iff n_obs >= min_inliers && n_inliers >= min_inliers,
 * the status is neither TOO_FEW nor BAD_INPUT, and Z is finite.  s = noise_base / sqrt(n_inliers);  sigma = (max(s, 0.02) x3,
 * max(s, 0.20) x3);  huber_k2 = 7.815;  the enable byte is the accepted flag.  A record that is not accepted carries Z and (i, j) as
 * given and sigma = (0.02 x3, 0.20 x3).  Every entry of the five outputs is written.  The reference's min_inliers is 30, noise_base 0.1. */
int sship_pg_loops_from_pose_batch_device(const sship_pg* pg, const int32_t* from_dev, const int32_t* to_dev, const double* pose_dev,
                                          const int32_t* stats_dev, int graphs, int min_inliers, double noise_base, int32_t* loop_ij_dev,
                                          double* loop_z_dev, double* loop_sigma_dev, double* loop_k2_dev, uint8_t* loop_enable_dev,
                                          void* stream);
/* Measurement hook: re-run the last solve call's launch on this handle `iters` times (over the same buffers, which the caller of a batch
 * call keeps alive), timed with hipEvents on the handle's stream; *avg_ms = mean duration of one launch. */
int sship_pg_bench(sship_pg* pg, int iters, float* avg_ms);

/* ------------------------------------------------------------------------------------------------
 * Rectification - the two cv::remap calls of the EuRoC runner (examples/stereo/euroc.cc:88-133,176-177) as a device stage, and the maps
 * cv::initUndistortRectifyMap builds for them.  The rule is OpenCV's, restated here; OpenCV is not a dependency and equality with cv::remap
 * is the intent of the rule, NOT something the tests check (they check the library against tests/_rect_ref.py, which restates this text).
 *
 * Map construction (cv::initUndistortRectifyMap, m1type = CV_32F): pure host, fp64, this operation order.
 *   K 3x3 row-major (fx = K[0], cx = K[2], fy = K[4], cy = K[5]);  D = n_dist coefficients of k1 k2 p1 p2 k3 k4 k5 k6, missing ones 0,
 *   n_dist in {0, 4, 5, 8};  R 3x3 (NULL = identity);  Pnew 3x3 (the left block of P).
 *   A = Pnew R with A[i][j] = (Pnew[i][0] R[0][j] + Pnew[i][1] R[1][j]) + Pnew[i][2] R[2][j];  iR = adj(A) / det(A) by cofactors,
 *   det = (A00 c00 + A01 c01) + A02 c02.  det == 0 or a non-finite iR -> SSHIP_ERR_INVALID.
 *   For the destination pixel (u, v):  X = (iR00 u + iR01 v) + iR02, Y and W alike from rows 1 and 2;  x = X / W, y = Y / W;
 *   x2 = x x, y2 = y y, r2 = x2 + y2, xy2 = (2 x) y;
 *   kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2);
 *   xd = (x kr + p1 xy2) + p2 (r2 + 2 x2);    yd = (y kr + p1 (r2 + 2 y2)) + p2 xy2;
 *   map_x = fx xd + cx, map_y = fy yd + cy, each rounded once to fp32.  Tables are [dst_h, dst_w] row-major.
 *
 * Remap (cv::remap, u8, INTER_LINEAR, BORDER_CONSTANT 0, OpenCV's fixed-point form), per destination pixel:
 *   sx = rint(map_x * 32), sy = rint(map_y * 32)        the product is exact in fp32; ties to even
 *   ix = sx >> 5, iy = sy >> 5, ax = sx & 31, ay = sy & 31
 *   acc = (32-ax)(32-ay) S(iy,ix) + ax (32-ay) S(iy,ix+1) + (32-ax) ay S(iy+1,ix) + ax ay S(iy+1,ix+1)     a tap outside the source is 0
 *   dst = (acc + 512) >> 10
 * All of it integer arithmetic: the result does not depend on summation order, batch position or path.
 * Our additions: a map entry that is not finite, or has |map * 32| > 2^20, makes its pixel 0.  That is decided when the table is built,
 * on the host; the kernel never sees such an entry.
 *
 * sship_rect_fixed_table is the table of the rule, pure host: ix / iy i32, frac u16 = ax | ay << 5; a degenerate entry is (0, 0, 0xFFFF).
 * The handle's device table (sship_rect_read_table) is that table after set_maps has resolved the border: a pixel none of whose taps is
 * both inside the source and of non-zero weight - degenerate ones included - reads (-2, -2, 0); every other pixel reads as the rule states.
 *
 * The handle: `cameras` (1 or 2) tables for one source and one destination size (each axis in [1, 4096]).  sship_rect_set_maps takes
 * host fp32 tables (what a holder of cv::Mat maps has), builds the fixed-point table and one source box per 64 x 16 destination tile
 * on the host, and uploads them (it synchronises the device first: do not call it with a remap of this handle in flight).  A tile whose
 * box fits 16 KiB of LDS is remapped from a staged copy of the box; any other tile (a transpose, a strong minification) reads its taps
 * from global memory.  Same arithmetic, same bits.  sship_rect_tile_paths reports how many tiles of a camera took each path.
 * sship_rect_set_camera = sship_rect_build_maps + sship_rect_set_maps.
 *
 * sship_rect_remap_batch_device: src_dev [images, src_h, src_stride] u8 (src_stride in bytes, >= src_w; no alignment is required of the
 * pointer or the stride), dst_dev [images, dst_h, dst_w] contiguous u8.  Image i uses camera i % cameras: with cameras = 2 the output is
 * the L0, R0, L1, R1, ... layout sship_frontend_batch_device takes.  One launch, asynchronous on `stream`, no host synchronisation.
 * A camera the batch uses that has no maps -> SSHIP_ERR_INVALID.  sship_rect_remap_host: one image from host arrays through the handle's
 * own stream (dst is [dst_h, dst_w] contiguous), the drop-in for one cv::remap call.
 * sship_rect_bench: `images` synthetic images through the handle's tables, `iters` launches timed with hipEvents; path = SSHIP_RECT_PATH_TILE
 * (each tile on the path set_maps chose) or SSHIP_RECT_PATH_DIRECT (every tile from global memory).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_rect sship_rect;
#define SSHIP_RECT_PATH_TILE 0
#define SSHIP_RECT_PATH_DIRECT 1
int sship_rect_build_maps(const double* K, const double* D, int n_dist, const double* R, const double* Pnew, int dst_w, int dst_h,
                          float* map_x, float* map_y);
int sship_rect_fixed_table(const float* map_x, const float* map_y, size_t count, int32_t* ix, int32_t* iy, uint16_t* frac);
int sship_rect_create(int src_w, int src_h, int dst_w, int dst_h, int cameras, sship_rect** out);
void sship_rect_destroy(sship_rect* rect);
int sship_rect_set_maps(sship_rect* rect, int camera, const float* map_x, const float* map_y);
int sship_rect_set_camera(sship_rect* rect, int camera, const double* K, const double* D, int n_dist, const double* R, const double* Pnew);
int sship_rect_read_table(sship_rect* rect, int camera, int32_t* ix, int32_t* iy, uint16_t* frac);
int sship_rect_tile_paths(const sship_rect* rect, int camera, int* staged, int* direct);
int sship_rect_remap_batch_device(sship_rect* rect, const uint8_t* src_dev, int images, int src_stride, uint8_t* dst_dev, void* stream);
int sship_rect_remap_host(sship_rect* rect, int camera, const uint8_t* src, int src_stride, uint8_t* dst);
int sship_rect_bench(sship_rect* rect, int images, int path, int iters, float* avg_ms);

/* ------------------------------------------------------------------------------------------------
 * RGB-D association - the per-keypoint loop of RgbdFrontEnd::process (src/RgbdFrontEnd.cc:27-56) as a device stage.
 * kp_dev [frames, max_keypoints, 3] f32 (x, y, score) raw keypoints as the extractor writes them, n_dev [frames] i32 (clamped to
 * [0, max_keypoints] on the device), depth_dev [frames, h, depth_stride] with depth_stride in bytes (a multiple of the sample size),
 * depth_type SSHIP_DEPTH_U16 or SSHIP_DEPTH_F32.  Per keypoint (u, v):
 *   hasDist = any of dist[0..7] (k1 k2 p1 p2 k3 k4 k5 k6) is non-zero.
 *   hasDist: cv::undistortPoints' fixed 5 iterations, fp64:  x0 = (u - cx) / fx, y0 = (v - cy) / fy, x = x0, y = y0;  each iteration
 *     r2 = x x + y y;  ic = (1 + ((k6 r2 + k5) r2 + k4) r2) / (1 + ((k3 r2 + k2) r2 + k1) r2);  ic < 0: restore (x0, y0) and stop;
 *     x = (x0 - (2 p1 x y + p2 (r2 + 2 x x))) ic,  y = (y0 - (p1 (r2 + 2 y y) + 2 p2 x y)) ic   (both from the x, y before the step);
 *     u' = fx x + cx, v' = fy y + cy, rounded to fp32.    Not hasDist: (u', v') are the keypoint's own bits.
 *   Depth is sampled at (lround(u), lround(v)) of the RAW keypoint - half away from zero; a sample outside the image, or a NaN coordinate, is 0.
 *   Z = d / depth_factor in fp64;   has_depth = (Z > 0 && Z < max_depth), this positive form: a NaN depth gives none.
 *   stereo = (u', has_depth ? fp32(u' - bf / Z) : quiet NaN, v')       the subtraction and the division in fp64
 * Rows >= n are (0, NaN, 0) / 0 and every entry is written: the output convention of sship_stereo_associate_batch_device, so the result
 * feeds sship_pose_obs_from_matches_batch_device and sship_ba_tracks_from_matches_batch_device unchanged.  kp_undist_dev (optional, NULL =
 * not wanted) [frames, max_keypoints, 3] = (u', v', score), rows >= n zero.  One launch, asynchronous on `stream`.
 * frames >= 1, max_keypoints in [1, 4096], h, w in [1, 16384]; fx, fy, depth_factor finite and > 0; max_depth not NaN.
 * ---------------------------------------------------------------------------------------------- */
#define SSHIP_DEPTH_U16 0
#define SSHIP_DEPTH_F32 1
typedef struct sship_rgbd_params {
  double fx, fy, cx, cy;
  double dist[8];       /* k1 k2 p1 p2 k3 k4 k5 k6 */
  double bf;            /* fx * baseline (Camera.bf) */
  double depth_factor;  /* DepthMapFactor */
  double max_depth;
} sship_rgbd_params;
int sship_rgbd_associate_batch_device(const float* kp_dev, const int* n_dev, int frames, int max_keypoints, const void* depth_dev,
                                      int depth_type, int h, int w, int depth_stride, const sship_rgbd_params* params,
                                      float* kp_undist_dev, float* stereo_dev, uint8_t* has_depth_dev, void* stream);
/* One frame from host arrays (the loop of RgbdFrontEnd::process as it stands): keypoints[i * kp_stride + {0, 1}] = (x, y), n in [0, 4096]
 * (0: nothing is touched), depth [h, depth_stride bytes]; kp_undist [n, 2], stereo [n, 3], has_depth [n].  Synchronous. */
int sship_rgbd_associate_host(const float* keypoints, int kp_stride, int n, const void* depth, int depth_type, int h, int w, int depth_stride,
                              const sship_rgbd_params* params, float* kp_undist, float* stereo, uint8_t* has_depth);

/* ------------------------------------------------------------------------------------------------
 * Stereo refinement - sub-pixel uR by a short 1-D patch search in the rectified image pair, after descriptor matching.  No reference
 * counterpart: StereoFrontEnd::process copies uR from the right image's keypoint (src/StereoFrontEnd.cc:35-47), an integer NMS peak found
 * independently of the left one.  The rule is this library's own (zero-mean SSD, parabola through the three costs around the minimum) and
 * is stated here in full; tests/_stereo_refine_ref.py restates this text.  All of it is integer arithmetic on u8 pixels, one fp64 division,
 * two fp64 additions and one rounding to fp32: the result does not depend on summation order, batch position or entry point.
 *
 * imgs_dev [2 * pairs, h, stride] u8, the L0, R0, L1, R1, ... layout sship_rect_remap_batch_device writes: IL = image 2p, IR = image
 * 2p + 1 of pair p.  stride is in bytes, >= w; no alignment is required of the pointer or the stride.  stereo_in_dev [pairs, max_keypoints,
 * 3] f32 = (uL, uR, vL) and has_depth_in_dev [pairs, max_keypoints] u8 as the association stages write them.  The left count n0 of pair
 * p is n_dev[p * n_stride] clamped to [0, max_keypoints] on the device: n_stride = 2 for an extractor's [2 * pairs] count array, 1 for
 * a [pairs] array.  w = half_window, L = search_radius, N = (2w+1)^2.  Keypoint i of pair p, in this order:
 *   1. i >= n0: (0, quiet NaN, 0), has_depth 0, status NONE, cost -1 - the association's convention; every entry is written.
 *   2. has_depth_in == 0: (uL, quiet NaN, vL), has_depth 0, status NONE, cost -1.
 *   3. Any of uL, uR, vL not finite or outside [0, 16384): status BORDER.  Otherwise, in fp64 on the fp32 value, xl = floor(uL + 0.5),
 *      xr = floor(uR + 0.5), y = floor(vL + 0.5) - both patches use the LEFT keypoint's row - and the status is BORDER unless
 *      xl-w >= 0, xl+w < w_img, y-w >= 0, y+w < h, xr-L-w >= 0 and xr+L+w < w_img.  BORDER is not a rejection: the output is the input's
 *      bits, has_depth 1, cost -1.
 *   4. For k = -L .. L over (dy, dx) in [-w, w]^2:  d = IL[y+dy, xl+dx] - IR[y+dy, xr+k+dx];  S1 = sum d, S2 = sum d^2 (int32);
 *      C_k = N S2 - S1^2 in int64 (N^2 times the zero-mean variance of the difference: invariant to a brightness offset; it reaches
 *      3 291 825 600 at w = 7).
 *   5. k* = the smallest k attaining the minimum, cost = C_k*.  |k*| == L: status EDGE.  Otherwise, with max_rms > 0 and
 *      t = (double)max_rms (double)N:  (double)cost > t t: status COST.
 *   6. Otherwise den = C_{k*-1} + C_{k*+1} - 2 C_k* (>= 1, because k* is the smallest minimiser),
 *      delta = (double)(C_{k*-1} - C_{k*+1}) / (double)(2 den)  (|delta| <= 0.5).
 *   7. uR' = (float)(((double)uL - (double)(xl - xr - k*)) + delta).  The left patch is centred on xl, not on uL, so a fractional uL keeps
 *      its fraction.
 *   8. In fp32, this positive form: uL - uR' >= min_disparity -> status REFINED, output (uL, uR', vL), has_depth 1; else status DISPARITY.
 *   9. EDGE, COST and DISPARITY are rejections: on_reject KEEP writes the input's bits with has_depth 1, DROP writes (uL, quiet NaN, vL)
 *      with has_depth 0.  cost is reported either way.
 * status_dev [pairs, max_keypoints] u8 and cost_dev [pairs, max_keypoints] i64 are optional (NULL = not wanted).  stereo_out_dev ==
 * stereo_in_dev and has_depth_out_dev == has_depth_in_dev are allowed: a row is read and written by its owner only.  One launch,
 * asynchronous on `stream`, no host synchronisation.  pairs >= 1, max_keypoints in [1, 4096], h, w in [1, 16384], half_window in [1, 7],
 * search_radius in [1, 15], max_rms (<= 0: no cost gate) and min_disparity not NaN; anything else, a NULL required pointer or stride < w
 * is SSHIP_ERR_INVALID before any device is touched.
 * ---------------------------------------------------------------------------------------------- */
#define SSHIP_REFINE_KEEP 0
#define SSHIP_REFINE_DROP 1
#define SSHIP_REFINE_STATUS_NONE 0
#define SSHIP_REFINE_STATUS_REFINED 1
#define SSHIP_REFINE_STATUS_BORDER 2
#define SSHIP_REFINE_STATUS_EDGE 3
#define SSHIP_REFINE_STATUS_COST 4
#define SSHIP_REFINE_STATUS_DISPARITY 5
typedef struct sship_stereo_refine_params {
  int half_window;      /* w: the patch is (2w+1) x (2w+1) pixels; default 5 */
  int search_radius;    /* L: offsets -L .. +L are searched; default 5 */
  float max_rms;        /* cost gate on the zero-mean RMS difference in grey levels; <= 0 is off (default 0) */
  float min_disparity;  /* smallest accepted refined disparity; default 0 */
  int on_reject;        /* SSHIP_REFINE_KEEP (default) or SSHIP_REFINE_DROP */
} sship_stereo_refine_params;
int sship_stereo_refine_batch_device(const uint8_t* imgs_dev, int pairs, int h, int w, int stride, const float* stereo_in_dev,
                                     const uint8_t* has_depth_in_dev, const int* n_dev, int n_stride, int max_keypoints,
                                     const sship_stereo_refine_params* params, float* stereo_out_dev, uint8_t* has_depth_out_dev,
                                     uint8_t* status_dev, int64_t* cost_dev, void* stream);
/* One pair from host arrays, the drop-in after one StereoFrontEnd::process: left / right [h, *_stride bytes] u8, stereo [n, 3], has_depth [n],
 * n in [0, 4096] (0: nothing is touched); stereo_out [n, 3] and has_depth_out [n] may be the inputs; status [n] and cost [n] are optional.
 * Synchronous. */
int sship_stereo_refine_host(const uint8_t* left, int left_stride, const uint8_t* right, int right_stride, int h, int w, const float* stereo,
                             const uint8_t* has_depth, int n, const sship_stereo_refine_params* params, float* stereo_out,
                             uint8_t* has_depth_out, uint8_t* status, int64_t* cost);

/* ------------------------------------------------------------------------------------------------
 * Stereo search - uR for a left keypoint by a 1-D patch search along its row of the rectified right image, over the whole disparity
 * range: no right-image extraction and no stereo matcher call are needed.  No reference counterpart: StereoFrontEnd::process extracts
 * both images and matches them (src/StereoFrontEnd.cc:14-47).  The rule is this library's own (the zero-mean SSD and the parabola of the
 * stereo refinement, with a texture gate, a uniqueness gate and a left-right check in front of the fit) and is stated here in full;
 * tests/_stereo_search_ref.py restates this text.  All of it is integer arithmetic on u8 pixels up to two fp64 compares, one fp64 division,
 * two fp64 subtractions and one rounding to fp32: the result does not depend on summation order, batch position or entry point.
 *
 * imgs_dev [2 * pairs, h, stride] u8, the L0, R0, L1, R1, ... layout: IL = image 2p, IR = image 2p + 1 of pair p.  stride is in bytes,
 * >= w; no alignment is required of the pointer or the stride.  kp_dev [units, max_keypoints, 3] f32 = (x, y, score) as an extractor
 * writes it and n_dev [units] i32; pair p reads unit p * unit_stride: unit_stride = 2 for the [2 * pairs] arrays of an extractor that ran
 * on both images, 1 for a left-only extraction.  The count n0 of pair p is n_dev[p * unit_stride] clamped to [0, max_keypoints] on the
 * device.  w = half_window, pw = 2w+1, N = pw^2, dlo = min_disparity, dhi = max_disparity (integers, pixels), W = the image width,
 * u = uniqueness, mt = min_texture, lr = lr_check.  Keypoint i of pair p, in this order:
 *   1. i >= n0: (0, quiet NaN, 0), has_depth 0, status NONE, cost -1 - the association's convention; every entry is written.
 *   2. x or y not finite or outside [0, 16384): status BORDER.  Otherwise, in fp64 on the fp32 value, xl = floor(x + 0.5),
 *      yl = floor(y + 0.5), and the status is BORDER unless xl-w >= 0, xl+w < W, yl-w >= 0 and yl+w < h.
 *   3. dmax = min(dhi, xl - w): the right patch at xl - d stays inside the image.  dmax - dlo + 1 < 3: status RANGE.
 *   4. Texture gate on the left patch A (the pixels IL[yl+dy, xl+dx], (dy, dx) in [-w, w]^2): T = N sum A^2 - (sum A)^2 in int64.  With
 *      mt > 0 and t = (double)mt (double)N:  (double)T < t t: status TEXTURE.
 *   5. For d = dlo .. dmax over (dy, dx) in [-w, w]^2:  e = IL[yl+dy, xl+dx] - IR[yl+dy, xl-d+dx];  S1 = sum e, S2 = sum e^2;
 *      C_d = N S2 - S1^2 in int64 - the refinement's cost; both patches lie on the left keypoint's row.
 *   6. d* = the smallest d attaining the minimum, cost = C_d*.  d* == dlo or d* == dmax: status EDGE.
 *   7. With max_rms > 0 and t = (double)max_rms (double)N:  (double)cost > t t: status COST.
 *   8. Uniqueness, with u > 0: C2 = min C_d over |d - d*| > 1.  If such a d exists and 100 cost < (100 - u) C2 does NOT hold (int64):
 *      status AMBIGUOUS.
 *   9. Left-right check, with lr >= 0: xr = xl - d*, emax = min(dhi, W - 1 - w - xr) (always >= d*).  For e = dlo .. emax, B_e is the
 *      same cost between the right patch at xr and the left patch at xr + e;  e* = the smallest e attaining the minimum.
 *      |e* - d*| > lr: status LRCHECK.
 *  10. den = C_{d*-1} + C_{d*+1} - 2 cost (>= 1, because d* is the smallest minimiser),
 *      delta = (double)(C_{d*-1} - C_{d*+1}) / (double)(2 den)  (|delta| <= 0.5),
 *      uR' = (float)(((double)x - (double)d*) - delta).  The patch is centred on xl, not on x, so a fractional x keeps its fraction.
 *      Status FOUND, output (x, uR', y) with the input's bits for x and y, has_depth 1.
 *  11. Every status other than FOUND writes (x, quiet NaN, y) with the input's bits, has_depth 0.  cost is -1 for NONE, BORDER, RANGE
 *      and TEXTURE and C_d* otherwise.
 * status_dev [pairs, max_keypoints] u8 and cost_dev [pairs, max_keypoints] i64 are optional (NULL = not wanted).  One launch,
 * asynchronous on `stream`, no host synchronisation.  pairs >= 1, max_keypoints in [1, 4096], h, w in [1, 16384], half_window in [1, 7],
 * 0 <= min_disparity <= max_disparity, max_disparity - min_disparity + 1 in [3, 512], uniqueness in [0, 99], lr_check in [-1, 16]
 * (-1: no check), min_texture and max_rms not NaN (<= 0: off), unit_stride 1 or 2; anything else, a NULL required pointer or
 * stride < w is SSHIP_ERR_INVALID before any device is touched.
 * ---------------------------------------------------------------------------------------------- */
#define SSHIP_SEARCH_STATUS_NONE 0
#define SSHIP_SEARCH_STATUS_FOUND 1
#define SSHIP_SEARCH_STATUS_BORDER 2
#define SSHIP_SEARCH_STATUS_RANGE 3
#define SSHIP_SEARCH_STATUS_TEXTURE 4
#define SSHIP_SEARCH_STATUS_EDGE 5
#define SSHIP_SEARCH_STATUS_COST 6
#define SSHIP_SEARCH_STATUS_AMBIGUOUS 7
#define SSHIP_SEARCH_STATUS_LRCHECK 8
typedef struct sship_stereo_search_params {
  int half_window;    /* w: the patch is (2w+1) x (2w+1) pixels; default 5 */
  int min_disparity;  /* dlo, pixels; default 0 */
  int max_disparity;  /* dhi, pixels; default 128 */
  int uniqueness;     /* u, percent: the best cost must be below (100 - u) % of the best one further than 1 px away; 0 is off; default 10 */
  float min_texture;  /* texture gate on the standard deviation of the left patch in grey levels; <= 0 is off (default 0) */
  float max_rms;      /* cost gate on the zero-mean RMS difference in grey levels; <= 0 is off (default 0) */
  int lr_check;       /* largest accepted |e* - d*| of the left-right check; -1 is off; default 1 */
} sship_stereo_search_params;
int sship_stereo_search_batch_device(const uint8_t* imgs_dev, int pairs, int h, int w, int stride, const float* kp_dev, const int* n_dev,
                                     int unit_stride, int max_keypoints, const sship_stereo_search_params* params, float* stereo_out_dev,
                                     uint8_t* has_depth_out_dev, uint8_t* status_dev, int64_t* cost_dev, void* stream);
/* One pair from host arrays: left / right [h, *_stride bytes] u8, keypoints[i * kp_stride + {0, 1}] = (x, y) with kp_stride >= 2, n in
 * [0, 4096] (0: nothing is touched); stereo_out [n, 3], has_depth_out [n]; status [n] and cost [n] are optional.  Synchronous. */
int sship_stereo_search_host(const uint8_t* left, int left_stride, const uint8_t* right, int right_stride, int h, int w,
                             const float* keypoints, int kp_stride, int n, const sship_stereo_search_params* params, float* stereo_out,
                             uint8_t* has_depth_out, uint8_t* status, int64_t* cost);

/* ------------------------------------------------------------------------------------------------
 * Patch tracking - the keypoints of a keyframe (or of the previous frame) carried into a new image by a bounded 2-D patch search: the
 * temporal twin of the stereo search.  With it a frame needs no network: track left to left, sship_stereo_search_batch_device at the
 * tracked positions (unit_stride 1), sship_pose_obs_from_matches_batch_device, sship_ransac_* / sship_pose_*; the extractor and the
 * matcher run on keyframes only.  No reference counterpart: StereoFrontEnd ties two frames by extracting both and matching them.  The rule
 * is this library's own (the zero-mean SSD of the stereo stages over a 2-D box, a texture gate, a uniqueness gate and a forward-backward
 * check in front of a parabola per axis) and is stated here in full; tests/_patch_track_ref.py restates this text.  All of it is integer
 * arithmetic on u8 pixels up to two fp64 compares, two fp64 divisions, four fp64 additions and two roundings to fp32: the result does not
 * depend on summation order, batch position or entry point.
 *
 * Image I0 of pair p is at imgs0_dev + p * image_stride0 (bytes) with rows of stride0 bytes, I1 at imgs1_dev + p * image_stride1 with
 * rows of stride1 bytes; both are h x W u8.  An image stride of 2 * h * stride reads the left images of an L0, R0, L1, R1, ... batch, an
 * image stride of 0 reads one image for every pair (a keyframe against many frames).  No alignment is required of any pointer or stride.
 * kp_dev [units, max_keypoints, 3] f32 = (x, y, score) as an extractor writes it and n_dev [units] i32; pair p reads unit p * unit_stride
 * (unit_stride 1 or 2).  The count n0 of pair p is n_dev[p * unit_stride] clamped to [0, max_keypoints] on the device.  pred_dev
 * [pairs, max_keypoints, 3] f32 is optional: (px, py, .) of row i is where the search for keypoint i is centred in I1; NULL means
 * (px, py) = (x, y).  pred_dev may be kp_out_dev: the output of one call seeds the next while the template stays the keyframe's.
 * w = half_window, pw = 2w+1, N = pw^2, R = search_radius, u = uniqueness, mt = min_texture, fb = fb_check.  Keypoint i of pair p, in
 * this order:
 *   1. i >= n0: kp_out (0, 0, 0), matches0 -1, status NONE, cost -1; every entry of every output is written.
 *   2. x, y, px or py not finite or outside [0, 16384): status BORDER.  Otherwise, in fp64 on the fp32 values, xa = floor(x + 0.5),
 *      ya = floor(y + 0.5), xp = floor(px + 0.5), yp = floor(py + 0.5), and the status is BORDER unless the template lies inside I0:
 *      xa-w >= 0, xa+w < W, ya-w >= 0 and ya+w < h.
 *   3. The search box, clipped so that every candidate patch lies inside I1: lox = max(-R, w - xp), hix = min(R, W-1-w-xp),
 *      loy = max(-R, w - yp), hiy = min(R, h-1-w-yp).  hix - lox + 1 < 3 or hiy - loy + 1 < 3: status RANGE.
 *   4. Texture gate on the template A (the pixels I0[ya+j, xa+i], (j, i) in [-w, w]^2): T = N sum A^2 - (sum A)^2 in int64.  With mt > 0
 *      and t = (double)mt (double)N:  (double)T < t t: status TEXTURE.
 *   5. For dy = loy .. hiy, dx = lox .. hix over (j, i) in [-w, w]^2:  e = I0[ya+j, xa+i] - I1[yp+dy+j, xp+dx+i];  S1 = sum e,
 *      S2 = sum e^2;  C(dx, dy) = N S2 - S1^2 in int64 - the stereo stages' cost.
 *   6. The candidates are ordered by k = (dy - loy)(hix - lox + 1) + (dx - lox).  (dx*, dy*) = the candidate of the smallest k attaining
 *      the minimum, cost = C(dx*, dy*).  dx* == lox, dx* == hix, dy* == loy or dy* == hiy: status EDGE.
 *   7. With max_rms > 0 and t = (double)max_rms (double)N:  (double)cost > t t: status COST.
 *   8. Uniqueness, with u > 0: C2 = min C(dx, dy) over the candidates with max(|dx - dx*|, |dy - dy*|) > 1.  If such a candidate exists
 *      and 100 cost < (100 - u) C2 does NOT hold (int64): status AMBIGUOUS.
 *   9. Forward-backward check, with fb >= 0: the template becomes the I1 patch at (xb, yb) = (xp + dx*, yp + dy*), and B(ex, ey) is the
 *      same cost between it and the I0 patch at (xa + dx* - ex, ya + dy* - ey), for (ex, ey) in [-R, R]^2 clipped so that the patch lies
 *      inside I0: elox = max(-R, xa + dx* - (W-1-w)), ehix = min(R, xa + dx* - w), and eloy, ehiy likewise with ya, dy* and h; the box
 *      always contains e = d*.  Order and smallest-index minimiser (ex*, ey*) as in step 6, with k = (ey - eloy)(ehix - elox + 1) +
 *      (ex - elox).  max(|ex* - dx*|, |ey* - dy*|) > fb: status FBCHECK.
 *  10. Fit, per axis: Cm = C(dx*-1, dy*), Cp = C(dx*+1, dy*) for x, Cm = C(dx*, dy*-1), Cp = C(dx*, dy*+1) for y;
 *      den = Cm + Cp - 2 cost (>= 1 on both axes: the left and the upper neighbour have a smaller k than the smallest minimiser),
 *      delta = (double)(Cm - Cp) / (double)(2 den)  (|delta| <= 0.5),
 *      x' = (float)(((double)x + (double)(xp - xa + dx*)) + delta_x), y' = (float)(((double)y + (double)(yp - ya + dy*)) + delta_y).
 *      The template is centred on (xa, ya), not on (x, y), so a fractional keypoint keeps its fraction.
 *      Status TRACKED: kp_out (x', y', the input's score bits), matches0 i.
 *  11. Every status other than TRACKED and NONE writes kp_out (quiet NaN, quiet NaN, the input's score bits) and matches0 -1.  cost is
 *      -1 for NONE, BORDER, RANGE and TEXTURE and C(dx*, dy*) otherwise.  A NaN row tracked again stays BORDER.
 * kp_out_dev [pairs, max_keypoints, 3] f32 and matches0_dev [pairs, max_keypoints] i32 have the shape of an extractor's and a matcher's
 * output for the new frame: sship_stereo_search_batch_device (unit_stride 1), sship_pose_obs_from_matches_batch_device and
 * sship_ba_tracks_from_matches_batch_device take them unchanged.  n_out_dev [pairs] i32 receives n0; it is optional, as are status_dev
 * [pairs, max_keypoints] u8 and cost_dev [pairs, max_keypoints] i64 (NULL = not wanted).  One launch, asynchronous on `stream`, no host
 * synchronisation.  pairs >= 1, max_keypoints in [1, 4096], h, w in [1, 16384], stride0 and stride1 >= w, image strides >= 0,
 * half_window in [1, 7], search_radius in [1, 16], uniqueness in [0, 99], fb_check in [-1, 16] (-1: no check), min_texture and max_rms
 * not NaN (<= 0: off), unit_stride 1 or 2; anything else or a NULL required pointer is SSHIP_ERR_INVALID before any device is touched.
 * ---------------------------------------------------------------------------------------------- */
#define SSHIP_TRACK_STATUS_NONE 0
#define SSHIP_TRACK_STATUS_TRACKED 1
#define SSHIP_TRACK_STATUS_BORDER 2
#define SSHIP_TRACK_STATUS_RANGE 3
#define SSHIP_TRACK_STATUS_TEXTURE 4
#define SSHIP_TRACK_STATUS_EDGE 5
#define SSHIP_TRACK_STATUS_COST 6
#define SSHIP_TRACK_STATUS_AMBIGUOUS 7
#define SSHIP_TRACK_STATUS_FBCHECK 8
typedef struct sship_patch_track_params {
  int half_window;    /* w: the patch is (2w+1) x (2w+1) pixels; 1 .. 7, default 5 */
  int search_radius;  /* R: displacements of up to R pixels per axis around the prediction are searched; 1 .. 16, default 8 */
  int uniqueness;     /* u, percent: the best cost must be below (100 - u) % of the best one further than 1 px away; 0 .. 99, 0 is off; default 10 */
  float min_texture;  /* texture gate on the standard deviation of the template in grey levels; <= 0 is off (default 0) */
  float max_rms;      /* cost gate on the zero-mean RMS difference in grey levels; <= 0 is off (default 0) */
  int fb_check;       /* largest accepted max(|ex* - dx*|, |ey* - dy*|) of the forward-backward check; -1 .. 16, -1 is off; default 1 */
} sship_patch_track_params;
int sship_patch_track_batch_device(const uint8_t* imgs0_dev, long long image_stride0, int stride0, const uint8_t* imgs1_dev,
                                   long long image_stride1, int stride1, int pairs, int h, int w, const float* kp_dev, const int* n_dev,
                                   int unit_stride, const float* pred_dev, int max_keypoints, const sship_patch_track_params* params,
                                   float* kp_out_dev, int* n_out_dev, int32_t* matches0_dev, uint8_t* status_dev, int64_t* cost_dev,
                                   void* stream);
/* One pair from host arrays: img0 / img1 [h, stride* bytes] u8, keypoints[i * kp_stride + {0, 1}] = (x, y) with kp_stride >= 2 (where
 * kp_stride >= 3 the third float is the score, else the score is 0), pred (optional) likewise with pred_stride >= 2, n in [0, 4096]
 * (0: nothing is touched); kp_out [n, 3], matches0 [n]; status [n] and cost [n] are optional.  Staged through one device block, the same
 * launch with pairs = 1: the same bits.  Synchronous. */
int sship_patch_track_host(const uint8_t* img0, int stride0, const uint8_t* img1, int stride1, int h, int w, const float* keypoints,
                           int kp_stride, const float* pred, int pred_stride, int n, const sship_patch_track_params* params, float* kp_out,
                           int32_t* matches0, uint8_t* status, int64_t* cost);

/* ------------------------------------------------------------------------------------------------
 * Image pyramid - a batch of u8 images reduced level by level on the device: the primitive under the coarse-to-fine tracker below, and a
 * source of half-, quarter-, ... resolution images for the other image stages (sship_stereo_search_batch_device on level 1 is
 * half-resolution depth at a quarter of the candidates).  The reduction rule is the one OpenCV documents for cv::pyrDown with its default
 * border; equality with cv::pyrDown is the intent, not a measured fact (OpenCV is on none of this project's machines), exactly as for the
 * rectification remap.  tests/_pyr_ref.py restates this text.  Integers only: the result does not depend on tiling, batch position or
 * entry point.
 *   Level l+1 of a level of h x w pixels S has h' = (h + 1) / 2 rows and w' = (w + 1) / 2 columns (integer division), and
 *     D(y, x) = (sum over j, i in -2 .. 2 of k_j k_i S(r(2y + j, h), r(2x + i, w)) + 128) >> 8,   k = (1, 4, 6, 4, 1),
 *   where r is reflect-101: r(i, 1) = 0; otherwise i < 0 becomes -i and i >= n becomes 2 (n - 1) - i, repeated until 0 <= i < n.
 *   The weights sum to 256; the largest accumulator is 255 * 256 = 65 280.
 * A handle is made for one image size, `levels` levels (1 .. 8, level 0 counted) and at most max_images (1 .. 65 535) images.  It owns the
 * storage of levels 1 and above: level l holds max_images images of lh x lw pixels in rows of pitch_l = lw rounded up to 64 bytes, image
 * i at i * pitch_l * lh bytes from the level's base, every level's base on 256 bytes; the bytes of a row past lw are zero.  Nothing is
 * allocated after sship_pyr_create.  Level 0 is the caller's memory, borrowed, never copied: a byte pointer, a row stride >= w and an
 * image stride >= 0, all in bytes, no alignment required (an image stride of 2 * h * stride picks the left images of an L0, R0, L1, R1,
 * ... batch).  It must stay valid and unchanged until the next build or sship_pyr_destroy: sship_pyr_level(0) and the tracker read it.
 * sship_pyr_build_batch_device reduces images [0, images) (images <= max_images; a later build may hold fewer) with one launch per level,
 * asynchronous on `stream`, no host synchronisation.  sship_pyr_level describes a level of the last build (every output pointer is
 * optional): with it sship_patch_track_batch_device, sship_stereo_search_batch_device (where the stride fits its int) and any other
 * consumer of (pointer, strides) run on any level.  sship_pyr_read_level copies images [first, first + count) of a level to the host in rows
 * of out_stride >= lw bytes, image after image (synchronous; it waits for the device).  sship_pyr_down_host is one image and one reduction
 * from host arrays, staged through one device block - the drop-in for one cv::pyrDown; dst is ((h + 1) / 2) x ((w + 1) / 2) in rows of
 * dst_stride bytes.  sship_pyr_bench re-runs the last build's launches `iters` times on the handle's stream (*avg_ms per build).
 * A NULL required pointer, h or w outside [1, 16384], levels outside [1, 8], max_images outside [1, 65535], images outside
 * [1, max_images], stride < w, a negative image stride, a level outside [0, levels), images outside the last build, or a level asked for
 * before the first build is SSHIP_ERR_INVALID before any device is touched.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_pyr sship_pyr;
int sship_pyr_create(int h, int w, int levels, int max_images, sship_pyr** out);
void sship_pyr_destroy(sship_pyr* pyr);
int sship_pyr_build_batch_device(sship_pyr* pyr, const uint8_t* imgs_dev, long long image_stride, int stride, int images, void* stream);
int sship_pyr_level(const sship_pyr* pyr, int level, const uint8_t** ptr, int* h, int* w, int* stride, long long* image_stride, int* images);
int sship_pyr_read_level(const sship_pyr* pyr, int level, int first, int count, uint8_t* out_host, int out_stride);
int sship_pyr_down_host(const uint8_t* src, int src_stride, int h, int w, uint8_t* dst, int dst_stride);
int sship_pyr_bench(sship_pyr* pyr, int iters, float* avg_ms);

/* ------------------------------------------------------------------------------------------------
 * Coarse-to-fine patch tracking - the patch-tracking rule above run on the levels of two image pyramids from the top down, each level's
 * result centring the search of the next: the reach grows to roughly (coarse_radius - 1) * 2^(L-1) pixels per axis around the prediction
 * (plus the fine radius) while every level searches a small box.  tests/_pyr_track_ref.py restates this text on top of
 * tests/_patch_track_ref.py.
 * Pair p reads image first0 + p * step0 of pyr0 as I0 and image first1 + p * step1 of pyr1 as I1 (a step of 0: one keyframe for every
 * pair; pyr0 == pyr1 is allowed, e.g. P + 1 consecutive frames built once and first1 = first0 + 1).  The indices must lie inside the last
 * build of each pyramid; both pyramids must have the same h and w and at least params.levels levels.  kp_dev, n_dev, unit_stride,
 * pred_dev, max_keypoints and the outputs are those of sship_patch_track_batch_device; pred_dev may be kp_out_dev.
 * L = levels, I0_l / I1_l = level l of the two images.  Keypoint i of pair p with (x, y) and the prediction (px, py) (= (x, y) without
 * pred_dev):
 *   1. i >= n0: the outputs of step 1 of the patch-tracking rule, levels_tracked 0.
 *   2. The top level t = L - 1 starts from p_t = ((float)((double)px 2^-t), (float)((double)py 2^-t)).
 *   3. Each level l = t, t - 1, ..., 1 applies steps 2 to 10 of the patch-tracking rule to I0_l and I1_l, the keypoint
 *      ((float)((double)x 2^-l), (float)((double)y 2^-l)) - the product formed in fp64, rounded once - and the prediction p_l, with
 *      half_window and uniqueness of `fine`, search_radius = coarse_radius, and the texture gate, the cost gate and the forward-backward
 *      check off.
 *   4. Status TRACKED with the fp32 output (x', y'): p_(l-1) = (2 x', 2 y').  Any other status: p_(l-1) = 2 p_l.  Both doublings are exact.
 *      A coarse failure (a template that does not fit the small level, a minimiser on the box's edge, a periodic texture, a box that
 *      leaves the image) is therefore not fatal: the prediction is carried down unchanged and the finer levels search around it.
 *   5. Level 0 is the patch-tracking rule with the original (x, y), the prediction p_0 and all of `fine`; its outputs are the call's
 *      kp_out, matches0, status and cost.
 *   6. levels_tracked_dev [pairs, max_keypoints] u8 (optional): bit l is set when level l ended TRACKED.
 *   7. levels == 1 gives exactly the bits of sship_patch_track_batch_device.
 * One launch, asynchronous on `stream`, no host synchronisation.  levels in [1, 8], coarse_radius in [1, 16], `fine` as
 * sship_patch_track_params, first and step >= 0, pairs >= 1, max_keypoints in [1, 4096], unit_stride 1 or 2; anything else, a NULL
 * required pointer, unequal pyramids, too few levels, a pyramid that was never built or an image index outside the last build is
 * SSHIP_ERR_INVALID before any device is touched.  sship_patch_track_pyramid_host is one pair from host arrays (arguments as
 * sship_patch_track_host, levels_tracked [n] optional): both images are staged in one device block, a two-image pyramid is built for the
 * call, and the same launch runs with pairs = 1 - the same bits.  Synchronous.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_pyr_track_params {
  sship_patch_track_params fine;  /* level 0: every field as in sship_patch_track_batch_device */
  int levels;                     /* L: levels walked, level 0 counted; 1 .. 8, default 3 */
  int coarse_radius;              /* search radius of the levels above 0; 1 .. 16, default 8 */
} sship_pyr_track_params;
int sship_patch_track_pyramid_batch_device(const sship_pyr* pyr0, int first0, int step0, const sship_pyr* pyr1, int first1, int step1,
                                           int pairs, const float* kp_dev, const int* n_dev, int unit_stride, const float* pred_dev,
                                           int max_keypoints, const sship_pyr_track_params* params, float* kp_out_dev, int* n_out_dev,
                                           int32_t* matches0_dev, uint8_t* status_dev, int64_t* cost_dev, uint8_t* levels_tracked_dev,
                                           void* stream);
int sship_patch_track_pyramid_host(const uint8_t* img0, int stride0, const uint8_t* img1, int stride1, int h, int w, const float* keypoints,
                                   int kp_stride, const float* pred, int pred_stride, int n, const sship_pyr_track_params* params,
                                   float* kp_out, int32_t* matches0, uint8_t* status, int64_t* cost, uint8_t* levels_tracked);

/* ------------------------------------------------------------------------------------------------
 * CLAHE - contrast-limited adaptive histogram equalisation of a batch of u8 images on the device: the stage in front of the patch
 * trackers and the stereo search above, whose zero-mean SSD cost forgives a brightness offset and nothing else (a gain between the two
 * cameras, or between two frames of an auto-exposure camera, is paid in accuracy).  VINS-Mono / VINS-Fusion (`equalize: 1`) and OpenVINS
 * (`histogram_method: CLAHE`) equalise in front of their trackers; here the image stays on the device.  The rule is modelled on OpenCV's
 * 8-bit cv::CLAHE; equality with cv::CLAHE is the intent, not a measured fact (OpenCV is on none of this project's machines), exactly as
 * for the rectification remap and cv::pyrDown.  tests/_clahe_ref.py restates this text.  Integers plus a handful of fp32 operations that
 * are each rounded once (round to nearest even, no fused multiply-add): an image has the same bits alone, at any position of any batch,
 * at any pointer alignment or stride, and on the host entry.
 *   Parameters: tiles_x, tiles_y in 1 .. 16; clip_limit fp64, finite, >= 0 (0: no clipping).  S is the h x w source, h, w <= 16384.
 *   Extension.  If w % tiles_x == 0 and h % tiles_y == 0: (ew, eh) = (w, h).  Otherwise ew = w + (tiles_x - w % tiles_x) and
 *     eh = h + (tiles_y - h % tiles_y) - an axis that already divides grows by a whole `tiles` pixels when the other does not divide
 *     (OpenCV's behaviour, kept).  E(y, x) = S(r(y, h), r(x, w)) with reflect-101: r(i, n) = i for i < n, else 2 (n - 1) - i.  The call is
 *     refused unless ew - w <= w - 1 and eh - h <= h - 1 (one reflection lands inside).
 *   Tiles.  tw = ew / tiles_x, th = eh / tiles_y, A = tw th; refused unless A <= 2^24, so that every partial sum is an exact fp32.
 *   Limit.  clip_limit > 0: L = min(A, max(1, trunc((clip_limit * A) / 256))), product and quotient in fp64.  Otherwise no clipping.
 *   Histogram of tile (j, i): the 256 counts hist[v] of E over rows [j th, (j + 1) th) and columns [i tw, (i + 1) tw).
 *   Clip (with a limit only).  clipped = sum over v of max(hist[v] - L, 0); hist[v] = min(hist[v], L); batch = clipped / 256 and
 *     residual = clipped % 256 (integers); every bin += batch; if residual > 0: step = max(256 / residual, 1) (integer) and the bins
 *     0, step, 2 step, ... each += 1, stopping after `residual` bins or at bin 256, whichever comes first (always `residual` bins: the
 *     histogram still sums to A).
 *   Table.  s_v = hist[0] + ... + hist[v]; lut[v] = sat_u8(rint((float)s_v * scale)), scale = 255.f / (float)A (one fp32 division).
 *   Output pixel (y, x), v = S(y, x):
 *     txf = (float)x * inv_tw - 0.5f, inv_tw = 1.f / (float)tw;  t1 = floor(txf);  xa = txf - (float)t1;  xa1 = 1.f - xa;
 *     tx2 = min(t1 + 1, tiles_x - 1);  tx1 = max(t1, 0);  the same in y with inv_th = 1.f / (float)th: ty1, ty2, ya, ya1;
 *     res = (lut[ty1][tx1][v] xa1 + lut[ty1][tx2][v] xa) ya1 + (lut[ty2][tx1][v] xa1 + lut[ty2][tx2][v] xa) ya,
 *     the table entries converted to fp32, every product and every sum rounded once to fp32 in exactly this association;
 *     D(y, x) = sat_u8(rint(res)).  Exact halves are common (thousands per EuRoC-sized image): the rounding mode matters.
 *   scale, inv_tw, inv_th and L are formed on the host and passed to the kernels by value: no device division enters the rule.
 * A handle is made for one image size, one tile grid and at most max_images (1 .. 65 535) images; it owns the table workspace
 * [max_images, tiles_y, tiles_x, 256] u8, and nothing is allocated after sship_clahe_create.  sship_clahe_set_clip_limit changes the
 * limit for the calls that follow; sship_clahe_get_params reads the handle back (every output pointer is optional).
 * sship_clahe_apply_batch_device equalises images [0, images): image i is read at src_dev + i * src_image_stride in rows of src_stride
 * bytes and written at dst_dev + i * dst_image_stride in rows of dst_stride bytes, all strides in bytes, row strides >= w, image strides
 * >= 0, no alignment asked of pointers or strides (src_image_stride = 2 * h * stride reads the left images of an L0, R0, L1, R1, ...
 * batch).  dst_dev == src_dev with equal strides is allowed (in place); any other overlap of source and destination is undefined.  Two
 * launches (tables, then pixels), asynchronous on `stream`, no host synchronisation; every destination pixel is written and nothing
 * outside w bytes of a row.  sship_clahe_read_luts copies the tables of images [first, first + count) of the last call to the host,
 * [count, tiles_y, tiles_x, 256] u8 (synchronous; it waits for the device).  sship_clahe_apply_host is one image from host arrays,
 * staged through one device block - the drop-in for one cv::CLAHE::apply; the same two launches with images = 1, hence the same bits.
 * sship_clahe_bench re-runs the last call's two launches `iters` times on the handle's stream (*avg_ms per call; an in-place call is
 * re-run on its own output); sship_clahe_bench_kernels the chosen ones (1: the tables, 2: the pixels, 3: both).
 * A NULL required pointer, h or w outside [1, 16384], tiles outside [1, 16], either extension condition, A > 2^24, a negative or
 * non-finite clip limit, max_images outside [1, 65535], images outside [1, max_images], a row stride < w, a negative image stride, or
 * tables asked for before the first call is SSHIP_ERR_INVALID before any device is touched; valid create arguments without a GPU are
 * SSHIP_ERR_NO_DEVICE.  Not wired into sship_frontend_batch_device; 8-bit images only.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_clahe sship_clahe;
int sship_clahe_create(int h, int w, int tiles_x, int tiles_y, double clip_limit, int max_images, sship_clahe** out);
void sship_clahe_destroy(sship_clahe* clahe);
int sship_clahe_set_clip_limit(sship_clahe* clahe, double clip_limit);
int sship_clahe_get_params(const sship_clahe* clahe, int* h, int* w, int* tiles_x, int* tiles_y, double* clip_limit, int* max_images);
int sship_clahe_apply_batch_device(sship_clahe* clahe, const uint8_t* src_dev, long long src_image_stride, int src_stride, uint8_t* dst_dev,
                                   long long dst_image_stride, int dst_stride, int images, void* stream);
int sship_clahe_read_luts(const sship_clahe* clahe, int first, int count, uint8_t* out_host);
int sship_clahe_apply_host(const uint8_t* src, int src_stride, int h, int w, int tiles_x, int tiles_y, double clip_limit, uint8_t* dst,
                           int dst_stride);
int sship_clahe_bench(sship_clahe* clahe, int iters, float* avg_ms);
int sship_clahe_bench_kernels(sship_clahe* clahe, int kernels, int iters, float* avg_ms);

/* ------------------------------------------------------------------------------------------------
 * FAST corners - a corner detector with track refill on the device: the one stage of the no-network chain that CREATES keypoints
 * (detect -> patch tracker -> stereo search -> RANSAC -> pose needs no checkpoint with it), and the classical baseline of the extractor.
 * VINS-Fusion and OpenVINS re-detect corners outside a mask around their live tracks and append them to the track list; this does the
 * same without leaving the device.  The rule is modelled on FAST-9/16 (Rosten and Drummond) as OpenCV's cv::FAST implements it.
 * Equality with OpenCV is NOT claimed: points 2 and 3 differ from it on purpose.  Everything is integer arithmetic on u8 pixels and
 * comparison of distinct 64-bit keys: the kernels equal the numpy restatement (tests/_fast_ref.py) bit for bit.
 * The rule.  Image I is u8, h x W; parameters t = threshold in [0, 254], b = border in [3, 64], d = min_distance in [0, 32].
 *   1. Score.  Ring offsets (dx, dy), k = 0..15, clockwise from the top: (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3)
 *      (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3).  For 3 <= x < W-3 and 3 <= y < h-3: e_k = I[y+dy_k, x+dx_k] - I[y, x] (int32),
 *      bright = max over a in 0..15 of min over j in 0..8 of e_{(a+j) mod 16}, dark the same with -e, s(x, y) = max(bright, dark, 0);
 *      elsewhere s = 0.  s lies in 0..255 and is the largest t' such that 9 contiguous ring pixels all differ from the centre by at
 *      least t' in one direction: OpenCV's score plus one.
 *   2. Corner and non-maximum suppression.  A pixel is a candidate iff s > t, it lies inside the border (b <= x < W-b, b <= y < h-b) and
 *      the triple (s, y, x) is lexicographically greater than (s_q, y_q, x_q) of each of its 8 neighbours q: a plateau keeps its last
 *      pixel in raster order.  (OpenCV's strict > drops whole plateaus: a clean synthetic step corner has three equal scores in a row,
 *      and OpenCV returns nothing for it.)  This is the order the selection sorts by.  Two candidates are never 8-neighbours, so an
 *      image has at most ceil(h/2) * ceil(W/2) candidates; the handle sizes its candidate list to that bound, the list cannot
 *      overflow, and the result therefore cannot depend on the order the slot-reservation atomics resolve in.
 *   3. Mask.  keep is [units, max_keypoints, 3] f32 with counts keep_n clamped to [0, max_keypoints] on the device; image p reads unit
 *      p * unit_stride (1 or 2), as the patch tracker does.  Row i < n_keep is LIVE iff x and y are finite and in [0, 16384).  For a
 *      live row xa = floor(x + 0.5), ya = floor(y + 0.5) in fp64 (the tracker's step 2).  With d > 0 and keep given, a candidate at
 *      (cx, cy) with max(|cx - xa|, |cy - ya|) < d for any live row is removed.  The mask is applied after step 2: a masked pixel still
 *      suppresses its neighbours.  M is the number of candidates left.
 *   4. Selection.  The existing rule, unchanged, on the M keys (bits((float)s) << 32) | (cy * W + cx) with scale 1: SSHIP_SELECT_TOPK
 *      takes the first K = min(M, max_new) in descending (s, y, x) order; SSHIP_SELECT_BALANCED with bucket_px is the rule stated at
 *      sship_sp_set_keypoint_selection, written in the default mode's order.  A new keypoint is ((float)cx, (float)cy, (float)s).
 *   5. Merge.  L is the number of live rows (0 without keep).  The live rows are written first to kp_out, in input order, all three
 *      floats bit for bit; carry0[i] is the output row of input row i, -1 for dead rows and rows at or beyond n_keep.  Then the first
 *      A = min(K, max_keypoints - L, target > 0 ? max(0, target - L) : K) selected keypoints are appended; n_out = L + A; rows at or
 *      beyond n_out are (0, 0, 0).  Every entry of every output is written.  carry0 has the shape and meaning of a matcher's matches0
 *      between the old list and the new one: sship_ba_tracks_from_matches_batch_device and sship_pose_obs_from_matches_batch_device
 *      take it unchanged.  In balanced mode with a target that truncates, the kept rows are a score-ordered prefix of the balanced set
 *      (the K selected keys are emitted in descending key order, and the first A of them are appended), not the balanced set of size A.
 * sship_fast_params: threshold (default 20), border (8), min_distance (10), selection (SSHIP_SELECT_TOPK), bucket_px (32; read in
 * balanced mode only, [8, 65535]), max_new in [1, max_keypoints] (default max_keypoints), target >= 0 (0 = off).  sship_fast_create: h
 * and w in [7, 16384], max_keypoints in [1, 4096], max_images in [1, 65535]; every workspace (the key list of 8 bytes per candidate of
 * the bound, the balanced rule's workspace, the selected keypoints - per image) is allocated here and nothing later; the mask needs
 * none (k_fast_detect builds its tile's part of it in LDS from the keep rows, by OR, so it does not depend on execution order).  sship_fast_detect_batch_device: imgs_dev holds `images` <= max_images images, image i at imgs_dev + i *
 * image_stride, rows `stride` bytes apart (>= w), image_stride >= 0, no alignment asked (image_stride = 2 * h * stride reads the left
 * images of an L0, R0, ... batch).  keep_dev may be NULL (no live rows, no mask; keep_n_dev and unit_stride are then ignored); given,
 * keep_n_dev is required and keep_dev must not overlap kp_out_dev (refused).  kp_out_dev [images, max_keypoints, 3] f32, n_out_dev
 * [images] i32, carry0_dev [images, max_keypoints] i32 or NULL, n_candidates_dev [images] i32 (M) or NULL.  Asynchronous on `stream`,
 * no host synchronisation: one memset node (the candidate counters), k_fast_detect, k_select_balanced (that mode only), k_topk,
 * k_fast_merge.  sship_fast_detect_host is one image from host arrays (keep rows keep_stride >= 3 floats apart, n_keep
 * in [0, max_keypoints]; kp_out [max_keypoints, 3], carry0 [max_keypoints] or NULL), staged through one device block: the same launches
 * with images = 1, hence the same bits.  sship_fast_score_batch_device is the stage form of step 1 alone and needs no handle: the u8
 * score map of every image with caller strides.  sship_fast_bench re-runs the last call's launches `iters` times on the handle's
 * stream; sship_fast_bench_kernels the chosen ones (bit 0 k_fast_detect, 1 the selection, 2 k_fast_merge; 1 .. 7).
 * Every bad argument is SSHIP_ERR_INVALID before any device is touched; valid create arguments without a GPU are SSHIP_ERR_NO_DEVICE.
 * Not wired into sship_frontend_batch_device, bench.py or examples/frontend_benchmark.cc; 8-bit images only.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_fast sship_fast;
typedef struct sship_fast_params {
  int threshold, border, min_distance, selection, bucket_px, max_new, target;
} sship_fast_params;
int sship_fast_create(int h, int w, int max_keypoints, int max_images, sship_fast** out);
void sship_fast_destroy(sship_fast* fast);
int sship_fast_set_params(sship_fast* fast, const sship_fast_params* params);
int sship_fast_get_params(const sship_fast* fast, sship_fast_params* params, int* h, int* w, int* max_keypoints, int* max_images);
int sship_fast_detect_batch_device(sship_fast* fast, const uint8_t* imgs_dev, long long image_stride, int stride, int images,
                                   const float* keep_dev, const int* keep_n_dev, int unit_stride, float* kp_out_dev, int* n_out_dev,
                                   int32_t* carry0_dev, int* n_candidates_dev, void* stream);
int sship_fast_detect_host(const uint8_t* img, int stride, int h, int w, int max_keypoints, const sship_fast_params* params,
                           const float* keep, int keep_stride, int n_keep, float* kp_out, int* n_out, int32_t* carry0,
                           int* n_candidates);
int sship_fast_score_batch_device(const uint8_t* imgs_dev, long long image_stride, int stride, int images, int h, int w, uint8_t* score_dev,
                                  long long score_image_stride, int score_stride, void* stream);
int sship_fast_bench(sship_fast* fast, int iters, float* avg_ms);
int sship_fast_bench_kernels(sship_fast* fast, int kernels, int iters, float* avg_ms);

/* ------------------------------------------------------------------------------------------------
 * Binary descriptors - steered BRIEF at given keypoints: the stage that lets the no-network chain RECOGNISE a point (re-acquire a lost
 * track, match a keyframe against a loop candidate of sship_index_*, associate left and right corner lists by appearance).  Modelled on
 * ORB's rBRIEF (Rublee et al.).  Equality with OpenCV is NOT claimed: the pattern is this library's own, generated by the rule below, not
 * OpenCV's learned table.  Integers and comparisons throughout: the kernel equals the numpy restatement (tests/_brief_ref.py) bit for
 * bit.  Stateless, like sship_patch_track_*.
 * The rule.  Image I is u8, h x W.  A descriptor is 256 bits in 8 u32 words; bit t is stored in word t >> 5 at position t & 31.
 *   Tables.  For k = 0..31, C[k] = rint(16384 cos(2 pi k / 32)):
 *      C = 16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, -11585, -13623, -15137, -16069,
 *          -16384, -16069, -15137, -13623, -11585, -9102, -6270, -3196, 0, 3196, 6270, 9102, 11585, 13623, 15137, 16069
 *      and S[k] = C[(k + 24) % 32] (the sine).  C[k+8] = -S[k] and S[k+8] = C[k] exactly (indices mod 32).
 *   Pattern.  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (mod 2^32; the RANSAC sampler's mix).
 *      v(c) = mix(mix(1 + 0x9e3779b9 * (c + 1))), coord(c) = v % 8 + (v >> 8) % 8 + (v >> 16) % 7 - 10, in [-10, 10].  Test t takes four
 *      consecutive counters as (ax, ay, bx, by); a draw with (ax, ay) == (bx, by) is discarded and the next four counters are used
 *      (the first 1024 counters give the 256 tests; none is discarded).  For bin k a point (x, y) becomes (rd(x C[k] - y S[k]),
 *      rd(x S[k] + y C[k])) with rd(v) = sgn(v) * ((|v| + 8192) >> 14): symmetric about zero, so that the table of bin k + 8 is the table
 *      of bin k turned by 90 degrees exactly (floor rounding would break that).  Every rotated coordinate has |.| <= 14; the reach is
 *      E = 16: 14 plus the box half-width 2, and not less than the moment radius 15.  sship_brief_pattern(bin, out[256 * 4]) returns the
 *      rotated table of a bin as int8 (ax', ay', bx', by') rows: pure host, no GPU.
 *   Keypoint i of image p is row i of unit p * unit_stride (1 or 2) of kp [units, max_keypoints, 3] f32 with counts n [units], as FAST
 *      reads keep.  If i >= n (n clamped to [0, max_keypoints] on the device) the status is NONE.  Otherwise, if x or y is not finite or
 *      lies outside [0, 16384), BORDER.  Otherwise xa = floor(x + 0.5), ya = floor(y + 0.5) in fp64 (the tracker's step 2), and the status
 *      is BORDER unless xa - 16 >= 0, xa + 16 < W, ya - 16 >= 0 and ya + 16 < h; else OK.
 *   Orientation (SSHIP_BRIEF_STEERED).  Over the disc dx^2 + dy^2 <= 225: m10 = sum dx I[ya+dy, xa+dx], m01 = sum dy I[ya+dy, xa+dx]
 *      (both fit int32).  bin = the smallest k attaining max over k of (m10 C[k] + m01 S[k]), in int64; a flat patch gives bin 0.  With
 *      SSHIP_BRIEF_UPRIGHT bin = 0 and no moments are computed.
 *   Bits.  B(x, y) is the sum of the 5 x 5 box of I centred on (x, y).  With (ax', ay', bx', by') the bin's rotated test t,
 *      bit t = B(xa + ax', ya + ay') < B(xa + bx', ya + by').
 *   Outputs.  desc [images, max_keypoints, 8] u32, all zero for every status other than OK; status u8 (optional): SSHIP_BRIEF_NONE 0,
 *      SSHIP_BRIEF_OK 1, SSHIP_BRIEF_BORDER 2; bin u8 (optional): 0 where the status is not OK.  Every entry of every output is written.
 * sship_brief_describe_batch_device: image i at imgs_dev + i * image_stride in rows of `stride` bytes (>= w), image_stride >= 0, no
 * alignment asked (image_stride = 2 * h * stride reads the left images of an L0, R0, ... batch); images in [1, 65535], max_keypoints in
 * [1, 4096], h and w in [33, 16384], unit_stride 1 or 2, mode SSHIP_BRIEF_STEERED or SSHIP_BRIEF_UPRIGHT.  One launch (k_brief_describe),
 * no host synchronisation.  sship_brief_describe_host is one image from host arrays (n rows kp_stride >= 2 floats apart, n in [0, 4096];
 * desc [n, 8], status [n] or NULL, bin [n] or NULL), staged through one device block: the same launch with images = 1 and max_keypoints =
 * n, hence the same bits.  Every bad argument is SSHIP_ERR_INVALID before any device is touched.
 *
 * Hamming matcher (sship_hm_*) - mutual nearest neighbour over such descriptors.  A handle whose workspace is sized at create, like
 * sship_nn_*.  The rule.  Sets d0 [n0, 8] and d1 [n1, 8] u32 with optional per-row status and, when the handle's gate is on, keypoints.
 * Entry (i, j) is PRESENT iff i < n0 and j < n1, both statuses are SSHIP_BRIEF_OK where a status array is given, and the gate admits it
 * where the gate is on.  The gate is sship_nn_set_gate's rule and form: with dx = x0_i - x1_j and dy = y0_i - y1_j in fp32, the entry is
 * admitted iff dx >= dx_lo && dx <= dx_hi && dy >= dy_lo && dy <= dy_hi (a NaN coordinate is in no window; infinite bounds are allowed;
 * the open gate gives the ungated bits).  Per row i: D_ij = sum over the 8 words of popcount(d0[i] ^ d1[j]); j1 is the smallest present j
 * of the minimum and e1 that minimum; e2 is the minimum over the other present entries, absent when fewer than two are present;
 * pass = (max_distance == 0 || e1 <= max_distance) && (ratio_percent == 0 || e2 absent || 100 e1 <= ratio_percent e2), in integers;
 * fwd_i = pass ? j1 : -1; a row with no present entry gives -1.  Columns follow the same rule (bwd).  matches0_i = fwd_i if fwd_i >= 0 and
 * (!mutual_check || bwd[fwd_i] == i), else -1; dist0_i = e1 when matched, else -1; the optional mscores0_i = (256 - e1) / 256 as f32 when
 * matched (exact), else 0 - with it sship_filter_matches yields distance = e1 / 256.  Rows >= n0 are -1 / -1 / 0.  A pair's result does
 * not depend on the other pairs of the call or on its position; no kernel has an atomic.
 * Defaults: max_distance 0 (off; 0..256), ratio_percent 0 (off; 0..100), mutual_check on, gate off.
 * sship_hm_create(max_keypoints 1..4096, max_pairs 1..65535): everything is allocated here and nothing later.
 * sship_hm_match_batch_device: n_dev [units] i32 (clamped to [0, max_keypoints] on the device), desc_dev [units, max_keypoints, 8] u32
 * (16-byte aligned), status_dev [units, max_keypoints] u8 or NULL, kp_dev [units, max_keypoints, 3] f32 (NULL unless gated; a gated
 * handle called without it is refused).  Set 0 of pair p is unit first0 + p * step0, set 1 is unit first1 + p * step1 (the pyramid
 * tracker's first / step convention; firsts and steps >= 0): (0, 2, 1, 2) is the stereo layout, (0, 1, 1, 1) consecutive frames,
 * (0, 0, 1, 1) one keyframe against many.  matches0_dev, dist0_dev [pairs, max_keypoints] i32, mscores0_dev [pairs, max_keypoints] f32 or
 * NULL.  Asynchronous on `stream`, no host synchronisation: k_hm_best, then k_hm_final.  matches0 has the shape and meaning of every
 * matcher's here: sship_stereo_associate_batch_device, sship_pose_obs_from_matches_batch_device and
 * sship_ba_tracks_from_matches_batch_device take it unchanged.  sship_hm_match_host is one pair from host arrays (n0, n1 in [0,
 * max_keypoints]; status0 / status1 may be NULL; kp0 / kp1 rows kp_stride >= 2 floats apart, read only when gated; outputs [n0]) through
 * the handle's staging arena: the same launches.  sship_hm_bench re-runs the last call's launches `iters` times on the handle's stream.
 * Not wired into sship_frontend_batch_device, bench.py or examples/frontend_benchmark.cc.
 * ---------------------------------------------------------------------------------------------- */
enum { SSHIP_BRIEF_STEERED = 0, SSHIP_BRIEF_UPRIGHT = 1 };
enum { SSHIP_BRIEF_NONE = 0, SSHIP_BRIEF_OK = 1, SSHIP_BRIEF_BORDER = 2 };
int sship_brief_pattern(int bin, int8_t* out_256x4);
int sship_brief_describe_batch_device(const uint8_t* imgs_dev, long long image_stride, int stride, int images, int h, int w,
                                      const float* kp_dev, const int* n_dev, int unit_stride, int max_keypoints, int mode,
                                      uint32_t* desc_dev, uint8_t* status_dev, uint8_t* bin_dev, void* stream);
int sship_brief_describe_host(const uint8_t* img, int stride, int h, int w, const float* keypoints, int kp_stride, int n, int mode,
                              uint32_t* desc, uint8_t* status, uint8_t* bin);
typedef struct sship_hm sship_hm;
int sship_hm_create(int max_keypoints, int max_pairs, sship_hm** out);
void sship_hm_destroy(sship_hm* hm);
int sship_hm_set_params(sship_hm* hm, int max_distance, int ratio_percent, int mutual_check);
int sship_hm_get_params(const sship_hm* hm, int* max_distance, int* ratio_percent, int* mutual_check, int* max_keypoints, int* max_pairs);
int sship_hm_set_gate(sship_hm* hm, int enabled, float dx_lo, float dx_hi, float dy_lo, float dy_hi);
int sship_hm_get_gate(const sship_hm* hm, int* enabled, float* dx_lo, float* dx_hi, float* dy_lo, float* dy_hi);
int sship_hm_match_batch_device(sship_hm* hm, const int* n_dev, const uint32_t* desc_dev, const uint8_t* status_dev, const float* kp_dev,
                                int first0, int step0, int first1, int step1, int pairs, int32_t* matches0_dev, int32_t* dist0_dev,
                                float* mscores0_dev, void* stream);
int sship_hm_match_host(sship_hm* hm, int n0, const uint32_t* desc0, const uint8_t* status0, const float* kp0, int kp_stride0, int n1,
                        const uint32_t* desc1, const uint8_t* status1, const float* kp1, int kp_stride1, int32_t* matches0,
                        int32_t* dist0, float* mscores0);
int sship_hm_bench(sship_hm* hm, int iters, float* avg_ms);

/* ------------------------------------------------------------------------------------------------
 * Fused front-end step: what StereoFrontEnd::process asks of the two interfaces per frame
 * (src/StereoFrontEnd.cc:14,33): SuperPoint on L and R (one batch) + gather x2 + one LightGlue match,
 * for `pairs` stereo pairs at once, device-resident, no host synchronisation.  imgs_dev is
 * [2*pairs, h, w] u8 ordered L0, R0, L1, R1, ...  Output shapes as in the two batch calls above.
 * ---------------------------------------------------------------------------------------------- */
int sship_frontend_batch_device(sship_sp* sp, sship_lg* lg, const uint8_t* imgs_dev, int pairs, int h, int w,
                                void* desc_out_dev, float* kp_out_dev, int* n_out_dev,
                                int32_t* matches0_dev, float* mscores0_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU exchange (BASELINE configs 3 and 5).  No reference counterpart: the reference is single-GPU.
 * Frames / pairs / cameras are sharded over one process per GPU with replicated weights and NO data-path collective; the
 * one exchange step is a fixed-stride all-gather of every rank's padded results into the image of the shared
 * DescriptorPool (include/DescriptorPool.h:13-91: [count, 256] fp16 rows per frame) on every rank.  RCCL (xGMI) is bound
 * at run time; without it these calls return SSHIP_ERR_NO_DEVICE and the rest of the library is unaffected.
 *   rank 0:      sship_comm_unique_id(id)  ->  hand the 128 bytes to the other ranks out of band (file, MPI, torch store, ...)
 *   every rank:  sship_init(device); sship_comm_create(id, rank, world, &comm)       (collective: all ranks must call)
 *   per batch:   sship_gather_features_rccl(comm, desc, kp, n, units, max_kp, desc_all, kp_all, n_all, stream)
 * Buffers are device memory: local desc [units, max_kp, 256] f16, kp [units, max_kp, 3] f32, n [units] i32; the *_all buffers
 * hold world x units units in rank order (rank r's block at r * units); ranks with fewer real units pad with n = 0.
 * The three all-gathers go out as ONE grouped RCCL step on `stream` (asynchronous; NULL = the default stream).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sship_comm sship_comm;
int sship_comm_unique_id(void* id_out_128);
int sship_comm_create(const void* id_128, int rank, int world, sship_comm** out);
void sship_comm_destroy(sship_comm* comm);
int sship_comm_rank(const sship_comm* comm);
int sship_comm_world(const sship_comm* comm);
int sship_gather_features_rccl(sship_comm* comm, const void* desc_local_dev, const float* kp_local_dev, const int* n_local_dev,
                               int units_per_rank, int max_keypoints, void* desc_all_dev, float* kp_all_dev, int* n_all_dev,
                               void* stream);

/* Per-stage device timings (ms) of the calling thread's last call sequence made with profiling enabled
 * (sship_set_profiling(1) inserts hipEvents; off by default; level 2 adds one event per SuperPoint layer launch - labels
 * "<scope>:<stage>/<layer>", e.g. "sp_gpu_infer:encoder/conv1a+conv1b+pool" - the IN-SITU launch durations bench.py's roofline
 * line reports; a profiled batch call also keeps a device copy of its input so that sship_sp_bench_layer re-launches on real pixels).  Labels are "<scope>:<stage>" where <scope> is the
 * reference's own SUPERSLAM_PROFILE label the stage belongs to - sp_gpu_infer (src/SuperPoint.cc:639),
 * sp_extract_stereo (:904), fe_lg_stereo_match (src/StereoFrontEnd.cc:32) - and <stage> this library's finer split
 * (encoder, heads, select, gather, posenc_qkv0, layers_x9, assign_filter); summing a scope's stages gives the
 * reference's figure.  At level 2 the SuperPoint stages are reported ONLY as their per-launch entries ("sp_gpu_infer:encoder/conv2a",
 * ...): no entry carries the bare "<scope>:<stage>" label, a stage's time is the sum over its "<scope>:<stage>/..." entries.  Timers are per thread.  Returns the number of stages. */
void sship_set_profiling(int level);
int sship_get_stage_timings(const char** labels, float* ms, int max_stages);

/* Measurement hook for bench.py's roofline line: re-launch ONE layer of the network `iters` times on the
 * handle's stream, bracketed by hipEvents on that same stream, over the activations left by the previous
 * sship_sp_* call of shape (batch, h, w); *avg_ms = mean launch duration.  layer: 0 conv1a, 1 conv1b (+pool),
 * 2 conv2a, 3 conv2b (+pool), 4 conv3a, 5 conv3b (+pool), 6 conv4a, 7 conv4b, 8 convPa, 9 convPb, 10 convDa,
 * 11 convDb.  *macs receives the layer's multiply-accumulate count for that shape. */
int sship_sp_bench_layer(sship_sp* sp, int layer, int batch, int h, int w, int iters, float* avg_ms, double* macs);
/* (layer ids 12-14 are the memory-bound stages of the same handle: 12 = softmax + depth-to-space + NMS + threshold +
 * candidate compaction, 13 = top-k, 14 = descriptor head at the selected keypoints (nearest or bilinear, as the handle is set); *macs = 0 for them.
 * 15 = conv2a + conv2b + pool as the ONE launch throughput batches run instead of layers 2 and 3 (csrc/conv_fuse2.hip; *macs = both layers').
 * 16 = the sub-pixel refinement of the selected keypoints (k_kp_refine), timed whatever mode the handle is in; *macs = 0.
 * 17 = the balanced selection alone (k_select_balanced) on the candidates of the handle's last selection, with the handle's bucket_px
 * (32 until set), timed whatever mode the handle is in; *macs = 0.)
 *
 * Same for one stage of the matcher, over the state the last match call left on this handle, timed with hipEvents on the
 * handle's stream: 0 first Wqkv projection, 1 self attention, 2 cross attention (both directions), 3 SelfBlock FFN + the
 * fused [to_qk|to_v] projection, 4 CrossBlock FFN + the fused next Wqkv, 5 last CrossBlock FFN + final_proj + matchability,
 * 6 assignment pass 1 (similarity tiles + row / column log-sum-exp), 7 assignment pass 2 (similarity tiles + row / column
 * arg-max of the double log-softmax scores). */
int sship_lg_bench_stage(sship_lg* lg, int stage, int iters, float* avg_ms);

/* Measurement aid for the roofline line: the v_mfma_f32_32x32x16_f16 rate (TFLOP/s) the device sustains from registers
 * for ~5 ms on every CU, with zero (random_operands = 0) or random fp16 operands.  The chip clocks to its power budget,
 * so the random-operand figure (about 1.6 PFLOP/s on MI355X) - not the 2.5 PFLOP/s datasheet peak - is what a real
 * convolution can approach.  No reference counterpart (the reference has no measurement API). */
int sship_mfma_probe(int random_operands, float* tflops);

#ifdef __cplusplus
}
#endif
#endif /* SSHIP_H_ */
