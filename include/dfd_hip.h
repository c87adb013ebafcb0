/*
 * dfd_hip.h - C ABI of libdfd_hip.so, the MI355X (gfx950) implementation of the
 * per-frame deepfake inference hot path.
 *
 * The reference (KrishTanna28/Real-Time-Video-Deepfake-Detection) is pure Python
 * and has no FFI of its own; each entry point below names the
 * reference call site whose arithmetic it replaces.  The ctypes binding that a
 * maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success and a negative dfd_status on failure;
 *     nothing throws or aborts across this boundary; the message for the last
 *     failure on a handle is dfd_last_error(handle) (dfd_last_error(NULL) for
 *     failures of dfd_create itself);
 *   - the caller owns every host buffer; pointers are borrowed for the call only;
 *   - "_device" variants take pointers into the handle's GPU (from dfd_device_alloc
 *     or any hipMalloc'd / torch CUDA tensor on that device), enqueue on the
 *     handle's HIP stream and return without synchronising;
 *   - a handle is not re-entrant: one caller thread per handle.
 */
#ifndef DFD_HIP_H
#define DFD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dfd_handle dfd_handle;

typedef enum dfd_status {
    DFD_OK = 0,
    DFD_ERR_ARG = -1,      /* bad argument (null, size, shape)            */
    DFD_ERR_BLOB = -2,     /* weights blob malformed or a tensor missing  */
    DFD_ERR_HIP = -3,      /* a HIP runtime call failed                   */
    DFD_ERR_NO_DEVICE = -4,/* no usable gfx950 device                     */
    DFD_ERR_STATE = -5,    /* call order (e.g. detector weights not set)  */
    DFD_ERR_CAPACITY = -6, /* batch larger than the handle was created for*/
    DFD_ERR_UNSUPPORTED = -7 /* valid input of a kind this path does not handle (e.g. progressive JPEG) */
} dfd_status;

#define DFD_ABI_VERSION 1
#define DFD_CROP 224          /* classifier input edge, reference deepfake_detection.py:383 */
#define DFD_FEATURES 1280     /* backbone feature width, reference model.py:46              */

int dfd_abi_version(void);

/* ---- lifetime ------------------------------------------------------------------
 * Replaces the import-time model construction + weight load of reference
 * deepfake_detection.py:30-90 (DeepfakeEfficientNet + load_state_dict + .to(DEVICE).eval()).
 * `blob` is the packed classifier produced by weights.pack_b0 (BatchNorm folded,
 * NHWC layouts).  `max_batch` sizes the activation workspace (9.6 MB of HBM per crop). */
int dfd_create(int device, const void* blob, size_t blob_len, int max_batch, dfd_handle** out);
void dfd_destroy(dfd_handle* h);
const char* dfd_last_error(const dfd_handle* h);
int dfd_max_batch(const dfd_handle* h);
/* Tuning switches (results stay within the parity tolerances either way):
 *   "fuse_expand" (default 1, env DFD_FUSE_EXPAND): MBConv blocks 1-5 compute the 1x1 expand conv
 *   inside the depthwise kernel instead of writing the expanded tensor to HBM.
 *   "fuse_late" (default 1 since round 4, env DFD_FUSE_LATE; needs "fuse_expand"): blocks 6-10 and 12-15 (14 x 14 / 7 x 7
 *   maps) do the same with whole images per thread block - the faster configuration; 0 = expand
 *   GEMM and depthwise kernel as separate launches.
 *   "fuse_late_skip" (bit b set = block b keeps separate launches although "fuse_late" is on; chosen per block by
 *   measurement at batch 256; env DFD_FUSE_LATE_SKIP).  Default: unset = blocks 8 and 9.  Changed with "fuse_k5": the
 *   value is signed now and any value < 0 means "unset" (it used to be read as an unsigned mask of every block); an
 *   unset mask and the explicit value (1 << 8) | (1 << 9) give the same results, but only the unset one lets "fuse_k5"
 *   take blocks 8 and 9.
 *   "fuse_k5" (default 1, env DFD_FUSE_K5; fp32 activations with "fuse_late"): blocks 6-11, every block whose input is
 *   a 14 x 14 map (6 and 7: k3; 8-10: k5; 11: k5 at stride 2, 14 -> 7), run
 *   expand + depthwise with ONE thread block per image that walks every 32-channel chunk - inputs loaded and split into
 *   bf16 terms once, four waves expanding chunk c + 1 while four run the depthwise phase of chunk c (mbconv_k5_kernel).
 *   Block 11 has no "fuse_late" form of its own: with this option off, below the threshold, or with bit 11 set in an
 *   explicit "fuse_late_skip" it runs expand GEMM + depthwise kernel, and the kernel gives it those launches' bits.
 *   A launch of one block per image takes the same time for 1 image and for one per compute unit, so the plan takes it
 *   only where the last round of blocks holds at least "fuse_k5_min" images (default, and any value <= 0: 208 of 256,
 *   the measured break-even; env DFD_FUSE_K5_MIN); smaller batches run the launches of "fuse_k5" = 0.  The kernel
 *   replaces whatever the block would run otherwise with that form's result bits (a block the unset mask covers: those
 *   of the separate launches; an unmasked block: those of the one-block-per-chunk launch; an explicitly masked block is
 *   left alone), so for a given "fuse_late_skip" neither this option nor the batch size changes a result.
 *   "fuse_stem" (default 1, env DFD_FUSE_STEM): the stem conv is computed inside block 0's depthwise
 *   kernel (the 112x112x32 stem activation stays in LDS).
 *   "fuse_proj0" (default 1, env DFD_FUSE_PROJ0; fp32 activations with "fuse_expand" and "split_gemm"): block 0's projection
 *   is computed inside block 1's expand + depthwise launch, from block 0's depthwise output; same result bits, one launch less.
 *   "split_gemm" (default 1, env DFD_SPLIT_GEMM): 1x1 convs (N >= 16) and the detector's k x k convs run on
 *   the split-precision GEMM (each fp32 operand = exact sum of three bf16 terms, six products on the bf16
 *   MFMA, fp32 accumulate: fp32-dot-product accuracy); 0 = the fp32 MFMA kernel everywhere.
 *   "mtcnn" (default 1): align every crop with the MTCNN cascade when the blob carries one.
 *   "overlap_forensics" (default 1): dfd_analyze_batch_device / dfd_analyze_frames_host run the six forensic signals of
 *   a batch on the handle's second stream beside the detector and the classifier and collect them at the end of the call;
 *   0 = in front of the detector on the main stream.  Same results.
 *   "forensic_chunk_bytes" (default 256 MiB; <= 0 restores it): work memory of one launch set of the general forensic
 *   chain in dfd_analyze_stream_batch / dfd_analyze_streams_batch - a size group runs in chunks of the frames that fit
 *   (one at least).  Same results at every value; tests force it small.
 *   "profile_stride" (default 1): between dfd_b0_profile_begin/end only every k-th forward records events.
 *   "stream_priority" (1 high, 0 normal - the default -, -1 low): re-creates the handle's main stream at that priority
 *   (the handle is drained first).  For a process that keeps two handles busy on one device (two batches in flight): the
 *   runtime maps streams of ONE priority onto a small pool of hardware queues and two main streams that land on the same
 *   queue run in line; streams of different priorities come from different pools. */
int dfd_set_option(dfd_handle* h, const char* name, int value);
/*   "bf16_activations" (default 0): every classifier activation that reaches HBM is stored as bf16 (arithmetic,
 *   accumulators, SE pools / gates and the MLP head stay fp32): BASELINE.json configs[3], DESIGN.md section 4a.
 *   "bf16_weight_planes" (3 or 1, default 3): with bf16 activations, the 1x1 convs multiply against the three exact
 *   bf16 planes of the fp32 weights (3) or against bf16-rounded weights (1).
 *   "gemm_tile" (default -1): >= 0 forces split-GEMM instance number value % (candidates of the shape) for every
 *   1x1 / k x k conv - parity tests walk 0 .. dfd_gemm_tile_count()-1 and require identical bits; -1 = the
 *   handle's tile table (measured by dfd_warmup, heuristic for shapes it has not seen).
 *   dfd_gemm_tile_count() is the largest candidate count any call can have, the pw8 / pw9 instances that only some
 *   calls may run included, so that walk reaches every instance of every shape. */
int dfd_gemm_tile_count(void);

/* One untimed pass over the classifier at batch `n_crops` (0 = skip; <= max_batch) and the detector at
 * `n_frames` frames (0 = skip) on synthetic data.  Sizes workspaces, splits the weights and MEASURES the
 * split-GEMM tile of every layer shape at those batch sizes (the only entry point that synchronises for
 * tuning; the "_device" entry points never do - a shape that was not warmed up runs a heuristic tile, with
 * the same result bits).  Call once per (n_crops, n_frames) you intend to serve; DFD_S6_TUNE=0 in the
 * environment skips the measurement. */
int dfd_warmup(dfd_handle* h, int n_crops, int n_frames);

/* The handle's measured tiles as text (one "M K N mode kind wm wn mt nt ks" line per shape) and back: a later
 * process - a profiled run, a server restart - imports them and dfd_warmup then measures only what is missing.
 * text_out == NULL queries the length.  Entries that name an instance this build cannot launch are dropped. */
int dfd_tiles_export(dfd_handle* h, char* text_out, size_t capacity, size_t* length);
int dfd_tiles_import(dfd_handle* h, const char* text, size_t length, int* accepted);

/* Host-only arithmetic of the split GEMM's 32-bit addressing guard: how many of `rows` rows of `row_bytes`
 * bytes one kernel launch may cover (a multiple of rows_per_image, whole `rows` when everything fits below
 * 2^31 bytes, -1 when a single image does not).  Batches above that are issued as several launches, so every
 * max_batch dfd_create accepts is addressable.  No GPU needed. */
long long dfd_gemm_chunk_rows(long long rows, long long row_bytes, long long rows_per_image);

/* One split-GEMM call on host data, through the launchers every network uses (launch_pointwise_split /
 * launch_conv_gemm_split on the handle's own tile table, so "gemm_tile" applies): tests/test_gemm_direct_gpu.py.
 *   pointwise (conv = 0): Y[M][N] = act((X[M][K] * gate[m / HW][K]) W^T + bias [+ R]) [+ R]
 *   conv      (conv = 1): n_img NHWC images H x W x Cin -> Ho x Wo x N, K = ksize^2 * Cin, M = n_img * Ho * Wo (M, K and
 *                         HW of the struct are ignored and filled in)
 * X, R and Y are fp32, or - bf16 = 1 - bf16 bit patterns (uint16); Wt is fp32 [N][K] (conv: [N][ky][kx][ci]), split on
 * the device; bias holds N values, followed by the N slopes when act = 3 (PReLU; 0 none, 1 swish, 2 relu); gate (may
 * be NULL, pointwise only) holds ceil(M / HW) rows of K; R (may be NULL) is added before (res_first = 1) or after the
 * activation; planes = 3, or 1 with bf16.  x_rows > 0 (pointwise): the host X holds only x_rows rows and the device
 * operand repeats them down all M rows (a 2 GiB operand from a small host block).
 * Y receives (M + 2 * DFD_GEMM_TAP_GUARD) rows of N: the device buffer is pre-filled with DFD_GEMM_TAP_SENTINEL (its
 * upper 16 bits with bf16) and returned whole - guard rows, result, guard rows - so a store past a ragged edge shows as a
 * changed guard and a missing store as a surviving sentinel.
 * Out: `candidates` = the number of instances "gemm_tile" indexes for this very call (its first launch), `tile` = the
 * instance that ran last (kind, wm, wn, mt, nt, ks; kind 0 pw6, 1 pw7, 2 pw8, 3 pw9), `launches` = kernel launches (the
 * 2^31-byte chunks of dfd_gemm_chunk_rows).
 * A result too large to return whole (above 2^32 bytes of Y): n_ranges > 0 and y_ranges = n_ranges pairs of rows [lo, hi)
 * - Y then receives the guard rows in front, the rows of the ranges in the order given, the guard rows behind, and
 * nothing else.  Either way `y_sentinels` = elements of the WHOLE result (guards excluded) still at the sentinel and
 * `y_digest` = the sum over its elements of bit pattern i x (2 i + 1) mod 2^64, computed on the device: two calls whose
 * digests agree stored the same bits in the same places.
 * DFD_ERR_UNSUPPORTED, without a launch and with Y at the sentinel, for shapes the launchers refuse (K % 8, K < 16,
 * conv Cin % 32). */
#define DFD_GEMM_TAP_GUARD 64
#define DFD_GEMM_TAP_SENTINEL 0x7FC5A5A5u
typedef struct dfd_gemm_tap_params {
    int32_t conv, bf16, planes, act, res_first, reserved;
    int32_t M, K, N, HW;
    int32_t n_img, H, W, Cin, ksize, stride, pad, dil, Ho, Wo;
    int64_t x_rows;
    const void* X;
    const float* Wt;
    const float* bias;
    const float* gate;
    const void* R;
    void* Y;
    int32_t candidates, launches;
    int32_t tile[6];
    int32_t n_ranges, reserved2;
    const int64_t* y_ranges;
    uint64_t y_sentinels, y_digest;
} dfd_gemm_tap_params;
int dfd_gemm_tap(dfd_handle* h, dfd_gemm_tap_params* p);

/* ---- device memory and stream plumbing (no reference counterpart) -------------- */
int dfd_device_alloc(dfd_handle* h, size_t bytes, void** dptr);
int dfd_device_free(dfd_handle* h, void* dptr);
int dfd_memcpy_h2d(dfd_handle* h, void* dst_dev, const void* src_host, size_t bytes);
int dfd_memcpy_d2h(dfd_handle* h, void* dst_host, const void* src_dev, size_t bytes);
int dfd_sync(dfd_handle* h);
/* Device-side ordering between two handles on the same device, without a host wait: everything queued on `h` after this
 * call starts only when the work queued on `other` so far has finished (an event recorded on other's stream, waited for by
 * h's stream).  bench.py orders its two classifier lanes with it around the step that carries per-launch events.
 * Threading: as every entry point, one caller thread per handle - no other thread may be inside a call on `h` or `other`. */
int dfd_wait_for(dfd_handle* h, dfd_handle* other);
/* device address of the handle's frame buffer: the last frame uploaded by a host-frame entry point or decoded by
 * dfd_decode_jpeg (packed BGR); valid until the next such call */
void* dfd_frame_ptr(dfd_handle* h);
/* HIP events on the handle's own stream (what bench.py times kernels with). */
int dfd_timer_begin(dfd_handle* h);
int dfd_timer_end(dfd_handle* h, float* elapsed_ms);

/* ---- classifier ------------------------------------------------------------------
 * DeepfakeEfficientNet.forward, reference model.py:63-72 (eval mode): normalised RGB
 * float32 NCHW (n,3,224,224) -> logits (n,1).  sigmoid is applied by the caller as at
 * reference deepfake_detection.py:397-398. */
int dfd_classify_nchw(dfd_handle* h, const float* nchw_host, int n, float* logits_host);
int dfd_classify_nchw_device(dfd_handle* h, const float* nchw_dev, int n, float* logits_dev);
/* DeepfakeEfficientNet.extract_features, reference model.py:74-89: -> (n,1280). */
int dfd_extract_features(dfd_handle* h, const float* nchw_host, int n, float* feat_host);

/* Runs the forward on `nchw_dev` and copies one named intermediate to the host
 * (NHWC float32): "stem", "b<i>.exp", "b<i>.dw", "b<i>.gate", "b<i>.out", "head",
 * "feat", "logit".  For stage-by-stage parity tests; `count` receives the number of
 * floats written (<= capacity). */
int dfd_b0_tap(dfd_handle* h, const float* nchw_dev, int n, const char* name,
               float* out_host, size_t capacity, size_t* count);

/* Per-launch timing with HIP events on the handle's stream.  Between begin and end every
 * dfd_classify_nchw_device call records an event after each kernel launch; end synchronises
 * and returns, per launch position, the elapsed milliseconds summed over the `steps`
 * instrumented forwards (every forward, or every "profile_stride"-th one) ("stem", "b<i>.exp", "b<i>.dw", "b<i>.se", "b<i>.proj", "head", "avgpool",
 * "mlp").  `names` receives pointers to static strings. */
int dfd_b0_profile_begin(dfd_handle* h);
int dfd_b0_profile_end(dfd_handle* h, float* ms_sum, const char** names, int max_layers,
                       int* count, int* steps);

/* ---- per-face pre-processing ----------------------------------------------------------
 * All take an 8-bit BGR image in host memory (rows `stride` bytes apart) as cv2 hands it to
 * the reference.  Boxes are (x, y, w, h) int32 quadruples inside the frame. */

/* cv2.resize(frame, (dw, dh), interpolation=INTER_LINEAR) for 8-bit BGR: reference
 * frame_analysis.py:71,112 (256x256) and face_detection.py:77 (300x300).  out: dh*dw*3. */
int dfd_resize_bgr(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride,
                   int dh, int dw, uint8_t* out);

/* DeepfakeDetector.preprocess_face_quality, reference deepfake_detection.py:357-370:
 * BGR->Lab, CLAHE(clipLimit 2.0, 8x8 tiles) on L, Lab->BGR.  out: height*width*3, packed. */
int dfd_preprocess_face_quality(dfd_handle* h, const uint8_t* bgr, int height, int width,
                                int stride, uint8_t* out);

/* One test-time-augmentation copy of a face crop, reference deepfake_detection.py:419-433:
 * cv2.flip(img, 1) when `flip`, cv2.convertScaleAbs(img, alpha=brightness, beta=0), then cv2.warpAffine(img,
 * cv2.getRotationMatrix2D((w/2, h/2), angle_deg, 1.0), (w, h)) with OpenCV's fixed-point bilinear sampling.
 * out: height*width*3, packed.  The random draws (flip probability .5, brightness 0.9..1.1, angle -3..3 degrees)
 * and the averaging of the per-copy probabilities stay on the host (DeepfakeDetector.analyze_face_with_tta). */
int dfd_tta_augment(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride, int flip, double brightness,
                    double angle_deg, uint8_t* out);

/* Test-time augmentation inside the batched pass.  A draw is one copy's (flip, brightness, angle_deg); a face with
 * `copies` draws is classified 1 + copies times: column 0 the un-augmented (CLAHE'd) crop, columns 1.. its copies in
 * draw order.  CLAHE runs once per face, ONE launch makes every copy of every face, all images go through the MTCNN
 * stage together (when it is on; a rejected image gets NaN and is never classified) and through the classifier in
 * chunks of max_batch images.  Nothing is averaged on the device: the host takes the mean of the sigmoids.
 *   dfd_tta_augment_crops : the copies alone, read straight from the frame (no CLAHE); draws [n][copies], face-major;
 *                           out = the images back to back, tight width*3 rows, face-major then copy
 *   dfd_classify_crops_tta: dfd_classify_crops with copies; logits_out [n][1 + copies], n <= max_batch faces
 *   dfd_tta_arm           : one-shot arming of the NEXT dfd_analyze_frame / dfd_analyze_jpeg / dfd_analyze_stream_batch /
 *                           dfd_analyze_streams_batch call on this handle, which consumes it whether it succeeds or
 *                           fails.  draws [capacity_faces][copies] are copied now; the faces of the call take rows in
 *                           the order the call returns them (frame-major, then face order).  That call checks at entry,
 *                           before any state moves, that capacity_faces >= n_frames x max_faces (else DFD_ERR_ARG).  Its
 *                           own logits_out keeps its meaning (column 0).  dfd_analyze_batch_device / dfd_analyze_frames_host
 *                           / dfd_analyze_jpegs_host do not take copies: armed, they return DFD_ERR_STATE.
 *   dfd_tta_logits        : the [n_faces][1 + copies] block of the last armed call (valid after it succeeded); with too
 *                           little room DFD_ERR_CAPACITY, *n_faces / *copies still set.
 * copies < 1 or null draws: DFD_ERR_ARG; copies > 63: DFD_ERR_CAPACITY (the per-face scratch layout). */
typedef struct dfd_tta_draw {
    int32_t flip;
    int32_t reserved;
    double brightness;
    double angle_deg;
} dfd_tta_draw;
int dfd_tta_augment_crops(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride, const int32_t* xywh, int n,
                          int copies, const dfd_tta_draw* draws, uint8_t* out);
int dfd_classify_crops_tta(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride, const int32_t* xywh, int n,
                           int apply_clahe, int copies, const dfd_tta_draw* draws, float* logits_out);
int dfd_tta_arm(dfd_handle* h, int copies, const dfd_tta_draw* draws, int capacity_faces);
int dfd_tta_logits(dfd_handle* h, float* logits_out, size_t capacity_floats, int* n_faces, int* copies);

/* crop (reference backend_server.py:160-161 / deepfake_detection.py:612) -> optional CLAHE ->
 * BGR->RGB, bilinear 224x224 (align_corners=False), /255, ImageNet normalise (reference
 * deepfake_detection.py:376,382-389).  When the blob carries an MTCNN cascade and option "mtcnn" is on, the re-crop at
 * :377 runs in between (P-/R-/O-Net, best face resampled to 160x160; a crop without a face gives the zero-filled
 * face's row here and NaN from the classify entry points).  nchw_out: (n,3,224,224) float32. */
int dfd_preprocess_crops(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride,
                         const int32_t* xywh, int n, int apply_clahe, float* nchw_out);

/* The same followed by the classifier: one logit per box (analyze_face without the
 * calibration/heuristic scalars, reference deepfake_detection.py:517-538). */
int dfd_classify_crops(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride,
                       const int32_t* xywh, int n, int apply_clahe, float* logits_out);

/* ---- Grad-CAM of the classifier ------------------------------------------------------------
 * pytorch_grad_cam 1.3.x GradCAM(model, target_layers=[net._conv_head]) with targets None (category 0 = the logit),
 * reference deepfake_detection.py:5-7 / :300-311 and model.py:100-102, computed without autograd (closed form of the
 * gradient through the MLP head and the head conv's swish + pool):
 *   cam7    (n,7,7)       float32: relu(sum_k alpha_k A_k) at the head conv's 7 x 7 grid, before any normalisation
 *   heat    (n,224,224)   float32: scale_cam_image (min-max, cv2 INTER_LINEAR 7 -> 224), then the one-layer
 *                                  aggregation's second min-max: the library's returned grayscale_cam
 *   overlay (n,224,224,3) uint8:   show_cam_on_image(img, heat, use_rgb=True) in BGR order, img = the de-normalised
 *                                  classifier input clamped to [0,1]; JET table: luts.JET_BGR (OpenCV parity unpinned)
 * cam7 / heat / overlay may each be NULL.  The logits are bit-identical to dfd_classify_nchw(_device) /
 * dfd_classify_crops on the same input and handle (the same forward runs).  n > max_batch: DFD_ERR_CAPACITY, the
 * handle stays usable.  Cost over a classify call: one more launch of the head GEMM without swish (z = BN(conv_head)
 * into the handle's dead expand buffer, handle activation type), an MLP backward (~0.34 GFLOP at n = 256) and one
 * map kernel per call that reads z once (250 KB fp32 per crop) - measured in DESIGN sections 4 / 5.  No HBM is
 * allocated: host-call outputs are staged in dead classifier workspace.
 *
 * dfd_gradcam_nchw_device: all pointers in HBM, enqueued on the handle's stream (no host wait), as
 * dfd_classify_nchw_device; the input must stay untouched until the stream has passed the call (the overlay reads it). */
int dfd_gradcam_nchw_device(dfd_handle* h, const float* nchw_dev, int n, float* logits_dev, float* cam7_dev,
                            float* heat_dev, uint8_t* overlay_dev);
/* the same from / to host memory (synchronises) */
int dfd_gradcam_nchw(dfd_handle* h, const float* nchw_host, int n, float* logits_host, float* cam7_host,
                     float* heat_host, uint8_t* overlay_host);
/* dfd_classify_crops followed by Grad-CAM (reference analyze_face with a heat map, deepfake_detection.py:517-546): a crop
 * the MTCNN stage rejects gets a NaN logit and all-zero cam7 / heat / overlay rows; the others run at the batch of the
 * crops kept.  Outputs are host arrays of n rows. */
int dfd_gradcam_crops(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride, const int32_t* xywh, int n,
                      int apply_clahe, float* logits_out, float* cam7_out, float* heat_out, uint8_t* overlay_out);

/* The three Grad-CAM launches with every stage returned (tests/test_gradcam_stages_gpu.py): the same kernels and grids as
 * the entry points above, on device buffers the call allocates itself.  All pointers are host memory.
 *   start = DFD_GRADCAM_TAP_FROM_X: x (n,3,224,224) runs through the forward and the un-activated head GEMM as in
 *     dfd_gradcam_nchw; z (n,49,1280; fp32, or bf16 bit patterns when the handle stores bf16 - z_bf16 is set on return),
 *     fc1 (n,512) and fc2 (n,256) receive what they left (each may be NULL).
 *   start = DFD_GRADCAM_TAP_FROM_Z: no forward; z (fp32, or uint16 bf16 bits with z_bf16 = 1, whatever the handle's
 *     option), fc1 and fc2 are inputs; x is read only for the overlay and may be NULL without one.  The handle's own
 *     fc1.w, fc2.w, fc3.w and head.b are used.
 * Stage outputs, each may be NULL: D1 (n + GUARD, 512), G (n + GUARD, 1280), cam7 (n + GUARD, 49), heat (n,224,224),
 * overlay (n,224,224,3).  The device buffers of D1, G and cam7 are pre-filled with DFD_GRADCAM_TAP_SENTINEL and returned
 * whole, with DFD_GRADCAM_TAP_GUARD rows (one row block of the MLP-backward kernels) behind row n - 1: a store past a
 * ragged batch shows as a changed guard, a missing store as a surviving sentinel.
 * n outside 1..max_batch (DFD_ERR_ARG / DFD_ERR_CAPACITY) and null required pointers (DFD_ERR_ARG) fail without a launch. */
#define DFD_GRADCAM_TAP_FROM_X 0
#define DFD_GRADCAM_TAP_FROM_Z 1
#define DFD_GRADCAM_TAP_GUARD 8
#define DFD_GRADCAM_TAP_SENTINEL 0x7FC5A5A5u
typedef struct dfd_gradcam_tap_params {
    int32_t start, n, z_bf16, reserved;
    const float* x;
    void* z;
    float* fc1;
    float* fc2;
    float* D1;
    float* G;
    float* cam7;
    float* heat;
    uint8_t* overlay;
} dfd_gradcam_tap_params;
int dfd_gradcam_tap(dfd_handle* h, dfd_gradcam_tap_params* p);

/* compute_frequency_features, reference model.py:105-149: BGR (channels = 3) or gray (1) 8-bit
 * image -> gray -> cv2.resize 224x224 -> channel 0 = min-max-normalised log1p|fftshift(fft2)|,
 * channel 1 = min-max-normalised log1p|cv2.dct(gray/255)|.  out: (2,224,224) float32.  The model
 * ignores this tensor (reference model.py:63-72); provided for API parity. */
int dfd_frequency_features(dfd_handle* h, const uint8_t* img, int height, int width, int stride,
                           int channels, float* out);

/* ---- face detector ----------------------------------------------------------------------
 * _detect_dnn, reference face_detection.py:71-105, for a blob packed with detector weights
 * (weights.pack_all): cv2.resize to 300x300, mean (104,177,123) subtraction, SSD forward,
 * DetectionOutput (NMS 0.45, top_k 400, keep_top_k 200), then the reference's integer
 * post-processing: conf > conf_thr (strict), scale by [w,h,w,h], truncate, clamp, keep
 * w > 20 and h > 20.  Writes up to max_out (x, y, w, h) quadruples in network (descending
 * confidence) order; frames smaller than 30 pixels in either direction give n_out = 0
 * (reference :55-56).  conf_out may be NULL. */
int dfd_detect_faces(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride,
                     float conf_thr, int32_t* xywh_out, float* conf_out, int max_out, int* n_out);
int dfd_has_detector(const dfd_handle* h);
/* Number of detections of the last dfd_detect_faces / dfd_analyze_frame call BEFORE the max_out / max_faces cut:
 * `len(faces)` of the reference (backend_server.py:181 reports it while classifying faces[0] only). */
int dfd_last_detection_count(const dfd_handle* h);
/* Crops the classifier has been run on since dfd_create (sum of its batch sizes over every entry point).  With the MTCNN
 * stage on, a crop the cascade rejects is never classified (reference deepfake_detection.py:377-380 returns before the
 * model runs): a call with n boxes of which k keep a face advances this by k.  Tests read it before / after a call. */
int dfd_classifier_crop_count(const dfd_handle* h, unsigned long long* total);
/* One named detector intermediate for parity tests: a layer name of ssd_arch.LAYERS,
 * "<source>.head", "prob", "boxes" (per prior) or "rows" (DetectionOutput: score,x1,y1,x2,y2). */
int dfd_ssd_tap(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride,
                const char* name, float* out, size_t capacity, size_t* count);
/* The detector's tail on caller-supplied host arrays, for parity tests (as dfd_mtcnn_net_tap): values and counts no
 * image produces.  n = 1..8 images in one call, P = the plan's prior count (8732), with the handle's own prior table,
 * variances, thresholds and keep_top_k, through the buffers the production path uses.
 *   heads != NULL (boxes_in = prob_in = NULL): the six head outputs as ssd_decode_kernel reads them, source after source,
 *   each [n][cells][p * 6] (p * 4 loc values, then p * 2 logits: background, face); runs the decode, then
 *   DetectionOutput; boxes_out [n][P][4] and prob_out [n][P] (either may be NULL) receive the decode's result.
 *   heads == NULL: boxes_in [n][P][4] and prob_in [n][P]; runs DetectionOutput alone.
 * rows_out [n][keep_top_k][5] (score, x1, y1, x2, y2; zero past an image's count; rows_capacity = its size in floats),
 * count_out [n].  DFD_ERR_HIP when an image's count comes back as -1 (see dfd_detect_faces). */
int dfd_ssd_detection_tap(dfd_handle* h, int n, const float* heads, const float* boxes_in, const float* prob_in,
                          float* boxes_out, float* prob_out, float* rows_out, size_t rows_capacity, int* count_out);

/* ---- Haar cascade fallback -------------------------------------------------------------
 * _detect_haar, reference face_detection.py:108-123: cv2.CascadeClassifier.detectMultiScale(gray, scaleFactor,
 * minNeighbors, minSize=(min_size, min_size)) for a stump cascade with upright HAAR features packed into the blob
 * (haar.load_cascade_xml reads OpenCV's XML; weights.pack_all(..., haar=...)).  The reference uses this path
 * whenever its SSD files are missing.  Boxes are the grouped rectangles in OpenCV's order; n_candidates (may be
 * NULL) receives the number of windows that passed the cascade before grouping.
 * scale_factor (> 1) is a double, as OpenCV's scaleFactor: the loop multiplies it up in double, and the float 1.1f would
 * round some scaled sizes the other way from scale 5 on.  dfd_create refuses (DFD_ERR_BLOB) a cascade whose stage,
 * feature or rectangle numbers would index outside its tables or its window. */
int dfd_has_haar(const dfd_handle* h);
int dfd_detect_faces_haar(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride, double scale_factor,
                          int min_neighbors, int min_size, int32_t* xywh_out, int max_out, int* n_out, int* n_candidates);
/* One named buffer of ONE scale of that loop, for parity tests (as dfd_ssd_tap): the production kernels through the
 * production buffers on the host frame `bgr`, at the scale_index-th factor 1, scale_factor, scale_factor^2, ... (every
 * scale counts; there is no min_size here).  name: "gray" (u8 [height][width]), "scaled" (u8 [sh][sw], the gray image
 * itself where the scale keeps the frame's size), "sum" (u32 [sh + 1][sw + 1]), "sqsum" (u64, same shape), "result"
 * (i32 [ny][nx] per grid position: 1 = passed, 0 = rejected by stage 0, -s = rejected by stage s), or NULL for the
 * geometry alone.  out receives *bytes bytes (capacity in bytes); dims[8] = sh, sw, ny, nx, grid step, reported window
 * width, height, number of scales; *factor = the factor used.  A scale_index past the last scale is DFD_ERR_ARG. */
int dfd_haar_tap(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride, double scale_factor, int scale_index,
                 const char* name, void* out, size_t capacity, size_t* bytes, int32_t* dims, double* factor);

/* ---- MTCNN align/crop -------------------------------------------------
 * The reference runs facenet-pytorch's MTCNN(select_largest=False, post_process=False) on every
 * already-cropped face before the classifier (deepfake_detection.py:24-28, 376-380): P-Net over a
 * 0.709 scale pyramid, R-Net, O-Net (thresholds .6/.7/.7, NMS .5/.7/.7/.7-Min), the box with the
 * highest probability, then PIL crop + 8-bit BILINEAR resize to 160x160.  Present when the blob
 * carries "mtcnn.*" tensors (weights.pack_mtcnn_tensors); the classify entry points
 * (dfd_classify_crops, dfd_preprocess_crops, dfd_analyze_frame, dfd_analyze_batch_device) then align
 * every crop with it and return a NaN logit where it finds no face (the reference returns None
 * there); dfd_set_option(h, "mtcnn", 0) bypasses the stage.  The box bookkeeping between the three networks (NMS,
 * regression, squaring, clipping, selection, extract_face geometry and resize tables) runs on the device, one thread
 * block per crop and stage (csrc/mtcnn_boxes.hip); environment DFD_MT_DEVICE_BOXES=0 keeps it on the library's host
 * side (identical results; also the fallback when a crop has more than 8192 P-Net candidates or 4096 windows).
 *   face_chw_out : NULL or 3*160*160 floats, RGB planes 0..255 (what MTCNN.forward returns)
 *   box_out      : NULL or 5 floats (x1, y1, x2, y2, probability) of the selected box
 *   found        : 1 / 0 */
int dfd_has_mtcnn(const dfd_handle* h);
int dfd_mtcnn_align(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride,
                    float* face_chw_out, float* box_out, int* found);
/* One named cascade intermediate for parity tests; dims[3] receives the shape.  Every buffer the cascade
 * materialises has a name (activations NHWC, fp32):
 *   "pnet.in.<level>" [sh][sw][3] the area-resized, normalised RGB level; "pnet.pool1.<level>" [ph][pw][10] conv1 + PReLU
 *   + ceil-mode pool of ONE launch (the conv1 map is never stored); "pnet.conv2.<level>" [ph-2][pw-2][16];
 *   "pnet.prob.<level>" [H][W], "pnet.reg.<level>" [H][W][4] (conv3 + both heads + softmax of one launch: the 32-channel
 *   conv3 map is never stored either);
 *   "pnet.cand": the raw candidate records of ALL images of the call in the order the conv3 launch appended them,
 *   [k][6] 32-bit words {cell (uint32, index into the concatenated maps of all levels of all images), p, r[4]}: dims =
 *   {records, 6, the launch's counter};
 *   "rnet.in" [n][24*24][3], "rnet.pool1" [n][11*11][32] (conv1 + PReLU + pool, one launch; channels 28..31 are zero
 *   padding), "rnet.conv2" [n][9*9][64] (48..63 zero padding), "rnet.pool2" [n][4*4][64], "rnet.conv3" [n][3*3][64],
 *   "rnet.dense4" [n][1][128], "rnet.prob" [n], "rnet.reg" [n][4] of the image's candidate windows in order;
 *   "onet.in" [n][48*48][3], "onet.pool1" [n][23*23][32], "onet.conv2" [n][21*21][64], "onet.pool2" [n][10*10][64],
 *   "onet.conv3" [n][8*8][64], "onet.pool3" [n][4*4][64], "onet.conv4" [n][3*3][128], "onet.dense5" [n][1][256],
 *   "onet.prob", "onet.reg", "onet.pts" [n][10] (the landmark head, evaluated for this tap only);
 *   "stage1" / "stage2" / "stage3" rows (x1,y1,x2,y2,score); "boxes.overflow" [1]: 1 when an image exceeded the device
 *   box blocks' capacity and the call ran on the host path (device box path only).
 * dfd_mtcnn_tap runs one image.  dfd_mtcnn_tap_batch runs n images in ONE cascade call - the ragged launches of
 * dfd_classify_crops / dfd_analyze_batch_device - and reads the buffer of image `crop`; a network that no window of that
 * image reached yields an empty tap.  dfd_mtcnn_net_tap runs the R-Net (onet = 0, 24 x 24) or O-Net (48 x 48) trunk alone,
 * on m windows, in chunks as in production, and reads rows [row0, row0 + rows) of an "rnet.*" / "onet.*" buffer.  Its
 * input is either `windows` [m][sz][sz][3], which takes the place of the window resize (values and counts no image
 * produces), or - windows = NULL - the source windows xywh [m][4] (x, y, w, h inside the image) of the BGR image given.
 * P-Net has no injected input: its ragged launches take their geometry from the image sizes.
 * A call that names no tap (every production entry point) downloads none of these. */
int dfd_mtcnn_tap(dfd_handle* h, const uint8_t* bgr, int height, int width, int stride,
                  const char* name, float* out, size_t capacity, size_t* count, int* dims);
int dfd_mtcnn_tap_batch(dfd_handle* h, int n_images, const uint8_t* const* bgr, const int* heights, const int* widths,
                        const int* strides, int crop, const char* name, float* out, size_t capacity, size_t* count, int* dims);
int dfd_mtcnn_net_tap(dfd_handle* h, int onet, const float* windows, const uint8_t* bgr, int height, int width, int stride,
                      const int* xywh, int m, int row0, int rows, const char* name, float* out, size_t capacity,
                      size_t* count, int* dims);

/* ---- MTCNN with every constructor argument of the package: all faces, landmarks, any crop size ----------
 * facenet_pytorch.MTCNN(image_size, margin, min_face_size, thresholds, factor, post_process, select_largest,
 * selection_method, keep_all) on a list of images in ONE device pass.  dfd_mtcnn_params_default fills the package's
 * defaults (160, 0, 20, .6/.7/.7, .709, post_process, select_largest).
 *   selection : order of the returned rows.  NONE: as stage 3 yields them (descending probability - MTCNN.detect with
 *               select_largest=False); PROBABILITY; LARGEST: box area; CENTER_WEIGHTED_SIZE: area - 2 x squared offset of
 *               the box centre from the image centre; LARGEST_OVER_THRESHOLD: area among the rows above 0.9 probability.
 *               Descending key; of equal keys the LATER stage-3 row comes first (np.argsort(..)[::-1], stable sort).
 *   keep_all  : 0: only row 0 of that order is returned (n_faces_out <= 1); 1: every row.
 *   factor    : double, as the package multiplies Python floats. */
enum {
    DFD_MT_SELECT_NONE = 0,
    DFD_MT_SELECT_PROBABILITY = 1,
    DFD_MT_SELECT_LARGEST = 2,
    DFD_MT_SELECT_CENTER_WEIGHTED_SIZE = 3,
    DFD_MT_SELECT_LARGEST_OVER_THRESHOLD = 4
};
typedef struct dfd_mtcnn_params {
    int image_size;        /* edge of the returned crops                                   */
    int margin;            /* extract_face margin, in pixels of the returned crop          */
    int min_face_size;     /* >= 12                                                        */
    float thresholds[3];   /* P-Net (>=), R-Net, O-Net (>) face probability                */
    double factor;         /* pyramid scale step, in (0, 1)                                */
    int selection;         /* DFD_MT_SELECT_*                                              */
    int keep_all;
    int post_process;      /* crops as (x - 127.5) / 128 instead of 0..255                 */
} dfd_mtcnn_params;
void dfd_mtcnn_params_default(dfd_mtcnn_params* params);
/* MTCNN.detect(landmarks=True) for n_images packed BGR images (bgr[i], heights[i] x widths[i], row stride strides[i] bytes).
 *   boxes_out     : [n_images][max_faces][5] (x1, y1, x2, y2, probability)
 *   landmarks_out : NULL (the landmark head is then not run) or [n_images][max_faces][5][2] (x, y) in image coordinates
 *   n_faces_out   : [n_images] rows of the order (may exceed max_faces: call again with more room); only
 *                   min(n_faces, max_faces) rows of an image are written, the rest of the arrays is left alone
 * DFD_ERR_ARG for parameters that make no sense (image_size <= margin, factor outside (0,1), min_face_size < 12, thresholds
 * outside [0,1], n_images x max_faces > 65535), DFD_ERR_CAPACITY beyond 64 pyramid levels per image, DFD_ERR_STATE when the
 * blob holds no cascade.  Results do not depend on DFD_MT_DEVICE_BOXES. */
int dfd_mtcnn_detect(dfd_handle* h, int n_images, const uint8_t* const* bgr, const int* heights, const int* widths,
                     const int* strides, const dfd_mtcnn_params* params, int max_faces, float* boxes_out,
                     float* landmarks_out, int* n_faces_out);
/* MTCNN.forward: the same, plus extract_face of every returned row (margin scaled to the box, corners clipped to the image,
 * PIL crop + 8-bit BILINEAR resize to image_size^2):
 *   faces_out : [n_images][max_faces][3][image_size][image_size] floats, RGB planes 0..255 or standardised; a row whose
 *               clipped box is empty (the package raises there) gets a zero face. */
int dfd_mtcnn_extract(dfd_handle* h, int n_images, const uint8_t* const* bgr, const int* heights, const int* widths,
                      const int* strides, const dfd_mtcnn_params* params, int max_faces, float* boxes_out,
                      float* landmarks_out, int* n_faces_out, float* faces_out);

/* ---- frame forensics ------------------------------------------------------------------
 * FrameForensicAnalyzer.analyze (full != 0) / analyze_fast (full == 0), reference
 * frame_analysis.py:58-126: cv2.resize to 256x256, then the six signals (:128-389), weighted
 * sum (:49-56,88 / :118-119), clip to [0,1].  Temporal state (previous gray frame, last 30
 * mean differences, frame counter; :35-37) is kept per `stream_id` inside the handle.
 *   scores_out[6] = frequency, noise, ela, edge, color, temporal   (NaN where the fast variant
 *                   does not compute a signal)
 *   prob_out      = fake_probability
 *   stats_out     = NULL or DFD_FORENSIC_NSTATS doubles: the quantities the thresholds act on
 *                   (low/mid/high band means, high ratio, mid ratio, mid cv, noise mean, noise cv,
 *                    ela mean, ela cv, edge density, laplacian variance, S std, V std, unique hues,
 *                    mean abs frame difference (-1 on a stream's first frame), temporal cv,
 *                    frame counter) */
#define DFD_FORENSIC_NSTATS 18
int dfd_forensics(dfd_handle* h, int stream_id, const uint8_t* bgr, int height, int width, int stride,
                  int full, double* scores_out, double* prob_out, double* stats_out);
/* FrameForensicAnalyzer.reset, reference frame_analysis.py:391-395. */
int dfd_forensics_reset(dfd_handle* h, int stream_id);
/* Drops a stream's state (reset keeps its 64 KB device plane and its entry): the plane goes to a free list inside the
 * handle and is reused by the next new stream, so short-lived streams cost no HBM and no device allocation.  The stream
 * id may be used again afterwards; it then starts as a new stream.  Unknown ids are a no-op. */
int dfd_forensics_release(dfd_handle* h, int stream_id);
/* Mirrors the analyzer's attributes frame_count, len(temporal_diffs), prev_frame_gray is not None. */
int dfd_forensics_state(dfd_handle* h, int stream_id, int* frame_count, int* n_diffs, int* has_prev);

/* One named buffer of the forensic kernel chain, for parity tests (as dfd_ssd_tap / dfd_mtcnn_tap).  The chain runs on n
 * (1..64) frames that are already 256x256 (no resize), in full or fast mode, touching no stream's temporal state, and
 * `name` of frame `frame` (-1: of all n frames, frame-major) is copied to `out` as raw bytes; *bytes receives their count.
 *   start = "rs": from bgr256, n x 256 x 256 x 3 BGR bytes (start_data unused).
 *   start = "gray" | "grad" | "map": teacher forcing - start_data (n planes: uint8 gray, int16 (dx, dy) pairs, uint8
 *           labels 0 candidate / 1 none / 2 strong) replaces that buffer and only the kernels downstream of it run
 *           (bgr256 unused); a buffer that is not downstream, or that needs `rs`, is refused.
 * Per frame: "rs" u8[256][256][3]; "gray", "map", "jy" u8[256][256]; "jcb", "jcr" u8[128][128]; "grad" i16[256][256][2];
 * "fft_tmp" (row pass) and "spectrum" (both passes) complex64 [kx][ky] (transposed); "logmag" f32 [kx][ky], the
 * log1pf(hypotf()) values the band sums add; "edges" u8[256][256] 0 / 1, the final hysteresis set; f64 "fft_part"
 * [256][7] (low sum, count | mid sum, sum of squares, count | high sum, count), "lap_part" [256][2], "hsv_part" [256][4],
 * "stats_noise" [64], "stats_ela" [64], "edge_count" [1], "stats" [9] (band means low, mid, high, mid std, Laplacian
 * variance, edge count, S std, V std, hues; only the first 6 unless full and start = "rs"); "hue_bits" u32[6]; and
 * "twiddle", complex64 [128], the FFT's table (not per frame). */
int dfd_forensic_tap(dfd_handle* h, const uint8_t* bgr256, int n, int full, const char* start, const void* start_data,
                     const char* name, int frame, void* out, size_t capacity, size_t* bytes);

/* ---- frame forensics at any square analysis size ---------------------------------------------
 * FrameForensicAnalyzer(analysis_size=(size, size)) of the reference (frame_analysis.py:28-46): dfd_forensics with the
 * resize target, the band radii size/8, size/4, size/2 around (size/2, size/2), the 32x32 blocks at i, j in
 * range(0, size - 31, 32) and every divisor derived from `size`, a multiple of 16 in 32..1024 (anything else:
 * DFD_ERR_ARG).  With fewer than 4 blocks (size < 64) the noise and ELA scores are 0.0 and their statistics NaN.
 * Outputs as dfd_forensics.  size = 256 is accepted and runs this general chain, not the 256x256 kernels.
 * A stream's analysis size is fixed by dfd_forensics_open or, unopened, by its first frame: this entry at another size,
 * or dfd_forensics (256x256) on a stream of another size, return DFD_ERR_STATE and change nothing.
 * dfd_forensics_reset keeps size and plane; dfd_forensics_release returns the size x size plane to a free list keyed
 * by plane size, after which the id may start again at any size. */
int dfd_forensics_sized(dfd_handle* h, int stream_id, const uint8_t* bgr, int height, int width, int stride, int size,
                        int full, double* scores_out, double* prob_out, double* stats_out);
/* Fixes the analysis size of a stream that has not seen a frame (a new id, or an id after dfd_forensics_release): size as
 * for dfd_forensics_sized, anything else DFD_ERR_ARG.  On a stream that already holds a size, the same size is a no-op
 * and another size returns DFD_ERR_STATE and changes nothing.  The stream-carrying entries - dfd_analyze_frame,
 * dfd_analyze_jpeg, dfd_analyze_stream_batch, dfd_analyze_streams_batch - run a stream at the size it holds: an opened
 * stream on the general chain of dfd_forensics_sized (size = 256 included), with results, bit for bit, those of
 * dfd_forensics_sized on the same frames; a stream whose first frame came through dfd_forensics_sized at another size than
 * 256 likewise; a stream that was never opened on the 256x256 kernels, as dfd_forensics.  dfd_analyze_streams_batch takes
 * streams of different sizes in one call: the frames are grouped by analysis size, each group gets one ragged resize and
 * one launch set per chunk of the frames that fit the work-memory budget (dfd_set_option "forensic_chunk_bytes", default
 * 256 MiB, values <= 0 restore it; one frame at least; the split changes no result), and one launch differences every
 * frame of the general chain against its predecessor, one more writes every such stream's last gray plane back. */
int dfd_forensics_open(dfd_handle* h, int stream_id, int size);
/* dfd_forensic_tap for the general chain: n (1..16) frames that are already size x size.  Same buffer names and
 * teacher-forcing starts; per frame, with S = size: "rs" u8[S][S][3]; "gray", "map", "jy", "edges" u8[S][S]; "jcb",
 * "jcr" u8[S/2][S/2]; "grad" i16[S][S][2]; "fft_tmp" (row pass), "spectrum" (both passes)
 * complex64 [S][S] and "logmag" f32 [S][S] ([kx][ky]);
 * f64 "fft_part" [S][7], "lap_part" [S][2], "hsv_part" [S][4] (one partial per row), "stats_noise", "stats_ela"
 * [(S/32)^2], "edge_count" [1], "stats" [9] / [6]; "hue_bits" u32[6]; "twiddle" complex64 [S], exp(-2 pi i j / S). */
int dfd_forensic_tap_sized(dfd_handle* h, const uint8_t* frames, int n, int size, int full, const char* start,
                           const void* start_data, const char* name, int frame, void* out, size_t capacity, size_t* bytes);

/* ---- one frame, end to end ---------------------------------------------------------------
 * The per-frame work of DeepfakeDetector.predict (reference deepfake_detection.py:597-626)
 * and of the /analyze handler (reference backend_server.py:147-164) with ONE upload of the
 * frame: forensics (full or fast) on `stream_id`, face detection, then crop -> CLAHE -> 224x224
 * -> classifier for the first min(n_detected, max_faces) boxes (predict uses all faces, the
 * server faces[0]; more faces than the handle's max_batch are classified in several passes).  scores_out[6]/forensic_prob_out as dfd_forensics; xywh_out receives
 * n_faces_out boxes and logits_out one logit per box.  Calibration, the +0.10 small-face
 * heuristic and the vote are host logic (scalars). */
int dfd_analyze_frame(dfd_handle* h, int stream_id, const uint8_t* bgr, int height, int width,
                      int stride, int full_forensics, float conf_thr, int max_faces, int apply_clahe,
                      double* scores_out, double* forensic_prob_out, int32_t* xywh_out,
                      int* n_faces_out, float* logits_out);

/* ---- image decode at the HTTP edge -----------------------------------------------------
 * cv2.imdecode(np.frombuffer(bytes), cv2.IMREAD_COLOR) of reference backend_server.py:139-145 for JPEG input (what
 * the extension sends): entropy decoding on the host, dequantisation + libjpeg's islow IDCT + fancy chroma
 * upsampling + YCbCr->RGB on the device - bit-identical to libjpeg's defaults.  8-bit sequential Huffman JPEGs, gray
 * or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, restart intervals; anything else returns
 * DFD_ERR_UNSUPPORTED (the host then decodes with its own library and calls dfd_analyze_frame).
 * Supported besides, with option "jpeg_progressive" = 1 (default 0: as above; the environment variable
 * DFD_JPEG_PROGRESSIVE sets the value a new handle starts with): 8-bit progressive Huffman files (SOF2) of the same
 * colour spaces and samplings, any number of scans with tables and restart intervals redefined between them, whose scan
 * script is in order (T.81 G.1.1.1.1) and COMPLETE - every coefficient of every component sent and refined to its last
 * bit, so that libjpeg does no block smoothing.  Incomplete or out-of-order scripts, a quantisation table redefined between
 * two scans, arithmetic, 12-bit and CMYK files stay DFD_ERR_UNSUPPORTED; a second SOF in such a file is DFD_ERR_ARG.  The option holds for every entry that takes JPEG bytes; the scans of progressive files are
 * decoded by the host decoder (csrc/jpeg_progressive.h), in batch calls one file per pool thread - or, with option
 * "jpeg_device_progressive" = 1 (default 0), in dfd_decode_jpeg_batch and the stream batch calls on the device
 * (csrc/jpeg_gpu_progressive.h: the bytes cross PCIe, the scans run by dependency level, one lane per restart segment; a
 * file the device reports a defect for is decoded again by the host decoder, which gives the status).
 * dfd_decode_jpeg: bgr_out may be NULL (size query through height / width; the frame stays on the device).
 * dfd_analyze_jpeg: dfd_analyze_frame without the raw upload - the decoded frame never visits the host. */
/* The host half alone (no GPU needed; tests pin it against libjpeg through the oracle's IDCT): info[14] = width,
 * height, components, hmax, vmax, then per component (blocks_w, blocks_h, quantisation table index);
 * qtables_out = 4 x 64 uint16 in natural order (NULL: skip); coef_out = int16 quantised coefficients in natural
 * order, 64 per block, blocks row-major per component incl. MCU padding, components concatenated (NULL: count only).
 * Errors of this function are reported through dfd_last_error(NULL). */
int dfd_jpeg_coefficients(const uint8_t* jpeg, size_t len, int* info, uint16_t* qtables_out, int16_t* coef_out,
                          size_t capacity, size_t* count);
/* dfd_jpeg_coefficients with flags: DFD_JPEG_ALLOW_PROGRESSIVE takes progressive files as option "jpeg_progressive"
 * does for a handle's calls; flags = 0 is dfd_jpeg_coefficients. */
#define DFD_JPEG_ALLOW_PROGRESSIVE 1u
int dfd_jpeg_coefficients_ex(const uint8_t* jpeg, size_t len, unsigned flags, int* info, uint16_t* qtables_out, int16_t* coef_out,
                             size_t capacity, size_t* count);
int dfd_decode_jpeg(dfd_handle* h, const uint8_t* jpeg, size_t len, uint8_t* bgr_out, size_t capacity, int* height, int* width);
/* n JPEGs of ONE size -> n packed BGR frames [n][H][W][3] (bgr_out may be NULL: the frames stay on the device).  Round 4:
 * in a batch the scans of restart-less files are entropy-decoded ON THE DEVICE (csrc/jpeg_gpu_entropy.h: a lane per
 * 512-byte chunk of the de-stuffed scan, the host decoder's speculative-chunk scheme as a fixed-point iteration) - the
 * JPEG bytes cross PCIe instead of 6.2 MB of coefficients per 1080p frame.  Restart-interval files (unless option
 * "jpeg_device_restart" is on), files of differing sampling, and any frame the device decoder's own checks do not vouch for
 * go through the host decoder; the result is the same bits either way (tests pin both to libjpeg).  Options:
 * "jpeg_device_entropy" (default 2: from 1 MiB of scan data per call - a small batch is quicker on the host pool; 1 =
 * always; 0 = never), "jpeg_device_restart" (default 0: files with a restart interval (DRI) take the host decoder; 1: they
 * are eligible for the device decoder under the "jpeg_device_entropy" rule like any other file, alone or mixed with
 * restart-less files of the same size and sampling - every RSTn marker is a certain start state for the lanes; a file whose
 * restart structure is malformed (marker missing, misnumbered or surplus) is still decoded by the host decoder, as are
 * single-file calls; the environment variable DFD_JPEG_DEVICE_RESTART sets the value a new handle starts with),
 * "jpeg_chunk_bytes" (default 512), "jpeg_rounds".  dfd_jpeg_decode_counts: frames of batch calls decoded on the device /
 * by the host decoder since dfd_create (restart-interval frames decoded on the device count as device decodes). */
int dfd_decode_jpeg_batch(dfd_handle* h, int n, const uint8_t* const* jpegs, const size_t* lens, uint8_t* bgr_out, size_t capacity,
                          int* height, int* width);
int dfd_jpeg_decode_counts(const dfd_handle* h, unsigned long long* on_device, unsigned long long* on_host);
/* dfd_analyze_frames_host with JPEG files instead of raw frames: n_total files of one size and sampling (jpegs[i], lens[i]; host
 * memory, from dfd_host_alloc for full speed) are analysed `batch` at a time - the scans of chunk k + 1 cross PCIe on the
 * copy stream while chunk k is entropy-decoded on the device, turned into frames (IDCT, upsampling, colour) and run
 * through dfd_analyze_batch_device.  0.3 - 1.2 MB per 1080p frame over the link instead of 6.2 MB: the path that is not
 * bound by the raw upload.  DFD_ERR_UNSUPPORTED for files only the host decoder takes (mixed layouts; restart intervals
 * unless option "jpeg_device_restart" is 1).
 * Results as dfd_analyze_batch_device; height_out / width_out (may be NULL) receive the frame size. */
int dfd_analyze_jpegs_host(dfd_handle* h, const uint8_t* const* jpegs, const size_t* lens, int n_total, int batch,
                           const int32_t* forced_xywh, int forced_k, float conf_thr, int max_faces, int apply_clahe, int with_forensics,
                           int32_t* xywh_out, int* n_faces_out, float* logits_out, double* forensic_prob_out, int* height_out,
                           int* width_out);
int dfd_analyze_jpeg(dfd_handle* h, int stream_id, const uint8_t* jpeg, size_t len, int full_forensics, float conf_thr,
                     int max_faces, int apply_clahe, double* scores_out, double* forensic_prob_out, int32_t* xywh_out,
                     int* n_faces_out, float* logits_out, int* height_out, int* width_out);

/* ---- baseline JPEG encode on the device (csrc/jpeg_encode.hip) ----------------------------------
 * Pixels -> a JFIF file whose BYTES equal what libjpeg(-turbo) writes for the same pixels with its default settings and
 * the Annex K Huffman tables (Pillow's `save(..., quality=q, subsampling=s, optimize=False)`): colour conversion, edge
 * replication, h2v1 / h2v2 downsampling, the islow FDCT, quantisation, Huffman coding, byte stuffing and the RSTn markers all
 * run on the device; only the ~600-byte header is built on the host.  One call encodes a batch of images of any sizes and
 * modes in one chain of launches; an image's bytes do not depend on what else is in the batch.
 * A source is BGR (rgb = 0) or RGB (rgb = 1) u8 with 3 bytes per pixel, or with subsampling DFD_JPEG_GRAY one u8 plane;
 * stride in bytes.  quality 1..100; restart_blocks = MCUs per restart interval (0 = none, at most 65535; Pillow's
 * restart_marker_blocks).  Images of fewer than 1 x 1 pixels or more than 65535 a side, quality outside 1..100, an unknown
 * subsampling or a bad restart_blocks: DFD_ERR_ARG.  An image above 2^24 pixels: DFD_ERR_UNSUPPORTED (a block codes to at
 * most 1,658 bits and a 4:4:4 image of 2^24 pixels has 3 x 2^18 blocks, so every bit offset inside one image fits 32 bits).
 * Output: host memory.  dfd_encode_jpeg writes one file to out and its size to *len.  The batch calls write the files back
 * to back into out, file i at offsets[i] with lens[i] bytes, and the sum to *total.  Sizes are exact before anything is
 * written: when capacity is too small the call returns DFD_ERR_ARG, *len / *total (and lens) hold what is needed, and out is
 * untouched.  dfd_encode_jpeg_bound: a capacity that always suffices for one image (0 for arguments the encoder refuses).
 * dfd_encode_jpeg_device: the sources' pixels are in HBM (frames of dfd_decode_jpeg_batch, dfd_device_alloc buffers);
 * only JPEG bytes cross to the host. */
enum { DFD_JPEG_444 = 0, DFD_JPEG_422 = 1, DFD_JPEG_420 = 2, DFD_JPEG_GRAY = 3 };
typedef struct dfd_jpeg_source {
    const uint8_t* pixels;
    int32_t height, width, stride;
    int32_t rgb, quality, subsampling, restart_blocks;
} dfd_jpeg_source;
size_t dfd_encode_jpeg_bound(int height, int width, int subsampling);
int dfd_encode_jpeg(dfd_handle* h, const uint8_t* pixels, int height, int width, int stride, int rgb, int quality,
                    int subsampling, int restart_blocks, uint8_t* out, size_t capacity, size_t* len);
int dfd_encode_jpeg_batch(dfd_handle* h, int n, const dfd_jpeg_source* images, uint8_t* out, size_t capacity, size_t* offsets,
                          size_t* lens, size_t* total);
int dfd_encode_jpeg_device(dfd_handle* h, int n, const dfd_jpeg_source* images, uint8_t* out, size_t capacity, size_t* offsets,
                           size_t* lens, size_t* total);

/* ---- one request, several consecutive frames of ONE stream (POST /analyze_batch) --------------
 * The per-frame flow of dfd_analyze_frame / dfd_analyze_jpeg (reference backend_server.py:139-164, executed once per
 * request there) for n frames in stream order with every stage batched: data[i] is a JPEG of len[i] bytes (entropy
 * decoding of the files in parallel on the library's host threads, IDCT / colour on the device) or, with len[i] = 0, a
 * packed BGR frame of height x width; all frames of a call share one size.  full_forensics[i]: the caller's full / fast
 * schedule (reference deepfake_detection.py:509-512).  The stream's temporal forensic state advances n frames.
 * Outputs: scores [n][6], forensic_prob [n], xywh [n][max_faces][4], n_faces [n] (boxes returned and classified),
 * n_detected [n] or NULL (len(faces) before the max_faces cut, backend_server.py:181), logits [n][max_faces] (NaN:
 * the MTCNN stage found no face), *height / *width or NULL.  Results equal n single calls in the same order.
 * DFD_ERR_UNSUPPORTED / DFD_ERR_ARG for a JPEG the device path does not decode: nothing of the stream's state has
 * moved yet (headers of all parts are parsed before any stage runs). */
int dfd_analyze_stream_batch(dfd_handle* h, int stream_id, int n, const uint8_t* const* data, const size_t* len, int height,
                             int width, const int* full_forensics, float conf_thr, int max_faces, int apply_clahe,
                             double* scores_out, double* forensic_prob_out, int32_t* xywh_out, int* n_faces_out,
                             int* n_detected_out, float* logits_out, int* height_out, int* width_out);

/* ---- one device pass over frames of MANY streams (the session pool; no reference counterpart) ----------------------
 * dfd_analyze_stream_batch for n frames of any streams and sizes: frame i belongs to stream stream_ids[i] (the frames of
 * one stream in stream order) and is a JPEG of len[i] bytes or, with len[i] = 0, a packed BGR frame of heights[i] x
 * widths[i] (heights / widths may be NULL when every part is a JPEG).  JPEG parts of one size are decoded as one batch;
 * frames under 30 px a side get forensics but no detection.  Outputs as dfd_analyze_stream_batch, per frame: scores
 * [n][6], forensic_prob [n], xywh [n][max_faces][4], n_faces [n], n_detected [n] or NULL, logits [n][max_faces],
 * height [n] / width [n] or NULL.  Per frame, bit for bit, the results (and every stream's state afterwards) equal those
 * of running each stream's frames alone, in order, through dfd_analyze_stream_batch / dfd_analyze_frame /
 * dfd_analyze_jpeg.  Every header is parsed and every check runs before anything moves: a part the device path does
 * not take fails the call (DFD_ERR_UNSUPPORTED for JPEG flavours, DFD_ERR_ARG for unreadable parts, among them scans
 * that are corrupt or cut off, found while decoding) with its index in *bad_index_out (NULL allowed); no stream state
 * has moved then.  More than 2^27 pixels in one call are refused with DFD_ERR_UNSUPPORTED and index -1.  The streams of
 * a call may hold different analysis sizes (dfd_forensics_open). */
int dfd_analyze_streams_batch(dfd_handle* h, int n, const uint8_t* const* data, const size_t* len, const int* heights,
                              const int* widths, const int* stream_ids, const int* full_forensics, float conf_thr, int max_faces,
                              int apply_clahe, double* scores_out, double* forensic_prob_out, int32_t* xywh_out, int* n_faces_out,
                              int* n_detected_out, float* logits_out, int* height_out, int* width_out, int* bad_index_out);

/* ---- many frames, resident in HBM (throughput path; BASELINE.json configs[2]/[3]) ----------
 * frames_dev: n packed 8-bit BGR frames of height x width on the handle's device (row stride
 * width*3).  Runs the detector on all frames in one launch set; then, per frame, classifies
 * either the detected boxes (forced_xywh == NULL, at most max_faces) or the caller's forced_k
 * boxes per frame (forced_xywh: n*forced_k quadruples - used by the benchmark so that the crop
 * workload does not depend on what a random-weight detector fires on).  with_forensics != 0 also
 * computes the stateless six-signal probability of every frame.
 *   xywh_out [n][max_faces][4], n_faces_out [n], logits_out [n][max_faces], forensic_prob_out [n]. */
int dfd_analyze_batch_device(dfd_handle* h, const uint8_t* frames_dev, int n, int height, int width,
                             const int32_t* forced_xywh, int forced_k, float conf_thr, int max_faces,
                             int apply_clahe, int with_forensics, int32_t* xywh_out, int* n_faces_out,
                             float* logits_out, double* forensic_prob_out);

/* ---- many frames from host memory, upload overlapped with compute ---------------------------------------------
 * The PCIe-inclusive form of dfd_analyze_batch_device: n_total packed BGR frames in host memory (ideally from
 * dfd_host_alloc = pinned, so that the copies run asynchronously) are processed `batch` at a time; batch k + 1 is
 * uploaded on a second HIP stream while batch k is analysed.  Output arrays are sized for n_total frames. */
int dfd_host_alloc(dfd_handle* h, size_t bytes, void** ptr);
int dfd_host_free(dfd_handle* h, void* ptr);
int dfd_analyze_frames_host(dfd_handle* h, const uint8_t* frames_host, int n_total, int batch, int height, int width,
                            const int32_t* forced_xywh, int forced_k, float conf_thr, int max_faces, int apply_clahe,
                            int with_forensics, int32_t* xywh_out, int* n_faces_out, float* logits_out,
                            double* forensic_prob_out);

/* ---- frame-sharded streams (BASELINE.json configs[4]) ------------------------------
 * With frame t of a stream on rank t % G, the only state that crosses frames is the vote window (reference
 * deepfake_detection.py:111-118) and the analyzer's temporal signal (reference frame_analysis.py:349-389: the
 * previous gray frame and the last 30 mean differences).  A rank therefore computes, for each of its frames,
 * the five stateless signals and the mean absolute gray difference against the frame's predecessor (which it
 * also holds: recomputed, not communicated), all ranks exchange fixed-size records with ONE all-gather per wave,
 * and every rank replays temporal score, weighted sum and vote in frame order (host: streams.py).
 *
 * dfd_forensic_signals_device: n packed BGR frames resident in HBM; prev_index[f] = index (inside this batch) of
 * frame f's predecessor, -1 (none), or -2: frame f is itself only a predecessor - it gets a gray plane and no
 * signals (its outputs are set to -1); such frames must form the tail of the batch.  scores5_out [n][5] =
 * frequency, noise, ela, edge, color (all five computed; the caller drops noise/ela/color on "fast" frames);
 * mean_diff_out [n] = mean |gray - gray_prev| or -1. */
int dfd_forensic_signals_device(dfd_handle* h, const uint8_t* frames_dev, int n, int height, int width,
                                const int32_t* prev_index, double* scores5_out, double* mean_diff_out);

/* Vote exchange over RCCL (xGMI inside a node).  Rank 0 obtains an id (ncclGetUniqueId) and hands its
 * DFD_COMM_ID_BYTES bytes to the other ranks by any host channel (file, socket, torch.distributed store); every
 * rank then calls dfd_comm_init on its handle.  dfd_vote_allgather copies `bytes_per_rank` bytes of records
 * to the device, runs ONE ncclAllGather on the handle's stream and returns all ranks' blocks, rank-major, in
 * host memory (world * bytes_per_rank bytes): the collective named in SURVEY 8(b)/(e).  librccl is opened on
 * first use (DFD_RCCL_LIB overrides the name); without it these three return DFD_ERR_STATE. */
#define DFD_COMM_ID_BYTES 128
int dfd_comm_unique_id(void* id_out);
int dfd_comm_init(dfd_handle* h, const void* id, int rank, int world);
int dfd_comm_destroy(dfd_handle* h);
int dfd_comm_info(const dfd_handle* h, int* rank, int* world);      /* world = 0: no communicator */
int dfd_vote_allgather(dfd_handle* h, const void* local_records, size_t bytes_per_rank, void* all_records_out);
/* `waves` consecutive waves in one call: one upload of [waves][bytes_per_rank], one ncclAllGather PER WAVE (slot w of
 * all_records_out = [world][bytes_per_rank] of wave w), one download, one stream wait. */
int dfd_vote_allgather_waves(dfd_handle* h, const void* local_records, int waves, size_t bytes_per_rank, void* all_records_out);

/* ---- classifier head training ---------------------------------------------------------------
 * The reference's training recipe (train.py: FocalLoss :360-392, mixup_criterion :352-354, AdamW :910, gradient
 * clipping and accumulation :587-605, EMAModel :398-416) for the 1280 -> 512 -> 256 -> 1 head (model.py:50-61) on the
 * pooled features dfd_extract_features returns; the backbone stays frozen.  fp32 throughout (no AMP).  A trainer hangs
 * off the handle between begin and end (dfd_destroy ends an open one), is single-caller like the handle and touches
 * nothing the inference entries read until dfd_head_train_commit.  Calling anything but begin without an open
 * trainer, a second begin, max_n outside 2..256, dropout outside [0,1), n > max_n, and n < 2 in accumulate
 * (BatchNorm1d's batch statistics need two rows) are DFD_ERR_ARG; host memory running out is DFD_ERR_CAPACITY, a failed
 * device allocation DFD_ERR_HIP.  All pointers are host memory.
 * dfd_head_train_begin also refuses, with DFD_ERR_ARG: a NaN or an infinity in any float field of the config; beta1 /
 * beta2 outside [0, 1); eps or clip_norm <= 0; ema_decay, bn_momentum or label_smoothing outside [0, 1]; a negative
 * focal_gamma; a negative weight_decay (as torch.optim.AdamW does).  Both ends of every closed range are legal, and
 * any finite focal_alpha is (the reference's FocalLoss takes any).  dfd_head_train_apply refuses a NaN or negative lr;
 * dfd_head_train_accumulate, _accumulate_trunk and _accumulate_block refuse a NaN lam or loss_scale and a lam outside
 * [0, 1].  A refused call leaves the trainer (or, for begin, the handle without one) as it was.
 *
 * Dropout keep masks are a stateless hash of (seed, accumulate counter since begin, layer 0..2, row * width + col)
 * compared against floor(p * 2^32); head_training.dropout_keep_mask (Python, numpy) is its specification and the
 * kernels reproduce it bit for bit.  Layer rates: dropout, 0.7 dropout, 0.5 dropout (as doubles of the float). */
typedef struct dfd_head_params {      /* torch layouts: w [out][in]; g / be = BatchNorm1d weight / bias; rm / rv = running stats */
    float *w1, *b1, *g1, *be1, *rm1, *rv1, *w2, *b2, *g2, *be2, *rm2, *rv2, *w3, *b3;
} dfd_head_params;
typedef struct dfd_head_config {
    int max_n;                         /* rows of one accumulate / eval call, 2..256 */
    unsigned long long seed;
    float dropout, beta1, beta2, eps, weight_decay, focal_gamma, focal_alpha, label_smoothing, clip_norm, ema_decay,
        bn_momentum;
} dfd_head_config;
/* train.py's argparse defaults: max_n 32, seed 0, dropout 0.5, weight_decay 0.05, focal 2.0 / 0.25, label_smoothing 0.1,
 * ema_decay 0.999; clip_norm 1.0, betas 0.9 / 0.999, eps 1e-8 (torch.optim.AdamW), bn_momentum 0.1 */
void dfd_head_config_default(dfd_head_config* cfg);
/* uploads the unfolded head (every pointer of `init` required); EMA shadow = the parameters, moments and gradients 0 */
int dfd_head_train_begin(dfd_handle* h, const dfd_head_params* init, const dfd_head_config* cfg);
/* train-mode forward (batch statistics, running statistics updated), loss = lam FL(z, labels_a) + (1 - lam) FL(z, labels_b)
 * (labels_b NULL: FL(z, labels_a)), mean over the n rows, and the backward of loss * loss_scale ADDED to the gradient
 * buffer.  *loss_out: the unscaled loss; logits_out [n] or NULL. */
int dfd_head_train_accumulate(dfd_handle* h, const float* feat, int n, const float* labels_a, const float* labels_b,
                              float lam, float loss_scale, float* loss_out, float* logits_out);
/* clip_grad_norm_ (coef = min(1, clip_norm / (norm + 1e-6))), torch.optim.AdamW's step with the given learning rate on
 * every trainable tensor (one group: biases and BN gamma / beta decay too), EMA update, gradients zeroed.
 * *grad_norm_out (or NULL): the global L2 norm before clipping. */
int dfd_head_train_apply(dfd_handle* h, float lr, float* grad_norm_out);
/* eval-mode forward (running statistics, no dropout) of n <= max_n rows on the live or the EMA parameters */
int dfd_head_train_eval(dfd_handle* h, const float* feat, int n, int use_ema, float* logits_out);
/* parameters (live or EMA) and the live running statistics into the caller's arrays */
int dfd_head_train_export(dfd_handle* h, int use_ema, dfd_head_params* out);
/* test tap: read (set = 0) or replace (set = 1) the accumulated gradients; rm / rv are not used */
int dfd_head_train_grads(dfd_handle* h, dfd_head_params* io, int set);
/* test tap of the last accumulate: "mask0" [n][1280], "mask1" [n][512], "mask2" [n][256] (1.0 = kept), "z1" [n][512],
 * "z2" [n][256] (BatchNorm outputs before ReLU), "x0" [n][1280], "a1" [n][512], "a2" [n][256] (what the three
 * Linear layers read: the features and relu(z) after dropout; a1 / a2 hold until the next eval call overwrites them).
 * capacity in floats; too small: DFD_ERR_ARG */
int dfd_head_train_tap(dfd_handle* h, const char* name, float* out, size_t capacity);
/* folds BatchNorm into fc1 / fc2 (float64 on the host, rounded once: weights._fold) and overwrites the tensors the
 * inference plan reads, on the handle's stream; the cached bf16 splits of fc1.w / fc2.w are rebuilt in place.  From
 * the next call on, every classify / fused / Grad-CAM entry of this handle uses the new head. */
int dfd_head_train_commit(dfd_handle* h, int use_ema);
int dfd_head_train_end(dfd_handle* h);

/* ---- train-time image augmentation ------------------------------------------------------------
 * The reference's training transform (train.py:462-489, 298-349) on `n` uint8 RGB crops of one size H x W (multiples
 * of 16 in 32..512): Pillow's bilinear Resize to (T + 20)^2, RandomCrop to T x T and flip, ColorJitter in a per-image
 * order, RandomGrayscale, RandomRotation, RandomAffine, RandomPerspective, GaussianBlur, ToTensor + Normalize,
 * RandomErasing, GaussianNoise and Mixup / CutMix over the batch, T = out_size (12..492).  The host draws every
 * parameter (train_augment.draw_batch) and passes one row per image; the kernels draw nothing but the noise, a
 * stateless hash of (seed, counter, image, element) specified by train_augment.noise_normal.  A stage whose flag is
 * clear leaves the image bit-identical; an image without DFD_AUG_CROP is resized straight to T x T (the reference's
 * validation transform).  The chain opens with the reference's JPEG round trip (DFD_AUG_JPEG, train.py:282-295): libjpeg
 * as cv2 runs it - 4:2:0, Annex K tables scaled by the quality, islow DCT, fancy upsampling - without the lossless
 * entropy coding.  The reference hands its RGB array to an encoder that reads BGR, so its result is the round trip of
 * the channel-reversed image; DFD_AUG_JPEG_RGB asks for the round trip of the image itself instead.  Sizes outside the
 * ranges above, n < 1, a quality outside 1..100, an unknown jitter op, an erase box outside the image and a mix
 * permutation outside 0..n-1 are DFD_ERR_ARG; nothing is kept from a refused call. */
enum {
    DFD_AUG_JPEG = 1, DFD_AUG_CROP = 2, DFD_AUG_FLIP = 4, DFD_AUG_GRAY = 8, DFD_AUG_ROTATE = 16, DFD_AUG_AFFINE = 32,
    DFD_AUG_PERSPECTIVE = 64, DFD_AUG_BLUR = 128, DFD_AUG_ERASE = 256, DFD_AUG_NOISE = 512, DFD_AUG_JPEG_RGB = 1024
};
enum { DFD_JITTER_NONE = 0, DFD_JITTER_BRIGHTNESS = 1, DFD_JITTER_CONTRAST = 2, DFD_JITTER_SATURATION = 3, DFD_JITTER_HUE = 4 };
enum { DFD_MIX_NONE = 0, DFD_MIX_MIXUP = 1, DFD_MIX_CUTMIX = 2 };
typedef struct dfd_train_aug_image {
    double rotate[6];               /* inverse matrix of Image.rotate (NEAREST, fill 0)                              */
    double affine[6];               /* inverse matrix of RandomAffine (NEAREST, fill 0)                              */
    double perspective[8];          /* Pillow PERSPECTIVE coefficients (BILINEAR, fill 0)                            */
    unsigned int flags;             /* DFD_AUG_*                                                                     */
    int jpeg_quality;               /* 1..100                                                                        */
    int crop_x, crop_y;             /* RandomCrop offset inside the (T + 20)^2 image, 0..20                          */
    int jitter_op[4];               /* DFD_JITTER_* of the four ColorJitter slots, in the order they run             */
    float jitter_factor[4];
    float blur_k[2];                /* float32 normalised Gaussian: outer tap, centre tap                            */
    int erase[4];                   /* x, y, w, h of the erased rectangle                                            */
    float noise_std;
    int reserved;
} dfd_train_aug_image;
typedef struct dfd_train_aug_batch {
    unsigned long long seed, counter;   /* noise key                                                                 */
    const int* perm;                    /* partner of every image (n entries); NULL allowed when mix_kind = 0        */
    int mix_kind;                       /* DFD_MIX_*                                                                 */
    float lam;                          /* Mixup: lam x + (1 - lam) x[perm]                                          */
    int box[4];                         /* CutMix: x1, y1, x2, y2 (exclusive) copied from the partner                */
} dfd_train_aug_batch;
/* the chain alone: rgb_host [n][H][W][3] -> nchw_out_host [n][3][T][T] float32 */
int dfd_train_augment(dfd_handle* h, const unsigned char* rgb_host, int n, int H, int W, int out_size,
                      const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, float* nchw_out_host);
/* the chain at T = 224 on all n images, then the backbone in chunks of max_batch -> feat_out_host [n][1280].  Only the
 * uint8 crops are uploaded; on_device = 1: `rgb` is device memory (dfd_device_alloc), e.g. a resident training set. */
int dfd_train_augment_features(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                               const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, float* feat_out_host);
/* crops idx[0 .. n) (host ints, each in 0 .. n_src - 1) of a resident set rgb_dev [n_src][H][W][3] -> out_dev [n][H][W][3],
 * both device memory (dfd_device_alloc), enqueued on the handle's stream: the shuffled batch of a training set that stays
 * in HBM, ready for dfd_train_augment_features(on_device = 1).  An index out of range is DFD_ERR_ARG. */
int dfd_train_augment_gather(dfd_handle* h, const unsigned char* rgb_dev, int n_src, int H, int W, const int* idx, int n,
                             unsigned char* out_dev);
/* test tap of the noise hash, on the host: the two uint32 words behind elements first .. first + count - 1 of image `row`
 * (the functions the noise kernel calls; train_augment.noise_words is their specification).  No handle, no GPU. */
int dfd_train_augment_noise_words(unsigned long long seed, unsigned long long counter, int row, unsigned int first,
                                  unsigned int count, unsigned int* u1_out, unsigned int* u2_out);
/* test tap: the images after the named stage - "jpeg" uint8 [n][H][W][3], "resize" uint8 [n][(T+20)^2 * 3] slots (an image without DFD_AUG_CROP
 * fills the first T * T * 3 bytes of its slot), "crop", "jitter0".."jitter3", "gray", "rotate", "affine", "perspective",
 * "blur" uint8 [n][T][T][3]; "norm", "erase", "noise", "mix" float32 [n][3][T][T].  capacity in bytes. */
int dfd_train_augment_tap(dfd_handle* h, const unsigned char* rgb_host, int n, int H, int W, int out_size,
                          const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, const char* stage_name,
                          void* out, size_t capacity);

/* ---- fine-tuning the head conv with the head ----------------------------------------------------
 * The first layer of the reference's unfrozen backbone group (train.py:863-924): net._conv_head (320 -> 1280, 1 x 1, no
 * bias), net._bn1 in train mode, swish and the 7 x 7 average pool, trained together with the MLP head as a second AdamW
 * group at lr * lr_scale.  Its input is block 15's output, "trunk rows": float32 NHWC [n][7][7][320] (15680 floats a crop). */
#define DFD_TRUNK_ROW 15680   /* 7 * 7 * 320 floats of one crop */

/* the forward up to block 15's output -> trunk_host [n][7][7][320]; equals dfd_b0_tap(.., "b15.out") bit for bit (under
 * "bf16_activations": the stored bf16 values, widened).  n as dfd_extract_features. */
int dfd_extract_trunk(dfd_handle* h, const float* nchw_host, int n, float* trunk_host);
/* dfd_train_augment_features with trunk rows in place of pooled rows -> trunk_out_host [n][7][7][320] */
int dfd_train_augment_trunk(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                            const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, float* trunk_out_host);

typedef struct dfd_headconv_params {   /* torch layouts: w [1280][320] (the 1 x 1 kernel), g / be = BatchNorm2d weight / bias, rm / rv = running stats */
    float *w, *g, *be, *rm, *rv;
} dfd_headconv_params;
/* Adds the conv stage to an open trainer: legal once, after dfd_head_train_begin and before the first accumulate
 * (anything else: DFD_ERR_ARG).  Allocates everything the stage needs for max_n crops.  The Python side passes lr_scale
 * 0.1, bn_momentum 0.01 and bn_eps 1e-3 (efficientnet_pytorch's; the float 1e-3f stands for weights._fold's double 1e-3).
 * From here on dfd_head_train_accumulate / _eval (pooled rows) are DFD_ERR_ARG and the _trunk entries take their place;
 * dfd_head_train_apply takes ONE gradient norm over both groups and steps the head at lr, w / g / be at lr * lr_scale
 * (product in double; same betas, eps, weight decay; EMA and zeroing cover both); dfd_head_train_commit also folds
 * _bn1 into _conv_head (float64, rounded once) and overwrites head.w / head.b and the cached split of head.w in place;
 * dfd_head_train_tap knows "cfeat" [n][1280] (pooled features), "dfeat" [n][1280] (their gradient) and "cz"
 * [n][49][1280] (the BatchNorm output before swish).  The stage has no dropout of its own. */
int dfd_head_train_unfreeze_conv(dfd_handle* h, const dfd_headconv_params* init, float lr_scale, float bn_momentum, float bn_eps);
/* dfd_head_train_accumulate on n trunk rows (2 <= n <= max_n): BatchNorm2d batch statistics over the 49 n positions */
int dfd_head_train_accumulate_trunk(dfd_handle* h, const float* trunk, int n, const float* labels_a, const float* labels_b,
                                    float lam, float loss_scale, float* loss_out, float* logits_out);
/* dfd_head_train_eval on n trunk rows (1 <= n <= max_n): running statistics; per row, so any chunking gives the same bits */
int dfd_head_train_eval_trunk(dfd_handle* h, const float* trunk, int n, int use_ema, float* logits_out);
/* w / g / be (live or EMA) and the live running statistics into the caller's arrays */
int dfd_head_train_export_conv(dfd_handle* h, int use_ema, dfd_headconv_params* out);
/* test tap, as dfd_head_train_grads: read (set = 0) or replace (set = 1) the gradients of w / g / be; rm / rv are not used */
int dfd_head_train_conv_grads(dfd_handle* h, dfd_headconv_params* io, int set);

/* ---- fine-tuning block 15 with the head conv and the head ---------------------------------------
 * The last block of the backbone, net._blocks.15 (MBConv k3, 192 -> 1152 -> 320, squeeze-excite 48, 7 x 7, no skip), in
 * train mode in front of the conv stage: its three BatchNorm2d layers use batch statistics.  Its input is block 14's
 * output: float32 NHWC [n][7][7][192] (9408 floats a crop). */
#define DFD_BLOCK14_ROW 9408   /* 7 * 7 * 192 floats of one crop */

/* dfd_extract_trunk / dfd_train_augment_trunk with the block whose output is returned: 15 gives the bits of those two,
 * 14 gives [n][7][7][192], the "b14.out" tap of the same forward.  Any other block: DFD_ERR_ARG. */
int dfd_extract_trunk_at(dfd_handle* h, const float* nchw_host, int n, int block, float* out_host);
int dfd_train_augment_trunk_at(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                               const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, int block, float* out_host);

typedef struct dfd_mbconv_params {   /* torch layouts: exp_w [1152][192], dw_w [1152][3][3], se_w1 [48][1152], se_b1 [48], se_w2 [1152][48],
                                        se_b2 [1152], proj_w [320][1152]; g / be / rm / rv of _bn0, _bn1 (1152) and _bn2 (320) */
    float *exp_w, *dw_w, *se_w1, *se_b1, *se_w2, *se_b2, *proj_w;
    float *g0, *be0, *rm0, *rv0, *g1, *be1, *rm1, *rv1, *g2, *be2, *rm2, *rv2;
} dfd_mbconv_params;
/* Adds block `block` to an open trainer: legal once, after dfd_head_train_unfreeze_conv and before the first accumulate
 * (anything else: DFD_ERR_ARG); `block` must be the last block, 15 (any other: DFD_ERR_UNSUPPORTED).  Allocates everything
 * the stage needs for max_n crops in one piece.  The Python side passes bn_momentum 0.01 and bn_eps 1e-3.  The block's 717 232
 * floats are a third arena that steps with the conv stage's lr_scale.  From here on the pooled and the _trunk entries are
 * DFD_ERR_ARG and the _block entries take their place; dfd_head_train_apply takes ONE gradient norm over the three
 * arenas (their partial sums added entry by entry: head, conv, block) and one clip coefficient, with the same betas, eps
 * and weight decay on every tensor; EMA and zeroing cover all three; dfd_head_train_commit also folds the block's three
 * BatchNorms (float64, rounded once) and overwrites the ten b15.* tensors and their cached splits in place;
 * dfd_head_train_tap knows "b15.out" [n][49][320] (BN2's output), "b15.gate" [n][1152], "b15.ad" [n][49][1152] (the
 * depthwise activation), "b15.dout" [n][49][320] (the gradient of b15.out) and "b15.dae" [n][49][1152] (the gradient of
 * the expand activation).  Block 14 stays frozen: no gradient leaves the stage. */
int dfd_head_train_unfreeze_block(dfd_handle* h, int block, const dfd_mbconv_params* init, float bn_momentum, float bn_eps);
/* dfd_head_train_accumulate on n input rows of the deepest unfrozen block (2 <= n <= max_n): block 14's output, or, once
 * block 14 is unfrozen (dfd_head_train_unfreeze_block_at, below), block 13's */
int dfd_head_train_accumulate_block(dfd_handle* h, const float* rows, int n, const float* labels_a, const float* labels_b,
                                    float lam, float loss_scale, float* loss_out, float* logits_out);
/* dfd_head_train_eval on n such rows (1 <= n <= max_n): running statistics; per row, so any chunking gives the same bits */
int dfd_head_train_eval_block(dfd_handle* h, const float* rows, int n, int use_ema, float* logits_out);
/* the trainable tensors (live or EMA) and the live running statistics into the caller's arrays */
int dfd_head_train_export_block(dfd_handle* h, int use_ema, dfd_mbconv_params* out);
/* test tap: read (set = 0) or replace (set = 1) the gradients of the trainable tensors; rm / rv are not used */
int dfd_head_train_block_grads(dfd_handle* h, dfd_mbconv_params* io, int set);

/* ---- frequency-domain analysis at any size -------------------------------------------------------
 * The reference's GAN-artefact check (deepfake_detection.py:457-487) on face windows at their own h x w, and
 * compute_frequency_features (model.py:105-149) at any even size: a rectangular, ragged, batched DFT and an orthonormal
 * DCT-II on the fp32 MFMA.  Sides are 1..4096. */
#define DFD_FREQ_MAX_SIDE 4096
#define DFD_FREQ_MAX_FEATURE_SIZE 1024

/* n windows boxes[n][4] = (x, y, w, h) of one uint8 frame [hh][ww][channels] (channels 3 = BGR, converted with cv2's
 * integer gray formula; 1 = gray; stride in bytes); boxes == NULL: the whole image, n = 1.  out[n][2] = (high, total):
 * the sum of |X| over the window's 2-D spectrum outside the central mask, and over all of it.  The mask is the
 * reference's slice of the shifted spectrum: with m = min(h, w) / 4 and the signed frequency s = k (k < ceil(N / 2)) or
 * k - N, a bin is masked when both of its s lie in [-m, m).  One launch set serves all windows (several when their work
 * memory exceeds the "forensic_chunk_bytes" budget); a window gives the same bits alone and among others.
 * A box that leaves the frame or has a side of 0: DFD_ERR_ARG; a side above 4096: DFD_ERR_UNSUPPORTED. */
int dfd_frequency_domain(dfd_handle* h, const unsigned char* img, int hh, int ww, int stride, int channels,
                         const int32_t* boxes, int n, double* out);
/* the same on a frame that is resident on the device, on the handle's stream; boxes and out are host memory */
int dfd_frequency_domain_device(dfd_handle* h, const unsigned char* img_dev, int hh, int ww, int stride, int channels,
                                const int32_t* boxes, int n, double* out);
/* test tap: the launches of dfd_frequency_domain on one gray window gray[hh][ww] (packed) -> the named buffer:
 * "rows" the pass-1 output, complex float [ww][hh] (transform along x, stored transposed); "spectrum" complex float
 * [ww][hh] ([kx][ky], the layout the kernels use); "mag" float [ww][hh], the magnitudes as summed; "sums" two doubles
 * (high, total).  capacity in bytes. */
int dfd_frequency_domain_tap(dfd_handle* h, const unsigned char* gray, int hh, int ww, const char* name, void* out,
                             size_t capacity);
/* dfd_frequency_features at any even size in 2..1024 (anything else: DFD_ERR_ARG) -> out [2][size][size]; the size-224
 * entry above keeps its own kernels */
int dfd_frequency_features_sized(dfd_handle* h, const unsigned char* img, int hh, int ww, int stride, int channels, int size,
                                 float* out);
/* test tap of the same launches: "gray" uint8 [size][size] after the resize; "spectrum" complex float [kx][ky],
 * unshifted; "dct" float [ky][kx], the coefficients before log1p.  capacity in bytes. */
int dfd_frequency_features_tap(dfd_handle* h, const unsigned char* img, int hh, int ww, int stride, int channels, int size,
                               const char* name, void* out, size_t capacity);

/* ---- fine-tuning block 14 with block 15, the head conv and the head -----------------------------
 * net._blocks.14 (MBConv k5, stride 1, pad 2 / 2, 192 -> 1152 -> 192, squeeze-excite 48, 7 x 7) in train mode in front of
 * block 15's stage: out = x13 + drop_connect(BN2(project(..))), efficientnet_pytorch's per-crop drop-connect.  Its input
 * is block 13's output, float32 NHWC [n][7][7][192]: DFD_BLOCK14_ROW floats a crop again.
 * In dfd_mbconv_params block 14's shapes are those of block 15 except dw_w [1152][5][5], proj_w [192][1152] and g2 / be2 /
 * rm2 / rv2 [192]: 587 952 trainable floats.
 *
 * dfd_head_train_unfreeze_block_at adds block `block` below block 15: `block` must be 14, or 13 or 12 under the rules of
 * the next section (any other: DFD_ERR_UNSUPPORTED); legal once, after dfd_head_train_unfreeze_block and before the first accumulate (anything else:
 * DFD_ERR_ARG); a null field, bn_momentum outside [0, 1], bn_eps <= 0, drop_connect outside [0, 1) or NaN: DFD_ERR_ARG.
 * One hipMalloc holds everything the stage needs for max_n crops; it is freed with the trainer and no later call
 * allocates.  The Python side passes bn_momentum 0.01, bn_eps 1e-3 and drop_connect 0.2 * 14 / 16 (efficientnet-b0's
 * drop_connect_rate times idx / len(blocks)).
 * From here on the rows of dfd_head_train_accumulate_block / _eval_block are the input rows of the deepest unfrozen
 * block: block 13's output.  A train-mode forward keeps crop i's branch with probability keep_prob = 1 - p, p the double
 * of the float32 drop_connect: out = x13 + (y / keep_prob) b_i, b_i = head_training.dropout_keep_mask(seed, counter,
 * layer = 3, n, width = 1, p)[i]; a dropped crop's output is its input row bit for bit, and it still counts in the batch
 * statistics and running updates of the block's BatchNorms, which come before the mask.  Eval applies no drop-connect.
 * Block 15 hands dOut14 = dZe15 . We15 down; BN2's gradient source is dOut14 b_i / keep_prob; while block 13 is frozen
 * no gradient leaves block 14.  dfd_head_train_apply takes ONE gradient norm over the four arenas (partial sums added
 * entry by entry: head, conv, block 15, block 14) and one clip coefficient; block 14 steps at lr * lr_scale with the same
 * betas, eps and weight decay; EMA and zeroing cover it.  dfd_head_train_commit also folds block 14's three BatchNorms
 * (float64, rounded once; dw.w re-laid [ky][kx][c] with 25 taps, se.w2 transposed) and overwrites the ten b14.* tensors
 * and the cached splits of b14.exp.w and b14.proj.w in place.
 * dfd_head_train_tap additionally knows "b14.out" [n][49][192] (the block's output after the skip: block 15's input),
 * "b14.gate" [n][1152], "b14.ad" [n][49][1152], "b14.keep" [n] (the factor applied to each crop's branch, 0 or
 * 1 / keep_prob), "b14.dout" [n][49][192] (the gradient arriving at b14.out) and "b14.dae" [n][49][1152]; without the
 * stage they are DFD_ERR_ARG.  A trainer without the stage launches exactly what it launched before. */
int dfd_head_train_unfreeze_block_at(dfd_handle* h, int block, const dfd_mbconv_params* init, float bn_momentum, float bn_eps,
                                     float drop_connect);
/* dfd_head_train_export_block / _block_grads for block 12 .. 15 (15: the bits of those two); any other block:
 * DFD_ERR_UNSUPPORTED; block 14 or 15 while it is not unfrozen: DFD_ERR_ARG; block 13 or 12 while it is not unfrozen:
 * DFD_ERR_UNSUPPORTED */
int dfd_head_train_export_block_at(dfd_handle* h, int block, int use_ema, dfd_mbconv_params* out);
int dfd_head_train_block_grads_at(dfd_handle* h, int block, dfd_mbconv_params* io, int set);
/* dfd_extract_trunk_at / dfd_train_augment_trunk_at for block 13, 14 or 15: 14 and 15 give the bits of those entries, 13
 * gives [n][7][7][192], the "b13.out" tap of the same forward.  Any other block: DFD_ERR_ARG. */
int dfd_extract_block_out(dfd_handle* h, const float* nchw_host, int n, int block, float* out_host);
int dfd_train_augment_block_out(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                                const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, int block, float* out_host);

/* ---- fine-tuning blocks 13 and 12 below block 14 ------------------------------------------------
 * net._blocks.13 and net._blocks.12 have block 14's geometry exactly (MBConv k5, stride 1, pad 2 / 2, 192 -> 1152 -> 192,
 * squeeze-excite 48, 7 x 7, identity skip, 587 952 trainable floats, the shapes of block 14 in dfd_mbconv_params) and run
 * block 14's launches on a state of their own: after them every 7 x 7 block of the reference's unfrozen group trains.
 *
 * dfd_head_train_unfreeze_block_at takes the blocks from the top down, before the first accumulate: 13 once 14 is
 * unfrozen, 12 once 13 is.  13 or 12 while the block above it is frozen: DFD_ERR_UNSUPPORTED; a block that is already
 * unfrozen, or any block after an accumulate: DFD_ERR_ARG; blocks outside 12..14: DFD_ERR_UNSUPPORTED.  Each stage is
 * ONE hipMalloc at max_n, freed with the trainer.  The Python side passes drop_connect 0.2 * b / 16: 0.175, 0.1625, 0.15.
 * The rows of dfd_head_train_accumulate_block / _eval_block are the input rows of the deepest unfrozen block (block 12's
 * or block 11's output; dfd_extract_block_input below).  Block b writes out = x_(b-1) + (BN2(Zp) / keep_prob_b) b_i
 * into block b + 1's input; its mask is head_training.dropout_keep_mask(seed, counter, layer = 17 - b, n, 1, p_b): 3 for
 * block 14, 4 for 13, 5 for 12, so the blocks drop independently.  A trained skip block with a trained block below it
 * hands down dX_b = dOut_b + dZe_b . We_b, the sum formed in double and rounded once; the deepest trained block hands
 * nothing down, and a trainer whose deepest block is 14 launches exactly what it launched before.  A dropped crop's
 * branch still receives a gradient through the batch statistics of the other crops; only when every crop of block b is
 * dropped are block b's gradients exactly 0 and dX_b == dOut_b element for element.
 * dfd_head_train_apply takes ONE norm over up to six arenas (partial sums added entry by entry: head, conv, 15, 14, 13,
 * 12); EMA, zeroing and dfd_head_train_commit (15, 14, 13, 12 in that order; the ten b13.* / b12.* tensors and their two
 * cached splits rewritten in place) cover every stage.  dfd_head_train_tap knows "b13.*" and "b12.*" with block 14's six
 * names (out, gate, ad, keep, dout, dae); without the stage they are DFD_ERR_ARG.
 *
 * dfd_extract_block_input / dfd_train_augment_block_input: the input rows of block `block` in 12..15, [n][7][7][192],
 * the "b{block-1}.out" tap of the same forward; for 14 and 15 the bits of dfd_extract_block_out /
 * dfd_train_augment_block_out at block - 1 (those entries serve the outputs of blocks 13..15).  Any other block: DFD_ERR_ARG.  n and capacity as those entries. */
int dfd_extract_block_input(dfd_handle* h, const float* nchw_host, int n, int block, float* out_host);
int dfd_train_augment_block_input(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                                  const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, int block, float* out_host);

/* ---- fine-tuning block 11, the stride-2 block below block 12 ------------------------------------
 * net._blocks.11 is the MBConv that takes the 14 x 14 maps to 7 x 7: expand 112 -> 672, depthwise 5 x 5 at stride 2 with
 * TF-"SAME" padding 1 before and 2 after on both axes (output (oy, ox) reads input (2 oy - 1 + ky, 2 ox - 1 + kx)),
 * squeeze-excite 28, projection 672 -> 192, no skip and therefore no drop-connect; 262 492 trainable floats.  In
 * dfd_mbconv_params: exp_w [672][112], dw_w [672][5][5], se_w1 [28][672], se_b1 [28], se_w2 [672][28], se_b2 [672],
 * proj_w [192][672], BatchNorms of 672, 672 and 192 channels.  Blocks 10 and 9 stay frozen.
 *
 * dfd_head_train_unfreeze_block_at also takes block 11, once 12 is unfrozen and before the first accumulate, with
 * drop_connect 0 (anything else: DFD_ERR_ARG).  11 while 12 is frozen: DFD_ERR_UNSUPPORTED; 11 again, or after an
 * accumulate: DFD_ERR_ARG; blocks outside 11..14: DFD_ERR_UNSUPPORTED.  dfd_head_train_export_block_at / _block_grads_at
 * serve 11 once it is unfrozen (frozen: DFD_ERR_UNSUPPORTED).  The stage is ONE hipMalloc at max_n.  The rows of
 * dfd_head_train_accumulate_block / _eval_block are then block 10's output, float32 NHWC [n][14][14][112]:
 * DFD_BLOCK11_INPUT_ROW floats a crop.  BatchNorm 0 takes its statistics over 196 n rows, BatchNorms 1 and 2 and the
 * squeeze-excite pool over 49 n.  Block 11 writes BN2(Zp) into block 12's input; block 12 hands down
 * dX12 = dOut12 + dZe12 . We12 as every trained skip block does, and block 11 forms no input gradient.
 * dfd_head_train_apply takes ONE norm over up to seven arenas (head, conv, 15, 14, 13, 12, 11); EMA, zeroing and
 * dfd_head_train_commit (15 .. 11 in that order) cover the stage.  dfd_head_train_tap knows "b11.out" [n][49][192] (block
 * 12's input), "b11.gate" [n][672], "b11.ad" [n][49][672], "b11.dout" [n][49][192] and "b11.dae" [n][196][672]; there is no
 * "b11.keep" (DFD_ERR_ARG), and every "b11.*" tap without the stage is DFD_ERR_ARG.
 *
 * dfd_extract_block_rows / dfd_train_augment_block_rows: dfd_extract_block_input / dfd_train_augment_block_input (their
 * bits for `block` in 12..15) with block 11 as well, whose rows are [n][14][14][112], the "b10.out" tap of the same
 * forward (fp32 and bf16-activation mode).  Any other block: DFD_ERR_ARG.  The two older entries keep refusing 11. */
#define DFD_BLOCK11_INPUT_ROW 21952   /* 14 * 14 * 112 floats of one crop */
int dfd_extract_block_rows(dfd_handle* h, const float* nchw_host, int n, int block, float* out_host);
int dfd_train_augment_block_rows(dfd_handle* h, const unsigned char* rgb, int on_device, int n, int H, int W,
                                 const dfd_train_aug_image* rows, const dfd_train_aug_batch* batch, int block, float* out_host);

#ifdef __cplusplus
}
#endif
#endif /* DFD_HIP_H */
