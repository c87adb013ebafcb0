// Shared host-side pieces of libdfd_hip.so: status plumbing, the weights-blob reader and
// the handle.  Nothing here crosses the C ABI; include/dfd_hip.h is the public surface.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/dfd_hip.h"
#include "blob_reader.h"
#include "imgproc_kernels.h"

namespace dfd {

struct ForensicState;   // forensic_api.hip
void forensic_destroy(dfd_handle* h);
struct FreqState;       // freq_kernels.hip
void freq_destroy(dfd_handle* h);
struct FreqDomainState; // freq_domain.hip
void freq_domain_destroy(dfd_handle* h);
struct SsdState;        // ssd_api.hip
int ssd_init(dfd_handle* h);
void ssd_destroy(dfd_handle* h);
int ssd_warmup(dfd_handle* h, int n_frames);   // detector forward on n synthetic 300x300 inputs (tile measurement)
struct HaarState;       // haar_api.hip: Haar cascade fallback detector
int haar_init(dfd_handle* h);
void haar_destroy(dfd_handle* h);
struct CommState;       // comm_api.hip: RCCL communicator of the vote exchange
void comm_destroy(dfd_handle* h);
struct S6Table;         // gemm_split.hip: measured split-GEMM tiles of this handle
struct MtcnnState;      // mtcnn_api.hip
int mtcnn_init(dfd_handle* h);
void mtcnn_destroy(dfd_handle* h);
struct HeadTrainState;  // head_train.hip: trainer of the classifier head (null until dfd_head_train_begin)
void head_train_destroy(dfd_handle* h);

// Tensor + parse_blob: blob_reader.h (plain C++, also built into the sanitizer harness)

struct B0Block {
    int kernel, stride, expand, c_in, c_out, c_exp, c_se, h_in, h_out, pad_lo;
    bool skip;
    const float *exp_w, *exp_b, *dw_w, *dw_b, *se_w1, *se_b1, *se_w2, *se_b2, *proj_w, *proj_b;
    int dw_tiles;
};

struct B0Plan {
    std::vector<B0Block> blocks;
    const float *stem_w, *stem_b, *head_w, *head_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *fc3_w, *fc3_b;
    // workspace (floats per image)
    size_t io_floats = 0, exp_floats = 0, dw_floats = 0, pool_floats = 0, gate_floats = 0;
};

// Pixel budget of ONE batched request (dfd_analyze_stream_batch / jpeg_decode_batch_to): 2^27 = 64 frames of 1080p.  A
// flat 8192 x 8192 JPEG is ~1 MB, so a 32-part request inside the server's body limit could otherwise ask for 13 GB of
// pinned coefficients + 6 GB of frames before anything is rejected; the check runs on the parsed headers, before any
// allocation (the server mirrors it: backend_server.MAX_BATCH_PIXELS).
constexpr size_t kMaxBatchPixels = (size_t)1 << 27;

// a device buffer that only ever grows (re-allocated outside of steady state)
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct B0Tap {
    const char* name = nullptr;   // stage to copy out, or null
    float* out = nullptr;
    size_t capacity = 0, count = 0;
    bool found = false;
};
struct B0Prof {
    std::vector<hipEvent_t> events;
    std::vector<const char*> names;
    bool enabled = false;
};

}  // namespace dfd

struct dfd_handle {
    int device = 0;
    int max_batch = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t order_ev = nullptr;       // dfd_wait_for: recorded on another handle's stream, waited for by this one
    // dfd_analyze_frames_host: copy stream + two staging slots (uploads overlap the previous batch's compute)
    // pinned mailbox for the small host<->device transfers of the batch path (mailbox_* below)
    char* mailbox = nullptr;
    size_t mailbox_cap = 0, mailbox_head = 0, mailbox_lap_end = 0;
    size_t mailbox_live = 0, mailbox_live_prev = 0;   // bytes handed out since the last / between the last two stream_sync
    std::vector<char*> mailbox_old, mailbox_old_prev; // replaced blocks: freed two stream_syncs after their retirement
    // second compute stream: the forensic launch set of a batch call runs beside detector / classifier
    hipStream_t aux_stream = nullptr;
    hipEvent_t aux_go = nullptr, aux_done = nullptr;
    bool overlap_forensics = true;
    size_t forensic_chunk_bytes = (size_t)256 << 20;   // work memory of one launch set of the general forensic chain in the batched
                                         // stream entries (option "forensic_chunk_bytes"): a size group runs in chunks of the
                                         // frames that fit, one frame at least
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_done[2] = {nullptr, nullptr}, slot_free[2] = {nullptr, nullptr};
    dfd::DevBuf stage[2];
    std::map<std::string, dfd::Tensor> tensors;
    std::vector<void*> owned;            // every hipMalloc the handle must free
    dfd::B0Plan b0;
    // classifier workspace
    float *in_nchw = nullptr, *io0 = nullptr, *io1 = nullptr, *expbuf = nullptr, *dwbuf = nullptr;
    float *pool = nullptr, *gate = nullptr, *headbuf = nullptr, *feat = nullptr, *fc1 = nullptr,
          *fc2 = nullptr, *logits = nullptr;
    // image pre-processing: colour LUTs + lazily grown scratch (frame upload, Lab/BGR crops)
    dfd::ColorTables color{};
    bool has_color = false;
    dfd::DevBuf frame_buf, lab_buf, crop_buf, lut_buf, desc_buf, u8_out, face_batch;
    dfd::DevBuf det_desc;                // detect_frames_run: FrameDesc table of the detector's ragged resize
    int last_detections = 0;             // detections of the last single-frame detector run, before the max_out cut
    std::vector<char> crop_valid;        // per crop of the last preprocess: 0 = the MTCNN stage found no face
    int n_compact = 0;                   // rows of in_nchw the last preprocess filled (= crops with a face, in crop order, when it compacts)
    // test-time augmentation (imgproc_api.hip): the one-shot arming of the next fused analyze call and the [faces][1 + copies]
    // logits of the last armed call
    bool tta_armed = false;
    int tta_copies = 0, tta_capacity = 0;      // of the arming
    std::vector<dfd_tta_draw> tta_draws;       // copied at arm time: tta_capacity x tta_copies, face-major
    std::vector<float> tta_logits;             // last armed call
    int tta_out_faces = 0, tta_out_copies = 0;
    dfd::DevBuf tta_desc, tta_logit_buf;       // augment table (rows + tile starts) / device logits of all images of a call
    unsigned long long classifier_crops = 0;   // crops b0_forward has been asked for since dfd_create (dfd_classifier_crop_count)
    dfd::ForensicState* forensic = nullptr;   // per-stream temporal state + work buffers
    dfd::FreqState* freq = nullptr;           // compute_frequency_features tables + scratch
    dfd::FreqDomainState* freq_domain = nullptr;   // frequency analysis at any size: tables per length + work buffers
    dfd::SsdState* ssd = nullptr;             // detector plan + workspace (null: blob has no detector)
    dfd::MtcnnState* mtcnn = nullptr;         // MTCNN cascade (null: blob has none)
    dfd::HaarState* haar = nullptr;           // Haar cascade (null: blob has none)
    dfd::CommState* comm = nullptr;           // vote exchange (null until dfd_comm_init)
    dfd::HeadTrainState* head_train = nullptr; // open head trainer (dfd_head_train_begin .. _end)
    bool use_mtcnn = true;                    // classify paths align each crop with the cascade when the blob has one
    bool fuse_stem = true;               // stem conv computed inside block 0's depthwise kernel
    bool fuse_expand = true;             // MBConv blocks 1-5: expand conv computed inside the depthwise kernel
    bool fuse_proj0 = true;              // block 0's projection computed inside block 1's expand + depthwise launch (fp32, with fuse_expand)
    bool warming = false;                // inside dfd_warmup: every GEMM shape of the unfused plan is launched, so that its tile is measured
    bool fuse_late = true;               // blocks 6-10 / 12-15: expand + depthwise of whole images in one launch (mbconv_late_kernel):
                                         // the faster configuration (round 3: +2.2-2.6 % per step, strictly fewer bytes), default since round 4
    int fuse_late_skip = -1;             // blocks that keep expand GEMM + depthwise kernel although fuse_late is on (option
                                         // "fuse_late_skip", a bit per block).  -1 = not set: blocks 8 and 9 where mbconv_late_kernel
                                         // would run them - measured per block at batch 256 (fused - separate, us): b6 -17.8, b7 -5.5,
                                         // b8 +2.1, b9 +3.6, b10 -1.4, b12 -9.8, b13 -4.9, b14 -4.7, b15 -2.3; only the unset mask
                                         // lets mbconv_k5_kernel take blocks 8 and 9 (fuse_k5; b0_plan.hip)
    int fuse_k5_min = 0;                 // crops in the last round of blocks from which the k5 kernel runs (<= 0: measured default, b0_plan.hip)
    int cu_count = 256;                  // compute units of the device (dfd_create)
    bool fuse_k5 = true;                 // fp32 blocks 6-11 (k3 / k5 on the 14 x 14 maps; block 11 at stride 2) of the fuse_late
                                         // launches: one block per image (mbconv_k5_kernel, rounds 6 and 7) instead of one per image
                                         // and 32 channels (block 11: instead of expand GEMM + depthwise kernel); same result bits.
                                         // Bit 11 of an explicit fuse_late_skip keeps block 11's two launches
    bool split_gemm = true;              // 1x1 / k x k convs on the bf16x3-split MFMA path (gemm_split.hip)
    bool act_bf16 = false;               // classifier activations stored as bf16 (fp32 arithmetic): configs[3]
    int bf16_planes = 3;                 // weight planes the bf16-activation GEMMs use: 3 = fp32-exact weights, 1 = bf16 weights
    dfd::DevBuf jpeg_work;               // dfd_decode_jpeg: coefficients, component planes, quantisation tables
    dfd::DevBuf jpeg_raw[2];             // dfd_analyze_jpegs_host: the scans of the chunk being decoded / being uploaded
    dfd::DevBuf jpeg_work2[2];           // ... and the decoder's scratch of the chunk being decoded / the one before
    hipStream_t jpeg_stream = nullptr;   // ... whose decode runs beside the analysis of the previous chunk (= aux_stream)
    hipEvent_t jpeg_done[2] = {nullptr, nullptr}, frames_free[2] = {nullptr, nullptr};
    void* jpeg_host = nullptr;           // pinned host buffer the entropy decoder writes the coefficients into
    size_t jpeg_host_cap = 0;
    int jpeg_device_entropy = 2;         // batch calls: 2 = restart-less JPEGs are entropy-decoded on the device (jpeg_gpu_entropy.h) from
                                         // 1 MiB of scan data per call (below that the host pool is quicker), 1 = always, 0 = never
    int jpeg_device_restart = 0;         // 1 = files with restart intervals are eligible for that decoder too (option "jpeg_device_restart",
                                         // initial value from DFD_JPEG_DEVICE_RESTART); 0 = they take the host decoder
    int jpeg_progressive = 0;            // 1 = progressive (SOF2) files are decoded (option "jpeg_progressive", initial value from
                                         // DFD_JPEG_PROGRESSIVE); 0 = DFD_ERR_UNSUPPORTED as for every other flavour
    int jpeg_device_progressive = 0;     // batch calls: 1 = the scans of progressive files are decoded on the device (jpeg_gpu_progressive.h,
                                         // option "jpeg_device_progressive"); 0 = by the host pool
    int jpeg_rounds = 16;                // rounds of that decoder's fixed-point iteration (option "jpeg_rounds", 2 .. 32; converged rounds cost ~nothing)
    int jpeg_chunk_bytes = 512;          // bytes of de-stuffed scan per lane of that decoder (option "jpeg_chunk_bytes", >= 256, % 4)
    unsigned long long jpeg_frames_device = 0, jpeg_frames_host = 0;   // frames of batch calls decoded there / by the host decoder
    dfd::DevBuf jpeg_enc[6];             // dfd_encode_jpeg*: staged sources, tables + descriptors, coefficients, scan arrays,
                                         // the unstuffed bit buffer, the packed files (jpeg_encode.hip)
    dfd::DevBuf tap_buf;                 // fp32 staging for taps of bf16 buffers
    dfd::DevBuf aug_idx;                 // dfd_train_augment_gather: the batch's indices
    dfd::DevBuf aug_u8, aug_f32, aug_tab; // train-time augmentation (train_augment.hip): uint8 source + ping-pong regions, the
                                         // float tensors, rows + resize tables + luma sums + partners
    std::map<const float*, unsigned short*> wsplit;   // fp32 weight tensor -> its three-plane bf16 split
    dfd::S6Table* gemm = nullptr;        // split-GEMM tile per shape (measured by dfd_warmup, heuristic otherwise)
    dfd::B0Prof prof;                    // layer events between profile_begin/end
    int prof_steps = 0;                  // forwards that carried events
    int prof_seen = 0, prof_stride = 1;  // forwards since profile_begin; every prof_stride-th one is instrumented
    std::string err;
};

namespace dfd {

extern thread_local std::string g_create_error;

int fail(dfd_handle* h, int code, const char* fmt, ...);

#define DFD_HIP_TRY(h, expr)                                                                    \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return dfd::fail((h), DFD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                             __FILE__, __LINE__);                                               \
    } while (0)

// grows `b` to at least `bytes` (frees and re-allocates; contents are not preserved)
int ensure(dfd_handle* h, DevBuf* b, size_t bytes);
// Small transfers on the compute stream without the DMA engines: descriptors, detection rows and logits are a few KB,
// but as hipMemcpyAsync they queue on the same SDMA engine as the 200-400 MB frame upload of the next batch and the
// batch in flight stalls until that upload has finished (measured: 32-frame batches ran at upload + compute, not at
// max(upload, compute)).  A copy kernel moves them through a pinned, device-visible mailbox instead.
//   mailbox_h2d: `src` is copied into the mailbox before the call returns (reusable at once); the device copy is enqueued.
//   mailbox_d2h: enqueues the copy and returns the host address that holds the data once the stream is synchronised.
// Every wait on the handle's stream goes through stream_sync: it is the point after which mailbox regions handed out
// before the PREVIOUS sync can be reused (the host reads a d2h region right after the sync that completes it).
hipError_t stream_sync(dfd_handle* h);
int mailbox_h2d(dfd_handle* h, void* dst_dev, const void* src, size_t bytes);
const void* mailbox_d2h(dfd_handle* h, const void* src_dev, size_t bytes);
void copy_kernel_async(void* dst, const void* src, size_t bytes, hipStream_t s);
// builds h->color from the "lut.*" tensors of the blob (imgproc_api.hip)
int color_tables_init(dfd_handle* h);

// stages that work on a frame already resident in HBM (forensic_api / ssd_api / imgproc_api)
// the analyzer for the fused single-frame entries: the stream at the analysis size and on the chain it holds - the general
// chain (forensic_kernels.hip with a run-time edge) for a stream that was opened (dfd_forensics_open) or holds another size
// than 256, the 256x256 chain (the same kernels with the edge a constant) otherwise.  One host path (forensic_api.hip forensics_chain_run) serves both, and dfd_forensics /
// dfd_forensics_sized with them.
int forensics_stream_run(dfd_handle* h, int stream_id, const uint8_t* frame_dev, int hh, int ww, int stride, int full,
                         double* scores_out, double* prob_out);
int detect_run(dfd_handle* h, const uint8_t* frame_dev, int hh, int ww, int stride, float conf_thr, int32_t* xywh_out,
               float* conf_out, int max_out, int* n_out);
// haar_api.hip: detectMultiScale + groupRectangles on a resident frame; *n_total = groups before the max_out cut
int haar_run(dfd_handle* h, const uint8_t* frame_dev, int hh, int ww, int stride, double scale_factor, int min_neighbors,
             int min_size, int32_t* xywh_out, int max_out, int* n_out, int* n_candidates, int* n_total = nullptr);
// frame_offs: per-crop byte offset of its frame inside frame_dev (null = single frame)
// compact: in_nchw receives only the crops the MTCNN stage kept (h->n_compact rows, flags in h->crop_valid)
int preprocess_run(dfd_handle* h, const uint8_t* frame_dev, int hh, int ww, int stride, const int32_t* xywh, int n,
                   int apply_clahe, const size_t* frame_offs = nullptr, bool compact = false);
// boxes of resident frame(s) -> logits on the host, m <= max_batch: crop / CLAHE / MTCNN / 224 x 224, then the classifier
// at the batch of the crops the cascade KEPT (reference deepfake_detection.py:377-380: `mtcnn()` -> None returns before
// the model runs) - a rejected crop costs no classifier work and gets NaN.  Ends with a stream wait.
// crop_frames (or null): per-crop frame of a ragged batch (offset in frame_dev, size, stride) instead of hh / ww / stride /
// frame_offs
// tta (or null): `copies` augmented images of every box ride in the same pass (CLAHE once per face, one augment launch, all
// m x (1 + copies) images through the cascade together, the classifier in chunks of max_batch images); draws: m x copies,
// face-major; logits_out still receives the un-augmented column, all_out [m][1 + copies] the whole block
struct TtaCall { int copies; const dfd_tta_draw* draws; float* all_out; };
int classify_boxes(dfd_handle* h, const uint8_t* frame_dev, int hh, int ww, int stride, const int32_t* xywh, int m,
                   int apply_clahe, const size_t* frame_offs, float* logits_out, const FrameDesc* crop_frames = nullptr,
                   const TtaCall* tta = nullptr);
// The arming of dfd_tta_arm as the fused entry points use it.  tta_take: called first thing by an entry point - consumes
// the arming (whatever becomes of the call) and checks its capacity against n_frames x max_faces; *armed tells whether the
// call carries copies.
constexpr int kMaxTtaCopies = 63;
int tta_take(dfd_handle* h, long long n_frames, int max_faces, bool* armed);
int tta_refuse(dfd_handle* h, const char* entry);       // entry points without the feature: DFD_ERR_STATE when armed
// classify_boxes on m <= max_batch faces of the running fused call; tta: with the arming's next m x copies draws, the
// [m][1 + copies] block appended to h->tta_logits
int classify_faces(dfd_handle* h, const uint8_t* frame_dev, int hh, int ww, int stride, const int32_t* xywh, int m, int apply_clahe,
                   float* logits_out, const FrameDesc* crop_frames, bool tta);

// DetectionOutput of `n` frames already resized to 300x300 -> rows/count on the host
int detect_batch_run(dfd_handle* h, const uint8_t* frames_dev, int n, int hh, int ww, int stride, size_t frame_bytes,
                     float conf_thr, int max_faces, int32_t* xywh_out, int* n_out, int* n_total_out = nullptr);
// the same for m frames of their own sizes: frame fd[idx[j]] of the arena at frames_dev (every one >= 30 px a side); its
// boxes go to xywh_out + idx[j] * max_faces * 4, its counts to n_out[idx[j]] / n_total_out[idx[j]]
int detect_frames_run(dfd_handle* h, const uint8_t* frames_dev, const FrameDesc* fd, const int* idx, int m, float conf_thr,
                      int max_faces, int32_t* xywh_out, int* n_out, int* n_total_out);
// the analyzer over n frames of any streams and sizes (frame f of stream stream_ids[f], descriptor fd[f] into the arena
// at frames_dev; the frames of one stream in stream order): one launch set per analysis size, every stream's temporal
// state advances by its frames - results identical to forensics_stream_run on each stream's frames in order
int forensics_streams_run(dfd_handle* h, const uint8_t* frames_dev, const FrameDesc* fd, int n, const int* stream_ids,
                          const int* full, double* scores_out, double* prob_out);
// jpeg_decode.hip: n JPEGs of one size -> packed BGR frames [n][hh][ww][3] at frames_dev (entropy decoding of the files
// in parallel on the host pool, one coefficient upload, IDCT / colour per frame).  *hh / *ww: in = expected size or 0
int jpeg_decode_batch_to(dfd_handle* h, const uint8_t* const* jpegs, const size_t* lens, int n, uint8_t* frames_dev_or_null,
                         int* hh, int* ww);
// stateless six-signal forensic probability of `n` device frames (temporal signal = first-frame value 0)
int forensics_batch_run(dfd_handle* h, const uint8_t* frames_dev, int n, int hh, int ww, int stride, size_t frame_bytes,
                        double* prob_out, double* scores_out);
// the same in two halves: begin enqueues the launch set on the handle's second stream (ordered after what the main
// stream holds at that moment) and returns; end waits for it and scores on the host.  Nothing else may use the
// forensic work buffers in between.
int forensics_batch_begin(dfd_handle* h, const uint8_t* frames_dev, int n, int hh, int ww, int stride, size_t frame_bytes);
int forensics_batch_end(dfd_handle* h, int n, double* prob_out, double* scores_out);

// mtcnn_api.hip: MTCNN.forward on a BGR image in HBM -> selected box (x1,y1,x2,y2,prob), *found, and the
// 160x160 BGR u8 crop at mtcnn_face_dev(h).  tap_* are for parity tests (null otherwise; tap_crop: the image they read).
struct MtImage { const uint8_t* src; int h, w; size_t stride; };
// the same for `n` images of a step at once: faces_out [n][160*160*3] (device), boxes_out [n][5] or null, found [n]
// returns after the step's last stream wait: `found` is final (the classifier is then sized by the faces that are left)
int mtcnn_align_batch_device(dfd_handle* h, const MtImage* imgs, int n, uint8_t* faces_out, float* boxes_out, char* found,
                             const char* tap_name, std::vector<float>* tap, int* tap_dims, int tap_crop = 0);
int mtcnn_align_device(dfd_handle* h, const uint8_t* img_dev, int hh, int ww, size_t stride, float* box_out, int* found,
                       const char* tap_name, std::vector<float>* tap, int* tap_dims);
const uint8_t* mtcnn_face_dev(dfd_handle* h);

// imgproc_api.hip: the per-frame work on a frame that is already in h->frame_buf
int analyze_frame_resident(dfd_handle* h, int stream_id, int hh, int ww, int stride, int full_forensics, float conf_thr,
                           int max_faces, int apply_clahe, double* scores_out, double* forensic_prob_out, int32_t* xywh_out,
                           int* n_faces_out, float* logits_out, bool tta = false);

// jpeg_decode.hip: baseline JPEG bytes -> packed BGR frame in h->frame_buf (stride width * 3)
int jpeg_decode_to_frame(dfd_handle* h, const uint8_t* jpeg, size_t len, int* hh, int* ww);

// b0_plan.hip
// three-plane bf16 split of a weight tensor of the handle, made on first use; null (+ error set) on failure
const unsigned short* split_weights(dfd_handle* h, const float* W, int N, int K, bool transposed = false);
// 1x1 conv through the split path when enabled and the shape allows, else the fp32 MFMA kernel
int pointwise(dfd_handle* h, const float* X, const float* W, const float* bias, const float* gate, const float* R,
              float* Y, int M, int K, int N, int HW, int act);
int b0_build_plan(dfd_handle* h);
// Runs the classifier on h->stream.  `stop_at_features`: leave after the pooled 1280-vector.
int b0_forward(dfd_handle* h, const float* nchw_dev, int n, float* logits_dev, B0Tap* tap,
               B0Prof* prof);
// the buffer (io0 or io1) that holds the last block's output after b0_forward
float* b0_last_block_out(const dfd_handle* h);
// after b0_forward on n crops: the head conv WITHOUT its swish into z_out [n][49][1280] (activation type of the handle)
int b0_head_preact(dfd_handle* h, int n, void* z_out);
// b0_forward up to the pooled features with block 15's output copied to the host as fp32 [n][7][7][320]; waits on the stream
int b0_trunk_to_host(dfd_handle* h, const float* x, int n, float* out_host, int block = -1);   // block: -1 = the last one

}  // namespace dfd
