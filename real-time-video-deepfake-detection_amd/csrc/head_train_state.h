// What head_train.hip and head_train_conv.hip share: the trainer's state, the layout of the head's parameter arena and
// the host entry points each file offers the other.  The conv stage (dfd_head_train_unfreeze_conv) hangs off the head
// trainer's state; everything from the pooled features on runs in head_train.hip's kernels.  Block 15
// (dfd_head_train_unfreeze_block, head_train_block.hip) hangs off it in turn and feeds the conv stage on the device;
// blocks 14, 13, 12 and 11 (dfd_head_train_unfreeze_block_at, the same file) each feed the block above them.
#pragma once
#include <cstdint>

#include "dfd_common.h"

namespace dfd {

constexpr int HT_IN = 1280, HT_H1 = 512, HT_H2 = 256, HT_MAX_N = 256, HT_THREADS = 256, HT_SLAB = 16;
// flat parameter arena (floats): every offset a multiple of 4, so weight rows stay 16-byte aligned
constexpr int O_W1 = 0, O_B1 = O_W1 + HT_H1 * HT_IN, O_G1 = O_B1 + HT_H1, O_BE1 = O_G1 + HT_H1;
constexpr int O_W2 = O_BE1 + HT_H1, O_B2 = O_W2 + HT_H2 * HT_H1, O_G2 = O_B2 + HT_H2, O_BE2 = O_G2 + HT_H2;
constexpr int O_W3 = O_BE2 + HT_H2, O_B3 = O_W3 + HT_H2, HT_COUNT = O_B3 + 1;
static_assert(O_W2 % 4 == 0 && O_W3 % 4 == 0, "weight rows must stay 16-byte aligned");
constexpr int NORM_BLOCKS = 256;
constexpr int HT_STAGES = 5;              // block stages a trainer can hold: _blocks.15 down to _blocks.11
constexpr int HT_ARENAS = 2 + HT_STAGES;  // head, conv, then the block stages

struct HeadConvState;   // head_train_conv.hip: _conv_head + _bn1 under training (null until dfd_head_train_unfreeze_conv)
struct HeadBlockState;  // head_train_block.hip: one MBConv block under training

// The partial sums of squares of every arena, in the order head, conv, block 15, 14, 13, 12, 11 (null: no such stage).  Each
// AdamW launch adds them entry by entry in this order before it takes the norm, so all see the same norm.
struct NormParts { const double* p[HT_ARENAS]; };

struct HeadTrainState {
    dfd_head_config cfg{};
    int max_n = 0, last_n = 0;
    unsigned long long step = 0, counter = 0;
    double p[3] = {0, 0, 0};                                    // dropout rate per layer
    uint32_t thr[3] = {0, 0, 0};
    float dscale[3] = {1, 1, 1};
    float *param = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr, *ema = nullptr;
    float *rm1 = nullptr, *rv1 = nullptr, *rm2 = nullptr, *rv2 = nullptr;
    float *feat = nullptr, *x0 = nullptr, *z1 = nullptr, *xh1 = nullptr, *a1 = nullptr, *dy1 = nullptr, *z2 = nullptr,
          *xh2 = nullptr, *a2 = nullptr, *dy2 = nullptr, *istd1 = nullptr, *istd2 = nullptr, *logits = nullptr,
          *dlogit = nullptr, *ya = nullptr, *yb = nullptr, *scalars = nullptr;   // scalars[0] = loss, [1] = grad norm
    double* partial = nullptr;
    uint8_t *mask0 = nullptr, *mask1 = nullptr, *mask2 = nullptr;
    void* pool = nullptr;
    HeadConvState* conv = nullptr;
    // stage[k] = _blocks.(15 - k), deepest last: stage[0] null until dfd_head_train_unfreeze_block, the others until
    // dfd_head_train_unfreeze_block_at; stage[k] is only ever set when stage[k - 1] is
    HeadBlockState* stage[HT_STAGES] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

// The trainer's counter-based hash: head_training.dropout_keep_mask is the specification of these three.  layer 0..2 are
// the head's dropouts, layer 17 - b block b's drop-connect (one draw per crop): 3 for block 14, 4 for 13, 5 for 12.
__host__ __device__ inline uint32_t fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
inline uint32_t mask_key(unsigned long long seed, unsigned long long counter, int layer) {
    uint32_t k = fmix32((uint32_t)seed + 0x9E3779B9u);
    k = fmix32(k ^ (uint32_t)(seed >> 32));
    k = fmix32(k ^ (uint32_t)counter);
    k = fmix32(k ^ (uint32_t)(counter >> 32));
    return fmix32(k ^ (uint32_t)(layer + 1));
}
__host__ __device__ inline bool mask_keep(uint32_t key, uint32_t idx, uint32_t thr) {
    return fmix32(fmix32(idx ^ key) + key) >= thr;
}

// what every accumulate entry accepts for its two scalars: lam in [0, 1] and a loss_scale that is a number (NaN fails both)
inline bool head_train_mix_ok(float lam, float loss_scale) { return lam >= 0.f && lam <= 1.f && loss_scale == loss_scale; }

// ---- head_train.hip, for the conv stage
// One train-mode forward / loss / backward on the n rows already in S->feat (device): uploads the labels, leaves the
// loss in S->scalars[0] and the logits in S->logits, adds the head's gradients.  dfeat (device, [n][1280]) or null:
// the gradient with respect to S->feat.  Nothing is downloaded and the stream is not waited on.
int head_train_step(dfd_handle* h, HeadTrainState* S, int n, const float* labels_a, const float* labels_b, float lam,
                    float loss_scale, float* dfeat);
// eval-mode forward of the n rows in S->feat with the parameters at P -> S->logits
int head_train_eval_step(dfd_handle* h, HeadTrainState* S, const float* P, int n);
void head_train_launch_sumsq(hipStream_t s, const float* g, int count, double* partial);
// every arena's partials of the last sumsq launches (head_train_apply), for the AdamW launches
NormParts head_train_norm_parts(HeadTrainState* S);
// clip + AdamW + EMA + zeroing over one arena at the rate `lr`, under the norm over all arenas of `parts`.
// t = 1-based step number.
void head_train_launch_adamw(hipStream_t s, float* p, float* g, float* m, float* v, float* ema, int count, const NormParts& parts,
                             const dfd_head_config& c, double lr, double t, float* norm_out);

// ---- head_train_conv.hip, for the head trainer
void headconv_destroy(HeadTrainState* S);
const double* headconv_sumsq(dfd_handle* h, HeadTrainState* S);             // launches; -> the conv arena's partials
void headconv_adamw(dfd_handle* h, HeadTrainState* S, double lr, double t);  // the conv group's step at lr * lr_scale
int headconv_commit(dfd_handle* h, HeadTrainState* S, int use_ema);
int headconv_tap(dfd_handle* h, HeadTrainState* S, const char* name, float* out, size_t capacity);   // "cfeat", "dfeat", "cz"
// ---- head_train_conv.hip, for block 15's stage: the conv stage on rows that are already on the device
float* headconv_rows(HeadTrainState* S);     // the stage's input, device [max_n][49][320]
float headconv_lr_scale(HeadTrainState* S);
const double* headconv_partial(HeadTrainState* S);   // the conv arena's partials of the last headconv_sumsq
// dfd_head_train_accumulate_trunk's launches on the n rows in headconv_rows(): forward, head, loss, backward.  dx (device
// [n][49][320]) or null: the gradient with respect to the rows, dZ . W.  Nothing is downloaded, the stream is not waited on.
int headconv_step(dfd_handle* h, HeadTrainState* S, int n, const float* labels_a, const float* labels_b, float lam,
                  float loss_scale, float* dx);
int headconv_eval_step(dfd_handle* h, HeadTrainState* S, int use_ema, int n);    // -> S->logits

// ---- head_train_block.hip, for the head trainer
// `k` = the stage's place in HeadTrainState::stage; a stage that is not unfrozen has no partials (null) and nothing to step
void headblock_destroy(HeadTrainState* S);                                   // every stage
const double* headblock_sumsq(dfd_handle* h, HeadTrainState* S, int k);      // launches; -> the stage arena's partials
const double* headblock_partial(HeadTrainState* S, int k);
void headblock_adamw(dfd_handle* h, HeadTrainState* S, double lr, double t);  // the block groups' steps at lr * the conv stage's lr_scale
int headblock_commit(dfd_handle* h, HeadTrainState* S, int use_ema);          // block 15, then 14, 13, 12, 11 where they are unfrozen
int headblock_tap(dfd_handle* h, HeadTrainState* S, const char* name, float* out, size_t capacity);  // "b15.*" .. "b11.*"

}  // namespace dfd
