// Host side of the classifier: weights blob -> device tensors -> per-layer launch plan.
// The block table restates efficientnet_pytorch's B0 arguments (the dependency the
// reference builds its backbone from, reference model.py:39-43) and must agree with
// b0_arch.py; dfd_create checks every tensor's shape against it.
#include <algorithm>

#include "b0_kernels.h"
#include "dfd_common.h"

namespace dfd {

thread_local std::string g_create_error;

int fail(dfd_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_create_error = buf;
    return code;
}

namespace {

struct Stage { int rep, k, s, e, ci, co; };
const Stage kStages[] = {{1, 3, 1, 1, 32, 16}, {2, 3, 2, 6, 16, 24}, {2, 5, 2, 6, 24, 40},
                         {3, 3, 2, 6, 40, 80}, {3, 5, 1, 6, 80, 112}, {4, 5, 2, 6, 112, 192},
                         {1, 3, 1, 6, 192, 320}};

const float* need(dfd_handle* h, const std::string& name, std::initializer_list<uint32_t> dims, bool* ok) {
    auto it = h->tensors.find(name);
    if (it == h->tensors.end()) {
        if (*ok) fail(h, DFD_ERR_BLOB, "weights blob: tensor '%s' missing", name.c_str());
        *ok = false;
        return nullptr;
    }
    const Tensor& t = it->second;
    size_t want = 1;
    for (uint32_t d : dims) want *= d;
    if (t.count != want) {
        if (*ok) fail(h, DFD_ERR_BLOB, "weights blob: tensor '%s' has %zu elements, expected %zu", name.c_str(), t.count, want);
        *ok = false;
        return nullptr;
    }
    return t.dev;
}

}  // namespace

int b0_build_plan(dfd_handle* h) {
    B0Plan& P = h->b0;
    bool ok = true;
    P.stem_w = need(h, "stem.w", {3, 3, 3, 32}, &ok);
    P.stem_b = need(h, "stem.b", {32}, &ok);
    int hcur = 112, idx = 0;
    P.io_floats = (size_t)112 * 112 * 32;
    for (const Stage& st : kStages) {
        for (int r = 0; r < st.rep; ++r, ++idx) {
            B0Block b{};
            b.kernel = st.k;
            b.stride = r == 0 ? st.s : 1;
            b.expand = st.e;
            b.c_in = r == 0 ? st.ci : st.co;
            b.c_out = st.co;
            b.c_exp = b.c_in * st.e;
            b.c_se = b.c_in / 4 > 0 ? b.c_in / 4 : 1;
            b.h_in = hcur;
            b.h_out = (hcur + b.stride - 1) / b.stride;
            const int total = (b.h_out - 1) * b.stride + b.kernel - b.h_in;
            b.pad_lo = (total > 0 ? total : 0) / 2;
            b.skip = b.stride == 1 && b.c_in == b.c_out;
            const std::string q = "b" + std::to_string(idx);
            const uint32_t ce = b.c_exp, ci = b.c_in, co = b.c_out, cs = b.c_se, k = b.kernel;
            if (b.expand != 1) {
                b.exp_w = need(h, q + ".exp.w", {ce, ci}, &ok);
                b.exp_b = need(h, q + ".exp.b", {ce}, &ok);
            }
            b.dw_w = need(h, q + ".dw.w", {k, k, ce}, &ok);
            b.dw_b = need(h, q + ".dw.b", {ce}, &ok);
            b.se_w1 = need(h, q + ".se.w1", {cs, ce}, &ok);
            b.se_b1 = need(h, q + ".se.b1", {cs}, &ok);
            b.se_w2 = need(h, q + ".se.w2", {cs, ce}, &ok);
            b.se_b2 = need(h, q + ".se.b2", {ce}, &ok);
            b.proj_w = need(h, q + ".proj.w", {co, ce}, &ok);
            b.proj_b = need(h, q + ".proj.b", {co}, &ok);
            b.dw_tiles = depthwise_tiles(b.h_in, b.c_exp, b.kernel, b.stride);
            if (b.dw_tiles < 0) return fail(h, DFD_ERR_STATE, "no depthwise kernel for block %d", idx);
            b.dw_tiles = std::max(b.dw_tiles, mbconv_tiles(b.h_in, b.c_exp, b.kernel, b.stride, b.c_in, true, true));
            auto mx = [](size_t& a, size_t v) { if (v > a) a = v; };
            mx(P.io_floats, (size_t)b.h_out * b.h_out * b.c_out);
            if (b.expand != 1) mx(P.exp_floats, (size_t)b.h_in * b.h_in * b.c_exp);
            mx(P.dw_floats, (size_t)b.h_out * b.h_out * b.c_exp);
            mx(P.pool_floats, (size_t)b.dw_tiles * b.c_exp);
            mx(P.gate_floats, (size_t)b.c_exp);
            P.blocks.push_back(b);
            hcur = b.h_out;
        }
    }
    P.head_w = need(h, "head.w", {1280, 320}, &ok);
    P.head_b = need(h, "head.b", {1280}, &ok);
    P.fc1_w = need(h, "fc1.w", {512, 1280}, &ok);
    P.fc1_b = need(h, "fc1.b", {512}, &ok);
    P.fc2_w = need(h, "fc2.w", {256, 512}, &ok);
    P.fc2_b = need(h, "fc2.b", {256}, &ok);
    P.fc3_w = need(h, "fc3.w", {1, 256}, &ok);
    P.fc3_b = need(h, "fc3.b", {1}, &ok);
    return ok ? DFD_OK : DFD_ERR_BLOB;
}

const unsigned short* split_weights(dfd_handle* h, const float* W, int N, int K, bool transposed) {
    const size_t count = split_weights_count(N, K);
    auto it = h->wsplit.find(W);
    if (it != h->wsplit.end()) return it->second;
    void* p = nullptr;
    if (hipMalloc(&p, count * 3 * sizeof(unsigned short)) != hipSuccess) {
        fail(h, DFD_ERR_HIP, "hipMalloc of %zu bytes for split weights failed", count * 6);
        return nullptr;
    }
    h->owned.push_back(p);
    launch_split_weights(W, static_cast<unsigned short*>(p), N, K, h->stream, transposed);
    h->wsplit[W] = static_cast<unsigned short*>(p);
    return static_cast<unsigned short*>(p);
}

// 1x1 conv.  XT = float: split path when enabled and the shape allows, else the fp32 MFMA kernel.
// XT = bf16_t ("bf16_activations"): always the split GEMM's bf16-activation instances.
template <typename XT>
int pointwise_t(dfd_handle* h, const XT* X, const float* W, const float* bias, const float* gate, const XT* R,
                XT* Y, int M, int K, int N, int HW, int act) {
    constexpr bool BF = sizeof(XT) == 2;
    if ((BF || h->split_gemm) && N >= 16 && split_gemm_supports(K, N)) {       // never on M: batch-invariant results
        const unsigned short* w3 = split_weights(h, W, N, K);
        if (!w3) return DFD_ERR_HIP;
        if (!launch_pointwise_split<XT>(h->gemm, X, w3, bias, gate, R, Y, M, K, N, HW, act, BF ? h->bf16_planes : 3, h->stream))
            return fail(h, DFD_ERR_CAPACITY, "1x1 conv M=%d K=%d: one image exceeds the 2^31-byte addressing of the split GEMM", M, K);
    } else {
        if constexpr (BF) return fail(h, DFD_ERR_STATE, "1x1 conv K=%d N=%d has no bf16-activation kernel", K, N);
        else launch_pointwise(X, W, bias, gate, R, Y, M, K, N, HW, act, h->stream);
    }
    return DFD_OK;
}

int pointwise(dfd_handle* h, const float* X, const float* W, const float* bias, const float* gate, const float* R,
              float* Y, int M, int K, int N, int HW, int act) {
    return pointwise_t<float>(h, X, W, bias, gate, R, Y, M, K, N, HW, act);
}

namespace {

struct Marks {
    B0Prof* prof;
    hipStream_t s;
    void mark(const char* name) {
        if (!prof || !prof->enabled) return;
        hipEvent_t e;
        hipEventCreate(&e);
        hipEventRecord(e, s);
        prof->events.push_back(e);
        prof->names.push_back(name);
    }
};

// copy a device buffer out if it is the requested tap (bf16 activations are widened to fp32 on the device first)
template <typename XT>
int tap_out(dfd_handle* h, B0Tap* tap, const std::string& name, const XT* dev, size_t count) {
    if (!tap || !tap->name || tap->found || name != tap->name) return DFD_OK;
    tap->found = true;
    if (count > tap->capacity) return fail(h, DFD_ERR_ARG, "tap '%s' needs %zu floats, capacity %zu", tap->name, count, tap->capacity);
    const float* src = nullptr;
    if constexpr (sizeof(XT) == 2) {
        const int rc = ensure(h, &h->tap_buf, count * 4);
        if (rc) return rc;
        launch_bf16_to_f32(dev, static_cast<float*>(h->tap_buf.p), count, h->stream);
        src = static_cast<const float*>(h->tap_buf.p);
    } else {
        src = dev;
    }
    DFD_HIP_TRY(h, hipMemcpyAsync(tap->out, src, count * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    tap->count = count;
    return DFD_OK;
}

// static names for the profiler (one per launch, in launch order)
const char* layer_name(int blk, const char* what) {
    static std::map<std::string, std::string> pool;
    const std::string key = "b" + std::to_string(blk) + "." + what;
    return pool.emplace(key, key).first->second.c_str();
}

}  // namespace

template <typename XT>
static int b0_forward_t(dfd_handle* h, const float* x, int n, float* logits_dev, B0Tap* tap, B0Prof* prof) {
    if (n <= 0) return fail(h, DFD_ERR_ARG, "batch must be positive");
    if (n > h->max_batch) return fail(h, DFD_ERR_CAPACITY, "batch %d exceeds handle capacity %d", n, h->max_batch);
    const B0Plan& P = h->b0;
    hipStream_t s = h->stream;
    Marks mk{prof, s};
    int rc;
    // the activation workspace is sized for fp32; bf16 storage uses the front half of each buffer
    XT* const io0 = reinterpret_cast<XT*>(h->io0);
    XT* const io1 = reinterpret_cast<XT*>(h->io1);
    XT* const expbuf = reinterpret_cast<XT*>(h->expbuf);
    XT* const dwbuf = reinterpret_cast<XT*>(h->dwbuf);
    XT* const headbuf = reinterpret_cast<XT*>(h->headbuf);
    mk.mark("start");
    // block 0 has no expand conv: its depthwise input IS the stem output, so the two fuse (option "fuse_stem")
    const bool stem_fused = h->fuse_stem && P.blocks[0].expand == 1;
    int stem_tiles = 0;
    if (stem_fused) {
        const bool want_stem = tap && tap->name && std::string(tap->name) == "stem";
        const unsigned short* ws3 = split_weights(h, P.stem_w, 32, 27, true);          // [ky][kx][ci][co] = [27][32], transposed
        if (!ws3) return DFD_ERR_HIP;
        launch_stem_dw<XT>(x, ws3, (int)split_weights_count(32, 27), 64, P.stem_b, P.blocks[0].dw_w, P.blocks[0].dw_b, dwbuf,
                           h->pool, want_stem ? io0 : (XT*)nullptr, n, &stem_tiles, s);
        mk.mark("b0.dw");                               // stem + depthwise of block 0 in one launch
    } else {
        launch_stem<XT>(x, P.stem_w, P.stem_b, io0, n, s);
        mk.mark("stem");
    }
    if ((rc = tap_out(h, tap, "stem", io0, (size_t)n * 112 * 112 * 32))) return rc;
    // Option "fuse_proj0": block 0's projection runs inside block 1's expand + depthwise launch (mbconv_kernel, PROJ0), which
    // reads block 0's depthwise output directly; the 16-channel block output never reaches HBM.  Only where block 1 runs on
    // that kernel (fp32 storage, split GEMM, "fuse_expand", no kernel experiment); a call that taps b0.out runs the two
    // launches (the same bits), and so does dfd_warmup, which measures the projection's tile for those calls.
    bool proj0 = false;
    if constexpr (sizeof(XT) == 4) {
        const B0Block &p0 = P.blocks[0], &p1 = P.blocks[1];
        proj0 = h->fuse_proj0 && h->fuse_expand && h->split_gemm && !h->warming && p0.expand == 1 && !p0.skip &&
                p0.c_out >= 16 && split_gemm_supports(p0.c_exp, p0.c_out) &&
                mbconv_proj0_supported(p1.h_in, p1.c_exp, p1.kernel, p1.stride, p1.c_in, p0.c_exp) &&
                !(tap && tap->name && std::string(tap->name) == "b0.out");
    }
    XT* cur = io0;
    XT* nxt = io1;
    int bi = 0;
    for (const B0Block& b : P.blocks) {
        const int m_in = n * b.h_in * b.h_in, m_out = n * b.h_out * b.h_out;
        const std::string q = "b" + std::to_string(bi);
        const XT* dw_in = cur;
        XT* dw_out = dwbuf;
        int tiles = 0;
        bool fused = false;
        const unsigned short* we3 = nullptr;
        if constexpr (sizeof(XT) == 4) {
            if (proj0 && bi == 1) {
                // input: block 0's depthwise output (dwbuf) and gate (h->gate, rewritten only by this block's se launch
                // below); this block's depthwise output goes to expbuf, which fused blocks leave unused
                const B0Block& p0 = P.blocks[0];
                const unsigned short* wp3 = split_weights(h, p0.proj_w, p0.c_out, p0.c_exp);
                if (!wp3) return DFD_ERR_HIP;
                dw_out = expbuf;
                if (!launch_mbconv_front_proj0(dwbuf, h->gate, wp3, (int)split_weights_count(p0.c_out, p0.c_exp),
                                               (p0.c_exp + 63) / 64 * 64, p0.proj_b, b.exp_w, b.exp_b, b.dw_w, b.dw_b, dw_out,
                                               h->pool, n, b.h_in, b.c_exp, b.kernel, b.stride, b.c_in, b.pad_lo, &tiles, s))
                    return fail(h, DFD_ERR_STATE, "no fused projection kernel for block 1");
                fused = true;
                mk.mark(layer_name(bi, "dw"));        // block 0's projection + expand + depthwise in one launch
                if (tap && tap->name && q + ".exp" == tap->name)
                    return fail(h, DFD_ERR_STATE, "tap '%s': the expanded tensor is not materialised when expand is fused "
                                                  "(dfd_set_option(h, \"fuse_expand\", 0))", tap->name);
            }
        }
        // whole-image launches (blocks 6-15) where they measure faster: per block, batch 256 (section 5, rounds 4 and 6).  As
        // mbconv_late_kernel launches blocks 8 and 9 (k5, 480 / 672 channels at 14 x 14) are 2-4 us slower than expand GEMM +
        // depthwise kernel: an unset "fuse_late_skip" masks them.
        // mbconv_k5_kernel (option "fuse_k5") runs ONE block per image, so its launch takes the same time for 1 and for
        // cu_count images: it is taken where the last round of blocks holds at least K5_MIN_DEFAULT images (measured,
        // section 5) and replaces whatever form the block would run otherwise WITH THAT FORM'S BITS - mode 2 (the separate
        // launches' bias order) for a block the unset mask covers, mode 1 (mbconv_late_kernel's) for an unmasked one; a block
        // masked explicitly keeps its separate launches.  So neither the option nor the batch size changes a result.
        // Blocks 6 and 7 (k3) and block 11 (k5, 14 -> 7) run on instances of the same kernel (round 7).  Block 11 has no
        // mbconv_late_kernel form (k5_only): it always takes mode 2, the bits of the launches it runs otherwise, and bit 11
        // of an explicit mask keeps those launches.
        constexpr int K5_MIN_DEFAULT = 208;
        const int k5_rounds = (n + h->cu_count - 1) / h->cu_count, k5_last = n - (k5_rounds - 1) * h->cu_count;
        const bool k5on = sizeof(XT) == 4 && h->fuse_k5 && h->fuse_late && h->fuse_expand && b.expand != 1 &&
                          k5_last >= (h->fuse_k5_min > 0 ? h->fuse_k5_min : K5_MIN_DEFAULT) &&
                          mbconv_k5_shape(b.h_in, b.c_exp, b.kernel, b.stride, b.c_in, b.pad_lo);
        const bool mask_unset = h->fuse_late_skip < 0;
        const unsigned late_skip = mask_unset ? (1u << 8) | (1u << 9) : (unsigned)h->fuse_late_skip;
        const bool masked = (late_skip >> bi) & 1u;
        const bool k5_only = k5on && mbconv_tiles(b.h_in, b.c_exp, b.kernel, b.stride, b.c_in, true) < 1;
        const int k5 = !k5on || (masked && !mask_unset) ? 0 : (masked || k5_only ? 2 : 1);
        const bool late_here = h->fuse_late && (!masked || k5 == 2);
        if (!fused && b.expand != 1 && h->fuse_expand && mbconv_tiles(b.h_in, b.c_exp, b.kernel, b.stride, b.c_in, late_here, k5 != 0) > 0 &&
            !(we3 = split_weights(h, b.exp_w, b.c_exp, b.c_in))) return DFD_ERR_HIP;
        if (we3 && launch_mbconv_front<XT>(cur, b.c_in, we3, (int)split_weights_count(b.c_exp, b.c_in), (b.c_in + 63) / 64 * 64,
                                           b.exp_w, b.exp_b, b.dw_w, b.dw_b, dwbuf, h->pool, n, b.h_in, b.c_exp,
                                           b.kernel, b.stride, b.pad_lo, &tiles, s, late_here, k5)) {
            fused = true;
            mk.mark(layer_name(bi, "dw"));            // expand + depthwise in one launch
            if (tap && tap->name && q + ".exp" == tap->name)
                return fail(h, DFD_ERR_STATE, "tap '%s': the expanded tensor is not materialised when expand is fused "
                                              "(dfd_set_option(h, \"fuse_expand\", 0))", tap->name);
        }
        if (!fused && k5) return fail(h, DFD_ERR_STATE, "no k5 kernel for block %d", bi);
        if (!fused && b.expand != 1) {
            if ((rc = pointwise_t<XT>(h, cur, b.exp_w, b.exp_b, nullptr, nullptr, expbuf, m_in, b.c_in, b.c_exp,
                                      b.h_in * b.h_in, ACT_SWISH))) return rc;
            mk.mark(layer_name(bi, "exp"));
            if ((rc = tap_out(h, tap, q + ".exp", expbuf, (size_t)m_in * b.c_exp))) return rc;
            dw_in = expbuf;
        }
        if (bi == 0 && stem_fused) {
            tiles = stem_tiles;
        } else if (!fused) {
            if (!launch_depthwise<XT>(dw_in, b.dw_w, b.dw_b, dwbuf, h->pool, n, b.h_in, b.c_exp, b.kernel,
                                      b.stride, b.pad_lo, &tiles, s))
                return fail(h, DFD_ERR_STATE, "no depthwise kernel for block %d", bi);
            mk.mark(layer_name(bi, "dw"));
        }
        if ((rc = tap_out(h, tap, q + ".dw", dw_out, (size_t)m_out * b.c_exp))) return rc;
        launch_se(h->pool, tiles, 1.0f / (float)(b.h_out * b.h_out), b.se_w1, b.se_b1, b.se_w2, b.se_b2,
                  h->gate, n, b.c_exp, b.c_se, s);
        mk.mark(layer_name(bi, "se"));
        if ((rc = tap_out(h, tap, q + ".gate", h->gate, (size_t)n * b.c_exp))) return rc;
        if (!(proj0 && bi == 0)) {                    // (fused: block 1's launch computes this projection, nxt stays unwritten)
            if ((rc = pointwise_t<XT>(h, dw_out, b.proj_w, b.proj_b, h->gate, b.skip ? cur : (const XT*)nullptr, nxt, m_out,
                                      b.c_exp, b.c_out, b.h_out * b.h_out, ACT_NONE))) return rc;
            mk.mark(layer_name(bi, "proj"));
            if ((rc = tap_out(h, tap, q + ".out", nxt, (size_t)m_out * b.c_out))) return rc;
        }
        XT* t = cur; cur = nxt; nxt = t;
        ++bi;
    }
    const B0Block& last = P.blocks.back();
    const int hw = last.h_out * last.h_out;
    if ((rc = pointwise_t<XT>(h, cur, P.head_w, P.head_b, nullptr, nullptr, headbuf, n * hw, last.c_out, 1280, hw,
                              ACT_SWISH))) return rc;
    mk.mark("head");
    if ((rc = tap_out(h, tap, "head", headbuf, (size_t)n * hw * 1280))) return rc;
    launch_avgpool<XT>(headbuf, h->feat, n, hw, 1280, s);
    mk.mark("avgpool");
    if ((rc = tap_out(h, tap, "feat", h->feat, (size_t)n * 1280))) return rc;
    if (!logits_dev) return DFD_OK;   // extract_features stops here
    if ((rc = pointwise(h, h->feat, P.fc1_w, P.fc1_b, nullptr, nullptr, h->fc1, n, 1280, 512, 1, ACT_RELU))) return rc;
    if ((rc = pointwise(h, h->fc1, P.fc2_w, P.fc2_b, nullptr, nullptr, h->fc2, n, 512, 256, 1, ACT_RELU))) return rc;
    launch_pointwise(h->fc2, P.fc3_w, P.fc3_b, nullptr, nullptr, logits_dev, n, 256, 1, 1, ACT_NONE, s);
    mk.mark("mlp");
    if ((rc = tap_out(h, tap, "logit", logits_dev, (size_t)n))) return rc;
    DFD_HIP_TRY(h, hipGetLastError());
    return DFD_OK;
}

// The block loop above swaps io0 / io1 once per block: after b0_forward the last block's output is in io0 for an even
// block count (16), in io1 otherwise.
float* b0_last_block_out(const dfd_handle* h) { return h->b0.blocks.size() % 2 == 0 ? h->io0 : h->io1; }

// The forward on n crops with block 15's output copied out as fp32 [n][7][7][320] (dfd_extract_trunk,
// dfd_train_augment_trunk): the "b15.out" tap of the forward that stops at the pooled features, so the rows are the
// tap's bits (bf16 storage widened) by construction.  Waits on the stream.  `block` (dfd_extract_trunk_at): the "b<block>.out"
// tap of the same forward instead, [n][h_out][h_out][c_out] of that block; -1 = the last block.
int b0_trunk_to_host(dfd_handle* h, const float* x, int n, float* out_host, int block) {
    if (block < 0) block = (int)h->b0.blocks.size() - 1;
    if (block >= (int)h->b0.blocks.size()) return fail(h, DFD_ERR_ARG, "no block %d", block);
    const std::string name = "b" + std::to_string(block) + ".out";
    const B0Block& last = h->b0.blocks[block];
    B0Tap tap;
    tap.name = name.c_str();
    tap.out = out_host;
    tap.capacity = (size_t)n * last.h_out * last.h_out * last.c_out;
    const int rc = b0_forward(h, x, n, nullptr, &tap, nullptr);
    if (rc) return rc;
    if (!tap.found) return fail(h, DFD_ERR_STATE, "the forward wrote no '%s'", name.c_str());
    return DFD_OK;
}

// Grad-CAM's z (gradcam.hip): after b0_forward on n crops, the head conv of the last block's output once more with
// ACT_NONE - BN(conv_head(x15)) with BN folded into head.w / head.b, the pre-swish values of the head GEMM - into
// z_out [n][49][1280] in the handle's activation type.  One extra launch of the same GEMM (same tile-table entry: the
// table's key has no activation); the classify path itself is not touched.
int b0_head_preact(dfd_handle* h, int n, void* z_out) {
    const B0Plan& P = h->b0;
    const B0Block& last = P.blocks.back();
    const int hw = last.h_out * last.h_out;
    if (h->act_bf16)
        return pointwise_t<bf16_t>(h, reinterpret_cast<const bf16_t*>(b0_last_block_out(h)), P.head_w, P.head_b, nullptr, nullptr,
                                   static_cast<bf16_t*>(z_out), n * hw, last.c_out, 1280, hw, ACT_NONE);
    return pointwise_t<float>(h, b0_last_block_out(h), P.head_w, P.head_b, nullptr, nullptr, static_cast<float*>(z_out),
                              n * hw, last.c_out, 1280, hw, ACT_NONE);
}

// fp32 activation storage, or - dfd_set_option(h, "bf16_activations", 1) - bf16 storage of every activation tensor
// that reaches HBM (depthwise / block / expand / head outputs) with fp32 arithmetic and accumulation throughout:
// BASELINE.json configs[3].  Squeeze-excite pools, gates, the pooled feature vector and the MLP head stay fp32.
int b0_forward(dfd_handle* h, const float* x, int n, float* logits_dev, B0Tap* tap, B0Prof* prof) {
    if (n > 0) h->classifier_crops += (unsigned long long)n;
    return h->act_bf16 ? b0_forward_t<bf16_t>(h, x, n, logits_dev, tap, prof)
                       : b0_forward_t<float>(h, x, n, logits_dev, tap, prof);
}

}  // namespace dfd
