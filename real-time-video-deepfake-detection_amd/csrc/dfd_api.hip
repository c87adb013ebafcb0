// extern "C" surface of libdfd_hip.so (declared in include/dfd_hip.h).
#include "b0_kernels.h"
#include "dfd_common.h"

using namespace dfd;

namespace {

int dev_alloc(dfd_handle* h, size_t bytes, float** out) {
    void* p = nullptr;
    DFD_HIP_TRY(h, hipMalloc(&p, bytes ? bytes : 4));
    h->owned.push_back(p);
    *out = static_cast<float*>(p);
    return DFD_OK;
}

// deterministic pseudo-random crops for dfd_warmup (roughly the range of normalised pixels)
__global__ __launch_bounds__(256) void fill_pattern_kernel(float* __restrict__ x, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t v = (uint32_t)i * 2654435761u;
    v ^= v >> 15; v *= 2246822519u; v ^= v >> 13;
    x[i] = ((float)(v >> 8) * (1.0f / 16777216.0f) - 0.5f) * 4.0f;
}

// dfd_gemm_tap's view of a WHOLE result that is too large to return: out[0] += elements still at the sentinel, out[1] +=
// sum of element i x (2 i + 1) mod 2^64 - position-sensitive (an odd multiplier is a bijection mod 2^64: a row written
// to another place changes it) and, being a sum, independent of the order the threads arrive in
template <typename T>
__global__ __launch_bounds__(256) void tap_digest_kernel(const T* __restrict__ y, size_t count, T sentinel,
                                                         unsigned long long* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * 256;
    unsigned long long left = 0, sum = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const T v = y[i];
        left += v == sentinel ? 1u : 0u;
        sum += (unsigned long long)v * (2ull * i + 1ull);
    }
    atomicAdd(out, left);
    atomicAdd(out + 1, sum);
}

int create_impl(dfd_handle* h, int device, const void* blob, size_t blob_len, int max_batch) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(h, DFD_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(h, DFD_ERR_ARG, "device %d out of range (0..%d)", device, ndev - 1);
    DFD_HIP_TRY(h, hipSetDevice(device));
    hipDeviceProp_t prop;
    DFD_HIP_TRY(h, hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(h, DFD_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    h->device = device;
    h->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->max_batch = max_batch;
    if (const char* e = getenv("DFD_FUSE_EXPAND")) h->fuse_expand = atoi(e) != 0;
    if (const char* e = getenv("DFD_FUSE_STEM")) h->fuse_stem = atoi(e) != 0;
    if (const char* e = getenv("DFD_FUSE_PROJ0")) h->fuse_proj0 = atoi(e) != 0;
    if (const char* e = getenv("DFD_FUSE_LATE")) h->fuse_late = atoi(e) != 0;
    if (const char* e = getenv("DFD_FUSE_LATE_SKIP")) h->fuse_late_skip = atoi(e);
    if (const char* e = getenv("DFD_FUSE_K5")) h->fuse_k5 = atoi(e) != 0;
    if (const char* e = getenv("DFD_FUSE_K5_MIN")) h->fuse_k5_min = atoi(e);
    if (const char* e = getenv("DFD_SPLIT_GEMM")) h->split_gemm = atoi(e) != 0;
    if (const char* e = getenv("DFD_BF16_ACTIVATIONS")) h->act_bf16 = atoi(e) != 0;
    if (const char* e = getenv("DFD_JPEG_DEVICE_RESTART")) h->jpeg_device_restart = atoi(e) != 0;
    if (const char* e = getenv("DFD_JPEG_PROGRESSIVE")) h->jpeg_progressive = atoi(e) != 0;
    h->gemm = s6_table_create();
    if (!h->gemm) return fail(h, DFD_ERR_ARG, "out of host memory");
    DFD_HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    DFD_HIP_TRY(h, hipEventCreate(&h->ev0));
    DFD_HIP_TRY(h, hipEventCreate(&h->ev1));

    std::string perr;
    if (!parse_blob(blob, blob_len, &h->tensors, &perr)) return fail(h, DFD_ERR_BLOB, "%s", perr.c_str());
    // one device allocation for all weights, 256-byte aligned slots
    size_t total = 0;
    for (auto& kv : h->tensors) total += (kv.second.count * 4 + 255) / 256 * 256;
    float* wbase = nullptr;
    int rc = dev_alloc(h, total, &wbase);
    if (rc) return rc;
    size_t off = 0;
    for (auto& kv : h->tensors) {
        Tensor& t = kv.second;
        t.dev = reinterpret_cast<float*>(reinterpret_cast<char*>(wbase) + off);
        DFD_HIP_TRY(h, hipMemcpy(t.dev, t.host, t.count * 4, hipMemcpyHostToDevice));
        t.host = nullptr;
        off += (t.count * 4 + 255) / 256 * 256;
    }
    if ((rc = b0_build_plan(h))) return rc;
    if ((rc = color_tables_init(h))) return rc;
    if ((rc = ssd_init(h))) return rc;
    if ((rc = mtcnn_init(h))) return rc;
    if ((rc = haar_init(h))) return rc;

    const B0Plan& P = h->b0;
    const size_t nb = (size_t)max_batch;
    if ((rc = dev_alloc(h, nb * 3 * 224 * 224 * 4, &h->in_nchw))) return rc;
    if ((rc = dev_alloc(h, nb * P.io_floats * 4, &h->io0))) return rc;
    if ((rc = dev_alloc(h, nb * P.io_floats * 4, &h->io1))) return rc;
    if ((rc = dev_alloc(h, nb * P.exp_floats * 4, &h->expbuf))) return rc;
    if ((rc = dev_alloc(h, nb * P.dw_floats * 4, &h->dwbuf))) return rc;
    if ((rc = dev_alloc(h, nb * P.pool_floats * 4, &h->pool))) return rc;
    if ((rc = dev_alloc(h, nb * P.gate_floats * 4, &h->gate))) return rc;
    if ((rc = dev_alloc(h, nb * 49 * 1280 * 4, &h->headbuf))) return rc;
    if ((rc = dev_alloc(h, nb * 1280 * 4, &h->feat))) return rc;
    if ((rc = dev_alloc(h, nb * 512 * 4, &h->fc1))) return rc;
    if ((rc = dev_alloc(h, nb * 256 * 4, &h->fc2))) return rc;
    if ((rc = dev_alloc(h, nb * 4, &h->logits))) return rc;
    DFD_HIP_TRY(h, stream_sync(h));           // the set-up copies enqueued above (mtcnn_init) have landed
    return DFD_OK;
}

void destroy_impl(dfd_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) stream_sync(h);
    comm_destroy(h);
    head_train_destroy(h);
    haar_destroy(h);
    forensic_destroy(h);
    ssd_destroy(h);
    mtcnn_destroy(h);
    freq_destroy(h);
    freq_domain_destroy(h);
    s6_table_destroy(h->gemm);
    h->gemm = nullptr;
    for (void* p : h->owned)
        if (p) hipFree(p);
    for (int i = 0; i < 2; ++i) {
        if (h->copy_done[i]) hipEventDestroy(h->copy_done[i]);
        if (h->slot_free[i]) hipEventDestroy(h->slot_free[i]);
    }
    if (h->copy_stream) hipStreamDestroy(h->copy_stream);
    for (int i = 0; i < 2; ++i) {
        if (h->jpeg_done[i]) hipEventDestroy(h->jpeg_done[i]);
        if (h->frames_free[i]) hipEventDestroy(h->frames_free[i]);
    }
    h->jpeg_stream = nullptr;                     // (the handle's second compute stream: destroyed below)
    if (h->aux_stream) {
        hipStreamSynchronize(h->aux_stream);
        hipStreamDestroy(h->aux_stream);
        hipEventDestroy(h->aux_go);
        hipEventDestroy(h->aux_done);
    }
    if (h->jpeg_host) hipHostFree(h->jpeg_host);
    if (h->mailbox) hipHostFree(h->mailbox);
    for (char* p : h->mailbox_old) hipHostFree(p);
    for (char* p : h->mailbox_old_prev) hipHostFree(p);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->order_ev) hipEventDestroy(h->order_ev);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

}  // namespace

extern "C" {

int dfd_abi_version(void) { return DFD_ABI_VERSION; }

int dfd_create(int device, const void* blob, size_t blob_len, int max_batch, dfd_handle** out) {
    if (!out) return fail(nullptr, DFD_ERR_ARG, "dfd_create: out is null");
    *out = nullptr;
    if (!blob || max_batch <= 0 || max_batch > 4096)
        return fail(nullptr, DFD_ERR_ARG, "dfd_create: blob is null or max_batch outside 1..4096");
    dfd_handle* h = new (std::nothrow) dfd_handle();
    if (!h) return fail(nullptr, DFD_ERR_ARG, "dfd_create: out of host memory");
    const int rc = create_impl(h, device, blob, blob_len, max_batch);
    if (rc != DFD_OK) {
        g_create_error = h->err;
        destroy_impl(h);
        return rc;
    }
    *out = h;
    return DFD_OK;
}

void dfd_destroy(dfd_handle* h) { destroy_impl(h); }

const char* dfd_last_error(const dfd_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int dfd_max_batch(const dfd_handle* h) { return h ? h->max_batch : DFD_ERR_ARG; }

int dfd_set_option(dfd_handle* h, const char* name, int value) {
    if (!h || !name) return DFD_ERR_ARG;
    if (strcmp(name, "fuse_expand") == 0) { h->fuse_expand = value != 0; return DFD_OK; }
    if (strcmp(name, "fuse_late") == 0) { h->fuse_late = value != 0; return DFD_OK; }
    if (strcmp(name, "fuse_late_skip") == 0) { h->fuse_late_skip = value; return DFD_OK; }   // < 0: the default again
    if (strcmp(name, "fuse_k5") == 0) { h->fuse_k5 = value != 0; return DFD_OK; }
    if (strcmp(name, "fuse_k5_min") == 0) { h->fuse_k5_min = value; return DFD_OK; }                  // <= 0: the default again
    if (strcmp(name, "fuse_stem") == 0) { h->fuse_stem = value != 0; return DFD_OK; }
    if (strcmp(name, "fuse_proj0") == 0) { h->fuse_proj0 = value != 0; return DFD_OK; }
    if (strcmp(name, "split_gemm") == 0) { h->split_gemm = value != 0; return DFD_OK; }
    if (strcmp(name, "mtcnn") == 0) { h->use_mtcnn = value != 0; return DFD_OK; }
    if (strcmp(name, "overlap_forensics") == 0) { h->overlap_forensics = value != 0; return DFD_OK; }
    if (strcmp(name, "forensic_chunk_bytes") == 0) { h->forensic_chunk_bytes = value > 0 ? (size_t)value : (size_t)256 << 20; return DFD_OK; }
    if (strcmp(name, "bf16_activations") == 0) { h->act_bf16 = value != 0; return DFD_OK; }
    if (strcmp(name, "bf16_weight_planes") == 0) {
        if (value != 1 && value != 3) return fail(h, DFD_ERR_ARG, "bf16_weight_planes must be 1 or 3");
        h->bf16_planes = value;
        return DFD_OK;
    }
    if (strcmp(name, "gemm_tile") == 0) { s6_table_set_force(h->gemm, value); return DFD_OK; }
    if (strcmp(name, "jpeg_device_entropy") == 0) { h->jpeg_device_entropy = value < 0 ? 0 : value; return DFD_OK; }
    if (strcmp(name, "jpeg_device_restart") == 0) { h->jpeg_device_restart = value != 0; return DFD_OK; }
    if (strcmp(name, "jpeg_progressive") == 0) { h->jpeg_progressive = value != 0; return DFD_OK; }
    if (strcmp(name, "jpeg_device_progressive") == 0) { h->jpeg_device_progressive = value != 0; return DFD_OK; }
    if (strcmp(name, "jpeg_rounds") == 0) { h->jpeg_rounds = value; return DFD_OK; }
    if (strcmp(name, "jpeg_chunk_bytes") == 0) {
        if (value < 256 || value > (1 << 20) || (value & (value - 1))) return fail(h, DFD_ERR_ARG, "jpeg_chunk_bytes: a power of two in 256 .. 2^20");
        h->jpeg_chunk_bytes = value;
        return DFD_OK;
    }
    if (strcmp(name, "stream_priority") == 0) {
        // the handle's main stream re-created at another priority (1 high, 0 normal, -1 low).  The runtime draws the
        // hardware queue of a stream from a pool per priority: two handles whose main streams have different priorities
        // can never be mapped onto one hardware queue (where their launches would run in line)
        if (value < -1 || value > 1) return fail(h, DFD_ERR_ARG, "stream_priority must be -1, 0 or 1");
        DFD_HIP_TRY(h, hipSetDevice(h->device));
        DFD_HIP_TRY(h, stream_sync(h));
        // the handle's other streams exchange events with the main one (forensic set, uploads, JPEG decode): drained too
        if (h->aux_stream) DFD_HIP_TRY(h, hipStreamSynchronize(h->aux_stream));
        if (h->copy_stream) DFD_HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
        int least = 0, greatest = 0;
        DFD_HIP_TRY(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
        const int prio = value > 0 ? greatest : (value < 0 ? least : (least + greatest) / 2);
        hipStream_t fresh = nullptr;
        DFD_HIP_TRY(h, hipStreamCreateWithPriority(&fresh, hipStreamNonBlocking, prio));
        hipStreamDestroy(h->stream);
        h->stream = fresh;
        return DFD_OK;
    }
    if (strcmp(name, "profile_stride") == 0) { h->prof_stride = value > 0 ? value : 1; return DFD_OK; }
    return fail(h, DFD_ERR_ARG, "unknown option '%s'", name);
}

int dfd_warmup(dfd_handle* h, int n_crops, int n_frames) {
    if (!h) return DFD_ERR_ARG;
    if (n_crops < 0 || n_crops > h->max_batch || n_frames < 0)
        return fail(h, DFD_ERR_ARG, "warmup: n_crops outside 0..%d or n_frames negative", h->max_batch);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    s6_table_set_tuning(h->gemm, true);
    h->warming = true;
    int rc = DFD_OK;
    if (n_crops > 0) {
        const size_t cnt = (size_t)n_crops * 3 * 224 * 224;
        hipLaunchKernelGGL(fill_pattern_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, h->in_nchw, cnt);
        rc = b0_forward(h, h->in_nchw, n_crops, h->logits, nullptr, nullptr);
    }
    if (rc == DFD_OK && n_frames > 0) rc = ssd_warmup(h, n_frames);
    s6_table_set_tuning(h->gemm, false);
    h->warming = false;
    if (rc) return rc;
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_classifier_crop_count(const dfd_handle* h, unsigned long long* total) {
    if (!h || !total) return DFD_ERR_ARG;
    *total = h->classifier_crops;
    return DFD_OK;
}

int dfd_jpeg_decode_counts(const dfd_handle* h, unsigned long long* on_device, unsigned long long* on_host) {
    if (!h || !on_device || !on_host) return DFD_ERR_ARG;
    *on_device = h->jpeg_frames_device;
    *on_host = h->jpeg_frames_host;
    return DFD_OK;
}

int dfd_gemm_tile_count(void) { return s6_max_candidates(); }

int dfd_tiles_export(dfd_handle* h, char* text_out, size_t capacity, size_t* length) {
    if (!h || !length) return DFD_ERR_ARG;
    const std::string t = s6_table_export(h->gemm);
    *length = t.size();
    if (!text_out) return DFD_OK;                                 // size query
    if (t.size() > capacity) return fail(h, DFD_ERR_ARG, "tiles_export: %zu bytes needed, capacity %zu", t.size(), capacity);
    memcpy(text_out, t.data(), t.size());
    return DFD_OK;
}

int dfd_tiles_import(dfd_handle* h, const char* text, size_t length, int* accepted) {
    if (!h || (!text && length)) return DFD_ERR_ARG;
    const int n = s6_table_import(h->gemm, text, length);
    if (accepted) *accepted = n < 0 ? 0 : n;
    return n < 0 ? fail(h, DFD_ERR_ARG, "tiles_import: bad arguments") : DFD_OK;
}

long long dfd_gemm_chunk_rows(long long rows, long long row_bytes, long long rows_per_image) {
    return s6_chunk_rows(rows, row_bytes, rows_per_image);
}

int dfd_gemm_tap(dfd_handle* h, dfd_gemm_tap_params* p) {
    if (!h || !p) return DFD_ERR_ARG;
    p->candidates = p->launches = 0;
    for (int i = 0; i < 6; ++i) p->tile[i] = 0;
    if (!p->X || !p->Wt || !p->bias || !p->Y) return fail(h, DFD_ERR_ARG, "gemm_tap: X, Wt, bias or Y is null");
    const bool bf = p->bf16 != 0, conv = p->conv != 0;
    if ((p->planes != 3 && !(p->planes == 1 && bf)) || p->act < ACT_NONE || p->act > ACT_PRELU)
        return fail(h, DFD_ERR_ARG, "gemm_tap: planes must be 3 (or 1 with bf16), act 0..3");
    ConvGeom g{};
    if (conv) {
        if (p->gate || p->x_rows > 0) return fail(h, DFD_ERR_ARG, "gemm_tap: gate and x_rows are pointwise only");
        if (p->n_img <= 0 || p->H <= 0 || p->W <= 0 || p->Cin <= 0 || p->ksize <= 0 || p->stride <= 0 || p->pad < 0 || p->dil <= 0)
            return fail(h, DFD_ERR_ARG, "gemm_tap: bad conv geometry");
        const int span = p->dil * (p->ksize - 1) + 1;
        if (p->H + 2 * p->pad < span || p->W + 2 * p->pad < span) return fail(h, DFD_ERR_ARG, "gemm_tap: kernel larger than the padded image");
        g.H = p->H; g.W = p->W; g.Cin = p->Cin; g.ksize = p->ksize; g.stride = p->stride; g.pad = p->pad; g.dil = p->dil;
        g.Ho = (p->H + 2 * p->pad - span) / p->stride + 1;
        g.Wo = (p->W + 2 * p->pad - span) / p->stride + 1;
        if ((p->Ho && p->Ho != g.Ho) || (p->Wo && p->Wo != g.Wo)) return fail(h, DFD_ERR_ARG, "gemm_tap: Ho x Wo must be %d x %d", g.Ho, g.Wo);
        const long long rows = (long long)p->n_img * g.Ho * g.Wo, kk = (long long)p->ksize * p->ksize * p->Cin;
        if (rows > (1ll << 30) || kk > (1ll << 20)) return fail(h, DFD_ERR_ARG, "gemm_tap: conv too large");
        p->Ho = g.Ho; p->Wo = g.Wo; p->M = (int)rows; p->K = (int)kk; p->HW = g.Ho * g.Wo;
    }
    const int M = p->M, K = p->K, N = p->N, HW = conv ? 1 : (p->HW > 0 ? p->HW : 1);
    if (M <= 0 || K <= 0 || N <= 0 || K > (1 << 20) || N > (1 << 16) || p->x_rows < 0 || p->x_rows > M)
        return fail(h, DFD_ERR_ARG, "gemm_tap: bad M, K, N or x_rows");
    if (p->n_ranges < 0 || (p->n_ranges > 0 && !p->y_ranges)) return fail(h, DFD_ERR_ARG, "gemm_tap: bad y_ranges");
    for (int i = 0; i < p->n_ranges; ++i)
        if (p->y_ranges[2 * i] < 0 || p->y_ranges[2 * i] >= p->y_ranges[2 * i + 1] || p->y_ranges[2 * i + 1] > M)
            return fail(h, DFD_ERR_ARG, "gemm_tap: y_ranges[%d] is not a range of rows inside 0..%d", i, M);
    p->y_sentinels = p->y_digest = 0;
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    const size_t esz = bf ? 2 : 4, G = DFD_GEMM_TAP_GUARD;
    const size_t xrows_host = conv ? 0 : (size_t)(p->x_rows > 0 ? p->x_rows : M);
    const size_t xcount = conv ? (size_t)p->n_img * g.H * g.W * g.Cin : (size_t)M * K;
    const size_t xhost = conv ? xcount : xrows_host * K;
    const size_t ycount = ((size_t)M + 2 * G) * N, nb = (size_t)(p->act == ACT_PRELU ? 2 * N : N);
    const size_t gcount = p->gate ? (size_t)((M + HW - 1) / HW) * K : 0;
    // the launchers' rule (gemm_split.hip): a chunk is bounded by the largest of the X, Y and R rows (conv: images)
    const long long row_bytes = conv ? std::max((long long)g.H * g.W * g.Cin, (long long)g.Ho * g.Wo * N) * (long long)esz
                                     : (long long)std::max(K, N) * (long long)esz;
    const bool ok = split_gemm_supports(K, N) && !(conv && g.Cin % 32 != 0) &&
                    s6_chunk_rows(conv ? p->n_img : M, row_bytes, p->gate ? HW : 1) > 0;
    // one allocation, 256-byte slots: Y (guard rows, result, guard rows) first, then the operands
    size_t total = 0;
    auto slot = [&](size_t bytes) { const size_t at = total; total += (bytes + 255) / 256 * 256; return at; };
    const size_t oy = slot(ycount * esz);
    const size_t ox = slot(ok ? xcount * esz : 0), ow = slot(ok ? (size_t)N * K * 4 : 0), ow3 = slot(ok ? split_weights_count(N, K) * 6 : 0);
    const size_t ob = slot(ok ? nb * 4 : 0), og = slot(ok ? gcount * 4 : 0), orr = slot(ok && p->R ? (size_t)M * N * esz : 0);
    const size_t od = slot(2 * sizeof(unsigned long long));
    char* base = nullptr;
    DFD_HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&base), total + 256));
    auto run = [&]() -> int {
        void* dy = base + oy;
        if (bf) DFD_HIP_TRY(h, hipMemsetD16Async(dy, (unsigned short)(DFD_GEMM_TAP_SENTINEL >> 16), ycount, h->stream));
        else DFD_HIP_TRY(h, hipMemsetD32Async(dy, (int)DFD_GEMM_TAP_SENTINEL, ycount, h->stream));
        if (ok) {
            char* dx = base + ox;
            float *dw = reinterpret_cast<float*>(base + ow), *db = reinterpret_cast<float*>(base + ob);
            unsigned short* w3 = reinterpret_cast<unsigned short*>(base + ow3);
            const float* dg = p->gate ? reinterpret_cast<const float*>(base + og) : nullptr;
            const void* dr = p->R ? base + orr : nullptr;
            DFD_HIP_TRY(h, hipMemcpyAsync(dx, p->X, xhost * esz, hipMemcpyHostToDevice, h->stream));
            for (size_t r0 = xrows_host; !conv && r0 < (size_t)M; r0 += xrows_host)      // x_rows: the block repeated down the operand
                DFD_HIP_TRY(h, hipMemcpyAsync(dx + r0 * K * esz, dx, std::min(xrows_host, (size_t)M - r0) * K * esz, hipMemcpyDeviceToDevice,
                                              h->stream));
            DFD_HIP_TRY(h, hipMemcpyAsync(dw, p->Wt, (size_t)N * K * 4, hipMemcpyHostToDevice, h->stream));
            DFD_HIP_TRY(h, hipMemcpyAsync(db, p->bias, nb * 4, hipMemcpyHostToDevice, h->stream));
            if (p->gate) DFD_HIP_TRY(h, hipMemcpyAsync(base + og, p->gate, gcount * 4, hipMemcpyHostToDevice, h->stream));
            if (p->R) DFD_HIP_TRY(h, hipMemcpyAsync(base + orr, p->R, (size_t)M * N * esz, hipMemcpyHostToDevice, h->stream));
            launch_split_weights(dw, w3, N, K, h->stream, false);
            const long long before = s6_table_dispatches(h->gemm);
            const long long chunk = conv ? M : s6_chunk_rows(M, row_bytes, p->gate ? HW : 1);
            p->candidates = s6_call_candidates(conv, p->gate != nullptr, bf, p->planes, (int)std::min<long long>(chunk, M), K, N, HW, p->act,
                                               p->R != nullptr, p->res_first ? 1 : 0);
            bool launched;
            if (bf) {
                bf16_t* y = static_cast<bf16_t*>(dy) + G * N;
                const bf16_t *x = reinterpret_cast<const bf16_t*>(dx), *r = static_cast<const bf16_t*>(dr);
                launched = conv ? launch_conv_gemm_split<bf16_t>(h->gemm, x, w3, db, r, y, p->n_img, g, N, p->act, p->res_first != 0, p->planes, h->stream)
                                : launch_pointwise_split<bf16_t>(h->gemm, x, w3, db, dg, r, y, M, K, N, HW, p->act, p->planes, h->stream,
                                                                 p->res_first ? 1 : 0);
            } else {
                float* y = static_cast<float*>(dy) + G * N;
                const float *x = reinterpret_cast<const float*>(dx), *r = static_cast<const float*>(dr);
                launched = conv ? launch_conv_gemm_split<float>(h->gemm, x, w3, db, r, y, p->n_img, g, N, p->act, p->res_first != 0, 3, h->stream)
                                : launch_pointwise_split<float>(h->gemm, x, w3, db, dg, r, y, M, K, N, HW, p->act, 3, h->stream, p->res_first ? 1 : 0);
            }
            if (!launched) return fail(h, DFD_ERR_ARG, "gemm_tap: the launcher refused M=%d K=%d N=%d", M, K, N);
            DFD_HIP_TRY(h, hipGetLastError());
            p->launches = (int)(s6_table_dispatches(h->gemm) - before);
            s6_table_last(h->gemm, p->tile);
        }
        // the whole result's digest, then the copy back: everything, or the guard rows and the requested ranges only
        unsigned long long* dd = reinterpret_cast<unsigned long long*>(base + od);
        unsigned long long digest[2] = {0, 0};
        const size_t rcount = (size_t)M * N, row = (size_t)N * esz;
        const unsigned dgrid = (unsigned)std::min<size_t>((rcount + 255) / 256, 4096);
        DFD_HIP_TRY(h, hipMemsetAsync(dd, 0, sizeof digest, h->stream));
        if (bf) hipLaunchKernelGGL(tap_digest_kernel<unsigned short>, dim3(dgrid), dim3(256), 0, h->stream, static_cast<const unsigned short*>(dy) + G * N,
                                   rcount, (unsigned short)(DFD_GEMM_TAP_SENTINEL >> 16), dd);
        else hipLaunchKernelGGL(tap_digest_kernel<unsigned>, dim3(dgrid), dim3(256), 0, h->stream, static_cast<const unsigned*>(dy) + G * N,
                                rcount, (unsigned)DFD_GEMM_TAP_SENTINEL, dd);
        DFD_HIP_TRY(h, hipMemcpyAsync(digest, dd, sizeof digest, hipMemcpyDeviceToHost, h->stream));
        if (p->n_ranges == 0) {
            DFD_HIP_TRY(h, hipMemcpyAsync(p->Y, dy, ycount * esz, hipMemcpyDeviceToHost, h->stream));
        } else {
            char* out = static_cast<char*>(p->Y);
            const char* src = static_cast<const char*>(dy);
            DFD_HIP_TRY(h, hipMemcpyAsync(out, src, G * row, hipMemcpyDeviceToHost, h->stream));
            out += G * row;
            for (int i = 0; i < p->n_ranges; ++i) {
                const size_t lo = (size_t)p->y_ranges[2 * i], cnt = (size_t)p->y_ranges[2 * i + 1] - lo;
                DFD_HIP_TRY(h, hipMemcpyAsync(out, src + (G + lo) * row, cnt * row, hipMemcpyDeviceToHost, h->stream));
                out += cnt * row;
            }
            DFD_HIP_TRY(h, hipMemcpyAsync(out, src + (G + (size_t)M) * row, G * row, hipMemcpyDeviceToHost, h->stream));
        }
        DFD_HIP_TRY(h, stream_sync(h));
        p->y_sentinels = digest[0];
        p->y_digest = digest[1];
        if (!ok) return fail(h, DFD_ERR_UNSUPPORTED, "gemm_tap: K=%d N=%d%s is not a split-GEMM shape", K, N, conv ? " (conv: Cin % 32)" : "");
        return DFD_OK;
    };
    const int rc = run();
    if (rc != DFD_OK && rc != DFD_ERR_UNSUPPORTED) hipStreamSynchronize(h->stream);
    hipFree(base);
    return rc;
}

int dfd_device_alloc(dfd_handle* h, size_t bytes, void** dptr) {
    if (!h || !dptr) return DFD_ERR_ARG;
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, hipMalloc(dptr, bytes ? bytes : 4));
    return DFD_OK;
}

int dfd_device_free(dfd_handle* h, void* dptr) {
    if (!h) return DFD_ERR_ARG;
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipFree(dptr));
    return DFD_OK;
}

int dfd_memcpy_h2d(dfd_handle* h, void* dst, const void* src, size_t bytes) {
    if (!h || (!dst && bytes) || (!src && bytes)) return h ? fail(h, DFD_ERR_ARG, "memcpy_h2d: null pointer") : DFD_ERR_ARG;
    DFD_HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_memcpy_d2h(dfd_handle* h, void* dst, const void* src, size_t bytes) {
    if (!h || (!dst && bytes) || (!src && bytes)) return h ? fail(h, DFD_ERR_ARG, "memcpy_d2h: null pointer") : DFD_ERR_ARG;
    DFD_HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_sync(dfd_handle* h) {
    if (!h) return DFD_ERR_ARG;
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_wait_for(dfd_handle* h, dfd_handle* other) {
    if (!h || !other) return DFD_ERR_ARG;
    if (h == other) return DFD_OK;                               // a stream is ordered with itself
    if (h->device != other->device) return fail(h, DFD_ERR_ARG, "wait_for: handles on devices %d and %d", h->device, other->device);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    if (!h->order_ev) DFD_HIP_TRY(h, hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming));
    // the event is re-recorded per call: a stream wait captures the record that precedes it (HIP semantics), so an
    // earlier wait on the same event object keeps its own point
    DFD_HIP_TRY(h, hipEventRecord(h->order_ev, other->stream));
    DFD_HIP_TRY(h, hipStreamWaitEvent(h->stream, h->order_ev, 0));
    return DFD_OK;
}

void* dfd_frame_ptr(dfd_handle* h) { return h ? h->frame_buf.p : nullptr; }

int dfd_timer_begin(dfd_handle* h) {
    if (!h) return DFD_ERR_ARG;
    DFD_HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    return DFD_OK;
}

int dfd_timer_end(dfd_handle* h, float* ms) {
    if (!h || !ms) return DFD_ERR_ARG;
    DFD_HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    DFD_HIP_TRY(h, hipEventSynchronize(h->ev1));
    DFD_HIP_TRY(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return DFD_OK;
}

int dfd_classify_nchw_device(dfd_handle* h, const float* nchw_dev, int n, float* logits_dev) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_dev || !logits_dev) return fail(h, DFD_ERR_ARG, "classify: null pointer");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    // between profile_begin and profile_end every prof_stride-th forward carries the per-launch events (an event
    // after each of the ~63 launches costs 5 % of a batch-256 step: 3.85 vs 3.66 ms)
    const bool sample = h->prof.enabled && (h->prof_seen++ % h->prof_stride == 0);
    if (sample) ++h->prof_steps;
    return b0_forward(h, nchw_dev, n, logits_dev, nullptr, sample ? &h->prof : nullptr);
}

int dfd_classify_nchw(dfd_handle* h, const float* nchw_host, int n, float* logits_host) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_host || !logits_host) return fail(h, DFD_ERR_ARG, "classify: null pointer");
    if (n <= 0 || n > h->max_batch) return fail(h, n <= 0 ? DFD_ERR_ARG : DFD_ERR_CAPACITY, "classify: batch %d outside 1..%d", n, h->max_batch);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, hipMemcpyAsync(h->in_nchw, nchw_host, (size_t)n * 3 * 224 * 224 * 4, hipMemcpyHostToDevice, h->stream));
    const int rc = b0_forward(h, h->in_nchw, n, h->logits, nullptr, nullptr);
    if (rc) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(logits_host, h->logits, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_extract_features(dfd_handle* h, const float* nchw_host, int n, float* feat_host) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_host || !feat_host) return fail(h, DFD_ERR_ARG, "extract_features: null pointer");
    if (n <= 0 || n > h->max_batch) return fail(h, n <= 0 ? DFD_ERR_ARG : DFD_ERR_CAPACITY, "extract_features: batch %d outside 1..%d", n, h->max_batch);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, hipMemcpyAsync(h->in_nchw, nchw_host, (size_t)n * 3 * 224 * 224 * 4, hipMemcpyHostToDevice, h->stream));
    const int rc = b0_forward(h, h->in_nchw, n, nullptr, nullptr, nullptr);
    if (rc) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(feat_host, h->feat, (size_t)n * 1280 * 4, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_extract_trunk(dfd_handle* h, const float* nchw_host, int n, float* trunk_host) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_host || !trunk_host) return fail(h, DFD_ERR_ARG, "extract_trunk: null pointer");
    if (n <= 0 || n > h->max_batch) return fail(h, n <= 0 ? DFD_ERR_ARG : DFD_ERR_CAPACITY, "extract_trunk: batch %d outside 1..%d", n, h->max_batch);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, hipMemcpyAsync(h->in_nchw, nchw_host, (size_t)n * 3 * 224 * 224 * 4, hipMemcpyHostToDevice, h->stream));
    return b0_trunk_to_host(h, h->in_nchw, n, trunk_host);
}

int dfd_extract_trunk_at(dfd_handle* h, const float* nchw_host, int n, int block, float* out_host) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_host || !out_host) return fail(h, DFD_ERR_ARG, "extract_trunk_at: null pointer");
    if (block != 14 && block != 15) return fail(h, DFD_ERR_ARG, "extract_trunk_at: block %d; 14 or 15", block);
    if (n <= 0 || n > h->max_batch) return fail(h, n <= 0 ? DFD_ERR_ARG : DFD_ERR_CAPACITY, "extract_trunk_at: batch %d outside 1..%d", n, h->max_batch);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, hipMemcpyAsync(h->in_nchw, nchw_host, (size_t)n * 3 * 224 * 224 * 4, hipMemcpyHostToDevice, h->stream));
    return b0_trunk_to_host(h, h->in_nchw, n, out_host, block);
}

int dfd_extract_block_out(dfd_handle* h, const float* nchw_host, int n, int block, float* out_host) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_host || !out_host) return fail(h, DFD_ERR_ARG, "extract_block_out: null pointer");
    if (block < 13 || block > 15) return fail(h, DFD_ERR_ARG, "extract_block_out: block %d; 13, 14 or 15", block);
    if (n <= 0 || n > h->max_batch) return fail(h, n <= 0 ? DFD_ERR_ARG : DFD_ERR_CAPACITY, "extract_block_out: batch %d outside 1..%d", n, h->max_batch);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, hipMemcpyAsync(h->in_nchw, nchw_host, (size_t)n * 3 * 224 * 224 * 4, hipMemcpyHostToDevice, h->stream));
    return b0_trunk_to_host(h, h->in_nchw, n, out_host, block);
}

int dfd_extract_block_input(dfd_handle* h, const float* nchw_host, int n, int block, float* out_host) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_host || !out_host) return fail(h, DFD_ERR_ARG, "extract_block_input: null pointer");
    if (block < 12 || block > 15) return fail(h, DFD_ERR_ARG, "extract_block_input: block %d; 12, 13, 14 or 15", block);
    if (n <= 0 || n > h->max_batch) return fail(h, n <= 0 ? DFD_ERR_ARG : DFD_ERR_CAPACITY, "extract_block_input: batch %d outside 1..%d", n, h->max_batch);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, hipMemcpyAsync(h->in_nchw, nchw_host, (size_t)n * 3 * 224 * 224 * 4, hipMemcpyHostToDevice, h->stream));
    return b0_trunk_to_host(h, h->in_nchw, n, out_host, block - 1);        // a block's input is the output of the block below it
}

int dfd_extract_block_rows(dfd_handle* h, const float* nchw_host, int n, int block, float* out_host) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_host || !out_host) return fail(h, DFD_ERR_ARG, "extract_block_rows: null pointer");
    if (block < 11 || block > 15) return fail(h, DFD_ERR_ARG, "extract_block_rows: block %d; 11, 12, 13, 14 or 15", block);
    if (n <= 0 || n > h->max_batch) return fail(h, n <= 0 ? DFD_ERR_ARG : DFD_ERR_CAPACITY, "extract_block_rows: batch %d outside 1..%d", n, h->max_batch);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    DFD_HIP_TRY(h, hipMemcpyAsync(h->in_nchw, nchw_host, (size_t)n * 3 * 224 * 224 * 4, hipMemcpyHostToDevice, h->stream));
    return b0_trunk_to_host(h, h->in_nchw, n, out_host, block - 1);        // block 11's rows are block 10's output, [14][14][112]
}

int dfd_b0_tap(dfd_handle* h, const float* nchw_dev, int n, const char* name, float* out_host,
               size_t capacity, size_t* count) {
    if (!h) return DFD_ERR_ARG;
    if (!nchw_dev || !name || !out_host || !count) return fail(h, DFD_ERR_ARG, "tap: null pointer");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    B0Tap tap;
    tap.name = name;
    tap.out = out_host;
    tap.capacity = capacity;
    const int rc = b0_forward(h, nchw_dev, n, h->logits, &tap, nullptr);
    if (rc) return rc;
    DFD_HIP_TRY(h, stream_sync(h));
    if (!tap.found) return fail(h, DFD_ERR_ARG, "tap: unknown stage '%s'", name);
    *count = tap.count;
    return DFD_OK;
}

int dfd_b0_profile_begin(dfd_handle* h) {
    if (!h) return DFD_ERR_ARG;
    for (hipEvent_t e : h->prof.events) hipEventDestroy(e);
    h->prof.events.clear();
    h->prof.names.clear();
    h->prof.enabled = true;
    h->prof_steps = 0;
    h->prof_seen = 0;
    return DFD_OK;
}

int dfd_b0_profile_end(dfd_handle* h, float* ms_sum, const char** names, int max_layers, int* count,
                       int* steps) {
    if (!h) return DFD_ERR_ARG;
    if (!ms_sum || !names || !count || !steps) return fail(h, DFD_ERR_ARG, "profile_end: null pointer");
    h->prof.enabled = false;
    DFD_HIP_TRY(h, stream_sync(h));
    const int nsteps = h->prof_steps;
    const size_t per = nsteps > 0 ? h->prof.events.size() / nsteps : 0;   // marks per forward
    int k = 0;
    for (size_t i = 1; i < per && k < max_layers; ++i, ++k) {
        double acc = 0.0;
        for (int st = 0; st < nsteps; ++st) {
            float t = 0.f;
            hipEventElapsedTime(&t, h->prof.events[st * per + i - 1], h->prof.events[st * per + i]);
            acc += t;
        }
        ms_sum[k] = (float)acc;
        names[k] = h->prof.names[i];
    }
    for (hipEvent_t e : h->prof.events) hipEventDestroy(e);
    h->prof.events.clear();
    h->prof.names.clear();
    *count = k;
    *steps = nsteps;
    return DFD_OK;
}

}  // extern "C"
