// C ABI of the forensic analyzer: device statistics -> the reference's threshold scoring
// (reference frame_analysis.py:58-389), with the per-stream temporal state kept here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>

#include "dfd_common.h"
#include "forensic_kernels.h"
#include "forensic_sized_kernels.h"

using namespace dfd;

namespace dfd {

struct ForensicStream {
    void* prev_gray = nullptr;     // size * size bytes on the device
    int size = 0;                  // analysis edge, fixed by dfd_forensics_open or the stream's first frame (0: neither yet)
    bool general = false;          // opened (dfd_forensics_open): the fused entries run it on the general chain, at 256 too
    bool has_prev = false;
    std::deque<double> diffs;      // last 30 mean absolute differences
    int frame_count = 0;
};

struct ForensicState {
    std::map<int, ForensicStream> streams;
    DevBuf work;                   // carved by forensic_carve for `cap` frames
    int cap = 0;
    ForensicBuffers buf{};
    float2* twiddle = nullptr;
    double* diff_part = nullptr;   // 256 partial sums
    DevBuf pair_idx, pair_part;    // dfd_forensic_signals_device: predecessor indices, [n][256] partial sums
    double* host_res = nullptr;    // pinned: statistics of a batch that ran on the second stream (forensics_batch_begin)
    size_t host_res_cap = 0;
    DevBuf frame_desc, prev_tab, copy_tab;   // forensics_streams_run: FrameDesc [n], predecessor planes [n], write-backs
    DevBuf sized_gray, sized_part;           // ... its frames on the general chain: their gray planes, kept for the whole call
                                             // (a predecessor may sit in an earlier chunk), and their per-row partial sums
    DevBuf sized_diff_tab, sized_copy_tab;   // ... SizedDiffRow per such frame, SizedPlaneCopy per such stream
    std::map<int, std::vector<void*>> free_planes;   // stored planes of released streams by analysis edge, reused by the
                                                     // next new stream of that edge
    struct Sized {                           // dfd_forensics_sized / dfd_forensic_tap_sized: per analysis edge
        DevBuf work, tap_store;
        int cap = 0;
        ForensicBuffers buf{};
        float2* table = nullptr;             // exp(-2 pi i j / S), S entries
        double* diff_part = nullptr;         // S partial sums
    };
    std::map<int, Sized> sized;
    DevBuf tap_store;                        // dfd_forensic_tap: spectrum, logmag, edges; allocated on its first call
};

void forensic_destroy(dfd_handle* h) {
    if (h->forensic && h->forensic->host_res) hipHostFree(h->forensic->host_res);
    delete h->forensic;
    h->forensic = nullptr;
}

}  // namespace dfd

namespace {

int state_init(dfd_handle* h, int frames) {
    if (!h->forensic) {
        h->forensic = new ForensicState();
        float2 tw[128];
        for (int k = 0; k < 128; ++k) {
            const double a = -2.0 * M_PI * k / 256.0;
            tw[k] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
        void* d = nullptr;
        DFD_HIP_TRY(h, hipMalloc(&d, sizeof tw));
        h->owned.push_back(d);
        DFD_HIP_TRY(h, hipMemcpy(d, tw, sizeof tw, hipMemcpyHostToDevice));
        h->forensic->twiddle = static_cast<float2*>(d);
        DFD_HIP_TRY(h, hipMalloc(&d, 256 * 8));
        h->owned.push_back(d);
        h->forensic->diff_part = static_cast<double*>(d);
    }
    ForensicState& F = *h->forensic;
    if (frames > F.cap) {
        const int rc = ensure(h, &F.work, forensic_bytes_per_frame() * frames + 65536);
        if (rc) return rc;
        forensic_carve(F.work.p, frames, &F.buf);
        F.cap = frames;
    }
    return DFD_OK;
}

double pop_std(const double* v, int n, double* mean_out) {
    double m = 0;
    for (int i = 0; i < n; ++i) m += v[i];
    m /= n;
    double q = 0;
    for (int i = 0; i < n; ++i) q += (v[i] - m) * (v[i] - m);
    *mean_out = m;
    return std::sqrt(q / n);
}

double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

// the five stateless signals from the device statistics (frame_analysis.py:150-347); sc[5] (temporal) = 0
// npix: pixels of the analysis image; nblk: its 32x32 blocks (fewer than 4: noise and ELA score 0.0, reference :204,:255)
void static_scores(const double* st, const double* noise, const double* ela, bool full, double* sc, double* ex,
                   double npix = 65536.0, int nblk = 64, bool f32_means = false) {
    const double nan = std::nan("");
    sc[0] = 0; sc[1] = nan; sc[2] = nan; sc[3] = 0; sc[4] = nan; sc[5] = 0;
    // ---- frequency (:150-180)
    const double lo = st[ST_FREQ_LOW], mi = st[ST_FREQ_MID], hi = st[ST_FREQ_HIGH];
    const double total = lo + mi + hi + 1e-10, hr = hi / total, mr = mi / total;
    const double mid_cv = st[ST_FREQ_MID_STD] / (mi + 1e-10);
    double s = 0.0;
    if (hr < 0.18) s += 0.4; else if (hr < 0.22) s += 0.2;
    if (mid_cv > 0.6) s += 0.25; else if (mid_cv > 0.45) s += 0.1;
    if (mr > 0.45 && hr < 0.2) s += 0.15;
    sc[0] = clip01(s);
    // ---- edges (:296-309)
    const double density = st[ST_EDGE_COUNT] / npix, lap_var = st[ST_LAP_VAR];
    s = 0.0;
    if (density < 0.02) s += 0.35; else if (density < 0.04) s += 0.15;
    if (lap_var < 50) s += 0.3; else if (lap_var < 100) s += 0.1;
    sc[3] = clip01(s);
    double noise_mean = nan, noise_cv = nan, ela_mean = nan, ela_cv = nan;
    if (full && nblk < 4) sc[1] = sc[2] = 0.0;
    if (full && nblk >= 4) {
        // ---- noise (:207-225)
        noise_cv = pop_std(noise, nblk, &noise_mean) / (noise_mean + 1e-10);
        s = 0.0;
        if (noise_cv > 0.7) s += 0.5; else if (noise_cv > 0.5) s += 0.25;
        if (noise_mean < 1.0) s += 0.3; else if (noise_mean < 2.0) s += 0.1;
        sc[1] = clip01(s);
        // ---- ELA (:258-276)
        ela_cv = pop_std(ela, nblk, &ela_mean);
        // the reference's block means are float32 and so is their mean (:250-256); at 256x256 the quotient by 64 is exact
        if (f32_means) ela_mean = (double)(float)ela_mean;
        ela_cv = ela_cv / (ela_mean + 1e-10);
        s = 0.0;
        if (ela_cv > 0.9) s += 0.5; else if (ela_cv > 0.6) s += 0.2;
        if (ela_mean > 15) s += 0.2; else if (ela_mean > 10) s += 0.1;
        sc[2] = clip01(s);
    }
    if (full) {
        // ---- colour (:326-347)
        s = 0.0;
        if (st[ST_SAT_STD] < 15) s += 0.3; else if (st[ST_SAT_STD] < 25) s += 0.1;
        if (st[ST_VAL_STD] < 15) s += 0.25; else if (st[ST_VAL_STD] < 25) s += 0.1;
        if (st[ST_HUES] < 30) s += 0.25; else if (st[ST_HUES] < 50) s += 0.1;
        sc[4] = clip01(s);
    }
    const double e[10] = {lo, mi, hi, hr, mr, mid_cv, noise_mean, noise_cv, ela_mean, ela_cv};
    for (int i = 0; i < 10; ++i) ex[i] = e[i];
}

// the host half of one frame of a stream, in the stream's frame order: frame counter, temporal deque and signal
// (frame_analysis.py:358-389; dpart = the frame's 256 partial sums against its predecessor, read only when the stream
// has one), then the weighted sum in the reference's dict order (:49-56,88 / :118-119).  sc[6] / ex[10] as static_scores;
// *mean_diff / *temporal_cv: -1 / NaN when not computed.
double score_frame(ForensicStream& S, const double* st, const double* noise, const double* ela, bool full, const double* dpart,
                   double* sc, double* ex, double* mean_diff, double* temporal_cv, int npart = 256, double npix = 65536.0,
                   int nblk = 64, bool f32_means = false) {
    S.frame_count += 1;                                              // frame_analysis.py:68,110
    static_scores(st, noise, ela, full, sc, ex, npix, nblk, f32_means);
    *mean_diff = -1.0;
    *temporal_cv = std::nan("");
    if (!S.has_prev) {
        S.has_prev = true;
    } else {
        double sum = 0;
        for (int i = 0; i < npart; ++i) sum += dpart[i];
        // np.mean of a float32 plane (:364): the integer sum (exact in float32 below 2^24) divided in float32
        const double md = f32_means ? (double)((float)sum / (float)npix) : sum / npix;
        *mean_diff = md;
        S.diffs.push_back(md);
        if (S.diffs.size() > 30) S.diffs.pop_front();
        if (S.diffs.size() >= 5) {
            std::vector<double> d(S.diffs.begin(), S.diffs.end());
            double dm;
            const double tcv = pop_std(d.data(), (int)d.size(), &dm) / (dm + 1e-10);
            *temporal_cv = tcv;
            double s = 0.0;
            if (tcv > 1.5) s += 0.4; else if (tcv > 1.0) s += 0.2;
            if (md < 0.3 && S.frame_count > 10) s += 0.3;
            else if (md < 0.8 && S.frame_count > 10) s += 0.1;
            sc[5] = clip01(s);
        }
    }
    double comb = 0.0;
    if (full) {
        const double w[6] = {0.25, 0.20, 0.20, 0.15, 0.10, 0.10};
        for (int i = 0; i < 6; ++i) comb += sc[i] * w[i];
    } else {
        comb += sc[0] * 0.45;
        comb += sc[5] * 0.25;
        comb += sc[3] * 0.30;
    }
    return clip01(comb);
}

// the stream's stored gray plane: a released stream's plane when there is one (no hipMalloc on the serving path)
int stream_plane(dfd_handle* h, ForensicStream& S, int size = 256) {
    if (S.prev_gray) return DFD_OK;
    ForensicState& F = *h->forensic;
    std::vector<void*>& fl = F.free_planes[size];
    if (!fl.empty()) {
        S.prev_gray = fl.back();
        fl.pop_back();
        S.size = size;
        return DFD_OK;
    }
    DFD_HIP_TRY(h, hipMalloc(&S.prev_gray, (size_t)size * size));
    h->owned.push_back(S.prev_gray);
    S.size = size;
    return DFD_OK;
}

// a stream's analysis edge is fixed by its first frame: any entry at another edge is refused before it touches anything
int stream_size_check(dfd_handle* h, int stream_id, int size) {
    if (!h->forensic) return DFD_OK;
    auto it = h->forensic->streams.find(stream_id);
    if (it != h->forensic->streams.end() && it->second.size && it->second.size != size)
        return fail(h, DFD_ERR_STATE, "forensics: stream %d runs at analysis size %d, this call at %d (dfd_forensics_release frees it)",
                    stream_id, it->second.size, size);
    return DFD_OK;
}

// the fused entries (dfd_analyze_*) run a stream at the size it holds: on the general chain when it was opened or holds
// another size than 256, on the 256x256 kernels otherwise (a stream nobody opened, or one that has no frame yet)
bool on_general_chain(const ForensicStream& S) { return S.general || (S.size && S.size != 256); }

int sized_init(dfd_handle* h, int S, int frames, ForensicState::Sized** out) {
    ForensicState& F = *h->forensic;
    ForensicState::Sized& Z = F.sized[S];
    if (!Z.table) {
        std::vector<float2> tw(S);
        forensic_sized_table(S, tw.data());
        void* d = nullptr;
        DFD_HIP_TRY(h, hipMalloc(&d, (size_t)S * sizeof(float2)));
        h->owned.push_back(d);
        DFD_HIP_TRY(h, hipMemcpy(d, tw.data(), (size_t)S * sizeof(float2), hipMemcpyHostToDevice));
        Z.table = static_cast<float2*>(d);
        DFD_HIP_TRY(h, hipMalloc(&d, (size_t)S * 8));
        h->owned.push_back(d);
        Z.diff_part = static_cast<double*>(d);
    }
    if (frames > Z.cap) {
        const int rc = ensure(h, &Z.work, forensic_sized_bytes_per_frame(S) * frames + 65536);
        if (rc) return rc;
        forensic_sized_carve(Z.work.p, S, frames, &Z.buf);
        Z.cap = frames;
    }
    *out = &Z;
    return DFD_OK;
}

}  // namespace

namespace dfd {

// the analyzer on a frame that is already in HBM (shared by dfd_forensics and dfd_analyze_frame)
int forensics_run(dfd_handle* h, int stream_id, const uint8_t* frame_dev, int hh, int ww, int stride, int full,
                  double* scores_out, double* prob_out, double* stats_out) {
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    int rc = stream_size_check(h, stream_id, 256);
    if (rc) return rc;
    if ((rc = state_init(h, 1))) return rc;
    ForensicState& F = *h->forensic;
    ForensicStream& S = F.streams[stream_id];
    if ((rc = stream_plane(h, S))) return rc;

    launch_resize_bgr(frame_dev, 1, hh, ww, stride, 0, F.buf.rs, 256, 256, h->stream);
    launch_forensics(F.buf, 1, full != 0, h->color, F.twiddle, h->stream);
    if (S.has_prev) launch_absdiff(F.buf.gray, (const uint8_t*)S.prev_gray, F.diff_part, h->stream);
    double st[FORENSIC_STATS], noise[64], ela[64], dpart[256];
    DFD_HIP_TRY(h, hipMemcpyAsync(st, F.buf.stats, sizeof st, hipMemcpyDeviceToHost, h->stream));
    if (full) {
        DFD_HIP_TRY(h, hipMemcpyAsync(noise, F.buf.stats_noise, sizeof noise, hipMemcpyDeviceToHost, h->stream));
        DFD_HIP_TRY(h, hipMemcpyAsync(ela, F.buf.stats_ela, sizeof ela, hipMemcpyDeviceToHost, h->stream));
    }
    if (S.has_prev) DFD_HIP_TRY(h, hipMemcpyAsync(dpart, F.diff_part, sizeof dpart, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(S.prev_gray, F.buf.gray, 65536, hipMemcpyDeviceToDevice, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());

    const double nan = std::nan("");
    double sc[6], ex[10], mean_diff, temporal_cv;
    *prob_out = score_frame(S, st, noise, ela, full != 0, dpart, sc, ex, &mean_diff, &temporal_cv);
    const double lo = ex[0], mi = ex[1], hi = ex[2], hr = ex[3], mr = ex[4], mid_cv = ex[5];
    const double noise_mean = ex[6], noise_cv = ex[7], ela_mean = ex[8], ela_cv = ex[9];
    const double density = st[ST_EDGE_COUNT] / 65536.0, lap_var = st[ST_LAP_VAR];
    for (int i = 0; i < 6; ++i) scores_out[i] = sc[i];
    if (stats_out) {
        const double out[DFD_FORENSIC_NSTATS] = {lo, mi, hi, hr, mr, mid_cv, noise_mean, noise_cv, ela_mean, ela_cv,
                                                 density, lap_var, full ? st[ST_SAT_STD] : nan, full ? st[ST_VAL_STD] : nan,
                                                 full ? st[ST_HUES] : nan, mean_diff, temporal_cv, (double)S.frame_count};
        for (int i = 0; i < DFD_FORENSIC_NSTATS; ++i) stats_out[i] = out[i];
    }
    return DFD_OK;
}

// n frames of any streams and sizes in one pass (POST /analyze_batch, the session pool).  The frames are grouped by the
// chain and analysis edge of their stream: the frames of 256x256 streams nobody opened run on the 256x256 kernels as one
// launch set, the frames of every other edge S on the general chain - one ragged resize to S x S and one launch set per
// chunk of the group, a chunk being as many frames as fit the handle's work-memory budget (forensic_chunk_bytes; the
// kernels treat every frame on its own, so the split changes no result).  The gray planes of the general chain are kept
// for the whole call outside the chunk memory, so that ONE launch differences every such frame, whatever its edge and
// chunk, against its predecessor - the previous frame of its stream in this call, else the stream's stored plane - and
// ONE launch writes every stream's last gray plane back to its stored slot (the 256x256 group: its own two launches, as
// before).  Then the host half is replayed frame by frame in call order: every stream's temporal deque, frame counter
// and stored plane end exactly where single calls in order would leave them.  No stream's state moves before the wait.
int forensics_streams_run(dfd_handle* h, const uint8_t* frames_dev, const FrameDesc* fd, int n, const int* stream_ids,
                          const int* full, double* scores_out, double* prob_out) {
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    int rc = DFD_OK;
    if ((rc = state_init(h, 1))) return rc;
    ForensicState& F = *h->forensic;
    std::vector<int> plain;                                          // frames on the 256x256 kernels, in call order
    std::map<int, std::vector<int>> groups;                          // analysis edge -> frames on the general chain
    std::vector<int> edge(n);                                        // 0: 256x256 kernels
    size_t gray_bytes = 0, part_doubles = 0;
    int n_sized = 0, max_S = 0;
    for (int f = 0; f < n; ++f) {
        ForensicStream& S = F.streams[stream_ids[f]];
        edge[f] = on_general_chain(S) ? S.size : 0;
        if ((rc = stream_plane(h, S, edge[f] ? edge[f] : 256))) return rc;
        if (!edge[f]) { plain.push_back(f); continue; }
        groups[edge[f]].push_back(f);
        gray_bytes += (size_t)edge[f] * edge[f];
        part_doubles += (size_t)edge[f];
        max_S = std::max(max_S, edge[f]);
        ++n_sized;
    }
    const int n_plain = (int)plain.size();
    if (n_plain && (rc = state_init(h, n_plain))) return rc;
    if ((rc = ensure(h, &F.sized_gray, gray_bytes))) return rc;
    if ((rc = ensure(h, &F.sized_part, part_doubles * 8))) return rc;
    struct Chunk { int S, first, count; ForensicState::Sized* Z; bool full; };   // first: index into the group's frames
    std::vector<Chunk> chunks;
    for (const auto& g : groups) {
        const int S = g.first, cnt = (int)g.second.size();
        const size_t fit = h->forensic_chunk_bytes / forensic_sized_bytes_per_frame(S);
        const int per = (int)std::min<size_t>(std::max<size_t>(fit, 1), (size_t)cnt);
        ForensicState::Sized* Z = nullptr;
        if ((rc = sized_init(h, S, per, &Z))) return rc;
        bool any = false;
        for (int f : g.second) any = any || full[f] != 0;
        for (int c0 = 0; c0 < cnt; c0 += per) chunks.push_back(Chunk{S, c0, std::min(per, cnt - c0), Z, any});
    }
    // where every frame's gray plane and partial sums are, and its slot in the descriptor table (group by group)
    std::vector<const uint8_t*> gray(n);
    std::vector<size_t> part_at(n, 0);
    std::vector<FrameDesc> desc;
    desc.reserve(n);
    for (int j = 0; j < n_plain; ++j) {
        gray[plain[j]] = F.buf.gray + (size_t)j * 65536;
        desc.push_back(fd[plain[j]]);
    }
    {
        size_t go = 0, po = 0;
        for (const auto& g : groups)
            for (int f : g.second) {
                gray[f] = (const uint8_t*)F.sized_gray.p + go;
                part_at[f] = po;
                go += (size_t)g.first * g.first;
                po += (size_t)g.first;
                desc.push_back(fd[f]);
            }
    }
    bool any_full = false;                                           // of the 256x256 group
    std::vector<const uint8_t*> pred(n);                             // every frame's predecessor plane, or null
    std::map<int, int> last;                                         // stream -> its latest frame so far in this call
    for (int f = 0; f < n; ++f) {
        const ForensicStream& S = F.streams[stream_ids[f]];
        auto it = last.find(stream_ids[f]);
        pred[f] = it != last.end() ? gray[it->second] : S.has_prev ? (const uint8_t*)S.prev_gray : nullptr;
        last[stream_ids[f]] = f;
        if (!edge[f]) any_full = any_full || full[f] != 0;
    }
    std::vector<const uint8_t*> prev(n_plain);
    for (int j = 0; j < n_plain; ++j) prev[j] = pred[plain[j]];
    std::vector<SizedDiffRow> rows;
    for (const auto& g : groups)
        for (int f : g.second) rows.push_back(SizedDiffRow{gray[f], pred[f], (double*)F.sized_part.p + part_at[f], g.first, 0});
    std::vector<PlaneCopy> back;
    std::vector<SizedPlaneCopy> back_sized;
    for (const auto& kv : last) {
        uint8_t* dst = (uint8_t*)F.streams[kv.first].prev_gray;
        const int S = edge[kv.second];
        if (S) back_sized.push_back(SizedPlaneCopy{gray[kv.second], dst, (size_t)S * S});
        else back.push_back(PlaneCopy{gray[kv.second], dst});
    }
    if ((rc = ensure(h, &F.frame_desc, (size_t)n * sizeof(FrameDesc)))) return rc;
    if ((rc = ensure(h, &F.prev_tab, (size_t)n_plain * sizeof(void*)))) return rc;
    if ((rc = ensure(h, &F.copy_tab, back.size() * sizeof(PlaneCopy)))) return rc;
    if ((rc = ensure(h, &F.pair_part, (size_t)n_plain * 256 * 8))) return rc;
    if ((rc = ensure(h, &F.sized_diff_tab, rows.size() * sizeof(SizedDiffRow)))) return rc;
    if ((rc = ensure(h, &F.sized_copy_tab, back_sized.size() * sizeof(SizedPlaneCopy)))) return rc;
    if ((rc = mailbox_h2d(h, F.frame_desc.p, desc.data(), (size_t)n * sizeof(FrameDesc)))) return rc;
    const FrameDesc* desc_dev = (const FrameDesc*)F.frame_desc.p;
    // per frame: where the host finds its statistics once the stream has been waited for
    std::vector<const double*> st(n, nullptr), noise(n, nullptr), ela(n, nullptr), part(n, nullptr);
    if (n_plain) {
        if ((rc = mailbox_h2d(h, F.prev_tab.p, prev.data(), (size_t)n_plain * sizeof(void*)))) return rc;
        if ((rc = mailbox_h2d(h, F.copy_tab.p, back.data(), back.size() * sizeof(PlaneCopy)))) return rc;
        launch_resize_bgr_ragged(frames_dev, desc_dev, n_plain, F.buf.rs, 256, 256, h->stream);
        launch_forensics(F.buf, n_plain, any_full, h->color, F.twiddle, h->stream);
        launch_absdiff_prev(F.buf.gray, (const uint8_t* const*)F.prev_tab.p, (double*)F.pair_part.p, n_plain, h->stream);
        launch_copy_planes((const PlaneCopy*)F.copy_tab.p, (int)back.size(), h->stream);
        const double* a = (const double*)mailbox_d2h(h, F.buf.stats, (size_t)n_plain * FORENSIC_STATS * 8);
        const double* b = (const double*)mailbox_d2h(h, F.buf.stats_noise, (size_t)n_plain * 64 * 8);
        const double* c = (const double*)mailbox_d2h(h, F.buf.stats_ela, (size_t)n_plain * 64 * 8);
        const double* d = (const double*)mailbox_d2h(h, F.pair_part.p, (size_t)n_plain * 256 * 8);
        if (!a || !b || !c || !d) return fail(h, DFD_ERR_HIP, "forensics: mailbox allocation failed");
        for (int j = 0; j < n_plain; ++j) {
            const int f = plain[j];
            st[f] = a + (size_t)j * FORENSIC_STATS;
            noise[f] = b + (size_t)j * 64;
            ela[f] = c + (size_t)j * 64;
            part[f] = d + (size_t)j * 256;
        }
    }
    if (n_sized) {
        if ((rc = mailbox_h2d(h, F.sized_diff_tab.p, rows.data(), rows.size() * sizeof(SizedDiffRow)))) return rc;
        if ((rc = mailbox_h2d(h, F.sized_copy_tab.p, back_sized.data(), back_sized.size() * sizeof(SizedPlaneCopy)))) return rc;
        int at = n_plain;                                            // the chunk's first slot of the descriptor table
        for (const Chunk& c : chunks) {
            const std::vector<int>& frames = groups[c.S];
            const size_t nblk = (size_t)sized_blocks(c.S);
            ForensicBuffers B = c.Z->buf;                            // the chunk's work memory, its gray planes in the call's store
            B.gray = const_cast<uint8_t*>(gray[frames[c.first]]);
            launch_resize_bgr_ragged(frames_dev, desc_dev + at, c.count, B.rs, c.S, c.S, h->stream);
            DFD_HIP_TRY(h, launch_forensics_sized(B, c.S, c.count, c.full, h->color, c.Z->table, h->stream));
            const double* a = (const double*)mailbox_d2h(h, B.stats, (size_t)c.count * FORENSIC_STATS * 8);
            const double* b = c.full ? (const double*)mailbox_d2h(h, B.stats_noise, (size_t)c.count * nblk * 8) : nullptr;
            const double* e = c.full ? (const double*)mailbox_d2h(h, B.stats_ela, (size_t)c.count * nblk * 8) : nullptr;
            if (!a || (c.full && (!b || !e))) return fail(h, DFD_ERR_HIP, "forensics: mailbox allocation failed");
            for (int j = 0; j < c.count; ++j) {
                const int f = frames[c.first + j];
                st[f] = a + (size_t)j * FORENSIC_STATS;
                if (c.full) {
                    noise[f] = b + (size_t)j * nblk;
                    ela[f] = e + (size_t)j * nblk;
                }
            }
            at += c.count;
        }
        launch_absdiff_prev_sized((const SizedDiffRow*)F.sized_diff_tab.p, n_sized, max_S, h->stream);
        launch_copy_planes_sized((const SizedPlaneCopy*)F.sized_copy_tab.p, (int)back_sized.size(), max_S, h->stream);
        const double* d = (const double*)mailbox_d2h(h, F.sized_part.p, part_doubles * 8);
        if (!d) return fail(h, DFD_ERR_HIP, "forensics: mailbox allocation failed");
        for (int f = 0; f < n; ++f)
            if (edge[f]) part[f] = d + part_at[f];
    }
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());
    for (int f = 0; f < n; ++f) {
        double sc[6], ex[10], md, tcv;
        ForensicStream& S = F.streams[stream_ids[f]];
        const int e = edge[f];
        prob_out[f] = e ? score_frame(S, st[f], noise[f], ela[f], full[f] != 0, part[f], sc, ex, &md, &tcv, e, (double)e * (double)e,
                                      sized_blocks(e), true)
                        : score_frame(S, st[f], noise[f], ela[f], full[f] != 0, part[f], sc, ex, &md, &tcv);
        for (int i = 0; i < 6; ++i) scores_out[(size_t)f * 6 + i] = sc[i];
    }
    return DFD_OK;
}

// Stateless batch variant for throughput runs: n device frames -> six-signal probability each, the
// temporal signal taking its first-frame value 0 (frame_analysis.py:358-360).  One launch set for all frames.
int forensics_batch_run(dfd_handle* h, const uint8_t* frames_dev, int n, int hh, int ww, int stride, size_t frame_bytes,
                        double* prob_out, double* scores_out) {
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    int rc = state_init(h, n);
    if (rc) return rc;
    ForensicState& F = *h->forensic;
    launch_resize_bgr(frames_dev, n, hh, ww, stride, frame_bytes, F.buf.rs, 256, 256, h->stream);
    launch_forensics(F.buf, n, true, h->color, F.twiddle, h->stream);
    // a few KB per frame, through the mailbox (dfd_common.h) rather than the DMA engines
    const double* st = (const double*)mailbox_d2h(h, F.buf.stats, (size_t)n * FORENSIC_STATS * 8);
    const double* noise = (const double*)mailbox_d2h(h, F.buf.stats_noise, (size_t)n * 64 * 8);
    const double* ela = (const double*)mailbox_d2h(h, F.buf.stats_ela, (size_t)n * 64 * 8);
    if (!st || !noise || !ela) return fail(h, DFD_ERR_HIP, "forensics: mailbox allocation failed");
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());
    const double w[6] = {0.25, 0.20, 0.20, 0.15, 0.10, 0.10};
    for (int f = 0; f < n; ++f) {
        double sc[6], ex[10];
        static_scores(&st[(size_t)f * FORENSIC_STATS], &noise[(size_t)f * 64], &ela[(size_t)f * 64], true, sc, ex);
        double comb = 0.0;
        for (int i = 0; i < 6; ++i) comb += sc[i] * w[i];
        prob_out[f] = clip01(comb);
        if (scores_out)
            for (int i = 0; i < 6; ++i) scores_out[(size_t)f * 6 + i] = sc[i];
    }
    return DFD_OK;
}

int forensics_batch_begin(dfd_handle* h, const uint8_t* frames_dev, int n, int hh, int ww, int stride, size_t frame_bytes) {
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    int rc = state_init(h, n);
    if (rc) return rc;
    ForensicState& F = *h->forensic;
    if (!h->aux_stream) {
        // LOWEST priority: the signals have the whole call to finish; their workgroups should take the CUs the main
        // stream leaves idle (DetectionOutput runs 64 blocks on 256 CUs, the detector's tail layers and the cascade's
        // R-/O-Net are small, four waits on the host) instead of competing with its large launches
        int least = 0, greatest = 0;
        DFD_HIP_TRY(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
        DFD_HIP_TRY(h, hipStreamCreateWithPriority(&h->aux_stream, hipStreamNonBlocking, least));
        DFD_HIP_TRY(h, hipEventCreateWithFlags(&h->aux_go, hipEventDisableTiming));
        DFD_HIP_TRY(h, hipEventCreateWithFlags(&h->aux_done, hipEventDisableTiming));
    }
    const size_t per = FORENSIC_STATS + 128, need = (size_t)n * per * 8;
    if (need > F.host_res_cap) {
        if (F.host_res) DFD_HIP_TRY(h, hipHostFree(F.host_res));
        F.host_res = nullptr;
        F.host_res_cap = 0;
        DFD_HIP_TRY(h, hipHostMalloc((void**)&F.host_res, need, hipHostMallocDefault));
        F.host_res_cap = need;
    }
    // the frames are complete where the main stream stands now (an upload it waited for, a decode it ran)
    DFD_HIP_TRY(h, hipEventRecord(h->aux_go, h->stream));
    DFD_HIP_TRY(h, hipStreamWaitEvent(h->aux_stream, h->aux_go, 0));
    launch_resize_bgr(frames_dev, n, hh, ww, stride, frame_bytes, F.buf.rs, 256, 256, h->aux_stream);
    launch_forensics(F.buf, n, true, h->color, F.twiddle, h->aux_stream);
    copy_kernel_async(F.host_res, F.buf.stats, (size_t)n * FORENSIC_STATS * 8, h->aux_stream);
    copy_kernel_async(F.host_res + (size_t)n * FORENSIC_STATS, F.buf.stats_noise, (size_t)n * 64 * 8, h->aux_stream);
    copy_kernel_async(F.host_res + (size_t)n * (FORENSIC_STATS + 64), F.buf.stats_ela, (size_t)n * 64 * 8, h->aux_stream);
    DFD_HIP_TRY(h, hipGetLastError());
    DFD_HIP_TRY(h, hipEventRecord(h->aux_done, h->aux_stream));
    return DFD_OK;
}

int forensics_batch_end(dfd_handle* h, int n, double* prob_out, double* scores_out) {
    ForensicState& F = *h->forensic;
    DFD_HIP_TRY(h, hipEventSynchronize(h->aux_done));
    const double* st = F.host_res;
    const double* noise = F.host_res + (size_t)n * FORENSIC_STATS;
    const double* ela = F.host_res + (size_t)n * (FORENSIC_STATS + 64);
    const double w[6] = {0.25, 0.20, 0.20, 0.15, 0.10, 0.10};
    for (int f = 0; f < n; ++f) {
        double sc[6], ex[10];
        static_scores(&st[(size_t)f * FORENSIC_STATS], &noise[(size_t)f * 64], &ela[(size_t)f * 64], true, sc, ex);
        double comb = 0.0;
        for (int i = 0; i < 6; ++i) comb += sc[i] * w[i];
        prob_out[f] = clip01(comb);
        if (scores_out)
            for (int i = 0; i < 6; ++i) scores_out[(size_t)f * 6 + i] = sc[i];
    }
    return DFD_OK;
}

}  // namespace dfd

extern "C" {

int dfd_forensics(dfd_handle* h, int stream_id, const uint8_t* bgr, int hh, int ww, int stride, int full,
                  double* scores_out, double* prob_out, double* stats_out) {
    if (!h) return DFD_ERR_ARG;
    if (!bgr || !scores_out || !prob_out || hh <= 0 || ww <= 0 || stride < ww * 3)
        return fail(h, DFD_ERR_ARG, "forensics: bad pointer or geometry");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    const int rc = ensure(h, &h->frame_buf, (size_t)hh * stride);
    if (rc) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(h->frame_buf.p, bgr, (size_t)hh * stride, hipMemcpyHostToDevice, h->stream));
    return forensics_run(h, stream_id, (const uint8_t*)h->frame_buf.p, hh, ww, stride, full, scores_out, prob_out, stats_out);
}

int dfd_forensic_signals_device(dfd_handle* h, const uint8_t* frames_dev, int n, int hh, int ww, const int32_t* prev_index,
                                double* scores5_out, double* mean_diff_out) {
    if (!h) return DFD_ERR_ARG;
    if (!frames_dev || n <= 0 || hh <= 0 || ww <= 0 || !prev_index || !scores5_out || !mean_diff_out)
        return fail(h, DFD_ERR_ARG, "forensic_signals: bad pointer or geometry");
    // prev_index[f] = -2: frame f is only somebody's predecessor - it needs a gray plane, no signals.  Such frames
    // form the tail of the batch (the kernels of the signals run on the leading ns frames).
    int ns = n;
    while (ns > 0 && prev_index[ns - 1] == -2) --ns;
    for (int f = 0; f < n; ++f) {
        if (prev_index[f] >= n) return fail(h, DFD_ERR_ARG, "forensic_signals: prev_index[%d] = %d outside the batch", f, prev_index[f]);
        if (prev_index[f] < -2 || (prev_index[f] == -2 && f < ns))
            return fail(h, DFD_ERR_ARG, "forensic_signals: predecessor-only frames (-2) must be the tail of the batch");
    }
    if (ns == 0) return fail(h, DFD_ERR_ARG, "forensic_signals: every frame of the batch is predecessor-only (-2): nothing to compute");
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    int rc = state_init(h, n);
    if (rc) return rc;
    ForensicState& F = *h->forensic;
    if ((rc = ensure(h, &F.pair_idx, (size_t)n * 4))) return rc;
    if ((rc = ensure(h, &F.pair_part, (size_t)n * 256 * 8))) return rc;
    const int stride = ww * 3;
    if ((rc = mailbox_h2d(h, F.pair_idx.p, prev_index, (size_t)n * 4))) return rc;
    launch_resize_bgr(frames_dev, n, hh, ww, stride, (size_t)hh * stride, F.buf.rs, 256, 256, h->stream);
    launch_forensics(F.buf, ns, true, h->color, F.twiddle, h->stream, n - ns);
    if (ns > 0) launch_absdiff_pairs(F.buf.gray, (const int*)F.pair_idx.p, (double*)F.pair_part.p, ns, h->stream);
    const size_t nz = ns > 0 ? ns : 1;
    const double* st = (const double*)mailbox_d2h(h, F.buf.stats, nz * FORENSIC_STATS * 8);
    const double* noise = (const double*)mailbox_d2h(h, F.buf.stats_noise, nz * 64 * 8);
    const double* ela = (const double*)mailbox_d2h(h, F.buf.stats_ela, nz * 64 * 8);
    const double* part = (const double*)mailbox_d2h(h, F.pair_part.p, nz * 256 * 8);
    if (!st || !noise || !ela || !part) return fail(h, DFD_ERR_HIP, "forensics: mailbox allocation failed");
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());
    for (int f = ns; f < n; ++f) {                           // predecessor-only frames: no signals
        for (int i = 0; i < 5; ++i) scores5_out[(size_t)f * 5 + i] = -1.0;
        mean_diff_out[f] = -1.0;
    }
    for (int f = 0; f < ns; ++f) {
        double sc[6], ex[10];
        static_scores(&st[(size_t)f * FORENSIC_STATS], &noise[(size_t)f * 64], &ela[(size_t)f * 64], true, sc, ex);
        for (int i = 0; i < 5; ++i) scores5_out[(size_t)f * 5 + i] = sc[i];
        if (prev_index[f] < 0) {
            mean_diff_out[f] = -1.0;
        } else {
            double sum = 0;                                      // the summation order of forensics_run
            for (int i = 0; i < 256; ++i) sum += part[(size_t)f * 256 + i];
            mean_diff_out[f] = sum / 65536.0;
        }
    }
    return DFD_OK;
}

int dfd_forensic_tap(dfd_handle* h, const uint8_t* bgr256, int n, int full, const char* start, const void* start_data,
                     const char* name, int frame, void* out, size_t capacity, size_t* bytes) {
    if (!h) return DFD_ERR_ARG;
    if (!start || !name || !out || !bytes || n <= 0 || n > 64 || frame < -1 || frame >= n)
        return fail(h, DFD_ERR_ARG, "forensic_tap: bad pointer, frame index or frame count (1..64)");
    constexpr size_t PIX = 65536;
    static const char* const starts[4] = {"rs", "gray", "grad", "map"};
    int st = -1;
    for (int i = 0; i < 4; ++i)
        if (!std::strcmp(start, starts[i])) st = i;
    if (st < 0) return fail(h, DFD_ERR_ARG, "forensic_tap: start '%s' is none of rs, gray, grad, map", start);
    if (st == FROM_RS ? !bgr256 : !start_data) return fail(h, DFD_ERR_ARG, "forensic_tap: no data for start '%s'", start);
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    int rc = state_init(h, n);
    if (rc) return rc;
    ForensicState& F = *h->forensic;
    if ((rc = ensure(h, &F.tap_store, (size_t)n * PIX * (sizeof(float2) + sizeof(float) + 1)))) return rc;
    ForensicTaps T;
    T.spectrum = static_cast<float2*>(F.tap_store.p);
    T.logmag = reinterpret_cast<float*>(T.spectrum + (size_t)n * PIX);
    T.edges = reinterpret_cast<uint8_t*>(T.logmag + (size_t)n * PIX);
    const ForensicBuffers& B = F.buf;
    // which buffer, bytes per frame, the last start that still computes it, and whether only full mode does
    struct Tap { const char* name; const void* p; size_t per; int last_start; bool full_only; };
    const bool stats_full = full && st == FROM_RS;
    const Tap taps[] = {
        {"rs", B.rs, PIX * 3, FROM_RS, false}, {"gray", B.gray, PIX, FROM_GRAY, false},
        {"fft_tmp", B.fft_tmp, PIX * sizeof(float2), FROM_GRAY, false}, {"spectrum", T.spectrum, PIX * sizeof(float2), FROM_GRAY, false},
        {"logmag", T.logmag, PIX * sizeof(float), FROM_GRAY, false}, {"fft_part", B.fft_part, 256 * 7 * 8, FROM_GRAY, false},
        {"grad", B.grad, PIX * sizeof(short2), FROM_GRAD, false}, {"lap_part", B.lap_part, 256 * 2 * 8, FROM_GRAY, false},
        {"map", B.map, PIX, FROM_MAP, false}, {"edges", T.edges, PIX, FROM_MAP, false}, {"edge_count", B.edge_count, 8, FROM_MAP, false},
        {"jy", B.jy, PIX, FROM_RS, true}, {"jcb", B.jcb, PIX / 4, FROM_RS, true}, {"jcr", B.jcr, PIX / 4, FROM_RS, true},
        {"stats_ela", B.stats_ela, 64 * 8, FROM_RS, true}, {"stats_noise", B.stats_noise, 64 * 8, FROM_GRAY, true},
        {"hsv_part", B.hsv_part, 256 * 4 * 8, FROM_RS, true}, {"hue_bits", B.hue_bits, 6 * 4, FROM_RS, true},
        {"stats", B.stats, (size_t)(stats_full ? FORENSIC_STATS : ST_SAT_STD) * 8, FROM_GRAY, false},
    };
    const char* src = nullptr;
    size_t per = 0, stride = 0;
    if (!std::strcmp(name, "twiddle")) {                        // the table every FFT launch reads; not per frame
        src = reinterpret_cast<const char*>(F.twiddle);
        per = 128 * sizeof(float2);
        frame = 0;
    }
    for (const Tap& t : taps)
        if (!src && !std::strcmp(name, t.name)) {
            if (st > t.last_start || (t.full_only && !full))
                return fail(h, DFD_ERR_ARG, "forensic_tap: '%s' is not computed from start '%s' with full = %d", name, start, full);
            src = static_cast<const char*>(t.p);
            per = t.per;
            stride = !std::strcmp(name, "stats") ? FORENSIC_STATS * 8 : t.per;
        }
    if (!src) return fail(h, DFD_ERR_ARG, "forensic_tap: no buffer named '%s'", name);
    const size_t nout = frame < 0 ? (size_t)n : 1, total = nout * per;
    *bytes = total;
    if (total > capacity) return fail(h, DFD_ERR_ARG, "forensic_tap '%s' needs %zu bytes, capacity %zu", name, total, capacity);
    if (st == FROM_RS) {
        DFD_HIP_TRY(h, hipMemcpyAsync(B.rs, bgr256, (size_t)n * PIX * 3, hipMemcpyHostToDevice, h->stream));
    } else {
        void* dst = st == FROM_GRAY ? (void*)B.gray : st == FROM_GRAD ? (void*)B.grad : (void*)B.map;
        DFD_HIP_TRY(h, hipMemcpyAsync(dst, start_data, (size_t)n * PIX * (st == FROM_GRAD ? sizeof(short2) : 1), hipMemcpyHostToDevice, h->stream));
    }
    launch_forensics(B, n, full != 0, h->color, F.twiddle, h->stream, 0, (ForensicStart)st, &T);
    DFD_HIP_TRY(h, hipGetLastError());
    const size_t first = frame < 0 ? 0 : (size_t)frame;
    if (stride == per || nout == 1) {
        DFD_HIP_TRY(h, hipMemcpyAsync(out, src + first * stride, total, hipMemcpyDeviceToHost, h->stream));
    } else {
        for (size_t f = 0; f < nout; ++f)
            DFD_HIP_TRY(h, hipMemcpyAsync((char*)out + f * per, src + f * stride, per, hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

int dfd_forensics_reset(dfd_handle* h, int stream_id) {
    if (!h) return DFD_ERR_ARG;
    if (!h->forensic) return DFD_OK;
    auto it = h->forensic->streams.find(stream_id);
    if (it == h->forensic->streams.end()) return DFD_OK;
    it->second.has_prev = false;                 // frame_analysis.py:391-395
    it->second.diffs.clear();
    it->second.frame_count = 0;
    return DFD_OK;
}

int dfd_forensics_release(dfd_handle* h, int stream_id) {
    if (!h) return DFD_ERR_ARG;
    if (!h->forensic) return DFD_OK;
    ForensicState& F = *h->forensic;
    auto it = F.streams.find(stream_id);
    if (it == F.streams.end()) return DFD_OK;
    if (it->second.prev_gray) F.free_planes[it->second.size].push_back(it->second.prev_gray);   // every call that used it has synchronised
    F.streams.erase(it);
    return DFD_OK;
}

int dfd_forensics_state(dfd_handle* h, int stream_id, int* frame_count, int* n_diffs, int* has_prev) {
    if (!h) return DFD_ERR_ARG;
    int fc = 0, nd = 0, hp = 0;
    if (h->forensic) {
        auto it = h->forensic->streams.find(stream_id);
        if (it != h->forensic->streams.end()) {
            fc = it->second.frame_count;
            nd = (int)it->second.diffs.size();
            hp = it->second.has_prev ? 1 : 0;
        }
    }
    if (frame_count) *frame_count = fc;
    if (n_diffs) *n_diffs = nd;
    if (has_prev) *has_prev = hp;
    return DFD_OK;
}

// ---- any square analysis size (forensic_sized_kernels.hip): the same host half, S in place of 256
}  // extern "C"

namespace dfd {

// the analyzer at analysis edge `size` on a frame that is already in HBM (shared by dfd_forensics_sized and the fused
// single-frame entries on a stream of the general chain)
int forensics_sized_run(dfd_handle* h, int stream_id, const uint8_t* frame_dev, int hh, int ww, int stride, int size, int full,
                        double* scores_out, double* prob_out, double* stats_out) {
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    int rc = stream_size_check(h, stream_id, size);
    if (rc) return rc;
    if ((rc = state_init(h, 1))) return rc;
    ForensicState& F = *h->forensic;
    ForensicState::Sized* Z = nullptr;
    if ((rc = sized_init(h, size, 1, &Z))) return rc;
    ForensicStream& S = F.streams[stream_id];
    if ((rc = stream_plane(h, S, size))) return rc;
    const size_t pix = (size_t)size * size;
    const int nblk = sized_blocks(size);
    const ForensicBuffers& B = Z->buf;

    launch_resize_bgr(frame_dev, 1, hh, ww, stride, 0, B.rs, size, size, h->stream);
    DFD_HIP_TRY(h, launch_forensics_sized(B, size, 1, full != 0, h->color, Z->table, h->stream));
    if (S.has_prev) launch_absdiff_sized(B.gray, (const uint8_t*)S.prev_gray, Z->diff_part, size, h->stream);
    double st[FORENSIC_STATS];
    std::vector<double> blk((size_t)2 * nblk + size);
    double *noise = blk.data(), *ela = noise + nblk, *dpart = ela + nblk;
    DFD_HIP_TRY(h, hipMemcpyAsync(st, B.stats, sizeof st, hipMemcpyDeviceToHost, h->stream));
    if (full) {
        DFD_HIP_TRY(h, hipMemcpyAsync(noise, B.stats_noise, (size_t)nblk * 8, hipMemcpyDeviceToHost, h->stream));
        DFD_HIP_TRY(h, hipMemcpyAsync(ela, B.stats_ela, (size_t)nblk * 8, hipMemcpyDeviceToHost, h->stream));
    }
    if (S.has_prev) DFD_HIP_TRY(h, hipMemcpyAsync(dpart, Z->diff_part, (size_t)size * 8, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(S.prev_gray, B.gray, pix, hipMemcpyDeviceToDevice, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());

    const double nan = std::nan("");
    double sc[6], ex[10], mean_diff, temporal_cv;
    *prob_out = score_frame(S, st, noise, ela, full != 0, dpart, sc, ex, &mean_diff, &temporal_cv, size, (double)pix, nblk, true);
    for (int i = 0; i < 6; ++i) scores_out[i] = sc[i];
    if (stats_out) {
        const double out[DFD_FORENSIC_NSTATS] = {ex[0], ex[1], ex[2], ex[3], ex[4], ex[5], ex[6], ex[7], ex[8], ex[9],
                                                 st[ST_EDGE_COUNT] / (double)pix, st[ST_LAP_VAR], full ? st[ST_SAT_STD] : nan,
                                                 full ? st[ST_VAL_STD] : nan, full ? st[ST_HUES] : nan, mean_diff, temporal_cv,
                                                 (double)S.frame_count};
        for (int i = 0; i < DFD_FORENSIC_NSTATS; ++i) stats_out[i] = out[i];
    }
    return DFD_OK;
}

// the fused single-frame entries: the stream at the size and on the chain it holds
int forensics_stream_run(dfd_handle* h, int stream_id, const uint8_t* frame_dev, int hh, int ww, int stride, int full,
                         double* scores_out, double* prob_out) {
    if (h->forensic) {
        auto it = h->forensic->streams.find(stream_id);
        if (it != h->forensic->streams.end() && on_general_chain(it->second))
            return forensics_sized_run(h, stream_id, frame_dev, hh, ww, stride, it->second.size, full, scores_out, prob_out, nullptr);
    }
    return forensics_run(h, stream_id, frame_dev, hh, ww, stride, full, scores_out, prob_out, nullptr);
}

}  // namespace dfd

extern "C" {

int dfd_forensics_sized(dfd_handle* h, int stream_id, const uint8_t* bgr, int hh, int ww, int stride, int size, int full,
                        double* scores_out, double* prob_out, double* stats_out) {
    if (!h) return DFD_ERR_ARG;
    if (!bgr || !scores_out || !prob_out || hh <= 0 || ww <= 0 || stride < ww * 3)
        return fail(h, DFD_ERR_ARG, "forensics_sized: bad pointer or geometry");
    if (!sized_ok(size))
        return fail(h, DFD_ERR_ARG, "forensics_sized: analysis size %d is not a multiple of 16 in %d..%d", size, SIZED_MIN, SIZED_MAX);
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    int rc = stream_size_check(h, stream_id, size);
    if (rc) return rc;
    if ((rc = ensure(h, &h->frame_buf, (size_t)hh * stride))) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(h->frame_buf.p, bgr, (size_t)hh * stride, hipMemcpyHostToDevice, h->stream));
    return forensics_sized_run(h, stream_id, (const uint8_t*)h->frame_buf.p, hh, ww, stride, size, full, scores_out, prob_out, stats_out);
}

int dfd_forensics_open(dfd_handle* h, int stream_id, int size) {
    if (!h) return DFD_ERR_ARG;
    if (!sized_ok(size))
        return fail(h, DFD_ERR_ARG, "forensics_open: analysis size %d is not a multiple of 16 in %d..%d", size, SIZED_MIN, SIZED_MAX);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    int rc = stream_size_check(h, stream_id, size);                  // another size already: refused, nothing changes
    if (rc) return rc;
    if ((rc = state_init(h, 1))) return rc;
    ForensicStream& S = h->forensic->streams[stream_id];
    if (S.size) return DFD_OK;                                       // the same size: as it is
    S.size = size;
    S.general = true;
    return DFD_OK;
}

int dfd_forensic_tap_sized(dfd_handle* h, const uint8_t* frames, int n, int size, int full, const char* start, const void* start_data,
                           const char* name, int frame, void* out, size_t capacity, size_t* bytes) {
    if (!h) return DFD_ERR_ARG;
    if (!start || !name || !out || !bytes || n <= 0 || n > 16 || frame < -1 || frame >= n)
        return fail(h, DFD_ERR_ARG, "forensic_tap_sized: bad pointer, frame index or frame count (1..16)");
    if (!sized_ok(size))
        return fail(h, DFD_ERR_ARG, "forensic_tap_sized: analysis size %d is not a multiple of 16 in %d..%d", size, SIZED_MIN, SIZED_MAX);
    const size_t PIX = (size_t)size * size, NB = (size_t)sized_blocks(size), SS = (size_t)size;
    static const char* const starts[4] = {"rs", "gray", "grad", "map"};
    int st = -1;
    for (int i = 0; i < 4; ++i)
        if (!std::strcmp(start, starts[i])) st = i;
    if (st < 0) return fail(h, DFD_ERR_ARG, "forensic_tap_sized: start '%s' is none of rs, gray, grad, map", start);
    if (st == FROM_RS ? !frames : !start_data) return fail(h, DFD_ERR_ARG, "forensic_tap_sized: no data for start '%s'", start);
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    int rc = state_init(h, 1);
    if (rc) return rc;
    ForensicState::Sized* Z = nullptr;
    if ((rc = sized_init(h, size, n, &Z))) return rc;
    if ((rc = ensure(h, &Z->tap_store, (size_t)n * PIX * (sizeof(float2) + sizeof(float) + 1)))) return rc;
    ForensicTaps T;
    T.spectrum = static_cast<float2*>(Z->tap_store.p);
    T.logmag = reinterpret_cast<float*>(T.spectrum + (size_t)n * PIX);
    T.edges = reinterpret_cast<uint8_t*>(T.logmag + (size_t)n * PIX);
    const ForensicBuffers& B = Z->buf;
    struct Tap { const char* name; const void* p; size_t per; int last_start; bool full_only; };
    const bool stats_full = full && st == FROM_RS;
    const Tap taps[] = {
        {"rs", B.rs, PIX * 3, FROM_RS, false}, {"gray", B.gray, PIX, FROM_GRAY, false},
        {"fft_tmp", B.fft_tmp, PIX * sizeof(float2), FROM_GRAY, false}, {"spectrum", T.spectrum, PIX * sizeof(float2), FROM_GRAY, false},
        {"logmag", T.logmag, PIX * sizeof(float), FROM_GRAY, false}, {"fft_part", B.fft_part, SS * 7 * 8, FROM_GRAY, false},
        {"grad", B.grad, PIX * sizeof(short2), FROM_GRAD, false}, {"lap_part", B.lap_part, SS * 2 * 8, FROM_GRAY, false},
        {"map", B.map, PIX, FROM_MAP, false}, {"edges", T.edges, PIX, FROM_MAP, false}, {"edge_count", B.edge_count, 8, FROM_MAP, false},
        {"jy", B.jy, PIX, FROM_RS, true}, {"jcb", B.jcb, PIX / 4, FROM_RS, true}, {"jcr", B.jcr, PIX / 4, FROM_RS, true},
        {"stats_ela", B.stats_ela, NB * 8, FROM_RS, true}, {"stats_noise", B.stats_noise, NB * 8, FROM_GRAY, true},
        {"hsv_part", B.hsv_part, SS * 4 * 8, FROM_RS, true}, {"hue_bits", B.hue_bits, 6 * 4, FROM_RS, true},
        {"stats", B.stats, (size_t)(stats_full ? FORENSIC_STATS : ST_SAT_STD) * 8, FROM_GRAY, false},
    };
    const char* src = nullptr;
    size_t per = 0, stride = 0;
    if (!std::strcmp(name, "twiddle")) {                        // the table both DFT launches read; not per frame
        src = reinterpret_cast<const char*>(Z->table);
        per = SS * sizeof(float2);
        frame = 0;
    }
    for (const Tap& t : taps)
        if (!src && !std::strcmp(name, t.name)) {
            if (st > t.last_start || (t.full_only && !full))
                return fail(h, DFD_ERR_ARG, "forensic_tap_sized: '%s' is not computed from start '%s' with full = %d", name, start, full);
            src = static_cast<const char*>(t.p);
            per = t.per;
            stride = !std::strcmp(name, "stats") ? FORENSIC_STATS * 8 : t.per;
        }
    if (!src) return fail(h, DFD_ERR_ARG, "forensic_tap_sized: no buffer named '%s'", name);
    const size_t nout = frame < 0 ? (size_t)n : 1, total = nout * per;
    *bytes = total;
    if (total > capacity) return fail(h, DFD_ERR_ARG, "forensic_tap_sized '%s' needs %zu bytes, capacity %zu", name, total, capacity);
    if (st == FROM_RS) {
        DFD_HIP_TRY(h, hipMemcpyAsync(B.rs, frames, (size_t)n * PIX * 3, hipMemcpyHostToDevice, h->stream));
    } else {
        void* dst = st == FROM_GRAY ? (void*)B.gray : st == FROM_GRAD ? (void*)B.grad : (void*)B.map;
        DFD_HIP_TRY(h, hipMemcpyAsync(dst, start_data, (size_t)n * PIX * (st == FROM_GRAD ? sizeof(short2) : 1), hipMemcpyHostToDevice, h->stream));
    }
    DFD_HIP_TRY(h, launch_forensics_sized(B, size, n, full != 0, h->color, Z->table, h->stream, (ForensicStart)st, &T));
    const size_t first = frame < 0 ? 0 : (size_t)frame;
    if (stride == per || nout == 1) {
        DFD_HIP_TRY(h, hipMemcpyAsync(out, src + first * stride, total, hipMemcpyDeviceToHost, h->stream));
    } else {
        for (size_t f = 0; f < nout; ++f)
            DFD_HIP_TRY(h, hipMemcpyAsync((char*)out + f * per, src + f * stride, per, hipMemcpyDeviceToHost, h->stream));
    }
    DFD_HIP_TRY(h, stream_sync(h));
    return DFD_OK;
}

}  // extern "C"
