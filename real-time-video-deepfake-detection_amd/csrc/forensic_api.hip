// C ABI of the forensic analyzer: device statistics -> the reference's threshold scoring (forensic_score.h; reference
// frame_analysis.py:58-389), with the per-stream temporal state kept here.  The 256x256 chain and the general chain at
// any edge S are two instantiations of one set of kernels (forensic_kernels.hip) behind ONE host path: a ForensicChain
// holds the geometry, work memory and table of one of them.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "dfd_common.h"
#include "forensic_kernels.h"

using namespace dfd;

namespace dfd {

struct ForensicStream : ForensicTemporal {
    void* prev_gray = nullptr;     // size * size bytes on the device
    int size = 0;                  // analysis edge, fixed by dfd_forensics_open or the stream's first frame (0: neither yet)
    bool general = false;          // opened (dfd_forensics_open): the fused entries run it on the general chain, at 256 too
};

// one chain's device resources: the 256x256 chain (G.general = false) or the general chain at one analysis edge
struct ForensicChain {
    ForensicGeometry G;
    DevBuf work, tap_store;        // work: carved into `buf` for `cap` frames; tap_store: spectrum, logmag, edges of the test tap
    int cap = 0;
    ForensicBuffers buf{};
    float2* table = nullptr;       // exp(-2 pi i j / S): S entries on the general chain, the first S / 2 on the 256x256 chain
    double* diff_part = nullptr;   // G.npart partial sums of the single-frame difference
};

constexpr int FIXED_EDGE = 256;

struct ForensicState {
    std::map<int, ForensicStream> streams;
    // keyed by (general, S): the 256x256 chain and a general chain at 256 differ in spectrum, table length and f32_means
    std::map<std::pair<bool, int>, ForensicChain> chains;
    DevBuf pair_idx, pair_part;    // dfd_forensic_signals_device: predecessor indices, [n][256] partial sums
    double* host_res = nullptr;    // pinned: statistics of a batch that ran on the second stream (forensics_batch_begin)
    size_t host_res_cap = 0;
    DevBuf frame_desc, diff_tab, copy_tab;   // forensics_streams_run: FrameDesc and DiffRow per frame, PlaneCopy per stream
    DevBuf stream_part;                      // ... every frame's per-row partial sums of the difference
    DevBuf sized_gray;                       // ... the gray planes of its frames on the general chain, kept for the whole call
                                             // (a predecessor may sit in an earlier chunk)
    std::map<int, std::vector<void*>> free_planes;   // stored planes of released streams by analysis edge, reused by the
                                                     // next new stream of that edge
};

void forensic_destroy(dfd_handle* h) {
    if (h->forensic && h->forensic->host_res) hipHostFree(h->forensic->host_res);
    delete h->forensic;
    h->forensic = nullptr;
}

}  // namespace dfd

namespace {

// the table's length is what differs between the two chains on the host: the FFT reads half of it
size_t chain_table_entries(const ForensicGeometry& G) { return (size_t)(G.general ? G.S : G.S / 2); }

// B: the chain's own buffers, or a copy with some of them elsewhere (forensics_streams_run)
hipError_t chain_launch(const ForensicChain& C, const ForensicBuffers& B, int n, bool full, const ColorTables& T, hipStream_t s,
                        int gray_only = 0, ForensicStart start = FROM_RS, const ForensicTaps* taps = nullptr) {
    return launch_forensics(B, C.G.general, C.G.S, n, full, T, C.table, s, gray_only, start, taps);
}

// the chain (general, S) with work memory for `frames` frames; creates the handle's forensic state and the chain's table
// on first use
int chain_reserve(dfd_handle* h, bool general, int S, int frames, ForensicChain** out) {
    if (!h->forensic) h->forensic = new ForensicState();
    ForensicChain& C = h->forensic->chains[{general, S}];
    if (!C.table) {
        C.G.S = S;
        C.G.npix = (double)S * (double)S;
        C.G.nblk = edge_blocks(S);
        C.G.npart = S;
        C.G.f32_means = C.G.general = general;
        std::vector<float2> tw(S);
        forensic_table(S, tw.data());
        const size_t bytes = chain_table_entries(C.G) * sizeof(float2);
        void *t = nullptr, *d = nullptr;
        DFD_HIP_TRY(h, hipMalloc(&t, bytes));
        h->owned.push_back(t);
        DFD_HIP_TRY(h, hipMemcpy(t, tw.data(), bytes, hipMemcpyHostToDevice));
        DFD_HIP_TRY(h, hipMalloc(&d, (size_t)C.G.npart * 8));
        h->owned.push_back(d);
        C.diff_part = static_cast<double*>(d);
        C.table = static_cast<float2*>(t);
    }
    if (frames > C.cap) {
        const int rc = ensure(h, &C.work, forensic_bytes_per_frame(S) * frames + 65536);
        if (rc) return rc;
        forensic_carve(C.work.p, S, frames, &C.buf);
        C.cap = frames;
    }
    *out = &C;
    return DFD_OK;
}

// the stream's stored gray plane: a released stream's plane when there is one (no hipMalloc on the serving path)
int stream_plane(dfd_handle* h, ForensicStream& S, int size) {
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

// the analyzer on a frame that is already in HBM, on the chain (general, size): shared by dfd_forensics,
// dfd_forensics_sized and the fused single-frame entries
int forensics_chain_run(dfd_handle* h, int stream_id, bool general, int size, const uint8_t* frame_dev, int hh, int ww, int stride,
                        int full, double* scores_out, double* prob_out, double* stats_out) {
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    int rc = stream_size_check(h, stream_id, size);
    if (rc) return rc;
    ForensicChain* C = nullptr;
    if ((rc = chain_reserve(h, general, size, 1, &C))) return rc;
    const ForensicGeometry& G = C->G;
    const ForensicBuffers& B = C->buf;
    ForensicStream& S = h->forensic->streams[stream_id];
    if ((rc = stream_plane(h, S, size))) return rc;

    launch_resize_bgr(frame_dev, 1, hh, ww, stride, 0, B.rs, size, size, h->stream);
    DFD_HIP_TRY(h, chain_launch(*C, B, 1, full != 0, h->color, h->stream));
    if (S.has_prev) launch_absdiff(B.gray, (const uint8_t*)S.prev_gray, C->diff_part, size, h->stream);
    double st[FORENSIC_STATS];
    std::vector<double> blk((size_t)2 * G.nblk + G.npart);
    double *noise = blk.data(), *ela = noise + G.nblk, *dpart = ela + G.nblk;
    DFD_HIP_TRY(h, hipMemcpyAsync(st, B.stats, sizeof st, hipMemcpyDeviceToHost, h->stream));
    if (full) {
        DFD_HIP_TRY(h, hipMemcpyAsync(noise, B.stats_noise, (size_t)G.nblk * 8, hipMemcpyDeviceToHost, h->stream));
        DFD_HIP_TRY(h, hipMemcpyAsync(ela, B.stats_ela, (size_t)G.nblk * 8, hipMemcpyDeviceToHost, h->stream));
    }
    if (S.has_prev) DFD_HIP_TRY(h, hipMemcpyAsync(dpart, C->diff_part, (size_t)G.npart * 8, hipMemcpyDeviceToHost, h->stream));
    DFD_HIP_TRY(h, hipMemcpyAsync(S.prev_gray, B.gray, (size_t)size * size, hipMemcpyDeviceToDevice, h->stream));
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());

    const double nan = std::nan("");
    double sc[6], ex[10], mean_diff, temporal_cv;
    *prob_out = score_frame(S, G, st, noise, ela, full != 0, dpart, sc, ex, &mean_diff, &temporal_cv);
    for (int i = 0; i < 6; ++i) scores_out[i] = sc[i];
    if (stats_out) {
        const double out[DFD_FORENSIC_NSTATS] = {ex[0], ex[1], ex[2], ex[3], ex[4], ex[5], ex[6], ex[7], ex[8], ex[9],
                                                 st[ST_EDGE_COUNT] / G.npix, st[ST_LAP_VAR], full ? st[ST_SAT_STD] : nan,
                                                 full ? st[ST_VAL_STD] : nan, full ? st[ST_HUES] : nan, mean_diff, temporal_cv,
                                                 (double)S.frame_count};
        for (int i = 0; i < DFD_FORENSIC_NSTATS; ++i) stats_out[i] = out[i];
    }
    return DFD_OK;
}

// the test taps (dfd_forensic_tap, dfd_forensic_tap_sized) after their own argument checks; who: the entry's message prefix
int forensic_tap_run(dfd_handle* h, const char* who, bool general, int size, const uint8_t* frames, int n, int full, const char* start,
                     const void* start_data, const char* name, int frame, void* out, size_t capacity, size_t* bytes) {
    static const char* const starts[4] = {"rs", "gray", "grad", "map"};
    int st = -1;
    for (int i = 0; i < 4; ++i)
        if (!std::strcmp(start, starts[i])) st = i;
    if (st < 0) return fail(h, DFD_ERR_ARG, "%s: start '%s' is none of rs, gray, grad, map", who, start);
    if (st == FROM_RS ? !frames : !start_data) return fail(h, DFD_ERR_ARG, "%s: no data for start '%s'", who, start);
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    ForensicChain* C = nullptr;
    int rc = chain_reserve(h, general, size, n, &C);
    if (rc) return rc;
    const size_t PIX = (size_t)size * size, NB = (size_t)C->G.nblk, SS = (size_t)size;
    if ((rc = ensure(h, &C->tap_store, (size_t)n * PIX * (sizeof(float2) + sizeof(float) + 1)))) return rc;
    ForensicTaps T;
    T.spectrum = static_cast<float2*>(C->tap_store.p);
    T.logmag = reinterpret_cast<float*>(T.spectrum + (size_t)n * PIX);
    T.edges = reinterpret_cast<uint8_t*>(T.logmag + (size_t)n * PIX);
    const ForensicBuffers& B = C->buf;
    // which buffer, bytes per frame, the last start that still computes it, and whether only full mode does
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
    if (!std::strcmp(name, "twiddle")) {                        // the table every spectrum launch reads; not per frame
        src = reinterpret_cast<const char*>(C->table);
        per = chain_table_entries(C->G) * sizeof(float2);
        frame = 0;
    }
    for (const Tap& t : taps)
        if (!src && !std::strcmp(name, t.name)) {
            if (st > t.last_start || (t.full_only && !full))
                return fail(h, DFD_ERR_ARG, "%s: '%s' is not computed from start '%s' with full = %d", who, name, start, full);
            src = static_cast<const char*>(t.p);
            per = t.per;
            stride = !std::strcmp(name, "stats") ? FORENSIC_STATS * 8 : t.per;
        }
    if (!src) return fail(h, DFD_ERR_ARG, "%s: no buffer named '%s'", who, name);
    const size_t nout = frame < 0 ? (size_t)n : 1, total = nout * per;
    *bytes = total;
    if (total > capacity) return fail(h, DFD_ERR_ARG, "%s '%s' needs %zu bytes, capacity %zu", who, name, total, capacity);
    if (st == FROM_RS) {
        DFD_HIP_TRY(h, hipMemcpyAsync(B.rs, frames, (size_t)n * PIX * 3, hipMemcpyHostToDevice, h->stream));
    } else {
        void* dst = st == FROM_GRAY ? (void*)B.gray : st == FROM_GRAD ? (void*)B.grad : (void*)B.map;
        DFD_HIP_TRY(h, hipMemcpyAsync(dst, start_data, (size_t)n * PIX * (st == FROM_GRAD ? sizeof(short2) : 1), hipMemcpyHostToDevice, h->stream));
    }
    DFD_HIP_TRY(h, chain_launch(*C, B, n, full != 0, h->color, h->stream, 0, (ForensicStart)st, &T));
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

}  // namespace

namespace dfd {

// the fused single-frame entries: the stream at the size and on the chain it holds
int forensics_stream_run(dfd_handle* h, int stream_id, const uint8_t* frame_dev, int hh, int ww, int stride, int full,
                         double* scores_out, double* prob_out) {
    bool general = false;
    int size = FIXED_EDGE;
    if (h->forensic) {
        auto it = h->forensic->streams.find(stream_id);
        if (it != h->forensic->streams.end() && on_general_chain(it->second)) {
            general = true;
            size = it->second.size;
        }
    }
    return forensics_chain_run(h, stream_id, general, size, frame_dev, hh, ww, stride, full, scores_out, prob_out, nullptr);
}

// n frames of any streams and sizes in one pass (POST /analyze_batch, the session pool).  The frames are grouped by the
// chain and analysis edge of their stream: the frames of 256x256 streams nobody opened run on the 256x256 chain as one
// launch set, the frames of every other edge S on the general chain - one ragged resize to S x S and one launch set per
// chunk of the group, a chunk being as many frames as fit the handle's work-memory budget (forensic_chunk_bytes; the
// kernels treat every frame on its own, so the split changes no result).  The gray planes of the general chain are kept
// for the whole call outside the chunk memory, so that ONE launch differences every frame, whatever its chain, edge and
// chunk, against its predecessor - the previous frame of its stream in this call, else the stream's stored plane - and
// ONE launch writes every stream's last gray plane back to its stored slot.  Then the host half is replayed frame by
// frame in call order: every stream's temporal deque, frame counter and stored plane end exactly where single calls in
// order would leave them.  No stream's state moves before the wait.
int forensics_streams_run(dfd_handle* h, const uint8_t* frames_dev, const FrameDesc* fd, int n, const int* stream_ids,
                          const int* full, double* scores_out, double* prob_out) {
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    int rc = DFD_OK;
    if (!h->forensic) h->forensic = new ForensicState();
    ForensicState& F = *h->forensic;
    std::vector<int> plain;                                          // frames on the 256x256 chain, in call order
    std::map<int, std::vector<int>> groups;                          // analysis edge -> frames on the general chain
    std::vector<int> edge(n);                                        // every frame's analysis edge
    std::vector<bool> general(n);
    size_t gray_bytes = 0, part_doubles = 0;
    int max_S = 0;
    for (int f = 0; f < n; ++f) {
        ForensicStream& S = F.streams[stream_ids[f]];
        general[f] = on_general_chain(S);
        edge[f] = general[f] ? S.size : FIXED_EDGE;
        if ((rc = stream_plane(h, S, edge[f]))) return rc;
        part_doubles += (size_t)edge[f];
        max_S = std::max(max_S, edge[f]);
        if (!general[f]) { plain.push_back(f); continue; }
        groups[edge[f]].push_back(f);
        gray_bytes += (size_t)edge[f] * edge[f];
    }
    const int n_plain = (int)plain.size();
    ForensicChain* P = nullptr;                                      // the 256x256 group's chain: all of its frames at once
    if (n_plain && (rc = chain_reserve(h, false, FIXED_EDGE, n_plain, &P))) return rc;
    std::vector<const ForensicChain*> chain(n, P);                   // every frame's chain
    if ((rc = ensure(h, &F.sized_gray, gray_bytes))) return rc;
    if ((rc = ensure(h, &F.stream_part, part_doubles * 8))) return rc;
    struct Chunk { int S, first, count; ForensicChain* Z; bool full; };   // first: index into the group's frames
    std::vector<Chunk> chunks;
    for (const auto& g : groups) {
        const int S = g.first, cnt = (int)g.second.size();
        const size_t fit = h->forensic_chunk_bytes / forensic_bytes_per_frame(S);
        const int per = (int)std::min<size_t>(std::max<size_t>(fit, 1), (size_t)cnt);
        ForensicChain* Z = nullptr;
        if ((rc = chain_reserve(h, true, S, per, &Z))) return rc;
        bool any = false;
        for (int f : g.second) {
            any = any || full[f] != 0;
            chain[f] = Z;
        }
        for (int c0 = 0; c0 < cnt; c0 += per) chunks.push_back(Chunk{S, c0, std::min(per, cnt - c0), Z, any});
    }
    // where every frame's gray plane is, and its slot in the descriptor and difference tables (the 256x256 group, then
    // group by group): the 256x256 group's planes in its chain's own buffers, the others in the call's store
    std::vector<const uint8_t*> gray(n);
    std::vector<int> order;
    order.reserve(n);
    for (int j = 0; j < n_plain; ++j) {
        gray[plain[j]] = P->buf.gray + (size_t)j * FIXED_EDGE * FIXED_EDGE;
        order.push_back(plain[j]);
    }
    {
        size_t go = 0;
        for (const auto& g : groups)
            for (int f : g.second) {
                gray[f] = (const uint8_t*)F.sized_gray.p + go;
                go += (size_t)g.first * g.first;
                order.push_back(f);
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
        if (!general[f]) any_full = any_full || full[f] != 0;
    }
    std::vector<FrameDesc> desc;
    std::vector<DiffRow> rows;
    std::vector<size_t> part_at(n, 0);                               // every frame's partial sums in F.stream_part
    size_t po = 0;
    for (int f : order) {
        desc.push_back(fd[f]);
        rows.push_back(DiffRow{gray[f], pred[f], (double*)F.stream_part.p + po, edge[f], 0});
        part_at[f] = po;
        po += (size_t)edge[f];
    }
    std::vector<PlaneCopy> back;
    for (const auto& kv : last)
        back.push_back(PlaneCopy{gray[kv.second], (uint8_t*)F.streams[kv.first].prev_gray, (size_t)edge[kv.second] * edge[kv.second]});
    if ((rc = ensure(h, &F.frame_desc, (size_t)n * sizeof(FrameDesc)))) return rc;
    if ((rc = ensure(h, &F.diff_tab, rows.size() * sizeof(DiffRow)))) return rc;
    if ((rc = ensure(h, &F.copy_tab, back.size() * sizeof(PlaneCopy)))) return rc;
    if ((rc = mailbox_h2d(h, F.frame_desc.p, desc.data(), (size_t)n * sizeof(FrameDesc)))) return rc;
    if ((rc = mailbox_h2d(h, F.diff_tab.p, rows.data(), rows.size() * sizeof(DiffRow)))) return rc;
    if ((rc = mailbox_h2d(h, F.copy_tab.p, back.data(), back.size() * sizeof(PlaneCopy)))) return rc;
    const FrameDesc* desc_dev = (const FrameDesc*)F.frame_desc.p;
    // per frame: where the host finds its statistics once the stream has been waited for.  One launch set's statistics
    // (count frames from `frames`, in the order of its buffers B) through the mailbox; blocks: the block arrays too.
    std::vector<const double*> st(n, nullptr), noise(n, nullptr), ela(n, nullptr);
    auto fetch_stats = [&](const ForensicBuffers& B, const ForensicGeometry& G, const int* frames, int count, bool blocks) {
        const double* a = (const double*)mailbox_d2h(h, B.stats, (size_t)count * FORENSIC_STATS * 8);
        const double* b = blocks ? (const double*)mailbox_d2h(h, B.stats_noise, (size_t)count * G.nblk * 8) : nullptr;
        const double* e = blocks ? (const double*)mailbox_d2h(h, B.stats_ela, (size_t)count * G.nblk * 8) : nullptr;
        if (!a || (blocks && (!b || !e))) return false;
        for (int j = 0; j < count; ++j) {
            const int f = frames[j];
            st[f] = a + (size_t)j * FORENSIC_STATS;
            if (blocks) {
                noise[f] = b + (size_t)j * G.nblk;
                ela[f] = e + (size_t)j * G.nblk;
            }
        }
        return true;
    };
    if (n_plain) {
        launch_resize_bgr_ragged(frames_dev, desc_dev, n_plain, P->buf.rs, P->G.S, P->G.S, h->stream);
        DFD_HIP_TRY(h, chain_launch(*P, P->buf, n_plain, any_full, h->color, h->stream));
        if (!fetch_stats(P->buf, P->G, plain.data(), n_plain, true)) return fail(h, DFD_ERR_HIP, "forensics: mailbox allocation failed");
    }
    int at = n_plain;                                                // the chunk's first slot of the descriptor table
    for (const Chunk& c : chunks) {
        const int* frames = groups[c.S].data() + c.first;
        ForensicBuffers B = c.Z->buf;                                // the chunk's work memory, its gray planes in the call's store
        B.gray = const_cast<uint8_t*>(gray[frames[0]]);
        launch_resize_bgr_ragged(frames_dev, desc_dev + at, c.count, B.rs, c.S, c.S, h->stream);
        DFD_HIP_TRY(h, chain_launch(*c.Z, B, c.count, c.full, h->color, h->stream));
        if (!fetch_stats(B, c.Z->G, frames, c.count, c.full)) return fail(h, DFD_ERR_HIP, "forensics: mailbox allocation failed");
        at += c.count;
    }
    launch_absdiff_prev((const DiffRow*)F.diff_tab.p, n, max_S, h->stream);
    launch_copy_planes((const PlaneCopy*)F.copy_tab.p, (int)back.size(), max_S, h->stream);
    const double* parts = (const double*)mailbox_d2h(h, F.stream_part.p, part_doubles * 8);
    if (!parts) return fail(h, DFD_ERR_HIP, "forensics: mailbox allocation failed");
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());
    for (int f = 0; f < n; ++f) {
        double sc[6], ex[10], md, tcv;
        prob_out[f] = score_frame(F.streams[stream_ids[f]], chain[f]->G, st[f], noise[f], ela[f], full[f] != 0, parts + part_at[f], sc, ex, &md, &tcv);
        for (int i = 0; i < 6; ++i) scores_out[(size_t)f * 6 + i] = sc[i];
    }
    return DFD_OK;
}

// Stateless batch variant for throughput runs: n device frames -> six-signal probability each, the
// temporal signal taking its first-frame value 0 (frame_analysis.py:358-360).  One launch set for all frames.
int forensics_batch_run(dfd_handle* h, const uint8_t* frames_dev, int n, int hh, int ww, int stride, size_t frame_bytes,
                        double* prob_out, double* scores_out) {
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    ForensicChain* C = nullptr;
    int rc = chain_reserve(h, false, FIXED_EDGE, n, &C);
    if (rc) return rc;
    const ForensicGeometry& G = C->G;
    launch_resize_bgr(frames_dev, n, hh, ww, stride, frame_bytes, C->buf.rs, G.S, G.S, h->stream);
    DFD_HIP_TRY(h, chain_launch(*C, C->buf, n, true, h->color, h->stream));
    // a few KB per frame, through the mailbox (dfd_common.h) rather than the DMA engines
    const double* st = (const double*)mailbox_d2h(h, C->buf.stats, (size_t)n * FORENSIC_STATS * 8);
    const double* noise = (const double*)mailbox_d2h(h, C->buf.stats_noise, (size_t)n * G.nblk * 8);
    const double* ela = (const double*)mailbox_d2h(h, C->buf.stats_ela, (size_t)n * G.nblk * 8);
    if (!st || !noise || !ela) return fail(h, DFD_ERR_HIP, "forensics: mailbox allocation failed");
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());
    score_stateless(G, st, noise, ela, n, prob_out, scores_out);
    return DFD_OK;
}

int forensics_batch_begin(dfd_handle* h, const uint8_t* frames_dev, int n, int hh, int ww, int stride, size_t frame_bytes) {
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    ForensicChain* C = nullptr;
    int rc = chain_reserve(h, false, FIXED_EDGE, n, &C);
    if (rc) return rc;
    ForensicState& F = *h->forensic;
    const ForensicGeometry& G = C->G;
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
    const size_t per = FORENSIC_STATS + 2 * (size_t)G.nblk, need = (size_t)n * per * 8;
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
    launch_resize_bgr(frames_dev, n, hh, ww, stride, frame_bytes, C->buf.rs, G.S, G.S, h->aux_stream);
    DFD_HIP_TRY(h, chain_launch(*C, C->buf, n, true, h->color, h->aux_stream));
    copy_kernel_async(F.host_res, C->buf.stats, (size_t)n * FORENSIC_STATS * 8, h->aux_stream);
    copy_kernel_async(F.host_res + (size_t)n * FORENSIC_STATS, C->buf.stats_noise, (size_t)n * G.nblk * 8, h->aux_stream);
    copy_kernel_async(F.host_res + (size_t)n * (FORENSIC_STATS + G.nblk), C->buf.stats_ela, (size_t)n * G.nblk * 8, h->aux_stream);
    DFD_HIP_TRY(h, hipGetLastError());
    DFD_HIP_TRY(h, hipEventRecord(h->aux_done, h->aux_stream));
    return DFD_OK;
}

int forensics_batch_end(dfd_handle* h, int n, double* prob_out, double* scores_out) {
    ForensicChain* C = nullptr;                                      // the chain forensics_batch_begin ran on
    const int rc = chain_reserve(h, false, FIXED_EDGE, n, &C);
    if (rc) return rc;
    const double* res = h->forensic->host_res;
    DFD_HIP_TRY(h, hipEventSynchronize(h->aux_done));
    score_stateless(C->G, res, res + (size_t)n * FORENSIC_STATS, res + (size_t)n * (FORENSIC_STATS + C->G.nblk), n, prob_out, scores_out);
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
    return forensics_chain_run(h, stream_id, false, FIXED_EDGE, (const uint8_t*)h->frame_buf.p, hh, ww, stride, full, scores_out,
                               prob_out, stats_out);
}

int dfd_forensics_sized(dfd_handle* h, int stream_id, const uint8_t* bgr, int hh, int ww, int stride, int size, int full,
                        double* scores_out, double* prob_out, double* stats_out) {
    if (!h) return DFD_ERR_ARG;
    if (!bgr || !scores_out || !prob_out || hh <= 0 || ww <= 0 || stride < ww * 3)
        return fail(h, DFD_ERR_ARG, "forensics_sized: bad pointer or geometry");
    if (!edge_ok(size))
        return fail(h, DFD_ERR_ARG, "forensics_sized: analysis size %d is not a multiple of 16 in %d..%d", size, EDGE_MIN, EDGE_MAX);
    if (!h->has_color) return fail(h, DFD_ERR_STATE, "forensics needs the colour tables (blob packed without luts)");
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    int rc = stream_size_check(h, stream_id, size);
    if (rc) return rc;
    if ((rc = ensure(h, &h->frame_buf, (size_t)hh * stride))) return rc;
    DFD_HIP_TRY(h, hipMemcpyAsync(h->frame_buf.p, bgr, (size_t)hh * stride, hipMemcpyHostToDevice, h->stream));
    return forensics_chain_run(h, stream_id, true, size, (const uint8_t*)h->frame_buf.p, hh, ww, stride, full, scores_out, prob_out,
                               stats_out);
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
    ForensicChain* C = nullptr;
    int rc = chain_reserve(h, false, FIXED_EDGE, n, &C);
    if (rc) return rc;
    ForensicState& F = *h->forensic;
    const ForensicGeometry& G = C->G;
    if ((rc = ensure(h, &F.pair_idx, (size_t)n * 4))) return rc;
    if ((rc = ensure(h, &F.pair_part, (size_t)n * G.npart * 8))) return rc;
    const int stride = ww * 3;
    if ((rc = mailbox_h2d(h, F.pair_idx.p, prev_index, (size_t)n * 4))) return rc;
    launch_resize_bgr(frames_dev, n, hh, ww, stride, (size_t)hh * stride, C->buf.rs, G.S, G.S, h->stream);
    DFD_HIP_TRY(h, chain_launch(*C, C->buf, ns, true, h->color, h->stream, n - ns));
    if (ns > 0) launch_absdiff_pairs(C->buf.gray, (const int*)F.pair_idx.p, (double*)F.pair_part.p, ns, h->stream);
    const size_t nz = ns > 0 ? ns : 1;
    const double* st = (const double*)mailbox_d2h(h, C->buf.stats, nz * FORENSIC_STATS * 8);
    const double* noise = (const double*)mailbox_d2h(h, C->buf.stats_noise, nz * G.nblk * 8);
    const double* ela = (const double*)mailbox_d2h(h, C->buf.stats_ela, nz * G.nblk * 8);
    const double* part = (const double*)mailbox_d2h(h, F.pair_part.p, nz * G.npart * 8);
    if (!st || !noise || !ela || !part) return fail(h, DFD_ERR_HIP, "forensics: mailbox allocation failed");
    DFD_HIP_TRY(h, stream_sync(h));
    DFD_HIP_TRY(h, hipGetLastError());
    for (int f = ns; f < n; ++f) {                           // predecessor-only frames: no signals
        for (int i = 0; i < 5; ++i) scores5_out[(size_t)f * 5 + i] = -1.0;
        mean_diff_out[f] = -1.0;
    }
    for (int f = 0; f < ns; ++f) {
        double sc[6], ex[10];
        static_scores(G, &st[(size_t)f * FORENSIC_STATS], &noise[(size_t)f * G.nblk], &ela[(size_t)f * G.nblk], true, sc, ex);
        for (int i = 0; i < 5; ++i) scores5_out[(size_t)f * 5 + i] = sc[i];
        // the summation order of a stream's frame (score_frame)
        mean_diff_out[f] = prev_index[f] < 0 ? -1.0 : mean_abs_diff(G, &part[(size_t)f * G.npart]);
    }
    return DFD_OK;
}

int dfd_forensic_tap(dfd_handle* h, const uint8_t* bgr256, int n, int full, const char* start, const void* start_data,
                     const char* name, int frame, void* out, size_t capacity, size_t* bytes) {
    if (!h) return DFD_ERR_ARG;
    if (!start || !name || !out || !bytes || n <= 0 || n > 64 || frame < -1 || frame >= n)
        return fail(h, DFD_ERR_ARG, "forensic_tap: bad pointer, frame index or frame count (1..64)");
    return forensic_tap_run(h, "forensic_tap", false, FIXED_EDGE, bgr256, n, full, start, start_data, name, frame, out, capacity, bytes);
}

int dfd_forensic_tap_sized(dfd_handle* h, const uint8_t* frames, int n, int size, int full, const char* start, const void* start_data,
                           const char* name, int frame, void* out, size_t capacity, size_t* bytes) {
    if (!h) return DFD_ERR_ARG;
    if (!start || !name || !out || !bytes || n <= 0 || n > 16 || frame < -1 || frame >= n)
        return fail(h, DFD_ERR_ARG, "forensic_tap_sized: bad pointer, frame index or frame count (1..16)");
    if (!edge_ok(size))
        return fail(h, DFD_ERR_ARG, "forensic_tap_sized: analysis size %d is not a multiple of 16 in %d..%d", size, EDGE_MIN, EDGE_MAX);
    return forensic_tap_run(h, "forensic_tap_sized", true, size, frames, n, full, start, start_data, name, frame, out, capacity, bytes);
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

int dfd_forensics_open(dfd_handle* h, int stream_id, int size) {
    if (!h) return DFD_ERR_ARG;
    if (!edge_ok(size))
        return fail(h, DFD_ERR_ARG, "forensics_open: analysis size %d is not a multiple of 16 in %d..%d", size, EDGE_MIN, EDGE_MAX);
    DFD_HIP_TRY(h, hipSetDevice(h->device));
    int rc = stream_size_check(h, stream_id, size);                  // another size already: refused, nothing changes
    if (rc) return rc;
    if (!h->forensic) h->forensic = new ForensicState();
    ForensicStream& S = h->forensic->streams[stream_id];
    if (S.size) return DFD_OK;                                       // the same size: as it is
    S.size = size;
    S.general = true;
    return DFD_OK;
}

}  // extern "C"
