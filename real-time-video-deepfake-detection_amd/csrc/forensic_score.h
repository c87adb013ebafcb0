// Host half of the forensic analyzer as plain C++ (no HIP): device statistics -> the reference's threshold scoring
// (reference frame_analysis.py:58-389) and the per-stream temporal step.  forensic_api.hip runs it after the wait;
// host_asan_driver.cpp runs it on recorded statistics under the sanitizers (tests/test_host_asan.py).
#pragma once
#include <cmath>
#include <cstddef>
#include <deque>
#include <vector>

namespace dfd {

// per-frame scalar statistics produced on the device (doubles)
enum ForensicStat {
    ST_FREQ_LOW = 0, ST_FREQ_MID, ST_FREQ_HIGH, ST_FREQ_MID_STD, ST_LAP_VAR, ST_EDGE_COUNT,
    ST_SAT_STD, ST_VAL_STD, ST_HUES, FORENSIC_STATS
};

// what the scoring needs to know of a chain (forensic_api.hip: ForensicChain)
struct ForensicGeometry {
    int S = 256;             // analysis edge
    double npix = 65536.0;   // S * S
    int nblk = 64;           // 32x32 blocks (fewer than 4: noise and ELA score 0.0, reference :204,:255)
    int npart = 256;         // partial sums of a frame's difference against its predecessor (one per image row)
    bool f32_means = false;  // the reference's np.mean of float32 values, divided in float32 (the general chain); in double
                             // otherwise (the 256x256 chain, where both quotients are exact)
    bool general = false;    // the run-time-edge instantiation of forensic_kernels.hip (DFT spectrum)
};

// what crosses the frames of a stream (frame_analysis.py:34-37)
struct ForensicTemporal {
    bool has_prev = false;
    std::deque<double> diffs;      // last 30 mean absolute differences
    int frame_count = 0;
};

inline double pop_std(const double* v, int n, double* mean_out) {
    double m = 0;
    for (int i = 0; i < n; ++i) m += v[i];
    m /= n;
    double q = 0;
    for (int i = 0; i < n; ++i) q += (v[i] - m) * (v[i] - m);
    *mean_out = m;
    return std::sqrt(q / n);
}

inline double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

// the five stateless signals from the device statistics (frame_analysis.py:150-347); sc[5] (temporal) = 0
inline void static_scores(const ForensicGeometry& G, const double* st, const double* noise, const double* ela, bool full,
                          double* sc, double* ex) {
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
    const double density = st[ST_EDGE_COUNT] / G.npix, lap_var = st[ST_LAP_VAR];
    s = 0.0;
    if (density < 0.02) s += 0.35; else if (density < 0.04) s += 0.15;
    if (lap_var < 50) s += 0.3; else if (lap_var < 100) s += 0.1;
    sc[3] = clip01(s);
    double noise_mean = nan, noise_cv = nan, ela_mean = nan, ela_cv = nan;
    if (full && G.nblk < 4) sc[1] = sc[2] = 0.0;
    if (full && G.nblk >= 4) {
        // ---- noise (:207-225)
        noise_cv = pop_std(noise, G.nblk, &noise_mean) / (noise_mean + 1e-10);
        s = 0.0;
        if (noise_cv > 0.7) s += 0.5; else if (noise_cv > 0.5) s += 0.25;
        if (noise_mean < 1.0) s += 0.3; else if (noise_mean < 2.0) s += 0.1;
        sc[1] = clip01(s);
        // ---- ELA (:258-276)
        ela_cv = pop_std(ela, G.nblk, &ela_mean);
        // the reference's block means are float32 and so is their mean (:250-256); at 256x256 the quotient by 64 is exact
        if (G.f32_means) ela_mean = (double)(float)ela_mean;
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

// the weighted sum in the reference's dict order: all six signals (:49-56,88) or the fast three (:118-119)
inline double weighted_sum(const double* sc, bool full) {
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

// mean |gray - previous gray| from the frame's partial sums, added in their order.  np.mean of a float32 plane (:364)
// is the integer sum (exact in float32 below 2^24) divided in float32.
inline double mean_abs_diff(const ForensicGeometry& G, const double* dpart) {
    double sum = 0;
    for (int i = 0; i < G.npart; ++i) sum += dpart[i];
    return G.f32_means ? (double)((float)sum / (float)G.npix) : sum / G.npix;
}

// the host half of one frame of a stream, in the stream's frame order: frame counter, temporal deque and signal
// (frame_analysis.py:358-389; dpart = the frame's partial sums against its predecessor, read only when the stream has
// one), then the weighted sum.  sc[6] / ex[10] as static_scores; *mean_diff / *temporal_cv: -1 / NaN when not computed.
inline double score_frame(ForensicTemporal& S, const ForensicGeometry& G, const double* st, const double* noise,
                          const double* ela, bool full, const double* dpart, double* sc, double* ex, double* mean_diff,
                          double* temporal_cv) {
    S.frame_count += 1;                                              // frame_analysis.py:68,110
    static_scores(G, st, noise, ela, full, sc, ex);
    *mean_diff = -1.0;
    *temporal_cv = std::nan("");
    if (!S.has_prev) {
        S.has_prev = true;
    } else {
        const double md = mean_abs_diff(G, dpart);
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
    return weighted_sum(sc, full);
}

// n frames without a stream (the temporal signal at its first-frame value 0, :358-360): statistics, block arrays -> the
// six-signal probability each
inline void score_stateless(const ForensicGeometry& G, const double* st, const double* noise, const double* ela, int n,
                            double* prob_out, double* scores_out) {
    for (int f = 0; f < n; ++f) {
        double sc[6], ex[10];
        static_scores(G, &st[(size_t)f * FORENSIC_STATS], &noise[(size_t)f * G.nblk], &ela[(size_t)f * G.nblk], true, sc, ex);
        prob_out[f] = weighted_sum(sc, true);
        if (scores_out)
            for (int i = 0; i < 6; ++i) scores_out[(size_t)f * 6 + i] = sc[i];
    }
}

}  // namespace dfd
