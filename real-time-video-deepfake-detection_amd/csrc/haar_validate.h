// Host-only check of a Haar cascade's four blob tensors (plain C++, no HIP; also built into the sanitizer harness).
// haar_eval_kernel indexes the stump table by the stages, the feature table by the stumps and the integral image by the
// rectangles without further checks, so haar_init refuses, before any launch, a cascade whose numbers would take one of
// those reads outside its buffer.  haar.validate_cascade is the same list in Python (the XML reader raises on it).
#pragma once
#include <cmath>
#include <cstddef>

namespace dfd {

// a float that holds an integer in [lo, hi] (NaN and infinities fail every comparison)
inline bool haar_int_in(float v, double lo, double hi) { return v >= lo && v <= hi && v == std::floor(v); }

// nullptr when the cascade is sound, else what is wrong with it.  win [2] = width, height; stages [n_stages][3] = first
// stump, stump count, threshold; stumps [n_stumps][4] = feature, threshold, left, right; rects [n_feats][3][5] = x, y, w,
// h, weight.  Slots 0 and 1 of a feature are always read, so their geometry must fit whatever their weight; slot 2 is
// read only when its weight is non-zero and is all zero otherwise.
inline const char* haar_cascade_error(const float* win, const float* stages, size_t n_stages, const float* stumps, size_t n_stumps,
                                      const float* rects, size_t n_feats) {
    constexpr double kMaxWin = 4096.0;
    if (!haar_int_in(win[0], 4, kMaxWin) || !haar_int_in(win[1], 4, kMaxWin)) return "window is not an integer size of 4 .. 4096";
    if (n_stages < 1 || n_stumps < 1 || n_feats < 1) return "no stages, stumps or features";
    if (n_stumps > (size_t)1 << 24 || n_feats > (size_t)1 << 24) return "more stumps or features than a float can index";
    const double win_w = win[0], win_h = win[1];
    double next = -1.0;
    for (size_t s = 0; s < n_stages; ++s) {
        const float* st = stages + 3 * s;
        if (!haar_int_in(st[0], 0, (double)n_stumps) || !haar_int_in(st[1], 1, (double)n_stumps) ||
            (double)st[0] + (double)st[1] > (double)n_stumps)
            return "a stage's stumps run outside the stump table";
        if (s && (double)st[0] != next) return "stages are not contiguous in order";
        if (!std::isfinite(st[2])) return "a stage threshold is not finite";
        next = (double)st[0] + (double)st[1];
    }
    for (size_t k = 0; k < n_stumps; ++k) {
        const float* sp = stumps + 4 * k;
        if (!haar_int_in(sp[0], 0, (double)n_feats - 1.0)) return "a stump's feature index is outside the feature table";
        if (!std::isfinite(sp[1]) || !std::isfinite(sp[2]) || !std::isfinite(sp[3])) return "a stump's threshold or leaf is not finite";
    }
    for (size_t f = 0; f < n_feats; ++f)
        for (int j = 0; j < 3; ++j) {
            const float* r = rects + 15 * f + 5 * j;
            for (int i = 0; i < 5; ++i)
                if (!std::isfinite(r[i])) return "a rectangle holds a value that is not finite";
            if (j == 2 && r[4] == 0.f) {
                if (r[0] != 0.f || r[1] != 0.f || r[2] != 0.f || r[3] != 0.f) return "an unused third rectangle has geometry";
                continue;
            }
            if (!haar_int_in(r[0], 0, win_w) || !haar_int_in(r[1], 0, win_h) || !haar_int_in(r[2], 1, win_w) ||
                !haar_int_in(r[3], 1, win_h) || (double)r[0] + (double)r[2] > win_w || (double)r[1] + (double)r[3] > win_h)
                return "a rectangle is not an integer box inside the window";
        }
    return nullptr;
}

}  // namespace dfd
