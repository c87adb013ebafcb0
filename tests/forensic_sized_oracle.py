"""Test helper (CPU): size-generic per-stage references for the general forensic chain (csrc/forensic_kernels.hip, run-time edge),
built only on oracle/imgproc_ref.py, oracle/jpeg_ref.py and numpy float64, the fixture frames of the sized tests and the
condition they must meet.  Buffer layouts are the device's: see dfd_forensic_tap_sized in include/dfd_hip.h."""
import functools

import numpy as np

import frames as F
from oracle import imgproc_ref as I
from oracle import jpeg_ref as J
from oracle.forensics_ref import ForensicsRef

# the bars of tests/test_forensics_gpu.py, restated
STAT_RTOL = 2e-4
EXACT = ("ela_mean", "edge_density", "unique_hues", "mean_diff")
THRESHOLDS = {"freq_high_ratio": (0.18, 0.2, 0.22), "freq_mid_cv": (0.45, 0.6), "freq_mid_ratio": (0.45,),
              "noise_cv": (0.5, 0.7), "noise_mean": (1.0, 2.0), "ela_cv": (0.6, 0.9), "ela_mean": (10, 15),
              "edge_density": (0.02, 0.04), "lap_var": (50, 100), "sat_std": (15, 25), "val_std": (15, 25),
              "unique_hues": (30, 50), "temporal_cv": (1.0, 1.5), "mean_diff": (0.3, 0.8)}
INTEGER_STATS = ("unique_hues",)
EPS64 = 2.0 ** -53
LOW, HIGH = 50, 150

# 48: one block (noise / ELA score 0.0); 64: four blocks, one bitboard word per row; 80: S % 32 == 16, a row ends inside
# a word, factor 5; 272 = 16 * 17, just over 256; 512; 1024: the largest, one frame only
SIZES = (48, 64, 80, 272, 512)
LARGEST = 1024
TAP_SIZES = (64, 80, 272)


# ------------------------------------------------------------------------------------------------ fixtures
def wave_frame(h=270, w=480, seed=3):
    """sinusoids + channel offsets + N(0, 6) noise: every thresholded statistic away from every threshold"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 96 + 60 * np.sin(xx / 17.0) + 40 * np.cos(yy / 11.0)
    img = base[..., None] + np.array([0.0, 12.0, -9.0]) + rng.normal(0.0, 6.0, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def largest_frame():
    """the frame of the single run at the largest size: the wave frame at 540 x 960 (the 270 x 480 one, upscaled 3.8
    times, leaves lap_var within 0.2 % of a threshold at 1024)"""
    return wave_frame(540, 960)


def constant_is_exact(S):
    """whether numpy's float64 fft2 of a constant S x S plane is exactly zero off the DC bin.  Where it is not (272 =
    16 * 17), the reference's mid-band statistics of a constant frame are ratios of its own rounding residue
    (freq_mid ~ 1e-12, freq_mid_cv = O(0.1) of nothing), not something a device can be held to: the constant frame
    does not qualify at that size and the near-constant `faint_frame` takes its place."""
    x = np.abs(np.fft.fft2(np.full((S, S), 128.0)))
    x[0, 0] = 0.0
    return bool(x.max() == 0.0)


def faint_frame(h=256, w=256):
    """a smooth frame that is not constant: 128 with a +-2 grey-level ripple, so every band holds real signal"""
    yy, xx = np.mgrid[0:h, 0:w]
    v = (128 + ((xx // 3 + yy // 5) % 5) - 2).astype(np.uint8)
    return np.repeat(v[..., None], 3, -1)


def fixture_frames(S=None):
    """the fixtures of the sized tests; at a size S where the constant frame does not qualify (see constant_is_exact)
    `smooth` is replaced by `faint`"""
    out = {"wave": wave_frame(), "smooth": F.smooth_image(), "noisy": F.noisy_image(), "gradient": F.gradient_image(),
           "determinism": F.determinism_frame()}
    if S is not None and not constant_is_exact(S):
        del out["smooth"]
        out["faint"] = faint_frame()
    return out


def moving_sequence(n=3, h=180, w=320):
    """a bright textured square moving over a wave background: n frames for the temporal signal"""
    out = []
    for i in range(n):
        f = wave_frame(h, w, seed=7).copy()
        x0 = 40 + 23 * i
        f[50:110, x0:x0 + 60] = np.random.RandomState(5).randint(120, 255, (60, 60, 3)).astype(np.uint8)
        out.append(f)
    return out


def schedule_frames(n=13, h=135, w=240):
    """n frames of one stream with the reference's full / fast mix (every third frame full): jitter around a base frame,
    frames 6 and 7 repeating frame 5 (zero difference), so the temporal deque fills, `frame_count > 10` engages and the
    temporal thresholds see both small and large coefficients of variation"""
    rs = np.random.RandomState(11)
    base = wave_frame(h, w, seed=9).astype(np.int16)
    out, cur = [], None
    for i in range(n):
        if i not in (6, 7):
            cur = np.clip(base + rs.randint(-3, 4, base.shape) + i, 0, 255).astype(np.uint8)
        out.append((cur, i % 3 == 0))
    return out


def margin(stats):
    """(smallest relative distance of a float statistic to one of its thresholds, smallest count distance of an integer
    one) over the statistics present"""
    rel, cnt = np.inf, np.inf
    for k, ts in THRESHOLDS.items():
        if k not in stats or (k == "mean_diff" and stats[k] < 0):
            continue
        for t in ts:
            if k in INTEGER_STATS:
                cnt = min(cnt, abs(stats[k] - t))
            else:
                rel = min(rel, abs(stats[k] - t) / max(1.0, abs(t)))
    return rel, cnt


# ------------------------------------------------------------------------------------------------ stages at size S
def resized(frame, S):
    return I.resize_linear_u8(frame, S, S)


def gray(bgr):
    return I.bgr2gray_u8(bgr)


def grad(g):
    dx, dy = I.sobel3_i32(g)
    return np.stack([dx, dy], -1).astype(np.int16)


def lap_part(g):
    """[S][2]: sum and sum of squares of the Laplacian over each image row"""
    lap = I.laplacian_i32(g).astype(np.int64)
    return np.stack([lap.sum(1), (lap * lap).sum(1)], -1)


def labels(gr):
    return I.canny_labels(gr[..., 0], gr[..., 1], LOW, HIGH)


def edges(lab):
    return I.hysteresis(lab).astype(np.uint8)


def jpeg_planes(bgr):
    """decoded Y, Cb, Cr planes of the quality-90 4:2:0 round trip (chroma at S/2 x S/2)"""
    y, cb, cr = J.rgb_to_ycc(bgr[..., ::-1])
    ql, qc = J.quant_table(J._LUMA, 90), J.quant_table(J._CHROMA, 90)
    return tuple(np.asarray(a, np.uint8) for a in (J.code_plane(y, ql), J.code_plane(J.h2v2_downsample(cb), qc),
                                                   J.code_plane(J.h2v2_downsample(cr), qc)))


def blocks(a, size=32):
    """the reference's block list (frame_analysis.py:196-199): [(S // 32)^2][32][32], row-major"""
    h, w = a.shape
    return np.stack([a[i:i + size, j:j + size] for i in range(0, h - size + 1, size) for j in range(0, w - size + 1, size)])


def ela_block_sums(bgr):
    jy, jcb, jcr = (p.astype(np.int64) for p in jpeg_planes(bgr))
    dec = J.ycc_to_rgb(jy, J.h2v2_fancy_upsample(jcb), J.h2v2_fancy_upsample(jcr))[..., ::-1]
    diff = np.abs(bgr.astype(np.int16) - dec.astype(np.int16)).astype(np.uint8)
    return blocks(I.bgr2gray_u8(diff).astype(np.int64)).sum((1, 2))


def noise_stds(g):
    g32 = g.astype(np.float32)
    r = (g32 - I.gaussian5_f32(g32)).astype(np.float64)
    return blocks(r).reshape(-1, 1024).std(1)


def hsv_part(bgr):
    """[S][4]: per image row, sums of S, S^2, V, V^2; and the 180-bit hue set as 6 words"""
    hsv = I.bgr2hsv_u8(bgr).astype(np.int64)
    s, v = hsv[..., 1], hsv[..., 2]
    bits = np.zeros(6, np.uint32)
    for h in np.unique(hsv[..., 0]):
        bits[h >> 5] |= np.uint32(1) << np.uint32(h & 31)
    return np.stack([s.sum(1), (s * s).sum(1), v.sum(1), (v * v).sum(1)], -1), bits


@functools.lru_cache(maxsize=None)
def band_masks(S):
    """ForensicsRef((S, S))'s three masks, moved from fftshift order to bin order [ky][kx]"""
    r = ForensicsRef((S, S))
    d = r._dist
    low, mid, high = d <= r._inner, (d > r._inner) & (d <= r._mid), (d > r._mid) & (d <= r._outer)
    return tuple(np.fft.ifftshift(m) for m in (low, mid, high))


def fft_float64(g):
    """(fft_tmp, spectrum) in float64, in the device's transposed layouts [kx][row], [kx][ky]"""
    g64 = g.astype(np.float64)
    return np.fft.fft(g64, axis=1).T, np.fft.fft2(g64).T


def band_sums(spec_t):
    """the seven band sums of a transposed spectrum in float64: low sum, count, mid sum, sum of squares, count, high
    sum, count"""
    S = spec_t.shape[0]
    mag = np.log1p(np.abs(spec_t))
    low, mid, high = (m.T for m in band_masks(S))
    return np.array([mag[low].sum(), low.sum(), mag[mid].sum(), (mag[mid] ** 2).sum(), mid.sum(), mag[high].sum(), high.sum()])


def stats_from_stages(frame, S, prev_gray=None):
    """the statistics ForensicsRef((S, S)).analyze reports, from the stage references above"""
    bgr = resized(frame, S)
    g = gray(bgr)
    out = {}
    b = band_sums(fft_float64(g)[1])
    lo, mi, hi = b[0] / b[1], b[2] / b[4], b[5] / b[6]
    total = lo + mi + hi + 1e-10
    mid_std = np.sqrt(max(b[3] / b[4] - mi * mi, 0.0))
    out.update(freq_low=lo, freq_mid=mi, freq_high=hi, freq_high_ratio=hi / total, freq_mid_ratio=mi / total,
               freq_mid_cv=mid_std / (mi + 1e-10))
    if (S // 32) ** 2 >= 4:
        ns = noise_stds(g)
        out.update(noise_mean=ns.mean(), noise_cv=ns.std() / (ns.mean() + 1e-10))
        em = ela_block_sums(bgr) / 1024.0
        out.update(ela_mean=em.mean(), ela_cv=em.std() / (em.mean() + 1e-10))
    lp = lap_part(g).sum(0)
    out.update(edge_density=edges(labels(grad(g))).sum() / float(S * S), lap_var=lp[1] / (S * S) - (lp[0] / (S * S)) ** 2)
    part, bits = hsv_part(bgr)
    s1, s2, v1, v2 = part.sum(0) / float(S * S)
    out.update(sat_std=np.sqrt(s2 - s1 * s1), val_std=np.sqrt(v2 - v1 * v1), unique_hues=float(sum(bin(int(x)).count("1") for x in bits)))
    # np.mean of a float32 plane: the integer sum (exact in float32 below 2^24) divided in float32
    out["mean_diff"] = -1.0 if prev_gray is None else float(
        np.float32(np.abs(g.astype(np.int64) - prev_gray.astype(np.int64)).sum()) / np.float32(S * S))
    return out, g


# ------------------------------------------------------------------------------------------------ FFT yardstick
FFT_RMS_X, FFT_MAX_X = 4.0, 8.0         # tests/forensic_oracle.py's multipliers of the fp32 yardstick's error


def fft_yardstick(g):
    """the fp32 yardstick: scipy's complex64 transforms of the float32 image, device layouts (any S)"""
    import scipy.fft

    g32 = g.astype(np.float32)
    a, b = scipy.fft.fft(g32, axis=1).T, scipy.fft.fft2(g32).T
    assert a.dtype == np.complex64 and b.dtype == np.complex64
    return a, b


def fft_error(got, ref64):
    d = np.abs(got.astype(np.complex128) - ref64)
    return float(np.sqrt(np.mean(d * d))), float(d.max())


def fft_ratios(got, ref64, yard):
    (r, m), (yr, ym) = fft_error(got, ref64), fft_error(yard, ref64)
    q = lambda a, b: 0.0 if a == 0 else (np.inf if b == 0 else a / b)
    return q(r, yr), q(m, ym)


def fft_meets_bar(got, ref64, yard):
    r, m = fft_ratios(got, ref64, yard)
    return r <= FFT_RMS_X and m <= FFT_MAX_X


# ------------------------------------------------------------------------------------------------ hysteresis maps
def hysteresis_maps(S):
    """label maps no image produces: serpentines that need one sweep per row or column, chains along a row through every
    64-bit word border and into the last (partial) word in both directions, diagonals, touches across each word border
    and at the row end, no wrap from the last column of a row to the first of the next"""
    m = {}
    blank = lambda: np.ones((S, S), np.uint8)
    a = blank(); a[0::2, :] = 0; a[1::4, S - 1] = 0; a[3::4, 0] = 0; a[0, 0] = 2; m["serpentine_rows"] = a
    m["serpentine_columns"] = np.ascontiguousarray(a.T)
    for name, row, src in (("row_l2r", S // 3, 0), ("row_r2l", S // 3 + 1, S - 1)):
        a = blank(); a[row, :] = 0; a[row, src] = 2; m[name] = a
    i = np.arange(S)
    a = blank(); a[i, i] = 0; a[0, 0] = 2; m["diag_down"] = a
    a = blank(); a[i, S - 1 - i] = 0; a[S - 1, 0] = 2; m["anti_up"] = a
    borders = list(range(64, S, 64)) + [S - 1]
    for r in (0, S // 2, S - 1):
        for border in borders:
            for k, (dy, dx) in enumerate([(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]):
                for side in (0, 1):
                    sx = border - 1 + side
                    wy, wx = r + dy, sx + dx
                    if not (0 <= wy < S and 0 <= wx < S and sx < S):
                        continue
                    a = blank(); a[r, sx] = 2; a[wy, wx] = 0
                    if 0 <= wy + dy < S and 0 <= wx + dx < S:
                        a[wy + dy, wx + dx] = 0
                    m[f"touch_r{r}_b{border}_d{k}_s{side}"] = a
    a = blank(); a[10, S - 1] = 2; a[11, 0] = 0; a[10, 0] = 0; a[9, 0] = 0; m["no_wrap_right"] = a
    a = blank(); a[10, 0] = 2; a[9, S - 1] = 0; a[10, S - 1] = 0; a[11, S - 1] = 0; m["no_wrap_left"] = a
    a = blank(); a[0, :] = 0; a[S - 1, :] = 0; a[:, 0] = 0; a[:, S - 1] = 0; a[0, 0] = 2; m["border_ring"] = a
    m["all_weak"] = np.zeros((S, S), np.uint8)
    m["all_strong"] = np.full((S, S), 2, np.uint8)
    return m


def random_maps(S, count=50, seed=5):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        p_strong, p_weak = 10.0 ** rs.uniform(-4, -1), rs.uniform(0.05, 0.7)
        u = rs.rand(S, S)
        out.append(np.where(u < p_strong, 2, np.where(u < p_strong + p_weak, 0, 1)).astype(np.uint8))
    return out
