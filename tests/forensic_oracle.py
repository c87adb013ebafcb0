"""Test helper (CPU): per-stage references for the forensic kernels at 256x256 (csrc/forensic_kernels.hip, the
compile-time edge), the inputs the stage tests run them on, and the bars they are held to.  Everything is built from oracle/imgproc_ref.py and
oracle/jpeg_ref.py; the integer stages are exact, the noise residual is the oracle's fp32 blur bit for bit, and the FFT
has two references: numpy's float64 fft2 and `fft_mirror`, the kernel's radix-2 butterflies restated in numpy float32
(every operation a single IEEE add or multiply, as the kernels are compiled without contraction).

Buffer layouts are the device's: see dfd_forensic_tap in include/dfd_hip.h."""
from fractions import Fraction

import numpy as np

import frames as F
from oracle import imgproc_ref as I
from oracle import jpeg_ref as J
from oracle.forensics_ref import ForensicsRef

FS = 256
EPS64 = 2.0 ** -53
LOW, HIGH = 50, 150

# ------------------------------------------------------------------------------------------------ bars
NOISE_RTOL = 4 * 1024 * EPS64           # 1024-term double sums, two passes and a sqrt
BAND_RTOL = 4 * 128 * EPS64             # a row partial adds at most 256 floats in a 128-leaf tree
FFT_RMS_X, FFT_MAX_X = 4.0, 8.0         # times the fp32 yardstick's error against float64 (the classifier's multipliers)


def cancel_rtol(sum1, sum2, n):
    """relative bar for var = E[x^2] - mean^2 in doubles: 8 * 2^-53 * E[x^2] / var (None where var == 0)"""
    var = Fraction(sum2, n) - Fraction(sum1, n) ** 2
    return None if var == 0 else 8 * EPS64 * float(Fraction(sum2, n) / var)


# ------------------------------------------------------------------------------------------------ integer stages
def gray(bgr):
    return I.bgr2gray_u8(bgr)


def grad(g):
    """Sobel dx, dy as the device stores them: int16 [256][256][2]"""
    dx, dy = I.sobel3_i32(g)
    return np.stack([dx, dy], -1).astype(np.int16)


def lap_part(g):
    """[256][2]: sum and sum of squares of the Laplacian over each image row (one 256-pixel block each)"""
    lap = I.laplacian_i32(g).astype(np.int64)
    return np.stack([lap.sum(1), (lap * lap).sum(1)], -1)


def labels(gr, **kw):
    return I.canny_labels(gr[..., 0], gr[..., 1], LOW, HIGH, **kw)


def edges(lab):
    return I.hysteresis(lab).astype(np.uint8)


def jpeg_planes(bgr, bias=(1, 2)):
    """decoded Y, Cb, Cr planes of the quality-90 4:2:0 round trip (chroma at 128x128).  `bias` = (1, 2) is libjpeg's
    alternating h2v2 rounding; anything else is a mutant."""
    y, cb, cr = J.rgb_to_ycc(bgr[..., ::-1])
    ql, qc = J.quant_table(J._LUMA, 90), J.quant_table(J._CHROMA, 90)
    if bias == (1, 2):
        down = J.h2v2_downsample
    else:
        down = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
                          + np.where(np.arange(p.shape[1] // 2) % 2 == 0, bias[0], bias[1])[None, :]) >> 2
    return tuple(np.asarray(a, np.uint8) for a in (J.code_plane(y, ql), J.code_plane(down(cb), qc), J.code_plane(down(cr), qc)))


def block_sums(a, size=32):
    """[64] sums of the 32x32 blocks, row-major"""
    return a.reshape(FS // size, size, FS // size, size).sum((1, 3)).ravel()


def ela_block_sums(bgr, planes=None):
    """[64] integer sums of gray(|frame - decoded|) per 32x32 block, decoded from `planes` (default: the reference's)"""
    jy, jcb, jcr = (p.astype(np.int64) for p in (planes or jpeg_planes(bgr)))
    dec = J.ycc_to_rgb(jy, J.h2v2_fancy_upsample(jcb), J.h2v2_fancy_upsample(jcr))[..., ::-1]
    diff = np.abs(bgr.astype(np.int16) - dec.astype(np.int16)).astype(np.uint8)
    return block_sums(I.bgr2gray_u8(diff).astype(np.int64))


def hsv_part(bgr):
    """[256][4]: per image row, sums of S, S^2, V, V^2; and the 180-bit hue set as 6 words"""
    hsv = I.bgr2hsv_u8(bgr).astype(np.int64)
    s, v = hsv[..., 1], hsv[..., 2]
    bits = np.zeros(6, np.uint32)
    for h in np.unique(hsv[..., 0]):
        bits[h >> 5] |= np.uint32(1) << np.uint32(h & 31)
    return np.stack([s.sum(1), (s * s).sum(1), v.sum(1), (v * v).sum(1)], -1), bits


# ------------------------------------------------------------------------------------------------ noise
def noise_residual(g, blur=I.gaussian5_f32):
    g32 = g.astype(np.float32)
    return g32 - blur(g32)


def blur_reflect(g32):
    """mutant: the same blur with BORDER_REFLECT (edge pixel repeated) instead of BORDER_REFLECT_101"""
    return I.gaussian5_f32(np.pad(g32, 2, mode="symmetric"))[2:-2, 2:-2]


def noise_stds(g, blur=I.gaussian5_f32):
    """[64] float64 population std of the fp32 residual per 32x32 block"""
    r = noise_residual(g, blur).astype(np.float64)
    return r.reshape(8, 32, 8, 32).transpose(0, 2, 1, 3).reshape(64, 1024).std(1)


# ------------------------------------------------------------------------------------------------ FFT
def band_masks():
    """ForensicsRef's three sqrt-distance masks, moved from fftshift order to bin order [ky][kx]"""
    r = ForensicsRef()
    d = r._dist
    low, mid, high = d <= r._inner, (d > r._inner) & (d <= r._mid), (d > r._mid) & (d <= r._outer)
    return tuple(np.fft.ifftshift(m) for m in (low, mid, high))


def twiddles():
    """the table the handle uploads: exp(-2 pi i k / 256), k < 128, cos / sin in double rounded to float"""
    a = -2.0 * np.pi * np.arange(128) / 256.0
    return (np.cos(a).astype(np.float32) + 1j * np.sin(a).astype(np.float32)).astype(np.complex64)


def twiddles_recurrence():
    """mutant: the table by repeated fp32 complex multiplication with its entry 1"""
    tw = twiddles()
    out = np.empty(128, np.complex64)
    out[0] = 1
    wr, wi = tw[1].real, tw[1].imag
    for k in range(1, 128):
        pr, pi = out[k - 1].real, out[k - 1].imag
        out[k] = np.float32(pr * wr - pi * wi) + 1j * np.float32(pr * wi + pi * wr)
    return out


_BREV = np.array([int(f"{i:08b}"[::-1], 2) for i in range(256)])


def fft256_mirror(x, tw):
    """fft256_lds on every row of complex64 x [..., 256]: bit-reversed load, 8 radix-2 DIT stages in float32"""
    xr, xi = x.real.astype(np.float32)[..., _BREV], x.imag.astype(np.float32)[..., _BREV]
    twr, twi = tw.real.astype(np.float32), tw.imag.astype(np.float32)
    tid = np.arange(128)
    half = 1
    while half < 256:
        pos = tid & (half - 1)
        i0 = ((tid - pos) << 1) + pos
        i1 = i0 + half
        wr, wi = twr[pos * (128 // half)], twi[pos * (128 // half)]
        ar, ai, br, bi = xr[..., i0], xi[..., i0], xr[..., i1], xi[..., i1]
        tr = br * wr - bi * wi
        ti = br * wi + bi * wr
        xr[..., i0], xi[..., i0] = ar + tr, ai + ti
        xr[..., i1], xi[..., i1] = ar - tr, ai - ti
        half <<= 1
    out = np.empty(x.shape, np.complex64)
    out.real, out.imag = xr, xi
    return out


def fft_mirror(g, tw=None):
    """(fft_tmp, spectrum) as the two kernels compute them: rows first, stored transposed [kx][row]; then the same
    transform along each of those rows: spectrum [kx][ky]"""
    tw = twiddles() if tw is None else tw
    tmp = np.ascontiguousarray(fft256_mirror(g.astype(np.complex64), tw).T)
    return tmp, fft256_mirror(tmp, tw)


def fft_float64(g):
    """(fft_tmp, spectrum) in float64, in the device's transposed layouts"""
    g64 = g.astype(np.float64)
    return np.fft.fft(g64, axis=1).T, np.fft.fft2(g64).T


def fft_yardstick(g):
    """the fp32 yardstick: scipy's complex64 transforms of the float32 image, same layouts"""
    import scipy.fft

    g32 = g.astype(np.float32)
    a, b = scipy.fft.fft(g32, axis=1).T, scipy.fft.fft2(g32).T
    assert a.dtype == np.complex64 and b.dtype == np.complex64
    return a, b


def fft_error(got, ref64):
    d = np.abs(got.astype(np.complex128) - ref64)
    return float(np.sqrt(np.mean(d * d))), float(d.max())


def fft_ratios(got, ref64, yard):
    """(rms ratio, max ratio) of got's error to the yardstick's; a zero yardstick error demands a zero error"""
    (r, m), (yr, ym) = fft_error(got, ref64), fft_error(yard, ref64)
    q = lambda a, b: 0.0 if a == 0 else (np.inf if b == 0 else a / b)
    return q(r, yr), q(m, ym)


def fft_meets_bar(got, ref64, yard):
    r, m = fft_ratios(got, ref64, yard)
    return r <= FFT_RMS_X and m <= FFT_MAX_X


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.complex64), np.ascontiguousarray(b, np.complex64)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def ulp32(x):
    """spacing of float32 at |x| (float64 in, float64 out)"""
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def logmag_ulps(got32, spec):
    """(error of got32, error of numpy's float32 log1p(hypot)) in float32 ulps of the float64 result, both maxima"""
    re, im = spec.real.astype(np.float64), spec.imag.astype(np.float64)
    ref = np.log1p(np.hypot(re, im))
    u = ulp32(np.maximum(ref, np.finfo(np.float32).tiny))
    yard = np.log1p(np.hypot(spec.real.astype(np.float32), spec.imag.astype(np.float32)))
    assert yard.dtype == np.float32
    return float((np.abs(got32.astype(np.float64) - ref) / u).max()), float((np.abs(yard.astype(np.float64) - ref) / u).max())


# ------------------------------------------------------------------------------------------------ hysteresis bitboard
def _fill_row(gen, pro):
    """Kogge-Stone occluded fill inside each 64-bit word, both directions (fill_row of the kernel)"""
    out = gen.copy()
    for shift in (np.left_shift, np.right_shift):
        g, p = gen.copy(), pro.copy()
        for k in (1, 2, 4, 8, 16, 32):
            k = np.uint64(k)
            g |= p & shift(g, k)
            p &= shift(p, k)
        out |= g
    return out


def hysteresis_bitboard(lab, carry=True):
    """canny_hyst_kernel restated on numpy uint64 words ([256][4], bit b of word w = column 64 w + b): sweeps of
    three-row OR, one-column dilation with the neighbour words' edge bits, AND with the weak set, then a fill along the
    row inside each word, until nothing changes.  carry = False is the mutant that drops the neighbour-word bits."""
    one = np.uint64(1)
    sh = np.arange(64, dtype=np.uint64)
    pack = lambda m: (m.reshape(FS, 4, 64).astype(np.uint64) << sh).sum(-1, dtype=np.uint64)
    s, w = pack(lab == 2), pack(lab == 0)
    allow = s | w
    zrow, zcol = np.zeros((1, 4), np.uint64), np.zeros((FS, 1), np.uint64)
    while True:
        v = s | np.concatenate([zrow, s[:-1]]) | np.concatenate([s[1:], zrow])
        dil = v | (v << one) | (v >> one)
        if carry:
            dil |= np.concatenate([zcol, v[:, :-1]], 1) >> np.uint64(63)
            dil |= np.concatenate([v[:, 1:], zcol], 1) << np.uint64(63)
        n = _fill_row(s | (w & dil), allow)
        if (n == s).all():
            break
        s = n
    return ((s[:, :, None] >> sh) & one).astype(np.uint8).reshape(FS, FS)


# ------------------------------------------------------------------------------------------------ inputs
def resized(frame):
    return I.resize_linear_u8(frame, FS, FS)


def fixture_frames():
    """the 8 frames of test_forensics_gpu.FRAMES at 256x256"""
    gen = {"determinism": F.determinism_frame, "noisy": F.noisy_image, "gradient": F.gradient_image,
           "smooth": F.smooth_image, "face_vga": F.face_frame, "blank": F.blank_frame,
           "natural_720p": F.natural_like, "face_1080p": lambda: F.face_frame(1920, 1080, 5)}
    return {k: resized(f()) for k, f in gen.items()}


def sobel_ramp():
    """gray plane with a vertical step at column 128 whose Sobel magnitude is exactly 50, 52, 150 and 152 in four bands
    of 64 rows (either side of `m > 50` and `m > 150`).  |dx| + |dy| of a 3x3 Sobel pair is always even - dx + dy =
    2 (f + l + k - a - d - b) in the kernel's names - so no image reaches 51 or 151; those come from the injected
    gradient fields (nms_fields).  Left of the step 0; right of it r or, alternating by row, r / r + 1: then
    dx = R(y-1) + 2 R(y) + R(y+1) = 4 r + 2 on every row and dy = 0."""
    g = np.zeros((FS, FS), np.uint8)
    odd = (np.arange(64) & 1).astype(np.uint8)[:, None]
    for band, (r, alt) in enumerate(((12, True), (13, False), (37, True), (38, False))):
        g[64 * band:64 * band + 64, 128:] = r + (odd if alt else 0)
    return g


def edge_frames():
    """BGR edge frames [256][256][3]"""
    out = {}
    out["all0"] = np.zeros((FS, FS, 3), np.uint8)
    out["all255"] = np.full((FS, FS, 3), 255, np.uint8)
    out["constant_colour"] = np.broadcast_to(np.array([37, 200, 91], np.uint8), (FS, FS, 3)).copy()
    prim = np.zeros((FS, FS, 3), np.uint8)
    cols = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (255, 255, 255), (0, 0, 0)]
    for i, c in enumerate(cols):
        prim[:, 32 * i:32 * i + 32] = c
    prim[128:] = prim[128:, ::-1]
    out["primaries"] = prim
    yy, xx = np.mgrid[0:FS, 0:FS]
    out["checkerboard"] = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    out["vstripes"] = np.repeat(((xx & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    out["hstripes"] = np.repeat(((yy & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    for name, (y, x) in {"px_tl": (0, 0), "px_tr": (0, 255), "px_bl": (255, 0), "px_br": (255, 255),
                         "px_127": (127, 127), "px_128": (128, 128)}.items():
        f = np.zeros((FS, FS, 3), np.uint8)
        f[y, x] = 255
        out[name] = f
    st = np.full((FS, FS, 3), 40, np.uint8)
    st[64:192, 64:192] = (210, 90, 160)                         # edges on 8x8 block borders
    out["step_aligned"] = st
    st = np.full((FS, FS, 3), 40, np.uint8)
    st[61:187, 67:197] = (210, 90, 160)                         # edges inside blocks, odd chroma phase
    out["step_misaligned"] = st
    # hues: 0 (v == r, g == b), 179 and the h < 0 wrap (v == r, g < b), across many saturations and values
    hue = np.zeros((FS, FS, 3), np.uint8)
    v = np.arange(FS)[None, :].repeat(FS, 0)
    d = np.minimum(np.arange(FS)[:, None], v)                   # diff <= v
    hue[..., 2] = v                                             # r = v
    hue[..., 1] = v - d                                         # g = min
    hue[..., 0] = v - d + (d * (xx % 7)) // 64                  # b slightly above g: small negative g - b
    out["hue_wrap"] = hue
    out["sobel_ramp"] = np.repeat(sobel_ramp()[..., None], 3, -1)
    return out


def gray_only_frames():
    """gray planes for injection that need no BGR frame (or are the gray of none of the frames above)"""
    rs = np.random.RandomState(77)
    out = {"gray_random": rs.randint(0, 256, (FS, FS)).astype(np.uint8), "gray_sobel_ramp_t": np.ascontiguousarray(sobel_ramp().T)}
    g = np.zeros((FS, FS), np.uint8)
    g[:, 128:] = 255
    g[128:] = 255 - g[128:]
    out["gray_max_sobel"] = g                                    # |dx| = 1020 along the step, |dy| = 1020 at the flip
    imp = np.zeros((FS, FS), np.uint8)
    imp[3, 200] = 255
    out["gray_impulse_off_origin"] = imp
    return out


def fft_inputs():
    """every gray plane the GPU stage test puts through the FFT kernels"""
    out = {k: gray(v) for k, v in {**fixture_frames(), **edge_frames()}.items()}
    out.update(gray_only_frames())
    return out


FFT_EXACT = ("smooth", "blank", "all0", "all255", "constant_colour", "px_tl", "checkerboard")


# label maps no image produces
def _blank():
    return np.ones((FS, FS), np.uint8)


def hysteresis_maps():
    m = {}
    for name, row, src in (("row_l2r", 100, 0), ("row_r2l", 101, 255)):          # (a)
        a = _blank(); a[row, :] = 0; a[row, src] = 2; m[name] = a
    a = _blank(); i = np.arange(FS); a[i, i] = 0; a[0, 0] = 2; m["diag_down"] = a          # (b)
    a = _blank(); a[i, i] = 0; a[255, 255] = 2; m["diag_up"] = a
    a = _blank(); a[i, 255 - i] = 0; a[0, 255] = 2; m["anti_down"] = a
    a = _blank(); a[i, 255 - i] = 0; a[255, 0] = 2; m["anti_up"] = a
    # (c) a one-pixel spiral with arms two apart, strong at the outer or the inner end; serpentines over the plane
    a = _blank(); y, x, dy, dx = 0, 0, 0, 1
    seen = np.zeros((FS + 4, FS + 4), bool); seen[:2] = seen[-2:] = True; seen[:, :2] = seen[:, -2:] = True
    blocked = lambda y, x, dy, dx: seen[y + dy + 2, x + dx + 2] or seen[y + 2 * dy + 2, x + 2 * dx + 2]
    path = []
    while True:
        path.append((y, x)); seen[y + 2, x + 2] = True
        if blocked(y, x, dy, dx):
            dy, dx = dx, -dy                                                      # turn right before touching an arm
            if blocked(y, x, dy, dx):
                break
        y, x = y + dy, x + dx
    for (py, px) in path:
        a[py, px] = 0
    a[0, 0] = 2; m["spiral_out_in"] = a
    b = a.copy(); b[0, 0] = 0; b[path[-1]] = 2; m["spiral_in_out"] = b
    a = _blank(); a[0::2, :] = 0; a[1::4, 255] = 0; a[3::4, 0] = 0; a[0, 0] = 2; m["serpentine_rows"] = a
    m["serpentine_columns"] = np.ascontiguousarray(a.T)                           # one row per sweep: ~32k sweeps
    # (d) weak pixel touching a strong one only across a word border, 8 directions, rows 0, 1, 254, 255
    for r in (0, 1, 254, 255):
        for border in (64, 128, 192):
            for k, (dy, dx) in enumerate([(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]):
                for side in (0, 1):                                               # strong left (col border-1) or right (col border) of the border
                    sx = border - 1 + side
                    wy, wx = r + dy, sx + dx
                    if not (0 <= wy < FS):
                        continue
                    a = _blank(); a[r, sx] = 2; a[wy, wx] = 0
                    # a second weak pixel one further step on, reachable only through the first
                    if 0 <= wy + dy < FS:
                        a[wy + dy, wx + dx] = 0
                    m[f"touch_r{r}_b{border}_d{k}_s{side}"] = a
    # (e) chains along the four borders; no wrap from column 255 of a row to column 0 of the next
    a = _blank(); a[0, :] = 0; a[255, :] = 0; a[:, 0] = 0; a[:, 255] = 0; a[0, 0] = 2; m["border_ring"] = a
    a = _blank(); a[10, 255] = 2; a[11, 0] = 0; a[10, 0] = 0; a[9, 0] = 0; m["no_wrap_right"] = a
    a = _blank(); a[10, 0] = 2; a[9, 255] = 0; a[10, 255] = 0; a[11, 255] = 0; m["no_wrap_left"] = a
    a = _blank(); a[0, 5] = 2; a[255, 4:7] = 0; m["no_wrap_top_bottom"] = a
    # (f)
    m["all_weak"] = np.zeros((FS, FS), np.uint8)
    m["all_strong"] = np.full((FS, FS), 2, np.uint8)
    m["all_none"] = _blank()
    return m


def random_maps(count=200, seed=5):
    """(g) label maps with per-map densities of strong / weak drawn log-uniformly"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        p_strong, p_weak = 10.0 ** rs.uniform(-4, -1), rs.uniform(0.05, 0.7)
        u = rs.rand(FS, FS)
        out.append(np.where(u < p_strong, 2, np.where(u < p_strong + p_weak, 0, 1)).astype(np.uint8))
    return out


# every branch of the reference that a pixel above `low` can take (at_tg22 / at_tg67, exact equality, cannot happen:
# 13573 is odd, so |dy| << 15 == |dx| * 13573 needs |dx| = 0 = |dy|; the fields sit one step of |dy| either side instead)
NMS_BRANCHES = ("horizontal", "vertical", "diagonal", "antidiagonal", "below_tg22", "above_tg22", "below_tg67",
                "above_tg67", "tie_left", "tie_right", "tie_up", "tie_down", "tie_diag_prev", "tie_diag_next", "border")


def nms_fields():
    """[k][256][256][2] int16 gradient fields for injection into the NMS kernel: random magnitudes over the whole
    Sobel range with runs of equal neighbours (ties), exact tg22 / tg67 boundary pairs, every sign combination, and
    content on the image border."""
    rs = np.random.RandomState(9)
    fields = []
    # 1: random (dx, dy) over the full range, repeated along rows / columns / diagonals in blocks so neighbours tie
    for rep in ((1, 1), (1, 3), (3, 1), (2, 2)):
        small = rs.randint(-1020, 1021, (FS // rep[0] + 1, FS // rep[1] + 1, 2))
        f = np.repeat(np.repeat(small, rep[0], 0), rep[1], 1)[:FS, :FS]
        fields.append(f)
    # 2: small magnitudes around the thresholds, few distinct values: dense ties in every direction class
    vals = np.array([-151, -150, -76, -51, -50, -26, -25, 0, 25, 26, 50, 51, 75, 76, 150, 151])
    fields.append(vals[rs.randint(0, len(vals), (FS, FS, 2))])
    diag = np.array([-80, -40, 40, 80])
    f = np.stack([diag[rs.randint(0, 4, (FS, FS))], diag[rs.randint(0, 4, (FS, FS))]], -1)   # |dx| == |dy| or 2:1 : diagonal class, ties
    fields.append(f)
    # 3: the class boundaries, one step of |dy| either side of tan 22.5 and tan 67.5 degrees for random |dx|
    f = np.zeros((FS, FS, 2), np.int64)
    ax = rs.randint(1, 1021, (FS, FS))
    lo22 = (ax * 13573) >> 15                                   # largest ay with ay << 15 < tg22
    side = rs.randint(0, 2, (FS, FS))
    ay22 = np.minimum(lo22 + side, 1020)
    ay67 = np.minimum(((ax * 13573 + (ax << 16)) >> 15) + side, 1020)
    which = rs.randint(0, 2, (FS, FS))
    f[..., 0] = ax * rs.choice([-1, 1], (FS, FS))
    f[..., 1] = np.where(which == 0, ay22, ay67) * rs.choice([-1, 1], (FS, FS))
    fields.append(f)
    # 4: ax == 0 columns / ay == 0 rows (tg22 == tg67 == 0: `ay < tg22` false, `ay > tg67` true unless ay == 0)
    f = rs.randint(-1020, 1021, (FS, FS, 2))
    f[:, ::3, 0] = 0
    f[::5, :, 1] = 0
    f[::15, ::3] = (0, 0)
    fields.append(f)
    return np.stack(fields).astype(np.int16)
