"""The train-time augmentation kernels (csrc/train_augment.hip) against tests/train_augment_oracle.py, stage by stage
through `dfd_train_augment_tap`: every uint8 stage, `norm` and `erase` bit-equal; `noise` and `mix` at the project's
float bar (b0_layer_oracle's RMS_FACTOR x / MAX_FACTOR x the error of the same formula in numpy float32, against the
float64 oracle; `head_train_oracle.bar_ratio`: <= 1 passes), every figure printed before it is asserted.  Then the
whole chain at 224, `train_augment_features` against `extract_features(train_augment(...))`, `fit_head(augment=...)`
against `fit_loop` driven by hand, and the argument errors.

The hash words behind the noise: the functions the kernel calls are held to `noise_words` bit for bit on the host
(test_train_augment_oracle.py, through `dfd_train_augment_noise_words`); here the kernel's use of them - key, element
index, the 24 bits taken - is held through z at the float bar.
"""
import numpy as np
import pytest

import head_train_oracle as HO
import train_augment_oracle as O
from rtdfd_amd import head_training as HT
from rtdfd_amd import train_augment as TA

pytestmark = pytest.mark.gpu

U8_STAGES = ("crop", "jitter0", "jitter1", "jitter2", "jitter3", "gray", "rotate", "affine", "perspective", "blur")
STAGE_FLAG = {"gray": TA.F_GRAY, "rotate": TA.F_ROTATE, "affine": TA.F_AFFINE, "perspective": TA.F_PERSPECTIVE, "blur": TA.F_BLUR}
ALL_ON = dict(jpeg_p=1.0, flip_p=1.0, gray_p=1.0, perspective_p=1.0, blur_p=1.0, erase_p=1.0, noise_p=1.0)


def _sources(n, h, w, seed):
    a = np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    a[:, :4] = a[:, :4, :, :1]                    # gray rows: the s == 0 / max == min branches of the hue stage
    return a


def _tables(n, h, w, t, seed, mix=None):
    """image 0: every stage on; image 1: every stage off (Resize(T) alone); the rest as the reference policy draws them.
    Images 0, 2, 3, 4 run the four jitter ops in the four rotations of their order: every op in every slot."""
    rng = np.random.RandomState(seed)
    on, _ = TA.draw_batch(TA.AugmentPolicy(**ALL_ON), rng, n, h, w, t)
    rows, batch = TA.draw_batch(TA.AugmentPolicy(), rng, n, h, w, t, mix=mix)
    off, _ = TA.draw_batch(TA.AugmentPolicy.validation(), rng, n, h, w, t)
    rows[0] = on[0]
    rows[0]["flags"] |= TA.F_ERASE                # a box that fits is not certain at this size: set one
    rows[0]["erase"] = (3, 5, 7, 11)
    rows[0]["noise_std"] = 0.04
    if n > 2:
        rows[2]["flags"] |= TA.F_JPEG | TA.F_JPEG_RGB     # the round trip without the reference's channel reversal
        rows[2]["jpeg_quality"] = 1 + (seed * 37) % 100
    if n > 1:
        rows[1] = off[1]
    for k, i in enumerate([i for i in (0, 2, 3, 4) if i < n]):
        factor = {int(op): f for op, f in zip(rows[i]["jitter_op"], rows[i]["jitter_factor"])}
        order = np.roll(np.arange(1, 5), k)
        rows[i]["jitter_op"] = order
        rows[i]["jitter_factor"] = [factor[int(op)] for op in order]
    return rows, batch


def _check_u8(h, rgb, rows, batch, t, want):
    n = rgb.shape[0]
    got = h.train_augment_tap(rgb, rows, batch, "jpeg", t)
    for i in range(n):
        assert np.array_equal(got[i], want["jpeg"][i]), ("jpeg", i)
        if not rows[i]["flags"] & TA.F_JPEG:
            assert np.array_equal(got[i], rgb[i]), ("jpeg", i, "a skipped stage changed the image")
    got = h.train_augment_tap(rgb, rows, batch, "resize", t)
    for i in range(n):
        s = want["resize"][i].shape[0]
        assert np.array_equal(got[i].reshape(-1)[:s * s * 3].reshape(s, s, 3), want["resize"][i]), ("resize", i)
    prev = None
    for name in U8_STAGES:
        got = h.train_augment_tap(rgb, rows, batch, name, t)
        for i in range(n):
            assert np.array_equal(got[i], want[name][i]), (name, i)
            skipped = (name in STAGE_FLAG and not rows[i]["flags"] & STAGE_FLAG[name]) or \
                (name.startswith("jitter") and rows[i]["jitter_op"][int(name[-1])] == TA.JITTER_NONE)
            if skipped:
                assert np.array_equal(got[i], prev[i]), (name, i, "a skipped stage changed the image")
        prev = got
    return prev


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("t", [32, 40])
@pytest.mark.parametrize("hw", [(32, 48), (48, 32)])
def test_stages_bit_equal(b0_handle, hw, t, n):
    rgb = _sources(n, hw[0], hw[1], 10 * n + t)
    rows, batch = _tables(n, hw[0], hw[1], t, 3 * n + t + hw[0])
    if n == 5:
        assert all(set(rows[i]["jitter_op"][k] for i in (0, 2, 3, 4)) == {1, 2, 3, 4} for k in range(4))
    want = O.chain(rgb, rows, batch, t)
    _check_u8(b0_handle, rgb, rows, batch, t, want)
    norm = b0_handle.train_augment_tap(rgb, rows, batch, "norm", t)
    erase = b0_handle.train_augment_tap(rgb, rows, batch, "erase", t)
    assert np.array_equal(norm, want["norm"]) and np.array_equal(erase, want["erase"])
    for i in range(n):
        if not rows[i]["flags"] & TA.F_ERASE:
            assert np.array_equal(erase[i], norm[i])
    noise = b0_handle.train_augment_tap(rgb, rows, batch, "noise", t)
    for i in range(n):
        if not rows[i]["flags"] & TA.F_NOISE:
            assert np.array_equal(noise[i], erase[i])
    assert np.array_equal(b0_handle.train_augment_tap(rgb, rows, batch, "mix", t), noise)      # no mix: a copy
    assert np.array_equal(b0_handle.train_augment(rgb, rows, batch, t), noise)


def _noise_case(t=40, n=4):
    """sources in the band where every channel's normalised value lies in (0, 1) (126..160: 0.04 .. 0.99), so that the
    clamp leaves most elements free; inputs and seed are fixed here, by the oracle alone (the excluded share is asserted)"""
    rgb = np.random.RandomState(77).randint(126, 161, (n, 32, 48, 3)).astype(np.uint8)
    rows, batch = TA.draw_batch(TA.AugmentPolicy.validation(), np.random.RandomState(1), n, 32, 48, t)
    rows["flags"] |= TA.F_NOISE
    rows["noise_std"] = [0.01, 0.04, 0.2, 0.5][:n]
    return rgb, rows, batch


def _clamp_report(name, got, ref64_unclamped, ref64, yard32):
    r = HO.bar_ratio(got, ref64, yard32)
    bar = (HO.B.MAX_FACTOR * r["yard_max"] + HO.B.MAX_FLOOR) * float(np.abs(ref64).max())
    near = (np.abs(ref64_unclamped) < bar) | (np.abs(ref64_unclamped - 1.0) < bar)
    print(f"{name}: ratio {r['ratio']:.3f} rms {r['rms']:.3e} (yard {r['yard_rms']:.3e}) max {r['max']:.3e} (yard {r['yard_max']:.3e}); "
          f"excluded from the clamp check {near.mean() * 100:.4f} % (|u| or |u - 1| < {bar:.3e})")
    return r, near


def test_noise_and_mixup_at_the_float_bar(b0_handle):
    t = 40
    rgb, rows, batch = _noise_case(t)
    n = rgb.shape[0]
    batch["mix_kind"], batch["lam"] = TA.MIX_MIXUP, 0.7
    batch.partners = np.array([2, 3, 1, 0], np.int32)
    w64, w32 = O.chain(rgb, rows, batch, t, np.float64), O.chain(rgb, rows, batch, t, np.float32)
    un = np.stack([w64["erase"][i].astype(np.float64) + float(rows[i]["noise_std"]) *
                   TA.noise_normal(int(batch["seed"]), 0, i, w64["erase"][i].size).reshape(w64["erase"][i].shape) for i in range(n)])
    free = float(np.mean((w64["noise"] > 0) & (w64["noise"] < 1)))
    print(f"elements the clamp leaves free: {free * 100:.1f} %")
    assert free > 0.5
    got = b0_handle.train_augment_tap(rgb, rows, batch, "noise", t)
    r, near = _clamp_report("noise", got, un, w64["noise"], w32["noise"])
    assert near.mean() < 0.01
    assert r["ratio"] <= 1.0
    ok = ~near
    assert np.array_equal((got == 0.0)[ok], (w64["noise"] == 0.0)[ok]) and np.array_equal((got == 1.0)[ok], (w64["noise"] == 1.0)[ok])
    mixed = b0_handle.train_augment_tap(rgb, rows, batch, "mix", t)
    rm = HO.bar_ratio(mixed, w64["mix"], w32["mix"])
    print(f"mix (Mixup): ratio {rm['ratio']:.3f} rms {rm['rms']:.3e} (yard {rm['yard_rms']:.3e}) max {rm['max']:.3e} (yard {rm['yard_max']:.3e})")
    assert rm["ratio"] <= 1.0
    assert np.array_equal(b0_handle.train_augment(rgb, rows, batch, t), mixed)
    # Mixup of the device's own noise output: bit-equal to the float32 formula
    lam = np.float32(batch["lam"])
    assert np.array_equal(mixed, lam * got + (np.float32(1) - lam) * got[batch.partners])


def test_cutmix_copies_the_box(b0_handle):
    t = 32
    rgb = _sources(3, 48, 32, 5)
    box, lam = TA.cutmix_box(0.6, 14, 30, t)
    rows, batch = _tables(3, 48, 32, t, 21, mix=(TA.MIX_CUTMIX, lam, np.array([1, 2, 0]), box))
    base = b0_handle.train_augment_tap(rgb, rows, batch, "noise", t)
    want = base.copy()
    x1, y1, x2, y2 = box
    assert x2 == t and x1 > 0 and y1 > 0                      # a box clipped at the right edge
    want[:, :, y1:y2, x1:x2] = base[[1, 2, 0]][:, :, y1:y2, x1:x2]
    assert np.array_equal(b0_handle.train_augment_tap(rgb, rows, batch, "mix", t), want)
    assert np.array_equal(b0_handle.train_augment(rgb, rows, batch, t), want)


def test_whole_chain_at_224(b0_handle):
    rgb = _sources(3, 224, 224, 31)
    rows, batch = TA.draw_batch(TA.AugmentPolicy(**ALL_ON), np.random.RandomState(12), 3, 224, 224, 224)
    assert all(int(f) & (TA.F_JPEG | TA.F_CROP | TA.F_FLIP | TA.F_GRAY | TA.F_ROTATE | TA.F_AFFINE | TA.F_PERSPECTIVE | TA.F_BLUR | TA.F_NOISE) ==
               (TA.F_JPEG | TA.F_CROP | TA.F_FLIP | TA.F_GRAY | TA.F_ROTATE | TA.F_AFFINE | TA.F_PERSPECTIVE | TA.F_BLUR | TA.F_NOISE) for f in rows["flags"])
    assert (rows["flags"] & TA.F_ERASE).any()
    rows["flags"][2] &= ~np.uint32(TA.F_GRAY)                     # one image keeps its colours through the warps
    want = O.chain(rgb, rows, batch, 224)
    _check_u8(b0_handle, rgb, rows, batch, 224, want)
    assert np.array_equal(b0_handle.train_augment_tap(rgb, rows, batch, "norm", 224), want["norm"])
    assert np.array_equal(b0_handle.train_augment_tap(rgb, rows, batch, "erase", 224), want["erase"])


# ------------------------------------------------------------------------------------------------ features
@pytest.fixture(scope="module")
def h2(pkg, seeded_sd):
    h = pkg._lib.Handle(pkg.weights.pack_b0(seeded_sd), device=0, max_batch=2)
    yield h
    h.close()


class _ByHand:
    """train_augment + extract_features in chunks of max_batch: what train_augment_features fuses"""

    def __init__(self, h):
        self.h = h

    def train_augment_features(self, rgb, rows, batch, shape=None):
        x = self.h.train_augment(rgb, rows, batch, 224)
        return np.concatenate([self.h.extract_features(x[i:i + self.h.max_batch]) for i in range(0, x.shape[0], self.h.max_batch)])


def test_features_equal_augment_then_extract(h2):
    rgb = _sources(5, 64, 96, 8)
    rng = np.random.RandomState(6)
    rows, batch = TA.draw_batch(TA.AugmentPolicy(), rng, 5, 64, 96, 224, mix=(TA.MIX_MIXUP, 0.8, np.array([4, 3, 0, 1, 2])))
    want = _ByHand(h2).train_augment_features(rgb, rows, batch)
    got = h2.train_augment_features(rgb, rows, batch)
    assert got.shape == (5, 1280) and np.array_equal(got, want)
    buf = h2.alloc(rgb.nbytes).upload(rgb)
    try:
        assert np.array_equal(h2.train_augment_features(buf, rows, batch, shape=rgb.shape[:3]), want)
    finally:
        buf.free()
    box, lam = TA.cutmix_box(0.5, 100, 120, 224)
    rows, batch = TA.draw_batch(TA.AugmentPolicy(), rng, 5, 64, 96, 224, mix=(TA.MIX_CUTMIX, lam, np.array([1, 2, 3, 4, 0]), box))
    assert np.array_equal(h2.train_augment_features(rgb, rows, batch), _ByHand(h2).train_augment_features(rgb, rows, batch))


def test_features_leave_an_open_trainer_alone(pkg, h2, seeded_sd):
    rgb = _sources(3, 32, 32, 2)
    rows, batch = TA.draw_batch(TA.AugmentPolicy(), np.random.RandomState(3), 3, 32, 32, 224)
    f = np.random.RandomState(4).randn(8, 1280).astype(np.float32)
    y = (np.arange(8) % 2).astype(np.float32)
    with HT.HeadTrainer(h2, seeded_sd, max_n=8, seed=5) as tr:
        loss1, z1 = tr.accumulate(f, y)
    with HT.HeadTrainer(h2, seeded_sd, max_n=8, seed=5) as tr:
        feats = h2.train_augment_features(rgb, rows, batch)
        loss2, z2 = tr.accumulate(f, y)
        again = h2.train_augment_features(rgb, rows, batch)
    assert loss1 == loss2 and np.array_equal(z1, z2) and np.array_equal(feats, again)


def test_fit_loop_on_resident_crops(pkg, h2, seeded_sd):
    """a training set kept in HBM (ResidentCrops: device gather of every shuffled batch) gives the host array's log"""
    rs = np.random.RandomState(21)
    crops = rs.randint(0, 256, (7, 48, 32, 3)).astype(np.uint8)
    y = (np.arange(7) % 2).astype(np.float32)
    kw = dict(epochs=2, batch_size=3, grad_accum=2, lr=1e-3, mix_alpha=0.4, cutmix_alpha=0.3)
    logs = []
    with TA.ResidentCrops(h2, crops) as res, TA.ResidentCrops(h2, crops[:3]) as vres:
        buf, shape = res.gather([6, 0, 6, 3])
        assert shape == (4, 48, 32) and np.array_equal(buf.download((4, 48, 32, 3), np.uint8), crops[[6, 0, 6, 3]])
        for idx in ([7], [-1], []):
            with pytest.raises(pkg._lib.DfdError) as e:
                res.gather(idx)
            assert e.value.code == -1
        for x, v in ((crops, crops[:3]), (res, vres)):
            with HT.HeadTrainer(h2, seeded_sd, max_n=3, seed=2) as tr:
                logs.append(tr.fit(x, y, val=(v, y[:3]), rng=np.random.RandomState(5), augment=(h2, TA.AugmentPolicy()), **kw))
    strip = lambda lg: [{k: v for k, v in e.items() if k != "time_seconds"} for e in lg]
    print(strip(logs[1]))
    assert len(logs[0]) == 2 and strip(logs[0]) == strip(logs[1])


def test_fit_head_with_augment(pkg):
    rs = np.random.RandomState(14)
    crops = rs.randint(0, 256, (8, 32, 32, 3)).astype(np.uint8)
    crops[::2] //= 3                                              # two brightness clusters
    y = (np.arange(8) % 2).astype(np.float32)
    policy = TA.AugmentPolicy()
    kw = dict(batch_size=4, grad_accum=2, lr=1e-3, mix_alpha=0.4, cutmix_alpha=0.3)
    held_out = (np.random.RandomState(15).randn(1, 3, 224, 224) * 0.8).astype(np.float32)
    m = pkg.model.DeepfakeEfficientNet(pretrained=False, max_batch=2, seed=0)
    by_hand = pkg.model.DeepfakeEfficientNet(pretrained=False, max_batch=2, seed=0)
    try:
        before = m(held_out).copy()
        log = m.fit_head(crops, y, epochs=2, augment=policy, val=(crops[:4], y[:4]), rng=np.random.RandomState(3),
                         trainer_config={"ema_decay": 0.5}, **kw)
        with HT.HeadTrainer(by_hand, max_n=4, ema_decay=0.5) as tr:
            want = HT.fit_loop(tr, crops, y, 2, val=(crops[:4], y[:4]), rng=np.random.RandomState(3),
                               augment=(_ByHand(by_hand.handle), policy), **kw)
        strip = lambda lg: [{k: v for k, v in e.items() if k != "time_seconds"} for e in lg]
        print(strip(log))
        assert len(log) == 2 and strip(log) == strip(want)
        after = m(held_out)
        assert not np.array_equal(after, before)
        fresh = pkg._lib.Handle(pkg.weights.pack_b0(m.state_dict()), device=0, max_batch=2)
        try:
            assert np.array_equal(fresh.classify(held_out), after)
        finally:
            fresh.close()
    finally:
        m.handle.close()
        by_hand.handle.close()


# ------------------------------------------------------------------------------------------------ errors
def test_argument_errors(pkg, b0_handle):
    E = pkg._lib.DfdError
    t = 32
    rgb = _sources(3, 32, 48, 1)
    rows, batch = _tables(3, 32, 48, t, 4)
    good = b0_handle.train_augment(rgb, rows, batch, t)

    def refused(code, rgb_=rgb, rows_=rows, batch_=batch, t_=t, call=None):
        with pytest.raises(E) as e:
            (call or b0_handle.train_augment)(rgb_, rows_, batch_, t_)
        assert e.value.code == code, str(e.value)
        assert np.array_equal(b0_handle.train_augment(rgb, rows, batch, t), good)          # a valid call still gives the same bits

    refused(-1, rgb_=_sources(3, 40, 48, 1))                       # not a multiple of 16
    refused(-1, rgb_=_sources(3, 16, 48, 1))                       # below 32
    refused(-1, rgb_=np.zeros((3, 528, 32, 3), np.uint8))          # above 512
    refused(-1, t_=8)                                              # out_size + 20 below what the chain resizes to
    refused(-1, t_=500)
    refused(-1, rgb_=rgb[:0], rows_=rows[:0])                      # n < 1
    bad = rows.copy()
    bad[1]["jitter_op"][2] = 7
    refused(-1, rows_=bad)
    bad = rows.copy()
    bad[0]["erase"] = (30, 0, 7, 5)
    refused(-1, rows_=bad)
    for box in ((3, 5, 2 ** 31 - 1, 5), (3, 5, 7, 2 ** 31 - 3), (2 ** 31 - 4, 0, 16, 5)):    # sums that would wrap in int
        bad[0]["erase"] = box
        refused(-1, rows_=bad)
    bad = rows.copy()
    bad[2]["flags"] |= TA.F_CROP
    bad[2]["crop_x"] = 21
    refused(-1, rows_=bad)
    bad = rows.copy()
    bad[2]["flags"] |= TA.F_JPEG
    bad[2]["jpeg_quality"] = 0
    refused(-1, rows_=bad)                                         # quality outside 1..100
    bad[2]["jpeg_quality"] = 101
    refused(-1, rows_=bad)
    mixed = batch.copy()
    mixed["mix_kind"], mixed["lam"] = TA.MIX_MIXUP, 0.7
    mixed.partners = np.array([0, 3, 1], np.int32)
    refused(-1, batch_=mixed)                                      # a partner out of range
    mixed.partners = None
    refused(-1, batch_=mixed)                                      # mix without partners
    with pytest.raises(E) as e:
        b0_handle.train_augment_tap(rgb, rows, batch, "sharpen", t)
    assert e.value.code == -1
    with pytest.raises(E) as e:
        b0_handle.train_augment_features(rgb[:0], rows[:0], batch)
    assert e.value.code == -1
    assert np.array_equal(b0_handle.train_augment(rgb, rows, batch, t), good)
