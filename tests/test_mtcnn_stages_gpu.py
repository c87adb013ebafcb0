"""GPU: every buffer the MTCNN cascade materialises (dfd_mtcnn_tap / _tap_batch / _net_tap) against the per-kernel
references of tests/mtcnn_stage_oracle.py, teacher-forced: each launch is compared from the HIP path's own input tap.

Bars (none invented here):
  * bit-exact: the area-resized pyramid ("pnet.in.<level>") and window inputs ("rnet.in" / "onet.in") against exact
    integer window sums + the float32 mirror of the normalisation; the ceil-mode max-pools ("rnet.pool2", "onet.pool2",
    "onet.pool3") from their input taps; the zero pad channels of the GEMM layouts; the candidate records against the
    maps (cells, p, r[4]); every tap of a crop in a ragged batch against the same crop run alone; every tap after a
    large call against a fresh handle.
  * floating launches (conv1 + PReLU + pool, conv + PReLU, dense + PReLU, heads + softmax, landmark head): the
    classifier suite's rule - rms(d) / rms(ref) <= 4 x the torch-fp32-on-CPU yardstick's + 2^-23 and max |d| / u <= 8 x
    the yardstick's + 2^-21, u = the op evaluated on magnitudes (mtcnn_stage_oracle.scale).
  * zero threshold flips: the float64 reference probability of every cell / window lies on the side of its threshold the
    HIP value lies on (tests/test_mtcnn_stage_oracle.py verifies on the CPU that no input is within 1e-4 of one).

Not reachable, by the code: a P-Net grid of 1 x 1 (a level exists while min(h, w) * scale >= 12 and its edge is
int(that + 1) >= 13, so the smallest grid is 2 x 2 - tested on the 20 px crops); candidates beyond `cand_cap` (the
capacity is the cell count, every cell appends at most once).  P-Net takes no injected input: its ragged launches take
their geometry from the image sizes, so shapes are reached through image sizes (mtcnn_stage_oracle.EDGE_CASES).

Measured on an MI355X, worst HIP error / torch-fp32 yardstick error per tap over every case of this file (1,318 launch
comparisons; the bar allows 4 rms / 8 max; the worst error / bar of any comparison is 0.52):
  pnet.pool1 0.84  pnet.conv2 0.90 (VALU path 1.09)  pnet.prob 1.36 (VALU 1.62)  pnet.reg 1.12 (VALU 1.15)
  rnet.pool1 0.89  rnet.conv2 1.24  rnet.conv3 1.32  rnet.dense4 1.93  rnet.prob 0.66  rnet.reg 0.93
  onet.pool1 0.84  onet.conv2 1.18  onet.conv3 1.70  onet.conv4 1.66  onet.dense5 2.29  onet.prob 0.77  onet.reg 0.99
  onet.pts 0.92
Every bit-exact comparison holds (pyramid, window resize, pools, pad channels, candidates, batch = alone, stale scratch).
Candidates: 700 x 900 dense 1,451 (no overflow), 2000 x 2400 dense 12,429 (overflow flag raised, host path identical).
Run time: 14 s for the file (26 tests), of which 6 s are the two child processes of the P-Net path test.
kernel bugs found: none.  (One stale claim found: the 700 x 900 case of tests/test_mtcnn_gpu.py was documented as
exceeding the device block's capacity; it has 1,451 candidates and never did.)
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import mtcnn_ref as M
from tests import mtcnn_stage_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}                       # tap -> worst HIP / yardstick ratio seen
THR = [np.float32(t) for t in M.THRESHOLDS]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("MEASURED worst HIP / yardstick ratio per tap:", {k: round(v, 2) for k, v in sorted(REPORT.items())})


def _bgr(rgb):
    return np.ascontiguousarray(rgb[..., ::-1])


def _sds(pkg, sd):
    t32 = pkg.weights.to_torch(sd)
    return t32, {k: v.double() for k, v in t32.items()}


@pytest.fixture(scope="module")
def dense(pkg, mt_handle, mtcnn_sd):
    return (mt_handle,) + _sds(pkg, mtcnn_sd)


@pytest.fixture(scope="module")
def selective(pkg, seeded_sd):
    W = pkg.weights
    sel = W.seeded_mtcnn_state_dict(0, W.MTCNN_SELECTIVE)
    h = pkg._lib.Handle(W.pack_all(seeded_sd, W.seeded_ssd_state_dict(0), sel), device=0, max_batch=16)
    yield (h,) + _sds(pkg, sel)
    h.close()


def _floating(name, got, get64, get32, sd64, sd32, where):
    """one floating launch against its bar; got: HIP outputs (float64 NCHW, real channels)"""
    for r in O.check(name, got, get64, get32, sd64, sd32):
        print(f"{where} {r['tap']}: rms {r['rms']:.3e} max/u {r['max']:.3e} yard rms {r['yard']['rms']:.3e} max/u {r['yard']['max']:.3e} "
              f"ratio {r['ratio']:.3f} vs_yard {r['vs_yard']:.2f}")
        REPORT[r["tap"]] = max(REPORT.get(r["tap"], 0.0), r["vs_yard"])
        assert r["ratio"] <= 1.0, (where, r)


def _getters(taps):
    """taps: name -> numpy device tap (n, h, w, c) -> getters of float64 / float32 NCHW tensors"""
    return (lambda k: O.to_nchw(taps[k], torch.float64)), (lambda k: O.to_nchw(taps[k], torch.float32))


def _net_taps(net, fetch, n):
    """every tap of R-Net / O-Net through fetch(name) -> {name: (n, edge, edge, c)}, prob (n,), reg (n, 4), pts (n, 10)"""
    taps = {}
    for name, (edge, ch) in O.NET_SHAPES.items():
        if name.startswith(net):
            t = np.asarray(fetch(name))
            assert t.size == n * edge * edge * ch, (name, t.shape, n)
            taps[name] = t.reshape(n, edge, edge, ch)
    taps[net + ".prob"] = np.asarray(fetch(net + ".prob")).reshape(n)
    taps[net + ".reg"] = np.asarray(fetch(net + ".reg")).reshape(n, 4)
    if net == "onet":
        taps["onet.pts"] = np.asarray(fetch("onet.pts")).reshape(n, 10)
    return taps


def _check_net(net, taps, sd32, sd64, where, want_in=None, stage_thr=None):
    """all launches of one R-/O-Net call from its taps"""
    n = len(taps[net + ".prob"])
    if want_in is not None:
        assert taps[net + ".in"].shape == want_in.shape, (where, taps[net + ".in"].shape, want_in.shape)
        assert np.array_equal(taps[net + ".in"], want_in), f"{where} {net}.in: {(taps[net + '.in'] != want_in).sum()} values differ"
    get64, get32 = _getters(taps)
    for name in (O.RNET_ORDER if net == "rnet" else O.ONET_ORDER):
        if name in O.POOLS:
            src, k, s = O.POOLS[name]
            want = O.maxpool(get32(src), k, s).permute(0, 2, 3, 1).numpy()
            assert np.array_equal(taps[name], want), (where, name)
            continue
        if name.endswith(".out"):
            got = (torch.from_numpy(taps[net + ".prob"]).double(), torch.from_numpy(taps[net + ".reg"]).double())
        elif name == "onet.pts":
            got = torch.from_numpy(taps[name]).double()
        else:
            real = O.REAL.get(name, taps[name].shape[-1])
            assert not taps[name][..., real:].any(), (where, name, "pad channels must be exactly zero")
            got = get64(name)[:, :real]
            if got.shape[2:] == (1, 1):
                got = got.flatten(1)
        _floating(name, got, get64, get32, sd64, sd32, where)
    for name, real in O.REAL.items():
        if name.startswith(net):
            assert not taps[name][..., real:].any(), (where, name)
    if stage_thr is not None and n:
        ref = O.layer(net + ".out", get64, sd64)[0].numpy()
        flips = (ref > np.float64(stage_thr)) != (taps[net + ".prob"] > stage_thr)
        assert not flips.any(), (where, net, int(flips.sum()))
    return n


def _check_crop(handle, sd32, sd64, rgbs, crop, where, alone=False, before=None):
    """every tap of image `crop` of one ragged call over `rgbs` -> {name: tap} (for comparisons between calls);
    before(): run ahead of every tap call"""
    bgrs = [_bgr(r) for r in rgbs]
    rgb = rgbs[crop]
    h, w = rgb.shape[:2]

    def tap(name):
        if before:
            before()
        return handle.mtcnn_tap_batch(bgrs, crop, name)
    out = {}
    for k, (sc, sh, sw, ph, pw, oh, ow) in enumerate(O.levels(h, w)):
        t = {"pnet.in": tap(f"pnet.in.{k}"), "pnet.pool1": tap(f"pnet.pool1.{k}"), "pnet.conv2": tap(f"pnet.conv2.{k}"),
             "pnet.prob": tap(f"pnet.prob.{k}"), "pnet.reg": tap(f"pnet.reg.{k}")}
        assert t["pnet.in"].shape == (sh, sw, 3) and t["pnet.pool1"].shape == (ph, pw, 10), (where, k)
        assert t["pnet.conv2"].shape == (ph - 2, pw - 2, 16) and t["pnet.prob"].size == oh * ow, (where, k)
        want = O.area_resize(rgb, sh, sw)
        assert np.array_equal(t["pnet.in"], want), f"{where} pnet.in.{k}: {(t['pnet.in'] != want).sum()} values differ"
        t["pnet.prob"] = t["pnet.prob"].reshape(oh, ow)
        t["pnet.reg"] = t["pnet.reg"].reshape(oh, ow, 4)
        get64, get32 = _getters({n: v[None] for n, v in t.items() if v.ndim == 3})
        _floating("pnet.pool1", get64("pnet.pool1"), get64, get32, sd64, sd32, f"{where} L{k}")
        _floating("pnet.conv2", get64("pnet.conv2"), get64, get32, sd64, sd32, f"{where} L{k}")
        got = (torch.from_numpy(t["pnet.prob"]).double()[None], get64("pnet.reg"))
        _floating("pnet.out", got, get64, get32, sd64, sd32, f"{where} L{k}")
        ref = O.layer("pnet.out", get64, sd64)[0][0].numpy()
        flips = (ref >= np.float64(THR[0])) != (t["pnet.prob"] >= THR[0])
        assert not flips.any(), (where, k, int(flips.sum()))
        for n, v in t.items():
            out[f"{n}.{k}"] = v
    if not O.levels(h, w):
        return out
    for st in ("stage1", "stage2", "stage3"):
        out[st] = tap(st)
    for net, rows, size, thr in (("rnet", out["stage1"], 24, THR[1]), ("onet", out["stage2"], 48, THR[2])):
        wins = O.windows_of(rows[:, :4], h, w) if len(rows) else []
        first = tap(net + ".prob")
        assert first.size == len(wins), (where, net, first.size, len(wins))
        if not wins:
            continue
        taps = _net_taps(net, tap, len(wins))
        _check_net(net, taps, sd32, sd64, where, O.window_inputs(rgb, wins, size), thr)
        out.update(taps)
        out[net + ".windows"] = np.asarray(wins, np.int32)
    if alone:
        single = _check_crop(handle, sd32, sd64, [rgb], 0, where + " alone")
        assert sorted(single) == sorted(out), where
        for n in out:
            assert np.array_equal(out[n], single[n]), f"{where}: tap {n} of the crop in the batch differs from the crop run alone"
    return out


def _check_candidates(handle, rgbs, maps, where):
    """the candidate records of a call against the prob / reg maps of all its crops, bit for bit"""
    rec, count = handle.mtcnn_tap_batch([_bgr(r) for r in rgbs], 0, "pnet.cand")
    assert count == len(rec), (where, count, len(rec))
    cells = rec[:, 0].copy().view(np.uint32).astype(np.int64)
    prob, reg = [], []
    for c, rgb in enumerate(rgbs):
        for k in range(len(O.levels(*rgb.shape[:2]))):
            prob.append(maps[c][f"pnet.prob.{k}"].reshape(-1))
            reg.append(maps[c][f"pnet.reg.{k}"].reshape(-1, 4))
    if not prob:
        assert len(rec) == 0
        return 0
    prob, reg = np.concatenate(prob), np.concatenate(reg)
    want = np.nonzero(prob >= THR[0])[0]
    assert np.array_equal(np.sort(cells), want), (where, len(cells), len(want))           # the multiset: no cell twice, none lost
    assert np.array_equal(rec[:, 1].view(np.uint32), prob[cells].view(np.uint32)), where
    assert np.array_equal(rec[:, 2:].view(np.uint32), reg[cells].view(np.uint32)), where
    return len(rec)


# ------------------------------------------------------------------------------------------------ single images
@pytest.mark.parametrize("case", O.SINGLE_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_single_image_every_tap(dense, case):
    handle, sd32, sd64 = dense
    rgb = O.image(case)
    taps = _check_crop(handle, sd32, sd64, [rgb], 0, f"{case[0]}x{case[1]}")
    if min(case[:2]) < 20:
        assert not taps and handle.mtcnn_align(_bgr(rgb)) == (None, None)
        return
    _check_candidates(handle, [rgb], [taps], str(case))
    # the one-image entry reads the same buffers
    assert np.array_equal(handle.mtcnn_tap(_bgr(rgb), "pnet.prob.0"), taps["pnet.prob.0"])
    assert np.array_equal(handle.mtcnn_tap(_bgr(rgb), "stage1"), taps["stage1"])


# ------------------------------------------------------------------------------------------------ ragged batches
def test_ragged_batch_of_five_crops(dense):
    """5 crops of different sizes in one ragged call: every tap of every crop against the oracle AND bit-identical to the
    same crop run alone; the candidate list of the whole call against all maps"""
    handle, sd32, sd64 = dense
    rgbs = [O.image(c) for c in O.BATCH5]
    maps = [_check_crop(handle, sd32, sd64, rgbs, c, f"batch5[{c}]", alone=True) for c in range(len(rgbs))]
    assert sum("rnet.prob" in m for m in maps) >= 3 and sum("onet.prob" in m for m in maps) >= 1     # the two smallest crops end at P-Net
    assert _check_candidates(handle, rgbs, maps, "batch5") > 100
    wins = np.concatenate([m["rnet.windows"] for m in maps if "rnet.windows" in m])
    assert (wins[:, 0] == 0).any() and (wins[:, 1] == 0).any(), "no window clipped at the left / top border"


def test_ragged_batch_selective_and_the_bench_crops(selective):
    handle, sd32, sd64 = selective
    for name, rgbs in (("sel5", [O.image(c) for c in O.BATCH5]), ("bench4", O.bench_crops())):
        maps = [_check_crop(handle, sd32, sd64, rgbs, c, f"{name}[{c}]", alone=True) for c in range(len(rgbs))]
        _check_candidates(handle, rgbs, maps, name)


def test_ragged_batch_whose_crops_all_reach_onet(dense):
    """window runs at non-zero offsets in BOTH networks: crops 1 and 2 follow crops that hand windows to R-Net and O-Net"""
    handle, sd32, sd64 = dense
    rgbs = [O.image(c) for c in O.BATCH4]
    maps = [_check_crop(handle, sd32, sd64, rgbs, c, f"batch4[{c}]", alone=True) for c in range(len(rgbs))]
    assert all("onet.prob" in m for m in maps[:3]) and all("rnet.prob" in m for m in maps)
    _check_candidates(handle, rgbs, maps, "batch4")


# ------------------------------------------------------------------------------------------------ windows and injection
def _window_list(h, w):
    """source windows that touch each border and both far corners, 1 px wide / high / both, the whole image, and squares"""
    wins = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (0, 5, 1, h - 5), (w - 1, 0, 1, h), (3, 0, w - 3, 1), (0, h - 1, w, 1),
            (w - 30, h - 31, 30, 31), (0, 0, 23, 25), (w - 49, 0, 49, 47), (0, h - 97, 95, 97), (7, 9, 24, 24), (11, 13, 48, 48),
            (5, 6, 2, 3), (w // 2, h // 2, 1, 40), (w // 3, h // 3, 60, 1)]
    rs = np.random.RandomState(9)
    for _ in range(21):
        ww, hh = int(rs.randint(1, w)), int(rs.randint(1, h))
        wins.append((int(rs.randint(0, w - ww + 1)), int(rs.randint(0, h - hh + 1)), ww, hh))
    return wins


@pytest.mark.parametrize("net", ["rnet", "onet"])
def test_windows_at_the_borders_and_one_pixel_wide(dense, net):
    """the window resize + the whole trunk on windows no cascade run is sure to produce: clipped at every border, 1 px
    wide, 1 px high, 1 x 1, larger and smaller than the network input; 37 windows - ragged against every GEMM tile"""
    handle, sd32, sd64 = dense
    rgb = O.image((161, 240, 7))
    wins = _window_list(161, 240)
    assert len(wins) == 37
    fetch = lambda name: handle.mtcnn_net_tap(net, np.asarray(wins, np.int32), name, image=_bgr(rgb))
    taps = _net_taps(net, fetch, len(wins))
    _check_net(net, taps, sd32, sd64, f"{net} windows", O.window_inputs(rgb, wins, 48 if net == "onet" else 24))


def _injected(m, sz, seed):
    """inputs no image produces: beyond the normalised range, constant windows, a window of zeros, one of denormals"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1, 1, (m, sz, sz, 3)).astype(np.float32)
    x[0] = 0.0
    if m > 3:
        x[1] = -0.99609375
        x[2] = rs.uniform(-4, 4, (sz, sz, 3))
        x[3] = 1e-39
    return x


@pytest.mark.parametrize("net,m", [("rnet", 1), ("rnet", 77), ("onet", 1), ("onet", 37)])
def test_injected_windows_ragged_counts(dense, net, m):
    handle, sd32, sd64 = dense
    x = _injected(m, 48 if net == "onet" else 24, m)
    taps = _net_taps(net, lambda name: handle.mtcnn_net_tap(net, x, name), m)
    _check_net(net, taps, sd32, sd64, f"{net} injected m={m}", x)


CHUNK = 4096                      # refine_gpu's kChunk


@pytest.mark.parametrize("net", ["rnet", "onet"])
def test_more_windows_than_one_chunk(dense, net):
    """4096 + 5 injected windows: the second chunk writes prob + 4096, reg + 4 * 4096, pts + 10 * 4096.  The "prob" /
    "reg" / "pts" taps read the FINAL arrays after every chunk has run (what the box kernels read), so a dropped offset
    (chunk 2 landing on rows 0..4) or a clobbered first chunk shows in the rows read here: 0..2, and 4090..4100 on both
    sides of the boundary, each against the oracle from the dense tap of the same call.  The windows are all different,
    so no wrong row can pass for the right one."""
    handle, sd32, sd64 = dense
    sz = 48 if net == "onet" else 24
    m = CHUNK + 5
    x = _injected(m, sz, 5)
    for row0, rows in ((CHUNK - 6, 11), (0, 3)):
        taps = _net_taps(net, lambda name: handle.mtcnn_net_tap(net, x, name, row0, rows), rows)
        _check_net(net, taps, sd32, sd64, f"{net} m={m} rows {row0}..", x[row0:row0 + rows])
    # the outputs of ALL windows in one read of the final arrays: the two chunks tile them without overlap
    prob = handle.mtcnn_net_tap(net, x, net + ".prob")
    reg = handle.mtcnn_net_tap(net, x, net + ".reg")
    assert prob.shape == (m,) and reg.shape == (m, 4)
    own = handle.mtcnn_net_tap(net, x[CHUNK:], net + ".prob"), handle.mtcnn_net_tap(net, x[CHUNK:], net + ".reg")
    first = handle.mtcnn_net_tap(net, x[:5], net + ".prob"), handle.mtcnn_net_tap(net, x[:5], net + ".reg")
    rtol = 1e-5 * max(1.0, float(np.abs(reg).max()))
    with torch.no_grad():
        t = O.chain(net, sd64, torch.from_numpy(x[CHUNK - 3:]).permute(0, 3, 1, 2).double())
    assert np.abs(prob[CHUNK - 3:] - t[net + ".prob"].numpy()).max() <= 1e-5            # chained float64 reference
    assert np.abs(reg[CHUNK - 3:] - t[net + ".reg"].numpy()).max() <= rtol
    assert np.abs(prob[CHUNK:] - own[0]).max() <= 1e-5 and np.abs(reg[CHUNK:] - own[1]).max() <= rtol
    assert np.abs(prob[:5] - first[0]).max() <= 1e-5 and np.abs(reg[:5] - first[1]).max() <= rtol     # chunk 2 did not land on rows 0..4
    assert np.abs(reg[CHUNK:] - first[1]).max() > 1e3 * rtol                           # (those rows do differ)


@pytest.mark.parametrize("net", ["rnet", "onet"])
def test_more_source_windows_than_one_chunk(dense, net):
    """4096 + 7 source windows of an image through the production window list (`wd_all + start`): the network inputs of
    the windows on both sides of the chunk boundary are bit-exact, and so the second chunk reads ITS windows; their
    layers and final prob / reg / pts rows against the oracle"""
    handle, sd32, sd64 = dense
    rgb = O.image((161, 240, 7))
    rs = np.random.RandomState(12)
    m = CHUNK + 7
    ww, hh = rs.randint(1, 120, m), rs.randint(1, 100, m)
    wins = np.stack([rs.randint(0, 240 - ww + 1), rs.randint(0, 161 - hh + 1), ww, hh], 1).astype(np.int32)
    assert len({tuple(w) for w in wins[CHUNK - 8:]}) == 15 and not any(tuple(w) in {tuple(v) for v in wins[:7]} for w in wins[CHUNK:])
    sz = 48 if net == "onet" else 24
    for row0, rows in ((CHUNK - 8, 15), (0, 4)):
        fetch = lambda name: handle.mtcnn_net_tap(net, wins, name, row0, rows, image=_bgr(rgb))
        taps = _net_taps(net, fetch, rows)
        _check_net(net, taps, sd32, sd64, f"{net} windows m={m} rows {row0}..",
                   O.window_inputs(rgb, [tuple(int(v) for v in w) for w in wins[row0:row0 + rows]], sz))


# ------------------------------------------------------------------------------------------------ capacity, stale scratch
def _device_and_host_box_paths(handle, rgb, monkeypatch):
    """(overflow flag, candidate count, {stage: rows}, (face, box)) of the device box path, after asserting that the
    candidate list equals the maps and that rows, box and face equal those of the host box path"""
    bgr = _bgr(rgb)
    monkeypatch.setenv("DFD_MT_DEVICE_BOXES", "1")
    flag = float(handle.mtcnn_tap_batch([bgr], 0, "boxes.overflow").reshape(-1)[0])
    maps = {}
    for k in range(len(O.levels(*rgb.shape[:2]))):
        maps[f"pnet.prob.{k}"] = handle.mtcnn_tap_batch([bgr], 0, f"pnet.prob.{k}")
        maps[f"pnet.reg.{k}"] = handle.mtcnn_tap_batch([bgr], 0, f"pnet.reg.{k}")
    n = _check_candidates(handle, [rgb], [maps], str(rgb.shape))
    fd, bd = handle.mtcnn_align(bgr)
    rows_d = [handle.mtcnn_tap_batch([bgr], 0, s) for s in ("stage1", "stage2", "stage3")]
    monkeypatch.setenv("DFD_MT_DEVICE_BOXES", "0")
    fh, bh = handle.mtcnn_align(bgr)
    rows_h = [handle.mtcnn_tap_batch([bgr], 0, s) for s in ("stage1", "stage2", "stage3")]
    assert (fd is None) == (fh is None)
    if fd is not None:
        assert np.array_equal(bd, bh) and np.array_equal(fd, fh)
    for a, b in zip(rows_d, rows_h):
        assert a.shape == b.shape and np.array_equal(a, b)
    return flag, n


def test_candidates_beyond_the_device_block_report_overflow(dense, monkeypatch):
    """More P-Net candidates in one crop than a stage-1 block holds (kMtCap1 = 8192): the overflow flag is raised, the
    candidate list still equals the maps record for record, and rows, box and face equal the host path's.  The 700 x 900
    dense case of tests/test_mtcnn_gpu.py does NOT get there: the seeded cascade passes 1.4 % of its 107,088 cells
    (1,451 candidates), so it runs on the device path with the flag clear - asserted here, with the same agreement.
    The 2000 x 2400 image of the same texture has 848,988 cells and ~12.4 k candidates, counted from the maps."""
    handle, sd32, sd64 = dense
    flag, n = _device_and_host_box_paths(handle, O.image((700, 900, 3)), monkeypatch)
    print(f"700x900: {n} candidates, overflow {flag}")
    assert 0 < n <= 8192 and flag == 0.0
    flag, n = _device_and_host_box_paths(handle, O.image((2000, 2400, 3)), monkeypatch)
    print(f"2000x2400: {n} candidates, overflow {flag}")
    assert n > 8192, n                                     # kMtCap1
    assert flag == 1.0


def test_stale_scratch_of_a_large_call_does_not_reach_a_small_one(pkg, dense, seeded_sd, mtcnn_sd):
    """conv2's MFMA rows read two floats past the last pooled row of the last level.  The scratch is filled with
    non-finite R-/O-Net leftovers again BEFORE EVERY tap call of a small image (one level, 6 x 9 x 10 pooled floats: the
    pad lies inside the 300 x 128 floats the R-Net call leaves in the same buffer); every tap, the candidate list and
    the rows equal those of a fresh handle bit for bit and hold no NaN.  The small image hands no box to R-Net (asserted),
    so nothing of its own overwrites the leftovers between the poisoning and the P-Net launches."""
    handle, sd32, sd64 = dense
    big, small = O.image(O.STALE_BIG), O.image(O.STALE_SMALL)
    x = _injected(600, 48, 8)
    x[:, :, :, :] = np.where(np.arange(600)[:, None, None, None] % 2 == 0, np.float32(np.nan), x)      # NaN leftovers too
    inf = np.full((300, 24, 24, 3), np.inf, np.float32)

    def poison():
        handle.mtcnn_net_tap("onet", x, "onet.prob")
        left = handle.mtcnn_net_tap("rnet", inf, "rnet.dense4").reshape(-1)                 # what R-Net leaves in that buffer
        assert not np.isfinite(left[6 * 9 * 10:6 * 9 * 10 + 16]).any()                      # ... where the pad of the small image is

    handle.mtcnn_align(_bgr(big))
    after = _check_crop(handle, sd32, sd64, [small], 0, "stale small", before=poison)
    assert len(after["stage1"]) == 0 and "rnet.prob" not in after
    poison()
    cand_a = handle.mtcnn_tap_batch([_bgr(small)], 0, "pnet.cand")
    poison()
    face_a = handle.mtcnn_align(_bgr(small))
    W = pkg.weights
    fresh = pkg._lib.Handle(W.pack_all(seeded_sd, W.seeded_ssd_state_dict(0), mtcnn_sd), device=0, max_batch=4)
    try:
        want = _check_crop(fresh, sd32, sd64, [small], 0, "fresh small")
        cand_f = fresh.mtcnn_tap_batch([_bgr(small)], 0, "pnet.cand")
        face_f = fresh.mtcnn_align(_bgr(small))
    finally:
        fresh.close()
    assert sorted(after) == sorted(want) and "pnet.conv2.0" in want
    for n in want:
        assert np.array_equal(after[n], want[n], equal_nan=True), n
        assert not np.isnan(np.asarray(after[n], np.float64)).any(), n
    assert cand_a[1] == cand_f[1] and cand_a[0].shape == cand_f[0].shape
    ua, uf = (np.ascontiguousarray(c[0]).view(np.uint32) for c in (cand_a, cand_f))
    assert np.array_equal(ua[np.argsort(ua[:, 0])], uf[np.argsort(uf[:, 0])])
    assert (face_a[0] is None) == (face_f[0] is None)
    if face_a[0] is not None:
        assert np.array_equal(face_a[0], face_f[0]) and np.array_equal(face_a[1], face_f[1])


# ------------------------------------------------------------------------------------------------ the VALU P-Net path
def _pnet_path_dump(path):
    """(child process) every check of every batched case of this file, both cascades, and the edge sizes on this
    process's P-Net path; stage rows, boxes and faces to `path`"""
    import rtdfd_amd as pkg

    W = pkg.weights
    dump = {}
    sets = {"dense": [("batch5", [O.image(c) for c in O.BATCH5]), ("batch4", [O.image(c) for c in O.BATCH4])],
            "selective": [("sel5", [O.image(c) for c in O.BATCH5]), ("bench4", O.bench_crops())]}
    for which, batches in sets.items():
        sd = W.seeded_mtcnn_state_dict(0) if which == "dense" else W.seeded_mtcnn_state_dict(0, W.MTCNN_SELECTIVE)
        handle = pkg._lib.Handle(W.pack_all(W.seeded_state_dict(0), W.seeded_ssd_state_dict(0), sd), device=0, max_batch=16)
        sd32, sd64 = _sds(pkg, sd)
        if which == "dense":
            batches = batches + [(f"edge{i}", [O.image(c)]) for i, c in enumerate(O.EDGE_CASES)]
        for name, rgbs in batches:
            maps = [_check_crop(handle, sd32, sd64, rgbs, c, f"path {name}[{c}]", alone=len(rgbs) > 1) for c in range(len(rgbs))]
            _check_candidates(handle, rgbs, maps, "path " + name)
            for c, (rgb, m) in enumerate(zip(rgbs, maps)):
                for st in ("stage1", "stage2", "stage3"):
                    dump[f"{name}.{c}.{st}"] = m[st]
                face, box = handle.mtcnn_align(_bgr(rgb))
                dump[f"{name}.{c}.found"] = np.asarray(face is not None)
                if face is not None:
                    dump[f"{name}.{c}.face"], dump[f"{name}.{c}.box"] = face, box
        handle.close()
    np.savez(path, **dump)
    print("vs_yard", {k: round(v, 2) for k, v in sorted(REPORT.items())})


def test_valu_pnet_path_in_a_process_of_its_own(tmp_path):
    """DFD_MT_PNET_MFMA is read once per process: a fresh child runs every batched case (both cascades) and the edge sizes with the VALU
    kernels (mt_convpx_kernel) against the same bars, another with the MFMA kernels; on these threshold-unambiguous
    inputs the stage rows and the selected 160 x 160 faces of the two paths are equal"""
    got = {}
    for flag in ("0", "1"):
        path = str(tmp_path / f"pnet{flag}.npz")
        code = "import sys; sys.path.insert(0, %r); from tests import test_mtcnn_stages_gpu as T; T._pnet_path_dump(%r)" % (ROOT, path)
        env = dict(os.environ, DFD_MT_PNET_MFMA=flag)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
        print(r.stdout[-3000:])
        assert r.returncode == 0, (flag, r.stdout[-3000:], r.stderr[-3000:])
        got[flag] = dict(np.load(path))
    valu, mfma = got["0"], got["1"]
    assert sorted(valu) == sorted(mfma)
    assert any(k.endswith(".face") for k in valu)
    worst = [0.0, 0.0]
    for k in valu:
        if k.endswith((".face", ".found")):
            assert np.array_equal(valu[k], mfma[k]), k
        else:
            # rows: the same boxes survive every stage.  Their coordinates are float32 box arithmetic on two P-Net
            # regressions that differ in summation order only, so they are held to the bar tests/test_mtcnn_gpu.py holds
            # rows to (1e-2 px, 1e-4 probability), not to bit equality
            assert valu[k].shape == mfma[k].shape, k
            valu[k], mfma[k] = valu[k].reshape(-1, 5), mfma[k].reshape(-1, 5)        # (the selected box: one row)
            if valu[k].size:
                worst[0] = max(worst[0], float(np.abs(valu[k][:, :4] - mfma[k][:, :4]).max()))
                worst[1] = max(worst[1], float(np.abs(valu[k][:, 4] - mfma[k][:, 4]).max()))
    print(f"VALU vs MFMA rows: max |d| {worst[0]:.3e} px, {worst[1]:.3e} probability")
    assert worst[0] <= 1e-2 and worst[1] <= 1e-4, worst
