"""CPU: the per-kernel MTCNN oracle (tests/mtcnn_stage_oracle.py) is itself right, its bars can fail, and the inputs of
the GPU suite (tests/test_mtcnn_stages_gpu.py) have the properties that suite relies on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mtcnn_ref as M
from tests import mtcnn_stage_oracle as O


@pytest.fixture(scope="module")
def sds(pkg, mtcnn_sd):
    W = pkg.weights
    sel = W.seeded_mtcnn_state_dict(0, W.MTCNN_SELECTIVE)
    f64 = lambda sd: {k: v.double() for k, v in W.to_torch(sd).items()}
    return {"dense": (W.to_torch(mtcnn_sd), f64(mtcnn_sd)), "selective": (W.to_torch(sel), f64(sel))}


def test_pool_out_is_torch_ceil_mode():
    for k, s in ((2, 2), (3, 2)):
        for n in range(k, 60):
            assert O.pool_out(n, k, s) == F.max_pool2d(torch.zeros(1, 1, n, n), k, s, ceil_mode=True).shape[-1], (n, k, s)


@pytest.mark.parametrize("case", [(40, 33, 6), (161, 240, 7), (20, 30, 22)])
def test_area_resize_is_torch_area_interpolation(case):
    """the exact integer reference agrees with interpolate(mode="area") to fp32 rounding (torch sums floats), and the
    float32 mirror is the formula's value exactly where torch's own arithmetic is exact: on the identity resize"""
    rgb = O.image(case)
    h, w = rgb.shape[:2]
    img = torch.from_numpy(rgb).permute(2, 0, 1)[None].float()
    for sc, sh, sw, *_ in O.levels(h, w):
        want = ((M.imresample(img, (sh, sw)) - 127.5) * 0.0078125)[0].permute(1, 2, 0).numpy()
        got = O.area_resize(rgb, sh, sw)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.abs(got - want).max() <= 2e-6, sc
    assert np.array_equal(O.area_resize(rgb, h, w), ((rgb.astype(np.float32) - np.float32(127.5)) * np.float32(0.0078125)))


def test_an_off_by_one_window_bound_fails_the_exact_comparison():
    rgb = O.image((90, 75, 5))
    good = O.area_resize(rgb, 55, 46)
    wide = O.area_resize(rgb, 55, 46, bounds=lambda o, size, out: ((o * size) // out, ((o + 1) * size + out - 1) // out + 1))
    low = O.area_resize(rgb, 55, 46, bounds=lambda o, size, out: (np.maximum((o * size) // out - 1, 0), ((o + 1) * size + out - 1) // out))
    floor_hi = O.area_resize(rgb, 55, 46, bounds=lambda o, size, out: ((o * size) // out, np.maximum(((o + 1) * size) // out, (o * size) // out + 1)))
    for bad in (wide, low, floor_hi):
        assert not np.array_equal(good, bad)
        assert (good != bad).mean() > 0.05          # not one stray pixel: a wrong bound moves many window sums


@pytest.mark.parametrize("net", ["rnet", "onet"])
@pytest.mark.parametrize("which", ["dense", "selective"])
def test_chained_float64_layers_reproduce_the_reference_networks(sds, net, which):
    sd32, sd64 = sds[which]
    sz = 24 if net == "rnet" else 48
    x = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, (7, 3, sz, sz)).astype(np.float32))
    taps = O.chain(net, sd64, x.double())
    with torch.no_grad():
        out = (M.rnet if net == "rnet" else M.onet)(sd32, x)
    reg, prob = out[0], out[-1][:, 1]
    assert float((taps[net + ".prob"] - prob.double()).abs().max()) <= 1e-5
    assert float((taps[net + ".reg"] - reg.double()).abs().max()) <= 1e-5 * max(1.0, float(reg.abs().max()))
    if net == "onet":
        assert float((taps["onet.pts"] - out[1].double()).abs().max()) <= 1e-5 * max(1.0, float(out[1].abs().max()))
    for name, (edge, ch) in O.NET_SHAPES.items():
        if name.startswith(net):
            assert tuple(taps[name].shape) == (7, ch, edge, edge), name
    for name, real in O.REAL.items():
        if name.startswith(net):
            assert float(taps[name][:, real:].abs().max()) == 0.0


@pytest.mark.parametrize("which", ["dense", "selective"])
def test_chained_float64_pnet_reproduces_the_reference_network(sds, which):
    sd32, sd64 = sds[which]
    x = torch.from_numpy(np.random.RandomState(4).uniform(-1, 1, (1, 3, 37, 52)).astype(np.float32))
    taps = {"pnet.in": x.double()}
    get = lambda k: taps[k]
    taps["pnet.pool1"] = O.layer("pnet.pool1", get, sd64)
    taps["pnet.conv2"] = O.layer("pnet.conv2", get, sd64)
    prob, reg = O.layer("pnet.out", get, sd64)
    with torch.no_grad():
        wreg, wprob = M.pnet(sd32, x)
    assert float((prob - wprob[:, 1].double()).abs().max()) <= 1e-5
    assert float((reg - wreg.double()).abs().max()) <= 1e-5 * max(1.0, float(wreg.abs().max()))


def test_a_perturbation_of_the_bar_in_one_channel_fails_the_check(sds):
    """the fp32 yardstick passes its own bar with room; the same tensor with ONE channel of ONE window moved by the max
    bar x its conditioning scale (a few fp32 ulps of the terms it sums) fails it"""
    sd32, sd64 = sds["dense"]
    x = torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, (5, 3, 24, 24)).astype(np.float32))
    taps64 = O.chain("rnet", sd64, x.double())
    get64 = lambda k: taps64[k]
    get32 = lambda k: taps64[k].float()
    for name, real in (("rnet.conv2", 48), ("rnet.dense4", 128), ("rnet.pool1", 28)):
        yard = O.layer(name, get32, sd32).double()
        base = O.check(name, yard, get64, get32, sd64, sd32)[0]
        assert base["ratio"] <= 0.5, (name, base)
        ref, u = O.layer(name, get64, sd64), O.scale(name, get64, sd64)
        step = 1.01 * O.max_bar(base["yard"]["max"])
        assert step < 64 * 2.0 ** -23                       # the bar is a few fp32 ulps of the scale
        bad = ref.clone()
        bad[2, 3] += step * u[2, 3]
        assert O.check(name, bad, get64, get32, sd64, sd32)[0]["ratio"] > 1.0, name
        one = ref.clone()                                   # ... and so does ONE element of that channel
        idx = (2, 3) + (0,) * (ref.dim() - 2)
        one[idx] += step * u[idx]
        assert O.check(name, one, get64, get32, sd64, sd32)[0]["ratio"] > 1.0, name
        assert O.check(name, ref, get64, get32, sd64, sd32)[0]["ratio"] == 0.0


def test_edge_cases_have_the_shapes_they_were_chosen_for():
    lv = O.levels(20, 33)
    assert len(lv) == 1 and lv[0][1:3] == (13, 20) and lv[0][5:] == (2, 5)
    assert [(sh - 2) % 2 for _, sh, sw, *_ in lv] == [1] and [(sw - 2) % 2 for _, sh, sw, *_ in lv] == [0]
    lv = O.levels(20, 30)
    assert len(lv) == 1 and (lv[0][1] - 2) % 2 == 1 and (lv[0][2] - 2) % 2 == 1
    lv = O.levels(33, 20)
    assert (lv[0][1] - 2) % 2 == 0 and (lv[0][2] - 2) % 2 == 1
    for h, w, _ in O.SINGLE_CASES:                         # no level of any size has a grid below 2 x 2
        assert all(oh >= 2 and ow >= 2 for *_, oh, ow in O.levels(h, w))
    lv = O.levels(47, 58)
    c2 = [(ph - 2, pw - 2) for _, _, _, ph, pw, _, _ in lv]
    assert len(lv) >= 3 and all(cw % 16 for _, cw in c2), c2                   # 16-pixel tiles straddle rows ...
    assert all((ch * cw) % 16 for ch, cw in c2[:-1]), c2                       # ... and levels
    assert all((lv[-1][3] * lv[-1][4]) % 256 for lv in (O.levels(h, w) for h, w, _ in O.SINGLE_CASES) if lv)
    assert len({c[:2] for c in O.BATCH5}) == 5


def _margin_inputs():
    cases = [("dense", c, O.image(c)) for c in O.SINGLE_CASES + O.BATCH5 + [O.STALE_BIG]]
    return cases + [("selective", None, c) for c in O.bench_crops()] + [("selective", c, O.image(c)) for c in O.BATCH5]


def test_no_probability_of_the_gpu_suites_inputs_is_near_its_threshold(sds):
    """every image the GPU suite sends through a whole cascade keeps all P-, R- and O-Net probabilities further than
    1e-4 from their thresholds (oracle alone), so that suite can assert equal rows instead of skipping ambiguous ones;
    the one shared fixture whose seed is not picked here (mtcnn_stage_oracle.NEAR_THRESHOLD) is held to its own figure"""
    worst = []
    with torch.no_grad():
        for which, case, rgb in _margin_inputs():
            if min(rgb.shape[:2]) < 20:
                continue
            worst.append((O.threshold_margin(sds[which][0], rgb) / O.NEAR_THRESHOLD.get(case, 1e-4), which, rgb.shape))
    assert min(w[0] for w in worst) > 1.0, sorted(worst)[:3]
    assert set(O.NEAR_THRESHOLD) <= set(O.SINGLE_CASES) and len(O.NEAR_THRESHOLD) == 1
