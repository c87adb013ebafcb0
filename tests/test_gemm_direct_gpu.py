"""GPU: the split GEMM on its own - every kernel family, ragged shapes, float64 (dfd_gemm_tap; oracle: tests/gemm_oracle.py,
whose teeth tests/test_gemm_oracle.py proves on the CPU).

Protocol, for every call in gemm_oracle.CASES: the tap reports the candidate count c of that very call; the heuristic
tile ("gemm_tile" = -1) and every i in range(c) run; every forced run must equal the heuristic one bit for bit; the 64
guard rows in front of and behind the result must still hold the sentinel and no sentinel may survive inside; the
heuristic result must hold b0_layer_oracle's bars against float64 (fp32: rms <= 4 x and max |d| / u <= 8 x the float32
CPU yardstick; bf16: <= 1 ulp and <= 1 % of the elements off the bf16 mirror), the exact families must equal float64 in
every candidate.  Over the module, the reported tiles must show every kernel family at least once at an M that is no
multiple of its block height, pw8 / pw9 among the candidates of every case built for them, and dfd_gemm_tile_count() at
least the largest count reported.  One call above 2^31 bytes of activations checks the chunk loop of
launch_pointwise_split.

FOUND by this test (both fixed): pw8 gave images past a block's second one the second one's gate row when
an image has fewer 16-row tiles than the block has waves (HW = 16; HW = 64 with the 8 waves of K = 232 / 256) - the
dispatcher let the wave count override the tiles-per-image bound; pw9 stored -0 where every other instance stores +0
(swish below about -88: its epilogue lacked the add of the absent residual's zeros).

MEASURED on one MI355X, 164 calls and every candidate of each:
  worst HIP error / float32 yardstick error per group (the worse of rms and max; the bar is 4 x / 8 x):
    pointwise 1.19 (cancel family 0.24), pw8 shapes 1.39, pw9 shapes 1.36, gated pw6 / pw7 1.04, conv mode 0.85;
    bf16 calls: worst exactly 1 ulp (bar 1), under 1 % of the elements off the mirror; exact families: equal to float64
  candidates the tap reported per (K, N):
    pointwise 16/2: 2, 24/10: 2, 40/30: 10, 72/64: 21, 104/100: 43, 264/196: 58 (the same with bf16)
    pw8 shapes (eight pw8 instances included) K <= 32: N = 16: 10, 24: 13, 40 and 48: 21; K > 32: N = 16: 12, 24: 18,
      40 and 48: 29; gated without pw8 (HW = 1, 49, 196) 96/24 and 104/30: 10, 240/40: 21
    pw9 shapes (three pw9 instances included) 72/192, 80/480, 112/672: 65, 128/196: 61
    conv K = 32 .. 576: N = 10: 2 (K = 32) or 4, N = 64: 21;  exact 16/30 and 32/30: 5, 16/24 and 32/24: 13, 72/192: 65
    dfd_gemm_tile_count() = 65 = the largest per-call count
  run time: pointwise 0.12 s, pw8 0.63 s, pw9 0.24 s, gated 0.05 s, conv 0.04 s, bf16 0.03 s, exact 0.03 s (1.1 s in
  all); the call above 2^31 bytes 1.35 s (host inputs 0.21 s, the tap 0.01 s, host checks 1.12 s): tile pw6 4 x (1 x 1),
  2 launches, 0.23 of the float64 bar (1.13 x the yardstick), every row within 0.0052 of the (7K + 4) 2^-24 u bound.
  the call above 2^32 bytes of OUTPUT (K = 16, N = 48, 22.4 M rows; the chunk is bounded by the largest of the X, Y and R
  rows): 21 candidates (8 pw6, 5 pw7, 8 pw8), 3 launches each, rows and whole-result digest of every instance equal to the
  heuristic tile's (pw6 4 x (1 x 3)), 0.10 of the float64 bar (0.31 x the yardstick); 4.4 s, the slowest call 1.1 s.
"""
import time

import numpy as np
import pytest

import gemm_oracle as G

pytestmark = pytest.mark.gpu

SENT32 = np.uint32(0x7FC5A5A5)
SEEN = {"ragged": set(), "counts": {}, "worst": {}, "groups": set()}
# (family key) every one of which must have run at an M that is no multiple of its block height
REQUIRED = {("pw6", 4, 1), ("pw6", 4, 2), ("pw6", 8, 1), ("pw6", 8, 2), ("pw7",), ("pw8", 1), ("pw8", 3), ("pw8", 5), ("pw8", 8),
            ("pw9", 6, 1), ("pw9", 4, 1), ("pw9", 4, 2)}


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.uint16 else np.uint32)


def _family(tile, k):
    kind, wm, wn, mt, nt, ks = tile
    if kind == 0:
        return ("pw6", wm, ks), wm * mt * 16
    if kind == 1:
        return ("pw7",), wm * mt * 16
    if kind == 2:
        return ("pw8", -(-k // 32)), 16
    return ("pw9", nt, ks), 128


def _tap(h, case, inp):
    conv = case.conv is not None
    x = inp["x"] if not case.bf16 else G.to_bits(inp["x"])
    res = inp["res"] if inp["res"] is None or not case.bf16 else G.to_bits(inp["res"])
    return h.gemm_tap(x, inp["w"], inp["bias"], act=case.act, gate=inp["gate"], res=res, res_first=case.res == "first", hw=case.HW,
                      bf16=case.bf16, planes=case.planes, conv=case.conv_dict() if conv else None)


def _guards_ok(r):
    sent = np.uint16(int(SENT32) >> 16) if r["y"].dtype == np.uint16 else SENT32
    return bool((_bits(r["before"]) == sent).all() and (_bits(r["after"]) == sent).all()), bool((_bits(r["y"]) != sent).all())


def _run_case(h, case, fails):
    ref = G.Reference(case)
    base = _tap(h, case, ref.inp)
    if base["rc"] != 0 or base["launches"] != 1:
        fails.append(f"{case.name}: rc {base['rc']}, {base['launches']} launches")
        return
    c = base["candidates"]
    SEEN["counts"].setdefault((case.group, case.K, case.N, case.gated, case.bf16), set()).add(c)
    kinds = set()
    runs = [(-1, base)]
    for i in range(c):
        h.set_option("gemm_tile", i)
        runs.append((i, _tap(h, case, ref.inp)))
    h.set_option("gemm_tile", -1)
    for i, r in runs:
        fam, rows = _family(r["tile"], case.K)
        kinds.add(fam[0])
        if case.M % rows:
            SEEN["ragged"].add(fam)
        outside, inside = _guards_ok(r)
        if not outside:
            fails.append(f"{case.name}: tile {i} {r['tile']} wrote into a guard row")
        if not inside:
            fails.append(f"{case.name}: tile {i} {r['tile']} left a sentinel inside the result")
        if i >= 0 and not np.array_equal(_bits(r["y"]), _bits(base["y"])):
            ne = _bits(r["y"]) != _bits(base["y"])
            d, at = np.flatnonzero(ne.any(axis=1)), tuple(np.argwhere(ne)[0])
            fails.append(f"{case.name}: tile {i} {r['tile']} differs from the heuristic {base['tile']} in {d.size} rows, first {d[:4]}; "
                         f"at {at}: {_bits(r['y'])[at]:#x} against {_bits(base['y'])[at]:#x}")
        if case.family.startswith("exact") and not ref.check(r["y"])["exact"]:
            fails.append(f"{case.name}: tile {i} {r['tile']} is not bit-equal to float64")
    m = ref.check(base["y"])
    key = (case.group, "bf16" if case.bf16 else case.family)
    SEEN["worst"][key] = max(SEEN["worst"].get(key, 0.0), m["ratio"] if case.bf16 else m["vs_yard"])
    if m["ratio"] > 1.0:
        fails.append(f"{case.name}: bar ratio {m['ratio']:.3f} ({m})")
    if case.expect and case.expect not in kinds:
        fails.append(f"{case.name}: {case.expect} is not among its {c} candidates")


@pytest.mark.parametrize("group", G.GROUPS)
def test_every_candidate_identical_guards_intact_bars_held(b0_handle, group):
    h = b0_handle
    fails, t0 = [], time.time()
    cases = [c for c in G.CASES if c.group == group]
    try:
        for case in cases:
            _run_case(h, case, fails)
    finally:
        h.set_option("gemm_tile", -1)
    SEEN["groups"].add(group)
    worst = {k[1]: round(v, 3) for k, v in SEEN["worst"].items() if k[0] == group}
    counts = sorted((k[1], k[2], k[3], k[4], sorted(v)) for k, v in SEEN["counts"].items() if k[0] == group)
    print(f"\n[gemm_direct] {group}: {len(cases)} calls in {time.time() - t0:.2f} s; worst HIP / yardstick (bf16: bar ratio) {worst}")
    print(f"[gemm_direct] {group}: candidates per (K, N, gated, bf16): {counts}")
    assert not fails, f"{len(fails)} failures, first: " + " | ".join(fails[:8])


def test_refused_shapes_return_the_error_code_and_launch_nothing(b0_handle):
    h = b0_handle
    rs = np.random.RandomState(3)
    for k, n in G.REFUSED_POINTWISE:
        r = h.gemm_tap(rs.randn(17, k), rs.randn(n, k), rs.randn(n))
        assert r["rc"] == -7 and r["launches"] == 0 and r["candidates"] == 0, (k, n, r["rc"])
        assert (_bits(r["y"]) == SENT32).all() and (_bits(r["before"]) == SENT32).all() and (_bits(r["after"]) == SENT32).all()
    g = G.REFUSED_CONV
    r = h.gemm_tap(rs.randn(g["n_img"], g["H"], g["W"], g["Cin"]), rs.randn(10, g["ksize"], g["ksize"], g["Cin"]), rs.randn(10), conv=g)
    assert r["rc"] == -7 and r["launches"] == 0
    assert (_bits(r["y"]) == SENT32).all() and (_bits(r["before"]) == SENT32).all() and (_bits(r["after"]) == SENT32).all()


def test_every_kernel_family_ran_ragged_and_the_tile_count_covers_every_call(pkg, b0_handle):
    if SEEN["groups"] != set(G.GROUPS):
        pytest.fail("run the whole module: this test reads what the case groups recorded")
    assert REQUIRED <= SEEN["ragged"], f"never ran at a ragged M: {sorted(REQUIRED - SEEN['ragged'])}"
    largest = max(max(v) for v in SEEN["counts"].values())
    count = pkg._lib.load().dfd_gemm_tile_count()
    print(f"\n[gemm_direct] dfd_gemm_tile_count() = {count}, largest per-call count {largest}")
    assert count >= largest


CHUNK_K, CHUNK_N, CHUNK_HW, CHUNK_IMAGES, CHUNK_BLOCK = 256, 16, 49, 42800, 65536


def test_one_call_above_2g_takes_two_launches_and_addresses_every_row(pkg, b0_handle):
    """Gated fp32, K = 256, HW = 49, N = 16, 42,800 images: M = 2,097,200 rows, 2,147,532,800 bytes of activations - 2
    launches by dfd_gemm_chunk_rows, of 42,799 images and of 1.  X repeats one random 64 MiB block; every image has its
    own gate row.  float64 bars on the first two images, the three images in front of the chunk boundary, and the image
    behind it (the last one); every row within (7K + 4) 2^-24 u of a float32 numpy matmul (the sum of both sides'
    worst-case dot-product bounds: it catches a misaddressed row, whose error is of order u)."""
    h, t0 = b0_handle, time.time()
    k, n, hw, images = CHUNK_K, CHUNK_N, CHUNK_HW, CHUNK_IMAGES
    m = images * hw
    assert m * k * 4 > (1 << 31) - 1
    chunk = pkg._lib.load().dfd_gemm_chunk_rows(m, k * 4, hw)
    assert chunk == 42799 * hw and -(-m // chunk) == 2
    rs = np.random.RandomState(11)
    block = rs.standard_normal((CHUNK_BLOCK, k)).astype(np.float32)
    gate = rs.uniform(0.05, 1.0, (images, k)).astype(np.float32)
    w = (rs.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    bias = rs.standard_normal(n).astype(np.float32)
    t1 = time.time()
    h.set_option("gemm_tile", -1)
    r = h.gemm_tap(block, w, bias, gate=gate, hw=hw, rows=m)
    t2 = time.time()
    assert r["rc"] == 0 and r["launches"] == 2, r["launches"]
    outside, inside = _guards_ok(r)
    assert outside and inside
    y = r["y"]
    # float64 bars on the images at the ends and around the boundary
    pick = [0, 1, 42796, 42797, 42798, 42799]
    rows = np.concatenate([np.arange(i * hw, (i + 1) * hw) for i in pick])
    sub = G.Case("chunk", rows.size, k, n, hw, gated=True)
    ref = G.Reference(sub, {"x": block[rows % CHUNK_BLOCK], "w": w, "bias": bias, "gate": gate[pick], "res": None})
    met = ref.check(y[rows])
    # every row against float32 numpy
    bound = np.float64((7 * k + 4) * 2.0 ** -24)
    wt, wa, worst = np.ascontiguousarray(w.T), np.ascontiguousarray(np.abs(w).T), 0.0
    step = 1337                                        # images per slab: 65,513 rows
    for i0 in range(0, images, step):
        i1 = min(images, i0 + step)
        xg = block[np.arange(i0 * hw, i1 * hw) % CHUNK_BLOCK] * np.repeat(gate[i0:i1], hw, axis=0)
        d = np.abs(y[i0 * hw:i1 * hw].astype(np.float64) - (xg @ wt + bias))
        u = (np.abs(xg) @ wa + np.abs(bias)).astype(np.float64)
        ratio = float((d / u).max()) / bound
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"images {i0}..{i1}: |d| / u = {ratio * bound:.3e} > {bound:.3e}, first row {i0 * hw + int(np.argmax((d / u).max(axis=1)))}"
    print(f"\n[gemm_direct] chunked call: tile {r['tile']}, float64 bars {met}, worst |d| / ((7K + 4) 2^-24 u) {worst:.4f}; "
          f"host inputs {t1 - t0:.2f} s, tap {t2 - t1:.2f} s, checks {time.time() - t2:.2f} s")
    assert met["ratio"] <= 1.0, met


WIDE_K, WIDE_N, WIDE_M, WIDE_BLOCK, WIDE_EDGE = 16, 48, 22_400_000, 65536, 160


def test_one_call_above_4g_of_output_is_chunked_by_its_largest_row_in_every_instance(pkg, b0_handle):
    """Thin fp32 call with K < N: K = 16, N = 48, M = 22,400,000 rows (HW = 1: a row is an image) - 1.43 GB of X and
    4.30 GB of Y, above 2^32 bytes on the OUTPUT side only.  pw8_kernel addresses Y with a 32-bit num_records and 32-bit
    byte offsets; bounded by X alone this call was ONE launch, whose offsets wrap.  The launchers bound a chunk by the
    largest of the X, Y and R rows: 11,184,810 rows (48 x 4 bytes each), 3 launches.  Every instance on the call's
    candidate list runs, the eight pw8 instances included, selected through "gemm_tile".  Of each run come back the first
    and the last 160 rows and the 160 rows on either side of both chunk borders (which are no multiples of 16: tiles
    straddle them), plus, computed on the device over ALL rows, the count of elements still at the sentinel and a
    position-sensitive digest.  The heuristic run's rows hold the float64 bars of this file; every forced run must
    return the same rows AND the same digest bit for bit, with no sentinel left and the guards intact."""
    h, t0 = b0_handle, time.time()
    k, n, m = WIDE_K, WIDE_N, WIDE_M
    assert m * n * 4 > 1 << 32 and m * k * 4 <= (1 << 31) - 1
    chunk = pkg._lib.load().dfd_gemm_chunk_rows(m, max(k, n) * 4, 1)
    assert chunk == ((1 << 31) - 1) // (n * 4) == 11_184_810 and -(-m // chunk) == 3 and chunk % 16 != 0
    assert pkg._lib.load().dfd_gemm_chunk_rows(m, k * 4, 1) == m                      # the rule before: one launch
    e = WIDE_EDGE
    keep = [(0, e), (chunk - e, chunk + e), (2 * chunk - e, 2 * chunk + e), (m - e, m)]
    rows = np.concatenate([np.arange(lo, hi) for lo, hi in keep])
    rs = np.random.RandomState(17)
    block = rs.standard_normal((WIDE_BLOCK, k)).astype(np.float32)
    w = (rs.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    bias = rs.standard_normal(n).astype(np.float32)
    sub = G.Case("chunk", rows.size, k, n, 1)
    ref = G.Reference(sub, {"x": block[rows % WIDE_BLOCK], "w": w, "bias": bias, "gate": None, "res": None})
    fails, kinds, times = [], {}, []
    try:
        h.set_option("gemm_tile", -1)
        base = h.gemm_tap(block, w, bias, rows=m, keep=keep)
        c = base["candidates"]
        runs = [(-1, base)]
        for i in range(c):
            h.set_option("gemm_tile", i)
            t1 = time.time()
            runs.append((i, h.gemm_tap(block, w, bias, rows=m, keep=keep)))
            times.append(time.time() - t1)
    finally:
        h.set_option("gemm_tile", -1)
    for i, r in runs:
        fam = _family(r["tile"], k)[0]
        kinds[fam[0]] = kinds.get(fam[0], 0) + 1
        if r["rc"] != 0 or r["launches"] != 3:
            fails.append(f"tile {i} {r['tile']}: rc {r['rc']}, {r['launches']} launches")
            continue
        outside, inside = _guards_ok(r)
        if not outside:
            fails.append(f"tile {i} {r['tile']} wrote into a guard row")
        if not inside or r["sentinels"] != 0:
            fails.append(f"tile {i} {r['tile']} left {r['sentinels']} elements of the result at the sentinel")
        if not np.array_equal(_bits(r["y"]), _bits(base["y"])):
            d = np.flatnonzero((_bits(r["y"]) != _bits(base["y"])).any(axis=1))
            fails.append(f"tile {i} {r['tile']} differs from the heuristic {base['tile']} in {d.size} of the rows returned, first at row {rows[d[0]]}")
        if r["digest"] != base["digest"]:
            fails.append(f"tile {i} {r['tile']}: digest of all rows {r['digest']:#x} against the heuristic's {base['digest']:#x}")
    met = ref.check(base["y"])
    print(f"\n[gemm_direct] 4.3 GB of Y: {c} candidates {kinds}, heuristic tile {base['tile']}, {base['launches']} launches, float64 bars {met}; "
          f"{time.time() - t0:.2f} s in all, {max(times):.2f} s the slowest forced call")
    assert c >= 10 and kinds.get("pw8", 0) == 8, kinds
    assert not fails, f"{len(fails)} failures, first: " + " | ".join(fails[:8])
    assert met["ratio"] <= 1.0, met
