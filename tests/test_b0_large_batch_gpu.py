"""GPU: the classifier at 257 to 4096 crops returns the bits of a 16-crop call (cases and their arithmetic:
tests/b0_batch_cases.py, held on the CPU by tests/test_b0_batch_cases.py).

dfd_create accepts max_batch up to 4096; the rest of the suite stops at 256 crops.  Above that the plan changes with n
against the CU count (mbconv_k5_kernel's second round, ragged 4-image groups of the 7 x 7 launches at large grids) and
tensors cross 2^31 bytes, 2^32 bytes and 2^31 elements.  Crop i of a large batch is crop idx[i] of a fixed 16-crop set
(the 9 random and the 7 edge crops of b0_layer_oracle, whose 16-crop bits test_b0_layers_gpu.py holds to float64), so
row i of every output must equal row idx[i] of ONE 16-crop call under the same options, bit for bit: every comparison
here is np.array_equal on uint32 views and no tolerance appears.

Per case: the logits (classify_device), the pooled features and block 15's output rows (the "feat" and "b15.out" taps
of the forward on the device-resident input: dfd_extract_features / dfd_extract_trunk are these taps by construction,
b0_plan.hip b0_trunk_to_host, but take host crops - 2.4 GB at 4096; at 257 crops, 155 MB, classify, extract_features
and extract_trunk run from host crops as well); on the 512 handle also the outputs of blocks 1, 5
and 10 and b8.dw, b8.exp either side of the k5 threshold (materialised below, "not materialised" from it on), the whole
2.2 GB b1.exp at 447 crops; Grad-CAM (logits and heatmaps) at 257 and 893.  The input is built on the device in slabs
of at most 256 crops.  Three handles, one open at a time; dfd_create running out of memory on the two large ones is a
skip with the message, anything else fails.

MEASURED on one MI355X (256 CUs, 288 GB): all three handles ran, none skipped for memory; every comparison held on the
first run (no kernel bug found in these paths).  Wall time per case (of which input upload), tensors compared:
  max_batch = 512, create_impl allocates 5.52 GB in 0.18 s:
    default 257 (k5 not taken; + Grad-CAM)            0.38 s (0.02)  8    default 463 = CUs + 207 (b8.exp exists)   0.26 s (0.03)  8
    default 464 = CUs + 208 (k5 taken, b8.exp refused) 0.19 s (0.03)  7    fuse0 447 (whole b1.exp, 2.15 GB: 0.51 s)  0.86 s (0.03)  8
  max_batch = 1792, 19.24 GB in 0.60 s:
    default 1339   1.28 s (0.54)  3      fuse0 893 (+ Grad-CAM 0.19 s)  0.61 s (0.32)  4      split_gemm0 893  0.42 s (0.34)  3
    fuse0 1785     0.84 s (0.67)  3      bf16_p3_unfused 893            0.50 s (0.35)  3      bf16_p3_unfused 1785  0.80 s (0.65)  3
  max_batch = 4096, 43.93 GB in 0.80 s:
    default 4096 (k5 taken, 16 rounds)  2.66 s (1.59)  3 - the worst case        bf16_p3_fused 4096  1.87 s (1.51)  3
  The whole file: 12 s.
"""
import time

import numpy as np
import pytest
import torch

import b0_batch_cases as B
import b0_layer_oracle as O

pytestmark = pytest.mark.gpu

CROP_BYTES = 3 * 224 * 224 * 4
SLAB = 256


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Rig:
    """the small reference handle, the one large handle that is open, and what was measured"""

    def __init__(self, pkg, sd):
        self.pkg, self.blob = pkg, pkg.weights.pack_b0(sd)
        self.x16 = B.crop_set()
        self.x16.setflags(write=False)
        self.small = pkg._lib.Handle(self.blob, device=0, max_batch=16)
        self.refs, self.big, self.size, self.footprint, self.oom, self.xbuf = {}, None, 0, {}, {}, None
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count

    def reference(self, cfg_name, names, gradcam):
        """{tensor: (16, row) float32} of the 16 crops in ONE call on the max_batch = 16 handle - computed once per
        configuration and tensor, never written again"""
        ref, h, cfg = self.refs.setdefault(cfg_name, {}), self.small, B.CONFIGS[cfg_name]
        need = [t for t in names if t not in ref] + (["heat"] if gradcam and "heat" not in ref else [])
        if not need:
            return ref
        xd, yd = h.alloc(self.x16.nbytes).upload(self.x16), h.alloc(16 * 4)
        try:
            for k, v in B.options(cfg).items():
                h.set_option(k, v)
            for t in need:
                if t == "logit":
                    h.classify_device(xd.ptr, 16, yd.ptr)
                    h.sync()
                    ref[t] = yd.download((16, 1))
                elif t == "heat":
                    hd = h.alloc(16 * 224 * 224 * 4)
                    try:
                        h.gradcam_device(xd.ptr, 16, yd.ptr, None, hd.ptr, None)
                        h.sync()
                        ref["heat"], ref["heat.logit"] = hd.download((16, 224 * 224)), yd.download((16, 1))
                    finally:
                        hd.free()
                else:
                    ref[t] = h.tap(xd.ptr, 16, t, O.tap_size(t, 16)).reshape(16, -1).copy()
            for a in ref.values():
                a.setflags(write=False)
        finally:
            for k, v in B.options(O.DEFAULT).items():
                h.set_option(k, v)
            xd.free()
            yd.free()
        return ref

    def handle(self, max_batch):
        """the large handle of this capacity: the previous one is closed first.  Out of memory in dfd_create is remembered
        (one attempt per handle) and skips the two large handles' cases; on the 512 handle it is a failure like any error"""
        if max_batch in self.oom:
            pytest.skip(self.oom[max_batch])
        if self.size != max_batch:
            self.close_big()
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            t0 = time.time()
            try:
                self.big = self.pkg._lib.Handle(self.blob, device=0, max_batch=max_batch)
            except self.pkg._lib.DfdError as e:
                if max_batch > 512 and "out of memory" in str(e).lower():
                    self.oom[max_batch] = f"dfd_create(max_batch={max_batch}) ran out of device memory ({free0 / 2 ** 30:.1f} GiB free): {e}"
                    print("\n[large_batch] " + self.oom[max_batch])
                    pytest.skip(self.oom[max_batch])
                raise
            self.size = max_batch
            self.footprint[max_batch] = free0 - torch.cuda.mem_get_info()[0]
            self.xbuf = self.big.alloc(max_batch * CROP_BYTES)
            print(f"\n[large_batch] handle max_batch={max_batch}: create_impl allocated {self.footprint[max_batch] / 1e9:.2f} GB "
                  f"in {time.time() - t0:.2f} s (+ {max_batch * CROP_BYTES / 1e9:.2f} GB for the test's input)")
        return self.big

    def close_big(self):
        if self.big is not None:
            self.xbuf.free()
            self.big.close()
        self.big, self.size, self.xbuf = None, 0, None

    def close(self):
        self.close_big()
        self.small.close()


@pytest.fixture(scope="module")
def rig(pkg, seeded_sd):
    r = Rig(pkg, seeded_sd)
    yield r
    r.close()


def _assert_rows(got, ref, idx, what):
    """row i of got == row idx[i] of ref, bit for bit, slab by slab; the failure names the first differing image"""
    n = idx.size
    got = got.reshape(n, -1)
    assert got.shape[1] == ref.shape[1], what
    step = max(1, min(SLAB, (160 << 20) // (4 * got.shape[1])))     # at most 160 MB of gathered reference rows at a time
    for s in range(0, n, step):
        a, b = _u32(got[s:s + step]), _u32(ref[idx[s:s + step]])
        if not np.array_equal(a, b):
            bad = np.flatnonzero((a != b).any(axis=1))
            i = s + int(bad[0])
            col = int(np.flatnonzero(a[bad[0]] != b[bad[0]])[0])
            total = sum(int((_u32(got[t:t + step]) != _u32(ref[idx[t:t + step]])).any(axis=1).sum()) for t in range(s, n, step))
            pytest.fail(f"{what}: {total} of {n} images differ from the 16-crop call, the first is image {i} (crop {idx[i]}), element {col} "
                        f"of {got.shape[1]}: {a[bad[0], col]:#010x} against {b[bad[0], col]:#010x}")


def _assert_reference_is_not_degenerate(ref, names):
    assert np.ptp(ref["logit"]) > 0.05
    for t in names:
        r = _u32(ref[t])
        assert all(not np.array_equal(r[i], r[j]) for i in range(16) for j in range(i)), f"{t}: two of the 16 reference rows are equal"


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: c.id)
def test_large_batch_equals_the_sixteen_crop_call(rig, case):
    assert 208 <= rig.cus <= 304, f"{rig.cus} CUs: the threshold cases (cu_count + 208 in the second round, on the 512 handle) need 208..304"
    cfg, n = B.CONFIGS[case.config], case.batch(rig.cus)
    claims = B.crossed(cfg, n, rig.cus)
    assert claims == case.claims
    names = ("logit", "feat", "b15.out") + tuple(t for t in case.taps if t != "b15.out")
    ref = rig.reference(case.config, names, case.gradcam)
    _assert_reference_is_not_degenerate(ref, names + (("heat",) if case.gradcam else ()))
    h = rig.handle(case.handle)
    t0 = time.time()
    idx = B.crop_index(n)
    for s in range(0, n, SLAB):                                   # the input, on the device, 154 MB of host crops at a time
        rig.xbuf.upload(rig.x16[idx[s:s + SLAB]], offset=s * CROP_BYTES)
    t_in = time.time() - t0
    xd, yd = rig.xbuf.ptr, h.alloc(n * 4)
    times = {}
    try:
        for k, v in B.options(cfg).items():
            h.set_option(k, v)
        # the plan around the k5 threshold: block 8's expanded tensor exists below it and not from it on
        if case.k5 is True:
            with pytest.raises(rig.pkg._lib.DfdError, match="not materialised"):
                h.tap(xd, n, "b8.exp", O.tap_size("b8.exp", n))
        elif case.k5 is False and "b8.exp" not in case.taps:
            assert h.tap(xd, n, "b8.exp", O.tap_size("b8.exp", n)).size == O.tap_size("b8.exp", n)
        for t in names:
            t1 = time.time()
            if t == "logit":
                h.classify_device(xd, n, yd.ptr)
                h.sync()
                got = yd.download((n, 1))
                assert np.ptp(got) > 0.05
            else:
                got = h.tap(xd, n, t, O.tap_size(t, n))
                assert got.size == O.tap_size(t, n), t
            _assert_rows(got, ref[t], idx, f"{case.id} n={n} {t}")
            times[t] = time.time() - t1
            del got
        if case.host_entries:
            # the entries that take HOST crops, themselves (the taps above are their device-input form): 155 MB at 257 crops
            t1 = time.time()
            xh = rig.x16[idx]
            assert xh.nbytes <= 160 << 20
            _assert_rows(h.classify(xh), ref["logit"], idx, f"{case.id} n={n} classify")
            _assert_rows(h.extract_features(xh), ref["feat"], idx, f"{case.id} n={n} extract_features")
            _assert_rows(h.extract_trunk(xh), ref["b15.out"], idx, f"{case.id} n={n} extract_trunk")
            times["host entries"] = time.time() - t1
            del xh
        if case.gradcam:
            t1 = time.time()
            hd = h.alloc(n * 224 * 224 * 4)
            try:
                h.gradcam_device(xd, n, yd.ptr, None, hd.ptr, None)
                h.sync()
                _assert_rows(yd.download((n, 1)), ref["heat.logit"], idx, f"{case.id} n={n} Grad-CAM logits")
                assert np.array_equal(_u32(ref["heat.logit"]), _u32(ref["logit"]))
                _assert_rows(hd.download((n, 224 * 224)), ref["heat"], idx, f"{case.id} n={n} Grad-CAM heatmaps")
            finally:
                hd.free()
            times["gradcam"] = time.time() - t1
    finally:
        for k, v in B.options(O.DEFAULT).items():
            h.set_option(k, v)
        yd.free()
    slow = max(times, key=times.get)
    print(f"\n[large_batch] {case.id}: n={n} on max_batch={case.handle} ({rig.footprint[case.handle] / 1e9:.2f} GB), crosses "
          f"{sorted(claims) if claims else 'no limit'}; k5 {'taken' if B.k5_taken(n, rig.cus) and not cfg.bf16 and cfg.fuse_late else 'not taken'}; "
          f"{len(times)} tensors equal to the 16-crop call; {time.time() - t0:.2f} s (input {t_in:.2f} s, slowest {slow} {times[slow]:.2f} s)")


def test_the_last_handle_is_closed_and_every_handle_reported(rig):
    rig.close_big()
    print(f"\n[large_batch] handles that ran: {sorted(rig.footprint)}; skipped for memory: {sorted(rig.oom)}")
    assert rig.big is None and 512 not in rig.oom
