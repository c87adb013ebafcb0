"""GPU: the device entropy decoder (csrc/jpeg_gpu_entropy.h) on files whose entropy-coded data is wrong INSIDE a block -
the corpus of tests/jpeg_damage_cases.py, built by construction: an unassigned Huffman code, a coefficient index past 63
or a DC category above 11 in one block of the first, an interior, the second-to-last or the last chunk of the lanes' grid
(or the only one), ZRLs that run past 63, zeroed padding bits, bytes between the last block and EOI, cut scans.

DESIGN 4d: the device decoder only vouches for a frame, the host decoder stays the arbiter of anything irregular.  So for
every file the outcome with the device decoder (option "jpeg_device_entropy" 1) equals the outcome with the host decoder
(0) - the same exception type and code, or the same pixels bit for bit - and both equal the verdict of the sequential
walker (tests/jpeg_walker.py); accepted files equal Pillow's decode.  jpeg_decode_counts() says who decoded: a rejected
file is never counted for the device, an accepted one of these always is."""
import numpy as np
import pytest

import frames as F
import jpeg_damage_cases as D
import jpeg_stream_cases as C
import jpeg_walker as W

pytestmark = pytest.mark.gpu

_walked = {}


def walked(data):
    if data not in _walked:
        _walked[data] = W.walk(data)
    return _walked[data]


class _device:
    """the device entropy decoder always, 16 rounds, the chunk size asked for; the defaults afterwards"""

    def __init__(self, h, chunk=None, restart=False):
        self.h, self.chunk, self.restart = h, chunk, restart

    def __enter__(self):
        self.h.set_option("jpeg_device_entropy", 1)
        self.h.set_option("jpeg_rounds", 16)
        self.h.set_option("jpeg_device_restart", 1 if self.restart else 0)
        if self.chunk:
            self.h.set_option("jpeg_chunk_bytes", self.chunk)
        return self.h

    def __exit__(self, *exc):
        self.h.set_option("jpeg_device_restart", 0)
        self.h.set_option("jpeg_device_entropy", 2)
        self.h.set_option("jpeg_chunk_bytes", 512)
        self.h.set_option("jpeg_rounds", 16)
        return False


class _host:
    def __init__(self, h):
        self.h = h

    def __enter__(self):
        self.h.set_option("jpeg_device_entropy", 0)
        return self.h

    def __exit__(self, *exc):
        self.h.set_option("jpeg_device_entropy", 2)
        return False


def _outcome(pkg, h, datas):
    try:
        return ("pixels", [a.copy() for a in h.decode_jpeg_batch(datas)])
    except pkg._lib.DfdError as e:
        return ("error", type(e), e.code)


def _counted(pkg, h, datas):
    d0, h0 = h.jpeg_decode_counts()
    out = _outcome(pkg, h, datas)
    d1, h1 = h.jpeg_decode_counts()
    return out, (d1 - d0, h1 - h0)


def _same(a, b):
    return a[0] == b[0] and (a[1:] == b[1:] if a[0] == "error" else all(np.array_equal(x, y) for x, y in zip(a[1], b[1])))


def _check(case, datas, on, moved, off):
    """one call that holds the case: the device decoder's outcome `on` and counts `moved` against the host
    decoder's outcome `off` and the walker's verdict"""
    res = walked(case.data)
    print(f"{case.id}: walker {type(res).__name__}, host {off[0]} {off[2] if off[0] == 'error' else ''}, "
          f"device {on[0]} {on[2] if on[0] == 'error' else ''}, (device, host) counts {moved}")
    assert _same(on, off), f"{case.id}: device decoder {on[0]} {on[1:] if on[0] == 'error' else ''}, host decoder {off[0]}"
    if isinstance(res, W.Ok):
        assert on[0] == "pixels", (case.id, on)
        for i, d in enumerate(datas):
            assert np.array_equal(on[1][i], D.pillow(d)), (case.id, i)
        assert moved == (len(datas), 0), (case.id, moved)           # decoded on the device, not quietly handed over
    else:
        assert on[0] == "error" and on[2] == -1, (case.id, on)
        assert moved[0] == 0, (case.id, moved)                      # a rejected file is never counted for the device


def _healthy_after(pkg, h, key, what):
    good = D.healthy(key)
    out, moved = _counted(pkg, h, good)
    assert out[0] == "pixels" and moved == (3, 0), (what, out[0], moved)
    for i in range(3):
        assert np.array_equal(out[1][i], D.pillow(good[i])), (what, i)


PLAIN_CASES = [c for c in D.cases() if c.base != "restart"]
RESTART_CASES = [c for c in D.cases() if c.base == "restart"]


@pytest.mark.parametrize("opt", D.OPTIONS)
@pytest.mark.parametrize("case", PLAIN_CASES, ids=lambda c: c.id)
def test_damaged_file_alone_and_in_a_batch(pkg, b0_handle, case, opt):
    """the file alone and between two healthy files of its size and sampling: device == host == walker, accepted files
    equal Pillow and are counted for the device; afterwards a healthy batch of three decodes on the device, (3, 0)"""
    h = b0_handle
    good = D.healthy(case.healthy)
    batch = [good[1], case.data, good[2]]
    with _host(h):
        off_alone, off_batch = _outcome(pkg, h, [case.data]), _outcome(pkg, h, batch)
    with _device(h, opt):
        on_alone, moved_alone = _counted(pkg, h, [case.data])
        on_batch, moved_batch = _counted(pkg, h, batch)
        _check(case, [case.data], on_alone, moved_alone, off_alone)
        _check(case, batch, on_batch, moved_batch, off_batch)
        _healthy_after(pkg, h, case.healthy, case.id)


@pytest.mark.parametrize("opt", D.OPTIONS)
@pytest.mark.parametrize("case", RESTART_CASES, ids=lambda c: c.id)
def test_damage_in_the_last_restart_segment(pkg, b0_handle, case, opt):
    """index and code damage in the last segment of a restart-interval file through the RST = true kernels (option
    "jpeg_device_restart" 1): the outcome of the option off (the host decoder), alone and in a batch"""
    h = b0_handle
    good = D.healthy(case.healthy)
    batch = [good[1], case.data, good[2]]
    with _device(h, opt, restart=False):                            # option off: restart files take the host path
        off_alone, m0 = _counted(pkg, h, [case.data])
        off_batch, m1 = _counted(pkg, h, batch)
        assert m0[0] == 0 and m1[0] == 0
    with _device(h, opt, restart=True):
        on_alone, moved_alone = _counted(pkg, h, [case.data])
        on_batch, moved_batch = _counted(pkg, h, batch)
        _check(case, [case.data], on_alone, moved_alone, off_alone)
        _check(case, batch, on_batch, moved_batch, off_batch)
        _healthy_after(pkg, h, case.healthy, case.id)


def test_damaged_row_next_to_a_file_that_needs_the_second_pass(pkg, b0_handle, monkeypatch, capfd):
    """a batch with a frame that is not at the fixed point after the rounds gets one more pass, with the round
    kernel that also iterates inside a launch (the RST = true instantiation).  A `reversed-420` file (72 x 104) needs it;
    the frame next to it, damaged in its last chunk, is judged by that pass: index damage is still rejected, a ZRL run
    past 63 is still accepted, and the reversed file still equals Pillow"""
    h = b0_handle
    rev = C.files("reversed-420")[0].data
    bad, healthy = D.damaged_frame(D._img(72, 104, 31), 90, "index", "lastchunk", 256)
    zrl, _ = D.damaged_frame(D._img(72, 104, 31), 90, "zrl", "lastchunk", 256)
    assert isinstance(walked(bad), W.Defect) and isinstance(walked(zrl), W.Ok)
    monkeypatch.setenv("DFD_JPEG_VERBOSE", "1")
    with _host(h):
        off = _outcome(pkg, h, [rev, bad])
    with _device(h, 256):
        capfd.readouterr()
        on, moved = _counted(pkg, h, [rev, bad])
        assert "second pass" in capfd.readouterr().err
        assert _same(on, off) and on[0] == "error" and on[2] == -1 and moved[0] == 0, (on, off, moved)
        for other in (zrl, healthy):
            capfd.readouterr()
            on, moved = _counted(pkg, h, [rev, other])
            assert "second pass" in capfd.readouterr().err
            assert on[0] == "pixels" and moved == (2, 0), (on[0], moved)
            assert np.array_equal(on[1][0], C.pillow("reversed-420")[0]) and np.array_equal(on[1][1], D.pillow(other))


def test_analyze_jpegs_host_rejects_a_frame_damaged_in_its_last_chunk(pkg, seeded_sd):
    """dfd_analyze_jpegs_host always takes the device decoder: with one frame of five index-damaged in its last chunk the
    call fails with the host decoder's code, and the same five healthy frames are analysed afterwards"""
    Wt = pkg.weights
    h = pkg._lib.Handle(Wt.pack_all(seeded_sd, Wt.seeded_ssd_state_dict(0)), device=0, max_batch=16)
    try:
        h.set_option("jpeg_chunk_bytes", 256)
        pairs = [D.damaged_frame(F.natural_like(270, 480, seed=260 + i), 85, "index", "lastchunk", 256) for i in range(5)]
        good = [p[1] for p in pairs]
        datas = good[:3] + [pairs[3][0]] + good[4:]
        assert isinstance(walked(datas[3]), W.Defect)
        with pytest.raises(pkg._lib.DfdError) as host:
            pkg._lib.jpeg_coefficients(datas[3])
        boxes = [[(40, 30, 120, 140), (250, 60, 160, 180)]] * 5
        d0, h0 = h.jpeg_decode_counts()
        with pytest.raises(pkg._lib.DfdError) as e:
            h.analyze_jpegs_host(datas, 3, forced_boxes=boxes, max_faces=2, with_forensics=True)
        assert e.value.code == host.value.code == -1
        decoded = np.stack([D.pillow(d) for d in good])
        fd = h.alloc(decoded.nbytes).upload(decoded)
        want = h.analyze_batch_device(fd.ptr, 5, 270, 480, forced_boxes=boxes, max_faces=2, with_forensics=True)
        fd.free()
        d0, h0 = h.jpeg_decode_counts()
        got = h.analyze_jpegs_host(good, 3, forced_boxes=boxes, max_faces=2, with_forensics=True)
        assert h.jpeg_decode_counts() == (d0 + 5, h0)
        assert got[3] == (270, 480) and got[0] == want[0]
        assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1])) and np.array_equal(got[2], want[2])
    finally:
        h.close()
