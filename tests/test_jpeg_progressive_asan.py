"""CPU: the progressive JPEG parser and scan decoders (csrc/jpeg_entropy.h, csrc/jpeg_progressive.h - the functions a
device decoder would call as they stand) under AddressSanitizer + UBSan, through the stand-alone driver
csrc/host_asan_driver.cpp (`make -C csrc asan-host`; modes `pjpeg` and `pjpegfuzz`), run as a subprocess.  A memory error
or an undefined operation aborts the driver: every case must exit 0.  The corpus of tests/test_jpeg_progressive.py - sound,
scripted, refused and damaged files - and 3,000 seeded mutations of three progressive files."""
import os
import subprocess

import pytest

import jpeg_progressive_cases as PC
import jpeg_progressive_history  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "real-time-video-deepfake-detection_amd", "csrc")
DRIVER = os.path.join(ROOT, "real-time-video-deepfake-detection_amd", "host_asan_driver")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes in this image")
    subprocess.run(["make", "-C", CSRC, "asan-host"], check=True, capture_output=True)

    def run(*args):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        env.pop("DFD_JPEG_CHUNKS", None)
        r = subprocess.run([DRIVER, *map(str, args)], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, f"sanitizer report or crash for {args}:\n{r.stderr[-3000:]}"
        return dict(kv.split("=") for kv in r.stdout.split())
    return run


def test_sound_files_decode_clean(driver, tmp_path):
    for i, p in enumerate(PC.corpus() + PC.scripted()):
        f = tmp_path / f"sound{i}.jpg"
        f.write_bytes(p.progressive)
        out = driver("pjpeg", f)
        assert int(out["rc"]) == 0, (p.name, out)
        base = tmp_path / f"base{i}.jpg"
        base.write_bytes(p.baseline)
        ref = driver("jpeg", base)
        # the hash covers the geometry, the tables and every coefficient: those of the baseline file of the same pixels
        assert (out["count"], out["hash"]) == (ref["count"], ref["hash"]), p.name
        assert int(driver("jpeg", f)["rc"]) == -7                     # without the flag


def test_refused_and_damaged_files_are_rejected_clean(driver, tmp_path):
    for i, (name, data) in enumerate(PC.refused()):
        f = tmp_path / f"refused{i}.jpg"
        f.write_bytes(data)
        assert int(driver("pjpeg", f)["rc"]) == -7, name
    for i, (name, data, status) in enumerate(PC.crafted()):
        f = tmp_path / f"crafted{i}.jpg"
        f.write_bytes(data)
        assert int(driver("pjpeg", f)["rc"]) == status, name
    for i, (name, data) in enumerate(PC.damaged()):
        f = tmp_path / f"damaged{i}.jpg"
        f.write_bytes(data)
        ok = PC.walker_verdict(data)[0] is not None
        assert (int(driver("pjpeg", f)["rc"]) == 0) == ok, name


@pytest.mark.parametrize("name", ["37x53.420.restart3", "96x128.444.optimize", "17x33.gray.q100"])
def test_a_thousand_mutations_of_a_file_leave_the_sanitizers_silent(driver, tmp_path, name):
    f = tmp_path / "source.jpg"
    f.write_bytes(PC.by_name(name).progressive)
    out = driver("pjpegfuzz", f, 11, 1000)
    print(name, out)
    assert int(out["ok"]) + int(out["rejected"]) == 1000 and int(out["rejected"]) > 100 and int(out["ok"]) > 0
