"""CPU: the public surface of the any-size frequency-domain path - the detector's methods, the five C entry points in
binding, header and library, and the size check of compute_frequency_features (a pure function, run before any handle)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dfd_frequency_domain", "dfd_frequency_domain_device", "dfd_frequency_domain_tap", "dfd_frequency_features_sized",
       "dfd_frequency_features_tap")


def test_detector_has_the_reference_method(pkg):
    d = pkg.deepfake_detection.DeepfakeDetector
    assert callable(getattr(d, "analyze_frequency_domain", None))
    assert callable(getattr(d, "analyze_frequency_domain_boxes", None))


def test_handle_has_the_entries(pkg):
    for name in ("frequency_domain", "frequency_domain_device", "frequency_domain_tap", "frequency_features", "frequency_features_tap"):
        assert callable(getattr(pkg._lib.Handle, name, None)), name


def test_entry_points_in_binding_header_and_library(pkg):
    src = open(os.path.join(ROOT, "include", "dfd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dfd_[a-z0-9_]+)\s*\(", src))
    if not os.path.exists(pkg._lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = pkg._lib.load()
    for name in NEW:
        assert name in pkg._lib.SIGNATURES, name
        assert name in declared, name
        assert hasattr(lib, name), name
    assert "#define DFD_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "dfd_hip.h")).read() or lib.dfd_abi_version() == 1
    assert lib.dfd_abi_version() == 1


def test_verdict_is_taken_in_double_on_the_host(pkg):
    v = pkg.deepfake_detection.DeepfakeDetector._frequency_verdict
    assert v(0.0, 100.0) == 0.15 and v(14.9999999, 100.0) == 0.15
    assert v(15.0, 100.0) == 0.15                                  # 15 / (100 + 1e-10) is below 0.15 in double, as in the reference
    assert v(15.0000001, 100.0) == 0.0 and v(100.0, 100.0) == 0.0
    assert v(0.0, 0.0) == 0.15                                     # 0 / 1e-10, as the reference computes an all-zero crop


def test_check_frequency_size(pkg, monkeypatch):
    check = pkg.model.check_frequency_size
    assert check(224) == 224 and check(224, False) == 224 and check(224, True) == 224
    with pytest.raises(ValueError):
        check(128)
    with pytest.raises(ValueError):
        check(128, False)
    for s in (2, 126, 1024, 128):
        assert check(s, True) == s
    for s in (127, 0, 1026, -2, 1):
        with pytest.raises(ValueError):
            check(s, True)


def test_size_check_runs_before_any_handle(pkg, monkeypatch):
    """the check needs no handle: a refused size raises ValueError even with a handle that cannot be used, and the
    environment variable is read when any_size is None"""
    import numpy as np

    class NoHandle:
        def frequency_features(self, image, size=224):
            return ("called", size)

    img = np.zeros((8, 8, 3), np.uint8)
    f = pkg.model.compute_frequency_features
    monkeypatch.delenv("DFD_FREQ_ANY_SIZE", raising=False)
    with pytest.raises(ValueError):
        f(img, size=128, handle=NoHandle())
    assert f(img, size=224, handle=NoHandle()) == ("called", 224)
    assert f(img, size=128, any_size=True, handle=NoHandle()) == ("called", 128)
    with pytest.raises(ValueError):
        f(img, size=127, any_size=True, handle=NoHandle())
    monkeypatch.setenv("DFD_FREQ_ANY_SIZE", "1")
    assert f(img, size=128, handle=NoHandle()) == ("called", 128)
    with pytest.raises(ValueError):
        f(img, size=128, any_size=False, handle=NoHandle())           # the argument wins over the variable
    with pytest.raises(ValueError):
        f(img, size=1026, handle=NoHandle())
    monkeypatch.setenv("DFD_FREQ_ANY_SIZE", "0")
    with pytest.raises(ValueError):
        f(img, size=128, handle=NoHandle())
