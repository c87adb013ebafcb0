"""CPU: the case table of tests/test_b0_large_batch_gpu.py (tests/b0_batch_cases.py) crosses what it claims.

Every case states, completely, which activation tensors reach 2^31 bytes, 2^32 bytes or 2^31 elements at its batch;
here that statement is recomputed from b0_arch.BLOCKS and the configuration's launch plan.  A case size moved below
the limit it claims, or a block table that moves a limit past a case, fails here instead of leaving the GPU test
running below the limit it was written for.  Also: the limits the table is built on, the plan threshold around the CU
count, the handle each case fits, and the properties of the crop pattern at every case size."""
import numpy as np
import pytest

import b0_batch_cases as B
import b0_layer_oracle as O

# the nominal count and both ends of the range the 512 handle's threshold cases allow: cu_count + 208 is in the SECOND
# round from 208 CUs on and fits the handle up to 304 (the GPU test asserts the device's count is in that range)
CUS = (B.NOMINAL_CUS, 304, 208)


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: c.id)
def test_case_crosses_what_it_claims_and_nothing_else(case):
    got = B.crossed(B.CONFIGS[case.config], case.batch())
    assert got == case.claims, f"claimed but not crossed {sorted(case.claims - got)}, crossed but not claimed {sorted(got - case.claims)}"
    assert 256 < case.batch() <= case.handle <= 4096
    # the case sits AT the limits it names: a few crops fewer and its newest crossing is gone (the sizes are the first n
    # past a limit, plus one where two limits coincide)
    if case.claims and case.n is not None and case.n != 4096:
        assert B.crossed(B.CONFIGS[case.config], case.n - 2) != case.claims


def test_first_crossings_match_the_figures_the_cases_were_chosen_from():
    f = B.tensors(B.CONFIGS["fuse0"])
    b = B.tensors(B.CONFIGS["bf16_p3_unfused"])
    d = B.tensors(B.CONFIGS["default"])
    assert f["input"] == (150528, 4) and f["stem"] == f["b0.dw"] == (401408, 4) and f["b1.exp"] == (1204224, 4)
    assert f["b2.exp"] == f["b3.exp"] == f["b2.dw"] == (451584, 4) and f["b1.dw"] == (301056, 4)
    first = lambda t, lim: B.first_n(*t, lim)
    assert [first(f["input"], k) for k in B.LIMITS] == [3567, 7134, 14267]
    assert [first(f["b0.dw"], k) for k in B.LIMITS] == [1338, 2675, 5350]
    assert [first(f["b1.exp"], k) for k in B.LIMITS] == [446, 892, 1784]
    assert [first(f["b2.exp"], k) for k in B.LIMITS][:2] == [1189, 2378]
    assert [first(f["b1.dw"], k) for k in B.LIMITS][:2] == [1784, 3567]
    assert [first(b["b1.exp"], k) for k in B.LIMITS] == [892, 1784, 1784]       # bf16 storage: the byte limits double
    # what a configuration does not write is not in its table
    assert "stem" not in d and "b0.out" not in d and "b1.exp" not in d and "b0.out" in B.tensors(B.CONFIGS["split_gemm0"])
    assert "b8.exp" in d and "b8.exp" not in B.tensors(B.CONFIGS["default"], B.NOMINAL_CUS + B.K5_MIN)
    assert "b8.exp" in B.tensors(B.CONFIGS["bf16_p3_fused"], B.NOMINAL_CUS + B.K5_MIN)


def test_every_limit_the_largest_tensors_reach_is_claimed_by_some_case():
    """every (configuration, tensor, limit) that is crossed anywhere up to 4096 crops: listed, with the first batch, so
    the table of DESIGN.md can be checked against this output; the five configurations the cases use must reach, in
    some case, every limit their LARGEST tensor crosses"""
    for name in ("default", "fuse0", "split_gemm0", "bf16_p3_unfused", "bf16_p3_fused"):
        cfg = B.CONFIGS[name]
        for t, (el, esz) in B.tensors(cfg).items():
            hits = {lim: B.first_n(el, esz, lim) for lim in B.LIMITS if B.first_n(el, esz, lim) <= 4096}
            if hits:
                print(f"{name:16s} {t:8s} {el * esz:9d} B/image  " + "  ".join(f"{k} at {v}" for k, v in hits.items()))
    claimed = {(c.config, t, lim) for c in B.CASES for t, lim in c.claims}
    for cfg, t in (("fuse0", "b1.exp"), ("bf16_p3_unfused", "b1.exp"), ("default", "b0.dw"), ("default", "input")):
        el, esz = B.tensors(B.CONFIGS[cfg])[t]
        for lim in B.LIMITS:
            if B.first_n(el, esz, lim) <= 4096:
                assert (cfg, t, lim) in claimed, (cfg, t, lim)


@pytest.mark.parametrize("cus", CUS)
def test_threshold_cases_sit_on_either_side_of_the_plan_switch(cus):
    below, at = (c for c in B.CASES if c.n is None)
    assert below.k5 is False and at.k5 is True and at.batch(cus) == below.batch(cus) + 1 == cus + B.K5_MIN
    assert not B.k5_taken(below.batch(cus), cus) and B.k5_taken(at.batch(cus), cus)
    assert -(-at.batch(cus) // cus) == 2, "the switch must happen in the SECOND round of one-block-per-image launches"
    assert at.batch(cus) <= at.handle
    cfg = B.CONFIGS["default"]
    assert "b8.exp" in B.tensors(cfg, below.batch(cus), cus) and "b8.exp" not in B.tensors(cfg, at.batch(cus), cus)
    assert "b8.exp" in below.taps                      # the GPU test reads the tap where it exists, expects the refusal where not
    # one image past a full round: the older forms, like every batch from cu_count + 1 to cu_count + 207
    assert not B.k5_taken(cus + 1, cus) and B.k5_taken(cus, cus)
    assert B.CASES[0].n == 257 and B.CASES[0].k5 is False and not B.k5_taken(257, B.NOMINAL_CUS)


def test_options_leave_the_mask_unset_for_the_default_plan():
    assert B.options(B.CONFIGS["default"])["fuse_late_skip"] == -1
    assert B.options(B.CONFIGS["late_all"])["fuse_late_skip"] == 0
    assert B.options(B.CONFIGS["fuse0"])["fuse_expand"] == 0


@pytest.mark.parametrize("n", sorted({c.batch(cu) for c in B.CASES for cu in CUS} | {16}))
def test_crop_pattern(n):
    idx = B.crop_index(n)
    assert idx.shape == (n,) and idx.min() == 0 and idx.max() == 15
    assert np.array_equal(idx[:16], (5 * np.arange(16)) % 16)
    assert set(idx[:16]) == set(range(16)) and set(idx[-16:]) == set(range(16))
    assert (idx[1:] != idx[:-1]).all()
    if n >= 257:
        for m in (4, 8, 16):
            for r in range(m):
                assert set(idx[r::m]) == set(range(16)), (m, r)


def test_crop_set_is_sixteen_different_crops():
    x = B.crop_set()
    assert x.shape == (16, 3, 224, 224) and x.dtype == np.float32
    assert np.array_equal(x[:9], O.random_crops(9)) and np.array_equal(x[9:], O.edge_crops())
    flat = x.reshape(16, -1)
    assert all(not np.array_equal(flat[i], flat[j]) for i in range(16) for j in range(i))
