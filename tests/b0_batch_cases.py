"""Large-batch cases of the classifier (tests/test_b0_large_batch_gpu.py) and the arithmetic that justifies them
(tests/test_b0_batch_cases.py, CPU).

dfd_create accepts max_batch up to 4096.  Between the 256 crops the rest of the suite stops at and that cap
  * the launch plan changes with n against the CU count (mbconv_k5_kernel: one block per image, taken when the last
    round of cu_count blocks holds at least K5_MIN images), and
  * activation tensors cross 2^31 bytes, 2^32 bytes and 2^31 elements - where a 32-bit index or byte offset wraps.
`tensors` derives, from b0_arch.BLOCKS and a b0_layer_oracle.Config, every activation tensor the configuration writes
to HBM with its elements per image and bytes per element; `first_n` the first batch at which a tensor reaches a limit;
`crossed` what a (configuration, batch) crosses.  Every case names what it claims to cross, completely: the CPU test
asserts claims == crossed, so a change to the block table or to a case size cannot quietly empty the GPU test.

The crop pattern: crop i of a large batch is crop IDX(i) of a fixed 16-crop set (b0_layer_oracle's 9 random_crops and
7 edge_crops), so the expected row i is row IDX(i) of ONE 16-crop call - bit for bit, no tolerance."""
import dataclasses
from typing import Dict, FrozenSet, Optional, Tuple

import numpy as np

import b0_layer_oracle as O
from rtdfd_amd import b0_arch

K5_MIN = 208                    # b0_plan.hip K5_MIN_DEFAULT
K5_BLOCKS = range(6, 12)        # blocks mbconv_k5_kernel has an instance for (fp32 storage, "fuse_k5" on: the default)
NOMINAL_CUS = 256               # MI355X; the GPU test reads the device's count and asserts its cases still fit
LIMITS = {"2^31 B": ("bytes", 1 << 31), "2^32 B": ("bytes", 1 << 32), "2^31 el": ("elements", 1 << 31)}

CONFIGS = {c.name: c for c in O.FP32_CONFIGS + O.BF16_CONFIGS}


def options(cfg: O.Config) -> Dict[str, int]:
    """Config.options with the late-block mask UNSET (-1) where the configuration keeps the default mask: an explicit
    mask of the same bits pins blocks 8 and 9 to their separate launches at every batch, the unset one lets
    mbconv_k5_kernel take them from the threshold on - the plan a handle nobody configured runs"""
    o = cfg.options()
    if o["fuse_late_skip"] == O.DEFAULT_LATE_SKIP:
        o["fuse_late_skip"] = -1
    return o


def k5_taken(n: int, cu_count: int) -> bool:
    """b0_forward_t: the images of the last round of one-block-per-image launches reach the threshold"""
    rounds = -(-n // cu_count)
    return n - (rounds - 1) * cu_count >= K5_MIN


def expand_fused(cfg: O.Config, i: int, n: int, cu_count: int) -> bool:
    """Config.expand_fused, plus the batch-dependent part of the plan: with the default options mbconv_k5_kernel takes
    blocks 6-11 - the masked blocks 8 and 9 and block 11, which have no other fused form, included - when k5_taken"""
    if cfg.expand_fused(i):
        return True
    k5 = (not cfg.bf16 and cfg.fuse_expand and cfg.fuse_late and i in K5_BLOCKS and k5_taken(n, cu_count)
          and cfg.fuse_late_skip == O.DEFAULT_LATE_SKIP)
    return bool(k5)


def tensors(cfg: O.Config, n: int = 1, cu_count: int = NOMINAL_CUS) -> Dict[str, Tuple[int, int]]:
    """{tensor: (elements per image, bytes per element)} of every activation tensor the forward of `cfg` writes to HBM
    at batch n.  The input is fp32 in every configuration; bf16 storage halves the rest; "stem" exists only where the
    stem runs as its own launch, "b<i>.exp" only where the expand does, and "b0.out" not where block 1's launch
    computes block 0's projection ("fuse_proj0": fp32, split GEMM, expand fused).  The per-image vectors (gate, feat,
    fc1, fc2, logit: at most 1280 floats) and the pool partial sums stay far below every limit and are left out."""
    esz = 2 if cfg.bf16 else 4
    out = {"input": (3 * b0_arch.IMAGE_SIZE ** 2, 4)}
    if not cfg.fuse_stem:
        out["stem"] = (b0_arch.BLOCKS[0].h_in ** 2 * b0_arch.STEM_OUT, esz)
    proj0 = not cfg.bf16 and cfg.fuse_expand and cfg.split_gemm
    for b in b0_arch.BLOCKS:
        i = b.index
        if b.expand != 1 and not expand_fused(cfg, i, n, cu_count):
            out[f"b{i}.exp"] = (b.h_in ** 2 * b.c_exp, esz)
        out[f"b{i}.dw"] = (b.h_out ** 2 * b.c_exp, esz)
        if not (i == 0 and proj0):
            out[f"b{i}.out"] = (b.h_out ** 2 * b.c_out, esz)
    out["head"] = (b0_arch.BLOCKS[-1].h_out ** 2 * b0_arch.HEAD_OUT, esz)
    return out


def first_n(elements: int, esz: int, limit: str) -> int:
    """the first batch at which a tensor of `elements` per image reaches the limit (the value a 32-bit count wraps at)"""
    unit, value = LIMITS[limit]
    per = elements * esz if unit == "bytes" else elements
    return -(-value // per)


def crossed(cfg: O.Config, n: int, cu_count: int = NOMINAL_CUS) -> FrozenSet[Tuple[str, str]]:
    """every (tensor, limit) the forward of `cfg` at batch n reaches"""
    return frozenset((name, lim) for name, (el, esz) in tensors(cfg, n, cu_count).items() for lim in LIMITS
                     if n >= first_n(el, esz, lim))


# ------------------------------------------------------------------------------------------------ crop pattern
def crop_set() -> np.ndarray:
    """(16, 3, 224, 224): the 9 random crops and the 7 edge crops of b0_layer_oracle"""
    return np.concatenate([O.random_crops(9), O.edge_crops()]).astype(np.float32)


def crop_index(n: int) -> np.ndarray:
    """idx[i] = (5 i + min(i // 16, n // 16 - 1)) % 16: row b of 16 images is the permutation 5 r shifted by b.  5 is a
    unit mod 16, so a row holds 16 different crops and neighbours differ by 5 (by 6 or 11 across a row border); the
    shift walks through all 16 values in 16 rows, so from 256 images on a fixed position mod 16 (hence mod 8 and mod 4)
    meets every crop.  With the plain shift i // 16 the LAST 16 images of a ragged batch straddle two rows with
    different shifts and repeat crops; the ragged last row therefore keeps the shift of the row before it, and the
    two together hold one whole permutation.  test_b0_batch_cases.py asserts all of this for every case size."""
    i = np.arange(n)
    return (5 * i + np.minimum(i // 16, n // 16 - 1)) % 16


# ------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class Case:
    handle: int                             # max_batch of the handle the case runs on
    config: str                             # b0_layer_oracle configuration
    n: Optional[int]                        # batch; None: cu_count + cu_offset
    claims: FrozenSet[Tuple[str, str]]      # every (tensor, limit) the forward crosses - complete
    cu_offset: int = 0
    k5: Optional[bool] = None               # the plan it must meet: mbconv_k5_kernel taken or not (fp32 defaults only)
    taps: Tuple[str, ...] = ()              # further taps compared whole
    gradcam: bool = False
    host_entries: bool = False              # also through classify / extract_features / extract_trunk from HOST crops

    def batch(self, cu_count: int = NOMINAL_CUS) -> int:
        return self.n if self.n is not None else cu_count + self.cu_offset

    @property
    def id(self) -> str:
        return f"{self.config}-{self.n if self.n is not None else 'cu+%d' % self.cu_offset}"


def _c(*pairs):
    return frozenset((t, lim) for names, lims in pairs for t in names.split() for lim in lims.split(", "))


B31, B32, E31 = "2^31 B", "2^31 B, 2^32 B", "2^31 B, 2^32 B, 2^31 el"
TAPS512 = ("b1.out", "b5.out", "b10.out", "b15.out", "b8.dw")
# 1.6 MB per image: stem / b0.dw (112 x 112 x 32); 1.8 MB: b2.exp, b2.dw (56 x 56 x 144) and b3.exp; 1.2 MB: b1.dw
CASES = (
    # one round plus one image: the second round holds a single block; k5 not taken (1 < 208)
    Case(512, "default", 257, _c(), k5=False, taps=TAPS512, gradcam=True, host_entries=True),
    # the threshold of the second round, either side
    Case(512, "default", None, _c(), cu_offset=K5_MIN - 1, k5=False, taps=TAPS512 + ("b8.exp",)),
    Case(512, "default", None, _c(), cu_offset=K5_MIN, k5=True, taps=TAPS512),
    Case(512, "fuse0", 447, _c(("b1.exp", B31)), taps=TAPS512 + ("b1.exp",)),
    Case(1792, "default", 1339, _c(("b0.dw", B31), ("b2.dw", B31))),
    Case(1792, "fuse0", 893, _c(("b1.exp", B32)), gradcam=True),
    Case(1792, "split_gemm0", 893, _c()),
    Case(1792, "fuse0", 1785, _c(("b1.exp", E31), ("stem b0.dw b1.dw b2.exp b2.dw b3.exp", B31))),
    Case(1792, "bf16_p3_unfused", 893, _c(("b1.exp", B31))),
    Case(1792, "bf16_p3_unfused", 1785, _c(("b1.exp", E31))),       # (2 bytes per element: 2^32 B and 2^31 elements coincide)
    # (b4.dw: 28 x 28 x 240, 0.75 MB per image; b9.dw, b10.dw: 14 x 14 x 672, 0.53 MB - 2^31 B at 4077 crops)
    Case(4096, "default", 4096, _c(("input", B31), ("b0.dw b1.dw b2.dw", B32), ("b4.dw b9.dw b10.dw", B31))),
    Case(4096, "bf16_p3_fused", 4096, _c(("input b0.dw b1.dw b2.dw", B31))),
)
HANDLES = (512, 1792, 4096)
