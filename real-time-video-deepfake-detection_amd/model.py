"""Host mirror of the reference's ``model.py`` over the HIP classifier.

`DeepfakeEfficientNet` keeps the constructor and call surface of reference
model.py:21-102 (``forward(rgb, freq=None) -> (B,1)`` logits, ``extract_features ->
(B,1280)``, ``forward_with_projection``); the arithmetic runs in libdfd_hip.so
(`dfd_classify_nchw`, include/dfd_hip.h).  The forward is the reference's ``.eval()``
path; `fit_head` trains the MLP head on the device with the backbone frozen
(head_training.py).  There is no CPU implementation behind either.
"""
from __future__ import annotations

import logging
import os
from typing import Dict, Mapping, Optional

import numpy as np

from . import b0_arch as A
from . import weights as W
from ._lib import DfdError, Handle

log = logging.getLogger(__name__)


class _LayerInfo:
    """Shape-only stand-in for one entry of the reference's ``net._fc`` Sequential."""

    def __init__(self, kind: str, **kw):
        self.kind = kind
        self.__dict__.update(kw)

    def __repr__(self):
        return f"{self.kind}({', '.join(f'{k}={v}' for k, v in self.__dict__.items() if k != 'kind')})"


def _fc_layout(dropout: float):
    d = A.MLP_DIMS
    return [
        _LayerInfo("Dropout", p=dropout),
        _LayerInfo("Linear", in_features=d[0], out_features=d[1]),
        _LayerInfo("BatchNorm1d", num_features=d[1]),
        _LayerInfo("ReLU"),
        _LayerInfo("Dropout", p=dropout * 0.7),
        _LayerInfo("Linear", in_features=d[1], out_features=d[2]),
        _LayerInfo("BatchNorm1d", num_features=d[2]),
        _LayerInfo("ReLU"),
        _LayerInfo("Dropout", p=dropout * 0.5),
        _LayerInfo("Linear", in_features=d[2], out_features=d[3]),
    ]


class _NetInfo:
    def __init__(self, dropout):
        self._fc = _fc_layout(dropout)      # reference model.py:50-61 (10 entries)
        self._conv_head = _LayerInfo("Conv2d", in_channels=320, out_channels=A.HEAD_OUT, kernel_size=1)


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class DeepfakeEfficientNet:
    """EfficientNet-B0 + 1280->512->256->1 head, executed on one MI355X.

    Args mirror reference model.py:36: ``pretrained`` is accepted for signature
    parity (the reference fetches ImageNet weights there; this build has no
    network and starts from `weights.seeded_state_dict(seed)` until
    `load_state_dict` is called), ``dropout`` only shapes the reported head.
    """

    def __init__(self, pretrained: bool = True, dropout: float = 0.5, *, device: int = 0,
                 max_batch: int = 8, seed: int = 0, state_dict: Optional[Mapping[str, np.ndarray]] = None):
        self.net = _NetInfo(dropout)
        self.device_index = int(device)
        self.max_batch = int(max_batch)
        self.training = False
        self._handle: Optional[Handle] = None
        self._state: Dict[str, np.ndarray] = dict(state_dict) if state_dict is not None else W.seeded_state_dict(seed)
        if pretrained and state_dict is None:
            log.info("pretrained=True: no ImageNet weights offline; using seeded random init (seed=%d)", seed)

    # ---- torch.nn.Module look-alikes used by the reference call sites
    def train(self, mode: bool = True):
        """signature parity only: the forward is always the eval path; training goes through `fit_head`"""
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, *_a, **_k):
        return self

    def parameters_count(self) -> int:
        return A.param_count()

    def state_dict(self) -> Dict[str, np.ndarray]:
        return dict(self._state)

    def load_state_dict(self, state: Mapping, strict: bool = False):
        """reference deepfake_detection.py:44-59: returns (missing, unexpected) key lists."""
        new = {k: (v.detach().cpu().numpy() if _is_torch(v) else np.asarray(v)) for k, v in state.items()}
        want = set(self._state)
        missing = sorted(k for k in want - set(new) if not k.endswith("num_batches_tracked"))
        unexpected = sorted(set(new) - want)
        if strict and (missing or unexpected):
            raise KeyError(f"missing={missing[:5]} unexpected={unexpected[:5]}")
        for k in want & set(new):
            if new[k].shape != self._state[k].shape:
                raise ValueError(f"shape mismatch for {k}: {new[k].shape} vs {self._state[k].shape}")
            self._state[k] = new[k]
        if self._handle is not None:
            self._handle.close()
            self._handle = None
        return missing, unexpected

    # ---- device
    @property
    def handle(self) -> Handle:
        if self._handle is None:
            self._handle = Handle(W.pack_b0(self._state), device=self.device_index, max_batch=self.max_batch)
        return self._handle

    def _run(self, x, fn):
        torch_in = _is_torch(x)
        a = x.detach().cpu().numpy() if torch_in else np.asarray(x)
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 4 or a.shape[1:] != (3, A.IMAGE_SIZE, A.IMAGE_SIZE):
            raise ValueError(f"expected (B,3,224,224), got {a.shape}")
        outs = []
        for i in range(0, a.shape[0], self.max_batch):
            outs.append(fn(a[i:i + self.max_batch]))
        out = np.concatenate(outs, axis=0)
        if torch_in:
            import torch

            return torch.from_numpy(out)
        return out

    def forward(self, rgb_input, freq_input=None):
        """(B,3,224,224) normalised RGB -> (B,1) logits; ``freq_input`` ignored (reference model.py:63-72)."""
        return self._run(rgb_input, self.handle.classify)

    __call__ = forward

    def extract_features(self, rgb_input):
        """(B,1280) pooled backbone features (reference model.py:74-89)."""
        return self._run(rgb_input, self.handle.extract_features)

    def extract_trunk(self, rgb_input, block: int = 15):
        """(B,7,7,320) block 15's output, NHWC: the rows `fit_head(train_conv_head=True)` trains on; `block=14`:
        (B,7,7,192) block 14's output, the rows `fit_head(train_block15=True)` trains on."""
        if block == 15:
            return self._run(rgb_input, self.handle.extract_trunk)
        return self._run(rgb_input, lambda a: self.handle.extract_trunk(a, block=block))

    def extract_block(self, rgb_input, block: int):
        """the output of block 13, 14 or 15, NHWC, `max_batch` crops at a time (`Handle.extract_block`): (B,7,7,192) for 13 -
        the rows `fit_head(train_block14=True)` trains on - and 14, (B,7,7,320) for 15"""
        return self._run(rgb_input, lambda a: self.handle.extract_block(a, block))

    def extract_block_input(self, rgb_input, block: int):
        """(B,7,7,192) the input rows of block 12, 13, 14 or 15, NHWC, `max_batch` crops at a time
        (`Handle.extract_block_input`): the rows `fit_head(train_block13=True)` (block 13) / `train_block12=True` (block 12)
        trains on"""
        return self._run(rgb_input, lambda a: self.handle.extract_block_input(a, block))

    def extract_block_rows(self, rgb_input, block: int):
        """`extract_block_input` with block 11 as well, `max_batch` crops at a time (`Handle.extract_block_rows`): (B,14,14,112),
        block 10's output, for 11 - the rows `fit_head(train_block11=True)` trains on - and (B,7,7,192) for 12..15"""
        return self._run(rgb_input, lambda a: self.handle.extract_block_rows(a, block))

    def forward_with_projection(self, rgb_input, freq_input=None):
        """reference model.py:91-98"""
        return self.forward(rgb_input), None

    def fit_head(self, images_or_features, labels, *, epochs: int = 20, val=None, commit_ema: bool = True,
                 trainer_config: Optional[Mapping] = None, augment=None, train_conv_head: bool = False,
                 train_block15: bool = False, train_block14: bool = False, train_block13: bool = False,
                 train_block12: bool = False, train_block11: bool = False, **fit_kw):
        """Train the 1280 -> 512 -> 256 -> 1 head on this engine's own pooled features and swap it in.

        `images_or_features`: (N,3,224,224) normalised RGB (features are extracted here, `max_batch` crops at a time) or
        (N,1280) features; `val`: the same pair for validation, or None.  `trainer_config`: `HeadTrainer` settings
        (seed, dropout, weight_decay, ...; max_n defaults to the batch size); `fit_kw`: `head_training.fit_loop`'s
        (batch_size, grad_accum, lr, mix_alpha, patience, rng).  The trained head (EMA by default) is committed to the
        open handle in place - the handle is NOT re-created - and `state_dict()` returns it from then on.  -> the log.

        `augment`: a `train_augment.AugmentPolicy`, with `images_or_features` (and `val[0]`) (N,H,W,3) uint8 RGB crops: every
        batch of every epoch is augmented on the device and pushed through the backbone anew, on this model's own handle
        (`fit_loop`'s `augment=`; `fit_kw` may then carry `cutmix_alpha`).

        `train_conv_head=True`: ``net._conv_head`` + ``net._bn1`` are fine-tuned with the head (`HeadTrainer`'s flag):
        images go through `extract_trunk`, arrays that are not images are taken as trunk rows ((N,7,7,320) or (N,15680)),
        and both the conv and the head are committed and returned by `state_dict()`.

        `train_block15=True` (implies `train_conv_head`): ``net._blocks.15`` is fine-tuned as well: images go through
        `extract_trunk(block=14)`, other arrays are rows of block 14's output ((N,7,7,192) or (N,9408)), `augment=` extracts
        them anew every batch, and block, conv and head are committed and returned by `state_dict()`.

        `train_block14=True` (implies `train_block15`): ``net._blocks.14`` is fine-tuned as well, with the reference's
        drop-connect rate: images go through `extract_block(block=13)`, other arrays are rows of block 13's output
        ((N,7,7,192) or (N,9408)).

        `train_block13=True` (implies `train_block14`) / `train_block12=True` (implies `train_block13`): ``net._blocks.13`` /
        ``net._blocks.12`` are fine-tuned as well, each with the reference's drop-connect rate and its own mask: images go
        through `extract_block_input` at the deepest block, other arrays are its input rows ((N,7,7,192) or (N,9408)).

        `train_block11=True` (implies `train_block12`): ``net._blocks.11``, the stride-2 block below block 12, is fine-tuned as
        well (no skip, no drop-connect): images go through `extract_block_rows(block=11)`, other arrays are rows of block
        10's output ((N,14,14,112) or (N,21952)).  Blocks 10 and 9 stay frozen."""
        from .head_training import HeadTrainer

        train_block12 = train_block12 or train_block11
        train_block13 = train_block13 or train_block12
        train_block14 = train_block14 or train_block13
        train_block15 = train_block15 or train_block14

        def feats(x):
            a = x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)
            if train_conv_head or train_block15:
                if a.ndim == 4 and a.shape[1:] == (3, A.IMAGE_SIZE, A.IMAGE_SIZE):
                    if train_block11:
                        a = self.extract_block_rows(a, 11)
                    elif train_block13:
                        a = self.extract_block_input(a, 12 if train_block12 else 13)
                    else:
                        a = self.extract_block(a, 13) if train_block14 else self.extract_trunk(a, block=14 if train_block15 else 15)
                return np.ascontiguousarray(a, np.float32).reshape(a.shape[0], -1)
            return np.ascontiguousarray(a, np.float32) if a.ndim == 2 else np.asarray(self.extract_features(a), np.float32)

        cfg = dict(trainer_config or {})
        cfg.setdefault("max_n", max(2, int(fit_kw.get("batch_size", 32))))
        if augment is not None:
            from .train_augment import ResidentCrops

            x = images_or_features if isinstance(images_or_features, ResidentCrops) else np.asarray(images_or_features)
            if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3:
                raise ValueError("fit_head(augment=...) needs (N,H,W,3) uint8 crops or a ResidentCrops of this model's handle")
            v = val                                                # fit_loop extracts the validation crops itself
            fit_kw = dict(fit_kw, augment=(self.handle, augment))
        else:
            x = feats(images_or_features)
            v = None if val is None else (feats(val[0]), np.asarray(val[1], np.float32))
        y = labels.detach().cpu().numpy() if _is_torch(labels) else np.asarray(labels)
        with HeadTrainer(self, train_conv_head=train_conv_head, train_block15=train_block15, train_block14=train_block14,
                         train_block13=train_block13, train_block12=train_block12, train_block11=train_block11, **cfg) as tr:
            log_ = tr.fit(x, y, epochs, val=v, **fit_kw)
            tr.commit(use_ema=commit_ema)
            self._state.update(tr.export_state_dict(use_ema=commit_ema))
        return log_

    def get_feature_extractor(self):
        """reference model.py:100-102 (GradCAM hook target; descriptor only here)."""
        return self.net._conv_head


def check_frequency_size(size, any_size: bool = False) -> int:
    """-> the size as an int, or ValueError: 224 always; with `any_size` every even size in 2..1024 (`cv2.dct` itself
    refuses odd sizes)"""
    size = int(size)
    if size != 224:
        if not any_size:
            raise ValueError("compute_frequency_features is built for size=224 only (the one value the reference ever "
                             "passes); any_size=True or DFD_FREQ_ANY_SIZE=1 admits every even size in 2..1024")
        if size % 2 or not 2 <= size <= 1024:
            raise ValueError(f"compute_frequency_features size {size}: supported are even sizes in 2..1024 "
                             "(cv2.dct refuses odd sizes)")
    return size


def compute_frequency_features(image_bgr_or_rgb, size: int = 224, *, any_size: Optional[bool] = None,
                               handle: Optional[Handle] = None):
    """FFT log-magnitude + DCT features, (2, size, size) float32 in [0,1] (reference model.py:105-149),
    computed on the GPU.  ``size=224`` (the one value the reference ever passes, deepfake_detection.py:392) runs its own
    kernels; `any_size` (None: the environment variable DFD_FREQ_ANY_SIZE, default off) admits every even size in
    2..1024, on the any-size kernels (`dfd_frequency_features_sized`)."""
    if any_size is None:
        any_size = os.environ.get("DFD_FREQ_ANY_SIZE", "").strip().lower() in ("1", "true", "yes", "on")
    size = check_frequency_size(size, any_size)
    if handle is None:
        from . import runtime

        handle = runtime.default_handle()
    return handle.frequency_features(image_bgr_or_rgb, size)


__all__ = ["DeepfakeEfficientNet", "DfdError", "check_frequency_size", "compute_frequency_features"]
