"""The input transform of the gradient pipe as Caffe describes it: `InputTransform`, the host side of hip_data_transform (csrc/kernels/data_f32.hip; DESIGN.md section
3.21).  It holds what a Data layer's transform_param says (prototxt.transform_spec reads one), makes the mean var's array, and makes and checks the per-image plans
(uint32 img:v=4 = y_off, x_off, mirror, unused) a ConvPipeBck or an EvalPipe uploads before every pass.  Nothing of it runs on the device: a plan is Python integers."""
from __future__ import annotations
from typing import Optional, Sequence, Tuple, Union

import numpy as np

from .op import Dims, RtErr

DATA_RAW_VAR = "data_raw"          # uint8: the batch at the source size, in the transform's layout
DATA_XF_PLAN_VAR = "data_xf_plan"  # uint32 img:v=4, uploaded before every pass
DATA_XF_MEAN_VAR = "data_xf_mean"  # float chan or chan:y:x, uploaded once
DATA_XF_TAG = "data_xf"            # the tag of the call in front of the step

_M32 = 0xFFFFFFFF
_GOLDEN = 0x9E3779B1


def fmix32(h: int) -> int:
    """The murmur3 finaliser (the dropout hash's)."""
    h &= _M32
    h ^= h >> 16; h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13; h = (h * 0xC2B2AE35) & _M32
    h ^= h >> 16
    return h


def plan_word(seed: int, k: int) -> int:
    """word(k) = fmix32((seed + k * 0x9E3779B1) mod 2^32)."""
    return fmix32((int(seed) + int(k) * _GOLDEN) & _M32)


class InputTransform:
    """InputTransform(src_hw, crop=0, mirror=False, scale=1.0, mean_value=None, mean=None, layout="hwc" | "chw", seed=0) -- Caffe's DataTransformer on a source of
    src_hw = (H, W) pels: a crop x crop window (0: the whole source), a random mirror, a mean (mean_value: one value or one per channel, Caffe's broadcast rule; or
    mean: a chan:y:x array at the SOURCE size, Caffe's mean_file) and a scale.  layout says how the uint8 batch lies: "hwc" img:y:x:chan (an image decoder's) or "chw"
    img:chan:y:x (a Caffe Datum's).
      plan("test", first_image, n)   [(H - ch) // 2, (W - cw) // 2, 0, 0] for every image: Caffe's centre crop, no mirror
      plan("train", first_image, n)  for the image with global index g = first_image + i: y_off = word(3g) mod (H - ch + 1), x_off = word(3g + 1) mod (W - cw + 1),
                                     mirror = word(3g + 2) & 1 if mirror else 0, word(k) = fmix32((seed + k * 0x9E3779B1) mod 2^32)
      check_plan(plan)               RtErr for an offset beyond the range (the kernel clamps; the host refuses before it uploads)
    """

    def __init__(self, src_hw: Tuple[int, int], crop: int = 0, mirror: bool = False, scale: float = 1.0, mean_value: Union[None, float, Sequence[float]] = None,
                 mean: Optional[np.ndarray] = None, layout: str = "hwc", seed: int = 0):
        try:
            H, W = (int(v) for v in src_hw)
        except (TypeError, ValueError):
            raise RtErr(f"InputTransform: src_hw must be (H, W), got {src_hw!r}")
        if H < 1 or W < 1:
            raise RtErr(f"InputTransform: src_hw must be positive, got {src_hw!r}")
        if layout not in ("hwc", "chw"):
            raise RtErr(f"InputTransform: layout must be 'hwc' | 'chw', got {layout!r}")
        if not isinstance(crop, (int, np.integer)) or isinstance(crop, bool) or crop < 0:
            raise RtErr(f"InputTransform: crop must be an int >= 0, got {crop!r}")
        if crop > H or crop > W:
            raise RtErr(f"InputTransform: crop={crop} is larger than the source {H} x {W}")
        if mean_value is not None and mean is not None:
            raise RtErr("InputTransform: both mean_value and mean are given; Caffe takes one of them")
        self.H, self.W = H, W
        self.ch, self.cw = (int(crop), int(crop)) if crop else (H, W)
        self.mirror = bool(mirror)
        self.scale = float(np.float32(scale))
        self.layout = layout
        self.seed = int(seed) & _M32
        if mean_value is not None:
            mv = np.atleast_1d(np.asarray(mean_value, np.float32))
            if mv.ndim != 1 or mv.size < 1:
                raise RtErr(f"InputTransform: mean_value must be one value or one per channel, got {mean_value!r}")
            self.mean_value: Optional[np.ndarray] = mv
        else:
            self.mean_value = None
        if mean is not None:
            m = np.ascontiguousarray(mean, np.float32)
            if m.ndim != 3 or m.shape[1:] != (H, W):
                raise RtErr(f"InputTransform: mean must be chan:y:x at the source size {H} x {W}, got shape {tuple(np.shape(mean))}")
            self.mean: Optional[np.ndarray] = m
        else:
            self.mean = None

    # -- dims and arrays for a pipe of `chan` channels
    def src_dims(self, img: int, chan: int) -> Dims:
        if self.layout == "hwc":
            return Dims(("img", "y", "x", "chan"), (int(img), self.H, self.W, int(chan)), "uint8_t")
        return Dims(("img", "chan", "y", "x"), (int(img), int(chan), self.H, self.W), "uint8_t")

    def mean_dims(self, chan: int) -> Dims:
        if self.mean is not None:
            return Dims(("chan", "y", "x"), (int(chan), self.H, self.W), "float")
        return Dims(("chan",), (int(chan),), "float")

    def mean_array(self, chan: int) -> np.ndarray:
        """What the mean var holds for a pipe of `chan` channels: the chan:y:x array; mean_value broadcast to one per channel; zeros with neither (v - 0 is v)."""
        chan = int(chan)
        if self.mean is not None:
            if self.mean.shape[0] != chan:
                raise RtErr(f"InputTransform: mean has {self.mean.shape[0]} channels, the data node {chan}")
            return self.mean
        if self.mean_value is None:
            return np.zeros(chan, np.float32)
        if self.mean_value.size == 1:
            return np.full(chan, self.mean_value[0], np.float32)
        if self.mean_value.size != chan:
            raise RtErr(f"InputTransform: {self.mean_value.size} mean values for {chan} channels: one value or one per channel")
        return self.mean_value.copy()

    # -- plans
    def plan(self, phase: str, first_image: int, n: int) -> np.ndarray:
        """-> uint32 (n, 4): the plan of images first_image .. first_image + n - 1 of `phase` ("train" | "test")."""
        if phase not in ("train", "test"):
            raise RtErr(f"InputTransform.plan: phase must be 'train' | 'test', got {phase!r}")
        ry, rx = self.H - self.ch + 1, self.W - self.cw + 1
        out = np.zeros((int(n), 4), np.uint32)
        if phase == "test":
            out[:, 0] = (self.H - self.ch) // 2; out[:, 1] = (self.W - self.cw) // 2
            return out
        for i in range(int(n)):
            g = int(first_image) + i
            out[i, 0] = plan_word(self.seed, 3 * g) % ry
            out[i, 1] = plan_word(self.seed, 3 * g + 1) % rx
            out[i, 2] = (plan_word(self.seed, 3 * g + 2) & 1) if self.mirror else 0
        return out

    def check_plan(self, plan: np.ndarray, n: Optional[int] = None) -> np.ndarray:
        """-> the plan as a contiguous uint32 (n, 4) array; RtErr for another shape or an offset beyond the range 0 .. H - ch / 0 .. W - cw."""
        a = np.asarray(plan)
        if a.ndim != 2 or a.shape[1] != 4 or (n is not None and a.shape[0] != int(n)) or a.dtype.kind not in "ui":
            raise RtErr(f"InputTransform.check_plan: a plan is an integer array of shape ({'n' if n is None else int(n)}, 4), got {a.dtype} {a.shape}")
        if a.size and (int(a.min()) < 0 or int(a.max()) > _M32):
            raise RtErr("InputTransform.check_plan: a plan word is outside uint32")
        for col, what, top in ((0, "y_off", self.H - self.ch), (1, "x_off", self.W - self.cw)):
            bad = np.nonzero(a[:, col].astype(np.int64) > top)[0]
            if bad.size:
                i = int(bad[0])
                raise RtErr(f"InputTransform.check_plan: image {i}: {what}={int(a[i, col])} is beyond the range 0 .. {top}")
        return np.ascontiguousarray(a, np.uint32)
