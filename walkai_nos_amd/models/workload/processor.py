"""The YOLOS image processor: what turns a photo into the model's pixels and the model's
``(logits, boxes)`` into detections (the reference demo's ``YolosImageProcessor``).

Resize to the processor's size rule (shortest edge 800, longest at most 1333, both sides cropped to a
multiple of 16), rescale by 1/255 and normalise with the ImageNet mean / std; after the model,
``post_process_object_detection``. On the GPU both ends are one HIP launch each
(:mod:`walkai_nos_amd.ops.image`).

What differs from the ``transformers`` processor: the resample is not rounded to uint8 between its
horizontal and vertical pass nor after them, so a pixel differs from the ``transformers`` one by
less than one uint8 step (``1 / (255 std_c)`` after normalisation); and there is no padding and no
pixel mask, because one call runs images of one size.

A video decoder's NV12 surface goes in as :class:`Nv12` wherever an image does: the colour conversion
(BT.601 or BT.709, limited or full range, in exact integers: ``ops.image.nv12_to_rgb``) is fused into
the same launch. It takes chroma nearest — luma ``(r, c)`` uses chroma ``(r >> 1, c >> 1)``, as the
usual one-call library conversions do; bilinear chroma upsampling is not offered.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ...ops import image as I

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


@dataclass(frozen=True)
class Nv12:
    """An NV12 frame (or a batch of one size): ``y`` uint8 ``[h, w]`` or ``[B, h, w]``, ``uv`` uint8
    ``[(h+1)//2, (w+1)//2, 2]`` (U, V) with the same leading ``B``; rows may be pitched. The planes are
    held as they are given — a captured graph reads them by address."""
    y: torch.Tensor
    uv: torch.Tensor
    matrix: str = "bt601"
    full_range: bool = False

    def __post_init__(self):
        I.nv12_planes(self.y, self.uv)
        I.nv12_table(self.matrix, self.full_range)

    @classmethod
    def from_buffer(cls, buf: Any, h: int, w: int, pitch: Optional[int] = None, matrix: str = "bt601",
                    full_range: bool = False) -> "Nv12":
        """A decoder's single surface — ``h`` rows of Y, then ``h / 2`` rows of UV, all ``pitch`` bytes
        apart (default ``w``) — as the two planes, without a copy. ``buf``: a contiguous uint8 tensor or
        ndarray of at least ``(3 h / 2 - 1) * pitch + 2 * ((w + 1) // 2)`` bytes."""
        t = torch.from_numpy(buf) if isinstance(buf, np.ndarray) else buf
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError("Nv12.from_buffer: a contiguous uint8 tensor or ndarray")
        h, w = int(h), int(w)
        pitch = w if pitch is None else int(pitch)
        cw2 = 2 * ((w + 1) // 2)
        if h <= 0 or w <= 0 or h % 2:
            raise ValueError("Nv12.from_buffer: positive sizes and an even height (UV rows follow the Y rows)")
        if pitch < cw2:
            raise ValueError(f"Nv12.from_buffer: pitch {pitch} is smaller than a row of {w} pixels")
        need = (h + h // 2 - 1) * pitch + cw2
        if t.numel() < need:
            raise ValueError(f"Nv12.from_buffer: {h}x{w} at pitch {pitch} takes {need} bytes, the buffer has {t.numel()}")
        off = t.storage_offset()
        return cls(t.as_strided((h, w), (pitch, 1), off),
                   t.as_strided((h // 2, cw2 // 2, 2), (pitch, 2, 1), off + h * pitch), matrix, full_range)

    def batched(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(y [B, h, w], uv [B, ch, cw, 2])`` views."""
        return I.nv12_planes(self.y, self.uv)

    # what the processor and the model ask of an image batch
    @property
    def shape(self) -> Tuple[int, int, int, int]:
        """``(B, h, w, 3)``: the shape of the RGB batch this frame stands for."""
        return tuple(self.batched()[0].shape) + (3,)

    @property
    def device(self) -> torch.device:
        return self.y.device

    @property
    def is_cuda(self) -> bool:
        return self.y.is_cuda

    def to(self, device) -> "Nv12":
        """On ``device``; the same object (and the same buffers) when it is there already."""
        if device is None or self.y.device == torch.device(device):
            return self
        return Nv12(self.y.to(device), self.uv.to(device), self.matrix, self.full_range)

    def rgb(self) -> torch.Tensor:
        """The frame converted: uint8 ``[B, h, w, 3]`` (``ops.image.nv12_to_rgb``)."""
        return I.nv12_to_rgb(self.y, self.uv, self.matrix, self.full_range)


class YolosProcessor:
    def __init__(self, shortest: int = 800, longest: Optional[int] = 1333, mod: Optional[int] = 16, patch: int = 16,
                 mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD):
        self.shortest, self.longest, self.mod, self.patch = shortest, longest, mod, patch
        self.mean, self.std = tuple(mean), tuple(std)

    def size(self, hw: Tuple[int, int]) -> Tuple[int, int]:
        """``(H, W)`` an ``(h, w)`` image is resized to."""
        return I.resize_size(hw, self.shortest, self.longest, self.mod)

    @staticmethod
    def as_batch(image: Any, device: Optional[torch.device] = None) -> torch.Tensor:
        """A uint8 ``[B, h, w, 3]`` tensor from a uint8 HWC (or BHWC) tensor or ndarray, or a PIL image;
        an :class:`Nv12` frame stays one (it answers ``shape``, ``device`` and ``is_cuda`` as the batch would)."""
        if isinstance(image, Nv12):
            return image.to(device)
        if not isinstance(image, (torch.Tensor, np.ndarray)):
            try:
                from PIL import Image
            except ImportError:
                Image = None
            if Image is None or not isinstance(image, Image.Image):
                raise TypeError("image: a uint8 HWC tensor or ndarray, or a PIL image")
            image = np.array(image.convert("RGB"))
        t = torch.from_numpy(np.ascontiguousarray(image)) if isinstance(image, np.ndarray) else image
        if t.dim() == 3:
            t = t[None]
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
            raise ValueError("image: uint8, height x width x 3 (RGB, interleaved)")
        return t.to(device) if device is not None else t

    def preprocess(self, image: Any, device: Optional[torch.device] = None) -> torch.Tensor:
        """Pixels fp32 ``[B, 3, H, W]`` on the image's device (or ``device``)."""
        img = self.as_batch(image, device)
        hw = self.size(tuple(img.shape[1:3]))
        if img.is_cuda:
            return self.patch_planes(img, hw, want_pixels=True)[1]
        return I.pixels_reference(img.rgb() if isinstance(img, Nv12) else img, hw, self.mean, self.std)

    def patch_planes(self, img: Any, hw: Tuple[int, int], want_pixels: bool = False) \
            -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """The x3 planes of the patch matrix (and the pixels on request) of :meth:`as_batch`'s result,
        resized to ``hw``: ``ops.image.image_patch_planes``, or ``nv12_patch_planes`` for an :class:`Nv12`."""
        if isinstance(img, Nv12):
            return I.nv12_patch_planes(img.y, img.uv, hw, self.patch, self.mean, self.std, img.matrix,
                                       img.full_range, want_pixels)
        return I.image_patch_planes(img, hw, self.patch, self.mean, self.std, want_pixels)

    @staticmethod
    def results(count: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, boxes: torch.Tensor) \
            -> List[Dict[str, torch.Tensor]]:
        """The compacted device tensors of ``ops.image.detections`` as ``transformers`` returns them:
        one ``{"scores", "labels", "boxes"}`` per image (this reads ``count`` on the host)."""
        return [{"scores": scores[i, :n], "labels": labels[i, :n].long(), "boxes": boxes[i, :n]}
                for i, n in enumerate(count.tolist())]

    def post_process(self, logits: torch.Tensor, boxes: torch.Tensor, threshold: float = 0.5,
                     target_sizes=None) -> List[Dict[str, torch.Tensor]]:
        """``post_process_object_detection``: per image the scores, labels and ``(x0, y0, x1, y1)`` boxes
        (in pixels of ``target_sizes`` = (height, width) per image, else 0..1) of the rows whose best
        class probability exceeds ``threshold``, in token order."""
        return self.results(*I.detections(logits, boxes, target_sizes, threshold))
