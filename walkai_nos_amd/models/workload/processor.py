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
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ...ops import image as I

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


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
        """A uint8 ``[B, h, w, 3]`` tensor from a uint8 HWC (or BHWC) tensor or ndarray, or a PIL image."""
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
            return I.image_patch_planes(img, hw, self.patch, self.mean, self.std, want_pixels=True)[1]
        return I.pixels_reference(img, hw, self.mean, self.std)

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
