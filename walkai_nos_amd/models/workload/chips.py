"""Detections cut out of the frame they were found in: :class:`Chips` holds the parameters and the device table of
``ops.image.chips`` (one launch that resamples the box of every selected detection to one size, as RGB bytes) and adds
the chips to the dict of ``YolosSmall.detect_image``, ``detect_tiled``, ``track_image`` or ``track_tiled``. A plate
reader, a re-identification model, a second-stage classifier or an event log's thumbnail take them from there. Nothing
here synchronises with the host, so ``YolosSmall.chip_image`` and ``chip_tiled`` capture as one graph: frame in,
detections and their pictures out. Every layout, chroma mode and transfer the front end reads is cut, PQ / HLG included.

Aspect-preserving or letterboxed chips, bilinear or bicubic enlargement, float or normalised output, rotated boxes,
batches above one and more than 256 chips are not offered."""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Tuple

import torch

from ...ops import image as I


class Chips:
    def __init__(self, size: Tuple[int, int] = (128, 64), labels: Optional[Iterable[int]] = None, capacity: int = 64,
                 margin: int = 0, min_hits: int = 1, num_labels: int = 91):
        """``size``: ``(rows, columns)`` of every chip. ``labels``: the labels that are cut out, by default every label
        in ``[0, num_labels)``. ``capacity``: the chips of one frame; selected rows beyond it get none. ``margin``: pixels
        added to a box on every side before it is clipped to the frame. With ids, rows of tracks seen in fewer than
        ``min_hits`` frames are not cut."""
        self.size = I._chips_params(size, capacity, margin)[:2]
        self.capacity, self.margin = int(capacity), int(margin)
        if not int(min_hits) >= 1:
            raise ValueError(f"Chips: min_hits {min_hits!r} is not a number of frames from 1 up")
        if not int(num_labels) >= 1:
            raise ValueError(f"Chips: num_labels {num_labels!r} is not a positive number of labels")
        chosen = set(range(int(num_labels))) if labels is None else {int(l) for l in labels}
        if any(not 0 <= l < int(num_labels) for l in chosen):
            raise ValueError(f"Chips: labels {sorted(chosen)} are not all in [0, {int(num_labels)})")
        self.labels = tuple(int(l in chosen) for l in range(int(num_labels)))
        self.min_hits = int(min_hits)
        self._select: Dict[str, torch.Tensor] = {}

    def select(self, device) -> torch.Tensor:
        """``ops.image.chips``' table of the labels on ``device``, made once, eagerly (a captured graph must not copy
        from the host)."""
        key = str(device)
        if key not in self._select:
            self._select[key] = torch.tensor(self.labels, dtype=torch.uint8).to(device)
        return self._select[key]

    def cut(self, det: Dict[str, object], frame) -> Dict[str, object]:
        """The detections ``det`` — the dict of ``detect_image`` (one image), ``detect_tiled``, ``track_image`` or
        ``track_tiled`` — cut out of ``frame``, whose pixels the boxes are in: the same dict with ``chips`` ``[capacity,
        S_h, S_w, 3]`` uint8, ``chip_rows`` ``[capacity]``, ``chip_rects`` ``[capacity, 4]`` and ``chip_count`` ``[1]``
        int32 added (``ops.image.chips``)."""
        scores = det["scores"]
        if scores.dim() == 2 and scores.shape[0] != 1:
            raise ValueError(f"Chips: one image's detections, not a batch of {scores.shape[0]}")
        chips, rows, rects, n = I.chips(frame, det["count"], scores, det["labels"], det["boxes"], det.get("track_id"),
                                        det.get("track_hits"), size=self.size, select=self.select(scores.device),
                                        capacity=self.capacity, margin=self.margin, min_hits=self.min_hits)
        return {**det, "chips": chips, "chip_rows": rows, "chip_rects": rects, "chip_count": n}
