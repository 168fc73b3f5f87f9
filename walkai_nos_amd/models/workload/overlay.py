"""Detections drawn into the frame they were found in: :class:`Overlay` holds the parameters and the device tables of
``ops.image.overlay`` (one launch that paints boxes, id tags and redactions into a surface's own planes) and paints the
dict of ``YolosSmall.detect_image``, ``detect_tiled``, ``track_image`` or ``track_tiled`` into a target of any SDR
layout the front end reads. Nothing here synchronises with the host, so ``YolosSmall.annotate_image`` and
``annotate_tiled`` capture as one graph: frame in, annotated (or redacted) frame out.

Alpha blending, antialiased lines, class names or any glyph but digits, PQ / HLG surfaces (an SDR colour has no code
there without the inverse tone map), batches above one and more than 1024 rows are not offered."""
from __future__ import annotations

from typing import Dict, Iterable, Mapping, Optional, Sequence

import numpy as np
import torch

from ...ops import image as I


class Overlay:
    def __init__(self, palette=None, thickness: Optional[int] = None, scale: Optional[int] = None, tags: bool = True,
                 modes: Optional[Mapping[int, int]] = None, redact: Iterable[int] = (),
                 redact_colour: Sequence[int] = (0, 0, 0), min_hits: int = 1, num_labels: int = 91):
        """``palette``: ``[K, 2, 3]`` uint8 RGB fill and text colours (default ``ops.image.overlay_palette()``); a row
        takes entry ``key mod K``, its track id or, without ids, its label. ``scale``: the side of a glyph's dot in
        pixels, by default ``max(1, round(min(h, w) / 360))`` of the target; ``thickness``: of a box's outline, by
        default twice the scale (even, so that an outline always carries its chroma on a subsampled surface).
        ``tags=False`` draws no id tags. Every label in ``[0, num_labels)`` is drawn as an outline, but those of
        ``redact``, which are filled with ``redact_colour``; ``modes`` (label -> 0 not drawn, 1 outline and tag, 2
        redacted, or the names of ``ops.image.OVERLAY_MODES``) overrides per label. With ids, rows of tracks seen in
        fewer than ``min_hits`` frames are not drawn."""
        self.palette = I.overlay_palette() if palette is None else np.asarray(palette)
        self.redact_colour = tuple(int(c) for c in redact_colour)
        I.overlay_host_codes(self.palette, self.redact_colour, None)        # the checks of both
        for name, v, least in (("thickness", thickness, 1), ("scale", scale, 0)):
            if v is not None and not int(v) >= least:
                raise ValueError(f"Overlay: {name} {v!r} is not a number of pixels from {least} up")
        if not int(min_hits) >= 1:
            raise ValueError(f"Overlay: min_hits {min_hits!r} is not a number of frames from 1 up")
        if not int(num_labels) >= 1:
            raise ValueError(f"Overlay: num_labels {num_labels!r} is not a positive number of labels")
        table = [1] * int(num_labels)
        for label, mode in [(l, 2) for l in redact] + list((modes or {}).items()):
            mode = I.OVERLAY_MODES.get(mode, mode)
            if not 0 <= int(label) < len(table) or mode not in (0, 1, 2):
                raise ValueError(f"Overlay: label {label!r} is not in [0, {len(table)}) or mode {mode!r} not 0, 1 or 2")
            table[int(label)] = int(mode)
        self.modes = tuple(table)
        self.thickness = None if thickness is None else int(thickness)
        self.scale = None if scale is None else int(scale)
        self.tags, self.min_hits = bool(tags), int(min_hits)
        self._modes: Dict[str, torch.Tensor] = {}

    def sizes(self, h: int, w: int) -> tuple:
        """``(thickness, scale)`` on an ``h x w`` target; the scale is 0 without tags."""
        scale = max(1, round(min(h, w) / 360)) if self.scale is None else self.scale
        thickness = max(1, 2 * scale) if self.thickness is None else self.thickness
        return thickness, scale if self.tags else 0

    def tables(self, surface: "I.OverlaySurface") -> tuple:
        """``(modes, codes)`` on the surface's device: made once, eagerly (a captured graph must not copy from the
        host), the codes in ``ops.image``'s cache."""
        key = str(surface.device)
        if key not in self._modes:
            self._modes[key] = torch.tensor(self.modes, dtype=torch.uint8).to(surface.device)
        return self._modes[key], I.overlay_codes(self.palette, self.redact_colour, surface)

    def draw(self, det: Dict[str, object], target):
        """The detections ``det`` — the dict of ``detect_image`` (one image), ``detect_tiled``, ``track_image`` or
        ``track_tiled`` — painted into ``target`` in place; returns ``target``. With ``track_id`` and ``track_hits`` in
        the dict a row is tagged and coloured by its id, else by its label. ``target``: a uint8 HWC tensor, ``Packed``,
        ``Nv12``, ``Yuv420p``, ``YuvPlanar``, ``YuvSemiPlanar`` or ``Yuyv``; pitched buffers and crop views are written
        through their strides, and the boxes are in the target's own pixels."""
        scores = det["scores"]
        if scores.dim() == 2 and scores.shape[0] != 1:
            raise ValueError(f"Overlay: one image's detections, not a batch of {scores.shape[0]}")
        surface = I.overlay_surface(target)
        thickness, scale = self.sizes(surface.h, surface.w)
        modes, codes = self.tables(surface)
        I.overlay(target, det["count"], scores, det["labels"], det["boxes"], det.get("track_id"),
                  det.get("track_hits"), thickness=thickness, scale=scale, modes=modes, min_hits=self.min_hits,
                  codes=codes)
        return target
