"""Detections drawn into the frame they were found in: :class:`Overlay` holds the parameters and the device tables of
``ops.image.overlay`` (one launch that paints boxes, id tags and redactions into a surface's own planes) and of
``ops.image.mosaic`` and ``ops.image.blur`` (launches before it that pixelate or blur the boxes of chosen labels in
place) and paints the dict of
``YolosSmall.detect_image``, ``detect_tiled``, ``track_image`` or ``track_tiled`` into a target of any SDR layout the
front end reads. Nothing here synchronises with the host, so ``YolosSmall.annotate_image`` and
``annotate_tiled`` capture as one graph: frame in, annotated (or redacted) frame out.

Alpha blending, antialiased lines, class names or any glyph but digits, PQ / HLG surfaces (an SDR colour has no code
there without the inverse tone map), batches above one and more than 1024 rows are not offered; nor are mosaic
cells of other sizes than ``ops.image.MOSAIC_CELLS`` or cells anchored to the box instead of the frame, blur radii
above ``ops.image.BLUR_MAX_RADIUS``, box or other blur kernels or feathered edges."""
from __future__ import annotations

from typing import Dict, Iterable, Mapping, Optional, Sequence

import numpy as np
import torch

from ...ops import image as I


class Overlay:
    def __init__(self, palette=None, thickness: Optional[int] = None, scale: Optional[int] = None, tags: bool = True,
                 modes: Optional[Mapping[int, int]] = None, redact: Iterable[int] = (),
                 redact_colour: Sequence[int] = (0, 0, 0), min_hits: int = 1, num_labels: int = 91,
                 pixelate: Iterable[int] = (), cell: Optional[int] = None, blur: Iterable[int] = (),
                 blur_radius: Optional[int] = None):
        """``palette``: ``[K, 2, 3]`` uint8 RGB fill and text colours (default ``ops.image.overlay_palette()``); a row
        takes entry ``key mod K``, its track id or, without ids, its label. ``scale``: the side of a glyph's dot in
        pixels, by default ``max(1, round(min(h, w) / 360))`` of the target; ``thickness``: of a box's outline, by
        default twice the scale (even, so that an outline always carries its chroma on a subsampled surface).
        ``tags=False`` draws no id tags. Every label in ``[0, num_labels)`` is drawn as an outline, but those of
        ``redact``, which are filled with ``redact_colour``; ``modes`` (label -> 0 not drawn, 1 outline and tag, 2
        redacted, or the names of ``ops.image.OVERLAY_MODES``) overrides per label. With ids, rows of tracks seen in
        fewer than ``min_hits`` frames are not drawn. The boxes of the labels in ``pixelate`` are pixelated
        (``ops.image.mosaic``) before anything is drawn, in cells of ``cell`` pixels, by default the largest of
        ``ops.image.MOSAIC_CELLS`` not above ``max(4, min(h, w) // 32)`` of the target; such a label is not drawn
        unless ``modes`` gives it mode 1, an outline and tag on the pixelated picture. The boxes of the labels in
        ``blur`` are blurred (``ops.image.blur``) behind the mosaic and before the drawing, at ``blur_radius`` luma
        pixels (1..``ops.image.BLUR_MAX_RADIUS``), by default ``min(32, max(1, min(h, w) // 64))`` of the target;
        they too are drawn only where ``modes`` gives them mode 1. A label is redacted, pixelated or blurred,
        exactly one."""
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
        redact, self.pixelate = tuple(redact), tuple(sorted({int(l) for l in pixelate}))
        if cell is not None and cell not in I.MOSAIC_CELLS:
            raise ValueError(f"Overlay: cell {cell!r} is none of {I.MOSAIC_CELLS}")
        for label in self.pixelate:
            mode = (modes or {}).get(label, 0)
            if not 0 <= label < len(table):
                raise ValueError(f"Overlay: pixelated label {label!r} is not in [0, {len(table)})")
            if label in redact or I.OVERLAY_MODES.get(mode, mode) == 2:
                raise ValueError(f"Overlay: label {label!r} is both redacted and pixelated")
        self.blur = tuple(sorted({int(l) for l in blur}))
        if blur_radius is not None and (isinstance(blur_radius, bool) or not isinstance(blur_radius, int)
                                        or not 1 <= blur_radius <= I.BLUR_MAX_RADIUS):
            raise ValueError(f"Overlay: blur_radius {blur_radius!r} is not an integer in 1..{I.BLUR_MAX_RADIUS}")
        for label in self.blur:
            mode = (modes or {}).get(label, 0)
            if not 0 <= label < len(table):
                raise ValueError(f"Overlay: blurred label {label!r} is not in [0, {len(table)})")
            if label in redact or label in self.pixelate or I.OVERLAY_MODES.get(mode, mode) == 2:
                raise ValueError(f"Overlay: label {label!r} is redacted, pixelated or blurred, exactly one")
        for label, mode in [(l, 2) for l in redact] + [(l, 0) for l in self.pixelate + self.blur] \
                + list((modes or {}).items()):
            mode = I.OVERLAY_MODES.get(mode, mode)
            if not 0 <= int(label) < len(table) or mode not in (0, 1, 2):
                raise ValueError(f"Overlay: label {label!r} is not in [0, {len(table)}) or mode {mode!r} not 0, 1 or 2")
            table[int(label)] = int(mode)
        self.modes = tuple(table)
        self.thickness = None if thickness is None else int(thickness)
        self.scale = None if scale is None else int(scale)
        self.tags, self.min_hits = bool(tags), int(min_hits)
        self.cell = None if cell is None else int(cell)
        self.blur_radius = blur_radius
        self._modes: Dict[str, torch.Tensor] = {}
        self._select: Dict[str, torch.Tensor] = {}

    def sizes(self, h: int, w: int) -> tuple:
        """``(thickness, scale)`` on an ``h x w`` target; the scale is 0 without tags."""
        scale = max(1, round(min(h, w) / 360)) if self.scale is None else self.scale
        thickness = max(1, 2 * scale) if self.thickness is None else self.thickness
        return thickness, scale if self.tags else 0

    def cell_size(self, h: int, w: int) -> int:
        """The side of a mosaic cell on an ``h x w`` target: 1080 rows give 32, 2160 give 64, 480 give 8."""
        if self.cell is not None:
            return self.cell
        return max(c for c in I.MOSAIC_CELLS if c <= max(4, min(h, w) // 32))

    def radius_size(self, h: int, w: int) -> int:
        """The blur's radius on an ``h x w`` target: 480 rows give 7, 1080 give 16, 2160 give 32."""
        if self.blur_radius is not None:
            return self.blur_radius
        return min(I.BLUR_MAX_RADIUS, max(1, min(h, w) // 64))

    def select(self, surface: "I.OverlaySurface", blur: bool = False) -> torch.Tensor:
        """``ops.image.mosaic``'s table of the pixelated labels — with ``blur`` ``ops.image.blur``'s of the blurred
        ones — on the surface's device, made once, eagerly."""
        key = f"{surface.device}{'/blur' if blur else ''}"
        if key not in self._select:
            chosen = self.blur if blur else self.pixelate
            table = [int(label in chosen) for label in range(len(self.modes))]
            self._select[key] = torch.tensor(table, dtype=torch.uint8).to(surface.device)
        return self._select[key]

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
        through their strides, and the boxes are in the target's own pixels. The order is fixed: the mosaic of the
        labels to pixelate, then the blur of the labels to blur, which reads the picture the mosaic left, then the
        drawing, so outlines and tags lie on the pixelated and blurred picture."""
        scores = det["scores"]
        if scores.dim() == 2 and scores.shape[0] != 1:
            raise ValueError(f"Overlay: one image's detections, not a batch of {scores.shape[0]}")
        surface = I.overlay_surface(target)
        thickness, scale = self.sizes(surface.h, surface.w)
        modes, codes = self.tables(surface)
        if self.pixelate:
            I.mosaic(target, det["count"], scores, det["labels"], det["boxes"], det.get("track_id"),
                     det.get("track_hits"), min_hits=self.min_hits, select=self.select(surface),
                     cell=self.cell_size(surface.h, surface.w))
        if self.blur:
            I.blur(target, det["count"], scores, det["labels"], det["boxes"], det.get("track_id"),
                   det.get("track_hits"), min_hits=self.min_hits, select=self.select(surface, blur=True),
                   radius=self.radius_size(surface.h, surface.w))
        I.overlay(target, det["count"], scores, det["labels"], det["boxes"], det.get("track_id"),
                  det.get("track_hits"), thickness=thickness, scale=scale, modes=modes, min_hits=self.min_hits,
                  codes=codes)
        return target
