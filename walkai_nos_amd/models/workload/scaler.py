"""A frame at the size its consumer wants: :class:`Scaler` holds the size and the target planes and returns a frame at
that size — an operator's wall, an encoder's ladder or an event log's thumbnail take it from there. Without a
``format`` the frame keeps its own layout: ``ops.image.rescale`` (one launch that resizes every sample plane by an
exact area average), a frame of the same class and parameters, no RGB frame and no colour conversion on the way. With
a ``format`` the frame is written in that layout instead: ``ops.image.convert`` (one launch: the source read as the
model reads it, PQ / HLG included, resized by the same area average, stored in the target's layout, depth, subsampling,
order, matrix and range). Nothing here synchronises with the host, so ``YolosSmall.annotate_image(..., scaler=...)``
captures as one graph: frame in, annotated frame out at another size and layout.

Bilinear, bicubic and Lanczos resizing, chroma sitings other than centred on the way out, dithering, PQ / HLG targets
(and, without a ``format``, PQ / HLG surfaces), batches, sides above 8192 and resizing in place are not offered."""
from __future__ import annotations

from dataclasses import replace
from typing import Optional, Tuple

import torch

from ...ops import image as I

#: the formats a :class:`Scaler` writes beside the 19 of ``surfaces.FORMATS``: packed pixels and 8-bit 4:2:0
PACKED_FORMATS, YUV420_FORMATS = ("rgb", "bgr", "rgba", "bgra"), ("nv12", "nv21", "i420", "yv12")


class Scaler:
    def __init__(self, size: Tuple[int, int], format: Optional[str] = None, matrix: Optional[str] = None,
                 full_range: Optional[bool] = None):
        """``size``: ``(rows, columns)`` of every frame :meth:`scale` returns, 1..8192 each. ``format``: None — the
        frame's own layout — or the layout of every frame :meth:`scale` returns: ``rgb``, ``bgr``, ``rgba``, ``bgra``,
        ``nv12``, ``nv21``, ``i420``, ``yv12`` or a name of ``surfaces.FORMATS``. ``matrix`` and ``full_range`` of a YUV
        ``format``: by default the source's where it is YUV and SDR, else ``bt709`` and limited range."""
        try:
            H, W = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"Scaler: size {size!r} is not (rows, columns)") from None
        if not (1 <= H <= I.RESCALE_MAX_SIDE and 1 <= W <= I.RESCALE_MAX_SIDE):
            raise ValueError(f"Scaler: size {size!r} is not (rows, columns) of 1..{I.RESCALE_MAX_SIDE}")
        if format is not None:
            from . import surfaces
            if format not in PACKED_FORMATS + YUV420_FORMATS + tuple(surfaces.FORMATS):
                raise ValueError(f"Scaler: format {format!r} is none of "
                                 f"{PACKED_FORMATS + YUV420_FORMATS + tuple(sorted(surfaces.FORMATS))}")
            if matrix is not None:
                I.yuv_real_matrix(matrix)
        self.size, self.format, self.matrix, self.full_range = (H, W), format, matrix, full_range

    def _converted(self, frame):
        """:meth:`target` with a ``format``: a contiguous frame of it at ``size``, cached under (device, format, matrix,
        range, size). A 4:2:0 format takes an even number of rows, as the buffers of its decoders do."""
        from . import surfaces
        from .processor import Nv12, Packed, Yuv420p
        H, W = self.size
        fmt, device = self.format, I._chip_source(frame)[3]
        yuv_sdr = not isinstance(frame, torch.Tensor) and hasattr(frame, "matrix") \
            and getattr(frame, "transfer", "sdr") == "sdr"
        matrix = self.matrix if self.matrix is not None else frame.matrix if yuv_sdr else "bt709"
        full = bool(self.full_range if self.full_range is not None else frame.full_range if yuv_sdr else False)
        if fmt in PACKED_FORMATS:
            matrix, full = None, None
        key = (str(device), "convert", fmt, matrix, full, H, W)

        def buffer(n: int, fill: int = 0) -> torch.Tensor:
            return I._scale_buffers.get(key, lambda: (torch.full((n,), fill, dtype=torch.uint8, device=device),))[0]
        if fmt in PACKED_FORMATS:
            C = len(fmt)
            return Packed(buffer(H * W * C, 0xFF).view(H, W, C), fmt)
        even = 2 * ((W + 1) // 2)       # a luma row's samples, rounded up to whole chroma pairs
        if fmt in ("nv12", "nv21"):
            return Nv12.from_buffer(buffer(even * (H + H // 2)), H, W, even, matrix, full, vu=fmt == "nv21")
        if fmt in YUV420_FORMATS:
            return Yuv420p.from_buffer(buffer(even * (H + H // 2)), H, W, even, order=fmt, matrix=matrix, full_range=full)
        kind, _, depth = surfaces.FORMATS[fmt][:3]
        row = 2 * even if kind == "packed" else even * (1 if depth == 8 else 2)
        # luma rows, then at most twice as many bytes of chroma (4:4:4)
        return surfaces.from_buffer(fmt, buffer(3 * row * H), H, W, row, matrix=matrix, full_range=full)

    def target(self, frame):
        """The frame :meth:`scale` writes for ``frame``. Without a ``format``: its class and parameters, its layout and
        sample type at ``size``, contiguous planes allocated once per (device, layout, size) and kept as
        ``ops.image``'s chip buffers are — a later call of the same key overwrites them, and a captured graph keeps
        them alive. A planar target is one allocation with U and V in the order they lie in ``frame``; the fourth byte
        of a packed pixel is 0xFF. With a ``format``: a ``Packed``, ``Nv12``, ``Yuv420p`` or ``surfaces`` frame of it
        over one buffer, kept the same way per (device, format, matrix, range, size)."""
        if self.format is not None:
            return self._converted(frame)
        s = I.overlay_surface(frame)
        H, W = self.size
        if s.packed is not None:
            data, order = s.packed
            dims = frame.dim() if isinstance(frame, torch.Tensor) else frame.data.dim()
            key = (str(s.device), "packed", order, dims, H, W)
            (out,) = I._scale_buffers.get(key, lambda: (torch.full(
                (1,) * (dims - 3) + (H, W, data.shape[-1]), 0xFF, dtype=torch.uint8, device=s.device),))
            return out if isinstance(frame, torch.Tensor) else replace(frame, data=out)
        layout, planes, sub, depth, msb, order = s.yuv
        hs, vs = I.YUV_SUBSAMPLING[sub]
        CH, CW = (H + (1 << vs) - 1) >> vs, (W + (1 << hs) - 1) >> hs
        dtype = planes[0].dtype
        empty = lambda *shape: torch.empty(shape, dtype=dtype, device=s.device)       # noqa: E731
        key = (str(s.device), type(frame).__name__, layout, sub, depth, msb, order, str(dtype), H, W)
        if layout == I.YUV_PACKED:
            (data,) = I._scale_buffers.get(key, lambda: (empty(H, 4 * ((W + 1) // 2)),))
            return replace(frame, data=data, width=W)
        if layout == I.YUV_SEMIPLANAR:
            y, uv = I._scale_buffers.get(key, lambda: (empty(H, W), empty(CH, CW, 2)))
            return replace(frame, y=y, uv=uv)
        v_first = planes[2].data_ptr() < planes[1].data_ptr() \
            and I._storage_bounds(planes[1]) == I._storage_bounds(planes[2])

        def planar():
            whole = empty(H * W + 2 * CH * CW)
            first, second = (whole[H * W + k * CH * CW:H * W + (k + 1) * CH * CW].view(CH, CW) for k in (0, 1))
            return (whole[:H * W].view(H, W),) + ((second, first) if v_first else (first, second))
        y, u, v = I._scale_buffers.get(key + (v_first,), planar)
        return replace(frame, y=y, u=u, v=v)

    def scale(self, frame):
        """``frame`` resized to ``size``. Without a ``format``: anything ``ops.image.overlay_surface`` takes (SDR, one
        frame), returned as a frame of the same class and parameters (matrix, range, ``vu``, order, depth, ...) whose
        planes are :meth:`target`'s. With a ``format``: anything ``ops.image.chips`` reads (PQ / HLG too, one frame),
        returned as :meth:`target`'s frame of that format."""
        if self.format is not None:
            return I.convert(frame, self.target(frame))
        return I.rescale(frame, self.target(frame))
