"""A frame at the size its consumer wants, in its own layout: :class:`Scaler` holds the size and the target planes of
``ops.image.rescale`` (one launch that resizes every sample plane by an exact area average) and returns a frame of the
same class and parameters — an operator's wall, an encoder's ladder or an event log's thumbnail take it from there,
with no RGB frame and no colour conversion on the way. Nothing here synchronises with the host, so
``YolosSmall.annotate_image(..., scaler=...)`` captures as one graph: frame in, annotated frame out at another size.

Bilinear, bicubic and Lanczos resizing, changing layout, depth or subsampling while resizing, PQ / HLG surfaces,
batches, sides above 8192 and resizing in place are not offered."""
from __future__ import annotations

from dataclasses import replace
from typing import Tuple

import torch

from ...ops import image as I


class Scaler:
    def __init__(self, size: Tuple[int, int]):
        """``size``: ``(rows, columns)`` of every frame :meth:`scale` returns, 1..8192 each."""
        try:
            H, W = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"Scaler: size {size!r} is not (rows, columns)") from None
        if not (1 <= H <= I.RESCALE_MAX_SIDE and 1 <= W <= I.RESCALE_MAX_SIDE):
            raise ValueError(f"Scaler: size {size!r} is not (rows, columns) of 1..{I.RESCALE_MAX_SIDE}")
        self.size = (H, W)

    def target(self, frame):
        """The frame :meth:`scale` writes for ``frame``: its class and parameters, its layout and sample type at
        ``size``, contiguous planes allocated once per (device, layout, size) and kept as ``ops.image``'s chip buffers
        are — a later call of the same key overwrites them, and a captured graph keeps them alive. A planar target is
        one allocation with U and V in the order they lie in ``frame``; the fourth byte of a packed pixel is 0xFF."""
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
        """``frame`` (anything ``ops.image.overlay_surface`` takes: SDR, one frame) resized to ``size``: a frame of the
        same class and parameters (matrix, range, ``vu``, order, depth, ...) whose planes are :meth:`target`'s."""
        return I.rescale(frame, self.target(frame))
