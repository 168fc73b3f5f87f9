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
the same launch. By default it takes chroma nearest — luma ``(r, c)`` uses chroma ``(r >> 1, c >> 1)``, as the
usual one-call library conversions do. ``chroma="bilinear"`` interpolates it as decoders and scalers do, at the
stream's ``siting`` (``left``: MPEG-2 / H.264, the default; ``center``: JPEG; ``topleft``: HEVC / BT.2020;
``top``), in exact integers (``ops.image.chroma_upsample``) and in the same launch; the bottom sitings, and
bicubic or Lanczos chroma, are not offered. NV21 is the same class
with ``vu=True``; a software decoder's planar I420 / YV12 surface is :class:`Yuv420p`; OpenCV's BGR, a
compositor's RGBA / BGRA, and any of them (or RGB) as a crop or with padded rows is :class:`Packed` — a
non-contiguous RGB view may also be passed as it is. None of them is copied or converted first: every
layout has its staging loop in the one kernel, and equals the RGB path on the converted frame bit for bit.
All of them are a :class:`Frame`, which is all the processor and the model know about them. Further frames —
4:2:2 and 4:4:4, packed YUY2 / UYVY, 10 / 12-bit P010 / ``yuv420p10le`` and kin, BT.2020 — live in
:mod:`.surfaces`; nothing here names them.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ...ops import image as I

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class Frame:
    """An image batch of one size that is not a plain interleaved RGB tensor: what the processor and the model
    ask of it. A subclass is a frozen dataclass whose tensor fields are named in ``PLANES`` and answers
    :meth:`shape`, :meth:`rgb` and :meth:`patch_planes`. The buffers are held as they are given — a captured
    graph reads them by address."""
    PLANES: Tuple[str, ...] = ()

    @property
    def shape(self) -> Tuple[int, int, int, int]:
        """``(B, h, w, 3)``: the shape of the RGB batch this frame stands for."""
        raise NotImplementedError

    def rgb(self) -> torch.Tensor:
        """The frame converted: contiguous uint8 ``[B, h, w, 3]``."""
        raise NotImplementedError

    def patch_planes(self, hw: Tuple[int, int], patch: int, mean: Sequence[float], std: Sequence[float],
                     want_pixels: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """``ops.image.image_patch_planes`` of :meth:`rgb`, by this layout's fused launch."""
        raise NotImplementedError

    def tile_planes(self, origins, tile_hw: Tuple[int, int], hw: Tuple[int, int], patch: int, mean: Sequence[float],
                    std: Sequence[float], want_pixels: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """:meth:`patch_planes` of the tiles of this one frame, each ``tile_hw`` large at its ``(y0, x0)`` of
        ``origins`` and resized to ``hw``: ``ops.image.tiled_patch_planes`` of :meth:`rgb`. A layout with a tile
        launch of its own answers with that instead, bit for bit the same."""
        return I.tiled_patch_planes(self.rgb(), "rgb", origins, tile_hw, hw, patch, mean, std, want_pixels)

    @property
    def device(self) -> torch.device:
        return getattr(self, self.PLANES[0]).device

    @property
    def is_cuda(self) -> bool:
        return getattr(self, self.PLANES[0]).is_cuda

    def to(self, device) -> "Frame":
        """On ``device``; the same object (and the same buffers) when it is there already."""
        if device is None or self.device == torch.device(device):
            return self
        return replace(self, **{k: getattr(self, k).to(device) for k in self.PLANES})


def _buffer(buf: Any, who: str) -> torch.Tensor:
    t = torch.from_numpy(buf) if isinstance(buf, np.ndarray) else buf
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_contiguous():
        raise ValueError(f"{who}: a contiguous uint8 tensor or ndarray")
    return t


@dataclass(frozen=True)
class Nv12(Frame):
    """An NV12 frame (or a batch of one size): ``y`` uint8 ``[h, w]`` or ``[B, h, w]``, ``uv`` uint8
    ``[(h+1)//2, (w+1)//2, 2]`` (U, V) with the same leading ``B``; rows may be pitched. The planes are
    held as they are given — a captured graph reads them by address. ``vu``: the chroma pairs are (V, U),
    which makes it NV21."""
    y: torch.Tensor
    uv: torch.Tensor
    matrix: str = "bt601"
    full_range: bool = False
    vu: bool = False
    chroma: str = "nearest"
    siting: str = "left"
    transfer: str = "sdr"       # 8-bit samples: the only one (the field is there to refuse the others by name)
    PLANES = ("y", "uv")

    def __post_init__(self):
        I.nv12_planes(self.y, self.uv)
        I.nv12_table(self.matrix, self.full_range)
        I._chroma_check(self.chroma, self.siting)
        I._transfer_check(self.transfer, 1000.0, 8)

    @classmethod
    def from_buffer(cls, buf: Any, h: int, w: int, pitch: Optional[int] = None, matrix: str = "bt601",
                    full_range: bool = False, vu: bool = False, chroma: str = "nearest",
                    siting: str = "left") -> "Nv12":
        """A decoder's single surface — ``h`` rows of Y, then ``h / 2`` rows of UV, all ``pitch`` bytes
        apart (default ``w``) — as the two planes, without a copy. ``buf``: a contiguous uint8 tensor or
        ndarray of at least ``(3 h / 2 - 1) * pitch + 2 * ((w + 1) // 2)`` bytes."""
        t = _buffer(buf, "Nv12.from_buffer")
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
                   t.as_strided((h // 2, cw2 // 2, 2), (pitch, 2, 1), off + h * pitch), matrix, full_range, vu,
                   chroma, siting)

    def batched(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(y [B, h, w], uv [B, ch, cw, 2])`` views."""
        return I.nv12_planes(self.y, self.uv)

    @property
    def shape(self) -> Tuple[int, int, int, int]:
        return tuple(self.batched()[0].shape) + (3,)

    def rgb(self) -> torch.Tensor:
        """The frame converted: uint8 ``[B, h, w, 3]`` (``ops.image.nv12_to_rgb``)."""
        if self.chroma != "nearest":
            return I.nv12_to_rgb(self.y, self.uv, self.matrix, self.full_range, self.vu, self.chroma, self.siting)
        if self.vu:
            return I.nv12_to_rgb(self.y, self.uv, self.matrix, self.full_range, vu=True)
        return I.nv12_to_rgb(self.y, self.uv, self.matrix, self.full_range)

    def patch_planes(self, hw, patch, mean, std, want_pixels=False):
        if self.chroma != "nearest":    # the general entry's semi-planar 4:2:0 at depth 8
            return I.yuv_semiplanar_patch_planes(self.y, self.uv, hw, patch, mean, std, "420", 8, False, self.matrix,
                                                 self.full_range, want_pixels, self.vu, self.chroma, self.siting)
        if self.vu:
            return I.nv12_patch_planes(self.y, self.uv, hw, patch, mean, std, self.matrix, self.full_range,
                                       want_pixels, vu=True)
        return I.nv12_patch_planes(self.y, self.uv, hw, patch, mean, std, self.matrix, self.full_range, want_pixels)

    def tile_planes(self, origins, tile_hw, hw, patch, mean, std, want_pixels=False):
        # the general entry's semi-planar 4:2:0 at depth 8, with either chroma
        return I.yuv_semiplanar_tiled_patch_planes(self.y, self.uv, origins, tile_hw, hw, patch, mean, std, "420", 8,
                                                   False, self.matrix, self.full_range, want_pixels, self.vu,
                                                   self.chroma, self.siting)


@dataclass(frozen=True)
class Yuv420p(Frame):
    """A planar 4:2:0 frame (or a batch of one size): ``y`` uint8 ``[h, w]`` or ``[B, h, w]``, ``u`` and ``v``
    uint8 ``[(h+1)//2, (w+1)//2]`` with the same leading ``B``; every plane may have its own row pitch. The
    fields say what a plane holds, not where it lies: for YV12 pass the second plane of the surface as ``u``."""
    y: torch.Tensor
    u: torch.Tensor
    v: torch.Tensor
    matrix: str = "bt601"
    full_range: bool = False
    chroma: str = "nearest"
    siting: str = "left"
    transfer: str = "sdr"       # 8-bit samples: the only one (the field is there to refuse the others by name)
    PLANES = ("y", "u", "v")

    def __post_init__(self):
        I.yuv420_planes(self.y, self.u, self.v)
        I.nv12_table(self.matrix, self.full_range)
        I._chroma_check(self.chroma, self.siting)
        I._transfer_check(self.transfer, 1000.0, 8)

    @classmethod
    def from_buffer(cls, buf: Any, h: int, w: int, pitch: Optional[int] = None, chroma_pitch: Optional[int] = None,
                    order: str = "i420", matrix: str = "bt601", full_range: bool = False, chroma: str = "nearest",
                    siting: str = "left") -> "Yuv420p":
        """A software decoder's single surface — ``h`` rows of Y ``pitch`` bytes apart (default ``w``), then
        ``h / 2`` rows of the first chroma plane ``chroma_pitch`` apart (default ``pitch // 2``), then the
        second chroma plane — as the three planes, without a copy. ``order``: ``i420`` has U first, ``yv12``
        V first. ``buf``: a contiguous uint8 tensor or ndarray that holds all of it."""
        t = _buffer(buf, "Yuv420p.from_buffer")
        h, w = int(h), int(w)
        if order not in ("i420", "yv12"):
            raise ValueError(f"Yuv420p.from_buffer: order {order!r} is neither 'i420' nor 'yv12'")
        if h <= 0 or w <= 0 or h % 2:
            raise ValueError("Yuv420p.from_buffer: positive sizes and an even height (chroma rows follow the Y rows)")
        pitch = w if pitch is None else int(pitch)
        cpitch = pitch // 2 if chroma_pitch is None else int(chroma_pitch)
        cw, ch = (w + 1) // 2, h // 2
        if pitch < w:
            raise ValueError(f"Yuv420p.from_buffer: pitch {pitch} is smaller than a row of {w} pixels")
        if cpitch < cw:
            raise ValueError(f"Yuv420p.from_buffer: chroma pitch {cpitch} is smaller than a chroma row of {cw} bytes")
        need = h * pitch + (2 * ch - 1) * cpitch + cw
        if t.numel() < need:
            raise ValueError(f"Yuv420p.from_buffer: {h}x{w} at pitches {pitch} and {cpitch} takes {need} bytes, "
                             f"the buffer has {t.numel()}")
        off = t.storage_offset()
        first = t.as_strided((ch, cw), (cpitch, 1), off + h * pitch)
        second = t.as_strided((ch, cw), (cpitch, 1), off + h * pitch + ch * cpitch)
        u, v = (first, second) if order == "i420" else (second, first)
        return cls(t.as_strided((h, w), (pitch, 1), off), u, v, matrix, full_range, chroma, siting)

    def batched(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(y [B, h, w], u [B, ch, cw], v [B, ch, cw])`` views."""
        return I.yuv420_planes(self.y, self.u, self.v)

    @property
    def shape(self) -> Tuple[int, int, int, int]:
        return tuple(self.batched()[0].shape) + (3,)

    def rgb(self) -> torch.Tensor:
        """The frame converted: uint8 ``[B, h, w, 3]`` (``ops.image.yuv420_to_rgb``)."""
        if self.chroma != "nearest":
            return I.yuv420_to_rgb(self.y, self.u, self.v, self.matrix, self.full_range, self.chroma, self.siting)
        return I.yuv420_to_rgb(self.y, self.u, self.v, self.matrix, self.full_range)

    def patch_planes(self, hw, patch, mean, std, want_pixels=False):
        if self.chroma != "nearest":    # the general entry's planar 4:2:0 at depth 8
            return I.yuv_planar_patch_planes(self.y, self.u, self.v, hw, patch, mean, std, "420", 8, False, self.matrix,
                                             self.full_range, want_pixels, self.chroma, self.siting)
        return I.yuv420p_patch_planes(self.y, self.u, self.v, hw, patch, mean, std, self.matrix, self.full_range,
                                      want_pixels)

    def tile_planes(self, origins, tile_hw, hw, patch, mean, std, want_pixels=False):
        # the general entry's planar 4:2:0 at depth 8, with either chroma
        return I.yuv_planar_tiled_patch_planes(self.y, self.u, self.v, origins, tile_hw, hw, patch, mean, std, "420", 8,
                                               False, self.matrix, self.full_range, want_pixels, self.chroma,
                                               self.siting)


@dataclass(frozen=True)
class Packed(Frame):
    """Packed pixels in another order or at another pitch than a plain RGB tensor: ``data`` uint8 ``[h, w, C]``
    or ``[B, h, w, C]`` in ``order`` (``rgb``, ``bgr``: C = 3; ``rgba``, ``bgra``: C = 4, the fourth byte
    ignored). The bytes of a row are contiguous; rows and images lie wherever their strides put them, so a
    crop of a larger frame or a capture buffer with padded rows is read in place."""
    data: torch.Tensor
    order: str = "rgb"
    PLANES = ("data",)

    def __post_init__(self):
        if self.order not in I.PACKED_ORDERS:
            raise ValueError(f"Packed: channel order {self.order!r} is none of {sorted(I.PACKED_ORDERS)}")
        C = I.PACKED_ORDERS[self.order][0]
        d = self.data
        if not isinstance(d, torch.Tensor) or d.dtype != torch.uint8 or d.dim() not in (3, 4) or d.shape[-1] != C \
                or 0 in d.shape:
            raise ValueError(f"Packed: {self.order} takes a uint8 [h, w, {C}] or [B, h, w, {C}] tensor")
        if not I._packed_strides(self.batched()):
            raise ValueError("Packed: rows may be pitched, but the bytes of a row are contiguous")

    def batched(self) -> torch.Tensor:
        """The ``[B, h, w, C]`` view."""
        return self.data if self.data.dim() == 4 else self.data[None]

    @property
    def shape(self) -> Tuple[int, int, int, int]:
        return tuple(self.batched().shape[:3]) + (3,)

    def rgb(self) -> torch.Tensor:
        """The colour bytes re-ordered: contiguous uint8 ``[B, h, w, 3]`` (``ops.image.packed_to_rgb``)."""
        return I.packed_to_rgb(self.batched(), self.order)

    def patch_planes(self, hw, patch, mean, std, want_pixels=False):
        return I.packed_patch_planes(self.batched(), self.order, hw, patch, mean, std, want_pixels)

    def tile_planes(self, origins, tile_hw, hw, patch, mean, std, want_pixels=False):
        return I.tiled_patch_planes(self.batched(), self.order, origins, tile_hw, hw, patch, mean, std, want_pixels)


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
        a :class:`Frame` (:class:`Nv12`, :class:`Yuv420p`, :class:`Packed`) stays one (it answers ``shape``,
        ``device`` and ``is_cuda`` as the batch would)."""
        if isinstance(image, Frame):
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
        return I.pixels_reference(img.rgb() if isinstance(img, Frame) else img, hw, self.mean, self.std)

    def patch_planes(self, img: Any, hw: Tuple[int, int], want_pixels: bool = False, patch: Optional[int] = None) \
            -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """The x3 planes of the patch matrix (and the pixels on request) of :meth:`as_batch`'s result,
        resized to ``hw``: ``ops.image.image_patch_planes``, or the fused launch of a :class:`Frame`'s layout
        (``patch``: another patch side than the processor's)."""
        patch = self.patch if patch is None else patch
        if isinstance(img, Frame):
            return img.patch_planes(hw, patch, self.mean, self.std, want_pixels)
        return I.image_patch_planes(img, hw, patch, self.mean, self.std, want_pixels)

    @staticmethod
    def tile_plan(hw: Tuple[int, int], tiles: Tuple[int, int] = (2, 2), overlap: float = 0.2,
                  num_detection_tokens: int = 100) -> Tuple[int, int, list]:
        """``(th, tw, origins)`` of an ``(h, w)`` frame cut into ``tiles = (R, C)`` overlapping tiles of one size
        (``ops.image.tile_plan``); one call then runs one model size, ``size((th, tw))``."""
        return I.tile_plan(hw[0], hw[1], tiles, overlap, num_detection_tokens)

    @staticmethod
    def as_packed(img: Any) -> Tuple[torch.Tensor, str]:
        """``(data [1, h, w, C], order)`` of :meth:`as_batch`'s result for the packed tile launch and for the stacked
        crops: a tensor or a :class:`Packed` frame as it lies; any other :class:`Frame` (NV12, P010 and the rest)
        converted once by its ``rgb()``. (On the GPU such a frame's tiles need no conversion: its
        :meth:`Frame.tile_planes` stages them from the planes, which is what :meth:`frame_tile_planes` asks for.)"""
        if isinstance(img, Packed):
            data, order = img.batched(), img.order
        else:
            data, order = (img.rgb() if isinstance(img, Frame) else img), "rgb"
        if data.shape[0] != 1:
            raise ValueError(f"tiles are cut from one frame, not from a batch of {data.shape[0]}")
        return data, order

    def tile_planes(self, data: torch.Tensor, order: str, origins, tile_hw: Tuple[int, int], hw: Tuple[int, int],
                    want_pixels: bool = False, patch: Optional[int] = None) \
            -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """:meth:`patch_planes` of the tiles of one packed frame (:meth:`as_packed`), each ``tile_hw`` large at its
        ``(y0, x0)`` of ``origins`` and resized to ``hw``, by one launch (``ops.image.tiled_patch_planes``)."""
        return I.tiled_patch_planes(data, order, origins, tile_hw, hw, self.patch if patch is None else patch,
                                    self.mean, self.std, want_pixels)

    @staticmethod
    def tiles_in_place(img: Any) -> bool:
        """True for :meth:`as_batch`'s result when it is a :class:`Frame` other than :class:`Packed`: its tiles are
        staged by :meth:`frame_tile_planes`, not from :meth:`as_packed`'s pixels."""
        return isinstance(img, Frame) and not isinstance(img, Packed)

    def frame_tile_planes(self, frame: Frame, origins, tile_hw: Tuple[int, int], hw: Tuple[int, int],
                          want_pixels: bool = False, patch: Optional[int] = None) \
            -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """:meth:`tile_planes` of a :class:`Frame` as it lies, by the frame's own tile launch
        (:meth:`Frame.tile_planes`): a YUV frame is not converted first."""
        return frame.tile_planes(origins, tile_hw, hw, self.patch if patch is None else patch, self.mean, self.std,
                                 want_pixels)

    @staticmethod
    def results(count: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, boxes: torch.Tensor) \
            -> List[Dict[str, torch.Tensor]]:
        """The compacted device tensors of ``ops.image.detections`` as ``transformers`` returns them:
        one ``{"scores", "labels", "boxes"}`` per image (this reads ``count`` on the host). The merged tensors of
        ``ops.image.merge_detections`` (one list for the frame: ``scores [N]``) give one entry."""
        if scores.dim() == 1:
            scores, labels, boxes = scores[None], labels[None], boxes[None]
        return [{"scores": scores[i, :n], "labels": labels[i, :n].long(), "boxes": boxes[i, :n]}
                for i, n in enumerate(count.tolist())]

    @staticmethod
    def tracked_results(count: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, boxes: torch.Tensor,
                        track_id: torch.Tensor, track_hits: torch.Tensor, min_hits: int = 1) \
            -> List[Dict[str, torch.Tensor]]:
        """:meth:`results` of a tracked frame (``YolosSmall.track_image`` / ``track_tiled``), each entry with the
        rows' ``"ids"`` and ``"hits"``, restricted to the rows that have a track seen in at least ``min_hits`` frames
        (this reads ``count`` on the host)."""
        if scores.dim() == 1:
            scores, labels, boxes, track_id, track_hits = scores[None], labels[None], boxes[None], \
                track_id[None], track_hits[None]
        track_id, track_hits = track_id.reshape(scores.shape), track_hits.reshape(scores.shape)
        out = []
        for i, n in enumerate(count.tolist()):
            keep = (track_id[i, :n] > 0) & (track_hits[i, :n] >= min_hits)
            out.append({"scores": scores[i, :n][keep], "labels": labels[i, :n][keep].long(),
                        "boxes": boxes[i, :n][keep], "ids": track_id[i, :n][keep].long(),
                        "hits": track_hits[i, :n][keep].long()})
        return out

    def post_process(self, logits: torch.Tensor, boxes: torch.Tensor, threshold: float = 0.5,
                     target_sizes=None) -> List[Dict[str, torch.Tensor]]:
        """``post_process_object_detection``: per image the scores, labels and ``(x0, y0, x1, y1)`` boxes
        (in pixels of ``target_sizes`` = (height, width) per image, else 0..1) of the rows whose best
        class probability exceeds ``threshold``, in token order."""
        return self.results(*I.detections(logits, boxes, target_sizes, threshold))
