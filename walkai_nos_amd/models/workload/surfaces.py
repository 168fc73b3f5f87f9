"""Video surfaces beyond 8-bit 4:2:0: what a pod meets when its source is not an 8-bit H.264 decoder.

* :class:`YuvPlanar` — three planes: I422 / YV16, I444 / YV24, and ``yuv420p10le`` / ``yuv422p10le`` /
  ``yuv444p10le`` (I010 / I210 / I410) and their 12-bit forms, the value in the low bits of a 16-bit word.
* :class:`YuvSemiPlanar` — luma and interleaved chroma pairs: NV16 / NV61, NV24 / NV42, and a hardware decoder's
  P010 / P012 / P210 / P410, the value in the high bits of a 16-bit word.
* :class:`Yuyv` — packed 4:2:2 from capture: YUY2, UYVY, YVYU.

Each is a :class:`~walkai_nos_amd.models.workload.processor.Frame`, so the processor and the model take it wherever
an image goes, and each is read in place by one launch of the image kernel (``ops.image.yuv_*_patch_planes``), bit
equal to the RGB path on :meth:`rgb`. :func:`from_buffer` builds any of them, by name, over a decoder's single
buffer. BT.601, BT.709 and BT.2020 (non-constant luminance), limited or full range.

Chroma is taken nearest — luma ``(r, c)`` takes chroma ``(r >> vs, c >> hs)`` — unless a frame says
``chroma="bilinear"``: then it is interpolated in exact integers (``ops.image.chroma_upsample``), still inside the one
launch, at the frame's ``siting``:

========= =========== ========= ====================================
siting    horizontal  vertical  whose
========= =========== ========= ====================================
left      co-sited    centred   MPEG-2, H.264 (the default)
center    centred     centred   JPEG, MPEG-1
topleft   co-sited    co-sited  HEVC with BT.2020
top       centred     co-sited
========= =========== ========= ====================================

On 4:2:2 only the horizontal part applies; on 4:4:4 bilinear is nearest.

A 10 / 12-bit planar or semi-planar frame whose codes are PQ (HDR10) or HLG says ``transfer="pq"`` or ``"hlg"`` and,
if it knows it, the stream's ``peak_nits`` (default 1000): its R'G'B' codes are then not cut to 8 bits but tone-mapped
to sRGB bytes — transfer function, an extended Reinhard curve per channel from that peak to SDR white (203 nits in),
BT.2020 to BT.709 primaries, the sRGB OETF — by two tables and an integer matrix (``ops.image.hdr_tables``), still
inside the one launch. The default, ``"sdr"``, reads the codes as they are.

Not offered: the bottom sitings; bicubic or Lanczos chroma; luminance-based or BT.2390 tone mapping; dynamic metadata
(HDR10+, Dolby Vision); 8-bit HLG; linear or float surfaces; 16-bit-deep samples; Y210 / Y410 / AYUV; big-endian
samples; BT.2020 constant luminance; batches above one on the fused model path and mixed sizes in one call.

Every SDR frame here is also a target of ``ops.image.overlay`` (``models/workload/overlay.py``), which paints detections
into its planes in place. Not offered there: alpha blending; antialiased lines; class names or any glyph but digits; PQ
/ HLG surfaces (an SDR colour has no code without the inverse tone map); batches above one; more than 1024 rows.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Tuple

import numpy as np
import torch

from ...ops import image as I
from .processor import Frame


@dataclass(frozen=True)
class YuvPlanar(Frame):
    """A planar frame (or a batch of one size): ``y`` ``[h, w]`` or ``[B, h, w]``, ``u`` and ``v`` ``[ch, cw]`` with
    the same leading ``B`` — ``subsampling`` ``"420"``, ``"422"`` or ``"444"`` says which. uint8 at ``depth`` 8;
    ``torch.uint16`` (or ``int16``) words at depth 10 or 12, the value in the high bits with ``msb``, else in the
    low bits. Every plane may have its own row pitch. The fields say what a plane holds, not where it lies."""
    y: torch.Tensor
    u: torch.Tensor
    v: torch.Tensor
    subsampling: str = "420"
    depth: int = 8
    msb: bool = False
    matrix: str = "bt601"
    full_range: bool = False
    chroma: str = "nearest"
    siting: str = "left"
    transfer: str = "sdr"
    peak_nits: float = 1000.0
    PLANES = ("y", "u", "v")

    def __post_init__(self):
        I.yuv_planes(self.y, self.u, self.v, self.subsampling, self.depth)
        I.yuv_table(self.matrix, self.full_range, self.depth)
        I._chroma_check(self.chroma, self.siting)
        I._transfer_check(self.transfer, self.peak_nits, self.depth)

    @property
    def shape(self) -> Tuple[int, int, int, int]:
        return tuple(I.yuv_planes(self.y, self.u, self.v, self.subsampling, self.depth)[0].shape) + (3,)

    def rgb(self) -> torch.Tensor:
        """The frame converted: uint8 ``[B, h, w, 3]`` (``ops.image.yuv_to_rgb``)."""
        return I.yuv_to_rgb(self.y, self.u, self.v, self.subsampling, self.depth, self.msb, self.matrix,
                            self.full_range, self.chroma, self.siting, self.transfer, self.peak_nits)

    def patch_planes(self, hw, patch, mean, std, want_pixels=False):
        return I.yuv_planar_patch_planes(self.y, self.u, self.v, hw, patch, mean, std, self.subsampling, self.depth,
                                         self.msb, self.matrix, self.full_range, want_pixels, self.chroma, self.siting,
                                         self.transfer, self.peak_nits)

    def tile_planes(self, origins, tile_hw, hw, patch, mean, std, want_pixels=False):
        return I.yuv_planar_tiled_patch_planes(self.y, self.u, self.v, origins, tile_hw, hw, patch, mean, std,
                                               self.subsampling, self.depth, self.msb, self.matrix, self.full_range,
                                               want_pixels, self.chroma, self.siting, self.transfer, self.peak_nits)


@dataclass(frozen=True)
class YuvSemiPlanar(Frame):
    """A semi-planar frame (or a batch of one size): ``y`` ``[h, w]`` or ``[B, h, w]`` and ``uv`` ``[ch, cw, 2]``
    pairs of (U, V) — of (V, U) with ``vu`` — with the same leading ``B``; samples as in :class:`YuvPlanar`."""
    y: torch.Tensor
    uv: torch.Tensor
    subsampling: str = "420"
    depth: int = 8
    msb: bool = False
    matrix: str = "bt601"
    full_range: bool = False
    vu: bool = False
    chroma: str = "nearest"
    siting: str = "left"
    transfer: str = "sdr"
    peak_nits: float = 1000.0
    PLANES = ("y", "uv")

    def __post_init__(self):
        I.yuv_semiplanar_planes(self.y, self.uv, self.subsampling, self.depth)
        I.yuv_table(self.matrix, self.full_range, self.depth)
        I._chroma_check(self.chroma, self.siting)
        I._transfer_check(self.transfer, self.peak_nits, self.depth)

    @property
    def shape(self) -> Tuple[int, int, int, int]:
        return tuple(I.yuv_semiplanar_planes(self.y, self.uv, self.subsampling, self.depth)[0].shape) + (3,)

    def rgb(self) -> torch.Tensor:
        """The frame converted: uint8 ``[B, h, w, 3]`` (``ops.image.yuv_semiplanar_to_rgb``)."""
        return I.yuv_semiplanar_to_rgb(self.y, self.uv, self.subsampling, self.depth, self.msb, self.matrix,
                                       self.full_range, self.vu, self.chroma, self.siting, self.transfer,
                                       self.peak_nits)

    def patch_planes(self, hw, patch, mean, std, want_pixels=False):
        return I.yuv_semiplanar_patch_planes(self.y, self.uv, hw, patch, mean, std, self.subsampling, self.depth,
                                             self.msb, self.matrix, self.full_range, want_pixels, self.vu, self.chroma,
                                             self.siting, self.transfer, self.peak_nits)

    def tile_planes(self, origins, tile_hw, hw, patch, mean, std, want_pixels=False):
        return I.yuv_semiplanar_tiled_patch_planes(self.y, self.uv, origins, tile_hw, hw, patch, mean, std,
                                                   self.subsampling, self.depth, self.msb, self.matrix,
                                                   self.full_range, want_pixels, self.vu, self.chroma, self.siting,
                                                   self.transfer, self.peak_nits)


@dataclass(frozen=True)
class Yuyv(Frame):
    """Packed 4:2:2 (or a batch of one size): ``data`` uint8 ``[h, rowbytes]`` or ``[B, h, rowbytes]``, four-byte
    macropixels in ``order`` ``yuyv`` (YUY2), ``uyvy`` or ``yvyu``, of which ``width`` pixels are shown (an odd
    width leaves the last macropixel's second luma as padding). Rows lie wherever their pitch puts them."""
    data: torch.Tensor
    width: int
    order: str = "yuyv"
    matrix: str = "bt601"
    full_range: bool = False
    chroma: str = "nearest"
    siting: str = "left"
    transfer: str = "sdr"       # 8-bit samples: the only one (the field is there to refuse the others by name)
    PLANES = ("data",)

    def __post_init__(self):
        I.yuyv_planes(self.data, self.width, self.order)
        I.yuv_table(self.matrix, self.full_range, 8)
        I._chroma_check(self.chroma, self.siting)
        I._transfer_check(self.transfer, 1000.0, 8)

    @property
    def shape(self) -> Tuple[int, int, int, int]:
        return tuple(I.yuyv_planes(self.data, self.width, self.order)[0].shape) + (3,)

    def rgb(self) -> torch.Tensor:
        """The frame converted: uint8 ``[B, h, width, 3]`` (``ops.image.yuyv_to_rgb``)."""
        return I.yuyv_to_rgb(self.data, self.width, self.order, self.matrix, self.full_range, self.chroma, self.siting)

    def patch_planes(self, hw, patch, mean, std, want_pixels=False):
        return I.yuyv_patch_planes(self.data, self.width, self.order, hw, patch, mean, std, self.matrix,
                                   self.full_range, want_pixels, self.chroma, self.siting)

    def tile_planes(self, origins, tile_hw, hw, patch, mean, std, want_pixels=False):
        return I.yuyv_tiled_patch_planes(self.data, self.width, self.order, origins, tile_hw, hw, patch, mean, std,
                                         self.matrix, self.full_range, want_pixels, self.chroma, self.siting)


#: name -> (layout, subsampling, depth, value in the high bits, second chroma first)
FORMATS = {
    "i422": ("planar", "422", 8, False, False), "yv16": ("planar", "422", 8, False, True),
    "i444": ("planar", "444", 8, False, False), "yv24": ("planar", "444", 8, False, True),
    "nv16": ("semiplanar", "422", 8, False, False), "nv61": ("semiplanar", "422", 8, False, True),
    "nv24": ("semiplanar", "444", 8, False, False), "nv42": ("semiplanar", "444", 8, False, True),
    "yuy2": ("packed", "422", 8, False, False), "uyvy": ("packed", "422", 8, False, False),
    "yvyu": ("packed", "422", 8, False, False),
    "p010": ("semiplanar", "420", 10, True, False), "p012": ("semiplanar", "420", 12, True, False),
    "p210": ("semiplanar", "422", 10, True, False), "p410": ("semiplanar", "444", 10, True, False),
    "i010": ("planar", "420", 10, False, False), "i012": ("planar", "420", 12, False, False),
    "i210": ("planar", "422", 10, False, False), "i410": ("planar", "444", 10, False, False),
}
_YUYV = {"yuy2": "yuyv", "uyvy": "uyvy", "yvyu": "yvyu"}


def from_buffer(name: str, buf: Any, h: int, w: int, pitch: Optional[int] = None, chroma_pitch: Optional[int] = None,
                matrix: str = "bt601", full_range: bool = False, chroma: str = "nearest",
                siting: str = "left", transfer: str = "sdr", peak_nits: float = 1000.0) -> Frame:
    """A decoder's or a capture card's single buffer as a frame of format ``name`` (:data:`FORMATS`), without a
    copy. ``buf``: a contiguous uint8 tensor or ndarray that holds all of it. Pitches are in bytes.

    * packed (``yuy2`` / ``uyvy`` / ``yvyu``): ``h`` rows ``pitch`` apart (default ``4 * ceil(w / 2)``).
    * planar and semi-planar: ``h`` rows of Y ``pitch`` apart (default: a row's bytes, ``w`` times 1 or 2), then
      at byte ``h * pitch`` the chroma rows ``chroma_pitch`` apart — ``h / 2`` of them for 4:2:0 (an even ``h``),
      else ``h``. Semi-planar: one plane of pairs, ``chroma_pitch`` by default ``pitch`` (``2 * pitch`` for 4:4:4).
      Planar: two planes, the second ``rows * chroma_pitch`` after the first, ``chroma_pitch`` by default ``pitch
      // 2`` (``pitch`` for 4:4:4) — in both cases at least a chroma row's bytes (an odd width); ``yv16`` / ``yv24`` have V first, ``nv61`` / ``nv42`` (V, U) pairs.
    * 16-bit formats (``p...``: value in the high bits; ``i...``: in the low bits): little-endian words, so the
      buffer starts at an even byte and both pitches are even; the planes come out as ``torch.uint16`` views.

    ``chroma`` and ``siting``: how the frame's chroma is brought to the luma grid (``ops.image.CHROMA`` and
    ``SITINGS``). ``transfer`` (``ops.image.TRANSFERS``) and ``peak_nits``: a 10 / 12-bit format's codes are PQ or HLG
    and are tone-mapped to SDR from that peak."""
    who = f"from_buffer({name!r})"
    if name not in FORMATS:
        raise ValueError(f"{who}: an unknown format; one of {sorted(FORMATS)}")
    layout, sub, depth, msb, swap = FORMATS[name]
    I._transfer_check(transfer, peak_nits, depth)
    t = torch.from_numpy(buf) if isinstance(buf, np.ndarray) else buf
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_contiguous():
        raise ValueError(f"{who}: a contiguous uint8 tensor or ndarray")
    t = t.reshape(-1)
    h, w = int(h), int(w)
    hs, vs = I.YUV_SUBSAMPLING[sub]
    if h <= 0 or w <= 0:
        raise ValueError(f"{who}: positive sizes")
    if vs and h % 2:
        raise ValueError(f"{who}: 4:2:0 takes an even height (chroma rows follow the Y rows)")
    off = t.storage_offset()
    if layout == "packed":
        row = 4 * ((w + 1) // 2)
        pitch = row if pitch is None else int(pitch)
        if pitch < row:
            raise ValueError(f"{who}: pitch {pitch} is smaller than a row of {w} pixels ({row} bytes)")
        need = (h - 1) * pitch + row
        if t.numel() < need:
            raise ValueError(f"{who}: {h}x{w} at pitch {pitch} takes {need} bytes, the buffer has {t.numel()}")
        return Yuyv(t.as_strided((h, row), (pitch, 1), off), w, _YUYV[name], matrix, full_range, chroma, siting)
    sb = 1 if depth == 8 else 2
    cw, ch = (w + (1 << hs) - 1) >> hs, h >> vs
    yrow = w * sb
    crow = cw * sb * (2 if layout == "semiplanar" else 1)
    pitch = yrow if pitch is None else int(pitch)
    if chroma_pitch is not None:
        cpitch = int(chroma_pitch)
    elif layout == "semiplanar":
        cpitch = max(pitch if hs else 2 * pitch, crow)
    else:
        cpitch = max(pitch // 2 if hs else pitch, crow)
    if pitch < yrow:
        raise ValueError(f"{who}: pitch {pitch} is smaller than a row of {w} pixels ({yrow} bytes)")
    if cpitch < crow:
        raise ValueError(f"{who}: chroma pitch {cpitch} is smaller than a chroma row of {crow} bytes")
    if sb == 2 and (pitch % 2 or cpitch % 2 or off % 2):
        raise ValueError(f"{who}: 16-bit samples take even pitches and a buffer that starts at an even byte, not "
                         f"pitches {pitch} and {cpitch} at offset {off}")
    nplanes = 1 if layout == "semiplanar" else 2
    need = h * pitch + (nplanes * ch - 1) * cpitch + crow
    if t.numel() < need:
        raise ValueError(f"{who}: {h}x{w} at pitches {pitch} and {cpitch} takes {need} bytes, the buffer has "
                         f"{t.numel()}")
    # sample-sized elements: a 16-bit surface as uint16 words of the same storage
    e = t if sb == 1 else t[:t.numel() // 2 * 2].view(torch.uint16)
    eo = e.storage_offset()

    def plane(byte0: int, rows: int, cols: int, rowpitch: int, inner: Tuple[int, ...] = ()):
        size, stride = (rows, cols), (rowpitch // sb, 1)
        if inner:       # interleaved pairs
            size, stride = size + inner, (rowpitch // sb, 2, 1)
        return e.as_strided(size, stride, eo + byte0 // sb)
    y = plane(0, h, w, pitch)
    if layout == "semiplanar":
        return YuvSemiPlanar(y, plane(h * pitch, ch, cw, cpitch, (2,)), sub, depth, msb, matrix, full_range, swap,
                             chroma, siting, transfer, peak_nits)
    first, second = plane(h * pitch, ch, cw, cpitch), plane(h * pitch + ch * cpitch, ch, cw, cpitch)
    u, v = (second, first) if swap else (first, second)
    return YuvPlanar(y, u, v, sub, depth, msb, matrix, full_range, chroma, siting, transfer, peak_nits)
