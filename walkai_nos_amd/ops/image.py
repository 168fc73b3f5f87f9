"""The image half of the workload: a uint8 image to the patch-embedding GEMM's operand, and
``(logits, boxes)`` to detections — HIP kernels on the GPU (``csrc/image.hip``, ``libnos_image.so``),
PyTorch reference math on the CPU and with the ``torch`` backend, the conventions of
:mod:`walkai_nos_amd.ops.kernels`.

* :func:`resize_size` — the YOLOS processor's size rule (shortest edge, longest-edge clamp, both
  sides cropped to a multiple of 16).
* :func:`image_patch_planes` — antialiased triangle ("bilinear") resample at half-pixel centres,
  the per-channel affine ``v / (255 std) - mean / std``, and the x3 split of the im2col, in one
  launch. The tap tables are built on the host in fp64, rounded to fp32 and cached on the device per
  ``(h, w, H, W)``, so the kernel reads constants and a captured graph stays valid: tables handed out
  under capture are kept until :func:`invalidate_cache` (:mod:`.graph_cache`). Per-axis scales up
  to 4 (9 taps) run in the kernel; anything larger takes the torch composition.
* :func:`detections` — ``post_process_object_detection`` as one launch without a host
  synchronisation: softmax, best of the first ``L`` classes, corner boxes in pixels of the original
  image, and the rows above the threshold compacted in token order, ``count`` written on the device.

The resample is what ``F.interpolate(..., mode="bilinear", antialias=True, align_corners=False)``
computes, which is PIL's ``BILINEAR`` resize in float. Unlike the ``transformers`` processor nothing
is rounded to uint8 between the two passes, so pixels differ from it by less than one uint8 step.

* :func:`nv12_to_rgb` / :func:`nv12_patch_planes` — the same from a video decoder's NV12 surface (a
  full-resolution Y plane and a half-resolution interleaved UV plane, each with its own row pitch):
  the colour conversion happens while the kernel stages a patch's source footprint, so no RGB frame
  is materialised. The conversion is defined in integers (:func:`nv12_table`), so the fused result is
  bit-equal to :func:`image_patch_planes` of :func:`nv12_to_rgb`. Chroma is taken nearest — luma
  ``(r, c)`` uses chroma ``(r >> 1, c >> 1)``, what the usual one-call library conversions do —
  unless ``chroma="bilinear"`` is asked for (below).
* :func:`yuv420_to_rgb` / :func:`yuv420p_patch_planes` — planar 4:2:0 (I420 / YV12: what a software decoder and
  most JPEG decoders give), three planes with a pitch each; ``nv12_patch_planes(..., vu=True)`` is NV21. The
  planar function is the definition of the conversion: :func:`nv12_to_rgb` is it on the de-interleaved planes.
* :func:`packed_patch_planes` — BGR, RGBA and BGRA, and RGB at any row pitch, batch stride and alignment: a
  crop ``frame[:, y0:y1, x0:x1]`` or a padded capture buffer is read in place. :func:`image_patch_planes`
  sends a non-contiguous RGB view there instead of copying it.
* :func:`yuv_to_rgb` / :func:`yuv_planar_patch_planes`, :func:`yuv_semiplanar_patch_planes`,
  :func:`yuyv_patch_planes` — the rest of the YUV front end behind one launch descriptor (:class:`NosYuvSrc`):
  4:2:2 and 4:4:4 beside 4:2:0, packed 4:2:2 (YUY2 / UYVY / YVYU), and 10 / 12-bit codes in 16-bit words (P010's
  high bits or ``yuv420p10le``'s low bits; the other bits are ignored), with BT.2020 (non-constant luminance)
  beside the two older matrices (:func:`yuv_table`). 16-bit-deep samples, Y210 / Y410 / AYUV and big-endian words
  are not offered.
* :func:`hdr_tables` / :func:`hdr_to_sdr` — ``transfer="pq"`` or ``"hlg"`` (:data:`TRANSFERS`) on a 10 / 12-bit planar
  or semi-planar frame: the R'G'B' codes at the source's depth go through a table (transfer function and an extended
  Reinhard curve from ``peak_nits`` to SDR white, per channel), a 3 x 3 integer gamut matrix (BT.2020 to BT.709
  primaries) and a second table (the sRGB OETF), all built in fp64 on the host and cached on the device; the kernel's
  staging loop knows only the tables. The default stays ``"sdr"``. Luminance-based or BT.2390 tone mapping, dynamic
  metadata, 8-bit HLG and linear or float surfaces are not offered.
* :func:`chroma_upsample` — ``chroma="bilinear", siting=...`` on every ``*_to_rgb`` and on the general entry's
  ``*_patch_planes``: chroma interpolated as decoders and scalers do, honouring where the stream's chroma samples
  lie (:data:`SITINGS`: ``left``, ``center``, ``topleft``, ``top``), in exact integers — two taps per subsampled
  axis, weights in quarters, ``(sum + 8) >> 4`` — inside the same launch's staging loop. The default stays
  ``"nearest"``. The bottom sitings and bicubic / Lanczos chroma are not offered.

Every layout is bit-equal to :func:`image_patch_planes` of the converted or re-ordered contiguous RGB frame,
which is also what runs on the CPU, with the ``torch`` backend and past a layout's footprint limit.

* :func:`tile_plan` / :func:`tiled_patch_planes` / :func:`merge_detections` — tiled ("sliced") detection of a frame
  too large to shrink to one model input: ``R x C`` overlapping tiles of one size, staged as one batch by one launch
  (the packed staging loops with a per-tile byte offset from a cached device table), and the tiles' detections mapped
  to frame pixels and merged by one launch — ordered by score, a box dropped when a kept box of the same label from
  *another* tile overlaps it by more than ``match_threshold`` (``inter / min(area)`` by default, or IoU). Tiles of
  unequal size, merging boxes instead of suppressing and more than 1024 rows are not offered.
* :func:`yuv_planar_tiled_patch_planes`, :func:`yuv_semiplanar_tiled_patch_planes`, :func:`yuyv_tiled_patch_planes` —
  the tiles of one YUV frame staged straight from its planes by one launch (every layout, depth, chroma mode and
  transfer of the general YUV front end; the tile origins come from :func:`origin_tensor`'s table, the one the merge
  reads), bit-equal to :func:`tiled_patch_planes` of the converted frame: no RGB frame is written and read back.
* :func:`track_state` / :func:`track_update` — the detections of successive frames associated on the device: a greedy
  IoU tracker with an optional constant-velocity prediction (:data:`MOTIONS`) as one launch per frame. Its state
  (:class:`TrackState`) lives in device buffers updated in place, so each replay of a captured graph is the next frame;
  the ids come back in the row order of the lists passed in. Kalman filtering, appearance features, Hungarian
  assignment, a second pass on low scores and more than 1024 tracks are not offered.
* :func:`overlay` / :func:`overlay_codes` / :func:`overlay_palette` — the write side: one frame's detections (and ids)
  painted into the frame's own planes by one launch, on every SDR layout the front end reads — outlines, id tags in
  5 x 7 digits (:data:`OVERLAY_FONT`) and redactions, in exact integers, colours turned into the surface's codes once
  on the host in fp64. No RGB frame, no host sync, no copy; :func:`overlay_reference` is the torch composition. Alpha
  blending, antialiased lines, class names or any glyph but digits, PQ / HLG surfaces, batches above one and more than
  1024 rows are not offered.
"""
from __future__ import annotations

import ctypes
import math
import threading
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import kernels as K
from .graph_cache import GraphCache
from .native import NativeUnavailable, available, load

LIB = "libnos_image.so"
#: weights per output row / column, and the per-axis scale they cover (``csrc/image.hip``)
TAPS = 9
MAX_SCALE = 4.0
MAX_PATCH = 16
MAX_FOOTPRINT = 72
#: columns of a patch's footprint the NV12 staging loop takes (4-column groups in the same LDS row)
NV12_MAX_FOOTPRINT = 69
#: the same for planar 4:2:0 and for packed pixels read through pitches (all of them stage 4-column groups)
YUV420P_MAX_FOOTPRINT = 69
PACKED_MAX_FOOTPRINT = 69
#: and for the general YUV entry (4:2:2, 4:4:4, packed 4:2:2, 10 / 12-bit samples)
YUV_MAX_FOOTPRINT = 69
#: packed channel orders: bytes per pixel and the index of red, green and blue in a pixel
PACKED_ORDERS = {"rgb": (3, (0, 1, 2)), "bgr": (3, (2, 1, 0)), "rgba": (4, (0, 1, 2)), "bgra": (4, (2, 1, 0))}
#: detections kernel limits: rows per image, classes with "no object"
MAX_ROWS, MAX_CLASSES = 1024, 128

_lib: Optional[ctypes.CDLL] = None
_lock = threading.Lock()


def hip_available() -> bool:
    return available(LIB)


def _L() -> ctypes.CDLL:
    global _lib
    with _lock:
        if _lib is None:
            L = load(LIB)
            vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
            fp = ctypes.POINTER(ctypes.c_float)
            i64, ip = ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)
            src, hdr = ctypes.POINTER(NosYuvSrc), ctypes.POINTER(NosYuvHdr)
            # what every image entry takes behind its source, from the output planes on (:func:`_tail_args`)
            tail = [vp] * 6 + [i32] * 5 + [fp, fp] + [i32] * 9 + [vp]
            L.nos_image_patch_planes_u8.argtypes = [vp] + tail
            L.nos_image_patch_planes_nv12.argtypes = [vp] * 6 + [i64] * 4 + [ip] + tail
            L.nos_image_patch_planes_nv12_order.argtypes = L.nos_image_patch_planes_nv12.argtypes + [i32]
            L.nos_image_patch_planes_yuv420p.argtypes = [vp] * 9 + [i64] * 6 + [ip] + tail
            L.nos_image_patch_planes_packed.argtypes = [vp, vp, vp, i64, i64, ctypes.c_char_p] + tail
            L.nos_image_patch_planes_yuv.argtypes = [src] + tail
            L.nos_image_patch_planes_yuv_hdr.argtypes = [src, hdr] + tail
            L.nos_detections_f32.argtypes = [vp, vp, vp, f32, i32, i32, i32, vp, vp, vp, vp, vp]
            L.nos_image_patch_planes_tiles.argtypes = [vp, vp, vp, i64, ctypes.c_char_p, ip, vp, i32, i32] + tail
            L.nos_image_patch_planes_yuv_tiles.argtypes = [src, hdr, ip, vp, i32, i32, i32] + tail
            L.nos_merge_detections_f32.argtypes = [vp, vp, vp, f32, f32, f32, f32, i32, i32, i32, i32, vp, vp, vp, vp,
                                                   vp, vp]
            L.nos_track_update_f32.argtypes = [vp] * 4 + [i32] + [vp] * 8 + [i32, f32, i32, f32, i32, f32, vp, vp, vp]
            # the lists, the tables and the parameters both overlay entries take behind their surface
            drawn = [vp] * 6 + [i32, vp, i32, vp, i32, vp, i32, i32, i32, vp]
            L.nos_overlay_packed.argtypes = [vp, vp, vp, i64, ctypes.c_char_p, i32, i32] + drawn
            L.nos_overlay_yuv.argtypes = [src, i32, i32] + drawn
            L.nos_image_last_error.restype = ctypes.c_char_p
            if (L.nos_overlay_tile_rows(), L.nos_overlay_tile_columns()) != OVERLAY_TILE:
                raise NativeUnavailable(f"{LIB} was built with another overlay tile than ops/image.py expects")
            if (L.nos_image_taps(), L.nos_image_max_footprint(), L.nos_image_max_patch(),
                    L.nos_image_nv12_max_footprint(), L.nos_image_yuv420p_max_footprint(),
                    L.nos_image_packed_max_footprint(), L.nos_image_yuv_max_footprint()) != \
                    (TAPS, MAX_FOOTPRINT, MAX_PATCH, NV12_MAX_FOOTPRINT, YUV420P_MAX_FOOTPRINT, PACKED_MAX_FOOTPRINT,
                     YUV_MAX_FOOTPRINT):
                raise NativeUnavailable(f"{LIB} was built with other limits than ops/image.py expects")
            _lib = L
        return _lib


def _use_hip(t: torch.Tensor) -> bool:
    if not t.is_cuda or K.get_backend() == "torch":
        return False
    if not hip_available():
        raise NativeUnavailable(f"{LIB} is not built but a GPU tensor reached the HIP op path")
    return True


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"nos {what} failed: {_L().nos_image_last_error().decode()} (rc={rc})")


def image_wgs() -> int:
    """Workgroups of the preprocess kernel (grid-stride over patches): one per patch on the whole
    GPU; on a slice that shares the GPU, 4 per CU of the slice (as ``kernels.layernorm_wgs``)."""
    cus = K.slice_cus()
    return 0 if cus >= K.total_cus() else 4 * cus


# ---- the size rule ------------------------------------------------------------------------------
def resize_size(hw: Tuple[int, int], shortest: int = 800, longest: Optional[int] = 1333,
                mod: Optional[int] = 16) -> Tuple[int, int]:
    """``(H, W)`` the YOLOS processor resizes an ``(h, w)`` image to: the shortest edge to
    ``shortest`` unless the longest would pass ``longest``, the other edge truncated, then both
    cropped to a multiple of ``mod``."""
    h, w = int(hw[0]), int(hw[1])
    size, raw = int(shortest), None
    if longest is not None:
        lo, hi = float(min(h, w)), float(max(h, w))
        if hi / lo * size > longest:
            raw = longest * lo / hi
            size = int(round(raw))
    if w < h:
        ow = size
        oh = int((raw if raw is not None else size) * h / w)
    elif (h <= w and h == size) or (w <= h and w == size):
        oh, ow = h, w
    else:
        oh = size
        ow = int((raw if raw is not None else size) * w / h)
    if mod is not None:
        ow -= ow % mod
        oh -= oh % mod
    return oh, ow


# ---- the resample -------------------------------------------------------------------------------
def tap_table(n_in: int, n_out: int, taps: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The antialiased triangle filter of one axis in fp64: ``(first [n_out], count [n_out],
    weights [n_out, taps])``. Output ``i`` is ``sum_k weights[i, k] * src[first[i] + k]`` over
    ``k < count[i]``: centre ``(i + 0.5) * n_in / n_out``, support ``max(scale, 1)``, weights
    normalised to sum 1 (so the edges renormalise instead of clamping)."""
    scale = n_in / n_out
    support = scale if scale >= 1.0 else 1.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    centre = scale * (np.arange(n_out, dtype=np.float64) + 0.5)
    first = np.maximum((centre - support + 0.5).astype(np.int64), 0)
    count = np.minimum((centre + support + 0.5).astype(np.int64), n_in) - first
    width = int(count.max()) if taps is None else taps
    if count.max() > width:
        raise ValueError(f"tap_table: {int(count.max())} taps at scale {scale:.3f}, room for {width}")
    k = np.arange(width, dtype=np.float64)
    x = (k[None, :] + first[:, None] - centre[:, None] + 0.5) * inv
    wt = np.clip(1.0 - np.abs(x), 0.0, None) * (k[None, :] < count[:, None])
    wt /= wt.sum(axis=1, keepdims=True)
    return first, count, wt


def resample_matrix(n_in: int, n_out: int) -> torch.Tensor:
    """The tap table of one axis as a dense fp64 ``[n_out, n_in]`` matrix."""
    first, count, wt = tap_table(n_in, n_out)
    m = np.zeros((n_out, n_in), dtype=np.float64)
    for k in range(wt.shape[1]):
        rows = np.nonzero(k < count)[0]
        m[rows, first[rows] + k] = wt[rows, k]
    return torch.from_numpy(m)


def resample_reference(img: torch.Tensor, out_hw: Tuple[int, int]) -> torch.Tensor:
    """The fp64 definition of the resample, from the tap tables: ``img`` ``[..., h, w]`` (any real
    dtype) -> ``[..., H, W]`` float64."""
    h, w = img.shape[-2:]
    return resample_matrix(h, out_hw[0]) @ img.double().cpu() @ resample_matrix(w, out_hw[1]).t()


#: the tap tables per ``(h, w, H, W, p, device)``. A launch recorded in a graph reads them by address, so
#: an entry handed out under capture stays until :func:`invalidate_cache`; of the sizes only seen
#: eagerly the 16 most recently used are kept (about 44 bytes per output row and column each: 80 KB
#: at 800 x 1056, so the bound is on the number of stale sizes, not on memory that matters). The tile-origin tables
#: of :func:`tiled_patch_planes` and :func:`origin_tensor` (a few dozen bytes each) live here too, under keys that
#: begin with ``"tiles"`` / ``"origins"``
_tables = GraphCache(16)


def invalidate_cache() -> None:
    """Drop every cached tap table, tile-origin table, HDR table and overlay table, also those a captured graph holds: capture such
    graphs again."""
    _tables.clear()
    _hdr_tables.clear()
    _overlay_tables.clear()


def _make_tables(h: int, w: int, H: int, W: int, p: int, device: torch.device) -> Optional[tuple]:
    if h / H > MAX_SCALE or w / W > MAX_SCALE:
        return None
    out = []
    for n_in, n_out in ((h, H), (w, W)):
        first, count, wt = tap_table(n_in, n_out, TAPS)
        starts = np.arange(0, n_out, p)
        lasts = np.minimum(starts + p, n_out) - 1
        out.append((first, count, wt, int((first[lasts] + count[lasts] - first[starts]).max())))
    if any(o[3] > MAX_FOOTPRINT for o in out):
        return None
    dev = []
    for first, count, wt, _ in out:
        dev.append(torch.from_numpy(np.stack((first, count)).astype(np.int32)).to(device))
        dev.append(torch.from_numpy(wt.astype(np.float32)).to(device))
    return dev[0], dev[1], dev[2], dev[3], out[0][3], out[1][3]


def _device_tables(h: int, w: int, H: int, W: int, p: int, device: torch.device) -> Optional[tuple]:
    """``(yidx, ywt, xidx, xwt, max_fh, max_fw)`` on ``device``, cached (:data:`_tables`); None when an
    axis needs more than ``TAPS`` weights or a patch's source footprint does not fit the kernel's LDS
    tile."""
    return _tables.get((h, w, H, W, p, str(device)), lambda: _make_tables(h, w, H, W, p, device))


def affine(mean: Sequence[float], std: Sequence[float]) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """``(a, b)`` with ``pixel = u8 * a_c + b_c``: ``a_c = 1 / (255 std_c)``, ``b_c = -mean_c / std_c``."""
    return tuple(1.0 / (255.0 * s) for s in std), tuple(-m / s for m, s in zip(mean, std))


def im2col(pixels: torch.Tensor, patch: int) -> torch.Tensor:
    """``[B, C, H, W]`` -> ``[B*gh*gw, C*p*p]``: row ``(b, i, j)``, column ``(c, u, v)``."""
    B, C, H, W = pixels.shape
    gh, gw = H // patch, W // patch
    return pixels[:, :, :gh * patch, :gw * patch].reshape(B, C, gh, patch, gw, patch) \
        .permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * patch * patch)


def pixels_reference(img_u8: torch.Tensor, out_hw: Tuple[int, int], mean: Sequence[float], std: Sequence[float],
                     dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The torch composition: ``[B, h, w, 3]`` uint8 -> ``[B, 3, H, W]`` in ``dtype``."""
    a, b = affine(mean, std)
    x = F.interpolate(img_u8.permute(0, 3, 1, 2).to(dtype), size=tuple(out_hw), mode="bilinear", antialias=True,
                      align_corners=False)
    # (the permuted view makes interpolate answer channels-last: the model takes plain NCHW)
    return (x * torch.tensor(a, dtype=dtype, device=x.device).view(1, 3, 1, 1)
            + torch.tensor(b, dtype=dtype, device=x.device).view(1, 3, 1, 1)).contiguous()


def fusable(hw: Tuple[int, int], out_hw: Tuple[int, int], patch: int) -> bool:
    """True when the kernel can take this resize: even patch side up to 16, at least one whole patch,
    and per-axis scales up to 4."""
    return (patch % 2 == 0 and 2 <= patch <= MAX_PATCH and out_hw[0] >= patch and out_hw[1] >= patch
            and hw[0] / out_hw[0] <= MAX_SCALE and hw[1] / out_hw[1] <= MAX_SCALE)


def _fused_tables(t: torch.Tensor, hw: Tuple[int, int], out_hw: Tuple[int, int], patch: int, limit: int) \
        -> Optional[tuple]:
    """The tap tables (:func:`_device_tables`) when the HIP launch takes this call — ``t`` on the GPU, a resize the
    kernel can take (:func:`fusable`) and no patch footprint wider than ``limit`` columns, the layout's
    ``*_MAX_FOOTPRINT`` — else None: the torch composition runs."""
    if not (_use_hip(t) and fusable(hw, out_hw, patch)):
        return None
    tabs = _device_tables(hw[0], hw[1], out_hw[0], out_hw[1], patch, t.device)
    return None if tabs is None or tabs[5] > limit else tabs


def image_patch_planes(img_u8: torch.Tensor, out_hw: Tuple[int, int], patch: int, mean: Sequence[float],
                       std: Sequence[float], want_pixels: bool = False) \
        -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """``[B, h, w, 3]`` uint8 (interleaved RGB) -> ``(planes [3, B*gh*gw, 3*p*p] bf16, pixels
    [B, 3, H, W] fp32 or None)``: resized to ``out_hw``, normalised, and split into the x3 planes of
    the patch matrix (``kernels.patch_planes``' layout). One HIP launch on the GPU; on a CPU tensor,
    with the ``torch`` backend, or past the kernel's limits (:func:`fusable`), the fp32 torch
    composition and ``split3`` of its im2col. A view whose pixels are whole but whose rows or images
    are not adjacent (a crop, a padded buffer) is read in place (:func:`packed_patch_planes`)."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[-1] != 3:
        raise ValueError("image_patch_planes: a uint8 [B, h, w, 3] image")
    B, h, w, _ = img_u8.shape
    H, W = int(out_hw[0]), int(out_hw[1])
    tabs = _fused_tables(img_u8, (h, w), (H, W), patch, MAX_FOOTPRINT)
    if tabs is None:
        px = pixels_reference(img_u8, (H, W), mean, std)
        return K.split3(im2col(px, patch)), (px if want_pixels else None)
    if not img_u8.is_contiguous() and _packed_strides(img_u8) and tabs[5] <= PACKED_MAX_FOOTPRINT:
        return packed_patch_planes(img_u8, "rgb", (H, W), patch, mean, std, want_pixels)
    img = img_u8.contiguous()
    planes, pixels, gh, gw = _outputs(B, H, W, patch, want_pixels, img.device)
    rc = _L().nos_image_patch_planes_u8(img.data_ptr(),
                                        *_tail_args(tabs, planes, pixels, mean, std, B, h, w, H, W, patch, gh, gw))
    _check(rc, "image_patch_planes")
    return planes, pixels


# ---- NV12 ---------------------------------------------------------------------------------------
#: ``(Kr, Kb)`` of the luma equation ``Y = Kr R + Kg G + Kb B``
NV12_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def nv12_real_matrix(matrix: str = "bt601", full_range: bool = False) -> Tuple[np.ndarray, Tuple[int, int, int]]:
    """The conversion in real numbers, derived in fp64 from ``(Kr, Kb)``: ``(M [3, 3], offsets)`` with
    ``rgb = M @ ((Y, U, V) - offsets)``. Limited range scales Y by 255/219 and chroma by 255/224 and
    takes 16 from Y; both ranges take 128 from chroma."""
    if matrix not in NV12_MATRICES:
        raise ValueError(f"nv12: matrix {matrix!r} is none of {sorted(NV12_MATRICES)}")
    kr, kb = NV12_MATRICES[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    m = np.array([[sy, 0.0, sc * 2.0 * (1.0 - kr)],
                  [sy, -sc * 2.0 * kb * (1.0 - kb) / kg, -sc * 2.0 * kr * (1.0 - kr) / kg],
                  [sy, sc * 2.0 * (1.0 - kb), 0.0]], dtype=np.float64)
    return m, (0 if full_range else 16, 128, 128)


def nv12_table(matrix: str = "bt601", full_range: bool = False) -> Tuple[int, ...]:
    """The 12 integers both :func:`nv12_to_rgb` and the kernel compute with: the matrix of
    :func:`nv12_real_matrix` as ``round(real * 2^16)`` by rows (R, G, B) x (Y, U, V), then the three
    offsets. Channel ``c`` is ``clip((t[3c] (Y - t[9]) + t[3c+1] (U - t[10]) + t[3c+2] (V - t[11]) +
    2^15) >> 16, 0, 255)``."""
    m, off = nv12_real_matrix(matrix, full_range)
    return tuple(int(v) for v in np.rint(m * 65536.0).astype(np.int64).reshape(-1)) + tuple(off)


def nv12_planes(y: torch.Tensor, uv: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two planes of an NV12 frame as ``[B, h, w]`` and ``[B, (h+1)//2, (w+1)//2, 2]`` views, checked:
    uint8, one device, matching shapes, rows possibly pitched but contiguous inside."""
    if not isinstance(y, torch.Tensor) or not isinstance(uv, torch.Tensor) or y.dtype != torch.uint8 \
            or uv.dtype != torch.uint8:
        raise ValueError("nv12: the Y and UV planes are uint8 tensors")
    if y.dim() == 2 and uv.dim() == 3:
        y, uv = y[None], uv[None]
    if y.dim() != 3 or uv.dim() != 4 or 0 in y.shape:
        raise ValueError("nv12: Y is [B, h, w] (or [h, w]) and UV [B, (h+1)//2, (w+1)//2, 2] (or without B)")
    B, h, w = y.shape
    if tuple(uv.shape) != (B, (h + 1) // 2, (w + 1) // 2, 2):
        raise ValueError(f"nv12: a {h}x{w} Y plane takes a UV plane of shape "
                         f"{(B, (h + 1) // 2, (w + 1) // 2, 2)}, not {tuple(uv.shape)}")
    if y.device != uv.device:
        raise ValueError(f"nv12: both planes on one device, not {y.device} and {uv.device}")
    if (w > 1 and y.stride(2) != 1) or uv.stride(3) != 1 or (uv.shape[2] > 1 and uv.stride(2) != 2):
        raise ValueError("nv12: rows may be pitched, but the bytes of a row are contiguous (U, V interleaved)")
    return y, uv


def yuv420_planes(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, any_strides: bool = False) \
        -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The three planes of a planar 4:2:0 frame as ``[B, h, w]`` and two ``[B, (h+1)//2, (w+1)//2]`` views,
    checked: uint8, one device, matching shapes, each plane's rows possibly pitched but contiguous inside
    (``any_strides``: not even that, for the torch definition, which reads the halves of an interleaved plane)."""
    if not all(isinstance(t, torch.Tensor) and t.dtype == torch.uint8 for t in (y, u, v)):
        raise ValueError("yuv420: the Y, U and V planes are uint8 tensors")
    if y.dim() == 2 and u.dim() == 2 and v.dim() == 2:
        y, u, v = y[None], u[None], v[None]
    if y.dim() != 3 or u.dim() != 3 or v.dim() != 3 or 0 in y.shape:
        raise ValueError("yuv420: Y is [B, h, w] (or [h, w]) and U, V [B, (h+1)//2, (w+1)//2] (or without B)")
    B, h, w = y.shape
    want = (B, (h + 1) // 2, (w + 1) // 2)
    if tuple(u.shape) != want or tuple(v.shape) != want:
        raise ValueError(f"yuv420: a {h}x{w} Y plane takes U and V planes of shape {want}, not {tuple(u.shape)} "
                         f"and {tuple(v.shape)}")
    if y.device != u.device or y.device != v.device:
        raise ValueError(f"yuv420: all planes on one device, not {y.device}, {u.device} and {v.device}")
    if not any_strides and any(t.shape[2] > 1 and t.stride(2) != 1 for t in (y, u, v)):
        raise ValueError("yuv420: rows may be pitched, but the bytes of a row are contiguous")
    return y, u, v


#: how chroma is brought to the luma grid: ``nearest`` — luma ``(r, c)`` takes chroma ``(r >> vs, c >> hs)`` — or
#: ``bilinear`` (:func:`chroma_upsample`)
CHROMA = ("nearest", "bilinear")
#: where a chroma sample lies (ffmpeg's / H.273's names) -> bit 0: horizontally co-sited with the even luma columns,
#: bit 1: vertically co-sited with the even luma rows; a clear bit is centred between the pair. ``left`` is MPEG-2's
#: and H.264's default, ``center`` JPEG's and MPEG-1's, ``topleft`` HEVC's for BT.2020. (``NosYuvSrc.siting``)
SITINGS = {"left": 1, "center": 0, "topleft": 3, "top": 2}


def _chroma_check(chroma: str, siting: str) -> None:
    if chroma not in CHROMA:
        raise ValueError(f"yuv: chroma {chroma!r} is none of {CHROMA}")
    if siting not in SITINGS:
        raise ValueError(f"yuv: siting {siting!r} is none of {tuple(SITINGS)}")


def _chroma_axis(n: int, nc: int, sub: int, cosited: bool, device) -> Tuple[torch.Tensor, ...]:
    """The two taps of every luma position of one axis: ``(i0, i1, w0, w1)``, indices clamped to the plane,
    weights in quarters. (Arithmetic on an ``arange``: nothing is copied from the host.)"""
    x = torch.arange(n, device=device)
    if not sub:
        return x, x, torch.full_like(x, 4), torch.zeros_like(x)
    i, odd = x >> 1, x & 1
    if cosited:     # even: (4, 0) of C[i], C[i]; odd: (2, 2) of C[i], C[i + 1]
        i0, i1, w0, w1 = i, i + odd, 4 - 2 * odd, 2 * odd
    else:           # even: (1, 3) of C[i - 1], C[i]; odd: (3, 1) of C[i], C[i + 1]
        i0, i1, w0, w1 = i - 1 + odd, i + odd, 1 + 2 * odd, 3 - 2 * odd
    return i0.clamp(0, nc - 1), i1.clamp(0, nc - 1), w0, w1


def chroma_upsample(codes: torch.Tensor, h: int, w: int, hs: int, vs: int, siting: str = "left") -> torch.Tensor:
    """Bilinear chroma in exact integers: int32 codes ``[B, ch, cw]`` of a plane subsampled by ``2^hs`` x ``2^vs``
    -> ``[B, h, w]`` codes of the same depth — what the kernel computes with ``chroma="bilinear"``. Per subsampled
    axis luma position ``x`` has ``i = x >> 1`` and takes two samples with weights in quarters:

    ========== ============================ ==============================
    the axis   even ``x``                   odd ``x``
    ========== ============================ ==============================
    co-sited   ``(4, 0)`` of C[i], C[i]     ``(2, 2)`` of C[i], C[i + 1]
    centred    ``(1, 3)`` of C[i - 1], C[i] ``(3, 1)`` of C[i], C[i + 1]
    ========== ============================ ==============================

    with indices clamped to the plane; an axis that is not subsampled has ``(4, 0)`` on the sample itself. The
    result is ``(sum of wy * wx * C over the 2 x 2 taps + 8) >> 4``, that is ``(wx0 C0 + wx1 C1 + 2) >> 2`` for
    4:2:2: round-half-up of the linear interpolation at the luma position. ``siting`` (:data:`SITINGS`): ``left``
    is co-sited horizontally and centred vertically, ``center`` centred on both axes (``F.interpolate``'s
    ``bilinear`` at scale 2, rounded half up), ``topleft`` co-sited on both, ``top`` centred horizontally."""
    _chroma_check("bilinear", siting)
    if codes.dim() != 3 or codes.dtype != torch.int32:
        raise ValueError("chroma_upsample: int32 codes [B, ch, cw]")
    ch, cw = codes.shape[1:]
    if (ch, cw) != ((h + (1 << vs) - 1) >> vs, (w + (1 << hs) - 1) >> hs):
        raise ValueError(f"chroma_upsample: a {h}x{w} picture subsampled by (2^{hs}, 2^{vs}) has chroma "
                         f"{((h + (1 << vs) - 1) >> vs, (w + (1 << hs) - 1) >> hs)}, not {(ch, cw)}")
    bits = SITINGS[siting]
    y0, y1, wy0, wy1 = _chroma_axis(h, ch, vs, bool(bits & 2), codes.device)
    x0, x1, wx0, wx1 = _chroma_axis(w, cw, hs, bool(bits & 1), codes.device)
    # 16 x a 12-bit code is below 2^16: int32 cannot overflow
    rows = codes[:, y0] * wy0.to(torch.int32)[None, :, None] + codes[:, y1] * wy1.to(torch.int32)[None, :, None]
    both = rows[:, :, x0] * wx0.to(torch.int32) + rows[:, :, x1] * wx1.to(torch.int32)
    return (both + 8) >> 4


def yuv420_to_rgb(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, matrix: str = "bt601",
                  full_range: bool = False, chroma: str = "nearest", siting: str = "left") -> torch.Tensor:
    """A planar 4:2:0 frame as interleaved RGB, uint8 ``[B, h, w, 3]``: the definition of the conversion (and
    what runs on the CPU, with the ``torch`` backend and past the kernel's limits). Nearest chroma,
    exact int32 arithmetic on :func:`nv12_table`. ``chroma="bilinear"``: :func:`yuv_to_rgb`'s, at ``siting``."""
    y, u, v = yuv420_planes(y, u, v, any_strides=True)
    t = nv12_table(matrix, full_range)
    _chroma_check(chroma, siting)
    if chroma == "bilinear":
        return yuv_to_rgb(y, u, v, "420", 8, False, matrix, full_range, chroma, siting)
    h, w = y.shape[1:]
    rows, cols = torch.arange(h, device=y.device) >> 1, torch.arange(w, device=y.device) >> 1
    # the largest term is below 2^25 (138 438 x 128, 76 309 x 255) and the sum below 2^27: int32 cannot overflow
    yy = y.to(torch.int32) - t[9]
    uu = u.to(torch.int32)[:, rows][:, :, cols] - t[10]
    vv = v.to(torch.int32)[:, rows][:, :, cols] - t[11]
    out = [(t[3 * k] * yy + t[3 * k + 1] * uu + t[3 * k + 2] * vv + 32768) >> 16 for k in range(3)]
    return torch.stack(out, dim=-1).clamp_(0, 255).to(torch.uint8)


def nv12_to_rgb(y: torch.Tensor, uv: torch.Tensor, matrix: str = "bt601", full_range: bool = False,
                vu: bool = False, chroma: str = "nearest", siting: str = "left") -> torch.Tensor:
    """An NV12 frame as interleaved RGB, uint8 ``[B, h, w, 3]``: :func:`yuv420_to_rgb` of its de-interleaved
    planes (``vu``: the pairs are (V, U), NV21)."""
    y, uv = nv12_planes(y, uv)
    return yuv420_to_rgb(y, uv[..., 1 if vu else 0], uv[..., 0 if vu else 1], matrix, full_range, chroma, siting)


def _storage_bounds(t: torch.Tensor) -> Tuple[int, int]:
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + s.nbytes()


def nv12_patch_planes(y: torch.Tensor, uv: torch.Tensor, out_hw: Tuple[int, int], patch: int, mean: Sequence[float],
                      std: Sequence[float], matrix: str = "bt601", full_range: bool = False,
                      want_pixels: bool = False, vu: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """:func:`image_patch_planes` of an NV12 frame (:func:`nv12_planes`' layout), bit-equal to
    ``image_patch_planes(nv12_to_rgb(y, uv, matrix, full_range), ...)`` — which is what runs on a CPU
    tensor, with the ``torch`` backend and past the kernel's limits. On the GPU one HIP launch reads
    the two planes in place, by their strides: a pitched surface is not copied. ``vu``: the chroma pairs
    are (V, U), which is NV21."""
    y, uv = nv12_planes(y, uv)
    table = nv12_table(matrix, full_range)
    B, h, w = y.shape
    H, W = int(out_hw[0]), int(out_hw[1])
    tabs = _fused_tables(y, (h, w), (H, W), patch, NV12_MAX_FOOTPRINT)
    if tabs is None:
        rgb = nv12_to_rgb(y, uv, matrix, full_range, vu=True) if vu else nv12_to_rgb(y, uv, matrix, full_range)
        return image_patch_planes(rgb, (H, W), patch, mean, std, want_pixels)
    planes, pixels, gh, gw = _outputs(B, H, W, patch, want_pixels, y.device)
    args = (y.data_ptr(), *_storage_bounds(y), uv.data_ptr(), *_storage_bounds(uv), y.stride(1), uv.stride(1),
            y.stride(0), uv.stride(0), (ctypes.c_int * 12)(*table),
            *_tail_args(tabs, planes, pixels, mean, std, B, h, w, H, W, patch, gh, gw))
    rc = _L().nos_image_patch_planes_nv12_order(*args, 1) if vu else _L().nos_image_patch_planes_nv12(*args)
    _check(rc, "nv12_patch_planes")
    return planes, pixels


def _outputs(B: int, H: int, W: int, patch: int, want_pixels: bool, device: torch.device):
    gh, gw = H // patch, W // patch
    planes = torch.empty(3, B * gh * gw, 3 * patch * patch, dtype=torch.bfloat16, device=device)
    pixels = torch.empty(B, 3, H, W, dtype=torch.float32, device=device) if want_pixels else None
    return planes, pixels, gh, gw


def _tail_args(tabs: tuple, planes: torch.Tensor, pixels: Optional[torch.Tensor], mean, std, B, h, w, H, W, patch,
               gh, gw) -> tuple:
    """The arguments every image entry shares, from the output planes on."""
    yidx, ywt, xidx, xwt, max_fh, max_fw = tabs
    a, b = affine(mean, std)
    F3 = ctypes.c_float * 3
    return (planes.data_ptr(), pixels.data_ptr() if pixels is not None else None, yidx.data_ptr(), ywt.data_ptr(),
            xidx.data_ptr(), xwt.data_ptr(), ywt.shape[0], xwt.shape[0], ywt.shape[1], max_fh, max_fw, F3(*a), F3(*b),
            B, h, w, H, W, patch, gh, gw, image_wgs(), torch.cuda.current_stream().cuda_stream)


# ---- planar 4:2:0 -------------------------------------------------------------------------------
def yuv420p_patch_planes(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, out_hw: Tuple[int, int], patch: int,
                         mean: Sequence[float], std: Sequence[float], matrix: str = "bt601", full_range: bool = False,
                         want_pixels: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """:func:`image_patch_planes` of a planar 4:2:0 frame (:func:`yuv420_planes`' layout; I420, or YV12 with
    the planes passed by what they hold), bit-equal to ``image_patch_planes(yuv420_to_rgb(y, u, v, matrix,
    full_range), ...)`` — which is what runs on a CPU tensor, with the ``torch`` backend and past the kernel's
    limits. On the GPU one HIP launch reads the three planes in place, each by its own strides."""
    y, u, v = yuv420_planes(y, u, v)
    table = nv12_table(matrix, full_range)
    B, h, w = y.shape
    H, W = int(out_hw[0]), int(out_hw[1])
    tabs = _fused_tables(y, (h, w), (H, W), patch, YUV420P_MAX_FOOTPRINT)
    if tabs is None:
        return image_patch_planes(yuv420_to_rgb(y, u, v, matrix, full_range), (H, W), patch, mean, std, want_pixels)
    planes, pixels, gh, gw = _outputs(B, H, W, patch, want_pixels, y.device)
    rc = _L().nos_image_patch_planes_yuv420p(y.data_ptr(), *_storage_bounds(y), u.data_ptr(), *_storage_bounds(u),
                                             v.data_ptr(), *_storage_bounds(v), y.stride(1), u.stride(1), v.stride(1),
                                             y.stride(0), u.stride(0), v.stride(0), (ctypes.c_int * 12)(*table),
                                             *_tail_args(tabs, planes, pixels, mean, std, B, h, w, H, W, patch, gh, gw))
    _check(rc, "yuv420p_patch_planes")
    return planes, pixels


# ---- packed pixels ------------------------------------------------------------------------------
def _packed_strides(img: torch.Tensor) -> bool:
    """Whole pixels side by side in a row (rows and images wherever their strides put them)."""
    C = img.shape[3]
    return img.stride(3) == 1 and (img.shape[2] == 1 or img.stride(2) == C) \
        and (img.shape[1] == 1 or img.stride(1) >= img.shape[2] * C)


def packed_to_rgb(img: torch.Tensor, order: str = "rgb") -> torch.Tensor:
    """Packed pixels ``[B, h, w, 3 | 4]`` in ``order`` as contiguous interleaved RGB ``[B, h, w, 3]``: the colour
    bytes re-indexed, a fourth byte dropped (no premultiplication)."""
    if order not in PACKED_ORDERS:
        raise ValueError(f"packed: channel order {order!r} is none of {sorted(PACKED_ORDERS)}")
    C, idx = PACKED_ORDERS[order]
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != C:
        raise ValueError(f"packed: {order} takes a uint8 [B, h, w, {C}] image")
    # (slices stacked, not an index list: no index tensor is copied from the host, so it can be captured)
    return torch.stack([img[..., i] for i in idx], dim=-1)


def packed_patch_planes(img: torch.Tensor, order: str, out_hw: Tuple[int, int], patch: int, mean: Sequence[float],
                        std: Sequence[float], want_pixels: bool = False) \
        -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """:func:`image_patch_planes` of packed pixels ``[B, h, w, C]`` uint8 in ``order`` (``rgb``, ``bgr``: C = 3;
    ``rgba``, ``bgra``: C = 4, the fourth byte ignored), bit-equal to ``image_patch_planes(packed_to_rgb(img,
    order), ...)`` — which is what runs on a CPU tensor, with the ``torch`` backend and past the kernel's limits.
    ``stride(3) == 1`` and ``stride(2) == C``; rows and images lie wherever ``stride(1)`` and ``stride(0)`` put
    them (a crop, a padded capture buffer, a flipped batch), and on the GPU one HIP launch reads them there."""
    if order not in PACKED_ORDERS:
        raise ValueError(f"packed: channel order {order!r} is none of {sorted(PACKED_ORDERS)}")
    C = PACKED_ORDERS[order][0]
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != C \
            or 0 in img.shape:
        raise ValueError(f"packed: {order} takes a uint8 [B, h, w, {C}] image")
    if not _packed_strides(img):
        raise ValueError("packed: rows may be pitched, but the bytes of a row are contiguous "
                         f"(stride(3) == 1, stride(2) == {C}, stride(1) >= {C} * w)")
    B, h, w, _ = img.shape
    H, W = int(out_hw[0]), int(out_hw[1])
    tabs = _fused_tables(img, (h, w), (H, W), patch, PACKED_MAX_FOOTPRINT)
    if tabs is None:
        return image_patch_planes(packed_to_rgb(img, order), (H, W), patch, mean, std, want_pixels)
    planes, pixels, gh, gw = _outputs(B, H, W, patch, want_pixels, img.device)
    rc = _L().nos_image_patch_planes_packed(img.data_ptr(), *_storage_bounds(img), img.stride(1), img.stride(0),
                                            order.encode(),
                                            *_tail_args(tabs, planes, pixels, mean, std, B, h, w, H, W, patch, gh, gw))
    _check(rc, "packed_patch_planes")
    return planes, pixels


# ---- tiles of one frame ---------------------------------------------------------------------------
def _axis_plan(n: int, k: int, overlap: float) -> Tuple[int, list]:
    if k == 1:
        return n, [0]
    t = min(n, int(math.ceil(n / (k - (k - 1) * overlap))))
    return t, [(2 * i * (n - t) + (k - 1)) // (2 * (k - 1)) for i in range(k)]


def tile_plan(h: int, w: int, tiles: Tuple[int, int] = (2, 2), overlap: float = 0.2,
              num_detection_tokens: int = 100) -> Tuple[int, int, list]:
    """``(th, tw, origins)``: an ``h x w`` frame cut into ``tiles = (R, C)`` tiles of one size that overlap their
    neighbours by about ``overlap`` of a tile; ``origins`` is the row-major list of ``(y0, x0)``, ``R * C`` long. Per
    axis of length ``n`` cut into ``k``: ``k == 1`` is the axis itself; otherwise ``t = min(n, ceil(n / (k - (k - 1)
    overlap)))`` and ``origin_i = i (n - t) / (k - 1)`` rounded half up, so the first tile starts at 0, the last ends
    at ``n`` and consecutive tiles touch or overlap. ``R * C * num_detection_tokens`` rows must fit
    :func:`merge_detections` (:data:`MAX_ROWS`)."""
    R, C = int(tiles[0]), int(tiles[1])
    if not 0.0 <= overlap < 1.0:
        raise ValueError(f"tile_plan: overlap {overlap!r} is not in [0, 1)")
    if R < 1 or C < 1:
        raise ValueError(f"tile_plan: at least one tile per axis, not {(R, C)}")
    if R * C * int(num_detection_tokens) > MAX_ROWS:
        raise ValueError(f"tile_plan: {R} x {C} tiles of {num_detection_tokens} detection tokens are more than "
                         f"{MAX_ROWS} rows")
    if h < 1 or w < 1:
        raise ValueError("tile_plan: a frame of at least one pixel")
    th, ys = _axis_plan(int(h), R, float(overlap))
    tw, xs = _axis_plan(int(w), C, float(overlap))
    return th, tw, [(y, x) for y in ys for x in xs]


def _tile_origins(origins, th: int, tw: int, h: int, w: int, who: str) -> Tuple[Tuple[int, int], ...]:
    out = tuple((int(y), int(x)) for y, x in origins)
    if not out:
        raise ValueError(f"{who}: at least one tile")
    if th < 1 or tw < 1 or any(y < 0 or x < 0 or y + th > h or x + tw > w for y, x in out):
        raise ValueError(f"{who}: every {th}x{tw} tile lies inside the {h}x{w} frame")
    return out


def tile_crops(img: torch.Tensor, origins, tile_hw: Tuple[int, int]) -> torch.Tensor:
    """The tiles of ``img`` ``[1, h, w, C]`` stacked: contiguous ``[B, th, tw, C]`` (slices stacked: nothing is copied
    from the host, so it can be captured)."""
    th, tw = int(tile_hw[0]), int(tile_hw[1])
    return torch.stack([img[0, y:y + th, x:x + tw] for y, x in origins])


def origin_tensor(origins, device: torch.device) -> torch.Tensor:
    """``[B, 2]`` int32 ``(y0, x0)`` on ``device``, cached beside the tap tables (a captured graph holds it); a tensor
    already there is used as it is."""
    if isinstance(origins, torch.Tensor):
        return origins.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    key = ("origins", tuple((int(y), int(x)) for y, x in origins), str(device))
    return _tables.get(key, lambda: torch.tensor(key[1], dtype=torch.int32).reshape(-1, 2).to(device))


def tiled_patch_planes(img: torch.Tensor, order: str, origins, tile_hw: Tuple[int, int], out_hw: Tuple[int, int],
                       patch: int, mean: Sequence[float], std: Sequence[float], want_pixels: bool = False) \
        -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """:func:`packed_patch_planes` of ``B`` tiles of one frame without stacking them: ``img`` uint8 ``[h, w, C]`` or
    ``[1, h, w, C]`` packed pixels in ``order`` (any row pitch, a crop view: :func:`packed_patch_planes`' contract),
    ``origins`` the ``(y0, x0)`` of the tiles, each ``tile_hw`` large and resized to ``out_hw`` -> ``(planes [3,
    B*gh*gw, 3*p*p], pixels [B, 3, H, W] or None)``, bit-equal to ``packed_patch_planes(tile_crops(img, origins,
    tile_hw), order, ...)`` — which is what runs on a CPU tensor, with the ``torch`` backend and past the kernel's
    limits. On the GPU one HIP launch reads every tile in place: tile ``b`` starts at a byte offset the kernel reads
    from a device table (built here, cached beside the tap tables, dropped by :func:`invalidate_cache`)."""
    if order not in PACKED_ORDERS:
        raise ValueError(f"tiled: channel order {order!r} is none of {sorted(PACKED_ORDERS)}")
    C = PACKED_ORDERS[order][0]
    if isinstance(img, torch.Tensor) and img.dim() == 3:
        img = img[None]
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[0] != 1 \
            or img.shape[3] != C or 0 in img.shape:
        raise ValueError(f"tiled: {order} takes one uint8 [h, w, {C}] (or [1, h, w, {C}]) frame")
    if not _packed_strides(img):
        raise ValueError("tiled: rows may be pitched, but the bytes of a row are contiguous "
                         f"(stride(3) == 1, stride(2) == {C}, stride(1) >= {C} * w)")
    _, h, w, _ = img.shape
    th, tw = int(tile_hw[0]), int(tile_hw[1])
    origins = _tile_origins(origins, th, tw, h, w, "tiled")
    B = len(origins)
    H, W = int(out_hw[0]), int(out_hw[1])
    tabs = _fused_tables(img, (th, tw), (H, W), patch, PACKED_MAX_FOOTPRINT)
    if tabs is None:
        return packed_patch_planes(tile_crops(img, origins, (th, tw)), order, (H, W), patch, mean, std, want_pixels)
    pitch = img.stride(1) if h > 1 else w * C
    table = _tables.get(("tiles", origins, pitch, C, str(img.device)),
                        lambda: torch.tensor([y * pitch + x * C for y, x in origins], dtype=torch.int64).to(img.device))
    planes, pixels, gh, gw = _outputs(B, H, W, patch, want_pixels, img.device)
    flat = (ctypes.c_int * (2 * B))(*[v for o in origins for v in o])
    rc = _L().nos_image_patch_planes_tiles(img.data_ptr(), *_storage_bounds(img), pitch, order.encode(), flat,
                                           table.data_ptr(), h, w,
                                           *_tail_args(tabs, planes, pixels, mean, std, B, th, tw, H, W, patch, gh, gw))
    _check(rc, "tiled_patch_planes")
    return planes, pixels


# ---- 4:2:2, 4:4:4, packed 4:2:2 and 10 / 12-bit samples -------------------------------------------
#: :data:`NV12_MATRICES` and BT.2020 in its non-constant-luminance form (what 10-bit content usually carries)
YUV_MATRICES = {**NV12_MATRICES, "bt2020": (0.2627, 0.0593)}
YUV_DEPTHS = (8, 10, 12)
#: log2 of the chroma subsampling ``(horizontal, vertical)``
YUV_SUBSAMPLING = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
#: packed 4:2:2: the byte of the first luma, of U and of V in a four-byte macropixel (the second luma two on)
YUYV_ORDERS = {"yuyv": (0, 1, 3), "uyvy": (1, 0, 2), "yvyu": (0, 3, 1)}


def _yuv_check(matrix: str, depth: int) -> None:
    if matrix not in YUV_MATRICES:
        raise ValueError(f"yuv: matrix {matrix!r} is none of {sorted(YUV_MATRICES)}")
    if depth not in YUV_DEPTHS:
        raise ValueError(f"yuv: depth {depth!r} is none of {YUV_DEPTHS}")


def yuv_real_matrix(matrix: str = "bt601", full_range: bool = False, depth: int = 8) \
        -> Tuple[np.ndarray, Tuple[int, int, int]]:
    """:func:`nv12_real_matrix` for codes of ``depth`` bits, to 8-bit RGB: ``(M [3, 3], offsets)`` with ``rgb = M @
    ((Y, U, V) - offsets)``. Limited range takes ``16 * 2^(depth-8)`` from Y and scales Y by ``255 / (219 *
    2^(depth-8))`` and chroma by ``255 / (224 * 2^(depth-8))``; full range scales both by ``255 / (2^depth - 1)``;
    both take ``2^(depth-1)`` from chroma."""
    _yuv_check(matrix, depth)
    kr, kb = YUV_MATRICES[matrix]
    kg = 1.0 - kr - kb
    up = float(1 << (depth - 8))
    sy, sc = (255.0 / ((1 << depth) - 1),) * 2 if full_range else (255.0 / (219.0 * up), 255.0 / (224.0 * up))
    m = np.array([[sy, 0.0, sc * 2.0 * (1.0 - kr)],
                  [sy, -sc * 2.0 * kb * (1.0 - kb) / kg, -sc * 2.0 * kr * (1.0 - kr) / kg],
                  [sy, sc * 2.0 * (1.0 - kb), 0.0]], dtype=np.float64)
    return m, (0 if full_range else 16 << (depth - 8), 1 << (depth - 1), 1 << (depth - 1))


def yuv_table(matrix: str = "bt601", full_range: bool = False, depth: int = 8) -> Tuple[int, ...]:
    """The 12 integers :func:`yuv_to_rgb` and the kernel compute with: ``rint(M * 2^(8 + depth))`` of
    :func:`yuv_real_matrix` by rows (R, G, B) x (Y, U, V), then the three offsets. Channel ``c`` is ``clip((t[3c]
    (Y - t[9]) + t[3c+1] (U - t[10]) + t[3c+2] (V - t[11]) + 2^(7+depth)) >> (8+depth), 0, 255)``. At depth 8 it
    is :func:`nv12_table`; in limited range the coefficients are the same integers at every depth. Every
    coefficient is at most 140 363 (24-bit multiplies) and every sum below 5.81e8 in size (int32)."""
    m, off = yuv_real_matrix(matrix, full_range, depth)
    return tuple(int(v) for v in np.rint(m * float(1 << (8 + depth))).astype(np.int64).reshape(-1)) + tuple(off)


def _sample_depth(t: torch.Tensor, depth: int, who: str) -> None:
    if depth not in YUV_DEPTHS:
        raise ValueError(f"{who}: depth {depth!r} is none of {YUV_DEPTHS}")
    want = (torch.uint8,) if depth == 8 else (torch.uint16, torch.int16)
    if not isinstance(t, torch.Tensor) or t.dtype not in want:
        raise ValueError(f"{who}: depth {depth} takes " + ("uint8 planes" if depth == 8 else
                                                            "uint16 (or int16) planes of little-endian words"))


def yuv_codes(plane: torch.Tensor, depth: int = 8, msb: bool = False) -> torch.Tensor:
    """A plane's sample codes as int32. uint8 (depth 8): its values. A 16-bit plane (``torch.uint16``, or
    ``torch.int16`` read as the same bits) of depth 10 or 12: ``(word >> (16 - depth)) & (2^depth - 1)`` with
    ``msb`` (P010's layout), ``word & (2^depth - 1)`` without (``yuv420p10le``'s). The other bits are ignored."""
    _sample_depth(plane, depth, "yuv_codes")
    if depth == 8:
        return plane.to(torch.int32)
    # (no shifts on uint16, and few other ops on the GPU: the same bits as int16, widened, the sign bits cut)
    word = (plane if plane.dtype == torch.int16 else plane.view(torch.int16)).to(torch.int32) & 0xffff
    return ((word >> (16 - depth)) if msb else word) & ((1 << depth) - 1)


def yuv_planes(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, subsampling: str = "420", depth: int = 8,
               any_strides: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The three planes of a planar frame as ``[B, h, w]`` and two ``[B, ch, cw]`` views, checked: ``subsampling``
    ``"420"`` has chroma ``[(h+1)//2, (w+1)//2]``, ``"422"`` ``[h, (w+1)//2]``, ``"444"`` ``[h, w]``; the dtype
    goes with ``depth`` (:func:`yuv_codes`); one device; rows possibly pitched but contiguous inside
    (``any_strides``: not even that, for the torch definition)."""
    if subsampling not in YUV_SUBSAMPLING:
        raise ValueError(f"yuv: subsampling {subsampling!r} is none of {sorted(YUV_SUBSAMPLING)}")
    for t in (y, u, v):
        _sample_depth(t, depth, "yuv")
    if u.dtype != y.dtype or v.dtype != y.dtype:
        raise ValueError("yuv: the three planes have one dtype")
    if y.dim() == 2 and u.dim() == 2 and v.dim() == 2:
        y, u, v = y[None], u[None], v[None]
    if y.dim() != 3 or u.dim() != 3 or v.dim() != 3 or 0 in y.shape:
        raise ValueError("yuv: Y is [B, h, w] (or [h, w]) and U, V [B, ch, cw] (or without B)")
    hs, vs = YUV_SUBSAMPLING[subsampling]
    B, h, w = y.shape
    want = (B, (h + (1 << vs) - 1) >> vs, (w + (1 << hs) - 1) >> hs)
    if tuple(u.shape) != want or tuple(v.shape) != want:
        raise ValueError(f"yuv: a {h}x{w} Y plane takes 4:{subsampling[1:2]}:{subsampling[2:]} U and V planes of "
                         f"shape {want}, not {tuple(u.shape)} and {tuple(v.shape)}")
    if y.device != u.device or y.device != v.device:
        raise ValueError(f"yuv: all planes on one device, not {y.device}, {u.device} and {v.device}")
    if not any_strides and any(t.shape[2] > 1 and t.stride(2) != 1 for t in (y, u, v)):
        raise ValueError("yuv: rows may be pitched, but the samples of a row are contiguous")
    return y, u, v


# ---- PQ and HLG frames, tone-mapped to SDR ----------------------------------------------------------
#: how a frame's R'G'B' codes are read: ``sdr`` — cut to 8 bits, as they are — or an HDR transfer function of a 10 /
#: 12-bit frame, ``pq`` (SMPTE ST 2084, HDR10) or ``hlg`` (BT.2100), tone-mapped to sRGB bytes (:func:`hdr_tables`)
TRANSFERS = ("sdr", "pq", "hlg")
#: linear light in ``lut1`` and behind the gamut matrix: SDR white; ``lut2`` has one entry more
HDR_WHITE = 16383
#: BT.2408's reference white in nits: what SDR white is mapped from
HDR_REFERENCE_WHITE = 203.0
#: the gamut matrix is in 2^-12 fixed point
HDR_GAMUT_ONE = 4096
#: CIE xy of the red, green and blue primaries; both sets have D65 as white
_PRIMARIES = {"bt709": ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060)),
              "bt2020": ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046))}
_D65 = (0.3127, 0.3290)


def _transfer_check(transfer: str, peak_nits: float, depth: int) -> None:
    if transfer not in TRANSFERS:
        raise ValueError(f"yuv: transfer {transfer!r} is none of {TRANSFERS}")
    if not float(peak_nits) > HDR_REFERENCE_WHITE:
        raise ValueError(f"yuv: peak_nits {peak_nits!r} must exceed the reference white, {HDR_REFERENCE_WHITE:g} nits")
    if transfer != "sdr" and depth not in (10, 12):
        raise ValueError(f"yuv: transfer {transfer!r} takes a frame of depth 10 or 12, not {depth!r} "
                         "(8-bit and packed sources are read as sdr)")


def _rgb_to_xyz(primaries: str) -> np.ndarray:
    """Linear RGB of a set of primaries to CIE XYZ, white D65 at Y = 1, in fp64."""
    m = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in _PRIMARIES[primaries]], dtype=np.float64).T
    white = np.array([_D65[0] / _D65[1], 1.0, (1.0 - _D65[0] - _D65[1]) / _D65[1]], dtype=np.float64)
    return m * np.linalg.solve(m, white)[None, :]


def hdr_gamut(matrix: str) -> np.ndarray:
    """The gamut step of :func:`hdr_to_sdr` as int32 ``[3, 3]`` in 2^-12 fixed point: BT.2020 to BT.709 primaries
    in linear light for ``matrix == "bt2020"`` — derived in fp64 from the two sets of primaries and D65, rounded —
    else ``4096 I`` (a BT.601 / BT.709 stream is taken to be in BT.709 primaries). Every row sums to 4096."""
    if matrix not in YUV_MATRICES:
        raise ValueError(f"yuv: matrix {matrix!r} is none of {sorted(YUV_MATRICES)}")
    if matrix != "bt2020":
        return np.eye(3, dtype=np.int32) * HDR_GAMUT_ONE
    m = np.linalg.solve(_rgb_to_xyz("bt709"), _rgb_to_xyz("bt2020"))
    return np.rint(m * HDR_GAMUT_ONE).astype(np.int32)


def hdr_nits(transfer: str, e: np.ndarray) -> np.ndarray:
    """Display light in nits of the non-linear signal ``e`` in 0..1, fp64. ``pq``: the ST 2084 EOTF. ``hlg``: BT.2100's
    inverse OETF and the OOTF per component, gamma 1.2, for a 1000-nit display."""
    e = np.asarray(e, dtype=np.float64)
    if transfer == "pq":
        m1, m2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
        c1, c2, c3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
        p = e ** (1.0 / m2)
        return 10000.0 * (np.maximum(p - c1, 0.0) / (c2 - c3 * p)) ** (1.0 / m1)
    if transfer == "hlg":
        a = 0.17883277
        b, c = 1.0 - 4.0 * a, 0.5 - a * np.log(4.0 * a)
        scene = np.where(e <= 0.5, e * e / 3.0, (np.exp((e - c) / a) + b) / 12.0)
        return 1000.0 * scene ** 1.2
    raise ValueError(f"yuv: transfer {transfer!r} has no light of its own (one of {TRANSFERS[1:]})")


def hdr_tone_map(nits: np.ndarray, peak_nits: float = 1000.0) -> np.ndarray:
    """The extended Reinhard curve on nits, fp64: ``x = N / 203``, ``p = peak_nits / 203``, ``clip(x (1 + x / p^2) /
    (1 + x), 0, 1)`` — 1 is SDR white, reached at ``peak_nits``."""
    x, p = np.asarray(nits, dtype=np.float64) / HDR_REFERENCE_WHITE, float(peak_nits) / HDR_REFERENCE_WHITE
    return np.clip(x * (1.0 + x / (p * p)) / (1.0 + x), 0.0, 1.0)


_hdr_host: dict = {}


def hdr_tables(transfer: str, depth: int, matrix: str, peak_nits: float = 1000.0) \
        -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(lut1, gamut, lut2)``: everything :func:`hdr_to_sdr` and the kernel know of an HDR transfer, built in fp64.

    * ``lut1`` uint16 ``[2^depth]``: code ``k`` of an R'G'B' channel at the source's depth stands for ``E' = min(k /
      (255 * 2^(depth-8)), 1)``; ``lut1[k] = rint(16383 T(N(E')))`` is its tone-mapped linear light, 16383 = SDR
      white (:func:`hdr_nits`, :func:`hdr_tone_map`).
    * ``gamut`` int32 ``[3, 3]``: :func:`hdr_gamut`.
    * ``lut2`` uint8 ``[16384]``: ``rint(255 sRGB_OETF(s / 16383))`` by IEC 61966-2-1.

    Tone mapping is per channel, in the source's primaries, before the gamut step. The arrays are shared and
    read-only."""
    _transfer_check(transfer, peak_nits, depth)
    if transfer == "sdr":
        raise ValueError("yuv: transfer 'sdr' has no tables (the codes are cut to 8 bits as they are)")
    key = (transfer, int(depth), matrix, float(peak_nits))
    hit = _hdr_host.get(key)
    if hit is None:
        gamut = hdr_gamut(matrix)
        e = np.minimum(np.arange(1 << depth, dtype=np.float64) / (255.0 * (1 << (depth - 8))), 1.0)
        lut1 = np.rint(HDR_WHITE * hdr_tone_map(hdr_nits(transfer, e), peak_nits)).astype(np.uint16)
        lin = np.arange(HDR_WHITE + 1, dtype=np.float64) / HDR_WHITE
        srgb = np.where(lin < 0.0031308, 12.92 * lin, 1.055 * lin ** (1.0 / 2.4) - 0.055)
        lut2 = np.rint(255.0 * srgb).astype(np.uint8)
        for t in (lut1, gamut, lut2):
            t.setflags(write=False)
        if len(_hdr_host) >= 16:
            _hdr_host.pop(next(iter(_hdr_host)))
        hit = _hdr_host[key] = (lut1, gamut, lut2)
    return hit


def _hdr_lut(t, device: torch.device) -> torch.Tensor:
    """A table as a tensor on ``device`` (an ndarray is widened to int32 first: no uint16 arithmetic in torch)."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t.astype(np.int32))
    return t.to(device)


def hdr_to_sdr(codes: torch.Tensor, tables: Sequence) -> torch.Tensor:
    """Steps 2 to 4 of the HDR conversion on int32 R'G'B' codes ``[..., 3]`` of the source's depth, in exact
    integers: ``l_j = lut1[k_j]``, ``s_c = clip((sum_j gamut[c][j] l_j + 2048) >> 12, 0, 16383)``, ``lut2[s_c]`` —
    uint8 sRGB ``[..., 3]``. ``tables``: :func:`hdr_tables`' result (the tables as ndarrays, or as integer tensors on
    the codes' device, the gamut's nine integers by rows or flat). Operands fit 24-bit multiplies (below 2^15 and 2^14) and the sums stay below 2^29."""
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.int32 or codes.dim() < 1 or codes.shape[-1] != 3:
        raise ValueError("hdr_to_sdr: int32 codes [..., 3]")
    lut1, gamut, lut2 = tables
    lut1, lut2 = _hdr_lut(lut1, codes.device), _hdr_lut(lut2, codes.device)
    g = np.asarray(gamut, dtype=np.int64).reshape(3, 3).tolist()    # nine integers, by rows or flat
    light = lut1[codes.clamp(0, lut1.numel() - 1).long()].to(torch.int32)
    out = [((g[c][0] * light[..., 0] + g[c][1] * light[..., 1] + g[c][2] * light[..., 2] + HDR_GAMUT_ONE // 2) >> 12)
           .clamp_(0, HDR_WHITE) for c in range(3)]
    return lut2[torch.stack(out, dim=-1).long()].to(torch.uint8)


#: the device copies of the HDR tables per ``(transfer, depth, matrix, peak_nits, device)``: as the tap tables, a
#: launch recorded in a graph reads them by address, so an entry handed out under capture stays until
#: :func:`invalidate_cache` (34 to 40 KB each)
_hdr_tables = GraphCache(8)


def _make_hdr_tables(transfer: str, depth: int, matrix: str, peak_nits: float, device: torch.device) -> tuple:
    lut1, gamut, lut2 = hdr_tables(transfer, depth, matrix, peak_nits)
    # (16383 fits int16, which torch handles everywhere: the same bits the kernel reads as uint16)
    return (torch.from_numpy(lut1.astype(np.int16)).to(device), tuple(int(c) for c in gamut.reshape(-1)),
            torch.from_numpy(lut2.copy()).to(device))


def _hdr_device_tables(transfer: str, depth: int, matrix: str, peak_nits: float, device: torch.device) -> tuple:
    """``(lut1 int16 [2^depth], gamut (9 integers), lut2 uint8 [16384])`` with the tables on ``device``, cached
    (:data:`_hdr_tables`)."""
    key = (transfer, int(depth), matrix, float(peak_nits), str(device))
    return _hdr_tables.get(key, lambda: _make_hdr_tables(transfer, depth, matrix, peak_nits, device))


def yuv_to_rgb(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, subsampling: str = "420", depth: int = 8,
               msb: bool = False, matrix: str = "bt601", full_range: bool = False, chroma: str = "nearest",
               siting: str = "left", transfer: str = "sdr", peak_nits: float = 1000.0) -> torch.Tensor:
    """A planar frame of any of the three chroma geometries and sample depths as interleaved RGB, uint8 ``[B, h,
    w, 3]``: the definition of the conversion (and what runs on the CPU, with the ``torch`` backend and past the
    kernel's limits). Nearest chroma — luma ``(r, c)`` takes chroma ``(r >> vs, c >> hs)`` — and exact int32
    arithmetic on :func:`yuv_table`. For ``"420"`` at depth 8 it equals :func:`yuv420_to_rgb`. With
    ``chroma="bilinear"`` the chroma codes are :func:`chroma_upsample`'s at ``siting`` instead (codes of the same
    depth, so the table arithmetic is the same and as far from overflow); on ``"444"`` that is nearest.

    ``transfer="pq"`` or ``"hlg"`` (depth 10 or 12): the colour matrix's sums are not cut to 8 bits but to codes of
    the source's depth, ``k_c = clip(sum + 2^15, 0, 2^(16+depth) - 1) >> 16`` — the 8-bit value times ``2^(depth-8)``
    — which go through :func:`hdr_to_sdr` on :func:`hdr_tables` ``(transfer, depth, matrix, peak_nits)``."""
    y, u, v = yuv_planes(y, u, v, subsampling, depth, any_strides=True)
    t = yuv_table(matrix, full_range, depth)
    _chroma_check(chroma, siting)
    _transfer_check(transfer, peak_nits, depth)
    hs, vs = YUV_SUBSAMPLING[subsampling]
    h, w = y.shape[1:]
    rows, cols = torch.arange(h, device=y.device) >> vs, torch.arange(w, device=y.device) >> hs
    # the largest sum is below 5.81e8 at depth 12: int32 cannot overflow
    yy = yuv_codes(y, depth, msb) - t[9]
    if chroma == "bilinear" and hs:
        uu = chroma_upsample(yuv_codes(u, depth, msb), h, w, hs, vs, siting) - t[10]
        vv = chroma_upsample(yuv_codes(v, depth, msb), h, w, hs, vs, siting) - t[11]
    else:
        uu = yuv_codes(u, depth, msb)[:, rows][:, :, cols] - t[10]
        vv = yuv_codes(v, depth, msb)[:, rows][:, :, cols] - t[11]
    if transfer != "sdr":
        # the same sums plus 2^15: still below 5.82e8
        codes = [(t[3 * k] * yy + t[3 * k + 1] * uu + t[3 * k + 2] * vv + 32768).clamp_(0, (1 << (16 + depth)) - 1) >> 16
                 for k in range(3)]
        tables = _hdr_device_tables(transfer, depth, matrix, peak_nits, y.device) if y.is_cuda else \
            hdr_tables(transfer, depth, matrix, peak_nits)
        return hdr_to_sdr(torch.stack(codes, dim=-1), tables)
    out = [(t[3 * k] * yy + t[3 * k + 1] * uu + t[3 * k + 2] * vv + (1 << (7 + depth))) >> (8 + depth)
           for k in range(3)]
    return torch.stack(out, dim=-1).clamp_(0, 255).to(torch.uint8)


def yuv_semiplanar_planes(y: torch.Tensor, uv: torch.Tensor, subsampling: str = "420", depth: int = 8) \
        -> Tuple[torch.Tensor, torch.Tensor]:
    """The two planes of a semi-planar frame (NV16, NV24, P010, P210 ...) as ``[B, h, w]`` and ``[B, ch, cw, 2]``
    views, checked as :func:`yuv_planes` checks; a chroma pair's two samples are adjacent."""
    if not isinstance(uv, torch.Tensor) or uv.dim() not in (3, 4) or uv.shape[-1] != 2:
        raise ValueError("yuv: the chroma plane of a semi-planar frame is [B, ch, cw, 2] (or without B)")
    y, u, v = yuv_planes(y, uv[..., 0], uv[..., 1], subsampling, depth, any_strides=True)
    uv = uv if uv.dim() == 4 else uv[None]
    if (y.shape[2] > 1 and y.stride(2) != 1) or uv.stride(3) != 1 or (uv.shape[2] > 1 and uv.stride(2) != 2):
        raise ValueError("yuv: rows may be pitched, but the samples of a row are contiguous (chroma interleaved)")
    return y, uv


def yuyv_planes(data: torch.Tensor, width: int, order: str = "yuyv") \
        -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The luma and the two chroma planes of packed 4:2:2 as strided views ``[B, h, width]`` and two ``[B, h,
    (width+1)//2]``. ``data``: uint8 ``[B, h, rowbytes]`` (or ``[h, rowbytes]``) with ``rowbytes >= 4 *
    ceil(width / 2)``, contiguous inside a row; a macropixel is four bytes, ``yuyv`` (YUY2: Y0 U Y1 V), ``uyvy``
    (U Y0 V Y1) or ``yvyu``. With an odd ``width`` the last macropixel's second luma is padding, never shown."""
    if order not in YUYV_ORDERS:
        raise ValueError(f"yuyv: order {order!r} is none of {sorted(YUYV_ORDERS)}")
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() not in (2, 3) or 0 in data.shape:
        raise ValueError("yuyv: a uint8 [B, h, rowbytes] (or [h, rowbytes]) tensor")
    data = data if data.dim() == 3 else data[None]
    width = int(width)
    cw = (width + 1) // 2
    if width <= 0 or data.shape[2] < 4 * cw:
        raise ValueError(f"yuyv: a row of {width} pixels takes {4 * cw} bytes, the rows have {data.shape[2]}")
    if data.stride(2) != 1:
        raise ValueError("yuyv: rows may be pitched, but the bytes of a row are contiguous")
    yo, uo, vo = YUYV_ORDERS[order]
    return data[..., yo::2][..., :width], data[..., uo::4][..., :cw], data[..., vo::4][..., :cw]


def yuyv_to_rgb(data: torch.Tensor, width: int, order: str = "yuyv", matrix: str = "bt601",
                full_range: bool = False, chroma: str = "nearest", siting: str = "left") -> torch.Tensor:
    """Packed 4:2:2 as interleaved RGB, uint8 ``[B, h, width, 3]``: :func:`yuv_to_rgb` of :func:`yuyv_planes`'
    three views as ``"422"``."""
    return yuv_to_rgb(*yuyv_planes(data, width, order), "422", 8, False, matrix, full_range, chroma, siting)


def yuv_semiplanar_to_rgb(y: torch.Tensor, uv: torch.Tensor, subsampling: str = "420", depth: int = 8,
                          msb: bool = False, matrix: str = "bt601", full_range: bool = False,
                          vu: bool = False, chroma: str = "nearest", siting: str = "left", transfer: str = "sdr",
                          peak_nits: float = 1000.0) -> torch.Tensor:
    """A semi-planar frame as interleaved RGB: :func:`yuv_to_rgb` of its de-interleaved planes (``vu``: the pairs
    are (V, U))."""
    y, uv = yuv_semiplanar_planes(y, uv, subsampling, depth)
    return yuv_to_rgb(y, uv[..., 1 if vu else 0], uv[..., 0 if vu else 1], subsampling, depth, msb, matrix, full_range,
                      chroma, siting, transfer, peak_nits)


class NosYuvPlane(ctypes.Structure):
    """One plane of :class:`NosYuvSrc` (``csrc/image_yuv.h``, field for field)."""
    _fields_ = [("p", ctypes.c_void_p), ("lo", ctypes.c_void_p), ("hi", ctypes.c_void_p),
                ("pitch", ctypes.c_longlong), ("bstride", ctypes.c_longlong)]


class NosYuvSrc(ctypes.Structure):
    """The general YUV entry's source descriptor (``csrc/image_yuv.h``, field for field)."""
    _fields_ = [("size", ctypes.c_int), ("layout", ctypes.c_int), ("hsub", ctypes.c_int), ("vsub", ctypes.c_int),
                ("sample_bytes", ctypes.c_int), ("depth", ctypes.c_int), ("shift", ctypes.c_int),
                ("order", ctypes.c_int), ("plane", NosYuvPlane * 3), ("tab", ctypes.c_int * 12),
                ("chroma", ctypes.c_int), ("siting", ctypes.c_int)]


class NosYuvHdr(ctypes.Structure):
    """The HDR entry's tables (``csrc/image_yuv.h``, field for field): device pointers to ``lut1`` (uint16 ``[entries]``)
    and ``lut2`` (uint8 ``[16384]``), and the gamut matrix by rows."""
    _fields_ = [("size", ctypes.c_int), ("entries", ctypes.c_int), ("lut1", ctypes.c_void_p),
                ("lut2", ctypes.c_void_p), ("gamut", ctypes.c_int * 9)]


YUV_PLANAR, YUV_SEMIPLANAR, YUV_PACKED = 0, 1, 2


def yuv_src(layout: int, planes: Sequence[torch.Tensor], subsampling: str, depth: int, msb: bool, order: int,
            table: Sequence[int], chroma: str = "nearest", siting: str = "left") -> NosYuvSrc:
    """The descriptor of ``planes`` — views ``[B, rows, row elements]`` of uint8 or 16-bit samples, each read by
    its own strides inside its own storage. Bilinear chroma of a 4:4:4 source is nearest, and is described so."""
    _chroma_check(chroma, siting)
    hs, vs = YUV_SUBSAMPLING[subsampling]
    bilinear = chroma == "bilinear" and hs != 0
    src = NosYuvSrc(size=ctypes.sizeof(NosYuvSrc), layout=layout, hsub=hs, vsub=vs, sample_bytes=1 if depth == 8 else 2,
                    depth=depth, shift=16 - depth if (msb and depth != 8) else 0, order=order,
                    chroma=int(bilinear), siting=SITINGS[siting] if bilinear else 0)
    for i, t in enumerate(planes):
        lo, hi = _storage_bounds(t)
        es = t.element_size()
        # (a single row's stride says nothing: its pitch is the row itself)
        src.plane[i] = NosYuvPlane(t.data_ptr(), lo, hi, (t.stride(1) if t.shape[1] > 1 else t.shape[2]) * es,
                                   t.stride(0) * es)
    for i, c in enumerate(table):
        src.tab[i] = c
    return src


def yuv_hdr(lut1: torch.Tensor, gamut: Sequence[int], lut2: torch.Tensor) -> NosYuvHdr:
    """The descriptor of HDR tables on the device (:func:`_hdr_device_tables`' three)."""
    return NosYuvHdr(size=ctypes.sizeof(NosYuvHdr), entries=lut1.numel(), lut1=lut1.data_ptr(), lut2=lut2.data_ptr(),
                     gamut=(ctypes.c_int * 9)(*gamut))


def _yuv_launch(src: NosYuvSrc, tabs: tuple, B: int, h: int, w: int, H: int, W: int, patch: int, mean, std,
                want_pixels: bool, device: torch.device, what: str, hdr: Optional[tuple] = None,
                origins: Optional[tuple] = None, frame_hw: Optional[Tuple[int, int]] = None):
    """One launch of the general YUV front end: on the ``B`` images of ``h x w`` that ``src`` describes or, with
    ``origins``, on the ``B = len(origins)`` tiles of ``h x w`` of the one ``frame_hw`` frame it describes (the device
    table is :func:`origin_tensor`'s, the one :func:`merge_detections` reads). ``hdr``: ``(transfer, depth, matrix,
    peak_nits)`` of a frame that is not ``sdr``; its launch reads the cached device tables."""
    planes, pixels, gh, gw = _outputs(B, H, W, patch, want_pixels, device)
    tail = _tail_args(tabs, planes, pixels, mean, std, B, h, w, H, W, patch, gh, gw)
    tables = None if hdr is None else ctypes.byref(yuv_hdr(*_hdr_device_tables(*hdr, device)))
    if origins is not None:
        flat = (ctypes.c_int * (2 * B))(*[v for o in origins for v in o])
        rc = _L().nos_image_patch_planes_yuv_tiles(ctypes.byref(src), tables, flat,
                                                   origin_tensor(origins, device).data_ptr(), frame_hw[0], frame_hw[1],
                                                   1, *tail)
    elif hdr is None:
        rc = _L().nos_image_patch_planes_yuv(ctypes.byref(src), *tail)
    else:
        rc = _L().nos_image_patch_planes_yuv_hdr(ctypes.byref(src), tables, *tail)
    _check(rc, what)
    return planes, pixels


def _yuv_patch_planes(source: tuple, name: str, out_hw: Tuple[int, int], patch: int, mean, std, want_pixels: bool,
                      tiles: Optional[tuple] = None):
    """What the six YUV functions do behind their layout's checks. ``source``: what the layout's ``_*_source`` gives —
    ``(first, (h, w), src, rgb, hdr)``, the tensor that says batch and device, the frame's size, the launch
    descriptor, a callable that gives the converted RGB frame, and :func:`_yuv_launch`'s ``hdr``. The plan, then one
    launch — or, on a CPU tensor, with the ``torch`` backend and past the kernel's limits, :func:`image_patch_planes`
    of the converted frame. With ``tiles = (origins, tile_hw)`` the images are those tiles of the one frame
    (:func:`tile_crops` of the converted frame in the composition)."""
    first, (h, w), src, rgb, hdr = source
    B, th, tw, origins = first.shape[0], h, w, None
    if tiles is not None:
        if B != 1:
            raise ValueError(f"{name}: tiles are cut from one frame, not from a batch of {B}")
        th, tw = int(tiles[1][0]), int(tiles[1][1])
        origins = _tile_origins(tiles[0], th, tw, h, w, name)
        B = len(origins)
    H, W = int(out_hw[0]), int(out_hw[1])
    tabs = _fused_tables(first, (th, tw), (H, W), patch, YUV_MAX_FOOTPRINT)
    if tabs is None:
        frame = rgb() if origins is None else tile_crops(rgb(), origins, (th, tw))
        return image_patch_planes(frame, (H, W), patch, mean, std, want_pixels)
    return _yuv_launch(src, tabs, B, th, tw, H, W, patch, mean, std, want_pixels, first.device, name + "_patch_planes",
                       hdr, origins, (h, w))


def _planar_source(y, u, v, subsampling, depth, msb, matrix, full_range, chroma, siting, transfer, peak_nits) -> tuple:
    """A planar frame, checked, as :func:`_yuv_patch_planes`' ``source``."""
    y, u, v = yuv_planes(y, u, v, subsampling, depth)
    table = yuv_table(matrix, full_range, depth)
    _chroma_check(chroma, siting)
    _transfer_check(transfer, peak_nits, depth)
    return (y, tuple(y.shape[1:]), yuv_src(YUV_PLANAR, (y, u, v), subsampling, depth, msb, 0, table, chroma, siting),
            lambda: yuv_to_rgb(y, u, v, subsampling, depth, msb, matrix, full_range, chroma, siting, transfer,
                               peak_nits),
            None if transfer == "sdr" else (transfer, depth, matrix, peak_nits))


def _semiplanar_source(y, uv, subsampling, depth, msb, matrix, full_range, vu, chroma, siting, transfer,
                       peak_nits) -> tuple:
    """A semi-planar frame, checked, as :func:`_yuv_patch_planes`' ``source``."""
    y, uv = yuv_semiplanar_planes(y, uv, subsampling, depth)
    table = yuv_table(matrix, full_range, depth)
    _chroma_check(chroma, siting)
    _transfer_check(transfer, peak_nits, depth)
    B, ch, cw = uv.shape[:3]
    pairs = uv.as_strided((B, ch, 2 * cw), (uv.stride(0), uv.stride(1), 1))   # a view, never a copy
    return (y, tuple(y.shape[1:]),
            yuv_src(YUV_SEMIPLANAR, (y, pairs), subsampling, depth, msb, int(bool(vu)), table, chroma, siting),
            lambda: yuv_semiplanar_to_rgb(y, uv, subsampling, depth, msb, matrix, full_range, vu, chroma, siting,
                                          transfer, peak_nits),
            None if transfer == "sdr" else (transfer, depth, matrix, peak_nits))


def _yuyv_source(data, width, order, matrix, full_range, chroma, siting) -> tuple:
    """A packed 4:2:2 frame, checked, as :func:`_yuv_patch_planes`' ``source``."""
    yv = yuyv_planes(data, width, order)[0]
    _chroma_check(chroma, siting)
    data = data if data.dim() == 3 else data[None]
    table = yuv_table(matrix, full_range, 8)
    return (data, tuple(yv.shape[1:]),
            yuv_src(YUV_PACKED, (data,), "422", 8, False, tuple(YUYV_ORDERS).index(order), table, chroma, siting),
            lambda: yuyv_to_rgb(data, width, order, matrix, full_range, chroma, siting), None)


def yuv_planar_patch_planes(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, out_hw: Tuple[int, int], patch: int,
                            mean: Sequence[float], std: Sequence[float], subsampling: str = "420", depth: int = 8,
                            msb: bool = False, matrix: str = "bt601", full_range: bool = False,
                            want_pixels: bool = False, chroma: str = "nearest", siting: str = "left",
                            transfer: str = "sdr", peak_nits: float = 1000.0) \
        -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """:func:`image_patch_planes` of a planar frame (:func:`yuv_planes`' layout: I422, I444, I010, ``yuv422p10le``
    ...), bit-equal to ``image_patch_planes(yuv_to_rgb(y, u, v, subsampling, depth, msb, matrix, full_range, chroma,
    siting), ...)`` — which is what runs on a CPU tensor, with the ``torch`` backend and past the kernel's limits.
    On the GPU one HIP launch reads the three planes in place, each by its own strides; with ``chroma="bilinear"``
    it interpolates the chroma at ``siting`` (:func:`chroma_upsample`) while it stages them, and with ``transfer``
    ``"pq"`` or ``"hlg"`` it takes the codes through the HDR tables (:func:`hdr_to_sdr`) there as well."""
    source = _planar_source(y, u, v, subsampling, depth, msb, matrix, full_range, chroma, siting, transfer, peak_nits)
    return _yuv_patch_planes(source, "yuv_planar", out_hw, patch, mean, std, want_pixels)


def yuv_semiplanar_patch_planes(y: torch.Tensor, uv: torch.Tensor, out_hw: Tuple[int, int], patch: int,
                                mean: Sequence[float], std: Sequence[float], subsampling: str = "420", depth: int = 8,
                                msb: bool = False, matrix: str = "bt601", full_range: bool = False,
                                want_pixels: bool = False, vu: bool = False, chroma: str = "nearest",
                                siting: str = "left", transfer: str = "sdr", peak_nits: float = 1000.0) \
        -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The same of a semi-planar frame (:func:`yuv_semiplanar_planes`' layout: NV12 / NV21, NV16 / NV61, NV24 / NV42,
    P010, P012, P210, P410), bit-equal to ``image_patch_planes(yuv_semiplanar_to_rgb(...), ...)``. ``vu``: the pairs
    are (V, U)."""
    source = _semiplanar_source(y, uv, subsampling, depth, msb, matrix, full_range, vu, chroma, siting, transfer,
                                peak_nits)
    return _yuv_patch_planes(source, "yuv_semiplanar", out_hw, patch, mean, std, want_pixels)


def yuyv_patch_planes(data: torch.Tensor, width: int, order: str, out_hw: Tuple[int, int], patch: int,
                      mean: Sequence[float], std: Sequence[float], matrix: str = "bt601", full_range: bool = False,
                      want_pixels: bool = False, chroma: str = "nearest", siting: str = "left") \
        -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The same of packed 4:2:2 (:func:`yuyv_planes`' layout: YUY2, UYVY, YVYU), bit-equal to
    ``image_patch_planes(yuyv_to_rgb(data, width, order, matrix, full_range, chroma, siting), ...)``. On the GPU one
    HIP launch reads a group's two macropixels in one read (with bilinear chroma the one before and the one after as
    well), the rows wherever their pitch puts them."""
    source = _yuyv_source(data, width, order, matrix, full_range, chroma, siting)
    return _yuv_patch_planes(source, "yuyv", out_hw, patch, mean, std, want_pixels)


# ---- tiles of one YUV frame -----------------------------------------------------------------------
def yuv_planar_tiled_patch_planes(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, origins,
                                  tile_hw: Tuple[int, int], out_hw: Tuple[int, int], patch: int,
                                  mean: Sequence[float], std: Sequence[float], subsampling: str = "420",
                                  depth: int = 8, msb: bool = False, matrix: str = "bt601", full_range: bool = False,
                                  want_pixels: bool = False, chroma: str = "nearest", siting: str = "left",
                                  transfer: str = "sdr", peak_nits: float = 1000.0) \
        -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """:func:`yuv_planar_patch_planes` of ``B`` tiles of one planar frame (a batch of 1) without converting or
    stacking them: ``origins`` the ``(y0, x0)`` of the tiles, each ``tile_hw`` large and resized to ``out_hw`` ->
    ``(planes [3, B*gh*gw, 3*p*p], pixels [B, 3, H, W] or None)``, bit-equal to ``image_patch_planes(tile_crops(
    yuv_to_rgb(y, u, v, ...), origins, tile_hw), ...)`` — which is what runs on a CPU tensor, with the ``torch``
    backend and past the kernel's limits — and so to :func:`tiled_patch_planes` of the converted frame. On the GPU
    one HIP launch stages every tile from the planes in place: the kernel reads tile ``b``'s origin from
    :func:`origin_tensor`'s device table (cached, dropped by :func:`invalidate_cache`) and moves the patch's
    footprint into the frame, so a chroma sample lies under its luma whatever the origin's parity, and bilinear
    chroma clamps at the frame's edge, not at the tile's."""
    source = _planar_source(y, u, v, subsampling, depth, msb, matrix, full_range, chroma, siting, transfer, peak_nits)
    return _yuv_patch_planes(source, "yuv_planar_tiled", out_hw, patch, mean, std, want_pixels, (origins, tile_hw))


def yuv_semiplanar_tiled_patch_planes(y: torch.Tensor, uv: torch.Tensor, origins, tile_hw: Tuple[int, int],
                                      out_hw: Tuple[int, int], patch: int, mean: Sequence[float],
                                      std: Sequence[float], subsampling: str = "420", depth: int = 8,
                                      msb: bool = False, matrix: str = "bt601", full_range: bool = False,
                                      want_pixels: bool = False, vu: bool = False, chroma: str = "nearest",
                                      siting: str = "left", transfer: str = "sdr", peak_nits: float = 1000.0) \
        -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The same of one semi-planar frame (NV12 / NV21, NV16, NV24, P010 ...: :func:`yuv_semiplanar_patch_planes`'
    arguments), bit-equal to ``image_patch_planes(tile_crops(yuv_semiplanar_to_rgb(...), origins, tile_hw), ...)``."""
    source = _semiplanar_source(y, uv, subsampling, depth, msb, matrix, full_range, vu, chroma, siting, transfer,
                                peak_nits)
    return _yuv_patch_planes(source, "yuv_semiplanar_tiled", out_hw, patch, mean, std, want_pixels, (origins, tile_hw))


def yuyv_tiled_patch_planes(data: torch.Tensor, width: int, order: str, origins, tile_hw: Tuple[int, int],
                            out_hw: Tuple[int, int], patch: int, mean: Sequence[float], std: Sequence[float],
                            matrix: str = "bt601", full_range: bool = False, want_pixels: bool = False,
                            chroma: str = "nearest", siting: str = "left") \
        -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The same of one packed 4:2:2 frame (YUY2, UYVY, YVYU: :func:`yuyv_patch_planes`' arguments), bit-equal to
    ``image_patch_planes(tile_crops(yuyv_to_rgb(data, width, order, ...), origins, tile_hw), ...)``. A tile may start
    at an odd column, in the middle of a macropixel: the kernel's column groups are the frame's."""
    source = _yuyv_source(data, width, order, matrix, full_range, chroma, siting)
    return _yuv_patch_planes(source, "yuyv_tiled", out_hw, patch, mean, std, want_pixels, (origins, tile_hw))


# ---- detections ---------------------------------------------------------------------------------
def target_tensor(target_sizes, batch: int, device: torch.device) -> torch.Tensor:
    """``[B, 2]`` fp32 (height, width) on ``device``; a tensor already there is used as it is (no
    copy, so a captured graph can hold it); None means unscaled boxes."""
    if target_sizes is None:
        return torch.ones(batch, 2, dtype=torch.float32, device=device)
    t = torch.as_tensor(target_sizes)
    t = t.to(device=device, dtype=torch.float32).reshape(-1, 2).contiguous()
    if t.shape[0] != batch:
        raise ValueError("detections: as many target sizes as images")
    return t


def detections_reference(logits: torch.Tensor, boxes: torch.Tensor, target: torch.Tensor, threshold: float) \
        -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The torch composition of :func:`detections` in the inputs' precision, without a host sync."""
    prob = torch.softmax(logits, -1)
    scores, labels = prob[..., :-1].max(-1)
    cx, cy, bw, bh = boxes.unbind(-1)
    xyxy = torch.stack((cx - 0.5 * bw, cy - 0.5 * bh, cx + 0.5 * bw, cy + 0.5 * bh), dim=-1)
    th, tw = target.to(boxes.dtype).unbind(1)
    xyxy = xyxy * torch.stack((tw, th, tw, th), dim=1)[:, None, :]
    keep = scores > threshold
    count = keep.sum(-1).to(torch.int32)
    order = torch.sort((~keep).to(torch.int8), dim=-1, stable=True).indices     # kept rows first, in order
    live = torch.arange(keep.shape[1], device=keep.device)[None, :] < count[:, None]
    # (selected, not multiplied: a NaN score behind the kept rows is a zero there, as the kernel's)
    scores = torch.gather(scores, 1, order)
    scores = torch.where(live, scores, torch.zeros_like(scores))
    labels = (torch.gather(labels, 1, order) * live).to(torch.int32)
    xyxy = torch.gather(xyxy, 1, order[..., None].expand(-1, -1, 4))
    xyxy = torch.where(live[..., None], xyxy, torch.zeros_like(xyxy))
    return count, scores, labels, xyxy


def detections(logits: torch.Tensor, boxes: torch.Tensor, target_sizes, threshold: float) \
        -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``logits [B, M, L+1]``, ``boxes [B, M, 4]`` (centre format, 0..1), ``target_sizes [B, 2]``
    (height, width of each original image) -> ``(count [B] int32, scores [B, M], labels [B, M] int32,
    boxes_xyxy [B, M, 4])``: row ``m`` survives when the largest softmax probability of its first
    ``L`` classes exceeds ``threshold``; survivors stand first, in token order, zeros behind them."""
    B, M, C = logits.shape
    target = target_tensor(target_sizes, B, logits.device)
    if not _use_hip(logits) or logits.dtype != torch.float32 or boxes.dtype != torch.float32 \
            or M > MAX_ROWS or C > MAX_CLASSES or C < 2:
        return detections_reference(logits, boxes, target, threshold)
    logits, boxes = logits.contiguous(), boxes.contiguous()
    dev = logits.device
    count = torch.empty(B, dtype=torch.int32, device=dev)
    scores = torch.empty(B, M, dtype=torch.float32, device=dev)
    labels = torch.empty(B, M, dtype=torch.int32, device=dev)
    xyxy = torch.empty(B, M, 4, dtype=torch.float32, device=dev)
    rc = _L().nos_detections_f32(logits.data_ptr(), boxes.data_ptr(), target.data_ptr(), float(threshold), B, M, C,
                                 count.data_ptr(), scores.data_ptr(), labels.data_ptr(), xyxy.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    _check(rc, "detections")
    return count, scores, labels, xyxy


# ---- the detections of a frame's tiles, merged ------------------------------------------------------
#: how two boxes' overlap is measured: ``ios`` — intersection over the smaller area (an object cut by a tile border
#: gives a partial box inside the fuller one: IoS near 1, IoU small) — or ``iou`` (``nos_merge_detections_f32``'s flag)
MATCHES = {"ios": 0, "iou": 1}


def _merge_check(match: str, match_threshold: float) -> None:
    if match not in MATCHES:
        raise ValueError(f"merge_detections: match {match!r} is none of {tuple(MATCHES)}")
    if not match_threshold >= 0.0:
        raise ValueError(f"merge_detections: match_threshold {match_threshold!r} is not a number from 0 up")


def pair_overlap(a: torch.Tensor, b: torch.Tensor, match: str = "ios") -> torch.Tensor:
    """The overlap of corner boxes ``a [..., 4]`` and ``b [..., 4]`` (broadcast): ``inter / min(area_a, area_b)`` for
    ``"ios"``, ``inter / union`` for ``"iou"``; a denominator that is not positive counts as overlap 0."""
    iw = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0])).clamp_min(0)
    ih = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1])).clamp_min(0)
    inter = iw * ih
    aa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    ab = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    den = aa + ab - inter if match == "iou" else torch.minimum(aa, ab)
    ok = den > 0
    return torch.where(ok, inter / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den))


def merge_detections_reference(logits: torch.Tensor, boxes: torch.Tensor, origins, tile_hw: Tuple[int, int],
                               threshold: float, match: str = "ios", match_threshold: float = 0.5) \
        -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The torch composition of :func:`merge_detections` in the inputs' precision, without a host sync (the greedy
    pass is a loop of ``B * M`` steps on the device, each over one row of the pairwise match matrix)."""
    _merge_check(match, match_threshold)
    B, M, _ = logits.shape
    N = B * M
    dev = logits.device
    org = origin_tensor(origins, dev)
    if org.shape[0] != B:
        raise ValueError("merge_detections: as many origins as tiles")
    th, tw = float(tile_hw[0]), float(tile_hw[1])
    prob = torch.softmax(logits, -1)
    scores, labels = prob[..., :-1].max(-1)
    cx, cy, bw, bh = boxes.unbind(-1)
    oy, ox = org[:, :1].to(boxes.dtype), org[:, 1:].to(boxes.dtype)
    xyxy = torch.stack(((cx - 0.5 * bw) * tw + ox, (cy - 0.5 * bh) * th + oy, (cx + 0.5 * bw) * tw + ox,
                        (cy + 0.5 * bh) * th + oy), dim=-1).reshape(N, 4)
    scores, labels = scores.reshape(N), labels.reshape(N)
    tile = torch.arange(B, device=dev).repeat_interleave(M)
    cand = scores > threshold
    # candidates first, by score descending; the stable sort leaves ties in row (tile, then token) order
    order = torch.sort(torch.where(cand, -scores, torch.full_like(scores, math.inf)), stable=True).indices
    scores, labels, tile, xyxy, cand = scores[order], labels[order], tile[order], xyxy[order], cand[order]
    ov = pair_overlap(xyxy[:, None, :], xyxy[None, :, :], match)
    idx = torch.arange(N, device=dev)
    # hit[p, k]: a kept p drops the later k
    hit = (ov > match_threshold) & (labels[:, None] == labels[None, :]) & (tile[:, None] != tile[None, :]) \
        & (idx[:, None] < idx[None, :]) & cand[:, None] & cand[None, :]
    keep = cand.clone()
    for p in range(N - 1):
        keep &= ~(hit[p] & keep[p])
    count = keep.sum().to(torch.int32).reshape(1)
    front = torch.sort((~keep).to(torch.int8), stable=True).indices     # kept rows first, in order
    live = idx < count
    # (selected, not multiplied: a NaN score or an infinite box behind the kept rows is a zero there, as the kernel's)
    scores, xyxy = scores[front], xyxy[front]
    return (count, torch.where(live, scores, torch.zeros_like(scores)), (labels[front] * live).to(torch.int32),
            torch.where(live[:, None], xyxy, torch.zeros_like(xyxy)), (tile[front] * live).to(torch.int32))


def merge_detections(logits: torch.Tensor, boxes: torch.Tensor, origins, tile_hw: Tuple[int, int], threshold: float,
                     match: str = "ios", match_threshold: float = 0.5) \
        -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The detections of ``B`` tiles of one frame as one list, with no host synchronisation: ``logits [B, M, L+1]``,
    ``boxes [B, M, 4]`` (centre format, 0..1 of a tile), ``origins`` the tiles' ``(y0, x0)`` in the frame (a list, or
    an int32 ``[B, 2]`` tensor on the device), ``tile_hw`` their size -> ``(count [1] int32, scores [B*M], labels [B*M]
    int32, boxes_xyxy [B*M, 4], tile [B*M] int32)``.

    A row is a candidate when its score — :func:`detections`' — exceeds ``threshold``; its box in frame pixels is
    ``((cx - w/2) tw + x0, (cy - h/2) th + y0, (cx + w/2) tw + x0, (cy + h/2) th + y0)``, not clipped. Candidates are
    ordered by score descending (ties: tile, then token, ascending) and passed greedily: one is dropped when an earlier
    *kept* one has the same label, comes from a *different* tile and overlaps it by more than ``match_threshold``
    (:func:`pair_overlap`, ``match`` of :data:`MATCHES`). Boxes of one tile never suppress each other, so one tile
    yields :func:`detections`' survivors stably sorted by score. The kept rows stand first in that order, zeros behind
    them. A row whose logits hold a NaN (or are all ``-inf``) has a NaN score, which exceeds no threshold: it is never
    a candidate, changes nothing about the other rows, and nothing that is not finite is written for it. A box whose
    width or height is not positive overlaps nothing. One HIP launch (one workgroup) up to ``B * M`` = 1024 rows and 128 classes; past that, on the CPU and with
    the ``torch`` backend :func:`merge_detections_reference`."""
    _merge_check(match, match_threshold)
    B, M, C = logits.shape
    if not _use_hip(logits) or logits.dtype != torch.float32 or boxes.dtype != torch.float32 \
            or B * M > MAX_ROWS or C > MAX_CLASSES or C < 2:
        return merge_detections_reference(logits, boxes, origins, tile_hw, threshold, match, match_threshold)
    dev = logits.device
    org = origin_tensor(origins, dev)
    if org.shape[0] != B:
        raise ValueError("merge_detections: as many origins as tiles")
    logits, boxes = logits.contiguous(), boxes.contiguous()
    N = B * M
    count = torch.empty(1, dtype=torch.int32, device=dev)
    scores = torch.empty(N, dtype=torch.float32, device=dev)
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    xyxy = torch.empty(N, 4, dtype=torch.float32, device=dev)
    tile = torch.empty(N, dtype=torch.int32, device=dev)
    rc = _L().nos_merge_detections_f32(logits.data_ptr(), boxes.data_ptr(), org.data_ptr(), float(tile_hw[0]),
                                       float(tile_hw[1]), float(threshold), float(match_threshold), MATCHES[match],
                                       B, M, C, count.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                                       xyxy.data_ptr(), tile.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _check(rc, "merge_detections")
    return count, scores, labels, xyxy, tile


# ---- detections associated across frames --------------------------------------------------------------
#: what a track's box is compared at: where it was (``none``), or one frame further along its velocity
#: (``nos_track_update_f32``'s flag)
MOTIONS = {"none": 0, "constant": 1}
#: tracker limits: slots of one state
MAX_TRACKS = 1024


@dataclass
class TrackState:
    """A tracker's state, entirely on the device (:func:`track_state`): ``boxes [T, 4]`` fp32 (corners, in the pixels
    the detections come in), ``vel [T, 4]`` fp32 (per-frame displacement of the four corners), ``labels``, ``ids``
    (0: a free slot; ids start at 1), ``hits`` (frames matched, birth included), ``misses`` (consecutive frames
    unmatched) ``[T]`` int32, ``next_id [1]`` and ``dropped [1]`` int32 (births refused for lack of a slot). A free
    slot holds zeros in every field."""
    boxes: torch.Tensor
    vel: torch.Tensor
    labels: torch.Tensor
    ids: torch.Tensor
    hits: torch.Tensor
    misses: torch.Tensor
    next_id: torch.Tensor
    dropped: torch.Tensor

    @property
    def capacity(self) -> int:
        return self.ids.shape[0]

    @property
    def device(self) -> torch.device:
        return self.ids.device

    def tensors(self) -> Tuple[torch.Tensor, ...]:
        return (self.boxes, self.vel, self.labels, self.ids, self.hits, self.misses, self.next_id, self.dropped)

    def reset(self) -> None:
        """No track, ``next_id`` 1, nothing dropped: fills on the current stream, in place (capturable)."""
        for t in self.tensors():
            t.zero_()
        self.next_id.fill_(1)


def track_state(capacity: int = 256, device=None) -> TrackState:
    """An empty :class:`TrackState` of ``capacity`` slots on ``device``."""
    T = int(capacity)
    if T < 1:
        raise ValueError(f"track_state: capacity {capacity!r} is not a positive number of slots")
    z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=device)      # noqa: E731
    state = TrackState(z(T, 4, dtype=torch.float32), z(T, 4, dtype=torch.float32), z(T), z(T), z(T), z(T), z(1), z(1))
    state.reset()
    return state


def track_params_check(match_threshold: float, max_age: int, motion: str, velocity_gain: float) -> None:
    """``ValueError`` for parameters :func:`track_update` does not take."""
    if motion not in MOTIONS:
        raise ValueError(f"track_update: motion {motion!r} is none of {tuple(MOTIONS)}")
    if not match_threshold >= 0.0:
        raise ValueError(f"track_update: match_threshold {match_threshold!r} is not a number from 0 up")
    if not max_age >= 0:
        raise ValueError(f"track_update: max_age {max_age!r} is not a number of frames from 0 up")
    if not 0.0 <= velocity_gain <= 1.0:
        raise ValueError(f"track_update: velocity_gain {velocity_gain!r} is not in [0, 1]")


def _track_check(state: TrackState, count, scores, labels, boxes, match_threshold, max_age, motion, velocity_gain) \
        -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The arguments of :func:`track_update` checked; the lists as ``count [1]``, ``scores [N]``, ``labels [N]``,
    ``boxes [N, 4]`` (``[1, M]`` views of one image's :func:`detections` are flattened)."""
    track_params_check(match_threshold, max_age, motion, velocity_gain)
    if scores.dim() == 2 and scores.shape[0] == 1:
        scores, labels, boxes = scores[0], labels.reshape(-1), boxes.reshape(-1, 4)
    if scores.dim() != 1 or count.numel() != 1:
        raise ValueError("track_update: count and scores are one image's: count [1], scores [N] (or [1, N])")
    N = scores.shape[0]
    if labels.shape != (N,) or boxes.shape != (N, 4):
        raise ValueError(f"track_update: labels {tuple(labels.shape)} and boxes {tuple(boxes.shape)} do not go with "
                         f"the {N} scores")
    for name, t in (("count", count), ("scores", scores), ("labels", labels), ("boxes", boxes)):
        if t.device != state.device:
            raise ValueError(f"track_update: state is on {state.device}, {name} on {t.device}")
    return count.reshape(1), scores, labels, boxes


def track_update_reference(state: TrackState, count: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor,
                           boxes: torch.Tensor, match_threshold: float = 0.3, max_age: int = 30,
                           birth_threshold: float = 0.0, motion: str = "constant", velocity_gain: float = 0.5) \
        -> Tuple[torch.Tensor, torch.Tensor]:
    """The torch composition of :func:`track_update`, with the same effect on ``state`` in place and without a host
    sync (the greedy pass is a loop of ``N`` steps on the device, each over one row of the candidate x track IoU
    matrix). The lists are taken in the state's fp32."""
    count, scores, labels, boxes = _track_check(state, count, scores, labels, boxes, match_threshold, max_age, motion,
                                                velocity_gain)
    if scores.shape[0] == 0:        # no row: one that is no candidate, and nothing to return
        none = track_update_reference(state, count, scores.new_zeros(1), labels.new_zeros(1), boxes.new_zeros(1, 4),
                                      match_threshold, max_age, birth_threshold, motion, velocity_gain)
        return none[0][:0], none[1][:0]
    N, T, dev = scores.shape[0], state.capacity, state.device
    scores, boxes, labels = scores.to(torch.float32), boxes.to(torch.float32), labels.to(torch.int32)
    constant = motion == "constant"
    rows, slots = torch.arange(N, device=dev), torch.arange(T, device=dev)
    cand = (rows < count.clamp(0, N)) & (scores > 0)
    # candidates first, by score descending; the stable sort leaves ties in row order
    order = torch.sort(torch.where(cand, -scores, torch.full_like(scores, math.inf)), stable=True).indices
    sc, lb, bx, cd = scores[order], labels[order], boxes[order], cand[order]
    live = state.ids != 0
    pred = state.boxes + state.vel if constant else state.boxes
    ov = pair_overlap(bx[:, None, :], pred[None, :, :], "iou")
    ok = (ov > match_threshold) & (lb[:, None] == state.labels[None, :]) & live[None, :] & cd[:, None]
    ov = torch.where(ok, ov, torch.full_like(ov, -1.0))
    taken = torch.zeros(T, dtype=torch.bool, device=dev)
    match = torch.full((N,), T, dtype=torch.int64, device=dev)          # T: no track
    for c in range(N):
        v = torch.where(taken, -1.0, ov[c])
        best = v.max()
        slot = torch.where((v == best) & (best >= 0), slots, T).min()   # the lowest slot of the largest overlap
        match[c] = slot
        taken = taken | (slots == slot)
    hit = match[:, None] == slots[None, :]                              # [N, T], at most a one per row and column
    rank_of = hit.to(torch.int8).argmax(0)                              # the candidate a taken track took
    box_in = bx[rank_of]
    vel = state.vel + velocity_gain * ((box_in - state.boxes) - state.vel) if constant else state.vel
    missed = live & ~taken
    misses = torch.where(missed, state.misses + 1, torch.zeros_like(state.misses))
    dead = missed & (misses > max_age)
    new_boxes = torch.where(taken[:, None], box_in, state.boxes + state.vel if constant else state.boxes)
    new_vel = torch.where(taken[:, None], vel, state.vel)
    hits = state.hits + taken.to(torch.int32)
    keep = live & ~dead
    k4 = keep[:, None]
    new_boxes, new_vel = torch.where(k4, new_boxes, 0.0), torch.where(k4, new_vel, 0.0)
    new_labels, new_ids = state.labels * keep, state.ids * keep
    hits, misses = hits * keep, misses * keep
    # births: the b-th unmatched candidate above the birth threshold into the b-th free slot
    want = cd & (match == T) & (sc > birth_threshold)
    free = ~keep
    b = torch.cumsum(want, 0) - 1
    nb, nf = want.sum(), free.sum()
    born = want & (b < nf)
    free_slots = torch.sort((~free).to(torch.int8), stable=True).indices        # free slots first, ascending
    dest = torch.where(born, free_slots[b.clamp(0, T - 1)], T)                   # T: a spare row behind the state
    first = state.next_id[0]
    new_id = (first + b).to(torch.int32) * born

    def place(old, new):
        ext = torch.cat((old, old.new_zeros((1,) + tuple(old.shape[1:]))))
        ext.index_copy_(0, dest, new.to(old.dtype))
        return ext[:T]
    one = born.to(torch.int32)
    new_boxes, new_vel = place(new_boxes, bx), place(new_vel, torch.zeros_like(bx))
    new_labels, new_ids = place(new_labels.to(torch.int32), lb), place(new_ids.to(torch.int32), new_id)
    hits, misses = place(hits.to(torch.int32), one), place(misses.to(torch.int32), torch.zeros_like(one))
    # the outputs by rank, then back to the input's rows
    ext_ids, ext_hits = torch.cat((new_ids, new_ids.new_zeros(1))), torch.cat((hits, hits.new_zeros(1)))
    out_id = torch.where(born, new_id, ext_ids[match] * cd)
    out_hits = torch.where(born, one, ext_hits[match] * cd)
    track_id = torch.zeros(N, dtype=torch.int32, device=dev).index_copy_(0, order, out_id.to(torch.int32))
    track_hits = torch.zeros(N, dtype=torch.int32, device=dev).index_copy_(0, order, out_hits.to(torch.int32))
    started = torch.minimum(nb, nf)
    state.next_id.add_(started.to(torch.int32))
    state.dropped.add_((nb - started).to(torch.int32))
    for t, new in zip(state.tensors()[:6], (new_boxes, new_vel, new_labels, new_ids, hits, misses)):
        t.copy_(new)
    return track_id, track_hits


def track_update(state: TrackState, count: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor,
                 boxes: torch.Tensor, match_threshold: float = 0.3, max_age: int = 30, birth_threshold: float = 0.0,
                 motion: str = "constant", velocity_gain: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """One frame's detections — ``count [1]`` int32, ``scores [N]``, ``labels [N]`` int32, ``boxes [N, 4]`` (corners),
    what :func:`detections` (one image; its ``[1, M]`` views are accepted) and :func:`merge_detections` return —
    associated with the tracks of ``state``, which is updated in place, with no host synchronisation: captured in a
    graph, each replay is the next frame. Returns ``(track_id [N], track_hits [N])`` int32 in the input's row order:
    the id of the row's track and its ``hits`` after this update, 0 for a row without one.

    Row ``r`` is a candidate when ``r < count`` (clamped to ``[0, N]``) and ``scores[r] > 0``; a NaN score never is.

    1. A live track's predicted box is ``boxes + vel`` (``motion="constant"``) or ``boxes`` (``"none"``).
    2. Candidates go by score descending (ties: the lower row). Each takes the live track of the same label that no
       earlier candidate took and whose IoU with the predicted box (:func:`pair_overlap`, ``"iou"``) is largest, when
       that exceeds ``match_threshold`` (ties: the lowest slot). A box of no or negative extent matches nothing.
    3. A matched track: ``vel += velocity_gain * ((box - boxes) - vel)`` (zero under ``"none"``), ``boxes = box`` bit
       for bit, ``hits += 1``, ``misses = 0``.
    4. Any other live track: ``misses += 1``; past ``max_age`` its slot is freed and zeroed, else ``boxes += vel``
       under ``"constant"``.
    5. Unmatched candidates with ``score > birth_threshold`` start tracks, in score order in the free slots ascending
       (those freed in step 4 included): ``ids = next_id++``, ``hits = 1``. When the slots run out, each remaining one
       adds 1 to ``dropped``.

    One HIP launch (one workgroup) for fp32 lists up to 1024 rows and a state up to 1024 slots; past that, for other
    dtypes, on the CPU and with the ``torch`` backend :func:`track_update_reference`."""
    lists = _track_check(state, count, scores, labels, boxes, match_threshold, max_age, motion, velocity_gain)
    count, scores, labels, boxes = lists
    N, T = scores.shape[0], state.capacity
    if not _use_hip(scores) or scores.dtype != torch.float32 or boxes.dtype != torch.float32 \
            or labels.dtype != torch.int32 or count.dtype != torch.int32 or N > MAX_ROWS or T > MAX_TRACKS or N < 1:
        return track_update_reference(state, *lists, match_threshold, max_age, birth_threshold, motion, velocity_gain)
    scores, labels, boxes = scores.contiguous(), labels.contiguous(), boxes.contiguous()
    track_id = torch.empty(N, dtype=torch.int32, device=scores.device)
    track_hits = torch.empty(N, dtype=torch.int32, device=scores.device)
    rc = _L().nos_track_update_f32(count.data_ptr(), scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(), N,
                                   *(t.data_ptr() for t in state.tensors()), T, float(match_threshold), int(max_age),
                                   float(birth_threshold), MOTIONS[motion], float(velocity_gain), track_id.data_ptr(),
                                   track_hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _check(rc, "track_update")
    return track_id, track_hits


# ---- detections drawn into the frame --------------------------------------------------------------------
#: the ten digits, 5 x 7: a digit's seven rows, bit 4 the leftmost column (the kernel reads the same table)
OVERLAY_FONT = (
    (0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110),
    (0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110),
    (0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111),
    (0b11111, 0b00010, 0b00100, 0b00010, 0b00001, 0b10001, 0b01110),
    (0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010),
    (0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110),
    (0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110),
    (0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000),
    (0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110),
    (0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100),
)
#: the drawing modes of a label (``nos_overlay_*``'s ``modes`` table)
OVERLAY_MODES = {"off": 0, "outline": 1, "redact": 2}
#: the raster tile of the kernel (rows, columns of luma pixels per workgroup), and its limits (``csrc/image_overlay.h``)
OVERLAY_TILE = (32, 64)
OVERLAY_MAX_THICKNESS, OVERLAY_MAX_SCALE, OVERLAY_MAX_COLOURS = 1 << 20, 1 << 10, 1 << 10
#: a coordinate is clamped to this size, in fp32, before it is floored
OVERLAY_CLAMP = float(1 << 20)


def overlay_palette(K: int = 16) -> np.ndarray:
    """``[K, 2, 3]`` uint8 RGB: ``K`` fill colours — hues a golden-ratio step apart at full saturation, in fp64 —
    each with the text colour that reads on it: black when the fill's BT.709 luma ``0.2126 R + 0.7152 G + 0.0722 B``
    is 128 or more, else white."""
    K = int(K)
    if not 1 <= K <= OVERLAY_MAX_COLOURS:
        raise ValueError(f"overlay_palette: {K!r} is not a number of colours in 1..{OVERLAY_MAX_COLOURS}")
    out = np.zeros((K, 2, 3), dtype=np.uint8)
    for k in range(K):
        hue = 6.0 * ((k * 0.6180339887498949) % 1.0)
        x = 1.0 - abs(hue % 2.0 - 1.0)
        rgb = ((1.0, x, 0.0), (x, 1.0, 0.0), (0.0, 1.0, x), (0.0, x, 1.0), (x, 0.0, 1.0), (1.0, 0.0, x))[int(hue) % 6]
        out[k, 0] = np.floor(255.0 * np.array(rgb) + 0.5)
        out[k, 1] = 0 if float(np.dot((0.2126, 0.7152, 0.0722), out[k, 0].astype(np.float64))) >= 128.0 else 255
    return out


@dataclass
class OverlaySurface:
    """What :func:`overlay` knows of a target (:func:`overlay_surface`): the frame's size, ``packed = (data [1, h, w,
    C], order)`` or ``yuv = (layout, planes, subsampling, depth, msb, order)`` as :func:`yuv_src` takes them, how a YUV
    colour becomes codes (``colour = (matrix, full_range, depth)``, None for packed pixels), and ``samples``: every
    written sample plane as ``(2-D strided view, colour component, hsub, vsub)``; ``shift`` moves a code into a
    16-bit word's high bits."""
    h: int
    w: int
    device: torch.device
    packed: Optional[tuple]
    yuv: Optional[tuple]
    colour: Optional[tuple]
    samples: list
    shift: int = 0


def _writable(views, who: str) -> None:
    for v in views:
        if any(st == 0 and n > 1 for st, n in zip(v.stride(), v.shape)):
            raise ValueError(f"{who}: the target is an expanded view, not memory a frame can be written into")


def overlay_surface(target) -> OverlaySurface:
    """A target described, without a copy. ``target``: a uint8 ``[h, w, 3]`` (or ``[1, h, w, 3]``) RGB tensor whose
    rows may be pitched, or a frame of ``models/workload``: ``Packed`` (``data``, ``order``), ``Nv12`` / ``YuvSemiPlanar``
    (``y``, ``uv``), ``Yuv420p`` / ``YuvPlanar`` (``y``, ``u``, ``v``) or ``Yuyv`` (``data``, ``width``) — told apart by
    those fields, so nothing here imports them. ``ValueError`` for a batch above one, a transfer that is not ``sdr``
    and memory that is not a writable surface of the layout."""
    who = "overlay"
    if getattr(target, "transfer", "sdr") != "sdr":
        raise ValueError(f"{who}: an SDR colour has no code on a {target.transfer!r} surface (no inverse tone map)")
    g = lambda name, default: getattr(target, name, default)    # noqa: E731
    if isinstance(target, torch.Tensor) or (hasattr(target, "data") and hasattr(target, "order")
                                            and not hasattr(target, "width")):
        data, order = (target, "rgb") if isinstance(target, torch.Tensor) else (target.data, target.order)
        if order not in PACKED_ORDERS:
            raise ValueError(f"{who}: channel order {order!r} is none of {sorted(PACKED_ORDERS)}")
        C, (r, _, b) = PACKED_ORDERS[order]
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() not in (3, 4) \
                or data.shape[-1] != C or 0 in data.shape:
            raise ValueError(f"{who}: {order} takes a uint8 [h, w, {C}] tensor")
        data = data if data.dim() == 4 else data[None]
        if data.shape[0] != 1:
            raise ValueError(f"{who}: one frame, not a batch of {data.shape[0]}")
        if not _packed_strides(data):
            raise ValueError(f"{who}: rows may be pitched, but the bytes of a row are contiguous")
        _writable((data,), who)
        return OverlaySurface(data.shape[1], data.shape[2], data.device, (data, order), None, None,
                              [(data[0, :, :, c], k, 0, 0) for k, c in enumerate((r, 1, b))])
    matrix, full = g("matrix", "bt601"), bool(g("full_range", False))
    if hasattr(target, "data") and hasattr(target, "width"):
        order = g("order", "yuyv")
        yv, uv, vv = yuyv_planes(target.data, target.width, order)
        data = target.data if target.data.dim() == 3 else target.data[None]
        planes, sub, depth, msb = (data,), "422", 8, False
        yuv = (YUV_PACKED, planes, sub, depth, msb, tuple(YUYV_ORDERS).index(order))
        views = (yv, uv, vv)
    elif hasattr(target, "y") and hasattr(target, "uv"):
        sub, depth, msb = g("subsampling", "420"), g("depth", 8), bool(g("msb", False))
        y, uv = yuv_semiplanar_planes(target.y, target.uv, sub, depth)
        B, ch, cw = uv.shape[:3]
        pairs = uv.as_strided((B, ch, 2 * cw), (uv.stride(0), uv.stride(1), 1))
        vu = int(bool(g("vu", False)))
        yuv = (YUV_SEMIPLANAR, (y, pairs), sub, depth, msb, vu)
        views = (y, uv[..., vu], uv[..., 1 - vu])
    elif hasattr(target, "y") and hasattr(target, "u") and hasattr(target, "v"):
        sub, depth, msb = g("subsampling", "420"), g("depth", 8), bool(g("msb", False))
        views = yuv_planes(target.y, target.u, target.v, sub, depth)
        yuv = (YUV_PLANAR, tuple(views), sub, depth, msb, 0)
    else:
        raise ValueError(f"{who}: the target is a uint8 [h, w, 3] tensor or a Packed, Nv12, Yuv420p, YuvPlanar, "
                         f"YuvSemiPlanar or Yuyv frame, not {type(target).__name__}")
    _yuv_check(matrix, yuv[3])
    if views[0].shape[0] != 1:
        raise ValueError(f"{who}: one frame, not a batch of {views[0].shape[0]}")
    _writable(yuv[1], who)
    hs, vs = YUV_SUBSAMPLING[yuv[2]]
    samples = [(views[0][0], 0, 0, 0), (views[1][0], 1, hs, vs), (views[2][0], 2, hs, vs)]
    return OverlaySurface(views[0].shape[1], views[0].shape[2], views[0].device, None, yuv, (matrix, full, yuv[3]),
                          samples, 16 - yuv[3] if (yuv[4] and yuv[3] != 8) else 0)


def overlay_host_codes(palette, redact_rgb, colour: Optional[tuple]) -> np.ndarray:
    """The colour table of :func:`overlay_codes` on the host, int32 ``[2 K + 1, 3]``: entry ``k``'s fill at ``2 k``,
    its text colour at ``2 k + 1``, the redact colour last. ``colour`` None: the RGB bytes. ``colour = (matrix,
    full_range, depth)``: Y, U, V codes — the inverse of :func:`yuv_real_matrix` applied in fp64, ``inv(M) @ rgb +
    offsets``, rounded half up and clipped to ``[0, 2^depth - 1]``."""
    pal = np.asarray(palette)
    if pal.ndim != 3 or pal.shape[1:] != (2, 3) or not 1 <= pal.shape[0] <= OVERLAY_MAX_COLOURS \
            or pal.dtype.kind not in "iu" or pal.min() < 0 or pal.max() > 255:
        raise ValueError(f"overlay: a palette is [K, 2, 3] integers in 0..255 with 1 <= K <= {OVERLAY_MAX_COLOURS}")
    red = np.asarray(redact_rgb)
    if red.shape != (3,) or red.dtype.kind not in "iu" or red.min() < 0 or red.max() > 255:
        raise ValueError("overlay: the redact colour is three integers in 0..255")
    rgb = np.concatenate((pal.reshape(-1, 3), red[None])).astype(np.float64)
    if colour is None:
        return rgb.astype(np.int32)
    matrix, full_range, depth = colour
    m, off = yuv_real_matrix(matrix, full_range, depth)
    yuv = rgb @ np.linalg.inv(m).T + np.array(off, dtype=np.float64)
    return np.clip(np.floor(yuv + 0.5), 0, (1 << depth) - 1).astype(np.int32)


#: the colour tables of :func:`overlay_codes` per (palette, redact colour, layout description, device), and the glyph
#: table per device: read by address by a recorded launch, so kept as :data:`_tables` are
_overlay_tables = GraphCache(16)


def overlay_codes(palette, redact_rgb, frame) -> torch.Tensor:
    """``palette`` (:func:`overlay_palette`'s shape) and the redact colour as the codes of ``frame``'s surface
    (:func:`overlay_host_codes`), an int32 ``[2 K + 1, 3]`` table on the frame's device, cached: a captured graph
    must not copy from the host, so make it eagerly first; :func:`invalidate_cache` drops it."""
    s = frame if isinstance(frame, OverlaySurface) else overlay_surface(frame)
    pal, red = np.asarray(palette), np.asarray(redact_rgb)
    key = ("codes", pal.shape, pal.tobytes(), red.tobytes(), s.colour, str(s.device))
    return _overlay_tables.get(key, lambda: torch.from_numpy(overlay_host_codes(pal, red, s.colour)).to(s.device))


def _overlay_table(name: str, values, device: torch.device) -> torch.Tensor:
    """A constant int32 table on ``device``, cached by name."""
    return _overlay_tables.get((name, str(device)), lambda: torch.tensor(values, dtype=torch.int32).to(device))


def _overlay_font(device: torch.device) -> torch.Tensor:
    return _overlay_table("font", OVERLAY_FONT, device)


def _overlay_check(surface: OverlaySurface, count, scores, labels, boxes, track_id, track_hits, thickness, scale, modes,
                   min_hits, codes) -> tuple:
    """The arguments of :func:`overlay` checked, ``ValueError`` before any launch; the lists as ``count [1]``,
    ``scores [N]``, ``labels [N]``, ``boxes [N, 4]``, ids and hits ``[N]`` or None (``[1, N]`` views are flattened)."""
    who = "overlay"
    if not 1 <= int(thickness) <= OVERLAY_MAX_THICKNESS:
        raise ValueError(f"{who}: thickness {thickness!r} is not in 1..{OVERLAY_MAX_THICKNESS}")
    if not 0 <= int(scale) <= OVERLAY_MAX_SCALE:
        raise ValueError(f"{who}: scale {scale!r} is not in 0..{OVERLAY_MAX_SCALE} (0: no tags)")
    if not int(min_hits) >= 1:
        raise ValueError(f"{who}: min_hits {min_hits!r} is not a number of frames from 1 up")
    if (track_id is None) != (track_hits is None):
        raise ValueError(f"{who}: track_id and track_hits go together")
    if scores.dim() == 2 and scores.shape[0] == 1:
        scores, labels, boxes = scores[0], labels.reshape(-1), boxes.reshape(-1, 4)
        if track_id is not None:
            track_id, track_hits = track_id.reshape(-1), track_hits.reshape(-1)
    if scores.dim() != 1 or count.numel() != 1:
        raise ValueError(f"{who}: count and scores are one frame's: count [1], scores [N] (or [1, N])")
    N = scores.shape[0]
    if labels.shape != (N,) or boxes.shape != (N, 4) or (track_id is not None and (track_id.shape != (N,)
                                                                                 or track_hits.shape != (N,))):
        raise ValueError(f"{who}: labels, boxes [N, 4] and ids do not go with the {N} scores")
    ints = (torch.int32, torch.int64)
    if not scores.is_floating_point() or not boxes.is_floating_point() or labels.dtype not in ints \
            or count.dtype not in ints or (track_id is not None and (track_id.dtype not in ints
                                                                    or track_hits.dtype not in ints)):
        raise ValueError(f"{who}: floating-point scores and boxes, int32 or int64 count, labels, ids and hits")
    if not isinstance(modes, torch.Tensor) or modes.dtype != torch.uint8 or modes.dim() != 1 or modes.numel() < 1:
        raise ValueError(f"{who}: modes is a uint8 [L] tensor of 0 (not drawn), 1 (outline and tag), 2 (redacted)")
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.int32 or codes.dim() != 2 or codes.shape[1] != 3 \
            or codes.shape[0] < 3 or codes.shape[0] % 2 != 1 or codes.shape[0] > 2 * OVERLAY_MAX_COLOURS + 1 \
            or not codes.is_contiguous():
        raise ValueError(f"{who}: codes is overlay_codes' contiguous int32 [2 K + 1, 3] table")
    for name, t in (("count", count), ("scores", scores), ("labels", labels), ("boxes", boxes), ("track_id", track_id),
                    ("track_hits", track_hits), ("modes", modes), ("codes", codes)):
        if t is not None and t.device != surface.device:
            raise ValueError(f"{who}: the target is on {surface.device}, {name} on {t.device}")
    return count.reshape(1), scores, labels, boxes, track_id, track_hits


def overlay_slots(h: int, w: int, count, scores, labels, boxes, track_id, track_hits, thickness: int, scale: int,
                  modes: torch.Tensor, min_hits: int, K: int) -> torch.Tensor:
    """The drawing rule of :func:`overlay` on the lists' device, without a host sync: int32 ``[h, w]``, the colour slot
    of every pixel (``2 k`` fill and ``2 k + 1`` text of palette entry ``k``, ``2 K`` the redact colour) or -1 where
    nothing is drawn. Written for clarity: a loop of ``N`` steps over full-frame masks."""
    dev, N, t, s = scores.device, scores.shape[0], int(thickness), int(scale)
    i32 = torch.int32
    Y = torch.arange(h, device=dev, dtype=i32)[:, None]
    X = torch.arange(w, device=dev, dtype=i32)[None, :]
    font, tens = _overlay_font(dev), _overlay_table("tens", (1, 10, 100, 1000, 10000, 100000), dev)
    L = modes.shape[0]
    lb = labels.to(torch.int64)
    inside = (lb >= 0) & (lb < L)
    mode = torch.where(inside, modes[lb.clamp(0, L - 1)].to(i32), 0)
    bx = boxes.to(torch.float32)
    finite = torch.isfinite(bx).all(dim=1)
    c = torch.where(finite[:, None], bx, 0.0).clamp(-OVERLAY_CLAMP, OVERLAY_CLAMP)
    x0, y0 = torch.floor(c[:, 0]).to(i32), torch.floor(c[:, 1]).to(i32)
    x1, y1 = torch.ceil(c[:, 2]).to(i32) - 1, torch.ceil(c[:, 3]).to(i32) - 1
    n = count.reshape(1)[0].clamp(0, N)
    ok = (torch.arange(N, device=dev) < n) & (scores.to(torch.float32) > 0) & ((mode == 1) | (mode == 2)) & finite \
        & (x1 >= x0) & (y1 >= y0)
    key = lb
    if track_id is not None:
        ok = ok & (track_id > 0) & (track_hits >= int(min_hits))
        key = track_id.to(torch.int64)
    key = torch.where(ok, key, 0)          # (a row that is not drawn may hold anything)
    v = (key % 1000000).to(i32)
    nd = 1 + sum((v >= p).to(i32) for p in (10, 100, 1000, 10000, 100000))
    col = torch.where(mode == 2, 2 * K, 2 * (key % K)).to(i32)
    ty = torch.where(y0 - 9 * s >= 0, y0 - 9 * s, y0)
    slot = torch.full((h, w), -1, dtype=i32, device=dev)
    for r in range(N):
        outer = (X >= x0[r]) & (X <= x1[r]) & (Y >= y0[r]) & (Y <= y1[r])
        inner = (X >= x0[r] + t) & (X <= x1[r] - t) & (Y >= y0[r] + t) & (Y <= y1[r] - t)
        mine = torch.where(outer & ((mode[r] == 2) | ~inner), col[r], -1)
        if s > 0:
            u, tv = X - x0[r], Y - ty[r]
            tag = (mode[r] == 1) & (u >= 0) & (u < (6 * nd[r] + 1) * s) & (tv >= 0) & (tv < 9 * s)
            gu, gv = u - s, tv - s
            glyph = (gu >= 0) & (gu < 6 * s * nd[r]) & (gv >= 0) & (gv < 7 * s)
            gu, gv = gu.clamp(0, 36 * s - 1), gv.clamp(0, 7 * s - 1)
            digit = torch.div(v[r], tens[(nd[r] - 1 - torch.div(gu, 6 * s, rounding_mode="floor")).clamp(0, 5).long()],
                              rounding_mode="floor") % 10
            cu = torch.div(gu % (6 * s), s, rounding_mode="floor")
            bits = font[digit.long(), torch.div(gv, s, rounding_mode="floor").long()]      # [h, w] by broadcast
            text = glyph & (cu < 5) & (((bits >> (4 - cu.clamp(max=4))) & 1) == 1)
            mine = torch.where(tag, torch.where(text, col[r] + 1, col[r]), mine)
        slot = torch.where((slot < 0) & ok[r], mine, slot)
    return slot


def overlay_reference(target, count: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, boxes: torch.Tensor,
                      track_id: Optional[torch.Tensor] = None, track_hits: Optional[torch.Tensor] = None, *,
                      thickness: int, scale: int, modes: torch.Tensor, min_hits: int = 1, codes: torch.Tensor):
    """The torch composition of :func:`overlay`, with the same effect on ``target`` in place and without a host sync:
    :func:`overlay_slots`, then every sample plane of the surface rewritten through its strided view — the sample of
    ``(cy, cx)`` takes the colour of luma pixel ``(cy << vsub, cx << hsub)`` where that pixel is painted and keeps its
    value elsewhere."""
    surface = overlay_surface(target)
    lists = _overlay_check(surface, count, scores, labels, boxes, track_id, track_hits, thickness, scale, modes,
                           min_hits, codes)
    if lists[1].shape[0] == 0:
        return target
    slot = overlay_slots(surface.h, surface.w, *lists, thickness, scale, modes, min_hits, (codes.shape[0] - 1) // 2)
    for view, comp, hs, vs in surface.samples:
        sub = slot[::1 << vs, ::1 << hs]
        val = codes[sub.clamp(min=0).long(), comp] << surface.shift
        if view.dtype == torch.uint8:
            view.copy_(torch.where(sub >= 0, val.to(torch.uint8), view))
        else:       # 16-bit words, written whole: the same bits as int16
            bits = view if view.dtype == torch.int16 else view.view(torch.int16)
            bits.copy_(torch.where(sub >= 0, ((val + 32768) % 65536 - 32768).to(torch.int16), bits))
    return target


def overlay(target, count: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, boxes: torch.Tensor,
            track_id: Optional[torch.Tensor] = None, track_hits: Optional[torch.Tensor] = None, *, thickness: int,
            scale: int, modes: torch.Tensor, min_hits: int = 1, codes: torch.Tensor):
    """One frame's detections — ``count [1]``, ``scores [N]``, ``labels [N]``, ``boxes [N, 4]`` (corners, frame pixels)
    as :func:`detections` (one image; its ``[1, N]`` views are accepted) and :func:`merge_detections` return them, and
    optionally ``track_id``, ``track_hits`` ``[N]`` of :func:`track_update` — painted into ``target``
    (:func:`overlay_surface`) in place, with no host synchronisation, no RGB frame and no copy; returns ``target``.
    ``modes``: uint8 ``[L]`` on the device, per label 0 (not drawn), 1 (outline and tag) or 2 (redacted); ``codes``:
    :func:`overlay_codes`' table of ``K`` palette entries and the redact colour. The rule, in exact integers:

    1. Row ``r`` is drawn when ``r < clamp(count, 0, N)``, ``scores[r] > 0`` (a NaN is not), ``0 <= labels[r] < L``
       with a mode of 1 or 2, all four coordinates finite, with ids ``track_id[r] > 0`` and ``track_hits[r] >=
       min_hits``, and its rectangle not empty.
    2. Each coordinate is clamped in fp32 to ``[-2^20, 2^20]``; pixel ``i`` covers ``[i, i + 1)``, so the outer
       rectangle is columns ``floor(x0) .. ceil(x1) - 1`` and rows ``floor(y0) .. ceil(y1) - 1``, inclusive.
    3. Mode 1 paints the outer rectangle minus the inner one, ``thickness`` in from every side (a box thinner than
       twice that is solid), in fill colour ``key mod K``; ``key`` is the row's id with ids, else its label. With
       ``scale = s > 0`` it also paints a tag: ``key mod 10^6`` in decimal, ``nd`` digits of :data:`OVERLAY_FONT` in
       cells ``6 s`` wide inside a margin of ``s`` — ``(6 nd + 1) s`` wide and ``9 s`` high, its columns from the box's
       first, its rows above the box when they fit the frame, else from the box's first row; the digits' set bits in the
       text colour, the rest of the tag in the fill colour. Mode 2 paints the whole outer rectangle in the redact colour.
    4. Everything is clipped to the frame; where several rows cover a pixel, the lowest row wins.
    5. Packed pixels: the three colour bytes, never a fourth. YUV: the luma sample of every painted pixel, and a chroma
       sample ``(cy, cx)`` exactly when luma pixel ``(cy << vsub, cx << hsub)`` is painted, in that pixel's colour (so a
       one-pixel line on an odd column of a subsampled surface changes luma only); 16-bit samples as whole words,
       ``code << shift``. No other byte is written: not the pitch padding, not the parent of a crop.

    One HIP launch (a workgroup per :data:`OVERLAY_TILE` of luma pixels) for fp32 / int32 lists up to 1024 rows on the
    GPU; past that, for other dtypes, on the CPU and with the ``torch`` backend :func:`overlay_reference`. Alpha
    blending, antialiased lines, class names or any glyph but digits, PQ / HLG surfaces, batches above one and more
    than 1024 rows are not offered."""
    surface = overlay_surface(target)
    lists = _overlay_check(surface, count, scores, labels, boxes, track_id, track_hits, thickness, scale, modes,
                           min_hits, codes)
    count, scores, labels, boxes, track_id, track_hits = lists
    N = scores.shape[0]
    i32 = torch.int32
    if not _use_hip(scores) or scores.dtype != torch.float32 or boxes.dtype != torch.float32 or labels.dtype != i32 \
            or count.dtype != i32 or (track_id is not None and (track_id.dtype != i32 or track_hits.dtype != i32)) \
            or N > MAX_ROWS or N < 1:
        return overlay_reference(target, *lists, thickness=thickness, scale=scale, modes=modes, min_hits=min_hits,
                                 codes=codes)
    scores, labels, boxes, modes = scores.contiguous(), labels.contiguous(), boxes.contiguous(), modes.contiguous()
    ids = (None, None) if track_id is None else (track_id.contiguous(), track_hits.contiguous())
    tail = (count.data_ptr(), scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(),
            None if ids[0] is None else ids[0].data_ptr(), None if ids[1] is None else ids[1].data_ptr(), N,
            modes.data_ptr(), modes.shape[0], codes.data_ptr(), (codes.shape[0] - 1) // 2,
            _overlay_font(surface.device).data_ptr(), int(thickness), int(scale), int(min_hits),
            torch.cuda.current_stream().cuda_stream)
    if surface.packed is not None:
        data, order = surface.packed
        lo, hi = _storage_bounds(data)
        pitch = data.stride(1) if data.shape[1] > 1 else data.shape[2] * data.shape[3]
        rc = _L().nos_overlay_packed(data.data_ptr(), lo, hi, pitch, order.encode(), surface.h, surface.w, *tail)
    else:
        src = yuv_src(*surface.yuv, (0,) * 12)
        rc = _L().nos_overlay_yuv(ctypes.byref(src), surface.h, surface.w, *tail)
    _check(rc, "overlay")
    return target
