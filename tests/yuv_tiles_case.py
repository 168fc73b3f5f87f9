"""What ``tests/test_yuv_tiles.py`` (CPU) and ``tests/test_gpu_yuv_tiles.py`` (HIP) share: one frame per YUV layout,
the tile origins, and the yardstick. The yardstick everywhere is bit equality with the packed tile launch on the
frame's ``rgb()`` — ``ops.image.tiled_patch_planes(frame.rgb(), "rgb", origins, tile_hw, out_hw, ...)`` — which on
the CPU is ``image_patch_planes`` of the stacked crops."""
import torch

from walkai_nos_amd.models.workload import surfaces
from walkai_nos_amd.models.workload.processor import Nv12, Yuv420p
from walkai_nos_amd.ops import image as I

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
P = 16
#: tiles of 56 x 72 resized to 32 x 48 (scales 1.75 and 1.5)
TILE_HW, OUT_HW = (56, 72), (32, 48)

#: every layout of the general YUV front end, nearest chroma. Odd sizes where the layout allows (then the chroma
#: planes are (h+1)/2 x (w+1)/2); an even width for packed 4:2:2, even sizes for the ``from_buffer`` surfaces.
LAYOUTS = ("nv12", "nv21", "i420", "yv12", "i422", "i444", "nv16", "yuy2", "uyvy", "yvyu", "p010", "i010", "i422p12",
           "i444p12")


def _gen(name, h, w, seed):
    return torch.Generator().manual_seed(seed * 7919 + h * 1009 + w + sum(name.encode()))


def _u8(g, *shape):
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


def _words(g, depth, *shape):
    """``depth``-bit codes in the low bits of uint16 words."""
    return torch.randint(0, 1 << depth, shape, generator=g, dtype=torch.int32).to(torch.int16).view(torch.uint16)


def frame_hw(name):
    if name in ("yv12", "p010"):
        return 98, 132
    if name in ("yuy2", "uyvy", "yvyu"):
        return 97, 132
    return 97, 131


def make_frame(name, seed=0, hw=None, **kw):
    """A CPU frame of layout ``name`` with random samples; ``kw``: chroma, siting, transfer, peak_nits, matrix,
    full_range as the frame classes take them."""
    h, w = hw or frame_hw(name)
    g = _gen(name, h, w, seed)
    ch2, cw2 = (h + 1) // 2, (w + 1) // 2
    if name in ("nv12", "nv21"):
        return Nv12(_u8(g, h, w), _u8(g, ch2, cw2, 2), vu=name == "nv21", **kw)
    if name == "i420":
        return Yuv420p(_u8(g, h, w), _u8(g, ch2, cw2), _u8(g, ch2, cw2), **kw)
    if name == "yv12":
        return Yuv420p.from_buffer(_u8(g, h * w + 2 * (h // 2) * (w // 2)), h, w, order="yv12", **kw)
    if name == "i422":
        return surfaces.YuvPlanar(_u8(g, h, w), _u8(g, h, cw2), _u8(g, h, cw2), "422", **kw)
    if name == "i444":
        return surfaces.YuvPlanar(_u8(g, h, w), _u8(g, h, w), _u8(g, h, w), "444", **kw)
    if name == "nv16":
        return surfaces.YuvSemiPlanar(_u8(g, h, w), _u8(g, h, cw2, 2), "422", **kw)
    if name in ("yuy2", "uyvy", "yvyu"):
        return surfaces.Yuyv(_u8(g, h, 4 * cw2), w, surfaces._YUYV[name], **kw)
    if name == "p010":      # all 16 bits random: the code is the high 10, the rest is ignored
        return surfaces.from_buffer("p010", _u8(g, 2 * (h * w + (h // 2) * w)), h, w, **kw)
    if name == "i010":
        y, u, v = _words(g, 10, h, w), _words(g, 10, ch2, cw2), _words(g, 10, ch2, cw2)
        return surfaces.YuvPlanar(y, u, v, "420", 10, **kw)
    if name == "i422p12":
        return surfaces.YuvPlanar(_words(g, 12, h, w), _words(g, 12, h, cw2), _words(g, 12, h, cw2), "422", 12, **kw)
    if name == "i444p12":
        return surfaces.YuvPlanar(_words(g, 12, h, w), _words(g, 12, h, w), _words(g, 12, h, w), "444", 12, **kw)
    raise KeyError(name)


def corner_origins(h, w, tile_hw=TILE_HW):
    """Four tiles: the first at the frame's first row and column, the last on its last; ``(0, 59)`` and ``(41, 0)``
    give an odd ``y0`` and ``x0 = 3 (mod 4)``."""
    return [(0, 0), (0, 59), (41, 0), (h - tile_hw[0], w - tile_hw[1])]


def reference(frame, origins, tile_hw=TILE_HW, out_hw=OUT_HW, want_pixels=True):
    """The yardstick: the packed tile launch on the frame's ``rgb()``."""
    return I.tiled_patch_planes(frame.rgb(), "rgb", origins, tile_hw, out_hw, P, MEAN, STD, want_pixels)


def same(got, want):
    """planes and pixels bit for bit"""
    return torch.equal(got[0], want[0]) and (got[1] is None) == (want[1] is None) and \
        (got[1] is None or torch.equal(got[1], want[1]))


def cropped(frame, y0, x0, th, tw):
    """The tile at an even ``(y0, x0)`` of a 4:2:0 / 4:2:2 frame as a frame of its own: the cropped planes, so that
    chroma interpolation clamps at the tile's edge. (What a tile launch must *not* compute.)"""
    assert y0 % 2 == 0 and x0 % 2 == 0
    from dataclasses import replace
    if isinstance(frame, surfaces.Yuyv):
        return replace(frame, data=frame.data[..., y0:y0 + th, 2 * x0:2 * x0 + 4 * ((tw + 1) // 2)], width=tw)
    vs = 1 if getattr(frame, "subsampling", "420") == "420" else 0
    cy0, cy1, cx0, cx1 = y0 >> vs, (y0 + th + vs) >> vs, x0 >> 1, (x0 + tw + 1) >> 1
    new = {"y": frame.y[..., y0:y0 + th, x0:x0 + tw]}
    for k in frame.PLANES[1:]:
        pl = getattr(frame, k)
        new[k] = pl[..., cy0:cy1, cx0:cx1, :] if k == "uv" else pl[..., cy0:cy1, cx0:cx1]
    return replace(frame, **new)
