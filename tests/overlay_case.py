"""The yardstick of the overlay tests (``test_overlay.py`` on the CPU, ``test_gpu_overlay.py`` on the GPU): the drawing
rule of ``ops.image.overlay`` as plain Python loops over ints and Python floats, per pixel, with its own copy of the ten
glyphs as ASCII art; the surfaces the tests paint, laid out here byte by byte inside a larger allocation; and the scenes
both files run. It shares no code with ``ops/image.py``.

Every comparison is equality of the whole storage: the allocation is filled with seeded random bytes, the code under
test paints into a surface inside it, and :func:`expected` rewrites, in a copy of those bytes, exactly the samples the
rule paints — so pitch padding, the bytes around the surface, the alpha byte of a four-byte pixel and the parent of a
crop must all come back as they were. There are no tolerances.

The rule (``slots``): row ``r`` is drawn when ``r < clamp(count, 0, N)``, its score is above 0 (a NaN is not), its label
lies in ``[0, L)`` with mode 1 or 2, its four coordinates are finite, with ids its id is positive and its hits reach
``min_hits``, and its rectangle is not empty. Coordinates are clamped to ``+-2^20``; pixel ``i`` covers ``[i, i + 1)``, so
the rectangle is columns ``floor(x0) .. ceil(x1) - 1`` and rows ``floor(y0) .. ceil(y1) - 1``. Mode 2 fills it with the
redact colour (slot ``2 K``). Mode 1 paints it minus the rectangle ``t`` further in, in fill colour ``2 (key mod K)``, and
with ``s > 0`` a tag of ``(6 nd + 1) s x 9 s`` pixels at the box's first column, above the box when it fits the frame
and else from the box's first row: the ``nd`` decimal digits of ``key mod 10^6`` in cells ``6 s`` wide behind a margin of
``s``, set bits in the text colour (the fill's slot plus one), everything else in the fill colour. The lowest row wins a
pixel. A sample ``(cy, cx)`` of a plane subsampled by ``(vs, hs)`` is written when luma pixel ``(cy << vs, cx << hs)``
is painted, with that pixel's colour, as ``code << shift`` in one byte or one little-endian 16-bit word."""
import math
import struct
from dataclasses import dataclass, field
from typing import List, Optional

import torch

GLYPHS = {
    0: (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    1: ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    2: (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    3: ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    4: ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    5: ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    6: ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    7: ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    8: (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    9: (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
}
BIG = float(1 << 20)
#: the kernel's raster tile (rows, columns): the frame sizes of the tests lie around it
TILE = (32, 64)


def f32(v: float) -> float:
    """``v`` rounded to fp32, as the lists hold it."""
    return struct.unpack("f", struct.pack("f", v))[0] if math.isfinite(v) else v


def ulp_up(v: float) -> float:
    """The next fp32 above a positive ``v``."""
    return struct.unpack("f", struct.pack("I", struct.unpack("I", struct.pack("f", v))[0] + 1))[0]


@dataclass
class Scene:
    """One frame's lists, as long as their allocation (every row behind ``N`` is drawable too), the ``N`` rows the
    code under test is handed as views, ``count`` as it stands on the device, and the parameters."""
    name: str
    scores: List[float]
    labels: List[int]
    boxes: List[List[float]]
    ids: Optional[List[int]] = None
    hits: Optional[List[int]] = None
    N: Optional[int] = None
    count: Optional[int] = None
    t: int = 1
    s: int = 0
    modes: List[int] = field(default_factory=lambda: [1, 1, 2, 0, 1, 1, 1, 1])
    min_hits: int = 1
    K: int = 16

    def __post_init__(self):
        self.N = len(self.scores) if self.N is None else self.N
        self.count = self.N if self.count is None else self.count
        self.boxes = [[f32(c) for c in b] for b in self.boxes]
        self.scores = [f32(v) for v in self.scores]

    def tensors(self, device="cpu"):
        """``(count, scores, labels, boxes, ids, hits)``: fp32 / int32 views ``[:N]`` of the whole allocations."""
        i32 = torch.int32
        t = [torch.tensor([self.count], dtype=i32), torch.tensor(self.scores, dtype=torch.float32)[:self.N],
             torch.tensor(self.labels, dtype=i32)[:self.N],
             torch.tensor(self.boxes, dtype=torch.float32).reshape(-1, 4)[:self.N]]
        t += [None, None] if self.ids is None else [torch.tensor(self.ids, dtype=i32)[:self.N],
                                                     torch.tensor(self.hits, dtype=i32)[:self.N]]
        return [v if v is None else v.to(device) for v in t]


def slots(sc: Scene, h: int, w: int) -> List[List[int]]:
    """The colour slot of every pixel of an ``h x w`` frame under the rule, -1 where nothing is drawn."""
    out = [[-1] * w for _ in range(h)]
    n = min(max(sc.count, 0), sc.N)
    L, t, s = len(sc.modes), sc.t, sc.s
    for r in range(n - 1, -1, -1):          # the last row first: a lower row paints over it
        if not sc.scores[r] > 0:
            continue
        label = sc.labels[r]
        if not 0 <= label < L or sc.modes[label] not in (1, 2):
            continue
        key = label
        if sc.ids is not None:
            key = sc.ids[r]
            if key <= 0 or sc.hits[r] < sc.min_hits:
                continue
        if not all(math.isfinite(c) for c in sc.boxes[r]):
            continue
        x0, y0, x1, y1 = (min(max(c, -BIG), BIG) for c in sc.boxes[r])
        bx0, by0, bx1, by1 = math.floor(x0), math.floor(y0), math.ceil(x1) - 1, math.ceil(y1) - 1
        if bx1 < bx0 or by1 < by0:
            continue
        if sc.modes[label] == 2:
            for y in range(max(by0, 0), min(by1, h - 1) + 1):
                for x in range(max(bx0, 0), min(bx1, w - 1) + 1):
                    out[y][x] = 2 * sc.K
            continue
        fill = 2 * (key % sc.K)
        for y in range(max(by0, 0), min(by1, h - 1) + 1):
            for x in range(max(bx0, 0), min(bx1, w - 1) + 1):
                if not (bx0 + t <= x <= bx1 - t and by0 + t <= y <= by1 - t):
                    out[y][x] = fill
        if s > 0:
            digits = [int(ch) for ch in str(key % 1000000)]
            tw, th = (6 * len(digits) + 1) * s, 9 * s
            top = by0 - th if by0 - th >= 0 else by0
            for y in range(max(top, 0), min(top + th, h)):
                for x in range(max(bx0, 0), min(bx0 + tw, w)):
                    gu, gv = x - bx0 - s, y - top - s
                    colour = fill
                    if 0 <= gu < 6 * s * len(digits) and 0 <= gv < 7 * s:
                        cu = (gu % (6 * s)) // s
                        if cu < 5 and GLYPHS[digits[gu // (6 * s)]][gv // s][cu] == "#":
                            colour = fill + 1
                    out[y][x] = colour
    return out


# ---- surfaces, byte by byte ---------------------------------------------------------------------------------------------
@dataclass
class Plane:
    """One component's samples in the storage: the sample of ``(cy, cx)`` is the ``sb`` bytes at ``off + cy * pitch +
    cx * step``; it belongs to luma pixel ``(cy << vs, cx << hs)`` and holds colour component ``comp``."""
    off: int
    pitch: int
    step: int
    sb: int
    comp: int
    hs: int = 0
    vs: int = 0
    shift: int = 0


#: name -> what it is. Packed: (bytes per pixel, the bytes of R, G, B). YUV: (layout, hs, vs, depth, msb, order).
PACKED = {"rgb": (3, (0, 1, 2)), "bgr": (3, (2, 1, 0)), "rgba": (4, (0, 1, 2)), "bgra": (4, (2, 1, 0)),
          "crop": (4, (2, 1, 0))}
YUV = {
    "nv12": ("semi", 1, 1, 8, False, 0), "nv21": ("semi", 1, 1, 8, False, 1),
    "i420": ("planar", 1, 1, 8, False, 0), "yv12": ("planar", 1, 1, 8, False, 1),
    "i422": ("planar", 1, 0, 8, False, 0), "i444": ("planar", 0, 0, 8, False, 0),
    "i010": ("planar", 1, 1, 10, False, 0), "p010": ("semi", 1, 1, 10, True, 0),
    "nv16": ("semi", 1, 0, 8, False, 0), "nv24": ("semi", 0, 0, 8, False, 0),
    "yuy2": ("yuyv", 1, 0, 8, False, 0), "uyvy": ("yuyv", 1, 0, 8, False, 1), "yvyu": ("yuyv", 1, 0, 8, False, 2),
}
LAYOUTS = tuple(PACKED) + tuple(YUV)
SUBSAMPLED = tuple(n for n, v in YUV.items() if v[1])
_YUYV = {0: ("yuyv", 0, 1, 3), 1: ("uyvy", 1, 0, 2), 2: ("yvyu", 0, 3, 1)}
LEAD, TAIL, PAD = 38, 54, 10        # bytes before and behind the surface, and of padding in every row (all even)


@dataclass
class Surface:
    name: str
    h: int
    w: int
    storage: torch.Tensor           # uint8, 1-D: the whole allocation
    target: object                  # what ``overlay`` is handed
    planes: List[Plane]
    depth: int = 8


def _view(storage, off, shape, strides, sb):
    """A strided view of samples of ``sb`` bytes at byte ``off`` (strides in bytes)."""
    base = storage if sb == 1 else storage.view(torch.uint16)
    return base.as_strided(shape, tuple(st // sb for st in strides), off // sb)


def surface(name: str, h: int, w: int, seed: int = 0, device="cpu", matrix: str = "bt601", full_range: bool = False):
    """Layout ``name`` of ``h x w`` inside an allocation of seeded random bytes: pitched rows, ``LEAD`` bytes before the
    first and ``TAIL`` behind the last plane."""
    from walkai_nos_amd.models.workload import processor as P, surfaces as S
    g = torch.Generator().manual_seed(1000 + seed)

    def alloc(n):
        return torch.randint(0, 256, (LEAD + n + TAIL,), generator=g, dtype=torch.uint8).to(device)
    if name in PACKED:
        C, rgb = PACKED[name]
        if name == "rgb":       # contiguous, behind an odd offset
            st = alloc(h * w * 3 + 1)
            off = LEAD + 1
            return Surface(name, h, w, st, _view(st, off, (h, w, 3), (w * 3, 3, 1), 1),
                           [Plane(off + c, w * 3, 3, 1, k) for k, c in enumerate(rgb)])
        # the crop: rows 3.. and columns 1.. of a parent 5 rows and 4 columns larger
        ph, pw, y0, x0 = (h + 5, w + 4, 3, 1) if name == "crop" else (h, w, 0, 0)
        pitch = pw * C + PAD + 1
        st = alloc(ph * pitch)
        parent = _view(st, LEAD + 1, (ph, pw, C), (pitch, C, 1), 1)
        off = LEAD + 1 + y0 * pitch + x0 * C
        return Surface(name, h, w, st, P.Packed(parent[y0:y0 + h, x0:x0 + w], "bgra" if name == "crop" else name),
                       [Plane(off + c, pitch, C, 1, k) for k, c in enumerate(rgb)])
    layout, hs, vs, depth, msb, order = YUV[name]
    sb = 1 if depth == 8 else 2
    shift = 16 - depth if msb else 0
    ch, cw = (h + (1 << vs) - 1) >> vs, (w + (1 << hs) - 1) >> hs
    sub = {(1, 1): "420", (1, 0): "422", (0, 0): "444"}[(hs, vs)]
    kw = dict(matrix=matrix, full_range=full_range)
    if layout == "yuyv":
        row = 4 * ((w + 1) // 2)
        pitch = row + PAD
        st = alloc(h * pitch)
        oname, yo, uo, vo = _YUYV[order]
        data = _view(st, LEAD, (h, row), (pitch, 1), 1)
        return Surface(name, h, w, st, S.Yuyv(data, w, oname, **kw),
                       [Plane(LEAD + yo, pitch, 2, 1, 0), Plane(LEAD + uo, pitch, 4, 1, 1, 1, 0),
                        Plane(LEAD + vo, pitch, 4, 1, 2, 1, 0)])
    ypitch = w * sb + PAD
    if layout == "semi":
        cpitch = 2 * cw * sb + PAD
        st = alloc(h * ypitch + ch * cpitch)
        yoff, coff = LEAD, LEAD + h * ypitch
        y = _view(st, yoff, (h, w), (ypitch, sb), sb)
        uv = _view(st, coff, (ch, cw, 2), (cpitch, 2 * sb, sb), sb)
        planes = [Plane(yoff, ypitch, sb, sb, 0, 0, 0, shift),
                  Plane(coff + order * sb, cpitch, 2 * sb, sb, 1, hs, vs, shift),
                  Plane(coff + (1 - order) * sb, cpitch, 2 * sb, sb, 2, hs, vs, shift)]
        if name in ("nv12", "nv21"):
            target = P.Nv12(y, uv, vu=bool(order), **kw)
        else:
            target = S.YuvSemiPlanar(y, uv, sub, depth, msb, vu=bool(order), **kw)
        return Surface(name, h, w, st, target, planes, depth)
    cpitch = cw * sb + PAD
    st = alloc(h * ypitch + 2 * ch * cpitch)
    yoff, first, second = LEAD, LEAD + h * ypitch, LEAD + h * ypitch + ch * cpitch
    uoff, voff = (second, first) if order else (first, second)          # yv12: V lies first
    y, u, v = (_view(st, o, shape, (p, sb), sb) for o, shape, p in
               ((yoff, (h, w), ypitch), (uoff, (ch, cw), cpitch), (voff, (ch, cw), cpitch)))
    planes = [Plane(yoff, ypitch, sb, sb, 0, 0, 0, shift), Plane(uoff, cpitch, sb, sb, 1, hs, vs, shift),
              Plane(voff, cpitch, sb, sb, 2, hs, vs, shift)]
    if name in ("i420", "yv12"):
        target = P.Yuv420p(y, u, v, **kw)
    else:
        target = S.YuvPlanar(y, u, v, sub, depth, msb, **kw)
    return Surface(name, h, w, st, target, planes, depth)


def expected(storage: bytes, planes: List[Plane], slot: List[List[int]], codes: List[List[int]]) -> bytes:
    """``storage`` with exactly the samples the rule paints rewritten."""
    out = bytearray(storage)
    h, w = len(slot), len(slot[0])
    for p in planes:
        for cy in range((h + (1 << p.vs) - 1) >> p.vs):
            row = slot[cy << p.vs]
            for cx in range((w + (1 << p.hs) - 1) >> p.hs):
                s = row[cx << p.hs]
                if s >= 0:
                    at = p.off + cy * p.pitch + cx * p.step
                    out[at:at + p.sb] = (codes[s][p.comp] << p.shift).to_bytes(p.sb, "little")
    return bytes(out)


def check(surf: Surface, before: bytes, slot, codes) -> int:
    """The whole allocation against :func:`expected`; the number of bytes the painting changed."""
    want = expected(before, surf.planes, slot, codes)
    got = bytes(surf.storage.cpu().numpy().tobytes())
    if got != want:
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        raise AssertionError(f"{surf.name} {surf.h}x{surf.w}: {len(bad)} bytes differ, the first at {bad[0]} "
                             f"(got {got[bad[0]]}, want {want[bad[0]]}, was {before[bad[0]]}); "
                             f"planes {[(p.off, p.pitch) for p in surf.planes]}")
    return sum(1 for a, b in zip(before, want) if a != b)


def run(I, paint, surf: Surface, sc: Scene, slot=None) -> int:
    """``paint`` (``I.overlay`` or ``I.overlay_reference``) on ``surf`` with scene ``sc``, checked."""
    dev = surf.storage.device
    codes = I.overlay_codes(I.overlay_palette(sc.K), (9, 200, 31), surf.target)
    before = bytes(surf.storage.cpu().numpy().tobytes())
    count, scores, labels, boxes, ids, hits = sc.tensors(dev)
    paint(surf.target, count, scores, labels, boxes, ids, hits, thickness=sc.t, scale=sc.s,
          modes=torch.tensor(sc.modes, dtype=torch.uint8).to(dev), min_hits=sc.min_hits, codes=codes)
    return check(surf, before, slots(sc, surf.h, surf.w) if slot is None else slot, codes.cpu().tolist())


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _scene(name, boxes, labels=None, scores=None, **kw):
    n = len(boxes)
    return Scene(name, scores or [0.9] * n, labels or [k % 2 for k in range(n)], boxes, **kw)


def edge_scene(h, w, t=1):
    """A box outside the frame on each side, one straddling each edge and each corner, one larger than the frame."""
    a, b = max(h // 3, 1), max(w // 3, 1)
    boxes = [[-9.5, 1, -2.25, a], [w + 1.5, 1, w + 8, a], [1, -7, b, -0.5], [1, h + 0.25, b, h + 6],          # outside
             [-3.5, a, 2.5, 2 * a], [w - 2.5, a, w + 4, 2 * a], [b, -2, 2 * b, 2.75], [b, h - 2.5, 2 * b, h + 3],
             [-2, -2, 2.5, 2.5], [w - 3, -3, w + 2, 3], [-3, h - 3, 3, h + 3], [w - 2.5, h - 2.5, w + 9, h + 9],
             [-5, -4, w + 6, h + 3]]
    return _scene(f"edges-t{t}", boxes, labels=[0, 1, 4, 5] * 3 + [6], t=t)


def degenerate_scene(h, w):
    """One pixel, zero and negative extent, NaN, infinities and 1e30, ``x1`` an integer and one ulp above it."""
    nan, inf = float("nan"), float("inf")
    m = min(h, w)
    boxes = [[1.25, 1.5, 1.75, 1.875],                              # one pixel
             [3, 3, 3, 9], [5, 4, 4, 9], [6.5, 5, 9, 5], [6, 9, 9, 2],    # no or negative extent: nothing
             [nan, 0, 5, 5], [0, 0, 5, nan], [0, -inf, 5, 5], [0, 0, inf, 5], [-inf, -inf, inf, inf],
             [-1e30, 0.5 * h, 1e30, 0.5 * h + 1.5], [0.25 * w, -1e30, 0.25 * w + 2, 1e30],  # finite: clamped, drawn
             [0, m - 2.0, 4.0, m - 1.0], [6, m - 2.0, ulp_up(10.0), m - 1.0],        # columns 0..3, and 6..10
             [0.999999, 0.0, 1.0, 1.0]]
    return _scene("degenerate", boxes, labels=[0, 1, 4, 5, 6] * 3)


def thickness_scenes(h, w):
    box = [[1, 1, min(w - 1, 13), min(h - 1, 11)], [min(w, 16), 0, min(w, 16) + 6.5, 5.5]]
    return [_scene(f"thickness-{t}", box, t=t) for t in (1, 2, 3, 5, 6, 40)]


def tag_scenes(h, w):
    out = []
    for s in (0, 1, 3):
        ids = [7, 305, 16, 123456, 1234567, 1000000, 42, 90]
        boxes = [[2, 1, 20, 8],                         # no room above: the tag inside, from the first row
                 [4, 9 * s + 3, 30, 9 * s + 12],        # room above
                 [-4.5, 9 * s + 20, 6, 9 * s + 26],     # clipped at the left edge
                 [w - 9, 9 * s + 4, w + 3, 9 * s + 10], [w - 20, h - 12, w - 2, h - 3],     # clipped at the right
                 [w // 2, h // 2, w // 2 + 3, h // 2 + 2],    # a tag larger than its box: v = 0
                 [30, 9 * s, 34, 9 * s + 4],            # by0 - TH == 0: just fits above
                 [40, 9 * s - 1, 47, 9 * s + 5]]        # one row short
        out.append(Scene(f"tags-s{s}", [0.9] * 8, [0, 1, 4, 5, 6, 7, 0, 1], boxes, ids=ids, hits=[3] * 8, s=s, t=2))
    # without ids the key is the label: label 0 tags "0"
    out.append(_scene("tags-by-label", [[3, 12, 25, 25], [28, 12, 45, 25]], labels=[0, 7], s=1))
    return out


def priority_scene(h, w):
    """Three overlapping boxes, a tag over another row's outline, a redacted box over and under an outlined one."""
    boxes = [[4, 12, 20, 24], [10, 16, 28, 30], [1, 20, 16, 31],
             [30, 11, 44, 20],                  # its tag, rows 2..10, lies over the next row's outline
             [28, 1, 50, 14],
             [2, 1, 12, 9], [6, 4, 18, 11],     # redacted (label 2) over outlined
             [52, 2, 62, 12], [48, 6, 58, 16]]  # outlined over redacted
    return _scene("priority", boxes, labels=[0, 1, 4, 5, 6, 2, 1, 4, 2], s=1, t=1)


def filter_scene(h, w, with_ids):
    nan = float("nan")
    boxes = [[1 + 6 * k, 2, 5.5 + 6 * k, 8] for k in range(10)]
    scores = [nan, 0.0, -0.5, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 1e-30]
    labels = [0, 0, 0, -1, 8, 3, 1, 1, 1, 4]      # 8 = L: outside; 3: mode 0
    if not with_ids:
        return Scene("filters", scores, labels, boxes)
    return Scene("filters-ids", scores, labels, boxes, ids=[1, 2, 3, 4, 5, 6, 0, 9, 11, 12],
                 hits=[5, 5, 5, 5, 5, 5, 5, 2, 3, 3], min_hits=3)


def odd_scene(h, w):
    """Boxes at odd origins and of odd sizes: on a subsampled surface the chroma rule decides."""
    boxes = [[1, 1, 4, 4], [7, 3, 12, 6], [15, 1, 16, 8], [1, 9, 10, 10], [19, 5, 26, 12], [29, 1, 30, 2]]
    return _scene("odd", boxes, labels=[0, 2, 1, 4, 2, 5], t=1)


def lattice_scene(N, h, w, seed=0, total=None, count=None, s=1):
    """``total`` (default ``N``) drawable rows on a lattice with seeded jitter, ids and hits; the first ``N`` handed in."""
    g = torch.Generator().manual_seed(77 + seed)
    total = N if total is None else total
    r = torch.rand(total, 4, generator=g).tolist()
    cols = max(1, w // 12)
    boxes = []
    for k, (a, b, c, d) in enumerate(r):
        x, y = (k % cols) * 12 + 6 * a - 3, ((k // cols) * 7) % max(h, 1) + 6 * b - 3
        boxes.append([x, y, x + 3 + 9 * c, y + 2 + 8 * d])
    labels = [(5 * k) % 8 for k in range(total)]
    name = f"lattice-N{N}" + ("" if count is None else f"-count{count}")
    return Scene(name, [0.5 + 0.4 * v[0] for v in r], labels, boxes, ids=[3 * k + 1 for k in range(total)],
                 hits=[1 + (k + 1) % 4 for k in range(total)], N=N, count=count, s=s, t=1, min_hits=2)


ROWS = (1, 64, 65, 100, 1024)


def count_scenes(h, w):
    """``count`` at 0, 1 and ``N``, above ``N`` and negative, over views of allocations of 90 drawable rows."""
    return [lattice_scene(65, h, w, seed=3, total=90, count=c) for c in (0, 1, 65, 80, 100000, -4)]


def scenes(h, w):
    """Every scene but the row counts."""
    return ([edge_scene(h, w, 1), edge_scene(h, w, 2), degenerate_scene(h, w), priority_scene(h, w), odd_scene(h, w),
             filter_scene(h, w, False), filter_scene(h, w, True)] + thickness_scenes(h, w) + tag_scenes(h, w))


#: frames around the raster tile, 2 x 2, and (packed layouts only) odd sizes
SIZES = (TILE, (TILE[0] + 2, TILE[1] + 2), (2 * TILE[0] + 2, 2 * TILE[1] + 2), (2, 2))
ODD_SIZE = (TILE[0] + 1, TILE[1] + 1)
