"""The general YUV front end on the GPU (``csrc/image.hip``'s ``stage_yuv`` behind ``nos_image_patch_planes_yuv``):
4:2:2, 4:4:4, packed 4:2:2 and 10 / 12-bit surfaces, each fused launch against the RGB kernel on the frame converted
on the CPU by the definition (``ops.image.yuv_to_rgb``, itself checked against the standards in
``test_surfaces.py``). The conversion is defined in integers and everything behind the staging loop is the RGB
kernel's code, so planes and pixels are compared with ``torch.equal`` — no tolerance. Each case is the smallest
size that reaches its branch (patch 16 unless said otherwise, seeded random planes, random ignored bits in every
16-bit word). Bounds are shown by results that do not depend on the pad bytes around a plane and by planes that end
on their storage's last byte, never by a fault."""
import ctypes
import json
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
P = 16
#: one name per kernel instantiation and runtime field value ...
LAYOUTS = ("i422", "i444", "nv61", "nv24", "yuy2", "uyvy", "p010", "i010", "p210", "i410", "i012")
#: ... and the names that share one of those instantiations
SHARED = ("yv16", "yv24", "nv16", "nv42", "yvyu", "p012", "p410", "i210")

#: (source h, w, target H, W, fused?)
CASES = ((48, 64, 80, 96, True),        # upscale: footprints start on odd rows and columns
         (37, 53, 80, 112, True),       # odd sizes: the last chroma column serves one luma column; w % 4 == 1
         (120, 160, 48, 64, True),      # scale 2.5
         (256, 256, 64, 64, True),      # scale 4, the widest footprint (69 columns: 18 groups of 4)
         (260, 260, 64, 64, False))     # past the limit: the fallback, still equal
IDS = ["{}x{}".format(*c[:2]) for c in CASES]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from walkai_nos_amd.ops import image, kernels
    assert kernels.hip_available(), "libnos_kernels.so must be built on a GPU box"
    assert image.hip_available(), "libnos_image.so must be built on a GPU box"
    kernels.set_backend("hip")
    kernels.set_fp32_matmul("x3")
    kernels.set_slice_cus(None)
    yield kernels
    kernels.set_backend("hip")
    kernels.set_fp32_matmul("x3")
    kernels.set_slice_cus(None)


@pytest.fixture(scope="module")
def I(K):
    from walkai_nos_amd.ops import image
    return image


@pytest.fixture(scope="module")
def S(I):
    from walkai_nos_amd.models.workload import surfaces
    return surfaces


class Counter:
    def __init__(self, monkeypatch, owner, name):
        self.n = 0
        fn = getattr(owner, name)

        def spy(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        monkeypatch.setattr(owner, name, spy)


def words(codes, depth, msb, g, noise=True):
    """int32 codes as little-endian 16-bit words in bytes ``[..., 2 * n]``: the value in the high (``msb``) or the
    low bits, the other bits random (``noise``) or zero."""
    junk = torch.randint(0, 1 << (16 - depth), codes.shape, generator=g, dtype=torch.int32) * int(noise)
    w = (codes << (16 - depth)) | junk if msb else codes | (junk << depth)
    return torch.stack((w & 255, w >> 8), dim=-1).to(torch.uint8).flatten(-2)


class Picture:
    """One seeded picture of a chroma geometry and sample depth (CPU codes), and every layout of it: ``planes(name)``
    are the CPU planes of format ``name`` as bytes ``[B, rows, rowbytes]``, ``rgb`` the contiguous RGB frame all of
    them convert to (by the definition, from planes without any ignored bit set)."""

    def __init__(self, I, S, sub, depth, h, w, batch=1, seed=0):
        self.g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w + 31 * depth + int(sub))
        hs, vs = I.YUV_SUBSAMPLING[sub]
        ch, cw = (h + (1 << vs) - 1) >> vs, (w + (1 << hs) - 1) >> hs
        self.I, self.S, self.sub, self.depth, self.h, self.w, self.B = I, S, sub, depth, h, w, batch
        self.y, self.u, self.v = (torch.randint(0, 1 << depth, (batch,) + s, generator=self.g, dtype=torch.int32)
                                  for s in ((h, w), (ch, cw), (ch, cw)))
        self.pad = torch.randint(0, 256, (batch, h, 1), generator=self.g, dtype=torch.int32)
        typed = [t.to(torch.uint8) if depth == 8 else t.to(torch.int16) for t in (self.y, self.u, self.v)]
        self.rgb = I.yuv_to_rgb(*typed, sub, depth, False)

    @classmethod
    def of(cls, I, S, name, h, w, batch=1, seed=0):
        return cls(I, S, S.FORMATS[name][1], S.FORMATS[name][2], h, w, batch, seed)

    def planes(self, name, noise=True):
        kind, sub, depth, msb, swap = self.S.FORMATS[name]
        assert (sub, depth) == (self.sub, self.depth)
        if kind == "packed":
            yo, uo, vo = self.I.YUYV_ORDERS[{"yuy2": "yuyv"}.get(name, name)]
            cw = (self.w + 1) // 2
            data = torch.zeros(self.B, self.h, 4 * cw, dtype=torch.int32)
            y = torch.cat((self.y, self.pad), dim=2)[..., :2 * cw]      # an odd width: a luma that is never shown
            data[..., yo::2], data[..., uo::4], data[..., vo::4] = y, self.u, self.v
            return [data.to(torch.uint8)]
        enc = (lambda t: t.to(torch.uint8)) if depth == 8 else (lambda t: words(t, depth, msb, self.g, noise))
        if kind == "planar":
            return [enc(self.y), enc(self.u), enc(self.v)]             # by what they hold, whatever the name's order
        pair = (self.v, self.u) if swap else (self.u, self.v)
        return [enc(self.y), enc(torch.stack(pair, dim=-1).flatten(2))]


def frame(S, name, views, w, **kw):
    """The frame of format ``name`` over its GPU planes as bytes ``[B, rows, rowbytes]`` (views of any pitch)."""
    kind, sub, depth, msb, swap = S.FORMATS[name]
    if kind == "packed":
        return S.Yuyv(views[0], w, {"yuy2": "yuyv"}.get(name, name), **kw)
    typed = [v if depth == 8 else v.view(torch.uint16) for v in views]
    if kind == "planar":
        return S.YuvPlanar(*typed, sub, depth, msb, **kw)
    return S.YuvSemiPlanar(typed[0], typed[1].unflatten(2, (-1, 2)), sub, depth, msb, vu=swap, **kw)


def run(S, name, views, w, out, patch=P, want_pixels=False):
    return frame(S, name, views, w).patch_planes(out, patch, MEAN, STD, want_pixels)


_want = {}


def yardstick(I, pic, out, key=None, patch=P):
    """The RGB kernel on the converted frame (converted on the CPU): ``(planes, pixels)`` on the GPU, computed once
    per ``key`` and left unchanged."""
    if key is not None:
        key = (key, pic.sub, pic.depth)
    if key is None or key not in _want:
        res = I.image_patch_planes(pic.rgb.cuda(), out, patch, MEAN, STD, want_pixels=True)
        if key is None:
            return res
        _want[key] = res
    return _want[key]


def same(S, name, views, w, out, want, patch=P):
    got, px = run(S, name, views, w, out, patch, want_pixels=True)
    only, none = run(S, name, views, w, out, patch)
    torch.cuda.synchronize()
    assert none is None and got.dtype == torch.bfloat16 and px.dtype == torch.float32
    assert torch.equal(px, want[1]), f"{name}: pixels"
    assert torch.equal(got, want[0]) and torch.equal(only, want[0]), f"{name}: planes"


def pitched(plane, pitch, pad, lead=0, tail=0, bstride=None):
    """``plane`` ``[B, rows, rowbytes]`` copied into a fresh GPU allocation with ``pitch`` bytes between rows,
    ``lead`` bytes before the first and ``tail`` after the last row's bytes, every other byte ``pad``; the view."""
    B, rows, rb = plane.shape
    per = (rows - 1) * pitch + rb if bstride is None else bstride
    buf = torch.full((lead + (B - 1) * per + (rows - 1) * pitch + rb + tail,), pad, dtype=torch.uint8, device="cuda")
    view = buf.as_strided((B, rows, rb), (per, pitch, 1), lead)
    view.copy_(plane)
    return view


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("name", LAYOUTS)
def test_layout_equals_the_rgb_kernel_on_the_converted_frame(K, I, S, monkeypatch, name, case):
    h, w, H, W, fused = case
    pic = Picture.of(I, S, name, h, w)
    want = yardstick(I, pic, (H, W), key=case)
    views = [t.cuda() for t in pic.planes(name)]
    fallback = Counter(monkeypatch, I, "yuv_to_rgb")
    same(S, name, views, w, (H, W), want)
    assert fallback.n == (0 if fused else 2)


@pytest.mark.parametrize("name", SHARED)
def test_names_that_share_an_instantiation(K, I, S, monkeypatch, name):
    pic = Picture.of(I, S, name, 37, 53)
    want = yardstick(I, pic, (80, 112), key=CASES[1])
    fallback = Counter(monkeypatch, I, "yuv_to_rgb")
    same(S, name, [t.cuda() for t in pic.planes(name)], 53, (80, 112), want)
    assert fallback.n == 0


@pytest.mark.parametrize("w", (5, 6, 7))
def test_the_last_column_group_straddles_the_row_end(K, I, S, w):
    for name in ("i444", "yuy2", "p010"):
        pic = Picture.of(I, S, name, 3, w, batch=2, seed=1)
        same(S, name, [t.cuda() for t in pic.planes(name)], w, (16, 16), yardstick(I, pic, (16, 16)))


def test_pitches_alignment_and_storage_ends(K, I, S, monkeypatch):
    # one 8-bit and one 16-bit format of each layout value (packed is 8-bit only)
    out = (80, 112)
    pics = {name: Picture.of(I, S, name, 37, 53, batch=2, seed=2) for name in ("i422", "i010", "nv24", "p210", "yuy2")}
    fallback = Counter(monkeypatch, I, "yuv_to_rgb")
    for name, pic in pics.items():
        want = yardstick(I, pic, out)
        assert not torch.equal(want[1][0], want[1][1])
        cpu = pic.planes(name)
        wide = S.FORMATS[name][2] != 8
        # per plane a pitch of its own (odd for bytes, even for words); the first byte 1, 2, 3 bytes into the storage
        # (words: 2 bytes, which is 2-aligned and not 4-aligned); trailing slack, and none (the plane's last byte is
        # the storage's last byte, the first its first)
        for leads, extra, tail in (((1, 2, 3), (11, 5, 9), 5), ((2, 3, 1), (1, 3, 7), 1), ((3, 1, 2), (0, 0, 0), 0),
                                   ((0, 0, 0), (0, 0, 0), 0), ((0, 0, 0), (3, 1, 5), 0)):
            if wide:
                leads, extra, tail = tuple(2 if ld else 0 for ld in leads), tuple(2 * e for e in extra), 2 * tail
            results = []
            for pad in (0x00, 0xFF):
                views = [pitched(t, t.shape[2] + e if wide else (t.shape[2] + e) | (1 if e else 0), pad, ld, tail)
                         for t, ld, e in zip(cpu, leads, extra)]
                for v, ld in zip(views, leads):
                    s = v.untyped_storage()
                    assert v.data_ptr() - s.data_ptr() == ld and (not wide or v.data_ptr() % 4 == ld)
                    if tail == 0:
                        last = v.data_ptr() + (v.shape[0] - 1) * v.stride(0) + (v.shape[1] - 1) * v.stride(1) + v.shape[2]
                        assert last == s.data_ptr() + s.nbytes()
                if len(views) == 3 and any(extra):
                    assert len({v.stride(1) for v in views[1:]}) == 2       # U's pitch is not V's
                same(S, name, views, 53, out, want)
                results.append(run(S, name, views, 53, out, want_pixels=True))
            assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert fallback.n == 0


def entry(I, src, B, h, w, out, patch=P, planes=None):
    """The library's entry through ctypes with the descriptor as given. Returns ``(rc, planes)``."""
    H, W = out
    tabs = I._device_tables(h, w, H, W, patch, torch.device("cuda", torch.cuda.current_device()))
    gh, gw = H // patch, W // patch
    if planes is None:
        planes = torch.empty(3, B * gh * gw, 3 * patch * patch, dtype=torch.bfloat16, device="cuda")
    rc = I._L().nos_image_patch_planes_yuv(ctypes.byref(src),
                                           *I._tail_args(tabs, planes, None, MEAN, STD, B, h, w, H, W, patch, gh, gw))
    return rc, planes


def descriptor(I, S, name, views):
    kind, sub, depth, msb, swap = S.FORMATS[name]
    layout = {"planar": I.YUV_PLANAR, "semiplanar": I.YUV_SEMIPLANAR, "packed": I.YUV_PACKED}[kind]
    order = tuple(I.YUYV_ORDERS).index({"yuy2": "yuyv"}.get(name, name)) if kind == "packed" else int(swap)
    src = I.yuv_src(layout, views, sub, depth, msb, order if kind != "planar" else 0, I.yuv_table("bt601", False, depth))
    return src


def test_batch_strides_with_a_gap_and_negative(K, I, S):
    out = (80, 112)
    for name in ("i444", "p010", "uyvy", "i210"):
        pic = Picture.of(I, S, name, 37, 53, batch=2, seed=4)
        want = yardstick(I, pic, out)
        wide = S.FORMATS[name][2] != 8
        cpu = pic.planes(name)
        for pad in (0x00, 0xFF):
            # a gap between the batch elements, one per plane
            views = [pitched(t, t.shape[2] + 4, pad, bstride=t.shape[1] * (t.shape[2] + 4) + 6 + 4 * k)
                     for k, t in enumerate(cpu)]
            same(S, name, views, 53, out, want)
            # the batch runs backwards through memory: element 0 is the last in the allocation
            views = [pitched(t.flip(0), t.shape[2] + (2 if wide else 3), pad, lead=2 if wide else 1) for t in cpu]
            src = descriptor(I, S, name, views)          # (bytes: the strides of the views are the byte strides)
            for k, v in enumerate(views):
                src.plane[k].p = v.data_ptr() + v.stride(0)
                src.plane[k].bstride = -v.stride(0)
            rc, got = entry(I, src, 2, 37, 53, out)
            torch.cuda.synchronize()
            assert rc == 0 and torch.equal(got, want[0]), name


def test_ignored_bits_and_the_times_four_law(K, I, S):
    out = (80, 112)
    for name in ("p010", "i010"):
        pic = Picture.of(I, S, name, 37, 53, seed=5)
        want = yardstick(I, pic, out)
        noisy, clean = pic.planes(name, noise=True), pic.planes(name, noise=False)
        assert not torch.equal(noisy[0], clean[0]) and not torch.equal(noisy[1], clean[1])
        for planes in (noisy, clean):
            same(S, name, [t.cuda() for t in planes], 53, out, want)
    # 10-bit codes that are 4 x the codes of an 8-bit frame (limited range): that frame's RGB, at any matrix
    eight = Picture(I, S, "420", 8, 37, 53, seed=6)
    y8, u8, v8 = (t.to(torch.uint8) for t in (eight.y, eight.u, eight.v))
    g = torch.Generator().manual_seed(7)
    for matrix in ("bt601", "bt709"):
        rgb = I.yuv420_to_rgb(y8, u8, v8, matrix)
        want = I.image_patch_planes(rgb.cuda(), out, P, MEAN, STD, want_pixels=True)
        views = [words(eight.y * 4, 10, True, g).cuda(),
                 words(torch.stack((eight.u, eight.v), dim=-1).flatten(2) * 4, 10, True, g).cuda()]
        got = frame(S, "p010", views, 53, matrix=matrix).patch_planes(out, P, MEAN, STD, True)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), matrix


def test_matrices_and_ranges(K, I, S):
    # the table is an argument of the launch: BT.2020 and full range at 10 and 8 bits
    for name, matrix, full in (("p010", "bt2020", False), ("i410", "bt2020", True), ("yuy2", "bt709", True),
                               ("nv24", "bt2020", False)):
        pic = Picture.of(I, S, name, 37, 53, seed=8)
        f = frame(S, name, [t.cuda() for t in pic.planes(name)], 53, matrix=matrix, full_range=full)
        want = I.image_patch_planes(f.to("cpu").rgb().cuda(), (80, 112), P, MEAN, STD, want_pixels=True)
        assert not torch.equal(want[1], yardstick(I, pic, (80, 112))[1])
        got = f.patch_planes((80, 112), P, MEAN, STD, True)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name


def test_grid_stride_on_a_sliced_grid(K, I, S, monkeypatch):
    # 2 x 13 x 11 tiles (pixels wanted, H and W no multiple of the patch) on 7 workgroups
    out = (200, 170)
    pics = {name: Picture.of(I, S, name, 53, 37, batch=2, seed=9) for name in ("nv16", "yuy2", "i410", "p010")}
    wants = {name: yardstick(I, pic, out) for name, pic in pics.items()}
    monkeypatch.setattr(I, "image_wgs", lambda: 7)
    for name, pic in pics.items():
        assert wants[name][0].shape[1] == 2 * 12 * 10
        same(S, name, [t.cuda() for t in pic.planes(name)], 37, out, wants[name])


def test_patch_side_8(K, I, S):
    for name in ("i444", "uyvy", "p010"):
        pic = Picture.of(I, S, name, 37, 53, seed=10)
        want = yardstick(I, pic, (40, 56), patch=8)
        assert want[0].shape == (3, 35, 192)
        same(S, name, [t.cuda() for t in pic.planes(name)], 53, (40, 56), want, patch=8)


def test_rejections_launch_nothing(K, I, S):
    out = (80, 96)
    L = I._L()
    sentinel = torch.full((3, 2 * 30, 768), 7.0, dtype=torch.bfloat16, device="cuda")
    planes = sentinel.clone()

    def refused(src, cause, name):
        rc, _ = entry(I, src, 2, 48, 64, out, planes=planes)
        assert rc != 0 and cause in L.nos_image_last_error().decode(), (name, cause, L.nos_image_last_error())

    for name in ("i422", "nv24", "yuy2", "p010", "i410"):
        pic = Picture.of(I, S, name, 48, 64, batch=2, seed=11)
        views = [t.cuda() for t in pic.planes(name)]
        k = len(views) - 1                                  # the last plane of the layout
        fresh = lambda: descriptor(I, S, name, views)       # noqa: E731
        src = fresh()
        src.size += 4
        refused(src, "descriptor size", name)
        for field, value, cause in (("layout", 3, "unknown layout"), ("vsub", 2, "unknown subsampling"),
                                    ("hsub", 1 - src.hsub if src.vsub else 2, "unknown subsampling"),
                                    ("depth", 9, "unknown sample format"), ("shift", 3, "unknown sample format"),
                                    ("sample_bytes", 3 - src.sample_bytes, "sample"), ("order", 3, "unknown order")):
            src = fresh()
            setattr(src, field, value)
            refused(src, cause, (name, field))
        src = fresh()
        src.plane[k].pitch = views[k].shape[2] - 1
        refused(src, "pitch is smaller", name)
        src = fresh()                                       # the last batch element ends past the storage
        src.plane[k].bstride += 2
        refused(src, "storage bounds", name)
        src = fresh()
        src.plane[k].hi -= 1
        refused(src, "storage bounds", name)
        src = fresh()
        src.tab[1] = 1 << 23
        refused(src, "colour table", name)
        if S.FORMATS[name][2] != 8:
            # an odd address, inside the storage: one byte further in a buffer with room for it
            roomy = [pitched(t, t.shape[2] + 2, 0, lead=2, tail=2) for t in views]
            src = descriptor(I, S, name, roomy)
            rc, _ = entry(I, src, 2, 48, 64, out, planes=planes.clone())
            assert rc == 0
            src.plane[k].p += 1
            refused(src, "even address", name)
            src = descriptor(I, S, name, roomy)
            src.plane[k].pitch += 1
            refused(src, "even", name)
    rc = L.nos_image_patch_planes_yuv(None, *([None] * 6), *([0] * 5), None, None, *([0] * 9), None)
    assert rc != 0
    torch.cuda.synchronize()
    assert torch.equal(planes, sentinel)                   # nothing was launched
    rc, _ = entry(I, descriptor(I, S, "i422", [t.cuda() for t in Picture.of(I, S, "i422", 48, 64, 2).planes("i422")]),
                  2, 48, 64, out, planes=planes)
    torch.cuda.synchronize()
    assert rc == 0 and not torch.equal(planes, sentinel)


# ---- end to end ---------------------------------------------------------------------------------
def randomize(module, seed=1):
    """Every parameter distinguishable (as ``test_gpu_image.randomize``)."""
    g = torch.Generator().manual_seed(seed)
    ln = {id(m.weight) for m in module.modules() if isinstance(m, torch.nn.LayerNorm)}
    with torch.no_grad():
        for _, p in sorted(module.named_parameters()):
            r = torch.randn(p.shape, generator=g, dtype=torch.float32)
            p.copy_(1.0 + r * 0.5 if id(p) in ln else r * (0.05 if p.dim() >= 2 else 0.5))


@pytest.fixture(scope="module")
def model(K):
    from walkai_nos_amd.models.workload.processor import YolosProcessor
    from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=2, use_mid_position_embeddings=True)).eval()
    randomize(m)
    m.invalidate_cache()
    m.processor = YolosProcessor(80, 133)
    return m.cuda()


@pytest.mark.parametrize("name", ("p010", "yuy2"))
def test_detect_image_graph_replay_on_a_new_frame(K, I, S, model, monkeypatch, name):
    h, w = 48, 64
    pitch = 160 if name == "p010" else 144                  # rows of 128 bytes on a pitched surface
    n = pitch * h * 3 // 2 if name == "p010" else pitch * h
    contents = [torch.randint(0, 256, (n,), generator=torch.Generator().manual_seed(s), dtype=torch.uint8) for s in (5, 6)]
    buf = contents[0].cuda()
    frame_ = S.from_buffer(name, buf, h, w, pitch, matrix="bt709")
    assert all(getattr(frame_, p).untyped_storage().data_ptr() == buf.untyped_storage().data_ptr() for p in frame_.PLANES)
    fused = Counter(monkeypatch, I, "yuv_semiplanar_patch_planes" if name == "p010" else "yuyv_patch_planes")
    converted = Counter(monkeypatch, I, "yuv_to_rgb")
    with torch.no_grad():
        s = model.detect_image(frame_, 0.0)["scores"][0].sort().values
        thr = 0.5 * (s[49] + s[50]).item()      # half of the rows survive on the first frame
        first = {k: v.clone() for k, v in model.detect_image(frame_, thr).items()}
        assert fused.n == 2 and converted.n == 0 and K.x3_active(model.pos_embed)
        want = model.detect_image(frame_.rgb(), thr)
    assert first["count"].tolist() == [50]
    for k, v in want.items():
        assert torch.equal(first[k], v), k
    assert torch.equal(model._target_sizes(frame_), torch.tensor([[48.0, 64.0]], device="cuda"))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=stream):
        held = model.detect_image(frame_, thr)
    for v in held.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, v in first.items():
        assert torch.equal(held[k], v), k
    # the next frame is written into the same buffer: the graph reads it by address
    buf.copy_(contents[1])
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        second = model.detect_image(frame_, thr)
    for k, v in second.items():
        assert torch.equal(held[k], v), k
    assert not torch.equal(held["logits"], first["logits"])
    del graph


# ---- the pod client (last: it starts a process, and nothing follows it if it fails) --------------
def test_pod_client_end_to_end_p010():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "walkai_nos_amd.dataplane.client", "--end-to-end",
           "--pixel-format", "p010", "--matrix", "bt2020", "--image-hw", "48,64", "--size", "80,133", "--seconds", "1",
           "--threshold", "0.0"]
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert p.stdout.readline().strip() == "READY"
        p.stdin.write(f"GO {time.time()}\n")
        p.stdin.flush()
        lines = p.stdout.read().strip().splitlines()
        assert p.wait(timeout=60) == 0
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["pixel_format"] == "p010" and out["end_to_end"] is True and out["input_hw"] == [80, 96]
    assert out["inferences"] > 0 and out["detections"] == 100      # threshold 0 keeps every detection token
