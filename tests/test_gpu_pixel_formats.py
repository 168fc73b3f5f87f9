"""The source layouts beside contiguous RGB and NV12 on the GPU (``csrc/image.hip``: planar 4:2:0, NV21, packed
BGR / RGBA / BGRA and pitched views): each fused launch against the RGB kernel on the frame converted or
re-ordered on the CPU. The conversion is defined in integers and everything behind the staging loop is the RGB
kernel's code, so planes and pixels are compared with ``torch.equal`` — no tolerance; the RGB kernel itself is
pinned against fp64 in ``test_gpu_image.py``. Each case is the smallest size that reaches its branch (patch 16
unless said otherwise, seeded random planes). Bounds are shown by results that do not depend on the pad bytes
around a plane and by planes that end on their storage's last byte, never by a fault."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
P = 16
LAYOUTS = ("i420", "nv21", "bgr", "rgba", "bgra")

#: (source h, w, target H, W, fused?)
CASES = ((48, 64, 80, 96, True),        # upscale: footprints start on odd rows and columns
         (37, 53, 80, 112, True),       # odd sizes: the last chroma row and column serve one luma line; w % 4 == 1
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


class Counter:
    def __init__(self, monkeypatch, owner, name):
        self.n = 0
        fn = getattr(owner, name)

        def spy(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        monkeypatch.setattr(owner, name, spy)


class Picture:
    """One seeded picture as planar 4:2:0 (CPU), and every layout of it: ``planes(layout)`` are the CPU planes
    ``[B, rows, rowbytes]`` of that layout, ``rgb`` the contiguous RGB frame all of them convert to."""

    def __init__(self, I, h, w, batch=1, seed=0):
        g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w)
        ch, cw = (h + 1) // 2, (w + 1) // 2
        self.h, self.w, self.B = h, w, batch
        self.y = torch.randint(0, 256, (batch, h, w), generator=g, dtype=torch.uint8)
        self.u = torch.randint(0, 256, (batch, ch, cw), generator=g, dtype=torch.uint8)
        self.v = torch.randint(0, 256, (batch, ch, cw), generator=g, dtype=torch.uint8)
        self.alpha = torch.randint(0, 256, (batch, h, w), generator=g, dtype=torch.uint8)
        self.rgb = I.yuv420_to_rgb(self.y, self.u, self.v)
        self.I = I

    def planes(self, layout):
        if layout == "i420":
            return [self.y, self.u, self.v]
        if layout == "nv21":
            return [self.y, torch.stack((self.v, self.u), dim=-1).flatten(2)]
        C, idx = self.I.PACKED_ORDERS[layout]
        img = torch.empty(self.B, self.h, self.w, C, dtype=torch.uint8)
        for k in range(3):
            img[..., idx[k]] = self.rgb[..., k]
        if C == 4:
            img[..., 3] = self.alpha
        return [img.flatten(2)]


def run(I, layout, planes, out, patch=P, want_pixels=False):
    """The fused call of ``layout`` on its GPU planes ``[B, rows, rowbytes]`` (views of any pitch)."""
    if layout == "i420":
        return I.yuv420p_patch_planes(*planes, out, patch, MEAN, STD, want_pixels=want_pixels)
    if layout == "nv21":
        return I.nv12_patch_planes(planes[0], planes[1].unflatten(2, (-1, 2)), out, patch, MEAN, STD,
                                   want_pixels=want_pixels, vu=True)
    C = I.PACKED_ORDERS[layout][0]
    return I.packed_patch_planes(planes[0].unflatten(2, (-1, C)), layout, out, patch, MEAN, STD, want_pixels)


_want = {}


def yardstick(I, pic, out, key=None, patch=P):
    """The RGB kernel on the converted frame (converted on the CPU): ``(planes, pixels)`` on the GPU, computed once
    per ``key`` and left unchanged."""
    if key is None or key not in _want:
        res = I.image_patch_planes(pic.rgb.cuda(), out, patch, MEAN, STD, want_pixels=True)
        if key is None:
            return res
        _want[key] = res
    return _want[key]


def same(I, layout, planes, out, want, patch=P):
    got, px = run(I, layout, planes, out, patch, want_pixels=True)
    only, none = run(I, layout, planes, out, patch)
    torch.cuda.synchronize()
    assert none is None and got.dtype == torch.bfloat16 and px.dtype == torch.float32
    assert torch.equal(px, want[1]), f"{layout}: pixels"
    assert torch.equal(got, want[0]) and torch.equal(only, want[0]), f"{layout}: planes"


def pitched(plane, pitch, pad, lead=0, tail=0, bstride=None):
    """``plane`` ``[B, rows, rowbytes]`` copied into a fresh GPU allocation with ``pitch`` bytes between rows,
    ``lead`` bytes before the first and ``tail`` after the last row's bytes, every other byte ``pad``; the view."""
    B, rows, rb = plane.shape
    per = (rows - 1) * pitch + rb if bstride is None else bstride
    buf = torch.full((lead + (B - 1) * per + (rows - 1) * pitch + rb + tail,), pad, dtype=torch.uint8, device="cuda")
    view = buf.as_strided((B, rows, rb), (per, pitch, 1), lead)
    view.copy_(plane)
    return view


FALLBACK = {"i420": "yuv420_to_rgb", "nv21": "nv12_to_rgb", "bgr": "packed_to_rgb", "rgba": "packed_to_rgb",
            "bgra": "packed_to_rgb"}


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layout_equals_the_rgb_kernel_on_the_converted_frame(K, I, monkeypatch, layout, case):
    h, w, H, W, fused = case
    pic = Picture(I, h, w)
    want = yardstick(I, pic, (H, W), key=case)
    planes = [t.cuda() for t in pic.planes(layout)]
    fallback = Counter(monkeypatch, I, FALLBACK[layout])
    same(I, layout, planes, (H, W), want)
    assert fallback.n == (0 if fused else 2)


@pytest.mark.parametrize("w", (5, 6, 7))
def test_the_last_column_group_straddles_the_row_end(K, I, w):
    pic = Picture(I, 3, w, batch=2, seed=1)
    want = yardstick(I, pic, (16, 16))
    for layout in LAYOUTS:
        same(I, layout, [t.cuda() for t in pic.planes(layout)], (16, 16), want)


def test_pitches_alignment_and_storage_ends(K, I, monkeypatch):
    pic = Picture(I, 37, 53, batch=2, seed=2)
    out = (80, 112)
    want = yardstick(I, pic, out)
    assert not torch.equal(want[1][0], want[1][1])
    spies = [Counter(monkeypatch, I, n) for n in set(FALLBACK.values())]
    for layout in LAYOUTS:
        cpu = pic.planes(layout)
        # per plane an odd pitch of its own; the first byte 1, 2, 3 bytes into the storage; trailing slack, and
        # none (the plane's last byte is the storage's last byte, the first its first)
        for leads, extra, tail in (((1, 2, 3), (11, 5, 9), 5), ((2, 3, 1), (1, 3, 7), 1), ((3, 1, 2), (0, 0, 0), 0),
                                   ((0, 0, 0), (0, 0, 0), 0), ((0, 0, 0), (3, 1, 5), 0)):
            results = []
            for pad in (0x00, 0xFF):
                views = [pitched(t, (t.shape[2] + e) | (1 if e else 0), pad, ld, tail)
                         for t, ld, e in zip(cpu, leads, extra)]
                for v, ld in zip(views, leads):
                    s = v.untyped_storage()
                    assert v.data_ptr() - s.data_ptr() == ld
                    if tail == 0:
                        last = v.data_ptr() + (v.shape[0] - 1) * v.stride(0) + (v.shape[1] - 1) * v.stride(1) + v.shape[2]
                        assert last == s.data_ptr() + s.nbytes()
                same(I, layout, views, out, want)
                results.append(run(I, layout, views, out, want_pixels=True))
            assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert all(s.n == 0 for s in spies)


def test_chroma_planes_with_pitches_of_their_own(K, I):
    # the U pitch is not the V pitch and neither is half the Y pitch; batch elements a plane-specific gap apart
    pic = Picture(I, 48, 64, batch=2, seed=3)
    want = yardstick(I, pic, (80, 96))
    y = pitched(pic.y, 80, 0xFF, bstride=48 * 80 + 33)
    u = pitched(pic.u, 37, 0xFF, lead=1, bstride=24 * 37 + 5)
    v = pitched(pic.v, 51, 0xFF, lead=2, bstride=24 * 51 + 64)
    assert u.stride(1) != v.stride(1) and 2 * u.stride(1) != y.stride(1) != 2 * v.stride(1)
    same(I, "i420", [y, u, v], (80, 96), want)
    from walkai_nos_amd.models.workload.processor import Yuv420p
    # a YV12 surface with an explicit chroma pitch: the planes by what they hold
    buf = torch.full((48 * 72 + 47 * 40 + 32,), 0xFF, dtype=torch.uint8, device="cuda")
    f = Yuv420p.from_buffer(buf, 48, 64, 72, 40, order="yv12")
    f.y.copy_(pic.y[0]), f.u.copy_(pic.u[0]), f.v.copy_(pic.v[0])
    assert f.v.data_ptr() < f.u.data_ptr() and f.u.data_ptr() + 23 * 40 + 32 == buf.data_ptr() + buf.numel()
    got = f.patch_planes((80, 96), P, MEAN, STD, True)
    assert torch.equal(got[0][:, :30], want[0][:, :30]) and torch.equal(got[1][0], want[1][0])


def entry(I, layout, views, out, patch=P, bstrides=None, pitches=None, order=None, his=None, planes=None):
    """The library's entry for ``layout`` through ctypes on GPU views ``[B, rows, rowbytes]``: batch strides, pitches,
    storage ends and the channel order as given instead of the views' own. Returns ``(rc, planes)``."""
    L = I._L()
    B, h = views[0].shape[:2]
    w = views[0].shape[2] // (I.PACKED_ORDERS[layout][0] if layout in I.PACKED_ORDERS else 1)
    H, W = out
    tabs = I._device_tables(h, w, H, W, patch, views[0].device)
    gh, gw = H // patch, W // patch
    if planes is None:
        planes = torch.empty(3, B * gh * gw, 3 * patch * patch, dtype=torch.bfloat16, device="cuda")
    bstrides = bstrides or [v.stride(0) for v in views]
    pitches = pitches or [v.stride(1) for v in views]
    ptrs = []
    for k, (v, bs) in enumerate(zip(views, bstrides)):
        lo, hi = I._storage_bounds(v)
        first = v.data_ptr() if bs >= 0 else v.data_ptr() + (B - 1) * v.stride(0)   # negative: start at the last
        ptrs += [first, lo, hi if his is None else his[k]]
    tail = I._tail_args(tabs, planes, None, MEAN, STD, B, h, w, H, W, patch, gh, gw)
    T12 = ctypes.c_int * 12
    if layout == "i420":
        rc = L.nos_image_patch_planes_yuv420p(*ptrs, *pitches, *bstrides, T12(*I.nv12_table()), *tail)
    elif layout == "nv21":
        rc = L.nos_image_patch_planes_nv12_order(*ptrs, *pitches, *bstrides, T12(*I.nv12_table()), *tail, 1)
    else:
        rc = L.nos_image_patch_planes_packed(*ptrs, pitches[0], bstrides[0], (layout if order is None else order).encode(), *tail)
    return rc, planes


def test_negative_batch_stride(K, I):
    # the batch runs backwards through memory: element 0 is the last in the allocation
    pic = Picture(I, 37, 53, batch=2, seed=4)
    out = (80, 112)
    want = yardstick(I, pic, out)[0]
    for layout in LAYOUTS:
        for pad in (0x00, 0xFF):
            views = [pitched(t.flip(0), t.shape[2] + 3, pad, lead=1) for t in pic.planes(layout)]
            rc, got = entry(I, layout, views, out, bstrides=[-v.stride(0) for v in views])
            torch.cuda.synchronize()
            assert rc == 0 and torch.equal(got, want), layout


def test_zero_copy_crop(K, I, monkeypatch):
    g = torch.Generator().manual_seed(5)
    frame = torch.randint(0, 256, (1, 128, 160, 4), generator=g, dtype=torch.uint8).cuda()
    rgb_frame = frame[..., :3].contiguous()
    crop, crop4 = rgb_frame[:, 40:88, 24:104], frame[:, 40:88, 24:104]
    assert not crop.is_contiguous() and crop.data_ptr() % 4 == 0 and crop[:, 1:, 1:].data_ptr() % 4 == 3
    out = (80, 128)
    want = I.image_patch_planes(crop.contiguous(), out, P, MEAN, STD, want_pixels=True)
    L = I._L()
    calls = []
    real = {n: getattr(L, n) for n in ("nos_image_patch_planes_u8", "nos_image_patch_planes_packed")}
    for n, fn in real.items():
        monkeypatch.setattr(L, n, lambda *a, _n=n, _f=fn: (calls.append(_n), _f(*a))[1])
    copies = Counter(monkeypatch, torch.Tensor, "contiguous")
    got = I.image_patch_planes(crop, out, P, MEAN, STD, want_pixels=True)
    got4 = I.packed_patch_planes(crop4, "bgra", out, P, MEAN, STD, want_pixels=True)
    odd = I.image_patch_planes(crop[:, 1:, 1:], (80, 128), P, MEAN, STD)            # first byte 3 past a dword
    assert calls == ["nos_image_patch_planes_packed"] * 3 and copies.n == 0
    bgra_want = I.image_patch_planes(crop4[..., [2, 1, 0]].contiguous(), out, P, MEAN, STD, want_pixels=True)
    odd_want = I.image_patch_planes(crop[:, 1:, 1:].contiguous(), (80, 128), P, MEAN, STD)
    torch.cuda.synchronize()
    for a, b in ((got, want), (got4, bgra_want)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(odd[0], odd_want[0])
    # a contiguous tensor still takes the RGB entry and nothing else
    del calls[:]
    I.image_patch_planes(rgb_frame, (80, 96), P, MEAN, STD)
    assert calls == ["nos_image_patch_planes_u8"]


def test_alpha_is_never_read_as_colour(K, I):
    pic = Picture(I, 37, 53, seed=6)
    a = pic.planes("rgba")[0].unflatten(2, (-1, 4)).cuda()
    b = a.clone()
    b[..., 3] = 255 - b[..., 3]
    assert not torch.equal(a, b) and torch.equal(a[..., :3], b[..., :3])
    pa, pb = (I.packed_patch_planes(t, "rgba", (80, 112), P, MEAN, STD, want_pixels=True) for t in (a, b))
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])
    assert torch.equal(pa[1], yardstick(I, pic, (80, 112))[1])


def test_grid_stride_on_a_slice(K, I):
    # 2 x 13 x 11 tiles (pixels wanted, H and W no multiple of the patch) on the 128 workgroups of a 32-CU slice
    pic = Picture(I, 53, 37, batch=2, seed=7)
    out = (200, 170)
    want = yardstick(I, pic, out)
    assert want[0].shape[1] == 2 * 12 * 10
    K.set_slice_cus(32)
    try:
        assert I.image_wgs() == 128
        for layout in ("bgra", "nv21", "i420"):
            same(I, layout, [t.cuda() for t in pic.planes(layout)], out, want)
    finally:
        K.set_slice_cus(None)


def test_patch_side_8(K, I):
    pic = Picture(I, 37, 53, seed=8)
    want = yardstick(I, pic, (40, 56), patch=8)
    assert want[0].shape == (3, 35, 192)
    for layout in ("bgr", "nv21", "i420"):
        same(I, layout, [t.cuda() for t in pic.planes(layout)], (40, 56), want, patch=8)


def test_rejections_launch_nothing(K, I):
    pic = Picture(I, 48, 64, batch=2, seed=9)
    out = (80, 96)
    L = I._L()
    sentinel = torch.full((3, 2 * 30, 768), 7.0, dtype=torch.bfloat16, device="cuda")
    planes = sentinel.clone()
    for layout in ("i420", "nv21", "bgr", "bgra"):
        views = [t.cuda() for t in pic.planes(layout)]
        k = len(views) - 1                                  # the last plane of the layout
        rows, rb = views[k].shape[1:]
        short = [v.stride(1) for v in views]
        short[k] = rb - 1
        # a batch stride one byte longer: the last batch element ends one byte past the storage
        far = [v.stride(0) for v in views]
        far[k] += 1
        for bad, cause in ((dict(pitches=short), "pitch is smaller"), (dict(bstrides=far), "storage bounds"),
                           (dict(his=[I._storage_bounds(v)[1] - (i == k) for i, v in enumerate(views)]), "storage bounds")):
            rc, _ = entry(I, layout, views, out, planes=planes, **bad)
            assert rc != 0 and cause in L.nos_image_last_error().decode(), (layout, bad)
        if layout in I.PACKED_ORDERS:
            for order in ("rbg", "argb", "", "RGB"):
                rc, _ = entry(I, layout, views, out, planes=planes, order=order)
                assert rc != 0 and "unknown channel order" in L.nos_image_last_error().decode(), order
    rc = L.nos_image_patch_planes_nv12_order(*([None] * 6), 0, 0, 0, 0, None, *([None] * 6), *([0] * 5), None, None,
                                             *([0] * 9), None, 2)
    assert rc != 0
    torch.cuda.synchronize()
    assert torch.equal(planes, sentinel)                   # nothing was launched
    rc, _ = entry(I, "i420", [t.cuda() for t in pic.planes("i420")], out, planes=planes)
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


@pytest.mark.parametrize("layout", ("i420", "bgra crop"))
def test_detect_image_graph_replay_on_a_new_frame(K, I, model, monkeypatch, layout):
    from walkai_nos_amd.models.workload.processor import Packed, Yuv420p
    h, w = 48, 64
    if layout == "i420":
        n, fused_name = h * 80 + h * 40, "yuv420p_patch_planes"
    else:
        n, fused_name = 64 * 80 * 4, "packed_patch_planes"
    contents = [torch.randint(0, 256, (n,), generator=torch.Generator().manual_seed(s), dtype=torch.uint8) for s in (5, 6)]
    buf = contents[0].cuda()
    if layout == "i420":
        frame = Yuv420p.from_buffer(buf, h, w, 80)
    else:
        frame = Packed(buf.view(64, 80, 4)[9:57, 7:71], "bgra")
        assert not frame.data.is_contiguous()
    fused = Counter(monkeypatch, I, fused_name)
    converted = [Counter(monkeypatch, I, name) for name in ("yuv420_to_rgb", "packed_to_rgb")]
    with torch.no_grad():
        s = model.detect_image(frame, 0.0)["scores"][0].sort().values
        thr = 0.5 * (s[49] + s[50]).item()      # half of the rows survive on the first frame
        first = {k: v.clone() for k, v in model.detect_image(frame, thr).items()}
        assert fused.n == 2 and all(c.n == 0 for c in converted) and K.x3_active(model.pos_embed)
        want = model.detect_image(frame.rgb(), thr)
    assert first["count"].tolist() == [50]
    for k, v in want.items():
        assert torch.equal(first[k], v), k
    # boxes in pixels of the view that was passed
    assert torch.equal(model._target_sizes(frame), torch.tensor([[48.0, 64.0]], device="cuda"))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=stream):
        held = model.detect_image(frame, thr)
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
        second = model.detect_image(frame, thr)
    for k, v in second.items():
        assert torch.equal(held[k], v), k
    assert not torch.equal(held["logits"], first["logits"])
    del graph
