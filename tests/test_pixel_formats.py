"""The source layouts beside contiguous RGB and NV12 (``ops.image``, ``models.workload.processor``), off the
GPU: the integer conversion chain (planar 4:2:0 is the definition, NV12 and NV21 are it on de-interleaved
planes), the packed re-ordering, the zero-copy views of a planar surface, validation, and that the model gives
the same detections whichever layout the same picture arrives in. On the CPU every layout is the composition
``image_patch_planes(converted contiguous RGB)``, which is what the GPU kernels are held to bit for bit in
``test_gpu_pixel_formats.py``."""
import numpy as np
import pytest
import torch

from walkai_nos_amd.models.workload import processor as PR
from walkai_nos_amd.models.workload.processor import Frame, Nv12, Packed, YolosProcessor, Yuv420p
from walkai_nos_amd.ops import image as I

MEAN, STD = PR.IMAGENET_MEAN, PR.IMAGENET_STD
P = 16
COMBOS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]


def planes420(h, w, batch=1, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return (torch.randint(0, 256, (batch, h, w), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (batch, ch, cw), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (batch, ch, cw), generator=g, dtype=torch.uint8))


def same(a, b):
    assert torch.equal(a[0], b[0])
    assert (a[1] is None and b[1] is None) or torch.equal(a[1], b[1])


# ---- the conversion chain -----------------------------------------------------------------------
@pytest.mark.parametrize("hw", ((37, 53), (2, 2)), ids=("37x53", "2x2"))
@pytest.mark.parametrize("matrix,full_range", COMBOS, ids=[f"{m}-{'full' if f else 'limited'}" for m, f in COMBOS])
def test_nv12_is_the_planar_definition_on_its_de_interleaved_planes(hw, matrix, full_range):
    y, u, v = planes420(*hw, batch=2)
    uv, vu = torch.stack((u, v), dim=-1), torch.stack((v, u), dim=-1)
    want = I.yuv420_to_rgb(y, u, v, matrix, full_range)
    assert want.shape == (2,) + hw + (3,) and want.dtype == torch.uint8
    assert torch.equal(I.nv12_to_rgb(y, uv, matrix, full_range), want)
    assert torch.equal(I.nv12_to_rgb(y, uv, matrix, full_range), I.yuv420_to_rgb(y, uv[..., 0], uv[..., 1], matrix, full_range))
    # the VU order is the planes swapped
    assert torch.equal(I.nv12_to_rgb(y, vu, matrix, full_range, vu=True), want)
    assert torch.equal(I.nv12_to_rgb(y, uv, matrix, full_range, vu=True), I.yuv420_to_rgb(y, v, u, matrix, full_range))
    if hw != (2, 2):
        assert not torch.equal(I.yuv420_to_rgb(y, v, u, matrix, full_range), want)
    # the definition, spelled out for one pixel: nearest chroma, the table's integers
    t = I.nv12_table(matrix, full_range)
    r, c = hw[0] - 1, hw[1] - 1
    yy, uu, vv = int(y[1, r, c]) - t[9], int(u[1, r >> 1, c >> 1]) - t[10], int(v[1, r >> 1, c >> 1]) - t[11]
    px = [min(max((t[3 * k] * yy + t[3 * k + 1] * uu + t[3 * k + 2] * vv + 32768) >> 16, 0), 255) for k in range(3)]
    assert want[1, r, c].tolist() == px


def test_patch_plane_fallbacks_are_the_composition():
    y, u, v = planes420(37, 53, seed=1)
    uv, vu = torch.stack((u, v), dim=-1), torch.stack((v, u), dim=-1)
    out = (80, 112)
    want = I.image_patch_planes(I.yuv420_to_rgb(y, u, v, "bt709", True), out, P, MEAN, STD, want_pixels=True)
    same(I.yuv420p_patch_planes(y, u, v, out, P, MEAN, STD, "bt709", True, want_pixels=True), want)
    same(I.nv12_patch_planes(y, uv, out, P, MEAN, STD, "bt709", True, want_pixels=True), want)
    same(I.nv12_patch_planes(y, vu, out, P, MEAN, STD, "bt709", True, want_pixels=True, vu=True), want)
    assert I.yuv420p_patch_planes(y, u, v, out, P, MEAN, STD)[1] is None


# ---- packed pixels ------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ("bgr", "rgba", "bgra"))
def test_packed_fallback_is_the_rgb_path_on_the_re_indexed_frame(order):
    g = torch.Generator().manual_seed(3)
    rgb = torch.randint(0, 256, (2, 37, 53, 3), generator=g, dtype=torch.uint8)
    out = (80, 112)
    want = I.image_patch_planes(rgb, out, P, MEAN, STD, want_pixels=True)
    C, idx = I.PACKED_ORDERS[order]
    alphas = (None,) if C == 3 else (0, 255, torch.randint(0, 256, (2, 37, 53), generator=g, dtype=torch.uint8))
    for alpha in alphas:
        img = torch.empty(2, 37, 53, C, dtype=torch.uint8)
        for k in range(3):
            img[..., idx[k]] = rgb[..., k]
        if C == 4:
            img[..., 3] = alpha
        assert torch.equal(I.packed_to_rgb(img, order), rgb)
        same(I.packed_patch_planes(img, order, out, P, MEAN, STD, want_pixels=True), want)
        same(Packed(img, order).patch_planes(out, P, MEAN, STD, True), want)
    other = {"bgr": "rgb", "bgra": "rgba", "rgba": "bgra"}[order]         # and the order matters
    assert not torch.equal(I.packed_patch_planes(img, other, out, P, MEAN, STD)[0], want[0])


def test_packed_views_and_validation():
    g = torch.Generator().manual_seed(4)
    frame = torch.randint(0, 256, (2, 64, 80, 3), generator=g, dtype=torch.uint8)
    crop = frame[:, 9:57, 7:71]
    assert not crop.is_contiguous()
    want = I.image_patch_planes(crop.contiguous(), (80, 96), P, MEAN, STD, want_pixels=True)
    same(I.packed_patch_planes(crop, "rgb", (80, 96), P, MEAN, STD, want_pixels=True), want)
    same(I.image_patch_planes(crop, (80, 96), P, MEAN, STD, want_pixels=True), want)
    assert Packed(crop[0], "rgb").shape == (1, 48, 64, 3) and Packed(crop, "bgr").shape == (2, 48, 64, 3)
    with pytest.raises(ValueError, match="channel order"):
        I.packed_patch_planes(crop, "argb", (80, 96), P, MEAN, STD)
    with pytest.raises(ValueError, match="channel order"):
        Packed(crop, "grb")
    with pytest.raises(ValueError, match="uint8"):
        I.packed_patch_planes(crop.float(), "rgb", (80, 96), P, MEAN, STD)
    with pytest.raises(ValueError, match=r"\[B, h, w, 4\]"):
        I.packed_patch_planes(crop, "bgra", (80, 96), P, MEAN, STD)
    with pytest.raises(ValueError, match="contiguous"):      # every other column: pixels are not side by side
        I.packed_patch_planes(frame[:, :, ::2], "rgb", (80, 96), P, MEAN, STD)
    with pytest.raises(ValueError, match="contiguous"):      # channels-first storage viewed channels-last
        Packed(torch.zeros(1, 3, 48, 64, dtype=torch.uint8).permute(0, 2, 3, 1), "rgb")


# ---- Yuv420p.from_buffer ------------------------------------------------------------------------
def test_from_buffer_views_alias_the_surface():
    h, w = 6, 10
    g = torch.Generator().manual_seed(5)
    # the default chroma pitch (pitch // 2) and an explicit one; a sliced buffer's storage offset
    for pitch, cpitch, off in ((None, None, 0), (16, None, 0), (13, 7, 0), (13, 9, 5), (10, 5, 3)):
        yp = w if pitch is None else pitch
        cp = yp // 2 if cpitch is None else cpitch
        need = h * yp + (h - 1) * cp + 5
        store = torch.randint(0, 256, (off + need + 4,), generator=g, dtype=torch.uint8)
        buf = store[off:]
        kw = {k: v for k, v in (("pitch", pitch), ("chroma_pitch", cpitch)) if v is not None}
        f = Yuv420p.from_buffer(buf, h, w, **kw)
        s = Yuv420p.from_buffer(buf, h, w, order="yv12", **kw)
        base = store.data_ptr()
        assert f.y.data_ptr() == base + off and f.y.shape == (h, w) and f.y.stride() == (yp, 1)
        assert f.u.data_ptr() == base + off + h * yp and f.u.shape == (3, 5) and f.u.stride() == (cp, 1)
        assert f.v.data_ptr() == base + off + h * yp + 3 * cp and f.v.shape == (3, 5) and f.v.stride() == (cp, 1)
        # yv12: the same bytes, the chroma planes named the other way round
        assert s.y.data_ptr() == f.y.data_ptr() and s.u.data_ptr() == f.v.data_ptr() and s.v.data_ptr() == f.u.data_ptr()
        for t in (f.y, f.u, f.v):
            assert t.untyped_storage().data_ptr() == store.untyped_storage().data_ptr()     # no copy
        flat = buf.tolist()
        assert f.y[5].tolist() == flat[5 * yp:5 * yp + w]
        assert f.u[2].tolist() == flat[h * yp + 2 * cp:h * yp + 2 * cp + 5]
        assert f.v[2].tolist() == flat[h * yp + 5 * cp:h * yp + 5 * cp + 5]
        assert torch.equal(s.rgb(), I.yuv420_to_rgb(f.y, f.v, f.u)) and f.shape == (1, h, w, 3)
        # exactly enough bytes is enough, one fewer is not
        Yuv420p.from_buffer(buf[:need], h, w, **kw)
        with pytest.raises(ValueError, match="takes .* bytes"):
            Yuv420p.from_buffer(buf[:need - 1], h, w, **kw)
    # an ndarray is viewed, not copied
    arr = np.zeros(h * w * 3 // 2, dtype=np.uint8)
    f = Yuv420p.from_buffer(arr, h, w)
    arr[h * w] = 77
    assert int(f.u[0, 0]) == 77
    buf = torch.zeros(400, dtype=torch.uint8)
    with pytest.raises(ValueError, match="pitch 9 is smaller"):
        Yuv420p.from_buffer(buf, h, w, pitch=9)
    with pytest.raises(ValueError, match="chroma pitch 4 is smaller"):
        Yuv420p.from_buffer(buf, h, w, pitch=10, chroma_pitch=4)
    with pytest.raises(ValueError, match="chroma pitch 4 is smaller"):      # the default, half of an odd row's pitch
        Yuv420p.from_buffer(buf, h, 9)
    with pytest.raises(ValueError, match="even height"):
        Yuv420p.from_buffer(buf, 5, w)
    with pytest.raises(ValueError, match="order"):
        Yuv420p.from_buffer(buf, h, w, order="nv12")
    with pytest.raises(ValueError, match="contiguous uint8"):
        Yuv420p.from_buffer(buf.float(), h, w)
    with pytest.raises(ValueError, match="contiguous uint8"):
        Yuv420p.from_buffer(buf[::2], h, w)


def test_nv12_from_buffer_takes_the_chroma_order():
    h, w = 4, 6
    buf = torch.arange(h * w * 3 // 2, dtype=torch.uint8)
    a, b = Nv12.from_buffer(buf, h, w), Nv12.from_buffer(buf, h, w, vu=True)
    assert a.vu is False and b.vu is True and a.uv.data_ptr() == b.uv.data_ptr()
    assert Nv12(a.y, a.uv, "bt709", True).vu is False           # the field trails the existing ones
    assert torch.equal(b.rgb(), I.yuv420_to_rgb(a.y, a.uv[..., 1], a.uv[..., 0]))
    assert torch.equal(a.rgb(), I.yuv420_to_rgb(a.y, a.uv[..., 0], a.uv[..., 1]))


# ---- plane validation ---------------------------------------------------------------------------
def test_planar_planes_are_checked():
    y, u, v = planes420(48, 64)

    def run(yy, uu, vv, **kw):
        return I.yuv420p_patch_planes(yy, uu, vv, (80, 96), P, MEAN, STD, **kw)
    run(y, u, v)
    run(y[0], u[0], v[0])
    for bad in ((y, u[:, :-1], v), (y, u, v[:, :, :-1]), (y, u, v[:1].expand(2, -1, -1)), (y, u[0], v)):
        with pytest.raises(ValueError, match="shape|without B"):
            run(*bad)
    with pytest.raises(ValueError, match="one device"):
        run(y, u.to("meta"), v)
    for bad in ((y.float(), u, v), (y, u.to(torch.int32), v), (y, u, v.numpy())):
        with pytest.raises(ValueError, match="uint8"):
            run(*bad)
    wide = torch.zeros(1, 24, 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="contiguous"):          # the halves of an interleaved plane are not planar
        run(y, wide[:, :, ::2], v)
    with pytest.raises(ValueError, match="contiguous"):
        Yuv420p(y, u, wide[:, :, 1::2])
    with pytest.raises(ValueError, match="matrix"):
        run(y, u, v, matrix="bt2020")
    with pytest.raises(ValueError, match="matrix"):
        Yuv420p(y, u, v, "bt2020")
    # the torch definition reads such halves (it is how NV12 is defined)
    assert I.yuv420_to_rgb(y, wide[:, :, ::2], wide[:, :, 1::2]).shape == (1, 48, 64, 3)


# ---- the model ----------------------------------------------------------------------------------
def test_the_model_detects_the_same_whatever_layout_the_picture_arrives_in():
    from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
    torch.manual_seed(0)
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=1)).eval()
    m.processor = YolosProcessor(80, 133)
    h, w = 48, 64
    y, u, v = planes420(h, w, seed=6)
    rgb = I.yuv420_to_rgb(y, u, v)
    g = torch.Generator().manual_seed(7)
    bgra = torch.cat((rgb[..., [2, 1, 0]], torch.randint(0, 256, (1, h, w, 1), generator=g, dtype=torch.uint8)), dim=-1)
    surface = torch.cat((y.flatten(), u.flatten(), v.flatten()))
    big = torch.randint(0, 256, (128, 160, 3), generator=g, dtype=torch.uint8)
    big[40:88, 24:88] = rgb[0]
    crop = big[40:88, 24:88]
    assert not crop.is_contiguous()
    frames = {"i420": Yuv420p.from_buffer(surface, h, w),
              "yv12": Yuv420p.from_buffer(torch.cat((y.flatten(), v.flatten(), u.flatten())), h, w, order="yv12"),
              "nv21": Nv12(y, torch.stack((v, u), dim=-1), vu=True),
              "bgra": Packed(bgra, "bgra"),
              "crop": crop,
              "crop as Packed": Packed(crop, "rgb")}
    with torch.no_grad():
        want = m.detect_image(rgb[0], 0.0)
        assert want["count"].tolist() == [100] and want["boxes"].abs().max() > 1.0      # pixels of the 48 x 64 view
        for name, f in frames.items():
            got = m.detect_image(f, 0.0)
            assert set(got) == set(want), name
            for k in want:
                assert torch.equal(got[k], want[k]), (name, k)
            assert torch.equal(m._target_sizes(m.processor.as_batch(f)), torch.tensor([[48.0, 64.0]])), name
            assert torch.equal(m.processor.preprocess(f), m.processor.preprocess(rgb)), name


# ---- one protocol, no branch per format ---------------------------------------------------------
def test_frames_share_one_protocol_and_the_model_knows_no_format():
    from walkai_nos_amd.models.workload import yolos
    y, u, v = planes420(4, 6)
    frames = (Nv12(y, torch.stack((u, v), dim=-1)), Yuv420p(y, u, v),
              Packed(torch.zeros(4, 6, 4, dtype=torch.uint8), "bgra"))
    formats = {c for c in vars(PR).values() if isinstance(c, type) and issubclass(c, Frame) and c is not Frame}
    assert formats == {Nv12, Yuv420p, Packed} == {type(f) for f in frames}
    for f in frames:
        assert isinstance(f, Frame) and f.shape == (1, 4, 6, 3) and f.device == torch.device("cpu") and not f.is_cuda
        assert f.to("cpu") is f and f.to(None) is f and YolosProcessor.as_batch(f) is f
        moved = f.to("meta")
        assert type(moved) is type(f) and moved.device.type == "meta" and moved.shape == f.shape
        rgb = f.rgb()
        assert rgb.shape == (1, 4, 6, 3) and rgb.dtype == torch.uint8 and rgb.is_contiguous()
        for name in ("shape", "device", "is_cuda", "to", "rgb", "patch_planes"):
            assert name in vars(Frame)                           # the protocol is the base class's, not each format's
        pr = YolosProcessor(32, 48)
        same(pr.patch_planes(f, (32, 48), want_pixels=True), I.image_patch_planes(rgb, (32, 48), P, MEAN, STD, True))
    # yolos.py reaches the formats only through the processor: none of them (and no module-level reference to
    # one) is among its names
    for name, obj in vars(yolos).items():
        assert obj is not Frame and not any(obj is c for c in formats), name
        assert not isinstance(obj, Frame), name
    assert not {"Nv12", "Yuv420p", "Packed", "Frame"} & set(vars(yolos))
    assert not {"Nv12", "Yuv420p", "Packed", "Frame", "isinstance"} & (set(yolos.YolosSmall.encode_image.__code__.co_names)
                                                                     | set(yolos.YolosSmall.detect_image.__code__.co_names)
                                                                     | set(yolos.YolosSmall._image_fused.__code__.co_names)
                                                                     | set(yolos.YolosSmall._target_sizes.__code__.co_names))
