"""Bilinear chroma with siting in the fused image kernel (``csrc/image.hip``'s ``stage_yuv_bilinear``), on the GPU:
each of the five instantiations against the RGB kernel on the frame converted on the CPU by the definition
(``ops.image.chroma_upsample``, itself checked in ``test_chroma_upsample.py``). The method is
``test_gpu_surfaces.py``'s, whose pictures and helpers are used: integers in front of a shared body, so planes and
pixels are compared with ``torch.equal`` — no tolerance; seeded random planes with random ignored bits in every 16-bit
word; patch 16 unless said otherwise. Every bilinear result is also required to differ from the nearest result of
the same planes. Bounds are shown by results that do not depend on the pad bytes around a plane and by planes that
begin and end on their storage's first and last byte, never by a fault."""
import pytest
import torch
from test_gpu_surfaces import (CASES, IDS, MEAN, STD, Counter, I, K, P, Picture, S, descriptor,  # noqa: F401
                               entry, frame, model, pitched)

pytestmark = pytest.mark.gpu

SITINGS = ("left", "center", "topleft", "top")
#: one format per bilinear instantiation (planar and semi-planar x 1- and 2-byte samples, packed), both vertical
#: geometries of each, both chroma orders, and the two older frame classes on the general entry
NAMES = ("i420", "nv12", "i422", "nv61", "p010", "i010", "p210", "yuy2", "uyvy")
#: the names ``surfaces.FORMATS`` does not know: (subsampling, depth)
OLDER = {"i420": ("420", 8), "nv12": ("420", 8)}


def picture(I, S, name, h, w, batch=1, seed=0):
    if name in OLDER:
        return Picture(I, S, *OLDER[name], h, w, batch, seed)
    return Picture.of(I, S, name, h, w, batch, seed)


def planes_of(pic, name, noise=True):
    """The CPU planes of format ``name`` as bytes ``[B, rows, rowbytes]``."""
    if name == "i420":
        return [t.to(torch.uint8) for t in (pic.y, pic.u, pic.v)]
    if name == "nv12":
        return [pic.y.to(torch.uint8), torch.stack((pic.u, pic.v), dim=-1).flatten(2).to(torch.uint8)]
    return pic.planes(name, noise)


def make(S, name, views, w, **kw):
    """The frame of format ``name`` over its GPU planes as bytes (views of any pitch)."""
    from walkai_nos_amd.models.workload.processor import Nv12, Yuv420p
    if name == "i420":
        return Yuv420p(*views, **kw)
    if name == "nv12":
        return Nv12(views[0], views[1].unflatten(2, (-1, 2)), **kw)
    return frame(S, name, views, w, **kw)


_want = {}


def yardstick(I, pic, out, siting, key=None, patch=P, **kw):
    """The RGB kernel on the frame converted on the CPU with bilinear chroma at ``siting``: ``(planes, pixels)`` on
    the GPU, computed once per ``key`` and left unchanged."""
    if key is not None:
        key = (key, pic.sub, pic.depth, siting)
        if key in _want:
            return _want[key]
    typed = [t.to(torch.uint8) if pic.depth == 8 else t.to(torch.int16) for t in (pic.y, pic.u, pic.v)]
    rgb = I.yuv_to_rgb(*typed, pic.sub, pic.depth, False, chroma="bilinear", siting=siting, **kw)
    res = I.image_patch_planes(rgb.cuda(), out, patch, MEAN, STD, want_pixels=True)
    if key is not None:
        _want[key] = res
    return res


def same(S, name, views, w, out, want, siting, patch=P, **kw):
    f = make(S, name, views, w, chroma="bilinear", siting=siting, **kw)
    got, px = f.patch_planes(out, patch, MEAN, STD, True)
    only, none = f.patch_planes(out, patch, MEAN, STD)
    torch.cuda.synchronize()
    assert none is None and got.dtype == torch.bfloat16 and px.dtype == torch.float32
    assert torch.equal(px, want[1]), f"{name} {siting}: pixels"
    assert torch.equal(got, want[0]) and torch.equal(only, want[0]), f"{name} {siting}: planes"
    return got, px


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("name", NAMES)
def test_bilinear_equals_the_rgb_kernel_on_the_converted_frame(K, I, S, monkeypatch, name, case):
    h, w, H, W, fused = case
    pic = picture(I, S, name, h, w)
    wants = {s: yardstick(I, pic, (H, W), s, key=case) for s in SITINGS}
    views = [t.cuda() for t in planes_of(pic, name)]
    nearest = make(S, name, views, w).patch_planes((H, W), P, MEAN, STD, True)
    fallback = Counter(monkeypatch, I, "yuv_to_rgb")
    for s in SITINGS:
        got, px = same(S, name, views, w, (H, W), wants[s], s)
        # the new code ran: not the nearest result of the same planes
        assert not torch.equal(px, nearest[1]) and not torch.equal(got, nearest[0]), (name, s)
    assert fallback.n == (0 if fused else 2 * len(SITINGS))
    # the sitings are told apart (on 4:2:2 the two that share their horizontal part are one)
    assert not torch.equal(wants["left"][1], wants["center"][1])
    assert torch.equal(wants["left"][1], wants["topleft"][1]) == (pic.sub == "422")


@pytest.mark.parametrize("hw", ((1, 1), (2, 2), (1, 3), (3, 2), (2, 5), (4, 4)), ids=lambda s: "{}x{}".format(*s))
def test_the_smallest_sources(K, I, S, monkeypatch, hw):
    # chroma planes of one or two rows and columns: every tap clamps
    h, w = hw
    assert I.fusable(hw, (16, 16), P)
    names = ("i420", "nv12", "p010", "i010", "i422", "yuy2")
    pics = {name: picture(I, S, name, h, w, batch=2, seed=1) for name in names}
    wants = {(name, s): yardstick(I, pic, (16, 16), s) for name, pic in pics.items() for s in SITINGS}
    fallback = Counter(monkeypatch, I, "yuv_to_rgb")
    for name, pic in pics.items():
        assert tuple(pic.u.shape[1:]) == ((h + 1) // 2 if pic.sub == "420" else h, (w + 1) // 2)
        views = [t.cuda() for t in planes_of(pic, name)]
        for s in SITINGS:
            same(S, name, views, w, (16, 16), wants[name, s], s)
    assert fallback.n == 0


def test_pitches_alignment_and_storage_ends(K, I, S, monkeypatch):
    # one 8-bit and one 16-bit format of each layout (packed is 8-bit only); the window of the first column group
    # begins one sample before its row and that of the last ends past it: in the pitch padding, in the neighbouring
    # row, or outside the storage
    out = (80, 112)
    names = ("i420", "i010", "nv12", "p210", "yuy2")
    pics = {name: picture(I, S, name, 37, 53, batch=2, seed=2) for name in names}
    wants = {(name, s): yardstick(I, pics[name], out, s) for name in names for s in SITINGS}
    fallback = Counter(monkeypatch, I, "yuv_to_rgb")
    for name, pic in pics.items():
        cpu = planes_of(pic, name)
        wide = pic.depth != 8
        for leads, extra, tail in (((1, 2, 3), (11, 5, 9), 5), ((3, 1, 2), (0, 0, 0), 0), ((0, 0, 0), (0, 0, 0), 0),
                                   ((0, 0, 0), (3, 1, 5), 0)):
            if wide:
                leads, extra, tail = tuple(2 if ld else 0 for ld in leads), tuple(2 * e for e in extra), 2 * tail
            for s in SITINGS:
                results = []
                for pad in (0x00, 0xFF):
                    views = [pitched(t, t.shape[2] + e if wide else (t.shape[2] + e) | (1 if e else 0), pad, ld, tail)
                             for t, ld, e in zip(cpu, leads, extra)]
                    for v, ld in zip(views, leads):
                        st = v.untyped_storage()
                        assert v.data_ptr() - st.data_ptr() == ld
                        if tail == 0:
                            last = v.data_ptr() + (v.shape[0] - 1) * v.stride(0) + (v.shape[1] - 1) * v.stride(1) \
                                + v.shape[2]
                            assert last == st.data_ptr() + st.nbytes()
                    results.append(same(S, name, views, 53, out, wants[name, s], s))
                assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert fallback.n == 0


def test_batch_of_two_with_a_gap(K, I, S):
    out = (80, 112)
    for name in ("i420", "p010", "uyvy", "nv61"):
        pic = picture(I, S, name, 37, 53, batch=2, seed=4)
        cpu = planes_of(pic, name)
        for s in ("left", "center"):
            want = yardstick(I, pic, out, s)
            assert not torch.equal(want[1][0], want[1][1])
            for pad in (0x00, 0xFF):
                views = [pitched(t, t.shape[2] + 4, pad, bstride=t.shape[1] * (t.shape[2] + 4) + 6 + 4 * k)
                         for k, t in enumerate(cpu)]
                same(S, name, views, 53, out, want, s)


def test_grid_stride_on_a_sliced_grid(K, I, S, monkeypatch):
    # 2 x 13 x 11 tiles (pixels wanted, H and W no multiple of the patch) on 7 workgroups
    out = (200, 170)
    pics = {name: picture(I, S, name, 53, 37, batch=2, seed=9) for name in ("nv12", "i422", "yuy2", "p010")}
    wants = {(name, s): yardstick(I, pic, out, s) for name, pic in pics.items() for s in ("left", "top")}
    monkeypatch.setattr(I, "image_wgs", lambda: 7)
    for (name, s), want in wants.items():
        assert want[0].shape[1] == 2 * 12 * 10
        same(S, name, [t.cuda() for t in planes_of(pics[name], name)], 37, out, want, s)


def test_patch_side_8(K, I, S):
    for name in ("i420", "uyvy", "p010"):
        pic = picture(I, S, name, 37, 53, seed=10)
        for s in ("left", "center"):
            want = yardstick(I, pic, (40, 56), s, patch=8)
            assert want[0].shape == (3, 35, 192)
            same(S, name, [t.cuda() for t in planes_of(pic, name)], 53, (40, 56), want, s, patch=8)


def test_matrices_and_ranges(K, I, S):
    for name, matrix, full in (("p010", "bt2020", False), ("yuy2", "bt709", True)):
        pic = picture(I, S, name, 37, 53, seed=8)
        views = [t.cuda() for t in planes_of(pic, name)]
        for s in SITINGS:
            want = yardstick(I, pic, (80, 112), s, matrix=matrix, full_range=full)
            assert not torch.equal(want[1], yardstick(I, pic, (80, 112), s)[1])
            same(S, name, views, 53, (80, 112), want, s, matrix=matrix, full_range=full)
            # and the frame's own CPU conversion is that frame
            f = make(S, name, views, 53, matrix=matrix, full_range=full, chroma="bilinear", siting=s)
            got = I.image_patch_planes(f.to("cpu").rgb().cuda(), (80, 112), P, MEAN, STD, want_pixels=True)
            assert torch.equal(got[1], want[1])


def test_rejections_launch_nothing(K, I, S):
    out = (80, 96)
    L = I._L()
    sentinel = torch.full((3, 2 * 30, 768), 7.0, dtype=torch.bfloat16, device="cuda")
    planes = sentinel.clone()

    def refused(src, cause, name):
        rc, _ = entry(I, src, 2, 48, 64, out, planes=planes)
        assert rc != 0 and cause in L.nos_image_last_error().decode(), (name, cause, L.nos_image_last_error())

    for name in ("i422", "p010", "yuy2", "i444", "nv24"):
        pic = Picture.of(I, S, name, 48, 64, batch=2, seed=11)
        views = [t.cuda() for t in pic.planes(name)]
        for chroma, siting, cause in ((2, 0, "unknown chroma reconstruction"), (-1, 0, "unknown chroma reconstruction"),
                                      (0, 4, "unknown chroma siting"), (1, 4, "unknown chroma siting"),
                                      (0, -1, "unknown chroma siting")):
            src = descriptor(I, S, name, views)
            assert (src.chroma, src.siting) == (0, 0)
            src.chroma, src.siting = chroma, siting
            refused(src, cause, (name, chroma, siting))
        if S.FORMATS[name][1] == "444":
            for siting in range(4):
                src = descriptor(I, S, name, views)
                src.chroma, src.siting = 1, siting
                refused(src, "bilinear chroma takes a subsampled source", (name, siting))
    torch.cuda.synchronize()
    assert torch.equal(planes, sentinel)                   # nothing was launched
    pic = Picture.of(I, S, "i422", 48, 64, 2)
    src = descriptor(I, S, "i422", [t.cuda() for t in pic.planes("i422")])
    src.chroma, src.siting = 1, 3
    rc, _ = entry(I, src, 2, 48, 64, out, planes=planes)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(planes, yardstick(I, pic, out, "topleft")[0])


def test_detect_image_of_a_bilinear_nv12_frame_eager_and_replayed(K, I, S, model, monkeypatch):
    from walkai_nos_amd.models.workload.processor import Nv12
    h, w, pitch = 48, 64, 96
    contents = [torch.randint(0, 256, (pitch * h * 3 // 2,), generator=torch.Generator().manual_seed(s),
                              dtype=torch.uint8) for s in (5, 6)]
    buf = contents[0].cuda()
    frame_ = Nv12.from_buffer(buf, h, w, pitch, matrix="bt709", chroma="bilinear", siting="center")
    base = buf.untyped_storage().data_ptr()
    assert all(getattr(frame_, p).untyped_storage().data_ptr() == base for p in frame_.PLANES)
    fused = Counter(monkeypatch, I, "yuv_semiplanar_patch_planes")
    converted = Counter(monkeypatch, I, "yuv_to_rgb")
    with torch.no_grad():
        s = model.detect_image(frame_, 0.0)["scores"][0].sort().values
        thr = 0.5 * (s[49] + s[50]).item()      # half of the rows survive on the first frame
        first = {k: v.clone() for k, v in model.detect_image(frame_, thr).items()}
        assert fused.n == 2 and converted.n == 0 and K.x3_active(model.pos_embed)
        want = model.detect_image(frame_.rgb(), thr)
        other = model.detect_image(Nv12.from_buffer(buf, h, w, pitch, matrix="bt709"), thr)
    assert first["count"].tolist() == [50] and {"logits", "pred_boxes"} <= set(want)
    for k, v in want.items():
        assert torch.equal(first[k], v), k
    assert not torch.equal(first["logits"], other["logits"])        # nearest chroma is another picture
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
        second = model.detect_image(frame_.rgb(), thr)
    for k, v in second.items():
        assert torch.equal(held[k], v), k
    assert not torch.equal(held["logits"], first["logits"])
    del graph
