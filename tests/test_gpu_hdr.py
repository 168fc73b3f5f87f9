"""PQ and HLG frames in the fused image kernel (``csrc/image.hip``'s ``hdr_pixel`` behind
``nos_image_patch_planes_yuv_hdr``), on the GPU: each of the six instantiations against the RGB kernel on the frame
converted on the CPU by the definition (``ops.image.hdr_to_sdr`` behind ``Frame.rgb()``, itself checked in
``test_hdr_tables.py``). The method is ``test_gpu_surfaces.py``'s, whose pictures and helpers are used: integers and
tables in front of a shared body, so planes and pixels are compared with ``torch.equal`` — no tolerance; seeded random
planes with random ignored bits in every 16-bit word; patch 16. Every result is also required to differ from the
``transfer="sdr"`` result of the same planes. Bounds are shown by results that do not depend on the pad bytes around a
plane and by planes that begin and end on their storage's first and last byte, never by a fault."""
import ctypes

import pytest
import torch
from test_gpu_surfaces import (CASES, IDS, MEAN, STD, Counter, I, K, P, Picture, S, descriptor,  # noqa: F401
                               frame, model, pitched)

pytestmark = pytest.mark.gpu

#: one format per instantiation — (planar, semi-planar) x (4:4:4, subsampled) with nearest chroma, and the two layouts
#: with bilinear chroma — then depth 12; the ``p`` names have the value in the high bits, the ``i`` names in the low
NAMES = {"i410": {}, "i010": {}, "p410": {}, "p010": {},
         "i210": {"chroma": "bilinear", "siting": "center"}, "p210": {"chroma": "bilinear", "siting": "left"},
         "p012": {}, "i012": {}}
#: both transfers, each with the gamut step applied (bt2020) and as the identity (bt709)
KINDS = [{"transfer": t, "matrix": m} for t in ("pq", "hlg") for m in ("bt2020", "bt709")]
FUSED = CASES[:2]


def want_of(I, S, name, cpu, w, out, **kw):
    """The RGB kernel on the frame converted on the CPU: ``(planes, pixels)`` on the GPU, and the converted frame."""
    rgb = frame(S, name, cpu, w, **kw).rgb()
    assert not rgb.is_cuda and rgb.dtype == torch.uint8
    return I.image_patch_planes(rgb.cuda(), out, P, MEAN, STD, want_pixels=True), rgb


def same(S, name, views, w, out, want, **kw):
    f = frame(S, name, views, w, **kw)
    got, px = f.patch_planes(out, P, MEAN, STD, True)
    only, none = f.patch_planes(out, P, MEAN, STD)
    torch.cuda.synchronize()
    assert none is None and got.dtype == torch.bfloat16 and px.dtype == torch.float32
    assert torch.equal(px, want[1]), f"{name} {kw}: pixels"
    assert torch.equal(got, want[0]) and torch.equal(only, want[0]), f"{name} {kw}: planes"
    return got, px


@pytest.mark.parametrize("case", FUSED, ids=IDS[:2])
@pytest.mark.parametrize("name", NAMES)
def test_hdr_equals_the_rgb_kernel_on_the_converted_frame(K, I, S, monkeypatch, name, case):
    h, w, H, W, fused = case
    assert fused
    # a batch of two once per layout, so that a wrong batch stride shows
    batch = 2 if (name in ("p010", "i210") and case is CASES[1]) else 1
    pic = Picture.of(I, S, name, h, w, batch=batch)
    cpu = pic.planes(name)
    views = [t.cuda() for t in cpu]
    wants = [want_of(I, S, name, cpu, w, (H, W), **NAMES[name], **kind) for kind in KINDS]
    fallback = Counter(monkeypatch, I, "yuv_to_rgb")
    for kind, (want, rgb) in zip(KINDS, wants):
        # the converted frame exercises the second table: at least half of the byte values occur
        assert len(torch.unique(rgb)) >= 128, (name, kind)
        sdr = frame(S, name, views, w, matrix=kind["matrix"], **NAMES[name]).patch_planes((H, W), P, MEAN, STD, True)
        got, px = same(S, name, views, w, (H, W), want, **NAMES[name], **kind)
        # the new code ran: not the sdr result of the same planes
        assert not torch.equal(px, sdr[1]) and not torch.equal(got, sdr[0]), (name, kind)
        if batch == 2:
            assert not torch.equal(px[0], px[1])
    assert fallback.n == 0
    # the transfers and the gamut step are told apart
    assert len({rgb.numpy().tobytes() for _, rgb in wants}) == len(KINDS)


def test_peak_nits_is_an_argument_of_the_launch(K, I, S, monkeypatch):
    pic = Picture.of(I, S, "p010", 37, 53, seed=3)
    cpu = pic.planes("p010")
    views = [t.cuda() for t in cpu]
    fallback = Counter(monkeypatch, I, "yuv_to_rgb")
    seen = []
    for peak in (1000.0, 400.0, 4000.0):
        kw = dict(transfer="pq", matrix="bt2020", peak_nits=peak)
        want, _ = want_of(I, S, "p010", cpu, 53, (80, 112), **kw)
        fallback.n = 0
        seen.append(same(S, "p010", views, 53, (80, 112), want, **kw)[1])
        assert fallback.n == 0
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[2])


@pytest.mark.parametrize("hw", ((1, 1), (2, 2), (3, 2), (2, 5)), ids=lambda s: "{}x{}".format(*s))
def test_the_smallest_sources(K, I, S, monkeypatch, hw):
    # chroma planes of one or two rows and columns: every tap clamps; a luma code at each end of its range, so the
    # matrix's sums leave the table at both ends and are clamped to its first and last entry
    h, w = hw
    assert I.fusable(hw, (16, 16), P)
    modes = ({}, {"chroma": "bilinear", "siting": "topleft"}, {"chroma": "bilinear", "siting": "center"})
    fallback = Counter(monkeypatch, I, "yuv_to_rgb")
    for name in ("p010", "i010"):
        pic = Picture.of(I, S, name, h, w, batch=2, seed=1)
        pic.y[0, 0, 0], pic.y[1, 0, 0] = 0, (1 << pic.depth) - 1
        cpu = pic.planes(name)
        views = [t.cuda() for t in cpu]
        for mode in modes:
            for kind in (KINDS[0], KINDS[3]):
                want, rgb = want_of(I, S, name, cpu, w, (16, 16), **mode, **kind)
                assert rgb[0].min() == 0 and rgb[1].max() == 255
                fallback.n = 0              # (the CPU frame's conversion is the definition's)
                same(S, name, views, w, (16, 16), want, **mode, **kind)
                assert fallback.n == 0


def test_pitches_alignment_and_storage_ends(K, I, S, monkeypatch):
    # the reads are stage_yuv's and chroma_window's; the tables are read by index, whatever the planes' addresses
    out = (80, 112)
    modes = ({"transfer": "pq", "matrix": "bt2020"},
             {"transfer": "hlg", "matrix": "bt2020", "chroma": "bilinear", "siting": "left"})
    planes = {name: Picture.of(I, S, name, 37, 53, batch=2, seed=2).planes(name) for name in ("p010", "i010")}
    wanted = {name: [want_of(I, S, name, cpu, 53, out, **mode)[0] for mode in modes] for name, cpu in planes.items()}
    fallback = Counter(monkeypatch, I, "yuv_to_rgb")
    for name, cpu in planes.items():
        wants = wanted[name]
        # per plane a pitch of its own and a first byte 2 bytes into the storage (2-aligned, not 4-aligned); trailing
        # slack, and none (the plane's last byte is the storage's last byte, the first its first)
        for leads, extra, tail in (((2, 2, 2), (22, 10, 18), 10), ((2, 2, 2), (0, 0, 0), 0), ((0, 0, 0), (0, 0, 0), 0),
                                   ((0, 0, 0), (6, 2, 10), 0)):
            for mode, want in zip(modes, wants):
                results = []
                for pad in (0x00, 0xFF):
                    views = [pitched(t, t.shape[2] + e, pad, ld, tail) for t, ld, e in zip(cpu, leads, extra)]
                    for v, ld in zip(views, leads):
                        st = v.untyped_storage()
                        assert v.data_ptr() - st.data_ptr() == ld
                        if tail == 0:
                            last = v.data_ptr() + (v.shape[0] - 1) * v.stride(0) + (v.shape[1] - 1) * v.stride(1) \
                                + v.shape[2]
                            assert last == st.data_ptr() + st.nbytes()
                    results.append(same(S, name, views, 53, out, want, **mode))
                assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert fallback.n == 0


def hdr_entry(I, src, hdr, B, h, w, out, planes=None):
    """The library's HDR entry through ctypes with both descriptors as given. Returns ``(rc, planes)``."""
    H, W = out
    tabs = I._device_tables(h, w, H, W, P, torch.device("cuda", torch.cuda.current_device()))
    gh, gw = H // P, W // P
    if planes is None:
        planes = torch.empty(3, B * gh * gw, 3 * P * P, dtype=torch.bfloat16, device="cuda")
    rc = I._L().nos_image_patch_planes_yuv_hdr(ctypes.byref(src) if src is not None else None,
                                               ctypes.byref(hdr) if hdr is not None else None,
                                               *I._tail_args(tabs, planes, None, MEAN, STD, B, h, w, H, W, P, gh, gw))
    return rc, planes


def test_rejections_launch_nothing(K, I, S):
    out = (80, 96)
    L = I._L()
    dev = torch.device("cuda", torch.cuda.current_device())
    sentinel = torch.full((3, 2 * 30, 768), 7.0, dtype=torch.bfloat16, device="cuda")
    planes = sentinel.clone()
    tables = {d: I._hdr_device_tables("pq", d, "bt2020", 1000.0, dev) for d in (10, 12)}

    def refused(src, hdr, cause, what):
        rc, _ = hdr_entry(I, src, hdr, 2, 48, 64, out, planes=planes)
        assert rc != 0 and cause in L.nos_image_last_error().decode(), (what, cause, L.nos_image_last_error())

    for name in ("p010", "i012", "i210"):
        depth = S.FORMATS[name][2]
        pic = Picture.of(I, S, name, 48, 64, batch=2, seed=11)
        views = [t.cuda() for t in pic.planes(name)]
        src = descriptor(I, S, name, views)
        fresh = lambda: I.yuv_hdr(*tables[depth])       # noqa: E731
        assert fresh().entries == 1 << depth
        refused(src, None, "null operand", name)
        refused(None, fresh(), "null operand", name)
        for delta in (4, -4):
            hdr = fresh()
            hdr.size += delta
            refused(src, hdr, "table descriptor size", name)
        for entries in (0, (1 << depth) - 1, 1 << (22 - depth), 1 << 16):
            hdr = fresh()
            hdr.entries = entries
            refused(src, hdr, "2^depth entries", (name, entries))
        refused(src, I.yuv_hdr(*tables[22 - depth]), "2^depth entries", name)       # the other depth's tables
        for field in ("lut1", "lut2"):
            hdr = fresh()
            setattr(hdr, field, None)
            refused(src, hdr, "null table", (name, field))
        for k, value in ((0, 1 << 15), (4, -(1 << 15)), (8, 1 << 20)):
            hdr = fresh()
            hdr.gamut[k] = value
            refused(src, hdr, "gamut coefficients", (name, k))
        # every check of the general entry is made here too
        bad = descriptor(I, S, name, views)
        bad.size += 4
        refused(bad, fresh(), "descriptor size", name)
        bad = descriptor(I, S, name, views)
        bad.plane[len(views) - 1].hi -= 1
        refused(bad, fresh(), "storage bounds", name)
        bad = descriptor(I, S, name, views)
        bad.chroma = 2
        refused(bad, fresh(), "unknown chroma reconstruction", name)
    # 8-bit and packed sources have no HDR form
    for name in ("i422", "nv24", "yuy2"):
        pic = Picture.of(I, S, name, 48, 64, batch=2, seed=11)
        src = descriptor(I, S, name, [t.cuda() for t in pic.planes(name)])
        for depth in (10, 12):
            refused(src, I.yuv_hdr(*tables[depth]), "16-bit samples", name)
    torch.cuda.synchronize()
    assert torch.equal(planes, sentinel)                   # nothing was launched
    pic = Picture.of(I, S, "p010", 48, 64, batch=2, seed=11)
    cpu = pic.planes("p010")
    src = descriptor(I, S, "p010", [t.cuda() for t in cpu])
    src.tab[:] = I.yuv_table("bt2020", False, 10)
    rc, _ = hdr_entry(I, src, I.yuv_hdr(*tables[10]), 2, 48, 64, out, planes=planes)
    torch.cuda.synchronize()
    want, _ = want_of(I, S, "p010", cpu, 64, out, transfer="pq", matrix="bt2020")
    assert rc == 0 and torch.equal(planes, want[0])


def test_detect_image_of_a_pq_p010_frame_eager_and_replayed(K, I, S, model, monkeypatch):
    h, w, pitch = 48, 64, 160                                # rows of 128 bytes on a pitched surface
    contents = [torch.randint(0, 256, (pitch * h * 3 // 2,), generator=torch.Generator().manual_seed(s),
                              dtype=torch.uint8) for s in (5, 6)]
    buf = contents[0].cuda()
    frame_ = S.from_buffer("p010", buf, h, w, pitch, matrix="bt2020", transfer="pq")
    base = buf.untyped_storage().data_ptr()
    assert all(getattr(frame_, p).untyped_storage().data_ptr() == base for p in frame_.PLANES)
    fused = Counter(monkeypatch, I, "yuv_semiplanar_patch_planes")
    converted = Counter(monkeypatch, I, "yuv_to_rgb")
    with torch.no_grad():
        s = model.detect_image(frame_, 0.0)["scores"][0].sort().values
        thr = 0.5 * (s[49] + s[50]).item()      # half of the rows survive on the first frame
        first = {k: v.clone() for k, v in model.detect_image(frame_, thr).items()}
        assert fused.n == 2 and converted.n == 0 and K.x3_active(model.pos_embed)
        want = model.detect_image(frame_.to("cpu").rgb().cuda(), thr)
        other = model.detect_image(S.from_buffer("p010", buf, h, w, pitch, matrix="bt2020"), thr)
    assert first["count"].tolist() == [50]
    assert {"logits", "pred_boxes", "count", "scores", "labels", "boxes"} <= set(want)
    for k, v in want.items():
        assert torch.equal(first[k], v), k
    assert not torch.equal(first["logits"], other["logits"])        # read as sdr it is another picture
    key = ("pq", 10, "bt2020", 1000.0, str(buf.device))
    assert key in I._hdr_tables
    torch.cuda.synchronize()
    made = Counter(monkeypatch, I, "_make_hdr_tables")
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=stream):
        held = model.detect_image(frame_, thr)
    # the tables were there already (no host copy under capture), and the graph keeps them
    assert made.n == 0 and I._hdr_tables.pinned(key)
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
        again = model.detect_image(frame_.to("cpu").rgb().cuda(), thr)
    for k, v in second.items():
        assert torch.equal(held[k], v), k
        assert torch.equal(again[k], v), k
    assert not torch.equal(held["logits"], first["logits"])
    del graph
