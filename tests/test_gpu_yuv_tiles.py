"""Tiles of a YUV frame staged in place from its planes (``csrc/image.hip``'s ``image_patch_planes_yuv*_tiles``): every
layout, depth, chroma mode and transfer of the general YUV front end, bit for bit against the packed tile launch on
the frame's ``rgb()`` (``tests/yuv_tiles_case.py``: no tolerance anywhere), the C entry's argument checks, the shared
origin table, ``detect_tiled`` of YUV frames (eager, as a graph replay on a new frame, ``torch`` and ``f32`` mode) and
the pod client. In every equality test of the launch the composition it could fall back to is patched to raise."""
import ctypes
import json
import os
import subprocess
import sys
import time
from dataclasses import replace

import pytest
import torch

import yuv_tiles_case as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD, P = C.MEAN, C.STD, C.P


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


TO_RGB = ("yuv_to_rgb", "yuv_semiplanar_to_rgb", "yuyv_to_rgb", "nv12_to_rgb", "yuv420_to_rgb")


def forbid(m, I, names=TO_RGB + ("tile_crops", "pixels_reference")):
    """The composition the tiled functions fall back to raises: a silent fallback cannot pass."""
    def refuse(*a, **kw):
        raise AssertionError("the composition ran instead of the tile launch")
    for name in names:
        m.setattr(I, name, refuse)


def fused(I, monkeypatch, f, origins, tile_hw=C.TILE_HW, out_hw=C.OUT_HW):
    """``f.tile_planes`` with and without the pixels, the fallback forbidden."""
    with monkeypatch.context() as m:
        forbid(m, I)
        got = f.tile_planes(origins, tile_hw, out_hw, P, MEAN, STD, True)
        only = f.tile_planes(origins, tile_hw, out_hw, P, MEAN, STD)
        torch.cuda.synchronize()
    assert only[1] is None and torch.equal(only[0], got[0])
    return got


def equal_to_rgb_route(I, monkeypatch, frame, origins, tile_hw=C.TILE_HW, out_hw=C.OUT_HW):
    f = frame.to("cuda")
    want = C.reference(f, origins, tile_hw, out_hw)
    got = fused(I, monkeypatch, f, origins, tile_hw, out_hw)
    B = len(origins)
    assert got[0].shape == (3, B * (out_hw[0] // P) * (out_hw[1] // P), 3 * P * P) and got[1].shape == (B, 3) + out_hw
    assert C.same(got, want)
    return got


# ---- 1: every layout, nearest chroma ------------------------------------------------------------
@pytest.mark.parametrize("name", C.LAYOUTS)
def test_every_layout(K, I, monkeypatch, name):
    frame = C.make_frame(name)
    h, w = frame.shape[1:3]
    origins = C.corner_origins(h, w)
    assert origins[1][1] % 4 == 3 and origins[2][0] % 2 == 1 and origins[3] == (h - 56, w - 72)
    equal_to_rgb_route(I, monkeypatch, frame, origins)


# ---- 2: origin residues -------------------------------------------------------------------------
#: x0 covers every residue mod 4 at both parities of y0 (for YUY2 an odd x0 starts in the middle of a macropixel)
RESIDUES = [(0, 0), (1, 1), (2, 2), (3, 3), (41, 56), (40, 57), (41, 58), (40, 59)]


@pytest.mark.parametrize("name", ("nv12", "yuy2"))
def test_origin_residues(K, I, monkeypatch, name):
    assert sorted((y % 2, x % 4) for y, x in RESIDUES) == [(a, b) for a in (0, 1) for b in range(4)]
    equal_to_rgb_route(I, monkeypatch, C.make_frame(name, 1), RESIDUES)


# ---- 3: bilinear chroma clamps at the frame's edge ----------------------------------------------
@pytest.mark.parametrize("name,siting", [(n, s) for n in ("nv12", "i010") for s in ("left", "center", "topleft", "top")]
                         + [("i422", "left"), ("yuy2", "left")])
def test_bilinear_chroma_clamps_at_the_frame(K, I, monkeypatch, name, siting):
    frame = C.make_frame(name, 2, chroma="bilinear", siting=siting)
    origins = [(20, 28), (21, 31), (0, 0)]         # interior tiles (an even and an odd origin) and a corner
    got = equal_to_rgb_route(I, monkeypatch, frame, origins)
    # the even-origin tile's own planes as a frame: chroma clamped at the tile's edge, which is another picture
    alone = C.cropped(frame, 20, 28, *C.TILE_HW).to("cuda")
    assert alone.shape == (1, 56, 72, 3)
    wrong = C.reference(alone, [(0, 0)])
    n = got[0].shape[1] // 3
    assert not torch.equal(wrong[1][0], got[1][0]) and not torch.equal(wrong[0][:, :n], got[0][:, :n])
    # and the nearest route of the same samples differs from both (the mode reached the kernel)
    near = C.reference(replace(frame, chroma="nearest").to("cuda"), origins)
    assert not torch.equal(near[1], got[1])


# ---- 4: the footprint limit ---------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", (("nv12", {}), ("p010", dict(chroma="bilinear")), ("uyvy", {})))
def test_downscale_of_four_stays_fused(K, I, monkeypatch, name, kw):
    # 128 x 192 -> 32 x 48: scale 4 on both axes, 9 taps; a patch's footprint is 68 columns (66 rows), which at
    # x0 = 3 (mod 4) takes all 18 column groups of a row
    tabs = I._device_tables(128, 192, 32, 48, P, torch.device("cuda", torch.cuda.current_device()))
    assert tabs is not None and tabs[4:] == (66, 68) and tabs[5] <= I.YUV_MAX_FOOTPRINT
    frame = C.make_frame(name, 3, (162, 260), **kw)
    equal_to_rgb_route(I, monkeypatch, frame, [(33, 67), (0, 0), (34, 68)], (128, 192), (32, 48))


def test_past_scale_four_takes_the_composition(K, I, monkeypatch):
    # 132 x 196 -> 32 x 48 is past 4: the composition runs (not forbidden here) and is the same
    assert not I.fusable((132, 196), (32, 48), P)
    f = C.make_frame("nv12", 3, (162, 260)).to("cuda")
    origins = [(29, 63), (0, 0)]
    want = C.reference(f, origins, (132, 196), (32, 48))
    n = {"crops": 0}
    crops = I.tile_crops

    def spy(*a, **kw):
        n["crops"] += 1
        return crops(*a, **kw)
    monkeypatch.setattr(I, "tile_crops", spy)
    got = f.tile_planes(origins, (132, 196), (32, 48), P, MEAN, STD, True)
    assert n["crops"] == 1 and C.same(got, want)


# ---- 5: storage bounds --------------------------------------------------------------------------
def pitched(name, fill, kw):
    """A 98 x 132 frame of random samples at padded pitches inside one buffer of exactly the surface's bytes, padding
    and all: the first plane's first byte is the storage's first, the last plane's last byte its last. ``fill``: what
    the padding holds."""
    from walkai_nos_amd.models.workload import surfaces
    from walkai_nos_amd.models.workload.processor import Nv12, Yuv420p
    h, w = 98, 132
    if name == "nv12":
        size, make = (h + h // 2 - 1) * 160 + w, lambda b: Nv12.from_buffer(b, h, w, 160, **kw)
    elif name == "i420":
        size, make = h * 160 + (h - 1) * 96 + w // 2, lambda b: Yuv420p.from_buffer(b, h, w, 160, 96, **kw)
    elif name == "p010":
        size, make = (h + h // 2 - 1) * 320 + 2 * w, lambda b: surfaces.from_buffer("p010", b, h, w, 320, **kw)
    else:
        size, make = (h - 1) * 288 + 2 * w, lambda b: surfaces.from_buffer("yuy2", b, h, w, 288, **kw)
    buf = torch.full((size,), fill, dtype=torch.uint8)
    host = make(buf)
    src = C.make_frame({"i420": "yv12"}.get(name, name), 4, (h, w))      # the same samples for either fill
    for k in host.PLANES:
        getattr(host, k).copy_(getattr(src, k))
    dev = buf.cuda()
    assert dev.untyped_storage().nbytes() == size
    f = make(dev)
    first, last = getattr(f, f.PLANES[0]), getattr(f, f.PLANES[-1])
    lo = dev.untyped_storage().data_ptr()
    assert first.data_ptr() == lo
    end = last.data_ptr() + ((last.shape[0] - 1) * last.stride(0) + last[0].numel()) * last.element_size()
    assert end == lo + size
    return f


@pytest.mark.parametrize("name,kw", (("nv12", {}), ("nv12", dict(chroma="bilinear")), ("i420", dict(chroma="bilinear")),
                                     ("p010", {}), ("yuy2", dict(chroma="bilinear"))))
def test_storage_bounds(K, I, monkeypatch, name, kw):
    origins = C.corner_origins(98, 132)        # the first tile reads the first bytes, the last one the last
    got = []
    for fill in (0x00, 0xFF):
        f = pitched(name, fill, kw)
        want = C.reference(f, origins)
        got.append(fused(I, monkeypatch, f, origins))
        assert C.same(got[-1], want), fill
    assert C.same(got[0], got[1])


# ---- 6: HDR -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,transfer", (("p010", "pq"), ("p010", "hlg"), ("i422p12", "pq"), ("i444p12", "pq")))
@pytest.mark.parametrize("chroma", ("nearest", "bilinear"))
def test_hdr(K, I, monkeypatch, name, transfer, chroma):
    frame = C.make_frame(name, 5, transfer=transfer, peak_nits=800.0, matrix="bt2020", chroma=chroma, siting="topleft")
    origins = C.corner_origins(*frame.shape[1:3])
    got = equal_to_rgb_route(I, monkeypatch, frame, origins)
    sdr = C.reference(replace(frame, transfer="sdr").to("cuda"), origins)
    assert not torch.equal(sdr[1], got[1])


# ---- 7: argument checks through the C entry -----------------------------------------------------
def test_yuv_tile_launch_argument_checks(K, I):
    f = C.make_frame("nv12").to("cuda")
    dev = f.device
    origins = C.corner_origins(97, 131)
    L = I._L()
    y, uv = I.yuv_semiplanar_planes(f.y, f.uv, "420", 8)
    pairs = uv.as_strided((1, uv.shape[1], 2 * uv.shape[2]), (uv.stride(0), uv.stride(1), 1))
    src = I.yuv_src(I.YUV_SEMIPLANAR, (y, pairs), "420", 8, False, 0, I.yuv_table("bt601", False, 8))
    tabs = I._device_tables(56, 72, 32, 48, P, dev)
    planes = torch.empty(3, 4 * 6, 768, dtype=torch.bfloat16, device=dev)
    table = torch.tensor(origins, dtype=torch.int32).to(dev)
    F3 = ctypes.c_float * 3
    resized = I.NosYuvSrc.from_buffer_copy(src)
    resized.size += 4
    hdr = I.yuv_hdr(*I._hdr_device_tables("pq", 10, "bt2020", 1000.0, dev))

    def call(B=4, org=origins, tab=table.data_ptr(), host=True, fh=97, fw=131, frames=1, s=src, tables=None):
        flat = (ctypes.c_int * (2 * len(org)))(*[v for o in org for v in o]) if host else None
        return L.nos_image_patch_planes_yuv_tiles(ctypes.byref(s), tables, flat, tab, fh, fw, frames, planes.data_ptr(),
                                                  None, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(),
                                                  tabs[3].data_ptr(), 32, 48, I.TAPS, tabs[4], tabs[5], F3(1, 1, 1),
                                                  F3(0, 0, 0), B, 56, 72, 32, 48, P, 2, 3, 0,
                                                  torch.cuda.current_stream().cuda_stream)
    assert call() == 0
    torch.cuda.synchronize()
    good = planes.clone()
    assert C.same((good, None), f.tile_planes(origins, C.TILE_HW, C.OUT_HW, P, (0.0,) * 3, (1 / 255.0,) * 3))
    planes.fill_(3.0)
    outside = [list(origins) for _ in range(4)]
    outside[0][3] = (42, 59)          # one row too low
    outside[1][3] = (41, 60)          # one column too far right
    outside[2][0] = (-1, 0)
    outside[3][1] = (0, -1)
    for bad in (dict(frames=2), dict(frames=0), dict(tab=None), dict(host=False), dict(s=resized),
                dict(tables=ctypes.byref(hdr)), dict(B=0), dict(fh=96), dict(fw=130), dict(fh=0)) \
            + tuple(dict(org=o) for o in outside):
        assert call(**bad) == -1 and L.nos_image_last_error(), bad
    torch.cuda.synchronize()
    assert bool((planes == 3.0).all())          # nothing was launched


# ---- 8: the origin table ------------------------------------------------------------------------
def test_origin_table_is_shared_and_dropped(K, I, monkeypatch):
    f = C.make_frame("nv12").to("cuda")
    origins = C.corner_origins(97, 131)
    key = ("origins", tuple(origins), str(f.device))
    I.invalidate_cache()
    assert key not in I._tables
    built = []
    tensor = torch.tensor

    def spy(data, *a, **kw):
        if kw.get("dtype") == torch.int32 and isinstance(data, (tuple, list)) and tuple(data) == tuple(origins):
            built.append(1)
        return tensor(data, *a, **kw)
    monkeypatch.setattr(torch, "tensor", spy)
    f.tile_planes(origins, C.TILE_HW, C.OUT_HW, P, MEAN, STD)
    table = I._tables._d[key]
    assert table.dtype == torch.int32 and table.tolist() == [list(o) for o in origins] and built == [1]
    f.tile_planes(list(origins), C.TILE_HW, C.OUT_HW, P, MEAN, STD, True)
    logits, boxes = torch.zeros(4, 5, 3, device="cuda"), torch.full((4, 5, 4), 0.5, device="cuda")
    I.merge_detections(logits, boxes, origins, C.TILE_HW, 0.5)
    assert I.origin_tensor(origins, f.device) is table and I._tables._d[key] is table and built == [1]
    assert not any(k[0] == "tiles" for k in I._tables._d)       # no byte-offset table: that is the packed launch's
    I.invalidate_cache()
    assert key not in I._tables


# ---- 9: the model -------------------------------------------------------------------------------
def small_model():
    from yolos_reference import randomize
    from walkai_nos_amd.models.workload.processor import YolosProcessor
    from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=2, use_mid_position_embeddings=True)).eval()
    randomize(m)
    m.invalidate_cache()
    m.processor = YolosProcessor(80, 133)
    return m


@pytest.fixture(scope="module")
def model(K):
    return small_model().cuda()


KEYS = ("logits", "pred_boxes", "origins", "count", "scores", "labels", "boxes", "tile")
MODEL_FRAMES = (("nv12", dict(chroma="bilinear")), ("p010", dict(transfer="pq", matrix="bt2020")))


def no_conversion(m, I, frame):
    def refuse(*a, **kw):
        raise AssertionError("the frame was converted to RGB")
    m.setattr(type(frame), "rgb", refuse)
    forbid(m, I, TO_RGB)


def threshold(model, rgb):
    """Between the 200th and the 201st of the 400 rows' scores."""
    c = torch.softmax(model.detect_tiled(rgb, (2, 2), 0.2, 0.0)["logits"], -1)[..., :-1].max(-1).values
    c = c.flatten().sort().values
    assert c[200].item() - c[199].item() > 1e-6
    return 0.5 * (c[199] + c[200]).item()


@pytest.mark.parametrize("name,kw", MODEL_FRAMES)
def test_detect_tiled_stages_yuv_in_place(K, I, model, monkeypatch, name, kw):
    first, second = (C.make_frame(name, s, (96, 128), **kw).to("cuda") for s in (6, 7))
    with torch.no_grad():
        thr = threshold(model, first.rgb()[0])
        want = {k: v.clone() for k, v in model.detect_tiled(first.rgb()[0], (2, 2), 0.2, thr).items() if k in KEYS}
        other = {k: v.clone() for k, v in model.detect_tiled(second.rgb()[0], (2, 2), 0.2, thr).items() if k in KEYS}
    assert want["logits"].shape == (4, 100, 92) and 0 < want["count"].item() <= 200
    assert not torch.equal(want["logits"], other["logits"])
    with monkeypatch.context() as m:
        no_conversion(m, I, first)
        with torch.no_grad():
            got = model.detect_tiled(first, (2, 2), 0.2, thr)
            torch.cuda.synchronize()
            for k in KEYS:
                assert torch.equal(got[k], want[k]), k
            # one graph, replayed on a new frame written into the same plane buffers
            stream = torch.cuda.Stream()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                held = model.detect_tiled(first, (2, 2), 0.2, thr)
        for k in KEYS:
            held[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(held[k], want[k]), k
        for k in first.PLANES:
            getattr(first, k).copy_(getattr(second, k))
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(held[k], other[k]), k
        del graph


@pytest.mark.parametrize("mode", ("torch", "f32"))
def test_detect_tiled_of_yuv_elsewhere(K, I, model, monkeypatch, mode):
    frame = C.make_frame("nv12", 6, (96, 128), chroma="bilinear").to("cuda")
    calls = []
    launch = I.yuv_semiplanar_tiled_patch_planes
    monkeypatch.setattr(I, "yuv_semiplanar_tiled_patch_planes", lambda *a, **kw: calls.append(1) or launch(*a, **kw))
    if mode == "torch":
        K.set_backend("torch")
    else:
        K.set_fp32_matmul("f32")
    try:
        with torch.no_grad():
            got = model.detect_tiled(frame, (2, 2), 0.2, 0.3)
            want = model.detect_tiled(frame.rgb()[0], (2, 2), 0.2, 0.3)
    finally:
        K.set_backend("hip")
        K.set_fp32_matmul("x3")
    assert not calls
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k


# ---- 10: the pod client (last: it starts processes, and nothing follows them if one fails) --------
@pytest.mark.parametrize("extra", (("--pixel-format", "nv12"),
                                   ("--pixel-format", "p010", "--transfer", "pq", "--peak-nits", "600",
                                    "--matrix", "bt2020")))
def test_pod_client_tiles_of_yuv(extra):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "walkai_nos_amd.dataplane.client", "--end-to-end",
           "--tiles", "2,2", "--tile-overlap", "0.2", "--threshold", "0.0", "--match-threshold", "1.0",
           "--image-hw", "96,128", "--size", "80,133", "--seconds", "1", *extra]
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert p.stdout.readline().strip() == "READY"
        p.stdin.write(f"GO {time.time()}\n")
        p.stdin.flush()
        out = json.loads(p.stdout.readline())
        assert p.wait(timeout=60) == 0
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    assert out["end_to_end"] is True and out["tiles"] == 4 and out["tile_hw"] == [54, 72]
    assert out["input_hw"] == [80, 96]
    assert out["detections"] == 400 and out["inferences"] > 0      # nothing is dropped at match threshold 1
    print(f"[yuv tiles] client --tiles 2,2 {extra[1]} 96x128 -> 4 x 80x96: {out['inferences']} inferences in "
          f"{out['window_s']} s, mean {out['latency_ms']['mean']} ms")
