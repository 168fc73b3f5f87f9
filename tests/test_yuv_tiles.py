"""Tiles of a YUV frame on the CPU: ``ops.image.yuv_*_tiled_patch_planes`` and ``Frame.tile_planes`` of every frame
class against ``image_patch_planes`` of the crops of ``rgb()`` (bit for bit: on the CPU they are that composition),
what they refuse, and ``detect_tiled`` of YUV frames on a 2-layer model. The HIP launch is
``tests/test_gpu_yuv_tiles.py``'s."""
import pytest
import torch

import yuv_tiles_case as C
from walkai_nos_amd.models.workload import surfaces
from walkai_nos_amd.models.workload.processor import Frame, Packed, YolosProcessor
from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
from walkai_nos_amd.ops import image as I

MEAN, STD, P = C.MEAN, C.STD, C.P


def crops_reference(frame, origins, want_pixels=True):
    crops = I.tile_crops(frame.rgb(), origins, C.TILE_HW)
    return I.image_patch_planes(crops, C.OUT_HW, P, MEAN, STD, want_pixels)


def ops_call(frame, origins, want_pixels=True, **over):
    """The ops function of the frame's layout, with the frame's fields."""
    f = frame
    if isinstance(f, surfaces.Yuyv):
        kw = dict(matrix=f.matrix, full_range=f.full_range, want_pixels=want_pixels, chroma=f.chroma, siting=f.siting)
        kw.update(over)
        return I.yuyv_tiled_patch_planes(f.data, f.width, f.order, origins, C.TILE_HW, C.OUT_HW, P, MEAN, STD, **kw)
    kw = dict(subsampling=getattr(f, "subsampling", "420"), depth=getattr(f, "depth", 8), msb=getattr(f, "msb", False),
              matrix=f.matrix, full_range=f.full_range, want_pixels=want_pixels, chroma=f.chroma, siting=f.siting,
              transfer=f.transfer, peak_nits=getattr(f, "peak_nits", 1000.0))
    kw.update(over)
    if "uv" in f.PLANES:
        return I.yuv_semiplanar_tiled_patch_planes(f.y, f.uv, origins, C.TILE_HW, C.OUT_HW, P, MEAN, STD, vu=f.vu, **kw)
    return I.yuv_planar_tiled_patch_planes(f.y, f.u, f.v, origins, C.TILE_HW, C.OUT_HW, P, MEAN, STD, **kw)


@pytest.mark.parametrize("name", C.LAYOUTS)
def test_tiles_equal_the_crops_of_rgb(name):
    frame = C.make_frame(name)
    h, w = frame.shape[1:3]
    origins = C.corner_origins(h, w)
    want = crops_reference(frame, origins)
    assert want[0].shape == (3, 4 * 2 * 3, 768) and want[1].shape == (4, 3, 32, 48)
    assert C.same(ops_call(frame, origins), want)
    assert C.same(frame.tile_planes(origins, C.TILE_HW, C.OUT_HW, P, MEAN, STD, True), want)
    only = frame.tile_planes(origins, C.TILE_HW, C.OUT_HW, P, MEAN, STD)
    assert only[1] is None and torch.equal(only[0], want[0])
    assert C.same(C.reference(frame, origins), want)


@pytest.mark.parametrize("name,kw", (("nv12", dict(chroma="bilinear", siting="center")),
                                     ("i420", dict(chroma="bilinear", siting="topleft")),
                                     ("yuy2", dict(chroma="bilinear")),
                                     ("p010", dict(transfer="pq", peak_nits=600.0, matrix="bt2020")),
                                     ("i422p12", dict(transfer="hlg", chroma="bilinear", matrix="bt2020"))))
def test_tiles_with_chroma_and_transfer(name, kw):
    frame = C.make_frame(name, 1, **kw)
    origins = C.corner_origins(*frame.shape[1:3])
    want = crops_reference(frame, origins)
    assert not C.same(crops_reference(C.make_frame(name, 1), origins), want)      # the fields matter
    assert C.same(ops_call(frame, origins), want)
    assert C.same(frame.tile_planes(origins, C.TILE_HW, C.OUT_HW, P, MEAN, STD, True), want)


def test_base_class_and_packed_frames():
    class Gray(Frame):
        """A frame class that knows nothing of tiles: the base class converts it."""
        PLANES = ("y",)

        def __init__(self, y):
            self.y = y

        def rgb(self):
            return self.y[None, :, :, None].expand(1, -1, -1, 3).contiguous()

    g = torch.Generator().manual_seed(5)
    y = torch.randint(0, 256, (97, 131), generator=g, dtype=torch.uint8)
    origins = C.corner_origins(97, 131)
    want = crops_reference(Gray(y), origins)
    assert C.same(Gray(y).tile_planes(origins, C.TILE_HW, C.OUT_HW, P, MEAN, STD, True), want)
    bgra = torch.cat((Gray(y).rgb()[0].flip(-1), torch.full((97, 131, 1), 77, dtype=torch.uint8)), -1)
    assert C.same(Packed(bgra, "bgra").tile_planes(origins, C.TILE_HW, C.OUT_HW, P, MEAN, STD, True), want)
    proc = YolosProcessor()
    assert C.same(proc.frame_tile_planes(Gray(y), origins, C.TILE_HW, C.OUT_HW, True), want)


@pytest.mark.parametrize("name", ("nv12", "i422", "yuy2", "p010"))
def test_tiles_refuse(name):
    frame = C.make_frame(name)
    h, w = frame.shape[1:3]
    good = C.corner_origins(h, w)
    assert ops_call(frame, good, False)[0].shape[1] == 24
    for bad in ([(h - 55, 0)], [(0, w - 71)], [(-1, 0)], [(0, -1)], good + [(h, w)], []):
        with pytest.raises(ValueError):
            ops_call(frame, bad)
        with pytest.raises(ValueError):
            frame.tile_planes(bad, C.TILE_HW, C.OUT_HW, P, MEAN, STD)
    for over in (dict(chroma="cubic"), dict(siting="bottom")) + \
            (() if name == "yuy2" else (dict(transfer="gamma"), dict(transfer="pq") if name != "p010" else
                                         dict(transfer="pq", peak_nits=100.0))):
        with pytest.raises(ValueError):
            ops_call(frame, good, **over)
    # a batch of two frames
    from dataclasses import replace
    two = replace(frame, **{k: torch.stack((getattr(frame, k),) * 2) for k in frame.PLANES})
    assert two.shape[0] == 2
    with pytest.raises(ValueError):
        ops_call(two, good)
    with pytest.raises(ValueError):
        two.tile_planes(good, C.TILE_HW, C.OUT_HW, P, MEAN, STD)


# ---- the model ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from yolos_reference import randomize
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=2, use_mid_position_embeddings=True)).eval()
    randomize(m)
    m.invalidate_cache()
    m.processor = YolosProcessor(80, 133)
    return m


KEYS = ("logits", "pred_boxes", "origins", "count", "scores", "labels", "boxes", "tile")


@pytest.mark.parametrize("name,kw", (("nv12", {}), ("p010", dict(transfer="pq", matrix="bt2020")), ("yuy2", {})))
def test_detect_tiled_of_yuv_frames_on_the_cpu(model, name, kw):
    frame = C.make_frame(name, 2, (96, 128), **kw)
    with torch.no_grad():
        a = model.detect_tiled(frame, (2, 2), 0.2, 0.0)
        b = model.detect_tiled(frame.rgb()[0], (2, 2), 0.2, 0.0)
    assert a["tile_hw"] == b["tile_hw"] == (54, 72) and a["logits"].shape == (4, 100, 92)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    from dataclasses import replace
    two = replace(frame, **{k: torch.stack((getattr(frame, k),) * 2) for k in frame.PLANES})
    with pytest.raises(ValueError):
        model.detect_tiled(two, (2, 2))
