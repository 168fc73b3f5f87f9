"""Tiled detection on the CPU: the tile plan, the torch reference of the cross-tile merge against an independent
double loop in fp64 (``tests/tiles_case.py``), the tile staging against the stacked crops, and ``detect_tiled`` on a
2-layer model. The HIP kernels are ``tests/test_gpu_tiles.py``'s."""
import itertools
import math

import pytest
import torch

import tiles_case as T
from walkai_nos_amd.models.workload.processor import Nv12, Packed, YolosProcessor
from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
from walkai_nos_amd.ops import image as I

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---- the plan -----------------------------------------------------------------------------------
def test_tile_plan_values():
    assert I.tile_plan(2160, 3840, (2, 2), 0.2) == (1200, 2134, [(0, 0), (0, 1706), (960, 0), (960, 1706)])
    assert I.tile_plan(97, 131, (3, 2), 0.3) == (41, 78, [(0, 0), (0, 53), (28, 0), (28, 53), (56, 0), (56, 53)])
    assert YolosProcessor.tile_plan((97, 131), (3, 2), 0.3) == I.tile_plan(97, 131, (3, 2), 0.3)
    assert I.tile_plan(480, 640, (1, 1)) == (480, 640, [(0, 0)])


def test_tile_plan_covers_the_axis():
    for n, k, ov in itertools.product((1, 2, 7, 16, 97, 131, 1000, 2160, 3840), (1, 2, 3, 4, 7),
                                      (0.0, 0.1, 0.2, 0.3, 0.5, 0.9)):
        t, _, origins = I.tile_plan(n, 5, (k, 1), ov, 1)
        ys = [y for y, _ in origins]
        assert len(ys) == k and 1 <= t <= n, (n, k, ov)
        assert ys[0] == 0 and ys[-1] + t == n, (n, k, ov, t, ys)
        assert all(a <= b <= a + t for a, b in zip(ys, ys[1:])), (n, k, ov, t, ys)   # ordered; touch or overlap
        if k == 1:
            assert t == n
        else:
            assert t == min(n, math.ceil(n / (k - (k - 1) * ov)))
        # the other axis is planned the same way
        assert I.tile_plan(5, n, (1, k), ov, 1) == (5, t, [(0, y) for y in ys])


def test_tile_plan_refuses():
    for bad in (dict(overlap=-0.1), dict(overlap=1.0), dict(tiles=(0, 2)), dict(tiles=(2, 0)), dict(tiles=(3, 4)),
                dict(tiles=(11, 1))):
        with pytest.raises(ValueError):
            I.tile_plan(480, 640, **{"tiles": (2, 2), "overlap": 0.2, **bad})
    assert len(I.tile_plan(480, 640, (2, 5))[2]) == 10       # 1000 rows fit, 1100 and 1200 do not
    with pytest.raises(ValueError):
        I.tile_plan(480, 640, (2, 2), 0.2, num_detection_tokens=257)


# ---- the merge ----------------------------------------------------------------------------------
@pytest.mark.parametrize("match", ("ios", "iou"))
@pytest.mark.parametrize("seed", (0, 1))
def test_merge_reference_matches_the_double_loop(seed, match):
    logits, boxes = T.synthetic(seed)
    kept, margins = T.merge_loop(logits, boxes, T.ORIGINS, T.TILE_HW, T.THRESHOLD, match, T.MATCH_THRESHOLD)
    T.decides_clearly(margins, T.THRESHOLD)
    assert len(kept) == (9 if match == "ios" else 11)
    N = logits.shape[0] * logits.shape[1]
    got = I.merge_detections_reference(logits.double(), boxes.double(), T.ORIGINS, T.TILE_HW, T.THRESHOLD, match,
                                       T.MATCH_THRESHOLD)
    assert got[1].dtype == torch.float64 and got[3].dtype == torch.float64
    T.check_merged(got, kept, N, 1e-12, 1e-9)
    # the two bit-identical rows (tiles 0 and 3) come out side by side, in tile order
    h = [i for i, k in enumerate(kept) if k[1] == 10]
    assert len(h) == 2 and h[1] == h[0] + 1 and [kept[i][3] for i in h] == [0, 3] and kept[h[0]][0] == kept[h[1]][0]
    # fp32 inputs, and the public entry on CPU tensors (which is the reference)
    got32 = I.merge_detections(logits, boxes, list(T.ORIGINS), T.TILE_HW, T.THRESHOLD, match, T.MATCH_THRESHOLD)
    assert got32[1].dtype == torch.float32
    T.check_merged(got32, kept, N, 1e-5, 1e-3)
    # the origins as a tensor
    again = I.merge_detections(logits, boxes, torch.tensor(T.ORIGINS), T.TILE_HW, T.THRESHOLD, match, T.MATCH_THRESHOLD)
    assert all(torch.equal(a, b) for a, b in zip(again, got32))


@pytest.mark.parametrize("match", ("ios", "iou"))
def test_merge_reference_on_a_dense_table(match):
    # 500 candidates of 1000 rows; under "ios" some survive only because the row that would have dropped them was
    # dropped itself (seed chosen so that the double loop decides clearly, which is asserted)
    logits, boxes = T.ramp(10, 100, seed=3, hole=True)
    origins = [(20 * b, 30 * b) for b in range(10)]
    dropped = []
    kept, margins = T.merge_loop(logits, boxes, origins, (100, 100), 0.3, match, 0.5, dropped)
    T.decides_clearly(margins, 0.3)
    assert len(kept) + len(dropped) == 500 and len(dropped) > 2
    assert match == "iou" or len(T.freed(kept, dropped, match, 0.5)) > 2
    got = I.merge_detections_reference(logits, boxes, origins, (100, 100), 0.3, match, 0.5)
    T.check_merged(got, kept, 1000, 1e-5, 1e-3)


def test_merge_of_one_tile_is_detections_sorted():
    g = torch.Generator().manual_seed(9)
    logits, boxes = 3.0 * torch.randn(1, 100, 92, generator=g), 0.2 + 0.6 * torch.rand(1, 100, 4, generator=g)
    logits[0, 40] = logits[0, 20]      # equal scores: token order
    count, scores, labels, xyxy = I.detections_reference(logits, boxes, torch.tensor([[37.0, 53.0]]), 0.3)
    n = count.item()
    assert 2 < n < 100
    order = torch.sort(-scores[0, :n], stable=True).indices
    got = I.merge_detections_reference(logits, boxes, [(0, 0)], (37, 53), 0.3)
    assert got[0].tolist() == [n]
    assert torch.equal(got[1][:n], scores[0, :n][order]) and torch.equal(got[2][:n], labels[0, :n][order])
    assert torch.equal(got[3][:n], xyxy[0, :n][order])
    assert not got[1][n:].any() and not got[2][n:].any() and not got[3][n:].any() and not got[4].any()
    # overlapping boxes of one tile never suppress each other: everything above the threshold is kept
    same = torch.cat((logits[:, :50], logits[:, :50]), 1), torch.cat((boxes[:, :50], boxes[:, :50]), 1)
    twice = I.merge_detections_reference(*same, [(0, 0)], (37, 53), 0.3)
    assert twice[0].item() == 2 * I.detections_reference(logits[:, :50], boxes[:, :50], torch.ones(1, 2), 0.3)[0].item()


def test_merge_extremes_and_argument_checks():
    logits, boxes = T.synthetic(0)
    N = logits.shape[0] * logits.shape[1]
    none = I.merge_detections(logits, boxes, T.ORIGINS, T.TILE_HW, 1.0)
    assert none[0].tolist() == [0] and not any(t.any() for t in none[1:])
    every = I.merge_detections(logits, boxes, T.ORIGINS, T.TILE_HW, 0.0, "ios", 1.0)     # nothing overlaps by more than 1
    assert every[0].tolist() == [N] and (every[1][:-1] >= every[1][1:]).all()
    with pytest.raises(ValueError):
        I.merge_detections(logits, boxes, T.ORIGINS, T.TILE_HW, 0.5, match="giou")
    with pytest.raises(ValueError):
        I.merge_detections(logits, boxes, T.ORIGINS[:3], T.TILE_HW, 0.5)
    res = YolosProcessor.results(*every[:4])
    assert len(res) == 1 and res[0]["scores"].shape == (N,) and res[0]["boxes"].shape == (N, 4) \
        and res[0]["labels"].dtype == torch.int64


# ---- the tiles ----------------------------------------------------------------------------------
def frame(h, w, C=3, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w)
    return torch.randint(0, 256, (h, w, C), generator=g, dtype=torch.uint8)


@pytest.mark.parametrize("order", ("rgb", "bgra"))
def test_tiled_patch_planes_is_packed_of_the_crops(order):
    C = I.PACKED_ORDERS[order][0]
    big = frame(110, 150, C)
    img = big[5:102, 9:140]                                   # a 97 x 131 crop view of a larger buffer
    th, tw, origins = I.tile_plan(97, 131, (3, 2), 0.3)
    out = YolosProcessor(80, 133).size((th, tw))
    assert (th, tw, out) == (41, 78, (64, 128))
    planes, px = I.tiled_patch_planes(img, order, origins, (th, tw), out, 16, MEAN, STD, want_pixels=True)
    crops = torch.stack([img[y:y + th, x:x + tw] for y, x in origins]).contiguous()
    want, wpx = I.packed_patch_planes(crops, order, out, 16, MEAN, STD, want_pixels=True)
    assert planes.shape == (3, 6 * 4 * 8, 768) and px.shape == (6, 3, 64, 128)
    assert torch.equal(planes, want) and torch.equal(px, wpx)
    only, nopx = I.tiled_patch_planes(img[None], order, origins, (th, tw), out, 16, MEAN, STD)
    assert nopx is None and torch.equal(only, want)
    for bad in ([(0, 54)], [(57, 0)], [(-1, 0)], []):
        with pytest.raises(ValueError):
            I.tiled_patch_planes(img, order, bad, (th, tw), out, 16, MEAN, STD)
    with pytest.raises(ValueError):
        I.tiled_patch_planes(torch.stack((img, img)), order, origins, (th, tw), out, 16, MEAN, STD)


# ---- the model ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from yolos_reference import randomize
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=2, use_mid_position_embeddings=True)).eval()
    randomize(m)
    m.invalidate_cache()
    m.processor = YolosProcessor(80, 133)
    return m


def test_detect_tiled_on_the_cpu(model):
    img = frame(97, 131)
    th, tw, origins = I.tile_plan(97, 131, (3, 2), 0.3)
    with torch.no_grad():
        out = model.detect_tiled(img, (3, 2), 0.3, 0.0, "ios", 0.5)
        crops = torch.stack([img[y:y + th, x:x + tw] for y, x in origins])
        logits, boxes = model(model.processor.preprocess(crops))
    assert out["tile_hw"] == (th, tw) and out["origins"].dtype == torch.int32 and out["origins"].tolist() == \
        [list(o) for o in origins]
    assert out["logits"].shape == (6, 100, 92) and out["pred_boxes"].shape == (6, 100, 4)
    assert torch.equal(out["logits"], logits) and torch.equal(out["pred_boxes"], boxes)
    s = torch.softmax(logits, -1)[..., :-1].max(-1).values.flatten().sort().values
    thr = 0.5 * (s[299] + s[300]).item()                     # half of the 600 rows are candidates
    assert s[300].item() - s[299].item() > 1e-6
    for match in ("ios", "iou"):
        with torch.no_grad():
            out = model.detect_tiled(img, (3, 2), 0.3, thr, match, 0.4)
        want = I.merge_detections_reference(logits, boxes, origins, (th, tw), thr, match, 0.4)
        for k, w in zip(("count", "scores", "labels", "boxes", "tile"), want):
            assert torch.equal(out[k], w), (match, k)
        assert 0 < out["count"].item() <= 300
    res = model.processor.results(out["count"], out["scores"], out["labels"], out["boxes"])
    assert len(res) == 1 and res[0]["scores"].shape[0] == out["count"].item()


def test_detect_tiled_takes_frames(model):
    img = frame(96, 128)
    with torch.no_grad():
        want = model.detect_tiled(img, (2, 2), 0.2, 0.0)
        bgr = model.detect_tiled(Packed(img.flip(-1).contiguous(), "bgr"), (2, 2), 0.2, 0.0)
        one = model.detect_tiled(img, (1, 1), 0.2, 0.0)
        whole = model.detect_image(img, 0.0)
    assert want["tile_hw"] == (54, 72) and want["logits"].shape[0] == 4
    for k in ("logits", "pred_boxes", "count", "scores", "labels", "boxes", "tile"):
        assert torch.equal(bgr[k], want[k]), k
    assert torch.equal(one["logits"], whole["logits"]) and torch.equal(one["pred_boxes"], whole["pred_boxes"])
    order = torch.sort(-whole["scores"][0], stable=True).indices
    assert one["count"].tolist() == [100] and torch.equal(one["scores"], whole["scores"][0][order])
    assert torch.equal(one["boxes"], whole["boxes"][0][order]) and torch.equal(one["labels"], whole["labels"][0][order])
    # any other frame is converted once by its rgb() and then tiled
    g = torch.Generator().manual_seed(3)
    nv = Nv12(torch.randint(0, 256, (96, 128), generator=g, dtype=torch.uint8),
              torch.randint(0, 256, (48, 64, 2), generator=g, dtype=torch.uint8))
    with torch.no_grad():
        a, b = model.detect_tiled(nv, (2, 2), 0.2, 0.0), model.detect_tiled(nv.rgb()[0], (2, 2), 0.2, 0.0)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["scores"], b["scores"])
    with pytest.raises(ValueError):
        model.detect_tiled(torch.stack((img, img)), (2, 2))
    with pytest.raises(ValueError):
        model.detect_tiled(img, (4, 3))
