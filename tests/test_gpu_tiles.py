"""Tiled detection on the GPU (``csrc/image.hip``): the tile staging launch bit for bit against the packed launch on
the stacked crops, the merge kernel against the fp64 double loop of ``tests/tiles_case.py``, ``detect_tiled`` end to
end (eager, as one replay of a captured graph, with the ``torch`` backend and in ``f32`` mode) and the pod client's
``--tiles``. The conventions are ``tests/test_gpu_image.py``'s: its pixel bound (``FACTOR * err_ref``, never more
than ``CAP``), the project's bounds for ``detections`` (scores 1e-5, boxes 1e-3 px) and, for the model, the suite's
yardstick (``tests/yolos_reference.py``: ``4 * err_ref``, floor ``2e-6 * max(1, |ref|max)``)."""
import ctypes
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import tiles_case as T
from kernel_inputs import Worst

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
P = 16
FACTOR, CAP = 2.0, 1e-4        # tests/test_gpu_image.py's pixel bound
SCORE_TOL = 1e-5


def box_tol(frame_hw):
    return max(5 * 2.0 ** -24 * max(frame_hw), 1e-3)


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


def u8_frame(h, w, C=3, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w + C)
    return torch.randint(0, 256, (h, w, C), generator=g, dtype=torch.uint8)


class Counter:
    def __init__(self, monkeypatch, owner, name):
        self.n = 0
        fn = getattr(owner, name)

        def spy(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        monkeypatch.setattr(owner, name, spy)


def tiles_equal_crops(I, monkeypatch, img, order, tiles, overlap, rule, want_plan, fused=True):
    """One tile launch on ``img`` (a device view ``[h, w, C]``) against the packed launch on the contiguous stacked
    crops: planes and pixels bit for bit, with and without the pixels."""
    from walkai_nos_amd.models.workload.processor import YolosProcessor
    h, w = img.shape[:2]
    th, tw, origins = I.tile_plan(h, w, tiles, overlap)
    out = YolosProcessor(*rule).size((th, tw))
    assert (th, tw, [y for y, _ in origins[::tiles[1]]], [x for _, x in origins[:tiles[1]]], out) == want_plan
    crops = torch.stack([img[y:y + th, x:x + tw] for y, x in origins]).contiguous()
    want, wpx = I.packed_patch_planes(crops, order, out, P, MEAN, STD, want_pixels=True)
    fallback = Counter(monkeypatch, I, "packed_patch_planes")
    planes, px = I.tiled_patch_planes(img, order, origins, (th, tw), out, P, MEAN, STD, want_pixels=True)
    only, none = I.tiled_patch_planes(img[None], order, origins, (th, tw), out, P, MEAN, STD)
    torch.cuda.synchronize()
    assert fallback.n == (0 if fused else 2) and none is None
    B = len(origins)
    assert planes.shape == (3, B * (out[0] // P) * (out[1] // P), 3 * P * P) and px.shape == (B, 3) + out
    assert torch.equal(planes, want) and torch.equal(px, wpx) and torch.equal(only, want)
    return crops, px, out


# ---- the tile launch ----------------------------------------------------------------------------
def test_tiles_of_a_contiguous_rgb_frame(K, I, monkeypatch):
    # 97 x 131 at (3, 2): tiles of 41 x 78 at rows 0, 28, 56 and columns 0, 53, upscaled to 64 x 128. Byte offset
    # 53 * 3 and the pitch 393 are odd, so every alignment of the staging loads occurs, and the last tile ends on the
    # last byte of the storage.
    img = u8_frame(97, 131).cuda()
    assert img.untyped_storage().nbytes() == 97 * 131 * 3
    tiles_equal_crops(I, monkeypatch, img, "rgb", (3, 2), 0.3, (80, 133), (41, 78, [0, 28, 56], [0, 53], (64, 128)))


@pytest.mark.parametrize("order", ("bgr", "bgra"))
def test_tiles_of_a_downscaled_frame(K, I, monkeypatch, order):
    # 250 x 330 at (2, 2): tiles of 139 x 184 down to 48 x 48 (scales 2.9 and 3.8, up to 9 taps); bgr contiguous,
    # bgra with a padded pitch as a crop out of a larger buffer
    if order == "bgr":
        img = u8_frame(250, 330).cuda()
    else:
        buf = u8_frame(260, 350, 4).cuda()
        img = buf[7:257, 11:341]
        assert img.stride(0) == 1400 and not img.is_contiguous()
    tiles_equal_crops(I, monkeypatch, img, order, (2, 2), 0.2, (48, 133), (139, 184, [0, 111], [0, 146], (48, 48)))


def test_tiles_past_the_tap_limit_take_the_torch_path(K, I, monkeypatch):
    # 280 x 540 at (1, 2): tiles of 280 x 285 to 64 x 64 are scales 4.4 and 4.5, past what the kernel takes
    img = u8_frame(280, 540).cuda()
    th, tw, origins = I.tile_plan(280, 540, (1, 2), 0.1)
    assert (th, tw, origins) == (280, 285, [(0, 0), (0, 255)]) and not I.fusable((th, tw), (64, 64), P)
    crops = torch.stack([img[y:y + th, x:x + tw] for y, x in origins]).contiguous()
    want, wpx = I.packed_patch_planes(crops, "rgb", (64, 64), P, MEAN, STD, want_pixels=True)
    torch_path = Counter(monkeypatch, I, "pixels_reference")
    planes, px = I.tiled_patch_planes(img, "rgb", origins, (th, tw), (64, 64), P, MEAN, STD, want_pixels=True)
    assert torch_path.n == 1 and torch.equal(planes, want) and torch.equal(px, wpx)
    a, b = I.affine(MEAN, STD)
    ref = I.resample_reference(crops.cpu().permute(0, 3, 1, 2), (64, 64)) \
        * torch.tensor(a, dtype=torch.float64).view(1, 3, 1, 1) + torch.tensor(b, dtype=torch.float64).view(1, 3, 1, 1)
    err_ref = (torch_path_pixels(I, crops.cpu()) - ref).abs().max().item()
    wst = Worst("tile pixels 280x285 -> 64x64 (torch path)", factor=FACTOR, label="tiles")
    err = (px.double().cpu() - ref).abs().max().item()
    wst.check(err, err_ref, 0.0, (280, 540))
    wst.done()
    assert err <= CAP


def torch_path_pixels(I, crops):
    return I.pixels_reference(crops, (64, 64), MEAN, STD).double()


def test_tile_launch_argument_checks(K, I):
    img = u8_frame(97, 131).cuda()
    th, tw, origins = I.tile_plan(97, 131, (3, 2), 0.3)
    L = I._L()
    tabs = I._device_tables(th, tw, 64, 128, P, img.device)
    planes = torch.empty(3, 6 * 32, 768, dtype=torch.bfloat16, device="cuda")
    table = torch.tensor([y * 393 + x * 3 for y, x in origins], dtype=torch.int64).cuda()
    lo = img.untyped_storage().data_ptr()
    F3 = ctypes.c_float * 3

    def call(B=6, org=origins, tab=table.data_ptr(), host=True, fh=97, fw=131, order=b"rgb"):
        flat = (ctypes.c_int * 12)(*[v for o in org for v in o]) if host else None
        return L.nos_image_patch_planes_tiles(img.data_ptr(), lo, lo + 97 * 131 * 3, 393, order, flat, tab, fh, fw,
                                              planes.data_ptr(), None, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                              tabs[2].data_ptr(), tabs[3].data_ptr(), 64, 128, I.TAPS, tabs[4], tabs[5],
                                              F3(1, 1, 1), F3(0, 0, 0), B, th, tw, 64, 128, P, 4, 8, 0,
                                              torch.cuda.current_stream().cuda_stream)
    assert call() == 0
    outside = [list(origins) for _ in range(4)]
    outside[0][5] = (57, 53)          # one row too low
    outside[1][5] = (56, 54)          # one column too far right
    outside[2][0] = (-1, 0)
    outside[3][3] = (28, -1)
    for bad in (dict(tab=None), dict(host=False), dict(B=0), dict(B=-1), dict(fh=96), dict(fw=130), dict(order=b"rbg")) \
            + tuple(dict(org=o) for o in outside):
        assert call(**bad) == -1 and L.nos_image_last_error(), bad
    torch.cuda.synchronize()


def test_tile_table_is_cached_and_dropped(K, I):
    img = u8_frame(97, 131).cuda()
    th, tw, origins = I.tile_plan(97, 131, (3, 2), 0.3)
    key = ("tiles", tuple(origins), 393, 3, str(img.device))
    I.tiled_patch_planes(img, "rgb", origins, (th, tw), (64, 128), P, MEAN, STD)
    assert key in I._tables and I._tables._d[key].dtype == torch.int64
    assert I._tables._d[key].tolist() == [y * 393 + x * 3 for y, x in origins]
    I.invalidate_cache()
    assert key not in I._tables


# ---- the merge kernel ---------------------------------------------------------------------------
def run_merge(I, logits, boxes, origins, tile_hw, thr, match, mt):
    got = I.merge_detections(logits.cuda(), boxes.cuda(), origins, tile_hw, thr, match, mt)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in got)


@pytest.mark.parametrize("match", ("ios", "iou"))
@pytest.mark.parametrize("seed", (0, 1))
def test_merge_matches_fp64(K, I, monkeypatch, seed, match):
    logits, boxes = T.synthetic(seed)
    kept, margins = T.merge_loop(logits, boxes, T.ORIGINS, T.TILE_HW, T.THRESHOLD, match, T.MATCH_THRESHOLD)
    T.decides_clearly(margins, T.THRESHOLD)
    assert len(kept) == (9 if match == "ios" else 11)
    ref = Counter(monkeypatch, I, "merge_detections_reference")
    got = run_merge(I, logits, boxes, T.ORIGINS, T.TILE_HW, T.THRESHOLD, match, T.MATCH_THRESHOLD)
    assert ref.n == 0
    ds, db = T.check_merged(got, kept, logits.shape[0] * logits.shape[1], SCORE_TOL, box_tol(T.FRAME_HW))
    print(f"[tiles] merge seed {seed} {match}: count {got[0].tolist()}, max |d score| {ds:.3g} (bound {SCORE_TOL:g}), "
          f"max |d box| {db:.3g} px (bound {box_tol(T.FRAME_HW):.3g}); margins {tuple(f'{m:.3g}' for m in margins)}")
    h = [i for i, k in enumerate(kept) if k[1] == 10]      # the two bit-identical rows: tile 0, then tile 3
    assert got[4][h].tolist() == [0, 3] and got[1][h[0]].item() == got[1][h[1]].item()
    # the fp64 torch reference says the same
    want = I.merge_detections_reference(logits.double(), boxes.double(), T.ORIGINS, T.TILE_HW, T.THRESHOLD, match,
                                        T.MATCH_THRESHOLD)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[4], want[4])


def test_merge_full_table_and_extremes(K, I):
    # 10 tiles of 100 rows, threshold 0: all 1000 rows are candidates; match_threshold 1.0 drops nothing (an overlap
    # is a quotient of a non-negative number by one at least as large, in fp32 as in fp64), so the kernel sorts
    logits, boxes = T.ramp(10, 100)
    origins = [(37 * b, 53 * b) for b in range(10)]
    kept, margins = T.merge_loop(logits, boxes, origins, (480, 640), 0.0, "ios", 1.0)
    assert len(kept) == 1000 and margins[1] >= 1e-3 and margins[2] >= 1e-5, margins
    got = run_merge(I, logits, boxes, origins, (480, 640), 0.0, "ios", 1.0)
    frame = (480 + 37 * 9, 640 + 53 * 9)
    ds, db = T.check_merged(got, kept, 1000, SCORE_TOL, box_tol(frame))
    print(f"[tiles] merge full table: count {got[0].tolist()}, max |d score| {ds:.3g}, max |d box| {db:.3g} px "
          f"(bound {box_tol(frame):.3g}); smallest score gap {margins[2]:.3g}")
    none = run_merge(I, logits, boxes, origins, (480, 640), 1.0, "ios", 0.5)
    assert none[0].tolist() == [0] and not any(t.any() for t in none[1:])


#: the dense table's seed: chosen on the CPU so that the fp64 loop decides clearly, which the test asserts
DENSE_SEED = 3


@pytest.mark.parametrize("match", ("ios", "iou"))
def test_merge_dense_table_with_chains(K, I, monkeypatch, match):
    # 10 tiles of 100 rows, 500 of them candidates at threshold 0.3, boxes of 20 to 80 % of a tile on tiles 20 x 30
    # apart: dozens of rows are dropped, and under "ios" some rows survive only because the earlier row that would
    # have dropped them was dropped itself (a pass that ignored the pivot's own fate would lose them)
    logits, boxes = T.ramp(10, 100, seed=DENSE_SEED, hole=True)
    origins = [(20 * b, 30 * b) for b in range(10)]
    dropped = []
    kept, margins = T.merge_loop(logits, boxes, origins, (100, 100), 0.3, match, 0.5, dropped)
    T.decides_clearly(margins, 0.3)
    chains = T.freed(kept, dropped, match, 0.5)
    assert len(kept) + len(dropped) == 500 and len(dropped) > 2 and (match == "iou" or len(chains) > 2)
    ref = Counter(monkeypatch, I, "merge_detections_reference")
    got = run_merge(I, logits, boxes, origins, (100, 100), 0.3, match, 0.5)
    assert ref.n == 0
    ds, db = T.check_merged(got, kept, 1000, SCORE_TOL, box_tol((280, 370)))
    print(f"[tiles] merge dense {match}: 500 candidates, {len(kept)} kept, {len(chains)} of them behind a dropped row; "
          f"max |d score| {ds:.3g}, max |d box| {db:.3g} px; margins {tuple(f'{m:.3g}' for m in margins)}")


#: the ramp's seed: chosen on the CPU so that the fp64 loop decides clearly (no compared pair's overlap within 1e-3 of
#: the match threshold), which the test asserts
PAST_SEED = 3


def test_merge_past_the_kernel_limit_takes_the_reference(K, I, monkeypatch):
    logits, boxes = T.ramp(11, 100, seed=PAST_SEED, hole=True)
    origins = [(20 * b, 30 * b) for b in range(11)]
    kept, margins = T.merge_loop(logits, boxes, origins, (100, 100), 0.3, "ios", 0.5)
    T.decides_clearly(margins, 0.3)
    assert 0 < len(kept) < 550          # 550 candidates, some of them dropped
    ref = Counter(monkeypatch, I, "merge_detections_reference")
    got = run_merge(I, logits, boxes, origins, (100, 100), 0.3, "ios", 0.5)
    assert ref.n == 1
    T.check_merged(got, kept, 1100, SCORE_TOL, box_tol((300, 400)))


def test_merge_argument_checks(K, I):
    L = I._L()
    z = torch.zeros(16, device="cuda")
    p = z.data_ptr()

    def call(B=1, M=4, C=3, iou=0, **null):
        a = dict(logits=p, boxes=p, origins=p, count=p, scores=p, labels=p, out=p, tile=p)
        a.update(null)
        return L.nos_merge_detections_f32(a["logits"], a["boxes"], a["origins"], 8.0, 8.0, 0.5, 0.5, iou, B, M, C,
                                          a["count"], a["scores"], a["labels"], a["out"], a["tile"], None)
    for bad in (dict(B=0), dict(M=0), dict(B=1, M=1025), dict(B=11, M=100), dict(B=1025, M=1), dict(C=129), dict(C=1),
                dict(iou=2), dict(logits=None), dict(boxes=None), dict(origins=None), dict(count=None),
                dict(scores=None), dict(labels=None), dict(out=None), dict(tile=None)):
        assert call(**bad) == -1 and L.nos_image_last_error(), bad
    torch.cuda.synchronize()


# ---- end to end ---------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def twin():
    """The same model in fp32 on the CPU: the yardstick's."""
    return small_model()


TILES, OVERLAP = (3, 2), 0.3


def against_fp64(twin, px, out, name):
    """The tiles' logits and boxes against the fp64 forward on the pixels ``px`` they were computed from."""
    from yolos_reference import yardstick
    (_, rl, rb), (_, el, eb) = yardstick(twin, px.cpu())
    wst = Worst(name, label="tiles")
    for b in range(px.shape[0]):
        for key, r, e in (("logits", rl, el), ("pred_boxes", rb, eb)):
            err = (out[key][b].double().cpu() - r[b]).abs().max().item()
            wst.check(err, e, 2e-6 * max(1.0, r.abs().max().item()), (b, key))
    wst.done()


def test_detect_tiled_is_the_model_on_the_kernel_pixels(K, I, model, twin, monkeypatch):
    frame = u8_frame(97, 131, seed=2).cuda()
    th, tw, origins = I.tile_plan(97, 131, TILES, OVERLAP)
    tiled = Counter(monkeypatch, I, "tiled_patch_planes")
    heads = Counter(monkeypatch, K, "detection_heads")
    with torch.no_grad():
        out = model.detect_tiled(frame, TILES, OVERLAP, 0.0, "ios", 0.5)
    assert tiled.n == 1 and heads.n == 1
    assert out["logits"].shape == (6, 100, 92) and out["pred_boxes"].shape == (6, 100, 4)
    assert out["origins"].tolist() == [list(o) for o in origins] and out["tile_hw"] == (th, tw)
    px = I.tiled_patch_planes(frame, "rgb", origins, (th, tw), (64, 128), P, MEAN, STD, want_pixels=True)[1]
    against_fp64(twin, px, out, "detect_tiled 97x131 (3, 2) -> 6 x 64x128, 2 layers, x3")
    s = out["scores"].sort().values
    assert out["count"].item() > 300 and s[-1].item() > s[0].item()
    cands = torch.softmax(out["logits"], -1)[..., :-1].max(-1).values.flatten().sort().values
    thr = 0.5 * (cands[299] + cands[300]).item()
    assert cands[300].item() - cands[299].item() > 1e-6
    for match in ("ios", "iou"):
        with torch.no_grad():
            o = model.detect_tiled(frame, TILES, OVERLAP, thr, match, 0.5)
        want = I.merge_detections(o["logits"], o["pred_boxes"], origins, (th, tw), thr, match, 0.5)
        for k, w in zip(("count", "scores", "labels", "boxes", "tile"), want):
            assert torch.equal(o[k], w), (match, k)
        assert 0 < o["count"].item() <= 300
        res = model.processor.results(o["count"], o["scores"], o["labels"], o["boxes"])
        assert len(res) == 1 and res[0]["boxes"].shape == (o["count"].item(), 4)
        print(f"[tiles] detect_tiled {match}: 300 candidates, {o['count'].item()} kept")


def test_one_tile_is_detect_image(K, I, model):
    frame = u8_frame(97, 131, seed=3).cuda()
    with torch.no_grad():
        s = model.detect_image(frame, 0.0)["scores"][0].sort().values
        thr = 0.5 * (s[49] + s[50]).item()
        assert s[50].item() - s[49].item() > 1e-6
        whole = model.detect_image(frame, thr)
        one = model.detect_tiled(frame, (1, 1), 0.2, thr)
    assert torch.equal(one["logits"], whole["logits"]) and torch.equal(one["pred_boxes"], whole["pred_boxes"])
    assert one["count"].tolist() == [50] and whole["count"].tolist() == [50]
    order = torch.sort(-whole["scores"][0, :50], stable=True).indices
    assert torch.equal(one["scores"][:50], whole["scores"][0, :50][order])
    assert torch.equal(one["labels"][:50], whole["labels"][0, :50][order])
    assert torch.equal(one["boxes"][:50], whole["boxes"][0, :50][order])
    assert not one["scores"][50:].any() and not one["boxes"][50:].any() and not one["tile"].any()


def test_detect_tiled_graph_replay(K, I, model):
    first, second = u8_frame(97, 131, seed=4), u8_frame(97, 131, seed=5)
    buf = first.cuda()
    keys = ("logits", "pred_boxes", "origins", "count", "scores", "labels", "boxes", "tile")
    with torch.no_grad():
        c = torch.softmax(model.detect_tiled(buf, TILES, OVERLAP, 0.0)["logits"], -1)[..., :-1].max(-1).values
        c = c.flatten().sort().values
        thr = 0.5 * (c[299] + c[300]).item()
        eager = {k: model.detect_tiled(buf, TILES, OVERLAP, thr)[k].clone() for k in keys}
        other = {k: model.detect_tiled(second.cuda(), TILES, OVERLAP, thr)[k].clone() for k in keys}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=stream):
        held = model.detect_tiled(buf, TILES, OVERLAP, thr)
    for k in keys:
        held[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert 0 < eager["count"].item() <= 300
    for k in keys:
        assert torch.equal(held[k], eager[k]), k
    buf.copy_(second)                     # the graph reads the frame's buffer by address
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(other["logits"], eager["logits"])
    for k in keys:
        assert torch.equal(held[k], other[k]), k
    del graph


@pytest.mark.parametrize("mode", ("torch", "f32"))
def test_detect_tiled_elsewhere(K, I, model, twin, monkeypatch, mode):
    frame = u8_frame(97, 131, seed=2).cuda()
    th, tw, origins = I.tile_plan(97, 131, TILES, OVERLAP)
    crops = torch.stack([frame[y:y + th, x:x + tw] for y, x in origins])
    tiled = Counter(monkeypatch, I, "tiled_patch_planes")
    if mode == "torch":
        K.set_backend("torch")
    else:
        K.set_fp32_matmul("f32")
    try:
        with torch.no_grad():
            out = model.detect_tiled(frame, TILES, OVERLAP, 0.3)
            px = model.processor.preprocess(crops)
            want = I.merge_detections(out["logits"], out["pred_boxes"], origins, (th, tw), 0.3)
    finally:
        K.set_backend("hip")
        K.set_fp32_matmul("x3")
    assert tiled.n == 0 and px.shape == (6, 3, 64, 128)
    against_fp64(twin, px, out, f"detect_tiled 97x131 (3, 2), {mode}")
    for k, w in zip(("count", "scores", "labels", "boxes", "tile"), want):
        assert torch.equal(out[k], w), k


# ---- the pod client (last: it starts a process, and nothing follows it if it fails) --------------
def test_pod_client_tiles():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "walkai_nos_amd.dataplane.client", "--end-to-end",
           "--tiles", "2,2", "--tile-overlap", "0.2", "--threshold", "0.0", "--match-threshold", "1.0",
           "--image-hw", "96,128", "--size", "80,133", "--seconds", "1"]
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
    assert out["end_to_end"] is True and out["tiles"] == 4 and out["tile_hw"] == [54, 72] and out["input_hw"] == [80, 96]
    assert out["detections"] == 400 and out["inferences"] > 0      # nothing is dropped at match threshold 1
    print(f"[tiles] client --tiles 2,2 96x128 -> 4 x 80x96: {out['inferences']} inferences in {out['window_s']} s, "
          f"mean {out['latency_ms']['mean']} ms")
