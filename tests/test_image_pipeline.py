"""The image pipeline off the GPU: the YOLOS size rule, the fp64 definition of the antialiased
resample against PIL, ``YolosProcessor`` against the ``transformers`` processor (pixels within one
uint8 step, detections equal), the tie rule of the labels, and the packaging of ``libnos_image.so``.

The ``transformers`` processor rounds to uint8 after its resize; this one does not. One uint8 step is
``1 / (255 std_c)`` in normalised units, which is the bound of the pixel comparison."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from walkai_nos_amd.models.workload.processor import IMAGENET_STD, YolosProcessor
from walkai_nos_amd.ops import build
from walkai_nos_amd.ops import image as I

SIZES = {(480, 640): (800, 1056), (640, 480): (1056, 800), (3024, 4032): (800, 1056), (500, 2000): (320, 1328),
         (800, 1200): (800, 1200)}


def u8_image(h, w, seed=0, batch=None):
    g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w)
    shape = (h, w, 3) if batch is None else (batch, h, w, 3)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


# ---- packaging: fails without the feature -------------------------------------------------------
def test_image_library_is_a_target_of_its_own():
    t = build.target("libnos_image.so")
    assert t.sources == ["image.hip"] and t.compiler == "hipcc" and not t.executable
    assert "image.hip" not in build.target("libnos_kernels.so").sources


# ---- the size rule ------------------------------------------------------------------------------
def test_resize_size_table():
    for hw, want in SIZES.items():
        assert I.resize_size(hw) == want, hw
    assert I.resize_size((48, 64), 80, 133) == (80, 96)
    assert I.resize_size((20, 100), 80, 133) == (16, 128)


def test_resize_size_matches_transformers():
    m = pytest.importorskip("transformers.models.yolos.image_processing_pil_yolos")
    n = 0
    for h in list(range(17, 140, 7)) + [480, 500, 640, 800, 1333, 3024]:
        for w in list(range(16, 150, 9)) + [480, 640, 1200, 2000, 4032]:
            for shortest, longest in ((800, 1333), (80, 133), (48, 133), (512, 512)):
                assert I.resize_size((h, w), shortest, longest) == \
                    tuple(m.get_size_with_aspect_ratio_yolos((h, w), shortest, longest)), (h, w, shortest, longest)
                n += 1
    assert n > 1000


# ---- the resample -------------------------------------------------------------------------------
RESIZES = (((48, 64), (80, 96)), ((37, 53), (80, 112)), ((120, 160), (48, 64)), ((256, 256), (64, 64)),
           ((80, 100), (80, 96)), ((20, 100), (16, 128)), ((300, 260), (64, 64)))


@pytest.mark.parametrize("hw,out", RESIZES, ids=lambda v: "x".join(map(str, v)))
def test_reference_resample_is_torch_antialias_and_pil(hw, out):
    img = u8_image(*hw).permute(2, 0, 1)
    ref = I.resample_reference(img, out)
    tor = F.interpolate(img[None].double(), size=out, mode="bilinear", antialias=True, align_corners=False)[0]
    assert (ref - tor).abs().max().item() <= 1e-10
    Image = pytest.importorskip("PIL.Image")
    worst = 0.0
    for c in range(3):
        pil = Image.fromarray(img[c].numpy().astype(np.float32), mode="F").resize((out[1], out[0]), Image.BILINEAR)
        worst = max(worst, float(np.abs(np.asarray(pil, dtype=np.float64) - ref[c].numpy()).max()))
    print(f"[image] reference vs PIL mode F {hw} -> {out}: max |d| {worst:.3g} on 0-255 data")
    assert worst <= 1e-4


def test_tap_tables_stay_within_nine_taps_up_to_scale_four():
    for n_in, n_out in ((4032, 1056), (3024, 800), (256, 64), (64, 96), (100, 96)):
        first, count, wt = I.tap_table(n_in, n_out, I.TAPS)
        assert count.min() >= 1 and count.max() <= I.TAPS and first.min() >= 0 and (first + count).max() <= n_in
        assert np.abs(wt.sum(1) - 1.0).max() < 1e-14 and (np.diff(first) >= 0).all()
    with pytest.raises(ValueError):
        I.tap_table(320, 64, I.TAPS)
    assert I.fusable((256, 256), (64, 64), 16) and not I.fusable((260, 260), (64, 64), 16)


# ---- the processor against transformers -----------------------------------------------------------
@pytest.mark.parametrize("hw,size,out", (((480, 640), None, (800, 1056)),
                                         ((48, 64), {"shortest_edge": 80, "longest_edge": 133}, (80, 96))),
                         ids=("480x640", "48x64"))
def test_preprocess_within_one_uint8_step_of_transformers(hw, size, out):
    m = pytest.importorskip("transformers.models.yolos.image_processing_pil_yolos")
    img = u8_image(*hw)
    hf = m.YolosImageProcessorPil(size=size) if size else m.YolosImageProcessorPil()
    want = hf(images=img.numpy(), return_tensors="pt")["pixel_values"]
    proc = YolosProcessor(size["shortest_edge"], size["longest_edge"]) if size else YolosProcessor()
    got = proc.preprocess(img)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) == (1, 3) + out
    for c in range(3):
        d = (got[0, c].double() - want[0, c].double()).abs().max().item()
        step = 1.0 / (255.0 * IMAGENET_STD[c])
        print(f"[image] preprocess vs transformers {hw} channel {c}: max |d| {d:.4f}, one uint8 step {step:.4f}")
        assert d < step
    # ndarray and batch inputs are the same pixels
    assert torch.equal(proc.preprocess(img.numpy()), got) and torch.equal(proc.preprocess(img[None]), got)


def test_preprocess_takes_a_pil_image():
    Image = pytest.importorskip("PIL.Image")
    img = u8_image(48, 64)
    proc = YolosProcessor(80, 133)
    assert torch.equal(proc.preprocess(Image.fromarray(img.numpy())), proc.preprocess(img))
    with pytest.raises(ValueError):
        proc.preprocess(img.float())


def test_cpu_planes_are_the_split_of_the_pixels():
    img = u8_image(37, 53, batch=2)
    proc = YolosProcessor(80, 133)
    planes, px = I.image_patch_planes(img, (80, 112), 16, proc.mean, proc.std, want_pixels=True)
    assert planes.shape == (3, 2 * 5 * 7, 768) and planes.dtype == torch.bfloat16 and px.shape == (2, 3, 80, 112)
    assert torch.equal(planes[0].float() + planes[1].float() + planes[2].float(), I.im2col(px, 16))
    assert torch.equal(px, proc.preprocess(img))
    ref = I.resample_reference(img.permute(0, 3, 1, 2), (80, 112))
    a, b = I.affine(proc.mean, proc.std)
    ref = ref * torch.tensor(a, dtype=torch.float64).view(1, 3, 1, 1) + torch.tensor(b, dtype=torch.float64).view(1, 3, 1, 1)
    # a tap or a centre off by one errs by order 1; fp32 torch computes its weights in fp32 (~1e-5)
    assert (px.double() - ref).abs().max().item() < 1e-4


# ---- detections ---------------------------------------------------------------------------------
def det_inputs(B, M=100, C=92, seed=0):
    g = torch.Generator().manual_seed(seed)
    return 3.0 * torch.randn(B, M, C, generator=g), 0.2 + 0.6 * torch.rand(B, M, 4, generator=g)


@pytest.mark.parametrize("threshold", (0.1, 0.3, 0.5))
def test_post_process_matches_transformers(threshold):
    m = pytest.importorskip("transformers.models.yolos.image_processing_pil_yolos")
    from types import SimpleNamespace
    logits, boxes = det_inputs(2)
    sizes = [(480, 640), (37, 53)]
    want = m.YolosImageProcessorPil().post_process_object_detection(
        SimpleNamespace(logits=logits, pred_boxes=boxes), threshold=threshold, target_sizes=sizes)
    got = YolosProcessor().post_process(logits, boxes, threshold, sizes)
    assert len(got) == len(want) == 2 and sum(len(w["scores"]) for w in want) > 0
    for g, w in zip(got, want):
        assert g["labels"].dtype == w["labels"].dtype and torch.equal(g["labels"], w["labels"])
        assert g["scores"].shape == w["scores"].shape and g["boxes"].shape == w["boxes"].shape
        assert len(w["scores"]) > 0
        assert (g["scores"] - w["scores"]).abs().max().item() <= 1e-6
        assert (g["boxes"] - w["boxes"]).abs().max().item() <= 1e-6
    # without target sizes the boxes stay in 0..1, as transformers leaves them
    want = m.YolosImageProcessorPil().post_process_object_detection(
        SimpleNamespace(logits=logits, pred_boxes=boxes), threshold=threshold)
    got = YolosProcessor().post_process(logits, boxes, threshold)
    for g, w in zip(got, want):
        assert torch.equal(g["labels"], w["labels"]) and (g["boxes"] - w["boxes"]).abs().max().item() <= 1e-6


def test_detections_layout_ties_and_no_object():
    logits, boxes = det_inputs(1, M=6, C=5, seed=3)
    logits[0, 1] = torch.tensor([1.0, 4.0, 4.0, 0.0, -1.0])     # two equal top logits: the lower label
    logits[0, 2] = torch.tensor([0.0, 1.0, 0.5, 2.0, 9.0])      # "no object" largest: score from the first L
    logits[0, 4] = torch.tensor([-9.0, -9.0, -9.0, -9.0, 9.0])  # below any threshold worth using
    count, scores, labels, xyxy = I.detections(logits, boxes, [(100, 200)], 0.0)
    assert count.dtype == torch.int32 and labels.dtype == torch.int32 and count.tolist() == [6]
    assert labels[0, 1].item() == 1 and labels[0, 2].item() == 3
    p = torch.softmax(logits[0, 2].double(), -1)
    assert abs(scores[0, 2].item() - p[3].item()) < 1e-7 and scores[0, 2].item() < 1e-3
    cx, cy, w, h = boxes[0, 0].tolist()
    assert torch.allclose(xyxy[0, 0], torch.tensor([(cx - w / 2) * 200, (cy - h / 2) * 100, (cx + w / 2) * 200,
                                                    (cy + h / 2) * 100]), atol=1e-4)
    # compaction keeps the token order and zeroes the slots past count
    thr = 0.5 * (scores[0].sort().values[2] + scores[0].sort().values[3]).item()
    c2, s2, l2, b2 = I.detections(logits, boxes, [(100, 200)], thr)
    keep = scores[0] > thr
    assert c2.tolist() == [3] and torch.equal(s2[0, :3], scores[0][keep]) and torch.equal(l2[0, :3], labels[0][keep])
    assert torch.equal(b2[0, :3], xyxy[0][keep])
    assert not s2[0, 3:].any() and not l2[0, 3:].any() and not b2[0, 3:].any()
    c3, s3, l3, b3 = I.detections(logits, boxes, [(100, 200)], 1.0)
    assert c3.tolist() == [0] and not s3.any() and not l3.any() and not b3.any()


def test_model_detect_image_on_the_cpu_is_preprocess_forward_post_process():
    from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=1)).eval()
    m.processor = YolosProcessor(80, 133)
    img = u8_image(48, 64)
    with torch.no_grad():
        out = m.detect_image(img, threshold=0.0)
        logits, boxes = m(m.processor.preprocess(img))
    assert torch.equal(out["logits"], logits) and torch.equal(out["pred_boxes"], boxes)
    want = m.processor.post_process(logits, boxes, 0.0, [(48, 64)])
    got = m.processor.results(out["count"], out["scores"], out["labels"], out["boxes"])
    assert out["count"].tolist() == [100] and len(got) == 1
    for k in ("scores", "labels", "boxes"):
        assert torch.equal(got[0][k], want[0][k])
