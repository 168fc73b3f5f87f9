"""The image pipeline on the GPU (``csrc/image.hip``): the fused uint8 -> patch-planes kernel at the
smallest sizes where each of its branches can go wrong, the detections kernel, ``detect_image`` end to
end (eager and as one replay of a captured graph) and the pod client's ``--end-to-end`` mode.

Pixels: the planes are the exact split of the fp32 pixel the kernel also writes (bit for bit, and
bit-equal to ``kernels.patch_planes`` of those pixels), and the pixels are compared with the fp64
definition of the resample (``ops.image.resample_reference``, which is torch's antialiased bilinear
``F.interpolate`` in fp64) in the suite's convention: ``err_ref`` is the error of the same formula in
plain fp32 on the CPU (``ops.image.pixels_reference``), the bound ``FACTOR * err_ref``, and never more
than ``CAP`` = 1e-4 in normalised units (9 x 9 taps and the affine are at most 85 roundings x 2^-24 /
0.224 = 2.3e-5; a tap off by one or a centre off by half a pixel errs by order 1 on random uint8).

Measured worst ``err / err_ref`` (MI355X; the run is kept in ``profiles/pytest_gpu_image.log``, one
``[image]`` line per test), bound ``FACTOR`` = 2: the kernel 0.789 (256x256 -> 64x64, scale 4), 0.773
(20x100 -> 16x128), 0.752 (120x160 -> 48x64) and 0.026-0.055 on the upscales, where torch's fp32 path
computes its weights in fp32 and loses 1-2e-5 itself; the torch path past the tap limit (260x260) 1.00,
the same arithmetic as the yardstick. The largest absolute error of the kernel is 6.6e-7 (cap 1e-4).
Detections against fp64: scores within 1.3e-7 (bound 1e-5), boxes within 6.9e-5 pixel (bound 1e-3)."""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

from kernel_inputs import Worst

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
P = 16
#: twice the worst measured err / err_ref (1.00, the torch path; the kernel 0.789), rounded up: the
#: order of the sums and FMA contraction legitimately move a result by about that much
FACTOR = 2.0
CAP = 1e-4

#: (source h, w, batch, (shortest, longest) of the size rule or None, target H, W, fused?)
CASES = ((48, 64, 1, (80, 133), (80, 96), True),       # upscale, 2 taps, edge clamping on all four sides
         (64, 48, 1, (80, 133), (96, 80), True),       # portrait branch of the size rule
         (37, 53, 1, (80, 133), (80, 112), True),      # odd source sizes; x and y scales differ
         (120, 160, 1, (48, 133), (48, 64), True),     # downscale 2.5, up to 7 taps
         (80, 100, 1, (80, 133), (80, 96), True),      # scale exactly 1 on one axis, 1.04 on the other
         (20, 100, 1, (80, 133), (16, 128), True),     # longest-edge clamp; up on one axis, down on the other
         (256, 256, 1, None, (64, 64), True),          # scale 4, the tap limit
         (260, 260, 1, None, (64, 64), False),         # just past it: the torch path, and still agrees
         (48, 64, 2, (80, 133), (80, 96), True))       # batch index in row addressing
IDS = ["{}x{}b{}".format(*c[:3]) for c in CASES]


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


def u8_image(h, w, batch, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w)
    return torch.randint(0, 256, (batch, h, w, 3), generator=g, dtype=torch.uint8)


_refs = {}


def pixel_reference(I, h, w, batch, out):
    """``(image, fp64 pixels, err_ref)``, computed once per case and left unchanged."""
    key = (h, w, batch, out)
    if key not in _refs:
        img = u8_image(h, w, batch)
        a, b = I.affine(MEAN, STD)
        ref = I.resample_reference(img.permute(0, 3, 1, 2), out) * torch.tensor(a, dtype=torch.float64).view(1, 3, 1, 1) \
            + torch.tensor(b, dtype=torch.float64).view(1, 3, 1, 1)
        err_ref = (I.pixels_reference(img, out, MEAN, STD).double() - ref).abs().max().item()
        _refs[key] = (img, ref, err_ref)
    return _refs[key]


class Counter:
    def __init__(self, monkeypatch, owner, name):
        self.n = 0
        fn = getattr(owner, name)

        def spy(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        monkeypatch.setattr(owner, name, spy)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_patch_planes_exact_split_and_accurate_pixels(K, I, monkeypatch, case):
    h, w, batch, rule, out, fused = case
    if rule is not None:
        assert I.resize_size((h, w), *rule) == out
    img, ref, err_ref = pixel_reference(I, h, w, batch, out)
    torch_path = Counter(monkeypatch, I, "pixels_reference")
    dev = img.cuda()
    planes, px = I.image_patch_planes(dev, out, P, MEAN, STD, want_pixels=True)
    only, none = I.image_patch_planes(dev, out, P, MEAN, STD)
    torch.cuda.synchronize()
    assert torch_path.n == (0 if fused else 2) and none is None
    gh, gw = out[0] // P, out[1] // P
    assert planes.shape == (3, batch * gh * gw, 3 * P * P) and planes.dtype == torch.bfloat16
    assert px.shape == (batch, 3) + out and px.dtype == torch.float32
    # exact: the planes sum (in this order, in fp32) to the pixel the kernel wrote, each plane is the
    # split kernels.patch_planes makes of those pixels, and the launch without pixels writes the same
    assert torch.equal(planes[0].float() + planes[1].float() + planes[2].float(), I.im2col(px, P))
    assert torch.equal(planes, K.patch_planes(px, P))
    assert torch.equal(only, planes)
    # accurate: against fp64, in units of what the same formula loses in fp32 on the CPU
    wst = Worst(f"pixels {h}x{w} b{batch} -> {out[0]}x{out[1]} ({'kernel' if fused else 'torch path'})",
                factor=FACTOR, label="image")
    err = (px.double().cpu() - ref).abs().max().item()   # NaN survives max(): it fails the bound
    wst.check(err, err_ref, 0.0, case[:3])
    wst.done()
    assert err <= CAP, (err, CAP)


def test_patch_planes_on_a_slice_and_uncropped_pixels(K, I):
    # on a 32-CU slice 128 workgroups loop over the 2 x 13 x 11 tiles (grid-stride); H, W that are no
    # multiple of the patch still get every pixel, and the planes only the whole patches
    h, w, out = 53, 37, (200, 170)
    img, ref, err_ref = pixel_reference(I, h, w, 2, out)
    dev = img.cuda()
    planes, px = I.image_patch_planes(dev, out, P, MEAN, STD, want_pixels=True)
    assert planes.shape[1] == 2 * 12 * 10
    assert torch.equal(planes, K.patch_planes(px, P))
    K.set_slice_cus(32)
    try:
        assert I.image_wgs() == 128
        sliced = I.image_patch_planes(dev, out, P, MEAN, STD, want_pixels=True)
    finally:
        K.set_slice_cus(None)
    assert torch.equal(sliced[0], planes) and torch.equal(sliced[1], px)
    wst = Worst(f"pixels {h}x{w} b2 -> {out[0]}x{out[1]} (uncropped, slice)", factor=FACTOR, label="image")
    err = (px.double().cpu() - ref).abs().max().item()
    wst.check(err, err_ref, 0.0, (h, w, 2))
    wst.done()
    assert err <= CAP


def test_patch_planes_argument_checks(K, I):
    img = u8_image(48, 64, 1).cuda()
    L = I._L()
    tabs = I._device_tables(48, 64, 80, 96, P, img.device)
    planes = torch.empty(3, 30, 768, dtype=torch.bfloat16, device="cuda")
    import ctypes
    F3 = ctypes.c_float * 3

    def call(B=1, p=P, gh=5, gw=6, ytab=80, xtab=96, taps=I.TAPS, fh=tabs[4], fw=tabs[5]):
        return L.nos_image_patch_planes_u8(img.data_ptr(), planes.data_ptr(), None, tabs[0].data_ptr(),
                                           tabs[1].data_ptr(), tabs[2].data_ptr(), tabs[3].data_ptr(), ytab, xtab, taps,
                                           fh, fw, F3(1, 1, 1), F3(0, 0, 0), B, 48, 64, 80, 96, p, gh, gw, 0,
                                           torch.cuda.current_stream().cuda_stream)
    assert call() == 0
    for bad in (dict(B=0), dict(p=15), dict(p=18), dict(gh=6), dict(gw=7), dict(ytab=79), dict(xtab=97),
                dict(taps=8), dict(fh=73), dict(fw=0)):
        assert call(**bad) == -1 and L.nos_image_last_error(), bad
    torch.cuda.synchronize()


# ---- detections ---------------------------------------------------------------------------------
THRESHOLD, DET_SEED = 0.3, 9
TARGETS = ((480, 640), (37, 53))


def det_case(B, seed=DET_SEED):
    g = torch.Generator().manual_seed(seed)
    return 3.0 * torch.randn(B, 100, 92, generator=g), 0.2 + 0.6 * torch.rand(B, 100, 4, generator=g)


def check_detections(I, logits, boxes, targets, thr, tag):
    """The kernel against the fp64 torch composition: equal count, labels and order; scores within
    1e-5 ((92 + 4) roundings x 2^-24 = 5.7e-6), boxes within 1e-3 pixel (4 roundings x 2^-24 x 1333)."""
    tgt = torch.tensor(targets, dtype=torch.float64)
    prob = torch.softmax(logits.double(), -1)[..., :-1]
    top = prob.topk(2, -1).values
    # the reference decides every row clearly: no score near the threshold, no near-tie of labels
    assert (top[..., 0] - thr).abs().min().item() >= 1e-3 or thr in (0.0, 1.0)
    assert (top[..., 0] - top[..., 1]).min().item() >= 1e-3
    want = I.detections_reference(logits.double(), boxes.double(), tgt, thr)
    got = I.detections(logits.cuda(), boxes.cuda(), targets, thr)
    torch.cuda.synchronize()
    count, scores, labels, xyxy = (t.cpu() for t in got)
    assert count.dtype == torch.int32 and labels.dtype == torch.int32
    assert scores.shape == logits.shape[:2] and xyxy.shape == boxes.shape
    ds = (scores.double() - want[1]).abs().max().item()
    db = (xyxy.double() - want[3]).abs().max().item()
    print(f"[image] detections {tag}: count {count.tolist()}, max |d score| {ds:.3g} (bound 1e-5), "
          f"max |d box| {db:.3g} px (bound 1e-3)")
    assert torch.equal(count, want[0]) and torch.equal(labels, want[2])
    assert ds <= 1e-5 and db <= 1e-3
    for b, n in enumerate(count.tolist()):   # slots past count are zero
        assert not scores[b, n:].any() and not labels[b, n:].any() and not xyxy[b, n:].any()
    return count, scores, labels, xyxy


@pytest.mark.parametrize("B", (1, 2))
def test_detections_match_fp64(K, I, B):
    logits, boxes = det_case(B)
    count, *_ = check_detections(I, logits, boxes, list(TARGETS[:B]), THRESHOLD, f"B={B}")
    assert 0 < count.min().item() and count.max().item() < 100


def test_detections_threshold_extremes_ties_and_no_object(K, I):
    logits, boxes = det_case(1)
    logits[0, 5, :] = -2.0
    logits[0, 5, 17] = logits[0, 5, 40] = logits[0, 5, 80] = 6.0    # a tie: the lowest label
    logits[0, 7, 91] = 30.0                                          # "no object" largest: score from the first L
    logits[0, 7, 70] = 12.0
    prob = torch.softmax(logits.double(), -1)[..., :-1]
    count, scores, labels, _ = (t.cpu() for t in I.detections(logits.cuda(), boxes.cuda(), [TARGETS[0]], 0.0))
    assert count.tolist() == [100]                                   # threshold 0 keeps all 100, in order
    assert labels[0, 5].item() == 17 and labels[0, 7].item() == 70
    assert abs(scores[0, 7].item() - prob[0, 7, 70].item()) <= 1e-5 and scores[0, 7].item() < 1e-6
    rows = [r for r in range(100) if r != 5]                         # every other row has one clear best class
    assert torch.equal(labels[0, rows].long(), prob[0, rows].argmax(-1))
    assert (scores[0].double() - prob[0].max(-1).values).abs().max().item() <= 1e-5
    count, scores, labels, xyxy = (t.cpu() for t in I.detections(logits.cuda(), boxes.cuda(), [TARGETS[0]], 1.0))
    assert count.tolist() == [0] and not scores.any() and not labels.any() and not xyxy.any()
    # the torch backend (the reference math on the GPU) agrees on what is kept
    K.set_backend("torch")
    try:
        ref = I.detections(logits.cuda(), boxes.cuda(), [TARGETS[0]], THRESHOLD)
    finally:
        K.set_backend("hip")
    got = I.detections(logits.cuda(), boxes.cuda(), [TARGETS[0]], THRESHOLD)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
    L = I._L()
    assert L.nos_detections_f32(None, None, None, 0.5, 1, 100, 92, None, None, None, None, None) == -1
    z = torch.zeros(4, device="cuda")
    for B, M, C in ((0, 100, 92), (1, 1025, 92), (1, 100, 129), (1, 100, 1)):
        assert L.nos_detections_f32(z.data_ptr(), z.data_ptr(), z.data_ptr(), 0.5, B, M, C, z.data_ptr(), z.data_ptr(),
                                    z.data_ptr(), z.data_ptr(), None) == -1, (B, M, C)


# ---- end to end ---------------------------------------------------------------------------------
def randomize(module, seed=1):
    """Every parameter distinguishable: matrices ``randn * 0.05``, vectors ``randn * 0.5``, LayerNorm
    weights ``1 + randn * 0.5`` (no zero bias, no unit LayerNorm), in sorted name order."""
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


def test_detect_image_is_the_model_on_the_kernel_pixels(K, I, model, monkeypatch):
    img = u8_image(48, 64, 1)[0].cuda()
    fused = Counter(monkeypatch, I, "image_patch_planes")
    with torch.no_grad():
        every = model.detect_image(img, 0.0)
        assert fused.n == 1 and K.x3_active(model.pos_embed)
        px = model.processor.preprocess(img)
        logits, boxes = model(px)
    assert px.shape == (1, 3, 80, 96)
    assert torch.equal(every["logits"], logits) and torch.equal(every["pred_boxes"], boxes)
    assert every["count"].tolist() == [100]
    s = every["scores"][0].sort().values
    thr = 0.5 * (s[49] + s[50]).item()      # half of the rows survive
    assert s[50].item() - s[49].item() > 1e-6
    with torch.no_grad():
        out = model.detect_image(img, thr)
    want = model.processor.post_process(logits, boxes, thr, [(48, 64)])
    got = model.processor.results(out["count"], out["scores"], out["labels"], out["boxes"])
    assert out["count"].tolist() == [50] and len(got) == len(want) == 1
    for k in ("scores", "labels", "boxes"):
        assert torch.equal(got[0][k], want[0][k]), k
    print(f"[image] detect_image 48x64 -> 80x96, 2 layers: threshold {thr:.4f} keeps {out['count'].tolist()}")
    # f32 mode takes preprocess + forward + post_process
    K.set_fp32_matmul("f32")
    try:
        with torch.no_grad():
            f32 = model.detect_image(img, thr)
            l32, b32 = model(px)
        assert fused.n == 4   # the processor's own call, not the fused encode
        assert torch.equal(f32["logits"], l32) and torch.equal(f32["pred_boxes"], b32)
    finally:
        K.set_fp32_matmul("x3")


def test_detect_image_graph_replay(K, I, model):
    img = u8_image(48, 64, 1, seed=1)[0].cuda()
    with torch.no_grad():
        s = model.detect_image(img, 0.0)["scores"][0].sort().values
        thr = 0.5 * (s[49] + s[50]).item()
        eager = {k: v.clone() for k, v in model.detect_image(img, thr).items()}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=stream):
        held = model.detect_image(img, thr)
    for v in held.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert eager["count"].tolist() == [50]
    for k, v in eager.items():
        assert torch.equal(held[k], v), k
    del graph


# ---- the pod client (last: it starts a process, and nothing follows it if it fails) --------------
def test_pod_client_end_to_end():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "walkai_nos_amd.dataplane.client", "--end-to-end",
           "--seconds", "1", "--image-hw", "48,64", "--size", "80,133", "--threshold", "0.0"]
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
    assert out["end_to_end"] is True and out["input_hw"] == [80, 96]
    assert out["detections"] == 100 and out["inferences"] > 0      # threshold 0 keeps every detection token
    print(f"[image] client --end-to-end 48x64 -> 80x96: {out['inferences']} inferences in {out['window_s']} s, "
          f"mean {out['latency_ms']['mean']} ms")
