"""NV12 frames on the GPU (``image_patch_planes_nv12`` in ``csrc/image.hip``): the fused launch against
the RGB kernel on ``ops.image.nv12_to_rgb`` of the same frame. The conversion is defined in integers
and everything behind the staging loop is the RGB kernel's code, so planes and pixels are compared with
``torch.equal`` — no tolerance; the RGB kernel itself is pinned against fp64 in ``test_gpu_image.py``.
Each case is the smallest size that reaches its branch (patch 16, seeded random planes)."""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
P = 16
COMBOS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]

#: (source h, w, target H, W, fused?)
CASES = ((48, 64, 80, 96, True),        # upscale: footprints start on odd rows and columns
         (37, 53, 80, 112, True),       # odd sizes: the last chroma row and column serve one luma line
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


def nv12_frame(h, w, batch=1, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w)
    return (torch.randint(0, 256, (batch, h, w), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (batch, (h + 1) // 2, (w + 1) // 2, 2), generator=g, dtype=torch.uint8))


class Counter:
    def __init__(self, monkeypatch, owner, name):
        self.n = 0
        fn = getattr(owner, name)

        def spy(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        monkeypatch.setattr(owner, name, spy)


_want = {}


def yardstick(I, y, uv, out, matrix="bt601", full_range=False, key=None):
    """The RGB kernel on the converted frame (converted on the CPU): ``(planes, pixels)`` on the GPU, computed
    once per ``key`` and left unchanged."""
    if key is None or key not in _want:
        rgb = I.nv12_to_rgb(y.cpu(), uv.cpu(), matrix, full_range).cuda()
        res = I.image_patch_planes(rgb, out, P, MEAN, STD, want_pixels=True)
        if key is None:
            return res
        _want[key] = res
    return _want[key]


def same(I, y, uv, out, want, matrix="bt601", full_range=False):
    planes, px = I.nv12_patch_planes(y, uv, out, P, MEAN, STD, matrix, full_range, want_pixels=True)
    only, none = I.nv12_patch_planes(y, uv, out, P, MEAN, STD, matrix, full_range)
    torch.cuda.synchronize()
    assert none is None and planes.dtype == torch.bfloat16 and px.dtype == torch.float32
    assert torch.equal(px, want[1]), "pixels"
    assert torch.equal(planes, want[0]) and torch.equal(only, want[0]), "planes"


def pitched(plane, pitch, pad, lead=0, tail=0):
    """``plane`` ``[B, rows, rowbytes]`` copied into a fresh GPU allocation with ``pitch`` bytes between rows,
    ``lead`` bytes before the first and ``tail`` after the last row's bytes, every other byte ``pad``; the view."""
    B, rows, rb = plane.shape
    per = (rows - 1) * pitch + rb
    buf = torch.full((lead + B * per + tail,), pad, dtype=torch.uint8, device="cuda")
    view = buf.as_strided((B, rows, rb), (per, pitch, 1), lead)
    view.copy_(plane)
    return view


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_nv12_equals_the_rgb_kernel_on_the_converted_frame(K, I, monkeypatch, case):
    h, w, H, W, fused = case
    y, uv = nv12_frame(h, w)
    want = yardstick(I, y, uv, (H, W), key=case)
    fallback = Counter(monkeypatch, I, "nv12_to_rgb")
    same(I, y.cuda(), uv.cuda(), (H, W), want)
    assert fallback.n == (0 if fused else 2)
    # the GPU conversion (the fallback's first half) is the CPU's
    assert torch.equal(I.nv12_to_rgb(y.cuda(), uv.cuda()).cpu(), I.nv12_to_rgb(y, uv))


@pytest.mark.parametrize("matrix,full_range", COMBOS, ids=[f"{m}-{'full' if f else 'limited'}" for m, f in COMBOS])
def test_every_matrix_and_range(K, I, matrix, full_range):
    y, uv = nv12_frame(48, 64, seed=1)
    want = yardstick(I, y, uv, (80, 96), matrix, full_range)
    same(I, y.cuda(), uv.cuda(), (80, 96), want, matrix, full_range)
    if (matrix, full_range) != COMBOS[0]:     # and the table matters: another one gives other pixels
        assert not torch.equal(want[1], yardstick(I, y, uv, (80, 96), *COMBOS[0])[1])


def test_pitch_padding_batch_stride_and_torch_backend(K, I, monkeypatch):
    h, w, out = 48, 64, (80, 96)
    y3, uv3 = nv12_frame(h, w, batch=3, seed=2)
    y, uv = y3[:2], uv3[:2]
    assert not torch.equal(y[0], y[1]) and not torch.equal(uv[0], uv[1])
    want = yardstick(I, y, uv, out)
    assert not torch.equal(want[1][0], want[1][1])
    fallback = Counter(monkeypatch, I, "nv12_to_rgb")
    for pad in (255, 0):
        # Y pitch 80 and UV pitch 96 for w = 64; batch 2 of a batch-3 allocation with a gap between the frames
        gy = torch.full((3, h * 80 + 33), pad, dtype=torch.uint8, device="cuda")
        guv = torch.full((3, (h // 2) * 96 + 7), pad, dtype=torch.uint8, device="cuda")
        yv = gy[:, :h * 80].unflatten(1, (h, 80))[:2, :, :w]
        uvv = guv[:, :(h // 2) * 96].unflatten(1, (h // 2, 96))[:2, :, :w].unflatten(2, (w // 2, 2))
        yv.copy_(y)
        uvv.copy_(uv)
        assert yv.stride() == (h * 80 + 33, 80, 1) and uvv.stride() == ((h // 2) * 96 + 7, 96, 2, 1)
        assert not yv.is_contiguous() and not uvv.is_contiguous()
        same(I, yv, uvv, out, want)
    assert fallback.n == 0
    # the torch backend takes the composition on the GPU, and agrees
    K.set_backend("torch")
    try:
        got = I.nv12_patch_planes(yv, uvv, out, P, MEAN, STD, want_pixels=True)
        ref = I.image_patch_planes(I.nv12_to_rgb(yv, uvv), out, P, MEAN, STD, want_pixels=True)
    finally:
        K.set_backend("hip")
    assert fallback.n == 2 and torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.mark.parametrize("hw,out", (((48, 64), (80, 96)), ((37, 53), (80, 112))), ids=("48x64", "37x53"))
def test_alignment_and_storage_ends(K, I, hw, out):
    y, uv = nv12_frame(*hw, seed=3)
    want = yardstick(I, y, uv, out, key=("align",) + hw)
    u2 = uv.flatten(2)                                        # [1, ch, 2 * cw]
    w = hw[1]
    # (Y lead, Y pitch, UV lead, UV pitch, UV tail): views 1, 2 and 3 bytes into their storage (byte loads on
    # every row, on alternate rows with an odd pitch); 0 / 0: the Y plane starts on the storage's first byte and
    # the UV plane ends on its last (dword loads, and the bytes of the dword that would pass the end)
    for ylead, ypitch, clead, cpitch, ctail in ((1, w + 11, 2, u2.shape[2] + 4, 5), (2, w + 2, 3, u2.shape[2] + 1, 1),
                                                (3, w, 1, u2.shape[2], 0), (0, w, 0, u2.shape[2], 0),
                                                (0, (w + 3) // 4 * 4, 0, (u2.shape[2] + 3) // 4 * 4, 0)):
        for pad in (255, 0):
            yv = pitched(y, ypitch, pad, ylead)
            uvv = pitched(u2, cpitch, pad, clead, ctail).unflatten(2, (-1, 2))
            ys, cs = yv.untyped_storage(), uvv.untyped_storage()
            assert yv.data_ptr() - ys.data_ptr() == ylead
            assert uvv.data_ptr() + (u2.shape[1] - 1) * cpitch + u2.shape[2] + ctail == cs.data_ptr() + cs.nbytes()
            same(I, yv, uvv, out, want)
    # one decoder surface: Y from the storage's first byte, the UV rows behind it to its last
    if hw[0] % 2 == 0:
        from walkai_nos_amd.models.workload.processor import Nv12
        pitch = 80
        buf = torch.full(((hw[0] * 3 // 2 - 1) * pitch + w,), 255, dtype=torch.uint8, device="cuda")
        f = Nv12.from_buffer(buf, hw[0], w, pitch)
        f.y.copy_(y[0])
        f.uv.copy_(uv[0])
        assert f.uv.data_ptr() + (hw[0] // 2 - 1) * pitch + w == buf.data_ptr() + buf.numel()
        same(I, f.y, f.uv, out, want)


def test_grid_stride_on_a_slice(K, I):
    # 2 x 13 x 11 tiles (pixels wanted, H and W no multiple of the patch) on the 128 workgroups of a 32-CU slice
    h, w, out = 53, 37, (200, 170)
    y, uv = nv12_frame(h, w, batch=2, seed=4)
    want = yardstick(I, y, uv, out)
    assert want[0].shape[1] == 2 * 12 * 10
    yd, uvd = y.cuda(), uv.cuda()
    same(I, yd, uvd, out, want)
    K.set_slice_cus(32)
    try:
        assert I.image_wgs() == 128
        same(I, yd, uvd, out, want)
    finally:
        K.set_slice_cus(None)


def test_bad_arguments_raise_and_launch_nothing(K, I):
    import ctypes
    y, uv = (t.cuda() for t in nv12_frame(48, 64))
    out = (80, 96)

    def run(yy, cc, **kw):
        return I.nv12_patch_planes(yy, cc, out, P, MEAN, STD, **kw)
    # the library's own checks: rows that overlap (pitch < w), for Y and for UV
    with pytest.raises(RuntimeError, match="Y pitch is smaller than the width"):
        run(y.as_strided((1, 48, 64), (48 * 64, 32, 1)), uv)
    with pytest.raises(RuntimeError, match="UV pitch is smaller"):
        run(y, uv.as_strided((1, 24, 32, 2), (24 * 64, 62, 2, 1)))
    with pytest.raises(ValueError, match="UV plane of shape"):
        run(y, uv[:, :-1])
    with pytest.raises(ValueError, match="UV plane of shape"):
        run(y, uv[:, :, :-1])
    with pytest.raises(ValueError, match="one device"):
        run(y, uv.cpu())
    with pytest.raises(ValueError, match="uint8"):
        run(y.float(), uv)
    with pytest.raises(ValueError, match="uint8"):
        run(y, uv.to(torch.int32))
    with pytest.raises(ValueError, match="matrix"):
        run(y, uv, matrix="bt2020")
    # the entry point itself: null operands, bounds that do not contain a plane, and what the u8 entry checks
    L = I._L()
    tabs = I._device_tables(48, 64, 80, 96, P, y.device)
    planes = torch.zeros(3, 30, 768, dtype=torch.bfloat16, device="cuda")
    F3, T12 = ctypes.c_float * 3, ctypes.c_int * 12
    ylo, yhi = I._storage_bounds(y)
    clo, chi = I._storage_bounds(uv)

    def call(yp=y.data_ptr(), ylo=ylo, yhi=yhi, cp=uv.data_ptr(), clo=clo, chi=chi, ypitch=64, cpitch=64, ybs=0, cbs=0,
             table=T12(*I.nv12_table()), B=1, p=P, gh=5, gw=6, taps=I.TAPS, fh=tabs[4], fw=tabs[5]):
        return L.nos_image_patch_planes_nv12(yp, ylo, yhi, cp, clo, chi, ypitch, cpitch, ybs, cbs, table,
                                             planes.data_ptr(), None, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                             tabs[2].data_ptr(), tabs[3].data_ptr(), 80, 96, taps, fh, fw, F3(1, 1, 1),
                                             F3(0, 0, 0), B, 48, 64, 80, 96, p, gh, gw, 0,
                                             torch.cuda.current_stream().cuda_stream)
    for bad in (dict(yp=None), dict(cp=None), dict(table=None), dict(ypitch=63), dict(cpitch=62), dict(ylo=ylo + 1),
                dict(yhi=yhi - 1), dict(clo=clo + 1), dict(chi=chi - 1), dict(ylo=None), dict(ypitch=65),
                dict(B=2, ybs=1), dict(table=T12(1 << 23, *I.nv12_table()[1:])), dict(table=T12(*I.nv12_table()[:9], 256, 128, 128)),
                dict(B=0), dict(p=15), dict(gh=6), dict(taps=8), dict(fh=73), dict(fw=70)):
        assert call(**bad) == -1 and L.nos_image_last_error(), bad
    torch.cuda.synchronize()
    assert not planes.any()                    # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert planes.any()


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


def test_detect_image_eager_and_graph_replay_on_a_new_frame(K, I, model, monkeypatch):
    from walkai_nos_amd.models.workload.processor import Nv12
    h, w, pitch = 48, 64, 80
    frames = []
    for seed in (5, 6):
        g = torch.Generator().manual_seed(seed)
        frames.append(torch.randint(0, 256, ((h * 3 // 2) * pitch,), generator=g, dtype=torch.uint8))
    buf = frames[0].cuda()
    frame = Nv12.from_buffer(buf, h, w, pitch)
    fused = Counter(monkeypatch, I, "nv12_patch_planes")
    converted = Counter(monkeypatch, I, "nv12_to_rgb")
    with torch.no_grad():
        s = model.detect_image(frame, 0.0)["scores"][0].sort().values
        thr = 0.5 * (s[49] + s[50]).item()      # half of the rows survive on the first frame
        first = {k: v.clone() for k, v in model.detect_image(frame, thr).items()}
        assert fused.n == 2 and converted.n == 0 and K.x3_active(model.pos_embed)
        rgb = frame.rgb()
        want = model.detect_image(rgb, thr)
    assert len(first) == 6 and first["count"].tolist() == [50]
    for k, v in want.items():
        assert torch.equal(first[k], v), k
    assert torch.equal(model.processor.preprocess(frame), model.processor.preprocess(rgb))
    # boxes in pixels of the Y plane
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
    # the decoder writes the next frame into the same surface: the graph reads it by address
    buf.copy_(frames[1])
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        second = model.detect_image(frame, thr)
    for k, v in second.items():
        assert torch.equal(held[k], v), k
    assert not torch.equal(held["logits"], first["logits"])
    del graph


# ---- the pod client (last: it starts a process, and nothing follows it if it fails) --------------
def test_pod_client_end_to_end_nv12():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "walkai_nos_amd.dataplane.client", "--end-to-end",
           "--pixel-format", "nv12", "--image-hw", "48,64", "--size", "80,133", "--seconds", "1", "--threshold", "0.0"]
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert p.stdout.readline().strip() == "READY"
        p.stdin.write(f"GO {time.time()}\n")
        p.stdin.flush()
        lines = p.stdout.read().strip().splitlines()
        assert p.wait(timeout=60) == 0
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["pixel_format"] == "nv12" and out["end_to_end"] is True and out["input_hw"] == [80, 96]
    assert out["inferences"] > 0 and out["detections"] == 100      # threshold 0 keeps every detection token
