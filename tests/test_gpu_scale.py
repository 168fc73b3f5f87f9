"""``rescale_k`` on the GPU against ``ops.image.rescale_reference`` on the CPU twin of the same seeded surfaces: the whole
target allocation after a second call on samples overwritten with 0x5A, the source unchanged, the reference never called."""
import ctypes
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import overlay_case as C
from test_gpu_overlay import Counter, I, K, model, small_model  # noqa: F401  (fixtures, and the two-layer model)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 66, 130
ids = lambda s: "x".join(str(v) for v in s) if isinstance(s[0], int) else "-".join(ids(v) for v in s)     # noqa: E731


def overwrite(I, target):      # 0x5A in every byte of every sample, and nowhere else
    for view, *_ in I.overlay_surface(target).samples:
        view.fill_(0x5A) if view.element_size() == 1 else view.view(torch.int16).fill_(0x5A5A)


def compare(I, monkeypatch, layouts, hw, HW, fallbacks=0, device="cuda", ones=False):
    """``I.rescale`` between GPU surfaces against the reference between their CPU twins; the last target's twin."""
    ref = Counter(monkeypatch, I, "rescale_reference")
    for layout in layouts:
        src, dst, twin, want = (C.surface(layout, *size, seed=seed, device=d) for size, seed, d in
                                ((hw, 1, device), (HW, 2, device), (hw, 1, "cpu"), (HW, 2, "cpu")))
        if ones:
            src.storage.fill_(0xFF), twin.storage.fill_(0xFF)
        if not fallbacks:
            overwrite(I, I.rescale(src.target, dst.target))
        assert I.rescale(src.target, dst.target) is dst.target
        n = ref.n
        I.rescale_reference(twin.target, want.target)
        ref.n = n       # (the twin's own call)
        assert torch.equal(dst.storage.cpu(), want.storage) and torch.equal(src.storage.cpu(), twin.storage), (layout, hw, HW)
    assert ref.n == fallbacks * len(layouts)
    return want


@pytest.mark.parametrize("size", ((66, 130), (34, 50), (2, 2), (100, 258), (20, 198)), ids=ids)
@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_rescale_every_layout(K, I, monkeypatch, layout, size):
    compare(I, monkeypatch, (layout,), (H, W), size)


@pytest.mark.parametrize("sizes", (((33, 17), (1, 1)), ((7, 31), (33, 17)),        # odd sizes, then past one chunk
                                   ((2, 1100), (2, 300)), ((2, 1100), (2, 1500)), ((2, 4200), (2, 300)), ((2, 4200), (2, 13)),
                                   ((700, 4), (90, 4)), ((700, 4), (900, 4)), ((700, 4), (20, 4))), ids=ids)
def test_rescale_odd_sizes_and_past_one_chunk(K, I, monkeypatch, sizes):
    (h, w), (Hh, Ww) = sizes
    tile, columns, rows = (getattr(I._L(), f"nos_rescale_{k}")() for k in ("tile", "column_chunk", "row_chunk"))
    assert tile < 300 and columns < 1100 and rows < 90
    if w == 4200:       # the source footprint of one target tile, not only the row, spans several column chunks
        assert min(tile * w // Ww, w) > 2 * columns
    if Hh == 20:        # and the source rows of one output row several row chunks
        assert h // Hh > 4 * rows
    compare(I, monkeypatch, ("rgb", "crop", "i444", "nv12", "yuy2") if max(h, w) < 40 else ("bgr", "nv12", "uyvy", "p010"), *sizes)


@pytest.mark.parametrize("size", ((3, 5), (1026, 1030)), ids=ids)
def test_rescale_the_wide_sum(K, I, monkeypatch, size):
    assert 2050 * 2050 * 1023 >= 2 ** 32        # code 1023 in every sample: a 32-bit accumulator cannot hold the sum
    for layout in ("i010", "p010"):
        want = compare(I, monkeypatch, (layout,), (2050, 2050), size, ones=True)
        for view, *_ in I.overlay_surface(want.target).samples:
            assert (view.view(torch.int16).to(torch.int32) & 0xffff == (0xFFC0 if layout == "p010" else 1023)).all()


def test_rescale_entries_refuse_before_any_launch(K, I):
    L = I._L()
    deep = I.overlay_surface(C.surface("p010", 4, 6, device="cuda").target)
    for layout in ("rgba", "nv12"):
        src, dst = C.surface(layout, 6, 10, device="cuda"), C.surface(layout, 4, 6, seed=2, device="cuda")  # (held)
        dst.storage.fill_(0x5A)
        s, d = I.overlay_surface(src.target), I.overlay_surface(dst.target)

        def call(h=6, H=4, null=False, size=None, to=d):
            if s.packed is not None:
                ends = [[t.data_ptr(), *I._storage_bounds(t), t.stride(1)] for t in (s.packed[0], to.packed[0])]
                ends[0][0] = None if null else ends[0][0]
                return L.nos_rescale_packed(*ends[0], h, 10, *ends[1], H, 6, b"rgba", None)
            a, b = I.yuv_src(*s.yuv, (0,) * 12), I.yuv_src(*to.yuv, (0,) * 12)
            a.plane[1].p = None if null else a.plane[1].p
            a.size = ctypes.sizeof(a) if size is None else size
            return L.nos_rescale_yuv(ctypes.byref(a), h, 10, ctypes.byref(b), H, 6, None)
        bad = [dict(null=True), dict(h=0), dict(H=8193), dict(to=s)]       # (to=s: the two storage ranges meet)
        for kw in bad + ([] if s.packed is not None else [dict(size=8), dict(to=deep)]):
            assert call(**kw) == -1 and L.nos_image_last_error(), kw
        assert (dst.storage == 0x5A).all() and call() == 0 and not (dst.storage == 0x5A).all()     # (.all() synchronises)


def test_rescale_other_inputs_take_the_reference(K, I, monkeypatch):
    compare(I, monkeypatch, ("p010",), (H, W), (34, 50), fallbacks=1, device="cpu")
    compare(I, monkeypatch, ("rgb",), (2, 8200), (2, 40), fallbacks=1)
    compare(I, monkeypatch, ("nv12",), (3, 40), (8194, 2), fallbacks=1)
    K.set_backend("torch")
    try:
        compare(I, monkeypatch, ("uyvy",), (H, W), (34, 50), fallbacks=1)
    finally:
        K.set_backend("hip")


def test_annotate_and_scale_in_a_captured_graph(K, I, monkeypatch, model):
    """Captured once, replayed on two frames: ``scaled`` is the reference of the painted frame, in the cached planes."""
    from walkai_nos_amd.models.workload.overlay import Overlay
    from walkai_nos_amd.models.workload.scaler import Scaler
    from walkai_nos_amd.models.workload.tracker import Tracker
    ref = Counter(monkeypatch, I, "rescale_reference")
    src, twin = C.surface("nv12", 96, 130, seed=20, device="cuda"), C.surface("nv12", 96, 130, seed=20, device="cpu")
    overlay = Overlay(thickness=2, scale=1, redact=range(0, 91, 3), num_labels=91)
    tracker, scaler = Tracker(64, device="cuda"), Scaler((48, 66))
    with torch.no_grad():
        thr = model.detect_image(src.target, 0.0)["scores"].flatten().sort().values[-40].item() - 1e-6
        model.annotate_image(src.target, overlay, thr, tracker, scaler=scaler)     # a warm-up, outside the capture
    tracker.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        scaled = model.annotate_image(src.target, overlay, thr, tracker, scaler=scaler)["scaled"]
    tracker.reset()
    assert type(scaled) is type(src.target) and scaled.y.shape == (48, 66) and scaled.uv.shape == (24, 33, 2)
    assert len(I._scale_buffers) - I._scale_buffers.unpinned() == 1 and scaler.target(src.target).y is scaled.y
    want = Scaler((48, 66)).target(twin.target)
    for fresh in (twin.storage.clone(), twin.storage.flip(0)):
        src.storage.copy_(fresh)
        overwrite(I, scaled)
        graph.replay()
        twin.storage.copy_(src.storage.cpu())       # the painted frame (the copy synchronises)
        assert not torch.equal(twin.storage, fresh)
        I.rescale_reference(twin.target, want)
        assert torch.equal(scaled.y.cpu(), want.y) and torch.equal(scaled.uv.cpu(), want.uv)
    assert ref.n == 2 and scaler.target(src.target).uv is scaled.uv     # the twin's own two calls, none from the GPU side
    del graph


def test_pod_client_scales_the_annotated_frame():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = f"timeout -k 10 240 {sys.executable} -m walkai_nos_amd.dataplane.client --end-to-end --seconds 1 --image-hw 96,128 " \
          "--size 80,133 --threshold 0.0 --annotate --scale-out 48,64 --pixel-format nv12"
    p = subprocess.Popen(cmd.split(), cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert p.stdout.readline().strip() == "READY"
        rest, _ = p.communicate(f"GO {time.time()}\n", timeout=120)
    finally:
        p.kill()
    out = json.loads(rest.strip().splitlines()[-1])
    assert p.returncode == 0 and out["inferences"] > 0 and out["scaled"]["hw"] == [48, 64] and out["scaled"]["nonzero_bytes"] > 0
