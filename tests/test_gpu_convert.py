"""``convert_k`` on the GPU against ``ops.image.convert_reference`` on the CPU twin of the same seeded surfaces: the whole
target allocation (lead, tail, pitch padding, crop parent, fourth bytes), the source unchanged, the reference never called
from the GPU side."""
import json
import os
import subprocess
import sys
import time
from dataclasses import replace

import pytest
import torch

import overlay_case as C
from test_gpu_overlay import Counter, I, K, model, small_model  # noqa: F401  (fixtures, and the two-layer model)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME, SHRINK, GROW, ONE, TINY = ((19, 261), (19, 261)), ((19, 261), (11, 135)), ((7, 9), (19, 133)), ((5, 3), (1, 1)), \
    ((1, 1), (2, 3))
CASES = (("rgb", "nv21", SAME), ("crop", "i420", SHRINK), ("nv12", "bgr", SAME), ("yv12", "rgba", SHRINK),
         ("yuy2", "nv16", SAME), ("p010", "yvyu", GROW), ("i420-bilinear", "p010", SAME), ("p010-pq", "i010", SHRINK),
         ("rgb", "i444", GROW), ("nv12", "p010", ONE), ("yuy2", "nv21", TINY), ("p010-pq", "bgr", SAME),
         ("i420-bilinear", "yvyu", SHRINK), ("crop", "i010", GROW), ("yv12", "nv16", ONE))


def source(name, h, w, device, seed=1):
    """The surface of a source and the frame that reads it: ``-bilinear`` and ``-pq`` say how."""
    layout, _, how = name.partition("-")
    surf = C.surface(layout, h, w, seed=seed, device=device, matrix="bt2020" if how == "pq" else "bt601")
    kw = {"bilinear": dict(chroma="bilinear"), "pq": dict(transfer="pq"), "": {}}[how]
    return surf, replace(surf.target, **kw) if kw else surf.target


def compare(I, monkeypatch, src, dst, hw, HW, fallbacks=0):
    ref = Counter(monkeypatch, I, "convert_reference")
    (gpu, frame), (twin, twin_frame) = source(src, *hw, "cuda"), source(src, *hw, "cpu")
    out, want = C.surface(dst, *HW, seed=2, device="cuda", matrix="bt709"), C.surface(dst, *HW, seed=2, matrix="bt709")
    assert I.convert(frame, out.target) is out.target and ref.n == fallbacks
    I.convert_reference(twin_frame, want.target)
    assert torch.equal(out.storage.cpu(), want.storage) and torch.equal(gpu.storage.cpu(), twin.storage)
    assert not torch.equal(want.storage, C.surface(dst, *HW, seed=2).storage)


@pytest.mark.parametrize("src,dst,sizes", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v[0] + v[1])))
def test_convert_is_the_reference(K, I, monkeypatch, src, dst, sizes):
    L = I._L()
    assert L.nos_convert_tile() < 133 and L.nos_convert_column_chunk() < 261 and L.nos_convert_row_chunk() < 19
    compare(I, monkeypatch, src, dst, *sizes)


def test_convert_past_the_limits_takes_the_reference(K, I, monkeypatch):
    compare(I, monkeypatch, "nv12", "bgr", (2, 8194), (2, 40), fallbacks=1)
    K.set_backend("torch")
    try:
        compare(I, monkeypatch, "yuy2", "nv12", *SHRINK, fallbacks=1)
    finally:
        K.set_backend("hip")


def test_convert_in_a_captured_graph(K, I, monkeypatch):
    """Captured once, replayed twice on a rewritten source, against the eager reference each time."""
    ref = Counter(monkeypatch, I, "convert_reference")
    (gpu, frame), (twin, twin_frame) = source("p010-pq", 19, 261, "cuda"), source("p010-pq", 19, 261, "cpu")
    out, want = C.surface("nv12", 11, 135, seed=2, device="cuda"), C.surface("nv12", 11, 135, seed=2)
    I.convert(frame, out.target)        # a warm-up, outside the capture: the library and the HDR tables
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        I.convert(frame, out.target)
    for k in (5, 6):
        fresh = C.surface("p010", 19, 261, seed=k).storage
        gpu.storage.copy_(fresh), twin.storage.copy_(fresh)
        for view, *_ in I.overlay_surface(out.target).samples:
            view.fill_(0x5A)
        graph.replay()
        I.convert_reference(twin_frame, want.target)
        assert torch.equal(out.storage.cpu(), want.storage)
    assert ref.n == 2       # the twin's own calls
    del graph


def test_annotate_image_scales_into_another_format(K, I, monkeypatch, model):
    from walkai_nos_amd.models.workload.overlay import Overlay
    from walkai_nos_amd.models.workload.scaler import Scaler
    ref = Counter(monkeypatch, I, "convert_reference")
    src, twin = C.surface("bgra", 96, 130, seed=20, device="cuda"), C.surface("bgra", 96, 130, seed=20)
    overlay, scaler = Overlay(thickness=2, scale=1, redact=range(0, 91, 3), num_labels=91), Scaler((48, 66), format="nv12")
    with torch.no_grad():
        thr = model.detect_image(src.target, 0.0)["scores"].flatten().sort().values[-40].item() - 1e-6
        scaled = model.annotate_image(src.target, overlay, thr, scaler=scaler)["scaled"]
    assert ref.n == 0 and type(scaled).__name__ == "Nv12" and scaled.y.shape == (48, 66) and scaled.uv.shape == (24, 33, 2)
    assert (scaled.matrix, scaled.full_range) == ("bt709", False) and scaler.target(src.target).y.data_ptr() == scaled.y.data_ptr()
    painted = src.storage.cpu()
    assert not torch.equal(painted, twin.storage)
    twin.storage.copy_(painted)
    want = I.convert_reference(twin.target, Scaler((48, 66), format="nv12").target(twin.target))
    assert torch.equal(scaled.y.cpu(), want.y) and torch.equal(scaled.uv.cpu(), want.uv)


def test_pod_client_converts_the_annotated_frame():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = f"timeout -k 10 240 {sys.executable} -m walkai_nos_amd.dataplane.client --end-to-end --seconds 1 --image-hw 96,128 " \
          "--size 80,133 --threshold 0.0 --annotate --scale-out 48,64 --scale-out-format nv12 --pixel-format bgra"
    p = subprocess.Popen(cmd.split(), cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert p.stdout.readline().strip() == "READY"
        rest, _ = p.communicate(f"GO {time.time()}\n", timeout=120)
    finally:
        p.kill()
    out = json.loads(rest.strip().splitlines()[-1])
    assert p.returncode == 0 and out["inferences"] > 0 and out["scaled"]["nonzero_bytes"] > 0
    assert (out["scaled"]["hw"], out["scaled"]["format"]) == ([48, 64], "nv12")
