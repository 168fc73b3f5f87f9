"""``mosaic_k`` (``csrc/image_mosaic.h``) on the GPU against ``ops.image.mosaic_reference`` on the CPU twin of the same
surface (the same seeded bytes; ``test_mosaic.py`` holds the reference to a loop): equality of the whole allocation, the
reference never called on the GPU side. There are no tolerances."""
import ctypes
import dataclasses
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
H, W = 66, 130      # 2 x 3 tiles; the last cells are 2 pixels thick, at cell 64 the edge cells 64 x 2


def mixed_scene():
    """Inside a cell, across tile borders, on and just past a cell border, half and wholly outside, NaN, score 0, an
    unselected label (3), labels outside ``[0, L)``."""
    boxes = [[5.2, 5.1, 6.5, 6.9], [60, 20, 70, 30], [100, 60, 110, 66], [16.5, 40.5, 32.0, 44.0],
             [16.5, 48.5, C.ulp_up(32.0), 50.0], [120, -10, 140, 8], [200, 10, 220, 20], [-30, -30, -2, -2],
             [float("nan"), 10, 50, 20], [80, 30, 90, 40], [40, 50, 50, 60], [84, 44, 90, 50], [92, 44, 96, 50]]
    return C.Scene("mixed", [0.9] * 9 + [0.0] + [0.9] * 3, [0, 1, 4, 5, 6, 7, 0, 1, 4, 5, 3, 8, -1], boxes)


def compare(I, monkeypatch, layouts, h, w, sc, cell, paint=None, fallbacks=0, device="cuda"):
    """``I.mosaic`` on the GPU surface against the reference on its CPU twin; the bytes changed."""
    ref = Counter(monkeypatch, I, "mosaic_reference")
    changed = 0
    for layout in layouts:
        gpu, cpu = C.surface(layout, h, w, device=device), C.surface(layout, h, w, device="cpu")
        before = cpu.storage.clone()
        select = torch.tensor(sc.modes, dtype=torch.uint8)
        kw = dict(min_hits=sc.min_hits, cell=cell)
        (paint or I.mosaic)(gpu.target, *sc.tensors(device), select=select.to(device), **kw)
        n = ref.n
        I.mosaic_reference(cpu.target, *sc.tensors("cpu"), select=select, **kw)
        ref.n = n       # (the twin's own call)
        assert torch.equal(gpu.storage.cpu(), cpu.storage), f"{layout} {h}x{w} cell {cell} {sc.name}"
        changed += int((cpu.storage != before).sum())
    assert ref.n == fallbacks
    return changed


@pytest.mark.parametrize("cell", (4, 16, 64))
@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_mosaic_every_layout(K, I, monkeypatch, layout, cell):
    assert compare(I, monkeypatch, (layout,), H, W, mixed_scene(), cell) > 0


@pytest.mark.parametrize("cell", (4, 64))
@pytest.mark.parametrize("size", ((64, 64), (2, 2), (65, 67)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_mosaic_sizes(K, I, monkeypatch, size, cell):
    h, w = size
    layouts = tuple(C.PACKED) if h % 2 else ("rgb", "crop", "nv12", "i422", "p010", "uyvy")
    assert compare(I, monkeypatch, layouts, h, w, C.edge_scene(h, w), cell) > 0


@pytest.mark.parametrize("N", (1, 65, 257, 1024))
def test_mosaic_rows(K, I, monkeypatch, N):
    assert compare(I, monkeypatch, ("bgr", "nv12", "yvyu"), H, W, C.lattice_scene(N, H, W), 4) > 0


@pytest.mark.parametrize("count", (0, -3, 70))
def test_mosaic_count_is_clamped(K, I, monkeypatch, count):
    sc = C.lattice_scene(65, H, W, seed=3, total=90, count=count)
    assert (compare(I, monkeypatch, ("rgba", "nv21"), H, W, sc, 8) == 0) == (count <= 0)


def test_mosaic_track_ids_and_min_hits(K, I, monkeypatch):
    sc = C.lattice_scene(100, H, W)             # ids, hits 1..4, min_hits 2
    held = compare(I, monkeypatch, ("nv12",), H, W, sc, 4)
    assert 0 < held < compare(I, monkeypatch, ("nv12",), H, W, dataclasses.replace(sc, min_hits=1), 4)


def test_mosaic_twice_changes_nothing(K, I, monkeypatch):
    ref = Counter(monkeypatch, I, "mosaic_reference")
    sc = mixed_scene()
    for layout in ("bgra", "i010", "yuy2"):
        surf = C.surface(layout, H, W, device="cuda")
        args = dict(select=torch.tensor(sc.modes, dtype=torch.uint8).cuda(), cell=8)
        I.mosaic(surf.target, *sc.tensors("cuda"), **args)
        once = surf.storage.clone()
        I.mosaic(surf.target, *sc.tensors("cuda"), **args)
        assert torch.equal(surf.storage, once)
    assert ref.n == 0


def test_mosaic_entries_refuse_before_any_launch(K, I):
    sc = mixed_scene()
    count, scores, labels, boxes, _, _ = sc.tensors("cuda")
    select = torch.tensor(sc.modes, dtype=torch.uint8).cuda()
    for layout in ("bgra", "nv12"):
        surf = C.surface(layout, H, W, device="cuda")
        before = surf.storage.clone()
        s = I.overlay_surface(surf.target)

        def call(sel, cell):
            tail = [count.data_ptr(), scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(), None, None, sc.N, sel,
                    len(sc.modes), 1, cell, None]
            if s.packed is not None:
                data, order = s.packed
                return I._L().nos_mosaic_packed(data.data_ptr(), *I._storage_bounds(data), data.stride(1), order.encode(),
                                                s.h, s.w, *tail)
            src = I.yuv_src(*s.yuv, (0,) * 12)
            return I._L().nos_mosaic_yuv(ctypes.byref(src), s.h, s.w, *tail)
        for sel, cell in [(select.data_ptr(), c) for c in (0, 6, 128)] + [(None, 8)]:
            assert call(sel, cell) == -1 and I._L().nos_image_last_error()
        torch.cuda.synchronize()
        assert torch.equal(surf.storage, before)
        assert call(select.data_ptr(), 8) == 0
        torch.cuda.synchronize()
        assert not torch.equal(surf.storage, before)


def test_mosaic_other_inputs_take_the_reference(K, I, monkeypatch):
    sc = mixed_scene()

    def double(target, count, scores, labels, boxes, ids, hits, **kw):
        return I.mosaic(target, count, scores.double(), labels, boxes.double(), ids, hits, **kw)
    compare(I, monkeypatch, ("nv12",), H, W, sc, 8, double, 1)
    compare(I, monkeypatch, ("bgr",), H, W, C.lattice_scene(1025, H, W), 8, None, 1)
    compare(I, monkeypatch, ("p010",), H, W, sc, 8, None, 1, device="cpu")
    K.set_backend("torch")
    try:
        compare(I, monkeypatch, ("uyvy",), H, W, sc, 8, None, 1)
    finally:
        K.set_backend("hip")


def test_annotate_pixelates_in_the_captured_graph(K, I, monkeypatch, model):
    """One graph replayed on two frames: the target equals both references on a CPU copy with the returned lists."""
    from walkai_nos_amd.models.workload.overlay import Overlay
    refs = [Counter(monkeypatch, I, name) for name in ("mosaic_reference", "overlay_reference")]
    h, w = 96, 130
    src, dst = C.surface("nv12", h, w, seed=20, device="cuda"), C.surface("nv12", h, w, seed=21, device="cuda")
    twin = C.surface("nv12", h, w, seed=21, device="cpu")
    overlay = Overlay(thickness=2, scale=1, pixelate=[k for k in range(91) if k % 7], modes={k: 1 for k in range(1, 45)}, num_labels=91)
    clean = src.storage.clone()
    with torch.no_grad():
        thr = model.detect_image(src.target, 0.0)["scores"].flatten().sort().values[-40].item() - 1e-6
        model.annotate_image(src.target, overlay, thr, None, dst.target)    # a warm-up: the tables are made outside the capture
    src.storage.copy_(clean)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        held = model.annotate_image(src.target, overlay, thr, None, dst.target)
    t, s = overlay.sizes(h, w)
    kw = dict(thickness=t, scale=s, modes=torch.tensor(overlay.modes, dtype=torch.uint8),
              codes=I.overlay_codes(overlay.palette, overlay.redact_colour, twin.target))
    select = torch.tensor([int(k in overlay.pixelate) for k in range(91)], dtype=torch.uint8)
    g = torch.Generator().manual_seed(8)
    total = 0
    for fresh in (clean, torch.randint(0, 256, src.storage.shape, generator=g, dtype=torch.uint8)):
        src.storage.copy_(fresh)
        twin.storage.copy_(torch.randint(0, 256, src.storage.shape, generator=g, dtype=torch.uint8))
        dst.storage.copy_(twin.storage)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        lists = [held[k].detach().cpu().reshape(shape) for k, shape in (("count", (1,)), ("scores", (-1,)),
                                                                      ("labels", (-1,)), ("boxes", (-1, 4)))]
        calls = [r.n for r in refs]
        before = twin.storage.clone()
        I.mosaic_reference(twin.target, *lists, select=select, cell=4)
        total += int((twin.storage != before).sum())
        I.overlay_reference(twin.target, *lists, **kw)
        assert [r.n - c for r, c in zip(refs, calls)] == [1, 1]      # the twin's own two calls, none from the GPU side
        assert torch.equal(dst.storage.cpu(), twin.storage)
        print(f"[mosaic] annotate_image nv12 {h}x{w}: {int(lists[0])} rows, {total} bytes pixelated so far")
    assert total > 0
    del graph


def test_pod_client_pixelates():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "walkai_nos_amd.dataplane.client", "--end-to-end",
           "--seconds", "1", "--image-hw", "96,128", "--size", "80,133", "--threshold", "0.0", "--annotate",
           "--pixel-format", "nv12", "--pixelate", "1,2,3"]
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert p.stdout.readline().strip() == "READY"
        rest, _ = p.communicate(f"GO {time.time()}\n", timeout=120)
    finally:
        p.kill()
    out = json.loads(rest.strip().splitlines()[-1])
    assert p.returncode == 0 and out["end_to_end"] and out["inferences"] > 0 and out["annotate"]["changed_bytes"] > 0
