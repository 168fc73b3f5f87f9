"""``blur_snapshot_k`` / ``blur_k`` (``csrc/image_blur.h``) on the GPU against ``ops.image.blur_reference`` on the CPU twin
of the same surface (the same seeded bytes; ``test_blur.py`` holds the reference to a loop): equality of the whole
allocation, the reference never called on the GPU side. There are no tolerances."""
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
from test_gpu_mosaic import mixed_scene
from test_gpu_overlay import Counter, I, K, model, small_model  # noqa: F401  (fixtures, and the two-layer model)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 66, 130      # 2 x 3 tiles; the last row of tiles is 2 pixels high, the last column 2 wide


def compare(I, monkeypatch, layouts, h, w, sc, radius, paint=None, fallbacks=0, device="cuda"):
    """``I.blur`` on the GPU surface against the reference on its CPU twin; the bytes changed."""
    ref = Counter(monkeypatch, I, "blur_reference")
    changed = 0
    for layout in layouts:
        gpu, cpu = C.surface(layout, h, w, device=device), C.surface(layout, h, w, device="cpu")
        before = cpu.storage.clone()
        select = torch.tensor(sc.modes, dtype=torch.uint8)
        kw = dict(min_hits=sc.min_hits, radius=radius)
        (paint or I.blur)(gpu.target, *sc.tensors(device), select=select.to(device), **kw)
        n = ref.n
        I.blur_reference(cpu.target, *sc.tensors("cpu"), select=select, **kw)
        ref.n = n       # (the twin's own call)
        assert torch.equal(gpu.storage.cpu(), cpu.storage), f"{layout} {h}x{w} radius {radius} {sc.name}"
        changed += int((cpu.storage != before).sum())
    assert ref.n == fallbacks
    return changed


@pytest.mark.parametrize("radius", (1, 5, 32))
@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_blur_every_layout(K, I, monkeypatch, layout, radius):
    assert compare(I, monkeypatch, (layout,), H, W, mixed_scene(), radius) > 0


@pytest.mark.parametrize("radius", (2, 32))
@pytest.mark.parametrize("size", ((64, 64), (2, 2), (65, 67)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_sizes(K, I, monkeypatch, size, radius):
    h, w = size
    layouts = tuple(C.PACKED) if h % 2 else ("rgb", "crop", "nv12", "i422", "p010", "uyvy")
    assert compare(I, monkeypatch, layouts, h, w, C.edge_scene(h, w), radius) > 0


@pytest.mark.parametrize("radius", (3, 32))
@pytest.mark.parametrize("N", (1, 257, 1024))
def test_blur_rows(K, I, monkeypatch, N, radius):
    """From 257 rows on every tile is painted and every halo lies in painted neighbours: reading the frame fails here."""
    assert compare(I, monkeypatch, ("bgr", "nv12", "yvyu"), H, W, C.lattice_scene(N, H, W), radius) > 0


@pytest.mark.parametrize("count", (0, -3, 70))
def test_blur_count_is_clamped(K, I, monkeypatch, count):
    sc = C.lattice_scene(65, H, W, seed=3, total=90, count=count)
    assert (compare(I, monkeypatch, ("rgba", "nv21"), H, W, sc, 4) == 0) == (count <= 0)


def test_blur_track_ids_and_min_hits(K, I, monkeypatch):
    sc = C.lattice_scene(100, H, W)             # ids, hits 1..4, min_hits 2
    held = compare(I, monkeypatch, ("nv12",), H, W, sc, 4)
    assert 0 < held < compare(I, monkeypatch, ("nv12",), H, W, dataclasses.replace(sc, min_hits=1), 4)


def test_blur_entries_refuse_before_any_launch(K, I):
    sc = mixed_scene()
    count, scores, labels, boxes, _, _ = sc.tensors("cuda")
    select = torch.tensor(sc.modes, dtype=torch.uint8).cuda()
    taps = I._blur_table(8, select.device)
    for layout in ("bgra", "nv12"):
        surf = C.surface(layout, H, W, device="cuda")
        before = surf.storage.clone()
        s = I.overlay_surface(surf.target)
        src = None if s.packed is not None else I.yuv_src(*s.yuv, (0,) * 12)
        if src is None:
            data, order = s.packed
            need = I._L().nos_blur_shadow_packed(data.stride(1), order.encode(), s.h, s.w)
        else:
            need = I._L().nos_blur_shadow_yuv(ctypes.byref(src), s.h, s.w)
        shadow = torch.empty(need, dtype=torch.uint8, device="cuda")

        def call(sel, radius, sh, size):
            tail = [count.data_ptr(), scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(), None, None, sc.N, sel,
                    len(sc.modes), 1, radius, taps.data_ptr(), sh, size, None]
            if src is None:
                return I._L().nos_blur_packed(data.data_ptr(), *I._storage_bounds(data), data.stride(1), order.encode(),
                                              s.h, s.w, *tail)
            return I._L().nos_blur_yuv(ctypes.byref(src), s.h, s.w, *tail)
        ok = (select.data_ptr(), 8, shadow.data_ptr(), need)
        for bad in ((ok[0], 0) + ok[2:], (ok[0], 33) + ok[2:], (None,) + ok[1:], ok[:2] + (None, need), ok[:3] + (need - 1,)):
            assert call(*bad) == -1 and I._L().nos_image_last_error()
        torch.cuda.synchronize()
        assert torch.equal(surf.storage, before)
        assert call(*ok) == 0
        torch.cuda.synchronize()
        assert not torch.equal(surf.storage, before)


def test_blur_other_inputs_take_the_reference(K, I, monkeypatch):
    sc = mixed_scene()

    def double(target, count, scores, labels, boxes, ids, hits, **kw):
        return I.blur(target, count, scores.double(), labels, boxes.double(), ids, hits, **kw)
    compare(I, monkeypatch, ("nv12",), H, W, sc, 8, double, 1)
    compare(I, monkeypatch, ("bgr",), H, W, C.lattice_scene(1025, H, W), 8, None, 1)
    compare(I, monkeypatch, ("p010",), H, W, sc, 8, None, 1, device="cpu")
    K.set_backend("torch")
    try:
        compare(I, monkeypatch, ("uyvy",), H, W, sc, 8, None, 1)
    finally:
        K.set_backend("hip")


def test_annotate_blurs_in_the_captured_graph(K, I, monkeypatch, model):
    """One graph replayed on two frames: the target equals the three references, in ``draw``'s order, on a CPU copy with
    the returned lists; the shadow and the tap table survive capture and replay."""
    from walkai_nos_amd.models.workload.overlay import Overlay
    refs = [Counter(monkeypatch, I, name) for name in ("mosaic_reference", "blur_reference", "overlay_reference")]
    h, w = 96, 130
    src, dst = C.surface("nv12", h, w, seed=20, device="cuda"), C.surface("nv12", h, w, seed=21, device="cuda")
    twin = C.surface("nv12", h, w, seed=21, device="cpu")
    overlay = Overlay(thickness=2, scale=1, blur=[k for k in range(91) if k % 7 in (2, 3, 5)], blur_radius=5,
                      pixelate=[k for k in range(91) if k % 7 in (1, 4, 6)], modes={k: 1 for k in range(1, 45)}, num_labels=91)
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
    pixelated, blurred = (torch.tensor([int(k in chosen) for k in range(91)], dtype=torch.uint8)
                          for chosen in (overlay.pixelate, overlay.blur))
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
        I.mosaic_reference(twin.target, *lists, select=pixelated, cell=4)
        before = twin.storage.clone()
        I.blur_reference(twin.target, *lists, select=blurred, radius=5)
        total += int((twin.storage != before).sum())
        I.overlay_reference(twin.target, *lists, **kw)
        assert [r.n - c for r, c in zip(refs, calls)] == [1, 1, 1]   # the twin's own three calls, none from the GPU side
        assert torch.equal(dst.storage.cpu(), twin.storage)
        print(f"[blur] annotate_image nv12 {h}x{w}: {int(lists[0])} rows of labels {sorted(set(lists[2][:int(lists[0])].tolist()))}, "
              f"{total} bytes blurred so far")
    assert total > 0
    del graph


def test_pod_client_blurs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "walkai_nos_amd.dataplane.client", "--end-to-end",
           "--seconds", "1", "--image-hw", "96,128", "--size", "80,133", "--threshold", "0.0", "--annotate",
           "--pixel-format", "nv12", "--blur", "1,2,3"]
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert p.stdout.readline().strip() == "READY"
        rest, _ = p.communicate(f"GO {time.time()}\n", timeout=120)
    finally:
        p.kill()
    out = json.loads(rest.strip().splitlines()[-1])
    assert p.returncode == 0 and out["end_to_end"] and out["inferences"] > 0 and out["annotate"]["changed_bytes"] > 0
