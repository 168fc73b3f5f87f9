"""``chips_k`` (``csrc/image_chips.h``) on the GPU against ``ops.image.chips_reference`` on the CPU twin of the same
surface (the same seeded bytes; ``test_chips.py`` holds the reference to a loop): equality of all four outputs after a
second call on buffers filled with 0xFF, the reference never called on the GPU side. There are no tolerances."""
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
H, W = 66, 130
SIZES = ((1, 1), (8, 12), (33, 17))     # one that shrinks, one that enlarges, one that does both by axis


def compare(I, monkeypatch, layouts, h, w, sc, size, capacity=16, margin=0, cut=None, fallbacks=0, device="cuda", **frame):
    """``I.chips`` of the GPU surface against the reference on its CPU twin; the chips of the last layout."""
    ref = Counter(monkeypatch, I, "chips_reference")
    for layout in layouts:
        gpu, cpu = (dataclasses.replace(C.surface(layout, h, w, device=d).target, **frame) if frame
                    else C.surface(layout, h, w, device=d).target for d in (device, "cpu"))
        select = torch.tensor(sc.modes, dtype=torch.uint8)
        kw = dict(size=size, capacity=capacity, margin=margin, min_hits=sc.min_hits)
        if not fallbacks:
            for t in I.chips(gpu, *sc.tensors(device), select=select.to(device), **kw):
                t.fill_(0xFF)       # the cached buffers: the second call writes every byte of them
        got = (cut or I.chips)(gpu, *sc.tensors(device), select=select.to(device), **kw)
        n = ref.n
        want = I.chips_reference(cpu, *sc.tensors("cpu"), select=select, **kw)
        ref.n = n       # (the twin's own call)
        for name, g, wnt in zip(("chips", "rows", "rects", "chip_count"), got, want):
            assert torch.equal(g.cpu(), wnt), f"{name}: {layout} {h}x{w} {size} {sc.name}"
    assert ref.n == fallbacks
    return int(want[3])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_chips_every_layout(K, I, monkeypatch, layout, size):
    assert compare(I, monkeypatch, (layout,), H, W, mixed_scene(), size) > 0


def box_scene(h, w):
    """A 1 x 1 box, the whole frame, ``X0`` at every residue mod 4 with odd and even ``Y0``, a box of 21 source rows
    (three chunks of 8, and two bands of a 12 x 256 chip), then ``edge_scene``'s boxes across and outside every edge."""
    boxes = [[9, 7, 10, 8], [0, 0, w, h]] + [[20 + r, 3 + r, 31 + 2 * r, 12 + r] for r in range(4)] \
        + [[41, 11, 97, 32]] + C.edge_scene(h, w).boxes
    return C.Scene("boxes", [0.9] * len(boxes), [k % 2 for k in range(len(boxes))], boxes)


@pytest.mark.parametrize("margin", (0, 5))
@pytest.mark.parametrize("size", ((5, 3), (12, 256)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_chips_boxes_where_the_kernel_can_go_wrong(K, I, monkeypatch, size, margin):
    layouts = ("rgb", "crop", "nv12", "i420", "i010", "uyvy")
    assert compare(I, monkeypatch, layouts, H, W, box_scene(H, W), size, 32, margin) >= 16


@pytest.mark.parametrize("size", ((1, 7), (2, 256)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_chips_wider_than_a_column_chunk(K, I, monkeypatch, size):
    h, w = 2, 1100
    assert I._L().nos_chips_column_chunk() == 256 < w and I._L().nos_chips_row_chunk() == 8
    sc = C.Scene("wide", [0.9] * 3, [0, 1, 0], [[0, 0, w, h], [3, 0, 1030.5, 1], [254, 1, 771, 2]])
    assert compare(I, monkeypatch, ("bgr", "nv12", "yuy2"), h, w, sc, size) == 3


@pytest.mark.parametrize("capacity", (1, 64, 256))
@pytest.mark.parametrize("N", (1, 257, 1024))
def test_chips_rows_and_capacity(K, I, monkeypatch, N, capacity):
    sc = C.lattice_scene(N, H, W)       # ids, hits 1..4, min_hits 2
    n = compare(I, monkeypatch, ("nv12",), H, W, sc, (8, 12), capacity)
    assert n == 1 if min(N, capacity) == 1 else 1 < n <= capacity       # (row 0 is selected: hits 2, label 0)


@pytest.mark.parametrize("count", (0, -3, 70))
def test_chips_count_is_clamped(K, I, monkeypatch, count):
    sc = C.lattice_scene(65, H, W, seed=3, total=90, count=count)
    assert (compare(I, monkeypatch, ("rgba", "nv21"), H, W, sc, (8, 12), 128) == 0) == (count <= 0)


def test_chips_track_ids_and_min_hits(K, I, monkeypatch):
    sc = C.lattice_scene(100, H, W)
    held = compare(I, monkeypatch, ("i422",), H, W, sc, (4, 4), 128)
    assert 0 < held < compare(I, monkeypatch, ("i422",), H, W, dataclasses.replace(sc, min_hits=1), (4, 4), 128)


@pytest.mark.parametrize("kind", [("nv12", dict(chroma="bilinear", siting="left")),
                                  ("i420", dict(chroma="bilinear", siting="center")),
                                  ("uyvy", dict(chroma="bilinear", siting="topleft")),
                                  ("p010", dict(chroma="bilinear", siting="top")),
                                  ("p010", dict(transfer="pq", matrix="bt2020")),
                                  ("p010", dict(transfer="hlg", matrix="bt2020", chroma="bilinear"))],
                         ids=lambda k: "-".join([k[0]] + [str(v) for v in k[1].values()]))
def test_chips_other_source_kinds(K, I, monkeypatch, kind):
    assert compare(I, monkeypatch, (kind[0],), H, W, box_scene(H, W), (8, 12), 32, 1, **kind[1]) > 16


def test_chips_entries_refuse_before_any_launch(K, I):
    sc = mixed_scene()
    count, scores, labels, boxes, _, _ = sc.tensors("cuda")
    select = torch.tensor(sc.modes, dtype=torch.uint8).cuda()
    out = [torch.full(s, 0x5A, dtype=d, device="cuda") for s, d in
           (((4, 8, 12, 3), torch.uint8), ((4,), torch.int32), ((4, 4), torch.int32), ((1,), torch.int32))]
    before = [t.clone() for t in out]
    for layout in ("bgra", "nv12"):
        surf = C.surface(layout, H, W, device="cuda")      # (held: the descriptor points into it)
        h, w, packed, yuv = (I._chip_source(surf.target)[k] for k in (1, 2, 4, 5))

        def call(N=sc.N, sel=select.data_ptr(), margin=0, capacity=4, sh=8, sw=12, chips=out[0].data_ptr(), h=h, size=None):
            tail = [count.data_ptr(), scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(), None, None, N, sel,
                    len(sc.modes), 1, margin, capacity, sh, sw, chips] + [t.data_ptr() for t in out[1:]] + [None]
            if packed is not None:
                data, order = packed
                return I._L().nos_chips_packed(data.data_ptr(), *I._storage_bounds(data), data.stride(1), order.encode(),
                                               h, w, *tail)
            src = yuv[0]
            src.size = ctypes.sizeof(src) if size is None else size
            return I._L().nos_chips_yuv(ctypes.byref(src), None, h, w, *tail)
        bad = [dict(N=0), dict(N=1025), dict(sel=None), dict(chips=None), dict(margin=-1), dict(margin=65),
               dict(capacity=0), dict(capacity=257), dict(sh=0), dict(sw=257), dict(h=h + 1), dict(h=1 << 16)]
        for kw in bad + ([] if packed is not None else [dict(size=8)]):
            assert call(**kw) == -1 and I._L().nos_image_last_error(), kw
        torch.cuda.synchronize()
        assert all(torch.equal(t, b) for t, b in zip(out, before))
        assert call() == 0
        torch.cuda.synchronize()
        assert out[3].item() == 4 and out[1].tolist() == [0, 1, 2, 3] and not torch.equal(out[0], before[0])
        for t, b in zip(out, before):
            t.copy_(b)
    # a frame of more than 2^24 pixels is refused by the entry (the wrapper then takes the reference)
    big = torch.zeros((4097, 4096, 3), dtype=torch.uint8, device="cuda")
    tail = [count.data_ptr(), scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(), None, None, sc.N,
            select.data_ptr(), len(sc.modes), 1, 0, 4, 8, 12] + [t.data_ptr() for t in out] + [None]
    assert I._L().nos_chips_packed(big.data_ptr(), *I._storage_bounds(big), 4096 * 3, b"rgb", 4097, 4096, *tail) == -1
    assert b"2^24" in I._L().nos_image_last_error()


def test_chips_other_inputs_take_the_reference(K, I, monkeypatch):
    sc = mixed_scene()

    def double(frame, count, scores, labels, boxes, ids, hits, **kw):
        return I.chips(frame, count, scores.double(), labels, boxes.double(), ids, hits, **kw)
    compare(I, monkeypatch, ("nv12",), H, W, sc, (8, 12), cut=double, fallbacks=1)
    compare(I, monkeypatch, ("bgr",), H, W, C.lattice_scene(1025, H, W), (8, 12), fallbacks=1)
    compare(I, monkeypatch, ("p010",), H, W, sc, (8, 12), fallbacks=1, device="cpu")
    compare(I, monkeypatch, ("rgb",), H, W, sc, (257, 2), fallbacks=1)
    compare(I, monkeypatch, ("rgb",), H, W, sc, (2, 2), 257, fallbacks=1)
    K.set_backend("torch")
    try:
        compare(I, monkeypatch, ("uyvy",), H, W, sc, (8, 12), fallbacks=1)
    finally:
        K.set_backend("hip")


def test_chip_image_in_a_captured_graph(K, I, monkeypatch, model):
    """``chip_image`` with a tracker, captured once and replayed on two frames: the chips equal the reference on a CPU
    copy of the frame with the returned lists, and the cached output buffers are the ones the graph writes."""
    from walkai_nos_amd.models.workload.chips import Chips
    from walkai_nos_amd.models.workload.tracker import Tracker
    ref = Counter(monkeypatch, I, "chips_reference")
    h, w = 96, 130
    src, twin = C.surface("nv12", h, w, seed=20, device="cuda"), C.surface("nv12", h, w, seed=20, device="cpu")
    chips = Chips(size=(16, 8), labels=range(0, 91, 3), capacity=24, margin=2)
    tracker = Tracker(64, device="cuda")
    with torch.no_grad():
        thr = model.detect_image(src.target, 0.0)["scores"].flatten().sort().values[-40].item() - 1e-6
        model.chip_image(src.target, chips, thr, tracker)       # a warm-up: the tables are made outside the capture
    tracker.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        held = model.chip_image(src.target, chips, thr, tracker)
    tracker.reset()
    key = (str(src.storage.device), 24, 16, 8)
    assert I._chip_buffers.pinned(key) and I._chip_buffers.get(key, lambda: None)[0] is held["chips"]
    g = torch.Generator().manual_seed(8)
    total = 0
    for fresh in (twin.storage.clone(), torch.randint(0, 256, twin.storage.shape, generator=g, dtype=torch.uint8)):
        twin.storage.copy_(fresh)
        src.storage.copy_(fresh)
        held["chips"].fill_(0xFF)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        lists = [held[k].detach().cpu().reshape(shape) for k, shape in
                 (("count", (1,)), ("scores", (-1,)), ("labels", (-1,)), ("boxes", (-1, 4)), ("track_id", (-1,)),
                  ("track_hits", (-1,)))]
        want = I.chips_reference(twin.target, *lists, size=(16, 8), select=torch.tensor(chips.labels, dtype=torch.uint8),
                                 capacity=24, margin=2)
        for name, wnt in zip(("chips", "chip_rows", "chip_rects", "chip_count"), want):
            assert torch.equal(held[name].cpu(), wnt), name
        total += int(want[3])
        print(f"[chips] chip_image nv12 {h}x{w}: {int(lists[0])} rows of labels {sorted(set(lists[2][:int(lists[0])].tolist()))}, "
              f"ids {lists[4][:4].tolist()}, {int(want[3])} chips")
    assert total > 0 and ref.n == 2         # the twin's own two calls, none from the GPU side
    assert I._chip_buffers.get(key, lambda: None)[0] is held["chips"]
    del graph


def test_pod_client_cuts_chips():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "walkai_nos_amd.dataplane.client", "--end-to-end",
           "--seconds", "1", "--image-hw", "96,128", "--size", "80,133", "--threshold", "0.0", "--chips", "all",
           "--pixel-format", "nv12"]
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert p.stdout.readline().strip() == "READY"
        rest, _ = p.communicate(f"GO {time.time()}\n", timeout=120)
    finally:
        p.kill()
    out = json.loads(rest.strip().splitlines()[-1])
    assert p.returncode == 0 and out["end_to_end"] and out["inferences"] > 0
    assert out["chips"]["count"] > 0 and out["chips"]["nonzero_bytes"] > 0
