"""The overlay kernel (``overlay_k``, ``csrc/image_overlay.h``) on the GPU against the per-pixel loop of
``tests/overlay_case.py``: every comparison is equality of the whole allocation the surface lies in — seeded random bytes
first, so pitch padding, the bytes around the planes, the alpha byte and the parent of a crop must come back untouched —
and asserts that the torch reference was not called, so a silent fall-back cannot pass. There are no tolerances.

What each group pins:

* every layout (contiguous RGB, ``Packed`` bgr / rgba / bgra and a crop at odd origins, NV12 / NV21, I420 / YV12, planar
  4:2:2, 4:4:4 and 10-bit low-bit 4:2:0, P010, NV16, NV24, YUY2 / UYVY / YVYU) on every scene of ``overlay_case.scenes``:
  boxes outside, across and around the frame, degenerate and non-finite coordinates, thickness, tags, priority, the
  filters, boxes at odd origins where the chroma rule decides;
* frames around the raster tile (32 x 64): the tile, two more each way, two tiles and two more, 2 x 2, and odd sizes for
  packed pixels; ``N`` at 1, 64, 65, 100 and 1024; ``count`` at 0, 1, ``N``, above ``N`` and negative over views of larger
  allocations full of drawable rows;
* two launches give the same bytes; the entries' refusals launch nothing; fp64 lists, 1025 rows, the ``torch`` backend
  and a CPU frame take the reference and still equal the loop;
* one captured launch replayed over ten frames, the frame refilled and the lists rewritten between replays;
* ``annotate_image`` and ``annotate_tiled``, with and without a tracker, captured on a model with distinguishable
  parameters, and the pod client with ``--annotate``.

One ``[overlay]`` line per comparison; the run on the MI355X is kept in ``profiles/pytest_gpu_overlay.log``."""
import ctypes
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import overlay_case as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = C.SIZES[1]
_slots = {}


def slot_of(sc, h, w):
    key = (sc.name, h, w)
    if key not in _slots:
        _slots[key] = C.slots(sc, h, w)
    return _slots[key]


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


class Counter:
    def __init__(self, monkeypatch, owner, name):
        self.n = 0
        fn = getattr(owner, name)

        def spy(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        monkeypatch.setattr(owner, name, spy)


def compare(I, monkeypatch, layouts, h, w, scenes):
    """The kernel on every layout and scene against the loop; the bytes painted."""
    ref = Counter(monkeypatch, I, "overlay_reference")
    changed = 0
    for layout in layouts:
        for k, sc in enumerate(scenes):
            changed += C.run(I, I.overlay, C.surface(layout, h, w, seed=k, device="cuda"), sc, slot_of(sc, h, w))
    assert ref.n == 0
    print(f"[overlay] {', '.join(layouts)} {h}x{w}: {len(scenes)} scenes ({', '.join(s.name for s in scenes[:4])}"
          f"{' ...' if len(scenes) > 4 else ''}), {changed} bytes painted, every other byte of the allocations as it was")
    return changed


# ---- layouts, sizes, rows ---------------------------------------------------------------------------------------------------
def test_overlay_tile_is_the_one_the_sizes_lie_around(K, I):
    assert (I._L().nos_overlay_tile_rows(), I._L().nos_overlay_tile_columns()) == C.TILE == I.OVERLAY_TILE


@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_overlay_every_layout(K, I, monkeypatch, layout):
    assert compare(I, monkeypatch, (layout,), H, W, C.scenes(H, W)) > 0


@pytest.mark.parametrize("size", (C.SIZES[0], C.SIZES[2], C.SIZES[3]), ids=lambda s: f"{s[0]}x{s[1]}")
def test_overlay_sizes_around_the_tile(K, I, monkeypatch, size):
    h, w = size
    scenes = [C.edge_scene(h, w), C.edge_scene(h, w, 2), C.degenerate_scene(h, w), C.odd_scene(h, w),
              C.priority_scene(h, w)] + C.tag_scenes(h, w)
    compare(I, monkeypatch, ("rgb", "crop", "nv12", "i420", "i422", "p010", "nv24", "uyvy"), h, w, scenes)


def test_overlay_odd_sizes_of_packed_pixels(K, I, monkeypatch):
    h, w = C.ODD_SIZE
    scenes = [C.edge_scene(h, w), C.priority_scene(h, w), C.odd_scene(h, w)] + C.tag_scenes(h, w)
    assert compare(I, monkeypatch, tuple(C.PACKED), h, w, scenes) > 0


@pytest.mark.parametrize("N", C.ROWS)
def test_overlay_rows(K, I, monkeypatch, N):
    h, w = C.SIZES[2]
    assert compare(I, monkeypatch, ("bgr", "nv12", "yvyu"), h, w, [C.lattice_scene(N, h, w)]) > 0


def test_overlay_count_is_clamped(K, I, monkeypatch):
    for sc in C.count_scenes(H, W):
        changed = compare(I, monkeypatch, ("rgba", "nv21"), H, W, [sc])
        assert (changed == 0) == (sc.count <= 0), sc.name


def test_overlay_two_launches_are_byte_equal(K, I, monkeypatch):
    ref = Counter(monkeypatch, I, "overlay_reference")
    h, w = C.SIZES[2]
    sc = C.lattice_scene(1024, h, w)
    for layout in ("bgra", "i010", "yuy2"):
        a, b = (C.surface(layout, h, w, device="cuda") for _ in range(2))
        assert torch.equal(a.storage, b.storage)
        for surf in (a, b):
            C.run(I, I.overlay, surf, sc, slot_of(sc, h, w))
        assert torch.equal(a.storage, b.storage)
    assert ref.n == 0


# ---- the entries' refusals ---------------------------------------------------------------------------------------------------
def raw_args(I, surf, sc):
    """``(entry, arguments, kept alive)`` of the raw call that paints ``sc`` into ``surf``."""
    dev = "cuda"
    count, scores, labels, boxes, ids, hits = sc.tensors(dev)
    modes = torch.tensor(sc.modes, dtype=torch.uint8).to(dev)
    codes = I.overlay_codes(I.overlay_palette(sc.K), (9, 200, 31), surf.target)
    font = I._overlay_font(torch.device(dev, 0))
    s = I.overlay_surface(surf.target)
    tail = [count.data_ptr(), scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(), None, None, sc.N, modes.data_ptr(),
            len(sc.modes), codes.data_ptr(), sc.K, font.data_ptr(), sc.t, sc.s, sc.min_hits, None]
    keep = [count, scores, labels, boxes, modes, codes, font, s]
    if s.packed is not None:
        data, order = s.packed
        lo, hi = I._storage_bounds(data)
        return I._L().nos_overlay_packed, [data.data_ptr(), lo, hi, data.stride(1), order.encode(), s.h, s.w] + tail, keep
    src = I.yuv_src(*s.yuv, (0,) * 12)
    return I._L().nos_overlay_yuv, [ctypes.byref(src), s.h, s.w] + tail, keep + [src]


def test_overlay_entries_refuse_before_any_launch(K, I):
    sc = C.priority_scene(H, W)
    L = I._L()
    for layout, first in (("bgra", 7), ("nv12", 3)):
        surf = C.surface(layout, H, W, device="cuda")
        before = surf.storage.clone()
        entry, good, keep = raw_args(I, surf, sc)
        # tail positions from `first`: count scores labels boxes id hits N modes L codes K font t s min_hits stream
        bad = [{first + i: None} for i in (0, 1, 2, 3, 7, 9, 11)]
        bad += [{first + 4: good[first]}, {first + 5: good[first]}]              # ids without hits, hits without ids
        bad += [{first + 6: v} for v in (0, -1, 1025)] + [{first + 8: 0}, {first + 10: 0}, {first + 10: 1025}]
        bad += [{first + 12: v} for v in (0, -1, (1 << 20) + 1)] + [{first + 13: v} for v in (-1, 1025)]
        bad += [{first + 14: 0}]
        bad += [{first - 2: 0}, {first - 1: 0}, {first - 2: 32769}, {first - 2: H + 1}, {first - 1: W + 40}]
        if layout == "bgra":
            bad += [{0: None}, {4: None}, {4: b"argb"}, {3: 4 * W - 1}, {2: good[2] - surf.storage.numel() + 60},
                    {1: good[0] + 1}]
        for change in bad:
            a = list(good)
            for k, v in change.items():
                a[k] = v
            assert entry(*a) == -1 and L.nos_image_last_error(), change
        if layout == "nv12":
            s = I.overlay_surface(surf.target)
            for field, value in (("size", 8), ("layout", 3), ("hsub", 2), ("sample_bytes", 2), ("order", 2)):
                src = I.yuv_src(*s.yuv, (0,) * 12)
                setattr(src, field, value)
                assert entry(ctypes.byref(src), *good[1:]) == -1, field
            for plane, field, value in ((0, "pitch", W - 1), (1, "p", None), (1, "hi", "short"), (0, "lo", "late")):
                src = I.yuv_src(*s.yuv, (0,) * 12)
                if value == "short":
                    value = src.plane[plane].hi - TAIL_AND_MORE
                elif value == "late":
                    value = src.plane[plane].p + 1
                setattr(src.plane[plane], field, value)
                assert entry(ctypes.byref(src), *good[1:]) == -1, (plane, field)
            assert entry(None, *good[1:]) == -1
        torch.cuda.synchronize()
        assert torch.equal(surf.storage, before)
        assert entry(*good) == 0
        torch.cuda.synchronize()
        assert not torch.equal(surf.storage, before)
    print("[overlay] both entries refuse null operands, sizes, limits and surfaces outside their storage; nothing is "
          "launched, the allocation is as it was")


TAIL_AND_MORE = C.TAIL + C.PAD + 1      # cuts the last chroma row's last sample out of [lo, hi)


def test_overlay_other_inputs_take_the_reference(K, I, monkeypatch):
    ref = Counter(monkeypatch, I, "overlay_reference")
    sc = C.priority_scene(H, W)
    slot = slot_of(sc, H, W)

    def paint(double=False):
        def f(target, count, scores, labels, boxes, ids, hits, **kw):
            if double:
                scores, boxes = scores.double(), boxes.double()
            return I.overlay(target, count, scores, labels, boxes, ids, hits, **kw)
        return f
    C.run(I, paint(), C.surface("nv12", H, W, device="cuda"), sc, slot)
    assert ref.n == 0
    C.run(I, paint(True), C.surface("nv12", H, W, device="cuda"), sc, slot)
    assert ref.n == 1
    many = C.lattice_scene(1025, H, W)
    C.run(I, I.overlay, C.surface("bgr", H, W, device="cuda"), many)
    assert ref.n == 2
    C.run(I, I.overlay, C.surface("p010", H, W, device="cpu"), sc, slot)
    assert ref.n == 3
    K.set_backend("torch")
    try:
        C.run(I, I.overlay, C.surface("uyvy", H, W, device="cuda"), sc, slot)
    finally:
        K.set_backend("hip")
    assert ref.n == 4


# ---- one captured launch, replayed ------------------------------------------------------------------------------------
def test_overlay_graph_replay_paints_each_frame(K, I, monkeypatch):
    ref = Counter(monkeypatch, I, "overlay_reference")
    h, w = C.SIZES[2]
    surf = C.surface("nv12", h, w, device="cuda")
    frames = [C.lattice_scene(100, h, w, seed=k, count=(100, 37, 0, 100, 1)[k % 5]) for k in range(10)]
    static = frames[0].tensors("cuda")
    modes = torch.tensor(frames[0].modes, dtype=torch.uint8).cuda()
    codes = I.overlay_codes(I.overlay_palette(16), (9, 200, 31), surf.target)
    kw = dict(thickness=1, scale=1, modes=modes, min_hits=2, codes=codes)
    I.overlay(surf.target, *static, **kw)       # eagerly first: the tables are made outside the capture
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        I.overlay(surf.target, *static, **kw)
    g = torch.Generator().manual_seed(4)
    changed = 0
    for sc in frames:
        surf.storage.copy_(torch.randint(0, 256, surf.storage.shape, generator=g, dtype=torch.uint8))
        for dst, src in zip(static, sc.tensors()):
            dst.copy_(src)
        before = bytes(surf.storage.cpu().numpy().tobytes())
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        changed += C.check(surf, before, C.slots(sc, h, w), codes.cpu().tolist())
    assert ref.n == 0 and changed > 0
    print(f"[overlay] one graph replayed over {len(frames)} frames of nv12 {h}x{w}, frame and lists rewritten between "
          f"replays: every replay equal to the loop, {changed} bytes painted")
    del graph


# ---- end to end -------------------------------------------------------------------------------------------------------
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


def scene_of(det, overlay, h, w):
    """The returned lists as the loop's scene."""
    flat = {k: det[k].detach().cpu() for k in ("count", "scores", "labels", "boxes", "track_id", "track_hits") if k in det}
    t, s = overlay.sizes(h, w)
    return C.Scene("returned", flat["scores"].flatten().tolist(), flat["labels"].flatten().tolist(),
                   flat["boxes"].reshape(-1, 4).tolist(),
                   ids=flat["track_id"].flatten().tolist() if "track_id" in flat else None,
                   hits=flat["track_hits"].flatten().tolist() if "track_id" in flat else None,
                   count=int(flat["count"].item()), t=t, s=s, modes=list(overlay.modes), min_hits=overlay.min_hits,
                   K=overlay.palette.shape[0])


@pytest.mark.parametrize("tiled", (False, True), ids=("annotate_image", "annotate_tiled"))
@pytest.mark.parametrize("tracked", (False, True), ids=("labels", "ids"))
def test_annotate_captured_on_the_model(K, I, monkeypatch, model, tiled, tracked):
    """``annotate_image`` / ``annotate_tiled`` as one graph, replayed on three different frames: after every replay the
    target equals the loop applied to the lists that replay returned, and the source frame is as it was put there.
    Without a tracker and untiled, ``target=None``: the frame itself is painted."""
    from walkai_nos_amd.models.workload.overlay import Overlay
    from walkai_nos_amd.models.workload.tracker import Tracker
    ref = Counter(monkeypatch, I, "overlay_reference")
    h, w = 96, 130
    in_place = not tiled and not tracked
    src = C.surface("nv12", h, w, seed=20, device="cuda")
    dst = src if in_place else C.surface("nv12", h, w, seed=21, device="cuda")
    tracker = Tracker(capacity=128, device="cuda") if tracked else None
    overlay = Overlay(thickness=2, scale=1, redact=range(0, 91, 3), modes={4: 0, 5: 0}, redact_colour=(9, 200, 31),
                      min_hits=2 if tracked else 1, num_labels=91)

    def annotate(thr):
        target = None if in_place else dst.target
        if tiled:
            return model.annotate_tiled(src.target, overlay, (2, 2), 0.3, thr, tracker=tracker, target=target)
        return model.annotate_image(src.target, overlay, thr, tracker, target)
    clean = src.storage.clone()
    with torch.no_grad():
        s = (model.detect_tiled(src.target, (2, 2), 0.3, 0.0) if tiled else model.detect_image(src.target, 0.0))["scores"]
        thr = s.flatten().sort().values[-40].item() - 1e-6
        annotate(thr)                               # a warm-up: the tables are made outside the capture
    if tracker is not None:
        tracker.reset()
    src.storage.copy_(clean)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=stream):
        held = annotate(thr)
    assert held["frame"] is (src.target if in_place else dst.target)
    if tracker is not None:
        tracker.reset()
    codes = I.overlay_codes(overlay.palette, overlay.redact_colour, dst.target).cpu().tolist()
    g = torch.Generator().manual_seed(8)
    painted, rows = 0, []
    for k in range(3):
        fresh = torch.randint(0, 256, src.storage.shape, generator=g, dtype=torch.uint8).cuda()
        if tracked and k == 1:
            fresh = put                             # the same frame again: its tracks reach min_hits
        put = fresh
        src.storage.copy_(fresh)
        before = bytes(dst.storage.cpu().numpy().tobytes())
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        sc = scene_of(held, overlay, h, w)
        painted += (n := C.check(dst, before, C.slots(sc, h, w), codes))
        rows.append((sc.count, n))
        if not in_place:
            assert torch.equal(src.storage, fresh)
    assert ref.n == 0 and painted > 0
    if tracked:
        assert rows[0][1] == 0 and rows[1][1] > 0       # hits 1 on the first frame: below min_hits, nothing drawn
    print(f"[overlay] {'annotate_tiled (2, 2)' if tiled else 'annotate_image'} nv12 {h}x{w}, "
          f"{'ids' if tracked else 'labels'}, {'in place' if in_place else 'into a second surface'}, one graph, three "
          f"replays: (rows, bytes painted) {rows}; the target equals the loop on the returned lists every time")
    del graph


# ---- the pod client (last: it starts a process) --------------------------------------------------------------------------
def test_pod_client_annotates():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "walkai_nos_amd.dataplane.client", "--end-to-end",
           "--seconds", "1", "--image-hw", "96,128", "--size", "80,133", "--threshold", "0.0", "--annotate", "--track",
           "--tiles", "2,2", "--pixel-format", "nv12", "--redact", "1,2,3"]
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert p.stdout.readline().strip() == "READY"
        p.stdin.write(f"GO {time.time()}\n")
        p.stdin.flush()
        lines = [ln for ln in p.stdout.read().splitlines() if ln.strip()]
        assert p.wait(timeout=60) == 0
    finally:
        if p.poll() is None:
            p.kill()
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["end_to_end"] and out["tiles"] == 4 and out["inferences"] > 0 and "track" in out
    assert out["annotate"]["changed_bytes"] > 0
    print(f"[overlay] client --annotate --track --tiles 2,2 nv12 96x128: {out['inferences']} inferences, "
          f"{out['detections']} detections, {out['annotate']['changed_bytes']} bytes of the second surface changed")
