"""``ops.image.overlay_reference`` — the torch composition that runs on the CPU, with the ``torch`` backend and past the
kernel's limits — against the per-pixel loop of ``tests/overlay_case.py`` on every scene and every layout, the whole
allocation compared byte for byte; the glyph table against the ASCII art and against bitmaps written out by hand; the
wrapper's and the pod client's refusals; ``Overlay``'s defaults; and the colour codes' round trip.

The round trip's bound (``test_codes_round_trip``). ``overlay_codes`` gives, per colour, the codes ``round(inv(M) rgb +
offsets)`` of ``yuv_real_matrix``'s ``M``, each within 1/2 of the real value (no palette colour is clipped: the codes of
an 8-bit RGB colour lie inside the range of either convention). Read back, channel ``c`` is ``sum_j M[c][j] code_j``, so
the rounding of the three codes moves it by at most ``sum_j |M[c][j]| / 2`` 8-bit levels: half the absolute row sum of
the YUV-to-RGB matrix scaled to 8-bit output. ``frame.rgb()`` does not use ``M`` but the integer table ``rint(M 2^(8 +
depth))`` and rounds its sum once: one more level covers both (the table's error is below ``3 * 2^depth * 2^-(9 +
depth)`` < 0.01 levels, the final rounding 1/2). The bound is ``0.5 * sum_j |M[c][j]| + 1``: at 8-bit limited range
BT.601 2.38 (R), 1.99 (G), 2.60 (B) — 2 to 3 levels — and about a quarter and a sixteenth of the first term at 10 and 12
bits. It is compared on the interior of a 16 x 16 block, two luma pixels from its border, so that bilinear chroma sees
the block's chroma only. It is not fitted to what the code gives."""
import numpy as np
import pytest
import torch

import overlay_case as C
from walkai_nos_amd.models.workload.overlay import Overlay
from walkai_nos_amd.ops import image as I

H, W = C.SIZES[1]
_slots = {}


def slot_of(sc, h, w):
    key = (sc.name, h, w)
    if key not in _slots:
        _slots[key] = C.slots(sc, h, w)
    return _slots[key]


@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_reference_is_the_loop_on_every_layout(layout):
    changed = 0
    for k, sc in enumerate(C.scenes(H, W)):
        changed += C.run(I, I.overlay_reference, C.surface(layout, H, W, seed=k), sc, slot_of(sc, H, W))
    print(f"[overlay] reference == loop on {layout} {H}x{W}: {len(C.scenes(H, W))} scenes, {changed} bytes painted, "
          f"every other byte of the allocation as it was")
    assert changed > 0


@pytest.mark.parametrize("layout", ("rgb", "bgra", "crop"))
def test_reference_on_odd_sizes(layout):
    h, w = C.ODD_SIZE
    for sc in (C.edge_scene(h, w), C.priority_scene(h, w), C.tag_scenes(h, w)[2]):
        assert C.run(I, I.overlay_reference, C.surface(layout, h, w), sc) > 0


@pytest.mark.parametrize("size", (C.SIZES[0], C.SIZES[2], C.SIZES[3]), ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_on_the_other_sizes(size):
    h, w = size
    for layout in ("rgb", "nv12", "yuy2", "p010"):
        for sc in (C.edge_scene(h, w), C.degenerate_scene(h, w), C.odd_scene(h, w), C.tag_scenes(h, w)[1]):
            C.run(I, I.overlay_reference, C.surface(layout, h, w), sc, slot_of(sc, h, w))


@pytest.mark.parametrize("N", C.ROWS)
def test_reference_row_counts(N):
    sc = C.lattice_scene(N, H, W)
    for layout in ("bgr", "nv12"):
        assert C.run(I, I.overlay_reference, C.surface(layout, H, W), sc, slot_of(sc, H, W)) > 0


def test_reference_count_is_clamped():
    for sc in C.count_scenes(H, W):
        changed = C.run(I, I.overlay_reference, C.surface("i420", H, W), sc)
        assert (changed == 0) == (sc.count <= 0), sc.name


def test_subsampled_odd_box_changes_luma_only_where_the_rule_says():
    # a one-pixel-wide line on an odd column: luma only
    sc = C.Scene("line", [0.9], [0], [[5.0, 2.0, 6.0, 12.0]])
    for layout in C.SUBSAMPLED:
        surf = C.surface(layout, H, W)
        before = surf.storage.clone()
        C.run(I, I.overlay_reference, surf, sc)
        diff = (surf.storage != before).nonzero().flatten().tolist()
        luma = surf.planes[0]
        # ten luma samples at most (a random byte may already hold the code), each inside the luma plane's column 5
        assert 0 < len(diff) <= 10 * luma.sb
        assert all(0 <= (i - luma.off) % luma.pitch - 5 * luma.step < luma.sb for i in diff)


# ---- the glyphs -----------------------------------------------------------------------------------------------------------
def test_font_is_the_ascii_art():
    assert len(I.OVERLAY_FONT) == 10
    for d, rows in enumerate(I.OVERLAY_FONT):
        assert tuple("".join("#" if (bits >> (4 - c)) & 1 else "." for c in range(5)) for bits in rows) == C.GLYPHS[d], d


ONE = (".......",
       "...#...",
       "..##...",
       "...#...",
       "...#...",
       "...#...",
       "...#...",
       "..###..",
       ".......")
EIGHT = (".......",
         "..###..",
         ".#...#.",
         ".#...#.",
         "..###..",
         ".#...#.",
         ".#...#.",
         "..###..",
         ".......")
THREE_O_FIVE = ("...................",
                ".#####..###..#####.",
                "....#..#...#.#.....",
                "...#...#..##.####..",
                "....#..#.#.#.....#.",
                ".....#.##..#.....#.",
                ".#...#.#...#.#...#.",
                "..###...###...###..",
                "...................")
ONE_2 = ("..............",
         "..............",
         "......##......",
         "......##......",
         "....####......",
         "....####......",
         "......##......",
         "......##......",
         "......##......",
         "......##......",
         "......##......",
         "......##......",
         "......##......",
         "......##......",
         "....######....",
         "....######....",
         "..............",
         "..............")
EIGHT_2 = ("..............",
           "..............",
           "....######....",
           "....######....",
           "..##......##..",
           "..##......##..",
           "..##......##..",
           "..##......##..",
           "....######....",
           "....######....",
           "..##......##..",
           "..##......##..",
           "..##......##..",
           "..##......##..",
           "....######....",
           "....######....",
           "..............",
           "..............")
THREE_O_FIVE_2 = ("......................................",
                  "......................................",
                  "..##########....######....##########..",
                  "..##########....######....##########..",
                  "........##....##......##..##..........",
                  "........##....##......##..##..........",
                  "......##......##....####..########....",
                  "......##......##....####..########....",
                  "........##....##..##..##..........##..",
                  "........##....##..##..##..........##..",
                  "..........##..####....##..........##..",
                  "..........##..####....##..........##..",
                  "..##......##..##......##..##......##..",
                  "..##......##..##......##..##......##..",
                  "....######......######......######....",
                  "....######......######......######....",
                  "......................................",
                  "......................................")


@pytest.mark.parametrize("key,s,bitmap", [(1, 1, ONE), (8, 1, EIGHT), (305, 1, THREE_O_FIVE), (1, 2, ONE_2),
                                          (8, 2, EIGHT_2), (305, 2, THREE_O_FIVE_2)],
                         ids=["1-s1", "8-s1", "305-s1", "1-s2", "8-s2", "305-s2"])
def test_digits_equal_bitmaps_written_out_by_hand(key, s, bitmap):
    th, tw = len(bitmap), len(bitmap[0])
    assert (th, tw) == (9 * s, (6 * len(str(key)) + 1) * s)
    frame = torch.zeros(th + 8, tw + 6, 3, dtype=torch.uint8)
    pal = np.array([[[10, 20, 30], [200, 210, 220]]], dtype=np.uint8)
    codes = I.overlay_codes(pal, (1, 1, 1), frame)
    lists = (torch.tensor([1], dtype=torch.int32), torch.tensor([0.9]), torch.tensor([0], dtype=torch.int32),
             torch.tensor([[0.0, th, tw + 4.0, th + 6.0]]), torch.tensor([key], dtype=torch.int32),
             torch.tensor([1], dtype=torch.int32))
    I.overlay_reference(frame, *lists, thickness=1, scale=s, modes=torch.tensor([1], dtype=torch.uint8), codes=codes)
    tag = frame[:th, :tw]
    got = tuple("".join("#" if tag[y, x].tolist() == [200, 210, 220] else "." for x in range(tw)) for y in range(th))
    assert got == tuple(bitmap)
    assert all(tag[y, x].tolist() in ([10, 20, 30], [200, 210, 220]) for y in range(th) for x in range(tw))
    assert not frame[:th, tw:].any()        # nothing beside the tag


# ---- colours ---------------------------------------------------------------------------------------------------------------
def test_palette():
    pal = I.overlay_palette()
    assert pal.shape == (16, 2, 3) and pal.dtype == np.uint8
    assert len({tuple(c) for c in pal[:, 0].tolist()}) == 16
    for fill, text in pal.tolist():
        luma = 0.2126 * fill[0] + 0.7152 * fill[1] + 0.0722 * fill[2]
        assert text == ([0, 0, 0] if luma >= 128 else [255, 255, 255])
    assert I.overlay_palette(3).shape == (3, 2, 3)
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            I.overlay_palette(bad)


def test_codes_are_cached_and_dropped():
    frame = C.surface("nv12", 4, 4).target
    a = I.overlay_codes(I.overlay_palette(4), (0, 0, 0), frame)
    assert a.shape == (9, 3) and a.dtype == torch.int32
    assert I.overlay_codes(I.overlay_palette(4), (0, 0, 0), frame) is a
    assert I.overlay_codes(I.overlay_palette(4), (0, 0, 1), frame) is not a
    I.invalidate_cache()
    assert I.overlay_codes(I.overlay_palette(4), (0, 0, 0), frame) is not a
    rgb = I.overlay_codes(I.overlay_palette(4), (7, 8, 9), torch.zeros(2, 2, 3, dtype=torch.uint8))
    assert rgb[-1].tolist() == [7, 8, 9] and rgb[:-1].tolist() == I.overlay_palette(4).reshape(-1, 3).tolist()


ROUND_TRIP = [(m, fr, d, ch) for m in ("bt601", "bt709", "bt2020") for fr in (False, True) for d in (8, 10, 12)
              for ch in ("nearest", "bilinear")]


@pytest.mark.parametrize("matrix,full_range,depth,chroma", ROUND_TRIP,
                         ids=[f"{m}-{'full' if f else 'limited'}-{d}-{c}" for m, f, d, c in ROUND_TRIP])
def test_codes_round_trip(matrix, full_range, depth, chroma):
    from walkai_nos_amd.models.workload.surfaces import YuvPlanar
    pal = I.overlay_palette()
    K = pal.shape[0]
    h, w = 16 * 4, 16 * 8           # 32 blocks of 16 x 16: fills and text colours
    dt = torch.uint8 if depth == 8 else torch.uint16
    g = torch.Generator().manual_seed(5)
    planes = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8).to(dt) for s in ((h, w), (h // 2, w // 2),
                                                                                          (h // 2, w // 2))]
    frame = YuvPlanar(*planes, "420", depth, False, matrix, full_range, chroma, "left")
    colours = pal.reshape(-1, 3)
    # entry k's fill and text colour as a palette of their own, each painted by a row of label k
    two = np.stack((colours, colours), axis=1)
    codes = I.overlay_codes(two, (0, 0, 0), frame)
    n = 2 * K
    boxes = torch.tensor([[16.0 * (k % 8), 16.0 * (k // 8), 16.0 * (k % 8) + 16, 16.0 * (k // 8) + 16] for k in range(n)])
    I.overlay_reference(frame, torch.tensor([n], dtype=torch.int32), torch.ones(n), torch.arange(n, dtype=torch.int32),
                        boxes, thickness=8, scale=0, modes=torch.ones(n, dtype=torch.uint8), codes=codes)
    rgb = frame.rgb()[0].to(torch.int32)
    m, _ = I.yuv_real_matrix(matrix, full_range, depth)
    bound = 0.5 * np.abs(m).sum(axis=1) + 1.0
    worst = np.zeros(3)
    for k in range(n):
        y0, x0 = 16 * (k // 8), 16 * (k % 8)
        block = rgb[y0 + 2:y0 + 14, x0 + 2:x0 + 14].reshape(-1, 3).numpy()
        worst = np.maximum(worst, np.abs(block - colours[k].astype(np.int64)).max(axis=0))
    print(f"[overlay] codes round trip {matrix} {'full' if full_range else 'limited'} {depth}-bit {chroma}: worst "
          f"|d| per channel {worst.tolist()} levels, bound {np.round(bound, 2).tolist()}")
    assert (worst <= bound).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _call(target=None, **kw):
    sc = C.priority_scene(H, W)
    count, scores, labels, boxes, ids, hits = sc.tensors()
    target = C.surface("nv12", H, W).target if target is None else target
    a = dict(count=count, scores=scores, labels=labels, boxes=boxes, track_id=None, track_hits=None, thickness=2,
             scale=1, modes=torch.tensor(sc.modes, dtype=torch.uint8), min_hits=1,
             codes=I.overlay_codes(I.overlay_palette(), (0, 0, 0), C.surface("nv12", H, W).target))
    a.update(kw)
    lists = [a.pop(k) for k in ("count", "scores", "labels", "boxes", "track_id", "track_hits")]
    return I.overlay(target, *lists, **a)


def test_wrapper_refuses():
    from walkai_nos_amd.models.workload.processor import Packed
    from walkai_nos_amd.models.workload.surfaces import YuvPlanar
    surf = C.surface("nv12", H, W)
    before = surf.storage.clone()
    _call(surf.target)
    assert not torch.equal(surf.storage, before)            # the call itself is sound
    n = len(C.priority_scene(H, W).scores)
    i32 = torch.int32
    hdr = YuvPlanar(torch.zeros(4, 4, dtype=torch.uint16), torch.zeros(2, 2, dtype=torch.uint16),
                    torch.zeros(2, 2, dtype=torch.uint16), "420", 10, transfer="pq")
    bad = [dict(target=torch.zeros(2, 4, 4, 3, dtype=torch.uint8)),                  # a batch
           dict(target=Packed(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), "bgr")),
           dict(target=hdr),                                                          # not SDR
           dict(target=torch.zeros(4, 4, 3)), dict(target=torch.zeros(4, 4, 4, dtype=torch.uint8)),
           dict(target=torch.zeros(1, 4, 3, dtype=torch.uint8).expand(4, 4, 3)),     # not writable memory
           dict(target=torch.zeros(4, 8, 3, dtype=torch.uint8)[:, ::2]),
           dict(target="frame"),
           dict(thickness=0), dict(scale=-1), dict(min_hits=0),
           dict(scores=torch.zeros(n, dtype=i32)), dict(labels=torch.zeros(n)), dict(boxes=torch.zeros(n, 3)),
           dict(labels=torch.zeros(n + 1, dtype=i32)), dict(count=torch.zeros(2, dtype=i32)),
           dict(scores=torch.zeros(2, n)), dict(track_id=torch.ones(n, dtype=i32)),
           dict(track_id=torch.ones(n, dtype=i32), track_hits=torch.ones(n)),
           dict(modes=[1, 1]), dict(modes=torch.ones(4, dtype=i32)), dict(modes=torch.ones(0, dtype=torch.uint8)),
           dict(codes=torch.zeros(4, 3, dtype=i32)), dict(codes=torch.zeros(5, 3)), dict(codes=torch.zeros(5, 4, dtype=i32)),
           dict(codes=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            _call(**kw)
    for pal in (np.zeros((2, 3, 3), dtype=np.uint8), np.zeros((0, 2, 3), dtype=np.uint8), np.full((2, 2, 3), 256),
                np.zeros((2, 2, 3))):
        with pytest.raises(ValueError):
            I.overlay_codes(pal, (0, 0, 0), surf.target)
    for red in ((0, 0), (0, 0, 256), (0.5, 0, 0)):
        with pytest.raises(ValueError):
            I.overlay_codes(I.overlay_palette(), red, surf.target)


def test_overlay_class_defaults_and_checks():
    o = Overlay()
    assert o.sizes(1080, 1920) == (6, 3) and o.sizes(97, 131) == (2, 1) and o.sizes(2160, 3840) == (12, 6)
    assert Overlay(tags=False).sizes(1080, 1920) == (6, 0) and Overlay(thickness=3, scale=2).sizes(50, 50) == (3, 2)
    o = Overlay(redact=(1, 5), modes={5: "off", 7: 2, 1: "redact"}, num_labels=9)
    assert o.modes == (1, 2, 1, 1, 1, 0, 1, 2, 1)
    for kw in (dict(thickness=0), dict(scale=-1), dict(min_hits=0), dict(num_labels=0), dict(redact=(91,)),
               dict(modes={0: 3}), dict(palette=np.zeros((2, 3))), dict(redact_colour=(0, 0))):
        with pytest.raises(ValueError):
            Overlay(**kw)
    # draw: by label without ids, by id with them; a CPU frame takes the reference
    surf = C.surface("bgra", H, W)
    sc = C.priority_scene(H, W)
    count, scores, labels, boxes, _, _ = sc.tensors()
    det = {"count": count, "scores": scores[None], "labels": labels[None], "boxes": boxes[None]}
    o = Overlay(thickness=sc.t, scale=sc.s, redact=(2,), modes={3: 0}, redact_colour=(9, 200, 31), num_labels=8)
    before = bytes(surf.storage.numpy().tobytes())
    assert o.draw(det, surf.target) is surf.target
    codes = I.overlay_codes(I.overlay_palette(), (9, 200, 31), surf.target)
    assert C.check(surf, before, C.slots(sc, H, W), codes.tolist()) > 0
    with pytest.raises(ValueError):
        o.draw({**det, "scores": scores[None].expand(2, -1)}, surf.target)


# ---- the pod client's flags ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,word", [
    (["--annotate"], "--end-to-end"),
    (["--end-to-end", "--annotate", "--pixel-format", "p010", "--transfer", "pq"], "--transfer"),
    (["--end-to-end", "--annotate", "--pixel-format", "i010", "--transfer", "hlg"], "--transfer"),
    (["--end-to-end", "--annotate", "--annotate-thickness", "0"], "--annotate-thickness"),
    (["--end-to-end", "--annotate", "--annotate-scale", "0"], "--annotate-scale"),
    (["--end-to-end", "--annotate", "--redact", "1,x"], "--redact"),
    (["--end-to-end", "--annotate", "--redact", "91"], "--redact"),
    (["--end-to-end", "--redact", "1"], "--annotate"),
    (["--end-to-end", "--no-tags"], "--annotate")])
def test_client_checks_the_annotate_flags(capsys, argv, word):
    from walkai_nos_amd.dataplane import client
    with pytest.raises(SystemExit) as e:
        client.main(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err
