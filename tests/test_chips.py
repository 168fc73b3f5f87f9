"""``ops.image.chips_reference`` on the CPU against the rule as a plain Python loop over ints (``loop`` below shares no
code with ``ops/image.py``), and the slot bookkeeping. There are no tolerances."""
import math

import pytest
import torch

from walkai_nos_amd.ops import image as I

H, W = 7, 9
BOXES = [[0, 0, 9, 7], [1.5, 2.25, 6.5, 5.0], [4, 3, 5, 4], [-3, -2, 2.5, 9], [7.2, 0, 30, 3], [20, 1, 25, 3],
         [2, 2, 2, 5], [float("nan"), 0, 3, 3]]


def frame():
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)


def lists(boxes, labels=None, scores=None, count=None):
    n = len(boxes)
    return (torch.tensor([n if count is None else count], dtype=torch.int32),
            torch.tensor(scores or [0.9] * n), torch.tensor(labels or [0] * n, dtype=torch.int32),
            torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4))


def loop(img, boxes, S_h, S_w, capacity, margin):
    """Rules 2 to 4 for rows that pass the filters: ``(chips, rows, rects)`` as nested lists."""
    chips, rows, rects = [], [], []
    for r, b in enumerate(boxes):
        if not all(math.isfinite(c) for c in b):
            continue
        x0, y0, x1, y1 = math.floor(b[0]), math.floor(b[1]), math.ceil(b[2]), math.ceil(b[3])
        if x1 <= x0 or y1 <= y0:
            continue
        X0, Y0, X1, Y1 = max(x0 - margin, 0), max(y0 - margin, 0), min(x1 + margin, W), min(y1 + margin, H)
        if X1 <= X0 or Y1 <= Y0 or len(rows) == capacity:
            continue
        bh, bw = Y1 - Y0, X1 - X0
        chip = [[[0] * 3 for _ in range(S_w)] for _ in range(S_h)]
        for j in range(S_h):
            for i in range(S_w):
                for c in range(3):
                    total = 0
                    for sy in range(bh):
                        wy = min((sy + 1) * S_h, (j + 1) * bh) - max(sy * S_h, j * bh)
                        for sx in range(bw):
                            wx = min((sx + 1) * S_w, (i + 1) * bw) - max(sx * S_w, i * bw)
                            if wy > 0 and wx > 0:
                                total += wy * wx * int(img[Y0 + sy][X0 + sx][c])
                    chip[j][i][c] = (total + bh * bw // 2) // (bh * bw)
        chips.append(chip), rows.append(r), rects.append([X0, Y0, X1, Y1])
    return chips, rows, rects


@pytest.mark.parametrize("margin", (0, 2))
@pytest.mark.parametrize("size", ((1, 1), (3, 5), (8, 8)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_is_the_loop(size, margin):
    img = frame()
    chips, rows, rects, n = I.chips_reference(img, *lists(BOXES), size=size, select=torch.ones(1, dtype=torch.uint8),
                                              capacity=8, margin=margin)
    want = loop(img.tolist(), BOXES, *size, 8, margin)
    k = len(want[1])
    assert k == 5 and n.tolist() == [k] and rows.tolist() == want[1] + [-1] * (8 - k)
    assert rects.tolist() == want[2] + [[0] * 4] * (8 - k)
    assert chips[:k].tolist() == want[0] and not chips[k:].any()
    assert chips.shape == (8,) + size + (3,) and chips.dtype == torch.uint8


def test_slots_filters_and_overflow():
    img = frame()
    boxes = [[k % 5, k % 3, k % 5 + 3, k % 3 + 2] for k in range(12)]
    labels = [0, 1, 2, 0, 5, -1, 0, 0, 1, 0, 0, 0]            # 2: not selected; 5 and -1: outside [0, L)
    scores = [0.9, 0.9, 0.9, 0.0, 0.9, 0.9, float("nan"), 0.9, 0.9, 0.9, 0.9, 0.9]
    select = torch.tensor([1, 1, 0], dtype=torch.uint8)
    kw = dict(size=(2, 2), select=select, margin=0)
    chips, rows, rects, n = I.chips_reference(img, *lists(boxes, labels, scores, count=11), capacity=4, **kw)
    assert rows.tolist() == [0, 1, 7, 8] and n.tolist() == [4]       # 9 and 10 overflow; 11 lies behind count
    assert rects[2].tolist() == [2, 1, 5, 3]
    full = I.chips_reference(img, *lists(boxes, labels, scores, count=99), capacity=16, **kw)
    assert full[1].tolist() == [0, 1, 7, 8, 9, 10, 11] + [-1] * 9 and torch.equal(full[0][:4], chips)
    ids, hits = torch.arange(12, dtype=torch.int32), torch.tensor([3] * 6 + [1] * 6, dtype=torch.int32)
    held = I.chips_reference(img, *lists(boxes, labels, scores), ids, hits, capacity=4, min_hits=2, **kw)
    assert held[1].tolist() == [1, -1, -1, -1] and held[3].tolist() == [1]      # id 0 is no track
    for count in (0, -5):
        none = I.chips_reference(img, *lists(boxes, labels, scores, count=count), capacity=4, **kw)
        assert none[3].tolist() == [0] and not none[0].any() and none[1].tolist() == [-1] * 4
    for bad in (dict(size=(0, 4)), dict(capacity=0), dict(margin=65), dict(margin=-1)):
        with pytest.raises(ValueError):
            I.chips(img, *lists(boxes), **{**kw, "capacity": 4, **bad})
    # on the CPU chips is the reference, and the op is served whatever the size
    big = I.chips(img, *lists(boxes), size=(300, 2), select=select, capacity=300)
    assert big[0].shape == (300, 300, 2, 3) and big[3].tolist() == [12]
