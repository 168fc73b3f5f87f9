"""The row rule the image effects share — rules 1 and 2 of ``ops.image.overlay`` — held to a loop written out here:
``overlay_slots``, ``mosaic_cells`` and ``chip_rects`` must mark exactly the pixels the loop marks, with and without ids."""
import math

import numpy as np
import pytest
import torch

from walkai_nos_amd.ops import image as I

H, W, MIN_HITS = 12, 16, 2
SELECT = (1, 1, 0)          # label 2 is not selected
NAN, INF = float("nan"), float("inf")
SPOT = [6.0, 3.0, 9.0, 6.0]     # where a row that must not be drawn would show
#: (score, label, box, track id, track hits)
ROWS = [
    (0.9, 0, [2.0, 1.0, 5.0, 4.0], 5, 3),               # plain: columns 2..4, rows 1..3
    (0.9, 0, [NAN, 3.0, 9.0, 6.0], 5, 3),               # a NaN coordinate
    (0.9, 1, [6.0, 3.0, INF, 6.0], 5, 3),               # an infinite one
    (0.9, 1, [-INF, 3.0, 9.0, 6.0], 5, 3),
    (0.0, 0, SPOT, 5, 3),                               # score 0
    (NAN, 0, SPOT, 5, 3),                               # a NaN score
    (0.9, -1, SPOT, 5, 3),                              # labels outside 0 .. L - 1
    (0.9, len(SELECT), SPOT, 5, 3),
    (0.9, 2, SPOT, 5, 3),                               # an unselected label
    (0.9, 0, [5.5, 7.2, 7.0, 9.0], 0, 3),               # id 0: drawn without ids only, columns 5..6, rows 7..8
    (0.9, 1, [10.0, 5.0, 12.5, 6.5], 5, MIN_HITS - 1),  # too few hits: likewise, columns 10..12, rows 5..6
    (0.9, 0, [7.0, 3.0, 7.0, 6.0], 5, 3),               # x1 == x0 on an integer: empty
    (0.9, 0, [20.5, 3.0, 25.0, 8.0], 5, 3),             # wholly outside the frame
    (0.9, 1, [-9.0, -9.0, -1.5, -2.0], 5, 3),
    (0.9, 1, [13.4, 9.3, 18.7, 14.2], 7, 2),            # across the far corner: columns 13..15, rows 9..11
    (0.9, 0, [-2.5, -1.5, 1.2, 0.6], 8, 9),             # across the near corner: columns 0..1, row 0
    (0.9, 1, [-3e6, 10.0, 3e6, 10.5], 6, 4),            # past the clamp to +-2^20: the whole of row 10
    (0.9, 0, [9.0, 0.0, 11.0, 2.0], 9, 2),              # the last row: drawn when count reaches it
]


def loop(count: int, ids: bool) -> set:
    """The pixels ``(y, x)`` the rule paints, row by row."""
    marked = set()
    for r, (score, label, box, tid, hits) in enumerate(ROWS):
        if r >= min(max(count, 0), len(ROWS)) or not score > 0:
            continue
        if not 0 <= label < len(SELECT) or not SELECT[label] or not all(math.isfinite(v) for v in box):
            continue
        if ids and (tid <= 0 or hits < MIN_HITS):
            continue
        c = [min(max(np.float32(v), np.float32(-2 ** 20)), np.float32(2 ** 20)) for v in box]
        x0, y0, x1, y1 = math.floor(c[0]), math.floor(c[1]), math.ceil(c[2]), math.ceil(c[3])
        marked |= {(y, x) for y in range(max(y0, 0), min(y1, H)) for x in range(max(x0, 0), min(x1, W))}
    return marked


@pytest.mark.parametrize("ids", (False, True))
@pytest.mark.parametrize("count", (len(ROWS), len(ROWS) - 1, len(ROWS) + 5, -3))
def test_three_consumers_mark_the_loops_pixels(count, ids):
    i32 = torch.int32
    lists = (torch.tensor([count], dtype=i32), torch.tensor([r[0] for r in ROWS], dtype=torch.float32),
             torch.tensor([r[1] for r in ROWS], dtype=i32), torch.tensor([r[2] for r in ROWS], dtype=torch.float32),
             torch.tensor([r[3] for r in ROWS], dtype=i32) if ids else None,
             torch.tensor([r[4] for r in ROWS], dtype=i32) if ids else None)
    select = torch.tensor(SELECT, dtype=torch.uint8)
    want = loop(count, ids)
    assert (count > 0) == bool(want) and ((7, 5) in want) == ((5, 10) in want) == (count > 0 and not ids)
    pixels = lambda mask: {tuple(p) for p in mask.nonzero().tolist()}        # noqa: E731

    slots = I.overlay_slots(H, W, *lists, 1, 0, 2 * select, MIN_HITS, 4)      # every selected label redacted
    assert slots.shape == (H, W) and pixels(slots >= 0) == want
    cells = I.mosaic_cells(H, W, *lists, MIN_HITS, select, 1)
    assert cells.shape == (H, W) and pixels(cells) == want
    ok, rects = I.chip_rects(H, W, *lists, MIN_HITS, select, 0)
    union = {(y, x) for X0, Y0, X1, Y1 in rects[ok].tolist() for y in range(Y0, Y1) for x in range(X0, X1)}
    assert union == want and ok.dtype == torch.bool and rects.dtype == i32
