"""Inputs and the independent reference of the tile tests (``tests/test_tiles.py`` on the CPU,
``tests/test_gpu_tiles.py`` on the GPU): a synthetic frame of four overlapping tiles with a handful of objects, and
the merge of ``ops.image.merge_detections`` written as a plain double loop over Python floats (fp64), with the
margins by which it decides.

The frame is 96 x 128, cut into four tiles of 56 x 72 at ``(0, 0), (0, 56), (40, 0), (40, 56)``: columns 56..72 and
rows 40..56 are seen twice, their crossing four times. A tile reports every object it sees as the object's box clipped
to the tile (a cut object yields a partial box), as a detector that sees only the tile would:

* ``A`` lies wholly inside the crossing: four tiles report the same box (one survives either way);
* ``B`` lies inside tile 1 and is cut by tile 0's border: a partial box inside the full one, IoS 1 and IoU about 0.3
  (``ios`` drops it, ``iou`` keeps it);
* ``C`` is seen by tile 2 alone;
* ``D`` and ``E`` share one place in tiles 2 and 3 with different labels (one of each survives);
* ``F`` is cut by the borders of tiles 1 and 3, neither part inside the other: IoS about 0.6, IoU about 0.4;
* ``G`` lies whole in tiles 0 and 2;
* ``H`` is one bit-identical row (logits and tile-relative box) in tiles 0 and 3, so two equal scores at two places of
  the frame: both survive, in tile order.

Every other row is dominated by "no object". 17 candidates; 9 survive under ``ios`` and 11 under ``iou``."""
import math

import torch

TILE_HW = (56, 72)
ORIGINS = ((0, 0), (0, 56), (40, 0), (40, 56))
FRAME_HW = (96, 128)
M, CLASSES = 12, 12            # rows per tile; classes with "no object"
THRESHOLD, MATCH_THRESHOLD = 0.5, 0.5
#: (name, label, x0, y0, x1, y1) in frame pixels
OBJECTS = (("A", 3, 58.0, 42.0, 70.0, 54.0), ("B", 5, 60.0, 5.0, 100.0, 30.0), ("C", 7, 5.0, 60.0, 30.0, 90.0),
           ("D", 1, 58.0, 60.0, 70.0, 90.0), ("E", 2, 58.0, 60.0, 70.0, 90.0), ("F", 5, 80.0, 30.0, 120.0, 70.0),
           ("G", 9, 20.0, 44.0, 50.0, 52.0))


def synthetic(seed: int = 0):
    """``(logits [4, M, CLASSES], boxes [4, M, 4])`` fp32 on the CPU: the objects above, jittered by ``seed``."""
    g = torch.Generator().manual_seed(1000 + seed)
    th, tw = TILE_HW
    logits = 0.3 * torch.randn(len(ORIGINS), M, CLASSES, generator=g)
    logits[..., -1] = 6.0                                      # "no object" wins every row that holds nothing
    boxes = 0.3 + 0.4 * torch.rand(len(ORIGINS), M, 4, generator=g)
    used = [0] * len(ORIGINS)
    n = 0
    for _, label, x0, y0, x1, y1 in OBJECTS:
        dx, dy = (torch.rand(2, generator=g) - 0.5).tolist()   # the object moves by up to half a pixel
        for b, (oy, ox) in enumerate(ORIGINS):
            cx0, cy0 = max(x0 + dx, ox), max(y0 + dy, oy)
            cx1, cy1 = min(x1 + dx, ox + tw), min(y1 + dy, oy + th)
            if cx1 - cx0 < 4.0 or cy1 - cy0 < 4.0:
                continue
            m = used[b]
            used[b] += 1
            boxes[b, m] = torch.tensor([(0.5 * (cx0 + cx1) - ox) / tw, (0.5 * (cy0 + cy1) - oy) / th,
                                        (cx1 - cx0) / tw, (cy1 - cy0) / th])
            logits[b, m, -1] = -1.0
            logits[b, m, label] = 4.0 + 0.17 * n               # a score of its own: 0.8 and up, about 0.01 apart
            n += 1
    # H: one row, bit for bit, in tiles 0 and 3 (the last row of each)
    logits[0, M - 1, -1] = -1.0
    logits[0, M - 1, 10] = 3.5
    boxes[0, M - 1] = torch.tensor([0.2, 0.2, 0.1, 0.1])
    logits[3, M - 1] = logits[0, M - 1]
    boxes[3, M - 1] = boxes[0, M - 1]
    return logits, boxes


def ramp(B: int = 10, rows: int = 100, classes: int = 92, seed: int = 0, hole: bool = False):
    """A full table: ``B * rows`` rows whose winning logit falls along a ramp, so that neighbouring scores differ by
    at least 1e-5 (random rows do not). ``(logits, boxes)`` fp32; the rows are shuffled. ``hole``: no winning logit
    in (-1, 1), so no score in (0.13, 0.5): a threshold of 0.3 decides every row clearly."""
    g = torch.Generator().manual_seed(2000 + seed)
    N = B * rows
    logits = torch.full((N, classes), -4.0)
    # winner at z, "no object" at 0, the rest at -4: score = e^z / (e^z + 1 + 90 e^-4); d score / dz >= 0.017 on
    # [-3, 3], so steps of at least 3.6e-3 move the score by at least 6e-5
    z = torch.linspace(-3.0, 3.0, N)
    if hole:
        z = torch.cat((torch.linspace(-3.0, -1.0, N // 2), torch.linspace(1.0, 3.0, N - N // 2)))
    z = z[torch.randperm(N, generator=g)]
    label = torch.randint(0, classes - 1, (N,), generator=g)
    logits[:, -1] = 0.0
    logits[torch.arange(N), label] = z
    boxes = 0.2 + 0.6 * torch.rand(N, 4, generator=g)
    return logits.reshape(B, rows, classes), boxes.reshape(B, rows, 4)


def _overlap(a, b, match):
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    inter = iw * ih
    aa, ab = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
    den = aa + ab - inter if match == "iou" else min(aa, ab)
    return inter / den if den > 0.0 else 0.0


def merge_loop(logits, boxes, origins, tile_hw, threshold, match, match_threshold, dropped=None):
    """The merge as a double loop over Python floats. Returns ``(kept, margins)``: ``kept`` the list of ``(score,
    label, (x0, y0, x1, y1), tile, row)`` in output order, ``margins`` the smallest ``|score - threshold|``, label
    gap of a candidate (best - second of the first L classes), gap between two different candidate scores, and ``|overlap -
    match_threshold|`` over the pairs the pass compared. The candidates it drops are appended to ``dropped``."""
    B, rows, C = logits.shape
    th, tw = tile_hw
    lg, bx = logits.double().tolist(), boxes.double().tolist()
    cands = []
    m_thr = m_label = m_gap = m_ov = math.inf
    for b in range(B):
        for m in range(rows):
            top = max(lg[b][m])
            e = [math.exp(v - top) for v in lg[b][m]]
            s = sum(e)
            p = [v / s for v in e[:-1]]
            score = max(p)
            label = p.index(score)
            m_thr = min(m_thr, abs(score - threshold))
            if score > threshold:
                # (the label of a row below the threshold is never written: its near-ties decide nothing)
                # (one class beside "no object": no second, and nothing to decide)
                m_label = min(m_label, score - max((v for i, v in enumerate(p) if i != label), default=-math.inf))
                cx, cy, w, h = bx[b][m]
                oy, ox = origins[b]
                cands.append((score, label, ((cx - 0.5 * w) * tw + ox, (cy - 0.5 * h) * th + oy,
                                             (cx + 0.5 * w) * tw + ox, (cy + 0.5 * h) * th + oy), b, b * rows + m))
    cands.sort(key=lambda c: (-c[0], c[4]))
    for a, b in zip(cands, cands[1:]):
        if a[0] != b[0]:
            m_gap = min(m_gap, a[0] - b[0])
    kept = []
    for c in cands:
        drop = False
        for k in kept:
            if k[1] == c[1] and k[3] != c[3]:
                ov = _overlap(k[2], c[2], match)
                m_ov = min(m_ov, abs(ov - match_threshold))
                if ov > match_threshold:
                    drop = True
                    break
        if not drop:
            kept.append(c)
        elif dropped is not None:
            dropped.append(c)
    return kept, (m_thr, m_label, m_gap, m_ov)


def freed(kept, dropped, match, match_threshold):
    """The kept candidates that an earlier *dropped* one would have suppressed: rows a pass that ignored whether the
    pivot is still kept would lose."""
    return [c for c in kept if any((-d[0], d[4]) < (-c[0], c[4]) and d[1] == c[1] and d[3] != c[3]
                                   and _overlap(d[2], c[2], match) > match_threshold for d in dropped)]


def decides_clearly(margins, threshold):
    """The conditions on the inputs under which fp32 and fp64 must agree on what is kept and in which order."""
    m_thr, m_label, m_gap, m_ov = margins
    assert m_thr >= 1e-3 or threshold in (0.0, 1.0), margins
    assert m_label >= 1e-3 and m_gap >= 1e-5 and m_ov >= 1e-3, margins


def check_merged(got, kept, N, score_tol, box_tol):
    """``got``: the five tensors of ``merge_detections`` (on the CPU) against ``merge_loop``'s list: equal count,
    labels, tiles and order, scores and boxes within the tolerances, zeros behind. Returns the worst differences."""
    count, scores, labels, xyxy, tile = got
    assert count.dtype == torch.int32 and labels.dtype == torch.int32 and tile.dtype == torch.int32
    assert count.shape == (1,) and scores.shape == (N,) and labels.shape == (N,) and xyxy.shape == (N, 4) \
        and tile.shape == (N,)
    n = len(kept)
    assert count.tolist() == [n], (count.tolist(), n)
    assert labels[:n].tolist() == [k[1] for k in kept]
    assert tile[:n].tolist() == [k[3] for k in kept]
    ds = max((abs(scores[i].item() - k[0]) for i, k in enumerate(kept)), default=0.0)
    db = max((abs(xyxy[i, c].item() - k[2][c]) for i, k in enumerate(kept) for c in range(4)), default=0.0)
    assert ds <= score_tol and db <= box_tol, (ds, score_tol, db, box_tol)
    assert not scores[n:].any() and not labels[n:].any() and not xyxy[n:].any() and not tile[n:].any()
    return ds, db
