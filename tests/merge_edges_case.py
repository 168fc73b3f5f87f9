"""Inputs of the merge edge tests (``tests/test_merge_edges.py`` on the CPU, ``tests/test_gpu_merge_edges.py`` on the
GPU), so that both build identical tables. The yardstick is ``tiles_case.merge_loop``, the fp64 double loop; a case
carries its inputs, the margins it sets by hand (``exact``) and the outcome it expects beyond the loop's (``explicit``).

Seeds are searched on the CPU against the double loop alone (``guard``), never against the kernel or the torch
reference; ``test_merge_seeds_pass_the_guard_on_the_reference_alone`` recomputes every one of them."""
import math

import numpy as np
import torch

import tiles_case as T

#: the largest fp32 below 0.5: the threshold at which a score or an overlap of exactly 0.5 passes
BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
assert BELOW_HALF < 0.5 and np.float32(BELOW_HALF) == BELOW_HALF


class Case:
    """One call of ``merge_detections``. ``exact``: the margins (``"threshold"``, ``"overlap"``) that the case sets
    to zero by hand (an exact tie with a threshold), for which ``explicit`` asserts the outcome; ``explicit(got, kept,
    dropped)`` gets the five output tensors on the CPU and the loop's lists."""

    def __init__(self, name, logits, boxes, origins, tile_hw, thr, match="ios", mt=0.5, exact=(), explicit=None):
        self.name, self.logits, self.boxes = name, logits, boxes
        self.origins, self.tile_hw = [(int(y), int(x)) for y, x in origins], tile_hw
        self.thr, self.match, self.mt, self.exact, self.explicit = thr, match, mt, tuple(exact), explicit
        self.N = logits.shape[0] * logits.shape[1]
        assert len(self.origins) == logits.shape[0] and boxes.shape == logits.shape[:2] + (4,)
        assert logits.dtype == torch.float32 and boxes.dtype == torch.float32

    @property
    def frame_hw(self):
        return (max(y for y, _ in self.origins) + self.tile_hw[0], max(x for _, x in self.origins) + self.tile_hw[1])

    def args(self):
        return self.origins, self.tile_hw, self.thr, self.match, self.mt


_solved = {}


def solve(case):
    """``(kept, margins, dropped)`` of the double loop, computed once per case and left unchanged."""
    if case.name not in _solved:
        dropped = []
        kept, margins = T.merge_loop(case.logits, case.boxes, *case.args(), dropped)
        _solved[case.name] = (kept, margins, dropped)
    return _solved[case.name]


def guard(case):
    """``tiles_case.decides_clearly`` on the loop's margins. A margin a case sets by hand to zero is exempt (its
    outcome is asserted by ``explicit``, which such a case must have). At a match threshold of 1.0 no overlap decides
    anything: an overlap is a quotient of a non-negative number by one at least as large, in fp32 as in fp64, so it
    never exceeds 1 (boxes inside one another give exactly 1); such a case asserts that nothing is dropped."""
    kept, margins, dropped = solve(case)
    m_thr, m_label, m_gap, m_ov = margins
    assert not case.exact or case.explicit is not None, case.name
    if case.mt == 1.0:
        assert not dropped, case.name
        m_ov = math.inf
    T.decides_clearly((math.inf if "threshold" in case.exact else m_thr, m_label, m_gap,
                       math.inf if "overlap" in case.exact else m_ov), case.thr)
    return kept, margins, dropped


def finite(got):
    return all(bool(torch.isfinite(t.double()).all()) for t in got)


def table(B, M, C, rows, fill_box=(0.5, 0.5, 0.25, 0.25)):
    """``B`` tiles of ``M`` rows of ``C`` classes in which "no object" wins by 10 (scores below 1e-4), but for ``rows``:
    ``(tile, row, label, z, (cx, cy, w, h))`` puts the winning logit ``z`` against "no object" at 0, the rest at -4:
    a score of ``e^z / (e^z + 1 + (C - 2) e^-4)``."""
    logits = torch.full((B, M, C), -4.0)
    logits[..., -1] = 6.0
    boxes = torch.tensor(fill_box).repeat(B, M, 1)
    for b, m, label, z, box in rows:
        logits[b, m, -1] = 0.0
        logits[b, m, label] = z
        boxes[b, m] = torch.tensor(box)
    return logits, boxes


def cxcywh(x0, y0, x1, y1, origin=(0, 0), tile=64):
    """The tile-relative centre box of the frame box ``(x0, y0, x1, y1)``; exact for multiples of 1/2 on tiles of 64."""
    oy, ox = origin
    return (0.5 * (x0 + x1) - ox) / tile, (0.5 * (y0 + y1) - oy) / tile, (x1 - x0) / tile, (y1 - y0) / tile


# ---- rows and splits ------------------------------------------------------------------------------------------------
ROW_SHAPES = ((1, 1), (1, 63), (63, 1), (1, 64), (5, 13), (33, 31), (1024, 1), (4, 256), (1, 1024))
#: (B, M, match) -> (seed of ``tiles_case.ramp``, survivors): the first seed of 0..5 at which the loop decides clearly
ROW_SEEDS = {(1, 1, "ios"): (0, 1), (1, 63, "ios"): (0, 32), (63, 1, "ios"): (0, 30), (1, 64, "ios"): (0, 32),
             (5, 13, "ios"): (0, 31), (33, 31, "ios"): (1, 296), (1024, 1, "ios"): (2, 292), (4, 256, "ios"): (0, 327),
             (1, 1024, "ios"): (0, 512), (4, 256, "iou"): (0, 484), (33, 31, "iou"): (0, 475)}


def row_origins(B):
    return [((7 * b) % 40, (11 * b) % 60) for b in range(B)]


def rows_case(B, M, match="ios"):
    seed, want = ROW_SEEDS[(B, M, match)]
    logits, boxes = T.ramp(B, M, seed=seed, hole=True)

    def explicit(got, kept, dropped):
        assert len(kept) == want and len(kept) + len(dropped) == B * M - (B * M) // 2
        assert B == 1 or B * M < 60 or dropped         # the tiles overlap: some rows go
        assert B > 1 or not dropped                    # one tile drops nothing
    return Case(f"rows {B}x{M} {match}", logits, boxes, row_origins(B), (100, 100), 0.3, match, 0.5, explicit=explicit)


def rows_full_case():
    """1024 rows, every one a candidate and kept: nothing is zero-filled."""
    logits, boxes = T.ramp(4, 256, seed=ROW_SEEDS[(4, 256, "ios")][0], hole=True)

    def explicit(got, kept, dropped):
        assert len(kept) == 1024 and got[0].tolist() == [1024] and bool((got[1] > 0).all())
    return Case("rows 4x256 all kept", logits, boxes, row_origins(4), (100, 100), 0.0, "ios", 1.0, explicit=explicit)


# ---- class counts ---------------------------------------------------------------------------------------------------
#: rows (of 4 x 25, as b * 25 + m) the class-count cases set by hand
HAND = (3, 40, 41, 77, 99)
#: C -> seed of the ramp at which the loop decides both runs clearly
CLASS_SEEDS = {2: 0, 3: 0, 64: 0, 65: 0, 66: 0, 128: 0}
CLASS_ORIGINS = [(0, 0), (0, 40), (30, 0), (30, 40)]


def class_hand_label(C, i):
    """The label the ``i``-th hand-set row is built for."""
    if C == 66:
        return 64                       # the first class of the upper 64-lane half
    if C == 128:
        return (126, 64, 63, 0, 65)[i]  # the last class, and around the halves
    return (11 * i + 5) % (C - 1)


def class_case(C, every=False):
    """4 tiles of 25 rows of ``C`` classes along the ramp. For 64 and 65 "no object" (lane 63 of the lower half, lane
    0 of the upper) is the largest logit on the hand-set rows, by 3 to 5, so their scores (0.05 to 0.007) stay a
    clear step apart; for 66 class 64 is their true best. ``every``: threshold 0 and match threshold 1, so that every
    row comes out with its label."""
    logits, boxes = T.ramp(4, 25, classes=C, seed=CLASS_SEEDS[C], hole=True)
    flat = logits.view(100, C)
    if C >= 64:
        for i, r in enumerate(HAND):
            flat[r] = -4.0
            flat[r, class_hand_label(C, i)] = 2.0 + 0.1 * i
            flat[r, C - 1] = 5.0 + 0.6 * i if C in (64, 65) else 0.0

    def explicit(got, kept, dropped):
        n = len(kept)
        assert int(got[2].min()) >= 0 and int(got[2].max()) <= C - 2
        rows = {k[4]: i for i, k in enumerate(kept)}
        if every:
            assert n == 100
            for r in range(100):        # every row's label is the largest of its first C - 1 logits
                assert got[2][rows[r]].item() == flat[r, :C - 1].argmax().item(), r
        if C >= 64:
            for i, r in enumerate(HAND):
                if C in (64, 65):
                    assert flat[r].argmax().item() == C - 1
                    assert every or r not in rows
                if r in rows:
                    assert got[2][rows[r]].item() == class_hand_label(C, i), (C, r)
                    assert (got[1][rows[r]].item() < 0.06) == (C in (64, 65))
        if C == 2 and not every:
            assert len(dropped) >= 3 and n + len(dropped) == 50     # one label: every cross-tile pair is compared
    if every:
        return Case(f"classes C={C} every row", logits, boxes, CLASS_ORIGINS, (100, 100), 0.0, "ios", 1.0,
                    explicit=explicit)
    return Case(f"classes C={C}", logits, boxes, CLASS_ORIGINS, (100, 100), 0.3, "ios", 0.5, explicit=explicit)


# ---- the ends of the pivot loop -------------------------------------------------------------------------------------
def _count(n, tiles=None):
    def explicit(got, kept, dropped):
        assert len(kept) == n and got[0].tolist() == [n]
        if tiles is not None:
            assert got[4][:n].tolist() == list(tiles)
    return explicit


def pivot_cases():
    two = [(0, 0), (0, 32)]
    dup0, dup1 = cxcywh(36, 8, 44, 24, two[0]), cxcywh(36, 8, 44, 24, two[1])
    out = []
    # scores 0.94, 0.86, 0.69, 0.43: the threshold 0.9 lies between the top two
    rows = [(0, 1, 2, 3.0, (0.3, 0.3, 0.2, 0.2)), (1, 3, 2, 2.0, (0.3, 0.3, 0.2, 0.2)),
            (1, 0, 1, 1.0, (0.6, 0.6, 0.2, 0.2)), (0, 4, 0, 0.0, (0.7, 0.2, 0.1, 0.1))]
    out.append(Case("pivot one candidate", *table(2, 5, 5, rows), two, (64, 64), 0.9, explicit=_count(1, [0])))
    rows = [(0, 4, 3, 2.0, dup0), (1, 1, 3, 3.0, dup1)]
    out.append(Case("pivot two duplicates", *table(2, 5, 5, rows), two, (64, 64), 0.5, explicit=_count(1, [1])))
    rows = [(1, 4, 3, 2.0, dup1), (1, 1, 3, 3.0, dup1)]
    out.append(Case("pivot two in one tile", *table(2, 5, 5, rows), two, (64, 64), 0.5, explicit=_count(2, [1, 1])))
    return out


#: the 1024-row table's hand-set rows: (tile, row) of the second-to-last and of the last candidate
LAST_PAIR = ((3, 250), (0, 5))


def pivot_last_case():
    """4 x 256 rows along the ramp (winning logits from 1 up among the candidates), and two hand-set rows with winning
    logits 0.9 and 0.8: the two lowest-scoring candidates, one box at (500..510, 500..510) of the frame seen from
    tiles 3 and 0, label 90, far from every other box (those end before 200). The second-to-last candidate is the
    last pivot of the pass and drops the last one."""
    logits, boxes = T.ramp(4, 256, seed=ROW_SEEDS[(4, 256, "ios")][0], hole=True)
    origins = row_origins(4)
    for (b, m), z in zip(LAST_PAIR, (0.9, 0.8)):
        logits[b, m] = -4.0
        logits[b, m, -1] = 0.0
        logits[b, m, 90] = z
        boxes[b, m] = torch.tensor(cxcywh(500, 500, 510, 510, origins[b], 100))
    assert boxes.view(-1, 4)[:, :2].max().item() > 4.0 and (boxes[..., 2:] > 0).all()

    def explicit(got, kept, dropped):
        n = len(kept)
        (b1, m1), (b0, m0) = LAST_PAIR
        assert kept[-1][4] == b1 * 256 + m1 and kept[-1][1] == 90 and dropped[-1][4] == b0 * 256 + m0
        assert dropped[-1][0] < kept[-1][0] < min(k[0] for k in kept[:-1])       # the two lowest scores
        assert got[0].tolist() == [n] and got[4][n - 1].item() == b1 and got[2][n - 1].item() == 90
        assert abs(got[3][n - 1, 0].item() - 500.0) < 1e-3 and not got[1][n:].any()
    return Case("pivot drops the last", logits, boxes, origins, (100, 100), 0.3, explicit=explicit)


# ---- strictness -----------------------------------------------------------------------------------------------------
def strict_match_cases():
    """Two tiles of 64 x 64 at (0, 0); corners in multiples of 1/2: frame coordinates, areas and the quotient are exact
    in fp32 and in fp64. The pair under test overlaps by exactly 0.5; a second pair of identical boxes of another label
    (overlap 1) is dropped to one at either threshold."""
    org = [(0, 0), (0, 0)]
    out = []
    for match, second in (("ios", (4, 0, 12, 8)), ("iou", (0, 0, 8, 4))):
        rows = [(0, 2, 1, 3.0, cxcywh(0, 0, 8, 8)), (1, 1, 1, 2.0, cxcywh(*second)),
                (0, 0, 4, 1.5, cxcywh(32, 32, 40, 40)), (1, 3, 4, 2.5, cxcywh(32, 32, 40, 40))]
        assert T._overlap((0.0, 0.0, 8.0, 8.0), tuple(float(v) for v in second), match) == 0.5
        logits, boxes = table(2, 4, 6, rows)
        for mt, n, tiles in ((0.5, 3, [0, 1, 1]), (BELOW_HALF, 2, [0, 1])):
            out.append(Case(f"strict {match} match threshold {'0.5' if mt == 0.5 else 'below 0.5'}", logits, boxes, org,
                            (64, 64), 0.5, match, mt, exact=("overlap",), explicit=_count(n, tiles)))
    return out


def strict_score_cases():
    """Logits ``[0, 0]`` at two classes score exactly 1 / 2 in fp32 and in fp64; every box lies apart from the others
    (one label: any overlap would be compared)."""
    logits = torch.tensor([[[3.0, -3.0], [0.0, 0.0], [-3.0, 3.0]], [[0.0, 0.0], [2.0, -2.0], [0.0, 0.0]]])
    boxes = torch.tensor([[[(2 * i + 1) / 16, (2 * b + 1) / 8, 1 / 16, 1 / 16] for i in range(3)] for b in range(2)])

    def at_half(got, kept, dropped):
        assert got[0].tolist() == [2] and got[4][:2].tolist() == [0, 1]

    def below(got, kept, dropped):
        assert got[0].tolist() == [5] and got[4][:5].tolist() == [0, 1, 0, 1, 1]
        assert got[1][2:5].tolist() == [0.5, 0.5, 0.5]              # the tie of three: rows 1, 3, 5
        assert got[3][2:5, 0].tolist() == [kept[i][2][0] for i in (2, 3, 4)] and [k[4] for k in kept] == [0, 4, 1, 3, 5]
    return [Case("strict score threshold 0.5", logits, boxes, [(0, 0), (0, 0)], (64, 64), 0.5, exact=("threshold",),
                 explicit=at_half),
            Case("strict score threshold below 0.5", logits, boxes, [(0, 0), (0, 0)], (64, 64), BELOW_HALF,
                 exact=("threshold",), explicit=below)]


TIE_ORIGINS = [(0, 0), (0, 64), (64, 0), (64, 64)]


def tie_block_case():
    """4 tiles of 20 rows. 64 rows hold one bit-identical logit row (label 7, z = 1.5), 16 per tile at scattered rows,
    each in a cell of its own of the tile's 4 x 4 grid; the other 16 rows score above (tiles 0, 1) or below (tiles 2,
    3) the block, with other labels. The block comes out in row order."""
    rows = []
    for b in range(4):
        for m in range(20):
            cell = ((m % 4 + 0.5) / 4, (m // 4 % 4 + 0.5) / 4, 1 / 8, 1 / 8)
            if m % 5 == 2:
                rows.append((b, m, b, (2.0 + 0.2 * m if b < 2 else 1.0 - 0.02 * m) + 0.01 * b, cell))
            else:
                rows.append((b, m, 7, 1.5, cell))
    logits, boxes = table(4, 20, 12, rows)
    block = [b * 20 + m for b in range(4) for m in range(20) if m % 5 != 2]
    assert len(block) == 64 and len({tuple(logits.view(80, 12)[r].tolist()) for r in block}) == 1

    def explicit(got, kept, dropped):
        assert got[0].tolist() == [80] and [k[4] for k in kept[8:72]] == block
        assert got[4][8:72].tolist() == [r // 20 for r in block] and len(set(got[1][8:72].tolist())) == 1
        assert got[2][8:72].tolist() == [7] * 64 and got[1][7].item() > got[1][8].item() > got[1][72].item()
        for i, r in enumerate(block):       # each box is its own row's
            b, m = divmod(r, 20)
            assert abs(got[3][8 + i, 0].item() - (((m % 4 + 0.5) / 4 - 1 / 16) * 64 + TIE_ORIGINS[b][1])) < 1e-3
    return Case("tie block of 64", logits, boxes, TIE_ORIGINS, (64, 64), 0.5, explicit=explicit)


def tie_pair_case():
    """Two equal-score pairs of one label each that overlap fully across tiles: the lower row survives, which is row 7
    of tile 0 against row 2 of tile 1, and row 9 of tile 1 against row 0 of tile 2."""
    org = [(0, 0), (0, 32), (0, 16)]
    rows = [(0, 7, 3, 2.0, cxcywh(36, 8, 44, 24, org[0])), (1, 2, 3, 2.0, cxcywh(36, 8, 44, 24, org[1])),
            (1, 9, 5, 1.0, cxcywh(50, 30, 60, 40, org[1])), (2, 0, 5, 1.0, cxcywh(50, 30, 60, 40, org[2]))]
    return Case("tie pair overlapping", *table(3, 10, 8, rows), org, (64, 64), 0.5, explicit=_count(2, [0, 1]))


# ---- what must not suppress -----------------------------------------------------------------------------------------
def same_tile_case():
    box = (0.5, 0.5, 0.25, 0.5)
    rows = [(1, m, 4, 1.0 + 0.2 * ((3 * m) % 10), box) for m in range(10)] + [(0, 3, 2, 2.5, box)]
    return Case("ten identical boxes in one tile", *table(2, 12, 6, rows), [(0, 0), (0, 0)], (64, 64), 0.5,
                explicit=_count(11))


def other_label_case():
    box = (0.5, 0.5, 0.25, 0.5)
    rows = [(0, 1, 2, 2.0, box), (1, 1, 3, 1.0, box), (0, 2, 0, 1.5, box), (1, 0, 4, 2.5, box)]
    return Case("identical boxes, other labels", *table(2, 3, 6, rows), [(0, 0), (0, 0)], (64, 64), 0.5,
                explicit=_count(4, [1, 0, 0, 1]))


def one_tile_inputs():
    """``B = 1``: 100 rows, 92 classes, two rows bit-identical; with the threshold and the target of ``detections``."""
    g = torch.Generator().manual_seed(9)
    logits, boxes = 3.0 * torch.randn(1, 100, 92, generator=g), 0.2 + 0.6 * torch.rand(1, 100, 4, generator=g)
    logits[0, 40] = logits[0, 20]
    return logits, boxes, (37, 53), 0.3


# ---- degenerate boxes -----------------------------------------------------------------------------------------------
def degenerate_cases():
    """Two tiles at one origin, match threshold 0: any positive overlap would drop a row. Zero-width, zero-area and
    negative-width boxes, each twice (one label, both tiles, identical), and a zero-area box of tile 1 inside a normal
    box of tile 0: every denominator that is not positive, or every intersection, is 0, so all rows are kept."""
    kinds = (("zero width", cxcywh(8, 8, 8, 16)), ("zero area", cxcywh(20, 20, 20, 20)),
             ("negative width", cxcywh(36, 8, 30, 16)))
    rows = []
    for i, (_, box) in enumerate(kinds):
        rows += [(0, i, i, 3.0 - 0.3 * i, box), (1, 2 - i, i, 2.0 - 0.3 * i, box)]
    rows += [(0, 3, 4, 1.2, cxcywh(40, 40, 60, 60)), (1, 3, 4, 1.1, cxcywh(50, 50, 50, 50))]
    logits, boxes = table(2, 4, 6, rows)

    def explicit(got, kept, dropped):
        assert got[0].tolist() == [8] and not dropped and finite(got)
        assert sorted(got[4][:8].tolist()) == [0] * 4 + [1] * 4
        assert got[3][0].tolist() == [8.0, 8.0, 8.0, 16.0] and got[3][2].tolist() == [36.0, 8.0, 30.0, 16.0]
    out = [Case(f"degenerate boxes {match}", logits, boxes, [(0, 0), (0, 0)], (64, 64), 0.5, match, 0.0,
                exact=("overlap",), explicit=explicit) for match in ("ios", "iou")]
    # the 2 x 2 table: a zero-area pair and a zero-area box inside a normal one
    small = [(0, 0, 1, 3.0, kinds[1][1]), (1, 0, 1, 2.0, kinds[1][1]), (0, 1, 4, 1.2, cxcywh(40, 40, 60, 60)),
             (1, 1, 4, 1.1, cxcywh(50, 50, 50, 50))]
    out += [Case(f"degenerate 2x2 {match}", *table(2, 2, 6, small), [(0, 0), (0, 0)], (64, 64), 0.5, match, 0.0,
                 exact=("overlap",), explicit=_count(4, [0, 1, 0, 1])) for match in ("ios", "iou")]
    return out


# ---- range ----------------------------------------------------------------------------------------------------------
RANGE_SEEDS = {"1e4": 0, "-inf": 1}
RANGE_ORIGINS = [(0, 0), (0, 30), (20, 0), (20, 30)]


def det_case(B, M, C, seed):
    g = torch.Generator().manual_seed(seed)
    return 3.0 * torch.randn(B, M, C, generator=g), 0.2 + 0.6 * torch.rand(B, M, 4, generator=g)


def midpoint(logits):
    """The threshold between the two middle fp64 scores."""
    s = torch.softmax(logits.double(), -1)[..., :-1].max(-1).values.flatten().sort().values
    n = s.numel()
    return 0.5 * (s[n // 2 - 1] + s[n // 2]).item()


def range_case(kind):
    """4 tiles of 25 rows, 12 classes (so that labels meet across tiles): logits of 1e4 scale, whose ``exp`` overflows
    without the max subtraction and whose scores are 0 or 1 (ties in row order), or 30 % of the entries ``-inf``, one
    row without "no object" and one with a single class left."""
    logits, boxes = det_case(4, 25, 12, RANGE_SEEDS[kind])
    if kind == "1e4":
        logits *= 1e4
        assert logits.abs().max().item() > 8e4
        thr = 0.5
    else:
        g = torch.Generator().manual_seed(RANGE_SEEDS[kind] + 1)
        logits[torch.rand(logits.shape, generator=g) < 0.3] = float("-inf")
        logits[:, 7, 11] = float("-inf")
        logits[:, 8, :11] = float("-inf")
        logits[:, 8, 6] = 1.0
        logits[:, 8, 11] = -5.0
        assert torch.isinf(logits).any(-1).sum().item() > 90 and not torch.isinf(logits).all(-1).any()
        thr = midpoint(logits)

    def explicit(got, kept, dropped):
        assert finite(got) and 0 < len(kept) < 100 and dropped
        if kind == "-inf":
            rows = {k[4]: i for i, k in enumerate(kept)}
            top = [rows[b * 25 + 8] for b in range(4) if b * 25 + 8 in rows]
            assert top and all(got[2][i].item() == 6 and got[1][i].item() > 0.99 for i in top)
    return Case(f"range {kind}", logits, boxes, RANGE_ORIGINS, (100, 100), thr, explicit=explicit)


NAN_ROW = (1, 4)


def nan_cases():
    """``(with a NaN, the same with that row "no object")``: the class-count table of 12 classes, in which row 4 of
    tile 1, rewritten to score 0.98 (the top of the list), holds a NaN among its logits. Such a row's score is NaN,
    no threshold is below it, it is never a candidate; nothing else changes."""
    logits, boxes = T.ramp(4, 25, classes=12, seed=0, hole=True)
    b, m = NAN_ROW
    clean = logits.clone()
    clean[b, m] = -4.0
    clean[b, m, -1] = 6.0
    logits[b, m] = -4.0
    logits[b, m, 3] = 5.0
    logits[b, m, -1] = 0.0
    loud = logits.clone()           # the row as it would be without the NaN: the top candidate
    logits[b, m, 5] = float("nan")

    def explicit(got, kept, dropped):
        assert finite(got) and all(k[4] != b * 25 + m for k in kept + dropped) and 0 < len(kept) < 50
    return (Case("nan row", logits, boxes, CLASS_ORIGINS, (100, 100), 0.3, explicit=explicit),
            Case("nan row as no object", clean, boxes, CLASS_ORIGINS, (100, 100), 0.3, explicit=explicit),
            Case("nan row without the nan", loud, boxes, CLASS_ORIGINS, (100, 100), 0.3))


# ---- origins --------------------------------------------------------------------------------------------------------
BIG_SEED = 0
BIG_ORIGINS = [(0, 0), (0, 1706), (960, 0), (2800, 4866), (3500, 6000), (4000, 7000)]
BIG_TILE = (1200, 2134)


def big_origins_case():
    """Six tiles of an 8K plan's size in a frame of 5200 x 9134: the boxes' ulp is at its coarsest, 2^-11 px."""
    logits, boxes = T.ramp(6, 40, seed=BIG_SEED, hole=True)

    def explicit(got, kept, dropped):
        assert dropped and max(k[2][2] for k in kept) > 8000.0
    return Case("origins up to (4000, 7000)", logits, boxes, BIG_ORIGINS, BIG_TILE, 0.3, explicit=explicit)


def same_origin_case():
    """Two tiles at one origin holding the same rows: each candidate of tile 0 is kept and drops its copy (an equal
    score at a higher row, overlap 1), and no row of tile 1 is ever kept to drop anything."""
    logits, boxes = T.ramp(1, 100, seed=0, hole=True)
    logits, boxes = torch.cat((logits, logits)), torch.cat((boxes, boxes))

    def explicit(got, kept, dropped):
        assert got[0].tolist() == [50] and not got[4].any() and len(dropped) == 50
        assert sorted(k[4] for k in kept) == sorted(d[4] - 100 for d in dropped)
    return Case("two tiles at one origin", logits, boxes, [(12, 34), (12, 34)], (100, 100), 0.3, explicit=explicit)


# ---- dirty buffers and graph replay ---------------------------------------------------------------------------------
def counted_case(B, M, n):
    """A table of ``N = B * M`` rows of which exactly ``n`` (0, 1, N - 1 or N) are kept: the ramp (scores 0.0185 to
    0.88) with one row raised to 0.9991 and one lowered to 0.0113 (a winning logit of -3.5 still leads the other
    classes' -4 by 0.004 of probability), nothing dropped (match threshold 1)."""
    N = B * M
    logits, boxes = T.ramp(B, M, seed=1)
    flat = logits.view(N, -1)
    flat[N // 3, flat[N // 3, :-1].argmax()] = 8.0
    flat[(2 * N) // 3, flat[(2 * N) // 3, :-1].argmax()] = -3.5
    thr = {0: 1.0, 1: 0.95, N - 1: 0.015, N: 0.0}[n]
    return Case(f"counted {B}x{M} keeps {n}", logits, boxes, row_origins(B), (100, 100), thr, "ios", 1.0,
                explicit=_count(n))


COUNTED = tuple((B, M, n) for B, M in ((5, 13), (4, 256)) for n in (0, 1, B * M - 1, B * M))


def shrinking_cases():
    """Three tables of one shape (4 x 64 x 92) that keep many rows, few and none."""
    many = Case("replay many", *T.ramp(4, 64, seed=0, hole=True), row_origins(4), (100, 100), 0.3)
    rows = [(0, 5, 3, 2.0, (0.3, 0.3, 0.2, 0.2)), (2, 60, 3, 1.0, (0.3, 0.3, 0.2, 0.2)),
            (3, 1, 9, 3.0, (0.5, 0.5, 0.1, 0.1))]
    few = Case("replay few", *table(4, 64, 92, rows), row_origins(4), (100, 100), 0.3, explicit=_count(3, [3, 0, 2]))
    none = Case("replay none", *table(4, 64, 92, []), row_origins(4), (100, 100), 0.3, explicit=_count(0))
    return many, few, none


def loop_cases():
    """Every case that is compared with the double loop, by name (built on demand: the 1024-row tables take a
    second each in the loop)."""
    out = {}
    for key in ROW_SEEDS:
        out[f"rows {key[0]}x{key[1]} {key[2]}"] = lambda key=key: rows_case(*key)
    out["rows 4x256 all kept"] = rows_full_case
    for C in CLASS_SEEDS:
        out[f"classes C={C}"] = lambda C=C: class_case(C)
        out[f"classes C={C} every row"] = lambda C=C: class_case(C, True)
    out["pivot drops the last"] = pivot_last_case
    out["tie block of 64"] = tie_block_case
    out["tie pair overlapping"] = tie_pair_case
    out["ten identical boxes in one tile"] = same_tile_case
    out["identical boxes, other labels"] = other_label_case
    for kind in RANGE_SEEDS:
        out[f"range {kind}"] = lambda kind=kind: range_case(kind)
    out["origins up to (4000, 7000)"] = big_origins_case
    out["two tiles at one origin"] = same_origin_case
    for i in range(3):
        out[("pivot one candidate", "pivot two duplicates", "pivot two in one tile")[i]] = lambda i=i: pivot_cases()[i]
    for i, c in enumerate(strict_match_cases()):
        out[c.name] = lambda i=i: strict_match_cases()[i]
    for i, c in enumerate(strict_score_cases()):
        out[c.name] = lambda i=i: strict_score_cases()[i]
    for i, c in enumerate(degenerate_cases()):
        out[c.name] = lambda i=i: degenerate_cases()[i]
    for i, c in enumerate(nan_cases()):
        out[c.name] = lambda i=i: nan_cases()[i]
    for key in COUNTED:
        out[counted_case(*key).name] = lambda key=key: counted_case(*key)
    for i, c in enumerate(shrinking_cases()):
        out[c.name] = lambda i=i: shrinking_cases()[i]
    return out
