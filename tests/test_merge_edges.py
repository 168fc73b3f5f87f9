"""The cross-tile merge at its edges, on the CPU: every case of ``tests/merge_edges_case.py`` through the torch
reference ``merge_detections_reference`` (in fp32 and in fp64) against the fp64 double loop of ``tests/tiles_case.py``,
so that the reference is held to the same edges as the kernel (``tests/test_gpu_merge_edges.py``), and the guard on
every seeded table recomputed on the double loop alone."""
import pytest
import torch

import merge_edges_case as E
import tiles_case as T
from walkai_nos_amd.ops import image as I

CASES = E.loop_cases()


def box_tol(frame_hw):
    return max(5 * 2.0 ** -24 * max(frame_hw), 1e-3)


def reference(case, dtype):
    return I.merge_detections_reference(case.logits.to(dtype), case.boxes.to(dtype), *case.args())


@pytest.mark.parametrize("name", list(CASES))
def test_merge_reference_at_the_edges(name):
    case = CASES[name]()
    assert case.name == name
    kept, margins, dropped = E.guard(case)
    for dtype, score_tol, tol in ((torch.float64, 1e-12, 1e-8), (torch.float32, 1e-5, box_tol(case.frame_hw))):
        got = reference(case, dtype)
        assert got[1].dtype == dtype and got[3].dtype == dtype
        T.check_merged(got, kept, case.N, score_tol, tol)
        assert E.finite(got)
        if case.explicit is not None:
            case.explicit(got, kept, dropped)


def test_merge_seeds_pass_the_guard_on_the_reference_alone():
    # every seeded table, built anew and run through the double loop alone: the margins by which it decides
    seeded = [lambda key=key: E.rows_case(*key) for key in E.ROW_SEEDS] + [E.rows_full_case, E.pivot_last_case]
    seeded += [lambda C=C, e=e: E.class_case(C, e) for C in E.CLASS_SEEDS for e in (False, True)]
    seeded += [lambda kind=kind: E.range_case(kind) for kind in E.RANGE_SEEDS]
    seeded += [E.big_origins_case, E.same_origin_case, lambda: E.nan_cases()[1], lambda: E.shrinking_cases()[0]]
    seeded += [lambda key=key: E.counted_case(*key) for key in E.COUNTED]
    for make in seeded:
        case = make()
        dropped = []
        kept, margins = T.merge_loop(case.logits, case.boxes, *case.args(), dropped)
        assert not case.exact, case.name
        if case.mt == 1.0:          # nothing compares above 1 (``merge_edges_case.guard``): the case only sorts
            assert not dropped, case.name
            margins = margins[:3] + (float("inf"),)
        T.decides_clearly(margins, case.thr)
        assert E.solve(case)[0] == kept, case.name
    for (B, M, match), (_, want) in E.ROW_SEEDS.items():
        assert len(E.solve(E.rows_case(B, M, match))[0]) == want, (B, M, match)
    assert [len(E.solve(E.rows_case(B, M))[0]) for B, M in E.ROW_SHAPES] == [1, 32, 30, 32, 31, 296, 292, 327, 512]


def test_merge_reference_ignores_a_nan_row():
    loud, clean, without = E.nan_cases()
    for dtype in (torch.float32, torch.float64):
        a, b, c = reference(loud, dtype), reference(clean, dtype), reference(without, dtype)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and E.finite(a)
        assert c[0].item() == a[0].item() + 1 and c[4][0].item() == E.NAN_ROW[0]    # without the NaN it leads the list
    # ``detections`` zero-fills behind its count in the same way
    count, scores, labels, xyxy = I.detections_reference(loud.logits, loud.boxes, torch.ones(4, 2), 0.3)
    assert E.finite((scores, xyxy)) and count.tolist() == I.detections_reference(clean.logits, clean.boxes,
                                                                                  torch.ones(4, 2), 0.3)[0].tolist()


def test_merge_reference_of_one_tile_is_detections_sorted():
    logits, boxes, hw, thr = E.one_tile_inputs()
    count, scores, labels, xyxy = I.detections_reference(logits, boxes, torch.tensor([hw], dtype=torch.float32), thr)
    n = count.item()
    order = torch.sort(-scores[0, :n], stable=True).indices
    got = I.merge_detections_reference(logits, boxes, [(0, 0)], hw, thr)
    assert 2 < n < 100 and got[0].tolist() == [n] and not got[4].any()
    assert torch.equal(got[1][:n], scores[0, :n][order]) and torch.equal(got[2][:n], labels[0, :n][order])
    assert torch.equal(got[3][:n], xyxy[0, :n][order])
    assert not got[1][n:].any() and not got[2][n:].any() and not got[3][n:].any()


def test_merge_reference_origin_forms():
    case = E.big_origins_case()
    listed = reference(case, torch.float32)
    tensor = I.merge_detections_reference(case.logits, case.boxes, torch.tensor(case.origins, dtype=torch.int32),
                                          case.tile_hw, case.thr, case.match, case.mt)
    assert all(torch.equal(a, b) for a, b in zip(listed, tensor))
