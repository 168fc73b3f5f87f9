"""The cross-tile merge kernel (``merge_detections_f32``, ``csrc/image_detect.h``) at its edges. The conventions are
``tests/test_gpu_tiles.py``'s: the yardstick is the fp64 double loop of ``tests/tiles_case.py`` (``merge_loop``
through ``check_merged``): count, labels, tiles and order equal, scores within 1e-5, boxes within ``box_tol`` of the
frame, zeros behind the count, on inputs the loop decides clearly (``merge_edges_case.guard``; the margins a case sets
by hand to an exact tie come with the outcome spelled out). Every comparison asserts that the torch reference was not
called, so a silent fall-back cannot pass. The cases are ``tests/merge_edges_case.py``'s, the ones the torch reference
is held to on the CPU (``tests/test_merge_edges.py``).

What each group pins:

* row counts around a wave and at the 1024-row limit, split over 1 to 1024 tiles (``tid / M``, the origin table);
* class counts around the two 64-lane halves of ``row_best``, and one label only, so that every cross-tile pair meets;
* the pivot loop's ends: no, one and two candidates, and the second-to-last candidate dropping the last;
* the strict ``>`` of the match threshold and of the score threshold on values exact in fp32 and fp64;
* ties: a block of 64 equal scores across four tiles in row order, the lower row surviving an equal-score duplicate;
* what must not suppress: one tile's own boxes, other labels; one tile is ``detections`` stably sorted, bit for bit;
* boxes of no or negative extent (``box_overlap``'s ``den > 0``), logits of 1e4, ``-inf`` and NaN;
* origins of an 8K frame, two tiles at one origin, the origins as a device tensor;
* the zero-fill behind ``count`` into buffers full of 0x7F, and a captured graph replayed on ever fewer survivors.

One ``[merge]`` line per comparison; the run on the MI355X is kept in ``profiles/pytest_gpu_merge_edges.log``."""
import pytest
import torch

import merge_edges_case as E
import tiles_case as T

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-5


def box_tol(frame_hw):
    return max(5 * 2.0 ** -24 * max(frame_hw), 1e-3)


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


def run_merge(I, logits, boxes, origins, tile_hw, thr, match, mt):
    got = I.merge_detections(logits.cuda(), boxes.cuda(), origins, tile_hw, thr, match, mt)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in got)


def compare(I, monkeypatch, case):
    """The kernel on ``case`` against the double loop; ``(got, kept, dropped)``."""
    kept, margins, dropped = E.guard(case)
    ref = Counter(monkeypatch, I, "merge_detections_reference")
    got = run_merge(I, case.logits, case.boxes, *case.args())
    assert ref.n == 0
    tol = box_tol(case.frame_hw)
    head = f"[merge] {case.name}: count {got[0].tolist()} (loop {len(kept)} kept, {len(dropped)} dropped)"
    try:
        ds, db = T.check_merged(got, kept, case.N, SCORE_TOL, tol)
    except AssertionError:
        print(f"{head}; margins {tuple(f'{m:.3g}' for m in margins)}")
        raise
    print(f"{head}, max |d score| {ds:.3g} (bound {SCORE_TOL:g}), max |d box| {db:.3g} px (bound {tol:.3g}); "
          f"margins {tuple(f'{m:.3g}' for m in margins)}")
    assert E.finite(got)
    if case.explicit is not None:
        case.explicit(got, kept, dropped)
    return got, kept, dropped


# ---- rows and splits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,match", list(E.ROW_SEEDS), ids=[f"{b}x{m}-{t}" for b, m, t in E.ROW_SEEDS])
def test_merge_rows_and_splits(K, I, monkeypatch, B, M, match):
    compare(I, monkeypatch, E.rows_case(B, M, match))
    if (B, M, match) == (4, 256, "ios"):
        got, _, _ = compare(I, monkeypatch, E.rows_full_case())     # all 1024 kept: nothing is zero-filled
        assert bool((got[1][:-1] >= got[1][1:]).all())


# ---- class counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", sorted(E.CLASS_SEEDS))
def test_merge_class_counts(K, I, monkeypatch, C):
    compare(I, monkeypatch, E.class_case(C))
    compare(I, monkeypatch, E.class_case(C, every=True))


# ---- the ends of the pivot loop -------------------------------------------------------------------------------------
def test_merge_no_one_and_two_candidates(K, I, monkeypatch):
    for case in E.pivot_cases():
        compare(I, monkeypatch, case)
    none = E.pivot_cases()[0]
    none.name, none.thr, none.explicit = "pivot no candidate", 1.0, None
    got, kept, _ = compare(I, monkeypatch, none)
    assert not kept and got[0].tolist() == [0]


def test_merge_second_to_last_candidate_drops_the_last(K, I, monkeypatch):
    compare(I, monkeypatch, E.pivot_last_case())


# ---- strictness and ties --------------------------------------------------------------------------------------------
def test_merge_match_threshold_is_strict(K, I, monkeypatch):
    for case in E.strict_match_cases():       # ios and iou, at 0.5 (3 kept) and just below (2 kept)
        compare(I, monkeypatch, case)


def test_merge_score_threshold_is_strict(K, I, monkeypatch):
    for case in E.strict_score_cases():
        compare(I, monkeypatch, case)


def test_merge_block_of_equal_scores_keeps_row_order(K, I, monkeypatch):
    compare(I, monkeypatch, E.tie_block_case())


def test_merge_equal_scores_the_lower_row_survives(K, I, monkeypatch):
    compare(I, monkeypatch, E.tie_pair_case())


# ---- what must not suppress -----------------------------------------------------------------------------------------
def test_merge_one_tile_and_other_labels_do_not_suppress(K, I, monkeypatch):
    compare(I, monkeypatch, E.same_tile_case())
    compare(I, monkeypatch, E.other_label_case())


def test_merge_of_one_tile_is_detections_sorted(K, I, monkeypatch):
    logits, boxes, hw, thr = E.one_tile_inputs()
    refs = [Counter(monkeypatch, I, "merge_detections_reference"), Counter(monkeypatch, I, "detections_reference")]
    lg, bx = logits.cuda(), boxes.cuda()
    count, scores, labels, xyxy = I.detections(lg, bx, [hw], thr)
    got = I.merge_detections(lg, bx, [(0, 0)], hw, thr)
    torch.cuda.synchronize()
    assert refs[0].n == 0 and refs[1].n == 0
    n = count.item()
    order = torch.sort(-scores[0, :n], stable=True).indices
    assert 2 < n < 100 and got[0].tolist() == [n] and not got[4].any()
    assert torch.equal(got[1][:n], scores[0, :n][order]) and torch.equal(got[2][:n], labels[0, :n][order])
    assert torch.equal(got[3][:n], xyxy[0, :n][order])
    assert not got[1][n:].any() and not got[2][n:].any() and not got[3][n:].any()
    tied = (got[1][:n - 1] == got[1][1:n]).sum().item()
    print(f"[merge] one tile of 100 rows: {n} kept, bit-equal to detections' survivors stably sorted; {tied} tie")
    assert tied == 1


# ---- degenerate boxes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", ("ios", "iou"))
def test_merge_degenerate_boxes_overlap_nothing(K, I, monkeypatch, match):
    for case in E.degenerate_cases():
        if case.match == match:
            compare(I, monkeypatch, case)


# ---- range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(E.RANGE_SEEDS))
def test_merge_range(K, I, monkeypatch, kind):
    compare(I, monkeypatch, E.range_case(kind))


def test_merge_ignores_a_nan_row(K, I, monkeypatch):
    loud, clean, without = E.nan_cases()
    a, _, _ = compare(I, monkeypatch, loud)
    b, _, _ = compare(I, monkeypatch, clean)
    c, _, _ = compare(I, monkeypatch, without)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and E.finite(a)
    assert c[0].item() == a[0].item() + 1 and c[4][0].item() == E.NAN_ROW[0]        # without the NaN it leads the list


# ---- origins --------------------------------------------------------------------------------------------------------
def test_merge_origins_of_an_8k_frame(K, I, monkeypatch):
    case = E.big_origins_case()
    assert case.frame_hw == (5200, 9134) and box_tol(case.frame_hw) > 2e-3
    listed, _, _ = compare(I, monkeypatch, case)
    org = torch.tensor(case.origins, dtype=torch.int32).cuda()
    ref = Counter(monkeypatch, I, "merge_detections_reference")
    tensor = run_merge(I, case.logits, case.boxes, org, case.tile_hw, case.thr, case.match, case.mt)
    assert ref.n == 0 and all(torch.equal(x, y) for x, y in zip(listed, tensor))


def test_merge_two_tiles_at_one_origin(K, I, monkeypatch):
    compare(I, monkeypatch, E.same_origin_case())


# ---- the zero-fill behind the count ---------------------------------------------------------------------------------
PAD = 64        # bytes behind every output that must stay as they were


@pytest.mark.parametrize("B,M,n", E.COUNTED, ids=[f"{b}x{m}-keeps{n}" for b, m, n in E.COUNTED])
def test_merge_zero_fills_dirty_buffers(K, I, monkeypatch, B, M, n):
    case = E.counted_case(B, M, n)
    want, _, _ = compare(I, monkeypatch, case)             # the wrapper's result, itself held to the loop
    N = case.N
    lg, bx = case.logits.cuda(), case.boxes.cuda()
    org = I.origin_tensor(case.origins, lg.device)
    raw = [torch.full((nbytes + PAD,), 0x7F, dtype=torch.uint8, device="cuda")
           for nbytes in (4, 4 * N, 4 * N, 16 * N, 4 * N)]
    rc = I._L().nos_merge_detections_f32(lg.data_ptr(), bx.data_ptr(), org.data_ptr(), float(case.tile_hw[0]),
                                         float(case.tile_hw[1]), case.thr, case.mt, I.MATCHES[case.match], B, M,
                                         lg.shape[2], *(t.data_ptr() for t in raw),
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert all(bool((t[-PAD:] == 0x7F).all()) for t in raw)
    count, scores, labels, xyxy, tile = (t[:-PAD].view(d).cpu() for t, d in zip(
        raw, (torch.int32, torch.float32, torch.int32, torch.float32, torch.int32)))
    got = (count, scores, labels, xyxy.view(N, 4), tile)
    assert count.tolist() == [n]
    assert not scores[n:].any() and not labels[n:].any() and not got[3][n:].any() and not tile[n:].any()
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    print(f"[merge] {case.name}: into buffers of 0x7F, {N - n} slots zeroed in each array, the {n} before them equal "
          f"to the wrapper's")


# ---- a captured graph on ever fewer survivors -----------------------------------------------------------------------
def test_merge_graph_replay_that_shrinks(K, I, monkeypatch):
    cases = E.shrinking_cases()
    eager = [compare(I, monkeypatch, c)[0] for c in cases]
    counts = [e[0].item() for e in eager]
    assert counts[0] > 100 and counts[1:] == [3, 0]
    many = cases[0]
    lg, bx = many.logits.cuda(), many.boxes.cuda()
    ref = Counter(monkeypatch, I, "merge_detections_reference")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        held = I.merge_detections(lg, bx, *many.args())
    for t in held:
        t.fill_(-7)
    for case, want in list(zip(cases, eager)) + [(many, eager[0])]:
        assert case.args() == many.args()
        lg.copy_(case.logits)
        bx.copy_(case.boxes)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for name, h, w in zip(("count", "scores", "labels", "boxes", "tile"), held, want):
            assert torch.equal(h.cpu(), w), (case.name, name)
    assert ref.n == 0
    print(f"[merge] one graph replayed on tables that keep {counts + counts[:1]}: every output equal to the eager run")
    del graph
