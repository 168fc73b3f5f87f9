"""Detections associated across frames, on the CPU: ``ops.image.track_update_reference`` (what runs off the GPU, with
the ``torch`` backend, for other dtypes and past 1024 rows or slots) held to the fp64 loop of ``tests/track_case.py`` on
every case the GPU tests run, with the guard recomputed here for each of them; the ``ValueError``s; ``Tracker``;
``YolosProcessor.tracked_results``; ``YolosSmall.track_image`` on the CPU route; the pod client's flag checks."""
import pytest
import torch

import track_case as C
from walkai_nos_amd.models.workload.processor import YolosProcessor
from walkai_nos_amd.models.workload.tracker import Tracker
from walkai_nos_amd.ops import image as I

CASES = C.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_reference_is_the_loop(case):
    print(C.run_case(I, case, I.track_update_reference))


def test_every_seed_in_the_tables_passes_the_guard():
    assert len(C.RANDOM_SEEDS) >= 4 and len({c.name for c in CASES}) == len(CASES)
    for case in CASES:
        C.guard(case)       # raises where a margin is short; nothing is skipped


def test_off_the_gpu_track_update_is_the_reference(monkeypatch):
    calls = []
    ref = I.track_update_reference
    monkeypatch.setattr(I, "track_update_reference", lambda *a, **kw: calls.append(1) or ref(*a, **kw))
    print(C.run_case(I, C.random_case(C.RANDOM_SEEDS[1]), I.track_update))
    assert len(calls) == len(C.random_case(C.RANDOM_SEEDS[1]).frames)


def test_views_of_one_image_and_other_dtypes():
    # [1, M] views as detections returns them, fp64 lists and int64 labels: the same ids as the flat fp32 lists
    case = C.random_case(C.RANDOM_SEEDS[2])
    a, b = I.track_state(case.T), I.track_state(case.T)
    for f in case.frames:
        count, scores, labels, boxes = f.lists()
        flat = I.track_update(a, count, scores, labels, boxes, **case.kwargs())
        wide = I.track_update(b, count.long(), scores[None].double(), labels[None].long(), boxes[None].double(),
                              **case.kwargs())
        assert all(torch.equal(x, y) for x, y in zip(flat, wide))
    assert all(torch.equal(x, y) for x, y in zip(a.tensors(), b.tensors()))


def test_no_rows():
    s = I.track_state(4)
    ids, hits = I.track_update(s, torch.zeros(1, dtype=torch.int32), torch.zeros(0), torch.zeros(0, dtype=torch.int32),
                               torch.zeros(0, 4))
    assert ids.shape == (0,) and hits.shape == (0,) and s.next_id.tolist() == [1] and not s.ids.any()


def test_state_layout_and_reset():
    s = I.track_state(5)
    assert s.capacity == 5 and s.boxes.shape == (5, 4) and s.vel.shape == (5, 4)
    assert s.boxes.dtype == s.vel.dtype == torch.float32
    for t in (s.labels, s.ids, s.hits, s.misses):
        assert t.shape == (5,) and t.dtype == torch.int32 and not t.any()
    assert s.next_id.tolist() == [1] and s.dropped.tolist() == [0] and s.next_id.dtype == torch.int32
    f = C.full_case().frames[0]
    I.track_update(s, *f.lists())
    I.track_update(I.track_state(3), *f.lists())
    assert s.ids.tolist() == [1, 2, 3, 4, 5] and s.next_id.tolist() == [6]
    s.reset()
    assert s.next_id.tolist() == [1] and all(not t.any() for t in s.tensors()[:6]) and s.dropped.tolist() == [0]
    assert I.MOTIONS == {"none": 0, "constant": 1}
    with pytest.raises(ValueError, match="capacity"):
        I.track_state(0)


@pytest.mark.parametrize("kw,word", [(dict(motion="kalman"), "motion"), (dict(match_threshold=-0.1), "match_threshold"),
                                     (dict(match_threshold=float("nan")), "match_threshold"),
                                     (dict(max_age=-1), "max_age"), (dict(velocity_gain=1.5), "velocity_gain"),
                                     (dict(velocity_gain=-0.1), "velocity_gain"),
                                     (dict(velocity_gain=float("nan")), "velocity_gain")])
def test_parameters_are_checked(kw, word):
    f = C.full_case().frames[0]
    for update in (I.track_update, I.track_update_reference):
        s = I.track_state(4)
        with pytest.raises(ValueError, match=word):
            update(s, *f.lists(), **kw)
        assert s.next_id.tolist() == [1] and not s.ids.any()
    with pytest.raises(ValueError, match=word):
        Tracker(**kw)


def test_lists_are_checked():
    s = I.track_state(4)
    count, scores, labels, boxes = C.full_case().frames[0].lists()
    with pytest.raises(ValueError, match="labels"):
        I.track_update(s, count, scores, labels[:4], boxes)
    with pytest.raises(ValueError, match="boxes"):
        I.track_update(s, count, scores, labels, boxes[:3])
    with pytest.raises(ValueError, match="boxes"):
        I.track_update(s, count, scores, labels, boxes[:, :3])
    with pytest.raises(ValueError, match="count"):
        I.track_update(s, torch.zeros(2, dtype=torch.int32), scores, labels, boxes)
    with pytest.raises(ValueError, match="scores"):
        I.track_update(s, count, scores.reshape(5, 1).expand(5, 2), labels, boxes)
    with pytest.raises(ValueError, match="state is on"):
        I.track_update(s, count.to("meta"), scores, labels, boxes)
    assert s.next_id.tolist() == [1]


# ---- Tracker ----------------------------------------------------------------------------------------------------------
def det_of(f):
    count, scores, labels, boxes = f.lists()
    return {"count": count, "scores": scores, "labels": labels, "boxes": boxes, "other": "kept"}


def test_tracker_update_reset_and_tracks():
    case = C.coasting_cases()[0]
    outs, snaps, _ = C.guard(case)
    tr = Tracker(capacity=case.T, **case.kwargs())
    assert tr.capacity == case.T and tr.tracks() == []
    for f, out in zip(case.frames, outs):
        det = tr.update(det_of(f))
        assert det["other"] == "kept" and torch.equal(det["scores"], f.scores[:f.N])
        assert det["track_id"].tolist() == out[0] and det["track_hits"].tolist() == out[1]
    assert tr.tracks() == [{"id": 1, "label": 1, "box": (150.0, 100.0, 250.0, 200.0), "hits": 4, "misses": 0}]
    tr.reset()
    assert tr.tracks() == [] and tr.state.next_id.tolist() == [1]
    # [1, M] lists, as detect_image returns them: the outputs take their shape
    f = C.full_case().frames[0]
    det = det_of(f)
    det.update(scores=det["scores"][None], labels=det["labels"][None], boxes=det["boxes"][None])
    got = Tracker(capacity=3).update(det)
    assert got["track_id"].shape == (1, 5) and got["track_id"].tolist() == [[0, 1, 0, 2, 3]]
    two = {**det, "scores": det["scores"].expand(2, 5)}
    with pytest.raises(ValueError, match="batch"):
        Tracker().update(two)
    with pytest.raises(ValueError, match="min_hits"):
        Tracker(min_hits=0)


def test_tracks_are_listed_by_id():
    tr = Tracker(capacity=2, max_age=0)
    case = C.slot_reuse_case()
    for f in case.frames:
        tr.update(det_of(f))
    assert [(t["id"], t["hits"]) for t in tr.tracks()] == [(2, 2), (3, 1)]       # slot 0 holds id 3


def test_tracked_results_and_min_hits():
    f = C.full_case().frames[0]
    tr = Tracker(capacity=3)
    det = tr.update(det_of(f))
    args = [det[k] for k in ("count", "scores", "labels", "boxes", "track_id", "track_hits")]
    res = YolosProcessor.tracked_results(*args)
    assert len(res) == 1 and res[0]["ids"].tolist() == [1, 2, 3] and res[0]["hits"].tolist() == [1, 1, 1]
    assert torch.equal(res[0]["scores"], f.scores[[1, 3, 4]]) and torch.equal(res[0]["boxes"], f.boxes[[1, 3, 4]])
    assert res[0]["labels"].dtype == torch.int64 and res[0]["ids"].dtype == torch.int64
    assert YolosProcessor.tracked_results(*args, min_hits=2)[0]["ids"].tolist() == []
    det = tr.update(det_of(f))
    args = [det[k] for k in ("count", "scores", "labels", "boxes", "track_id", "track_hits")]
    assert YolosProcessor.tracked_results(*args, min_hits=2)[0]["ids"].tolist() == [1, 2, 3]
    assert YolosProcessor.tracked_results(*args, min_hits=3)[0]["ids"].tolist() == []
    # [1, M] lists and a count below the tracked rows
    wide = [args[0].new_tensor([4])] + [a[None] for a in args[1:]]
    assert YolosProcessor.tracked_results(*wide)[0]["ids"].tolist() == [1, 2]


# ---- the model ----------------------------------------------------------------------------------------------------------
def small_model():
    from yolos_reference import randomize
    from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=2, use_mid_position_embeddings=True)).eval()
    randomize(m)
    m.invalidate_cache()
    m.processor = YolosProcessor(80, 133)
    return m


def test_track_image_keeps_its_ids_on_an_unchanged_frame():
    m = small_model()
    g = torch.Generator().manual_seed(11)
    frame = torch.randint(0, 256, (97, 131, 3), generator=g, dtype=torch.uint8)
    with torch.no_grad():
        s = m.detect_image(frame, 0.0)["scores"][0].sort().values
        thr = 0.5 * (s[-13] + s[-12]).item()
        tr = Tracker(capacity=32)
        plain = m.detect_image(frame, thr)
        seen = [m.track_image(frame, tr, thr) for _ in range(3)]
    n = plain["count"].item()
    assert n == 12
    for k, out in enumerate(seen):
        for key in ("logits", "pred_boxes", "count", "scores", "labels", "boxes"):
            assert torch.equal(out[key], plain[key]), key
        assert out["track_id"].shape == (1, 100) and out["track_id"].dtype == torch.int32
        assert torch.equal(out["track_id"], seen[0]["track_id"])
        assert sorted(out["track_id"][0, :n].tolist()) == list(range(1, n + 1)) and not out["track_id"][0, n:].any()
        assert out["track_hits"][0, :n].tolist() == [k + 1] * n and not out["track_hits"][0, n:].any()
    assert tr.state.next_id.tolist() == [n + 1] and [t["hits"] for t in tr.tracks()] == [3] * n
    res = m.processor.tracked_results(*(seen[2][k] for k in ("count", "scores", "labels", "boxes", "track_id",
                                                            "track_hits")), min_hits=3)
    assert res[0]["ids"].shape == (n,)
    with torch.no_grad():
        tiled = m.track_tiled(frame, Tracker(capacity=64), (2, 1), 0.3, thr)
    c = tiled["count"].item()
    assert tiled["track_id"].shape == (200,) and c > 0
    assert sorted(tiled["track_id"][:c].tolist()) == list(range(1, min(c, 64) + 1)) + [0] * max(c - 64, 0)


# ---- the pod client's flags -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,word", [(["--track"], "--end-to-end"),
                                       (["--end-to-end", "--track", "--track-iou", "-0.5"], "--track-iou"),
                                       (["--end-to-end", "--track", "--track-max-age", "-1"], "--track-max-age"),
                                       (["--end-to-end", "--track", "--track-min-hits", "0"], "--track-min-hits"),
                                       (["--end-to-end", "--track", "--track-capacity", "1025"], "--track-capacity"),
                                       (["--end-to-end", "--track", "--track-capacity", "0"], "--track-capacity")])
def test_client_checks_the_track_flags(capsys, argv, word):
    from walkai_nos_amd.dataplane import client
    with pytest.raises(SystemExit) as e:
        client.main(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err
