"""Stable ids for the detections of a video stream: :class:`Tracker` holds the device state of
``ops.image.track_update`` (a greedy IoU tracker with an optional constant-velocity prediction, one launch per frame)
and its parameters, and adds ``track_id`` and ``track_hits`` to what ``YolosSmall.detect_image`` or ``detect_tiled``
return. Nothing here synchronises with the host except :meth:`Tracker.tracks`, so ``YolosSmall.track_image`` and
``track_tiled`` capture as one graph whose replays advance the tracker: each replay is the next frame.

With an :class:`Appearance` the tracker also looks at the pictures: before it associates a frame's detections it cuts
their chips out of the frame (``ops.image.chips``), describes each by a striped colour histogram
(``ops.image.chip_features``) and compares them with the descriptors its tracks keep (``ops.image.feature_overlap``),
so that two boxes of one label that cross keep their ids (``gate``) and a track that was hidden for some frames is
found again away from where it coasted to (``reid_threshold``) — five launches more in the same graph.

Kalman filtering, learned embeddings, galleries of more than one descriptor a track, Hungarian assignment, a second
association pass on low scores, more than 1024 tracks and tracks across a batch of images are not offered."""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Tuple

from ...ops import image as I
from .chips import Chips


class Appearance:
    def __init__(self, size: Tuple[int, int] = (128, 64), labels: Optional[Iterable[int]] = None, capacity: int = 256,
                 margin: int = 0, stripes: int = 4, gate: float = 0.0, reid_threshold: Optional[float] = 0.6,
                 shift: int = 2, num_labels: int = 91):
        """What a :class:`Tracker` knows of its tracks' looks. ``size``, ``labels``, ``capacity``, ``margin``: the
        tracker's own chips, as ``chips.Chips`` takes them (a detection beyond ``capacity`` or of another label is
        associated by IoU alone). ``stripes``: 1, 2, 4 or 8 horizontal stripes of 64 colour bins. ``gate``: the
        fraction of a descriptor a detection must share with a track to continue it by overlap (0: no gate).
        ``reid_threshold``: the fraction at which a track that missed a frame is continued without any overlap
        (``None``: never). ``shift``: a matched track's descriptor moves ``2^-shift`` of the way to the new one."""
        self.chips = Chips(size, labels, capacity, margin, 1, num_labels)
        if stripes not in I.FEATURE_STRIPES or stripes > self.chips.size[0]:
            raise ValueError(f"Appearance: stripes {stripes!r} is none of {I.FEATURE_STRIPES} up to the chip's rows")
        if not 0.0 <= float(gate) <= 1.0 or (reid_threshold is not None and not 0.0 <= float(reid_threshold) <= 1.0):
            raise ValueError(f"Appearance: gate {gate!r} and reid_threshold {reid_threshold!r} are fractions in [0, 1]")
        if not 0 <= int(shift) <= I.FEATURE_MAX_SHIFT:
            raise ValueError(f"Appearance: shift {shift!r} is not in 0..{I.FEATURE_MAX_SHIFT}")
        self.stripes, self.length = int(stripes), I.FEATURE_BINS * int(stripes)
        self.params = dict(appearance_gate=float(gate), feature_shift=int(shift),
                           reid_threshold=None if reid_threshold is None else float(reid_threshold),
                           feature_total=I.feature_total(self.chips.size))

    def describe(self, det: Dict[str, object], frame) -> Tuple[object, object]:
        """``(features, rows)`` of the detections ``det`` in ``frame``: the chips cut without ids, then described."""
        plain = {k: v for k, v in det.items() if k not in ("track_id", "track_hits")}
        cut = self.chips.cut(plain, frame)
        return I.chip_features(cut["chips"], cut["chip_rows"], cut["chip_count"], self.stripes), cut["chip_rows"]


class Tracker:
    def __init__(self, capacity: int = 256, match_threshold: float = 0.3, max_age: int = 30,
                 birth_threshold: float = 0.0, motion: str = "constant", velocity_gain: float = 0.5, min_hits: int = 1,
                 device=None, appearance: Optional[Appearance] = None):
        """``capacity`` slots (1..1024 run as one HIP launch); a detection continues the track of its label whose
        predicted box it overlaps by an IoU above ``match_threshold``; a track unmatched for more than ``max_age``
        frames is dropped; unmatched detections with a score above ``birth_threshold`` start tracks; ``motion`` is
        ``"constant"`` (velocity, smoothed by ``velocity_gain``) or ``"none"``. ``min_hits`` is what
        ``YolosProcessor.tracked_results`` is meant to be given: tracks seen in fewer frames are not reported.
        ``appearance``: an :class:`Appearance`; :meth:`update` then takes the frame."""
        if not int(min_hits) >= 1:
            raise ValueError(f"Tracker: min_hits {min_hits!r} is not a number of frames from 1 up")
        I.track_params_check(float(match_threshold), int(max_age), motion, float(velocity_gain))
        self.appearance = appearance
        self.state = I.track_state(capacity, device, None if appearance is None else appearance.length)
        self.params = dict(match_threshold=float(match_threshold), max_age=int(max_age),
                           birth_threshold=float(birth_threshold), motion=motion, velocity_gain=float(velocity_gain))
        self.min_hits = int(min_hits)

    @property
    def capacity(self) -> int:
        return self.state.capacity

    def reset(self) -> None:
        """Forget every track and start the ids at 1 again (on the current stream, no synchronisation)."""
        self.state.reset()

    def update(self, det: Dict[str, object], frame=None) -> Dict[str, object]:
        """``det`` — the dict of ``detect_image`` (one image) or ``detect_tiled`` — with ``track_id`` and
        ``track_hits`` added, shaped like its ``labels``: the id of each row's track and the frames that track has
        been seen in, 0 for a row without one (behind ``count``, or a birth the full tracker refused). ``frame``: with
        an :class:`Appearance`, the frame whose pixels the boxes are in."""
        scores, labels = det["scores"], det["labels"]
        if scores.dim() == 2 and scores.shape[0] != 1:
            raise ValueError(f"Tracker: one image's detections, not a batch of {scores.shape[0]}")
        looks = {}
        if self.appearance is not None:
            if frame is None:
                raise ValueError("Tracker: a tracker with an Appearance takes the frame the detections were found in")
            features, rows = self.appearance.describe(det, frame)
            looks = dict(features=features, feature_rows=rows, **self.appearance.params)
        track_id, track_hits = I.track_update(self.state, det["count"], scores, labels, det["boxes"], **self.params,
                                              **looks)
        return {**det, "track_id": track_id.view(labels.shape), "track_hits": track_hits.view(labels.shape)}

    def tracks(self) -> List[Dict[str, object]]:
        """The live tracks on the host, by id: ``{"id", "label", "box" (x0, y0, x1, y1), "hits", "misses"}``. This is
        the one method that synchronises."""
        s = self.state
        ids = s.ids.cpu()
        live = ids.nonzero().flatten()
        boxes, labels, hits, misses = s.boxes.cpu(), s.labels.cpu(), s.hits.cpu(), s.misses.cpu()
        out = [{"id": int(ids[t]), "label": int(labels[t]), "box": tuple(boxes[t].tolist()), "hits": int(hits[t]),
                "misses": int(misses[t])} for t in live.tolist()]
        return sorted(out, key=lambda t: t["id"])
