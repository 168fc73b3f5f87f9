"""Stable ids for the detections of a video stream: :class:`Tracker` holds the device state of
``ops.image.track_update`` (a greedy IoU tracker with an optional constant-velocity prediction, one launch per frame)
and its parameters, and adds ``track_id`` and ``track_hits`` to what ``YolosSmall.detect_image`` or ``detect_tiled``
return. Nothing here synchronises with the host except :meth:`Tracker.tracks`, so ``YolosSmall.track_image`` and
``track_tiled`` capture as one graph whose replays advance the tracker: each replay is the next frame.

Kalman filtering, appearance or re-identification features, Hungarian assignment, a second association pass on low
scores, more than 1024 tracks and tracks across a batch of images are not offered."""
from __future__ import annotations

from typing import Dict, List

from ...ops import image as I


class Tracker:
    def __init__(self, capacity: int = 256, match_threshold: float = 0.3, max_age: int = 30,
                 birth_threshold: float = 0.0, motion: str = "constant", velocity_gain: float = 0.5, min_hits: int = 1,
                 device=None):
        """``capacity`` slots (1..1024 run as one HIP launch); a detection continues the track of its label whose
        predicted box it overlaps by an IoU above ``match_threshold``; a track unmatched for more than ``max_age``
        frames is dropped; unmatched detections with a score above ``birth_threshold`` start tracks; ``motion`` is
        ``"constant"`` (velocity, smoothed by ``velocity_gain``) or ``"none"``. ``min_hits`` is what
        ``YolosProcessor.tracked_results`` is meant to be given: tracks seen in fewer frames are not reported."""
        if not int(min_hits) >= 1:
            raise ValueError(f"Tracker: min_hits {min_hits!r} is not a number of frames from 1 up")
        I.track_params_check(float(match_threshold), int(max_age), motion, float(velocity_gain))
        self.state = I.track_state(capacity, device)
        self.params = dict(match_threshold=float(match_threshold), max_age=int(max_age),
                           birth_threshold=float(birth_threshold), motion=motion, velocity_gain=float(velocity_gain))
        self.min_hits = int(min_hits)

    @property
    def capacity(self) -> int:
        return self.state.capacity

    def reset(self) -> None:
        """Forget every track and start the ids at 1 again (on the current stream, no synchronisation)."""
        self.state.reset()

    def update(self, det: Dict[str, object]) -> Dict[str, object]:
        """``det`` — the dict of ``detect_image`` (one image) or ``detect_tiled`` — with ``track_id`` and
        ``track_hits`` added, shaped like its ``labels``: the id of each row's track and the frames that track has
        been seen in, 0 for a row without one (behind ``count``, or a birth the full tracker refused)."""
        scores, labels = det["scores"], det["labels"]
        if scores.dim() == 2 and scores.shape[0] != 1:
            raise ValueError(f"Tracker: one image's detections, not a batch of {scores.shape[0]}")
        track_id, track_hits = I.track_update(self.state, det["count"], scores, labels, det["boxes"], **self.params)
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
