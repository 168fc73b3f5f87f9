"""Inputs and the independent yardstick of the tracker tests (``tests/test_track.py`` on the CPU,
``tests/test_gpu_track.py`` on the GPU): ``ops.image.track_update`` written as a plain loop over Python floats (fp64),
with the margins of every decision it takes, and the scenes both files run.

The loop takes the fp32 lists converted to fp64 and keeps its own state in fp64. It records

* ``gap`` — the smallest difference between two different candidate scores that stand next to each other in the order;
* ``iou`` — the smallest ``|IoU - match_threshold|`` over the (candidate, track) pairs it compared;
* ``win`` — the smallest gap between a winning IoU and a competitor's (an untaken live track of the same label);
* ``birth`` — the smallest ``|score - birth_threshold|`` over the candidates left unmatched.

``guard`` asserts ``iou`` and ``win`` of at least 1e-3 and ``gap`` and ``birth`` of at least 1e-5: where these hold,
fp32 and fp64 take the same decisions. A case that sets a margin to an exact tie by hand lists it in ``exempt`` and
spells the outcome out in ``explicit``. No case is skipped: the seeds in the tables below all pass the guard.

**The bound on what is not compared equal.** ``ids``, ``labels``, ``hits``, ``misses``, ``next_id``, ``dropped`` and
both outputs are integers and compare equal. The box of a track matched or born in the last frame is the fp32 input,
bit for bit. What remains is ``vel`` and the box of a coasting track, which fp32 rounds. Let ``u = 2^-24`` and ``M``
the largest magnitude the loop saw among coordinates, predicted coordinates (coordinate plus displacement),
displacements ``d`` and velocities. With ``e_v`` and ``e_b`` the errors of one track's ``vel`` and ``boxes``:

* a match computes ``d = fl(box - boxes)`` (``|d| <= M``: one rounding of at most ``uM``, and the old box's error
  ``e_b``), ``t = fl(d - vel)`` (``|t| <= 2M``: ``2uM``), ``fl(g t)`` (``2uM``) and ``fl(vel + g t)`` (the new velocity,
  ``<= M``: ``uM``); so ``e_v' <= (1 - g) e_v + g e_b + 6uM`` (the first two roundings are scaled by ``g <= 1``), and
  ``e_b' = 0``. A fused multiply-add drops a rounding and stays inside this;
* a coasting step computes ``fl(boxes + vel)`` (``<= M``): ``e_b' <= e_b + e_v + uM``, ``e_v' = e_v``;
* a birth has ``e_v = e_b = 0``; under ``motion="none"`` nothing is rounded at all.

The loop carries the two coefficients (in units of ``uM``) per slot through exactly these recurrences, so the bound grows
with the frames since the track's birth; the comparison allows ``max(coefficient * uM, 1e-3)`` — the 1e-3 floor of the
merge tests' ``box_tol``. Nothing in it is taken from a kernel's output."""
import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

U = 2.0 ** -24
FLOOR = 1e-3
DEFAULTS = dict(match_threshold=0.3, max_age=30, birth_threshold=0.0, motion="constant", velocity_gain=0.5)


def iou(a, b):
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    inter = iw * ih
    den = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / den if den > 0.0 else 0.0


class Loop:
    """The tracker as a loop over Python floats. ``update`` is one frame; the state is the lists below."""

    def __init__(self, T: int):
        self.T = T
        self.reset()
        self.margins = {"gap": math.inf, "iou": math.inf, "win": math.inf, "birth": math.inf}
        self.M = 0.0

    def reset(self):
        T = self.T
        self.boxes = [[0.0] * 4 for _ in range(T)]
        self.vel = [[0.0] * 4 for _ in range(T)]
        self.labels, self.ids, self.hits, self.misses = [0] * T, [0] * T, [0] * T, [0] * T
        self.next_id, self.dropped = 1, 0
        self.ev, self.eb = [0.0] * T, [0.0] * T          # the error coefficients, in units of u M
        self.fresh = set()                               # slots whose box is the last frame's input, bit for bit
        self.births = 0

    def _saw(self, *values):
        for v in values:
            if math.isfinite(v):
                self.M = max(self.M, abs(v))

    def update(self, count, scores, labels, boxes, match_threshold=0.3, max_age=30, birth_threshold=0.0,
               motion="constant", velocity_gain=0.5):
        T, N, g, constant, m = self.T, len(scores), velocity_gain, motion == "constant", self.margins
        n = min(max(int(count), 0), N)
        cands = sorted((r for r in range(n) if scores[r] > 0.0), key=lambda r: (-scores[r], r))
        for a, b in zip(cands, cands[1:]):
            if scores[a] != scores[b]:
                m["gap"] = min(m["gap"], scores[a] - scores[b])
        live = [t for t in range(T) if self.ids[t] != 0]
        pred = {t: [b + v for b, v in zip(self.boxes[t], self.vel[t])] if constant else list(self.boxes[t])
                for t in live}
        for t in live:
            self._saw(*pred[t], *self.boxes[t], *self.vel[t])
        by_label: Dict[int, List[int]] = {}
        for t in live:
            by_label.setdefault(self.labels[t], []).append(t)
        taken: Dict[int, int] = {}
        match: Dict[int, int] = {}
        for r in cands:
            self._saw(*boxes[r])
            comps = [(iou(boxes[r], pred[t]), t) for t in by_label.get(labels[r], ()) if t not in taken]
            for o, _ in comps:
                m["iou"] = min(m["iou"], abs(o - match_threshold))
            if not comps:
                continue
            top = max(o for o, _ in comps)
            if top > match_threshold:
                slot = min(t for o, t in comps if o == top)
                for o, t in comps:
                    if t != slot:
                        m["win"] = min(m["win"], top - o)
                taken[slot] = r
                match[r] = slot
        self.fresh = set()
        for t in live:
            if t in taken:
                box = boxes[taken[t]]
                d = [b - o for b, o in zip(box, self.boxes[t])]
                self._saw(*d)
                if constant:
                    self.vel[t] = [v + g * (x - v) for v, x in zip(self.vel[t], d)]
                    self._saw(*self.vel[t])
                    self.ev[t] = (1.0 - g) * self.ev[t] + g * self.eb[t] + 6.0
                self.eb[t] = 0.0
                self.boxes[t] = list(box)
                self.hits[t] += 1
                self.misses[t] = 0
                self.fresh.add(t)
            else:
                self.misses[t] += 1
                if self.misses[t] > max_age:
                    self.boxes[t], self.vel[t] = [0.0] * 4, [0.0] * 4
                    self.labels[t] = self.ids[t] = self.hits[t] = self.misses[t] = 0
                    self.ev[t] = self.eb[t] = 0.0
                elif constant:
                    self.boxes[t] = [b + v for b, v in zip(self.boxes[t], self.vel[t])]
                    self._saw(*self.boxes[t])
                    self.eb[t] = self.eb[t] + self.ev[t] + 1.0
        free = [t for t in range(T) if self.ids[t] == 0]
        track_id, track_hits = [0] * N, [0] * N
        for r, t in match.items():
            track_id[r], track_hits[r] = self.ids[t], self.hits[t]
        for r in cands:
            if r in match:
                continue
            m["birth"] = min(m["birth"], abs(scores[r] - birth_threshold))
            if not scores[r] > birth_threshold:
                continue
            if not free:
                self.dropped += 1
                continue
            t = free.pop(0)
            self.boxes[t], self.vel[t] = list(boxes[r]), [0.0] * 4
            self.labels[t], self.ids[t], self.hits[t], self.misses[t] = labels[r], self.next_id, 1, 0
            self.ev[t] = self.eb[t] = 0.0
            self.fresh.add(t)
            track_id[r], track_hits[r] = self.next_id, 1
            self.next_id += 1
            self.births += 1
        return track_id, track_hits

    def snapshot(self):
        return {"boxes": [list(b) for b in self.boxes], "vel": [list(v) for v in self.vel], "labels": list(self.labels),
                "ids": list(self.ids), "hits": list(self.hits), "misses": list(self.misses), "next_id": self.next_id,
                "dropped": self.dropped, "ev": list(self.ev), "eb": list(self.eb), "fresh": set(self.fresh)}


@dataclass
class Frame:
    """One frame's lists as the tracker is handed them: views of the first ``N`` rows of the tensors held here (the
    rows behind ``N`` are plausible candidates that a missing clamp of ``count`` would read)."""
    count: int
    scores: torch.Tensor
    labels: torch.Tensor
    boxes: torch.Tensor
    N: int

    def lists(self, device=None):
        full = (self.scores, self.labels, self.boxes) if device is None else \
            tuple(t.to(device) for t in (self.scores, self.labels, self.boxes))
        count = torch.tensor([self.count], dtype=torch.int32, device=device)
        return (count,) + tuple(t[:self.N] for t in full)


def frame(count, scores, labels, boxes, N=None) -> Frame:
    scores = torch.as_tensor(scores, dtype=torch.float32).reshape(-1)
    labels = torch.as_tensor(labels, dtype=torch.int32).reshape(-1)
    boxes = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    return Frame(int(count), scores, labels, boxes, scores.shape[0] if N is None else N)


@dataclass
class Case:
    name: str
    T: int
    frames: List[Frame]
    params: dict = field(default_factory=dict)
    exempt: Tuple[str, ...] = ()
    explicit: Optional[Callable] = None          # explicit(outs, snaps): the outcome a hand-set tie must have
    reset_before: Tuple[int, ...] = ()           # frames before which the tracker is reset

    def kwargs(self) -> dict:
        return {**DEFAULTS, **self.params}


def run_loop(case: Case):
    """``(outs, snaps, loop)``: per frame the two output lists and the state after it."""
    loop = Loop(case.T)
    outs, snaps = [], []
    for i, f in enumerate(case.frames):
        if i in case.reset_before:
            loop.reset()
        sc = f.scores[:f.N].double().tolist()
        outs.append(loop.update(f.count, sc, f.labels[:f.N].tolist(), f.boxes[:f.N].double().tolist(),
                                **case.kwargs()))
        snaps.append(loop.snapshot())
    return outs, snaps, loop


def guard(case: Case):
    """The loop on ``case`` with its margins checked: ``(outs, snaps, loop)``."""
    outs, snaps, loop = run_loop(case)
    m = loop.margins
    for name, least in (("iou", 1e-3), ("win", 1e-3), ("gap", 1e-5), ("birth", 1e-5)):
        assert name in case.exempt or m[name] >= least, (case.name, name, m)
    assert not case.exempt or case.explicit is not None, case.name
    if case.explicit is not None:
        case.explicit(outs, snaps)
    return outs, snaps, loop


def tol(coefficient: float, M: float) -> float:
    return max(coefficient * U * M, FLOOR)


def check_frame(state, got_id, got_hits, out, snap, M):
    """A ``TrackState`` and the two outputs (on the CPU) against the loop's frame. Returns ``(worst vel difference,
    its bound, worst coasting-box difference, its bound)``; the bounds are the largest allowed among the slots."""
    T = len(snap["ids"])
    assert got_id.dtype == torch.int32 and got_hits.dtype == torch.int32
    assert got_id.tolist() == out[0], ("track_id", got_id.tolist(), out[0])
    assert got_hits.tolist() == out[1], ("track_hits", got_hits.tolist(), out[1])
    for name in ("labels", "ids", "hits", "misses"):
        t = getattr(state, name)
        assert t.dtype == torch.int32 and t.shape == (T,) and t.tolist() == snap[name], (name, t.tolist(), snap[name])
    assert state.next_id.tolist() == [snap["next_id"]] and state.dropped.tolist() == [snap["dropped"]], \
        (state.next_id.tolist(), snap["next_id"], state.dropped.tolist(), snap["dropped"])
    assert state.boxes.shape == (T, 4) and state.vel.shape == (T, 4) and state.boxes.dtype == torch.float32
    boxes, vel = state.boxes.double().tolist(), state.vel.double().tolist()
    dv = bv = db = bb = 0.0
    for t in range(T):
        if snap["ids"][t] == 0:
            assert boxes[t] == [0.0] * 4 and vel[t] == [0.0] * 4, ("a free slot holds zeros", t)
            continue
        tv, tb = tol(snap["ev"][t], M), tol(snap["eb"][t], M)
        ev = max(abs(a - b) for a, b in zip(vel[t], snap["vel"][t]))
        assert ev <= tv, ("vel", t, ev, tv)
        dv, bv = max(dv, ev), max(bv, tv)
        if t in snap["fresh"]:
            assert boxes[t] == snap["boxes"][t], ("the box of a matched or newborn track is the input's", t)
        else:
            eb = max(abs(a - b) for a, b in zip(boxes[t], snap["boxes"][t]))
            assert eb <= tb, ("box", t, eb, tb)
            db, bb = max(db, eb), max(bb, tb)
    return dv, bv, db, bb


def run_case(I, case: Case, update, device=None, state=None):
    """``update`` (``I.track_update`` or its reference) over the frames of ``case`` against the guarded loop, frame by
    frame. Returns the ``[track]`` line."""
    outs, snaps, loop = guard(case)
    state = I.track_state(case.T, device) if state is None else state
    worst = [0.0, 0.0, 0.0, 0.0]
    for i, (f, out, snap) in enumerate(zip(case.frames, outs, snaps)):
        if i in case.reset_before:
            state.reset()
        got_id, got_hits = update(state, *f.lists(device), **case.kwargs())
        host = I.TrackState(*(t.cpu() for t in state.tensors()))
        try:
            w = check_frame(host, got_id.cpu(), got_hits.cpu(), out, snap, loop.M)
        except AssertionError:
            print(f"[track] {case.name}: frame {i} of {len(case.frames)} differs; margins {fmt(loop.margins)}")
            raise
        worst = [max(a, b) for a, b in zip(worst, w)]
    live = sum(1 for v in snaps[-1]["ids"] if v)
    return (f"[track] {case.name}: {len(case.frames)} frames, N {case.frames[0].N}, T {case.T}, {live} live, "
            f"{loop.births} births, dropped {snaps[-1]['dropped']}; max |d vel| {worst[0]:.3g} (bound {worst[1]:.3g}), "
            f"max |d coasting box| {worst[2]:.3g} px (bound {worst[3]:.3g}), M {loop.M:.4g}; margins {fmt(loop.margins)}")


def fmt(m):
    return "{" + ", ".join(f"{k} {v:.3g}" for k, v in m.items()) + "}"


# ---- random scenes --------------------------------------------------------------------------------------------------
#: seeds whose scenes the loop decides clearly (of 0..39, the ones that pass ``guard``; the others are not used)
RANDOM_SEEDS = (0, 1, 2, 4)


def random_case(seed: int, **params) -> Case:
    """12-40 objects of 40-300 px over 8-12 frames of a 2000 px frame: up to 25 px / frame of motion, 2 px of jitter,
    3 labels, a fifth of the detections missing in any frame, the rows shuffled."""
    g = torch.Generator().manual_seed(7000 + seed)

    def rnd(*shape):
        return torch.rand(*shape, generator=g)
    n = int(torch.randint(12, 41, (1,), generator=g))
    nf = int(torch.randint(8, 13, (1,), generator=g))
    size = 40.0 + 260.0 * rnd(n, 2)
    pos = 100.0 + 1500.0 * rnd(n, 2)
    velocity = 50.0 * rnd(n, 2) - 25.0
    label = torch.randint(0, 3, (n,), generator=g)
    frames = []
    for _ in range(nf):
        seen = (rnd(n) > 0.2).nonzero().flatten()
        seen = seen[torch.randperm(seen.shape[0], generator=g)]
        k = seen.shape[0]
        jitter = 4.0 * rnd(k, 4) - 2.0
        xy = pos[seen]
        boxes = torch.cat((xy, xy + size[seen]), dim=1) + jitter
        scores = 0.3 + 0.69 * rnd(k)
        N = max(k, 1)
        pad = N - k
        frames.append(frame(k, torch.cat((scores, torch.zeros(pad))), torch.cat((label[seen], torch.zeros(pad))),
                            torch.cat((boxes, torch.zeros(pad, 4)))))
        pos = pos + velocity
    name = f"random scene {seed}" + "".join(f", {k} {v}" for k, v in params.items())
    return Case(name, 64, frames, dict(max_age=2, **params))


# ---- lattices: hundreds of rows, every IoU either 0 or far from the threshold ---------------------------------------
#: ``(N, T)``: rows and slots around a wave, around 100 and at the 1024 limit
LATTICE_SIZES = ((1, 1), (63, 64), (64, 63), (65, 100), (100, 65), (64, 64), (1023, 1024), (1024, 1023), (1024, 1024))


def lattice_case(N: int, T: int, seed: int = 0, nframes: int = 4, count=None, extra: int = 0, name=None,
                 **params) -> Case:
    """``N`` rows per frame on a lattice of 64 px cells holding 32 px boxes, 16 labels by column, scores along a shuffled
    ramp (neighbours at least 6e-4 apart). Frame 0 fills the tracker (``N - T`` births dropped when it is too small);
    in frame 1 the objects have moved by up to 3 px and every fifth row holds no candidate (score 0); in frame 2 they
    move on and every fifth object is replaced by a new one in the lattice's second half, which with ``max_age = 1`` kills
    the old one in frame 3 and reuses its slot. ``count``: per frame, else ``N``. ``extra``: rows behind ``N`` in the
    allocation, filled with more objects of the same kind."""
    g = torch.Generator().manual_seed(8000 + seed + 13 * N + T)
    side = 40
    rows = N + extra
    cell = torch.arange(2 * rows)
    origin = torch.stack((64.0 * (cell % side), 64.0 * (cell // side)), dim=1)
    label = (cell % 16).to(torch.int32)
    frames = []
    who = torch.arange(rows)
    shift = torch.zeros(2 * rows, 2)
    for k in range(nframes):
        if k == 2:
            who = torch.where(who % 5 == 2, who + rows, who)
        perm = torch.randperm(rows, generator=g)
        ids = who[perm]
        xy = origin[ids] + 8.0 + shift[ids]
        boxes = torch.cat((xy, xy + 32.0), dim=1)
        scores = 0.25 + 0.7 * (torch.randperm(rows, generator=g).float() + 1.0) / rows
        if k == 1:
            scores = torch.where(ids % 5 == 0, torch.zeros(()), scores)
        c = N if count is None else count[k]
        frames.append(frame(c, scores, label[ids], boxes, N))
        shift = shift + torch.randint(-3, 4, (2 * rows, 2), generator=g).float()
    return Case(name or f"lattice N {N} T {T}", T, frames, dict(max_age=1, **params))


def count_cases() -> List[Case]:
    """``count`` at 0, 1 and N, then above N and negative over lists that are views of larger allocations."""
    return [lattice_case(65, 64, seed=1, count=(65, 0, 1, 65), name="count N, 0, 1, N"),
            lattice_case(100, 128, seed=2, count=(100, 1000, -3, 163), extra=63, name="count N, 1000, -3, 163 of 100")]


# ---- matching ---------------------------------------------------------------------------------------------------------
def _expect(frame_outs):
    """``explicit`` that asserts the outputs, ``[(track_id, track_hits), ...]`` per frame."""
    def check(outs, snaps):
        assert [tuple(map(list, o)) for o in outs] == [tuple(map(list, o)) for o in frame_outs], (outs, frame_outs)
    return check


def contested_track_case() -> Case:
    # row 0 (score 0.9) overlaps the track less than row 1 (score 0.8) does: the score decides, row 1 starts a track
    f0 = frame(1, [0.7], [1], [[100, 100, 200, 200]])
    f1 = frame(2, [0.9, 0.8], [1, 1], [[130, 100, 230, 200], [105, 100, 205, 200]])
    return Case("two detections, one track", 4, [f0, f1], explicit=_expect([([1], [1]), ([1, 2], [2, 1])]))


def two_tracks_case() -> List[Case]:
    tracks = frame(2, [0.7, 0.6], [1, 1], [[0, 0, 10, 10], [10, 0, 20, 10]])
    # 4/10 of slot 0's box and 6/10 of slot 1's: slot 1 (IoU 3/7 against 1/4)
    larger = frame(1, [0.9], [1], [[6, 0, 16, 10]])
    # half of each: both IoUs are fl(50 / 150), the lower slot takes it
    tie = frame(1, [0.9], [1], [[5, 0, 15, 10]])
    p = dict(match_threshold=0.2, motion="none")
    return [Case("one detection, two tracks: the larger IoU", 4, [tracks, larger], p,
                 explicit=_expect([([1, 2], [1, 1]), ([2], [2])])),
            Case("one detection, two tracks: a tie goes to the lower slot", 4, [tracks, tie], p, exempt=("win",),
                 explicit=_expect([([1, 2], [1, 1]), ([1], [2])]))]


def label_case() -> Case:
    f0 = frame(1, [0.7], [1], [[100, 100, 200, 200]])
    f1 = frame(1, [0.9], [2], [[100, 100, 200, 200]])
    return Case("another label never matches", 4, [f0, f1], explicit=_expect([([1], [1]), ([2], [1])]))


#: the fp32 number just below one half
BELOW_HALF = 0.5 - 2.0 ** -25


def strict_match_cases() -> List[Case]:
    # integer boxes: inter 50, union 100, IoU exactly 0.5 in fp32 and in fp64
    f0 = frame(1, [0.7], [1], [[0, 0, 10, 10]])
    f1 = frame(1, [0.9], [1], [[0, 0, 10, 5]])
    return [Case("IoU 0.5 does not exceed 0.5", 4, [f0, f1], dict(match_threshold=0.5, motion="none"),
                 exempt=("iou",), explicit=_expect([([1], [1]), ([2], [1])])),
            Case("IoU 0.5 exceeds the fp32 number below 0.5", 4, [f0, f1],
                 dict(match_threshold=BELOW_HALF, motion="none"), exempt=("iou",),
                 explicit=_expect([([1], [1]), ([1], [2])]))]


def degenerate_case() -> Case:
    # a box of no extent and two of negative extent start tracks, and in the next frame match nothing, themselves included
    rows = [[50, 50, 50, 90], [80, 80, 40, 40], [80, 0, 40, 100], [200, 200, 300, 300]]
    f = frame(4, [0.9, 0.8, 0.7, 0.6], [1, 1, 1, 1], rows)
    return Case("boxes of no or negative extent match nothing", 16, [f, f], dict(motion="none"),
                explicit=_expect([([1, 2, 3, 4], [1, 1, 1, 1]), ([5, 6, 7, 4], [1, 1, 1, 2])]))


def not_candidates_case() -> Case:
    nan = float("nan")
    boxes = [[0, 0, 50, 50], [100, 0, 150, 50], [200, 0, 250, 50], [300, 0, 350, 50], [400, 0, 450, 50]]
    f = frame(4, [nan, 0.9, 0.0, -0.5, 0.8], [1, 1, 1, 1, 1], boxes)
    return Case("NaN, zero and negative scores, and a row behind count", 8, [f, f],
                explicit=_expect([([0, 1, 0, 0, 0], [0, 1, 0, 0, 0]), ([0, 1, 0, 0, 0], [0, 2, 0, 0, 0])]))


# ---- lifecycle --------------------------------------------------------------------------------------------------------
def _moving(k, step=30.0, size=100.0, y=100.0):
    return [[step * k, y, step * k + size, y + size]]


def max_age_zero_case() -> Case:
    # the track dies in the frame that misses it: the same box afterwards is a new track in the same slot
    seen, none = frame(1, [0.9], [1], _moving(0)), frame(0, [0.0], [0], [[0, 0, 0, 0]])
    return Case("max_age 0 dies on the first miss", 4, [seen, none, seen], dict(max_age=0),
                explicit=_expect([([1], [1]), ([0], [0]), ([2], [1])]))


def slot_reuse_case() -> Case:
    # a full tracker of two: slot 0's track dies in frame 1, whose new object is born into slot 0 in that same frame
    f0 = frame(2, [0.9, 0.8], [1, 1], [[0, 0, 50, 50], [100, 0, 150, 50]])
    f1 = frame(2, [0.9, 0.8], [1, 1], [[100, 0, 150, 50], [300, 0, 350, 50]])

    def explicit(outs, snaps):
        _expect([([1, 2], [1, 1]), ([2, 3], [2, 1])])(outs, snaps)
        assert snaps[1]["ids"] == [3, 2] and snaps[1]["dropped"] == 0
    return Case("a slot freed in a frame is reused by that frame's birth", 2, [f0, f1], dict(max_age=0),
                explicit=explicit)


def coasting_cases() -> List[Case]:
    # 30 px a frame, seen in frames 0-2, unseen in 3 and 4, seen again in 5 at 150: the constant-velocity box has
    # coasted to 120 + 30 = 150; a standing one is still at 60
    none = frame(0, [0.0], [0], [[0, 0, 0, 0]])
    frames = [frame(1, [0.9], [1], _moving(k)) for k in range(3)] + [none, none, frame(1, [0.9], [1], _moving(5))]
    hits = [([1], [1]), ([1], [2]), ([1], [3]), ([0], [0]), ([0], [0])]
    return [Case("a coasting track is found again", 4, frames, dict(motion="constant", velocity_gain=1.0),
                 explicit=_expect(hits + [([1], [4])])),
            Case("a standing track is lost", 4, frames, dict(motion="none"), explicit=_expect(hits + [([2], [1])]))]


def gain_case(gain: float) -> Case:
    # steps of 7 and then 11 px: the velocity is 0 (gain 0), the last step (gain 1), or half way there each time
    xs = (0.0, 7.0, 18.0, 29.0)
    frames = [frame(1, [0.9], [1], [[x, 100, x + 60, 160]]) for x in xs] + [frame(0, [0.0], [0], [[0, 0, 0, 0]])]

    def explicit(outs, snaps):
        want = {0.0: 0.0, 1.0: 11.0, 0.5: 0.5 * (0.5 * (0.5 * 7.0 + 11.0) + 11.0)}[gain]
        assert snaps[3]["vel"][0] == [want, 0.0, want, 0.0], snaps[3]["vel"][0]
        assert snaps[4]["boxes"][0][0] == 29.0 + want and snaps[4]["misses"][0] == 1
    return Case(f"velocity_gain {gain:g}", 4, frames, dict(velocity_gain=gain), explicit=explicit)


def full_case() -> Case:
    # five objects, three slots: the two lowest scores are dropped, and again in the next frame
    boxes = [[100.0 * k, 0, 100.0 * k + 50, 50] for k in range(5)]
    f = frame(5, [0.5, 0.9, 0.6, 0.8, 0.7], [1] * 5, boxes)

    def explicit(outs, snaps):
        _expect([([0, 1, 0, 2, 3], [0, 1, 0, 1, 1]), ([0, 1, 0, 2, 3], [0, 2, 0, 2, 2])])(outs, snaps)
        assert [s["dropped"] for s in snaps] == [2, 4] and snaps[1]["next_id"] == 4
    return Case("a full tracker drops the births it has no slot for", 3, [f, f], explicit=explicit)


def strict_birth_case() -> Case:
    f = frame(3, [0.5, 0.75, 0.25], [1, 1, 1], [[0, 0, 50, 50], [100, 0, 150, 50], [200, 0, 250, 50]])
    return Case("a score of 0.5 does not exceed a birth threshold of 0.5", 4, [f], dict(birth_threshold=0.5),
                exempt=("birth",), explicit=_expect([([0, 1, 0], [0, 1, 0])]))


def fifty_frames_case() -> Case:
    """Fifty frames of a 12 x 12 lattice in which an object is seen two frames of three: tracks coast, die after two
    misses in a row (never here) and new objects arrive every tenth frame."""
    g = torch.Generator().manual_seed(9000)
    frames = []
    n = 96
    cell = torch.arange(n)
    for k in range(50):
        active = cell < 48 + 8 * (k // 10)
        seen = active & ((cell + k) % 3 != 0)
        rows = seen.nonzero().flatten()
        rows = rows[torch.randperm(rows.shape[0], generator=g)]
        x = 160.0 * (rows % 12) + 3.0 * k + torch.randint(-1, 2, rows.shape, generator=g)
        y = 160.0 * (rows // 12) + 2.0 * k
        boxes = torch.stack((x, y, x + 64.0, y + 64.0), dim=1)
        scores = 0.3 + 0.6 * (torch.randperm(rows.shape[0], generator=g).float() + 1.0) / rows.shape[0]
        frames.append(frame(rows.shape[0], scores, (rows % 3).to(torch.int32), boxes))

    def explicit(outs, snaps):
        born = sum(1 for o in outs for v in o[1] if v == 1)
        assert snaps[-1]["next_id"] == 1 + born == 1 + 48 + 8 * 4 and snaps[-1]["dropped"] == 0
    return Case("fifty frames", 128, frames, dict(max_age=2), explicit=explicit)


def graph_cases() -> Tuple[Case, Case]:
    """Two ten-frame sequences of one shape (N 48, T 64) for one captured launch: the second starts after a reset."""
    def sequence(seed):
        g = torch.Generator().manual_seed(9100 + seed)
        frames = []
        for k in range(10):
            perm = torch.randperm(48, generator=g)
            x = 100.0 * (perm % 8) + 4.0 * k * (1 + seed)
            y = 100.0 * (perm // 8) + 2.0 * k
            scores = 0.3 + 0.6 * (torch.randperm(48, generator=g).float() + 1.0) / 48
            scores = torch.where((perm + k) % 7 == 0, torch.zeros(()), scores)
            frames.append(frame(48 - (k % 3), scores, (perm % 4).to(torch.int32),
                                torch.stack((x, y, x + 50.0, y + 50.0), dim=1)))
        return Case(f"graph sequence {seed}", 64, frames, dict(max_age=1))
    return sequence(0), sequence(1)


def all_cases() -> List[Case]:
    """Every case both files run (the graph sequences too, as plain frames)."""
    cases = [random_case(s) for s in RANDOM_SEEDS] + [random_case(RANDOM_SEEDS[0], motion="none")]
    cases += [lattice_case(N, T) for N, T in LATTICE_SIZES] + count_cases()
    cases += [contested_track_case(), *two_tracks_case(), label_case(), *strict_match_cases(), degenerate_case(),
              not_candidates_case(), max_age_zero_case(), slot_reuse_case(), *coasting_cases(),
              *(gain_case(v) for v in (0.0, 0.5, 1.0)), full_case(), strict_birth_case(), fifty_frames_case(),
              *graph_cases()]
    return cases
