"""The tracker kernel (``track_update_f32``, ``csrc/image_track.h``) on the GPU. The yardstick is the fp64 loop of
``tests/track_case.py`` on inputs it decides clearly (``track_case.guard``, recomputed for every case on the CPU by
``tests/test_track.py``; the margins a case sets by hand to an exact tie come with the outcome spelled out). Every
comparison asserts that the torch reference was not called, so a silent fall-back cannot pass.

``ids``, ``labels``, ``hits``, ``misses``, ``next_id``, ``dropped``, ``track_id`` and ``track_hits`` compare equal after
every frame, and so does, bit for bit against the fp32 input, the box of every track matched or born in that frame.
``vel`` and the boxes of coasting tracks compare within the bound derived in ``track_case``'s docstring from the fp32
rounding of the update rule: per slot ``max(c * 2^-24 * M, 1e-3)``, ``M`` the largest coordinate plus displacement the
loop saw, ``c`` carried through ``c_v' = (1 - g) c_v + g c_b + 6`` (a match) and ``c_b' = c_b + c_v + 1`` (a coasting
step) from the track's birth. It is not fitted to the kernel's output.

What each group pins:

* ``N`` and ``T`` at 1, 63, 64, 65, 100, 1023 and 1024; ``count`` at 0, 1 and ``N``, above ``N`` and negative over lists
  that are views of larger allocations full of plausible candidates;
* matching: the score decides between two detections, the IoU between two tracks, the lower slot an exact tie, labels
  never mix, ``match_threshold`` is strict at an IoU of exactly 0.5, boxes of no or negative extent match nothing, NaN
  and zero scores are no candidates;
* lifecycle: ``max_age = 0``, a slot freed and reused in one frame, coasting under ``"constant"`` against ``"none"``,
  ``velocity_gain`` 0, 0.5 and 1, a full tracker's ``dropped``, the strict ``birth_threshold``, fifty frames;
* the outputs written in full into buffers of 0x7F, and the wrapper's refusals;
* one captured launch replayed over two ten-frame sequences with a ``reset()`` between them;
* ``track_image`` and ``track_tiled`` captured on a model with distinguishable parameters.

One ``[track]`` line per comparison; the run on the MI355X is kept in ``profiles/pytest_gpu_track.log``."""
import pytest
import torch

import track_case as C

pytestmark = pytest.mark.gpu


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


def compare(I, monkeypatch, case):
    """The kernel on ``case`` against the guarded loop, frame by frame."""
    ref = Counter(monkeypatch, I, "track_update_reference")
    print(C.run_case(I, case, I.track_update, device="cuda"))
    assert ref.n == 0


# ---- sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T", C.LATTICE_SIZES, ids=[f"N{n}-T{t}" for n, t in C.LATTICE_SIZES])
def test_track_rows_and_slots(K, I, monkeypatch, N, T):
    compare(I, monkeypatch, C.lattice_case(N, T))


@pytest.mark.parametrize("seed", C.RANDOM_SEEDS)
def test_track_random_scenes(K, I, monkeypatch, seed):
    compare(I, monkeypatch, C.random_case(seed))
    if seed == C.RANDOM_SEEDS[0]:
        compare(I, monkeypatch, C.random_case(seed, motion="none"))


def test_track_count_is_clamped(K, I, monkeypatch):
    for case in C.count_cases():
        compare(I, monkeypatch, case)


# ---- matching ---------------------------------------------------------------------------------------------------------
def test_track_the_higher_score_takes_a_contested_track(K, I, monkeypatch):
    compare(I, monkeypatch, C.contested_track_case())


def test_track_the_larger_iou_wins_and_a_tie_goes_to_the_lower_slot(K, I, monkeypatch):
    for case in C.two_tracks_case():
        compare(I, monkeypatch, case)


def test_track_labels_never_mix(K, I, monkeypatch):
    compare(I, monkeypatch, C.label_case())


def test_track_match_threshold_is_strict(K, I, monkeypatch):
    for case in C.strict_match_cases():
        compare(I, monkeypatch, case)


def test_track_degenerate_boxes_match_nothing(K, I, monkeypatch):
    compare(I, monkeypatch, C.degenerate_case())


def test_track_nan_and_zero_scores_are_no_candidates(K, I, monkeypatch):
    compare(I, monkeypatch, C.not_candidates_case())


# ---- lifecycle --------------------------------------------------------------------------------------------------------
def test_track_max_age_zero_and_slot_reuse(K, I, monkeypatch):
    compare(I, monkeypatch, C.max_age_zero_case())
    compare(I, monkeypatch, C.slot_reuse_case())


def test_track_coasting_finds_what_standing_loses(K, I, monkeypatch):
    for case in C.coasting_cases():
        compare(I, monkeypatch, case)


@pytest.mark.parametrize("gain", (0.0, 0.5, 1.0))
def test_track_velocity_gain(K, I, monkeypatch, gain):
    compare(I, monkeypatch, C.gain_case(gain))


def test_track_full_tracker_and_birth_threshold(K, I, monkeypatch):
    compare(I, monkeypatch, C.full_case())
    compare(I, monkeypatch, C.strict_birth_case())


def test_track_fifty_frames(K, I, monkeypatch):
    compare(I, monkeypatch, C.fifty_frames_case())


# ---- the outputs, and what the wrapper refuses --------------------------------------------------------------------------
PAD = 64        # bytes behind every output that must stay as they were


def raw_call(I, state, lists, N, outs, kw):
    return I._L().nos_track_update_f32(*(t.data_ptr() for t in lists), N, *(t.data_ptr() for t in state.tensors()),
                                       state.capacity, kw["match_threshold"], kw["max_age"], kw["birth_threshold"],
                                       I.MOTIONS[kw["motion"]], kw["velocity_gain"], *(t.data_ptr() for t in outs),
                                       torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("N,T", ((100, 65), (1024, 1023), (65, 64)))
def test_track_writes_every_output_element(K, I, N, T):
    case = C.count_cases()[0] if (N, T) == (65, 64) else C.lattice_case(N, T)      # the first with counts 65, 0, 1, 65
    outs, snaps, loop = C.guard(case)
    state = I.track_state(T, "cuda")
    for f, out in zip(case.frames, outs):
        raw = [torch.full((4 * N + PAD,), 0x7F, dtype=torch.uint8, device="cuda") for _ in range(2)]
        lists = [t.contiguous() for t in f.lists("cuda")]
        assert raw_call(I, state, lists, N, raw, case.kwargs()) == 0
        torch.cuda.synchronize()
        assert all(bool((t[-PAD:] == 0x7F).all()) for t in raw)
        got = [t[:-PAD].view(torch.int32).cpu() for t in raw]
        assert not any(bool((g == 0x7F7F7F7F).any()) for g in got)
        assert got[0].tolist() == out[0] and got[1].tolist() == out[1]
    zeros = sum(1 for o in outs for v in o[0] if v == 0)
    print(f"[track] {case.name}: into buffers of 0x7F, every element of both outputs written in {len(outs)} frames "
          f"({zeros} of them zeros), the bytes behind them untouched")


def test_track_wrapper_refuses_before_any_launch(K, I):
    state = I.track_state(4, "cuda")
    lists = [t.contiguous() for t in C.full_case().frames[0].lists("cuda")]
    L, p = I._L(), lists[1].data_ptr()
    before = [t.clone() for t in state.tensors()]

    def call(N=5, T=4, motion=1, mt=0.3, max_age=30, gain=0.5, null=None):
        a = [p] * 4 + [N] + [p] * 8 + [T, mt, max_age, 0.0, motion, gain, p, p]
        if null is not None:
            a[null] = None
        return L.nos_track_update_f32(*a, None)
    for bad in (dict(N=0), dict(N=1025), dict(N=-1), dict(T=0), dict(T=1025), dict(motion=2), dict(motion=-1),
                dict(mt=-0.5), dict(mt=float("nan")), dict(max_age=-1), dict(gain=1.5), dict(gain=-0.5),
                *(dict(null=i) for i in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 19, 20))):
        assert call(**bad) == -1 and L.nos_image_last_error(), bad
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, state.tensors()))


def test_track_other_inputs_take_the_reference(K, I, monkeypatch):
    # fp64 lists and more than 1024 slots: the torch composition, by the wrapper's own choice, and the same ids
    ref = Counter(monkeypatch, I, "track_update_reference")
    f = C.full_case().frames[0]
    count, scores, labels, boxes = f.lists("cuda")
    hip = I.track_update(I.track_state(8, "cuda"), count, scores, labels, boxes)
    assert ref.n == 0
    wide = I.track_update(I.track_state(8, "cuda"), count, scores.double(), labels, boxes.double())
    many = I.track_update(I.track_state(1025, "cuda"), count, scores, labels, boxes)
    assert ref.n == 2
    K.set_backend("torch")
    try:
        off = I.track_update(I.track_state(8, "cuda"), count, scores, labels, boxes)
    finally:
        K.set_backend("hip")
    assert ref.n == 3
    for other in (wide, many, off):
        assert all(torch.equal(a, b) for a, b in zip(hip, other))


# ---- one captured launch, replayed ------------------------------------------------------------------------------------
def test_track_graph_replay_is_the_next_frame(K, I, monkeypatch):
    first, second = C.graph_cases()
    ref = Counter(monkeypatch, I, "track_update_reference")
    N, T = first.frames[0].N, first.T
    state = I.track_state(T, "cuda")
    static = [t.clone() for t in first.frames[0].lists("cuda")]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        held = I.track_update(state, *static, **first.kwargs())
    for case in (first, second):
        assert case.kwargs() == first.kwargs() and case.T == T
        outs, snaps, loop = C.guard(case)
        state.reset()
        worst = [0.0] * 4
        for f, out, snap in zip(case.frames, outs, snaps):
            assert f.N == N
            for dst, src in zip(static, f.lists()):
                dst.copy_(src)
            for t in held:
                t.fill_(-7)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            host = I.TrackState(*(t.cpu() for t in state.tensors()))
            w = C.check_frame(host, held[0].cpu(), held[1].cpu(), out, snap, loop.M)
            worst = [max(a, b) for a, b in zip(worst, w)]
        print(f"[track] {case.name}: one graph replayed over {len(case.frames)} frames, the state after every replay "
              f"equal to the loop's; max |d vel| {worst[0]:.3g} (bound {worst[1]:.3g}), max |d coasting box| "
              f"{worst[2]:.3g} px (bound {worst[3]:.3g}); next_id {snaps[-1]['next_id']}")
    assert ref.n == 0
    del graph


# ---- end to end -------------------------------------------------------------------------------------------------------
def small_model():
    from yolos_reference import randomize
    from walkai_nos_amd.models.workload.processor import YolosProcessor
    from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=2, use_mid_position_embeddings=True)).eval()
    randomize(m)
    m.invalidate_cache()
    m.processor = YolosProcessor(80, 133)
    return m


@pytest.fixture(scope="module")
def model(K):
    return small_model().cuda()


KEYS = ("count", "scores", "labels", "boxes")


@pytest.mark.parametrize("tiled", (False, True), ids=("track_image", "track_tiled"))
def test_track_captured_on_the_model(K, I, monkeypatch, model, tiled):
    """The graph of ``track_image`` / ``track_tiled`` replayed three times on one frame and twice on a shifted one. The
    loop is fed each replay's own detections, the fp32 numbers the kernel read, so the order of the scores is the same
    in both and only the IoU margins are asserted (the score gaps are printed)."""
    from walkai_nos_amd.models.workload.tracker import Tracker
    ref = Counter(monkeypatch, I, "track_update_reference")
    g = torch.Generator().manual_seed(13)
    frame = torch.randint(0, 256, (97, 131, 3), generator=g, dtype=torch.uint8)
    shifted = torch.roll(frame, (3, 5), (0, 1))
    buf = frame.cuda()
    tracker = Tracker(capacity=64, device="cuda")
    keep = 24 if tiled else 12

    def detect(thr):
        return model.detect_tiled(buf, (3, 2), 0.3, thr) if tiled else model.detect_image(buf, thr)

    def track(thr):
        return model.track_tiled(buf, tracker, (3, 2), 0.3, thr) if tiled else model.track_image(buf, tracker, thr)
    with torch.no_grad():
        s = detect(0.0)["scores"].flatten().sort().values
        thr = 0.5 * (s[-keep - 1] + s[-keep]).item()
        assert s[-keep].item() - s[-keep - 1].item() > 1e-7
        plain = {k: v.clone() for k, v in detect(thr).items() if k in KEYS}
        track(thr)                                      # a warm-up, no frame of the sequence
    tracker.reset()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=stream):
        held = track(thr)
    tracker.reset()
    loop = C.Loop(tracker.capacity)
    n = plain["count"].item()
    assert n == keep and held["track_id"].shape == held["labels"].shape
    seen = []
    for k in range(5):
        if k == 3:
            buf.copy_(shifted)
        for key in ("track_id", "track_hits"):
            held[key].fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        det = {key: held[key].cpu() for key in KEYS + ("track_id", "track_hits")}
        if k < 3:
            assert all(torch.equal(det[key], plain[key].cpu()) for key in KEYS)
        else:
            assert not torch.equal(det["boxes"], plain["boxes"].cpu()) and det["count"].item() > 2
        out = loop.update(det["count"].item(), det["scores"].flatten().double().tolist(),
                          det["labels"].flatten().tolist(), det["boxes"].reshape(-1, 4).double().tolist(),
                          **tracker.params)
        host = I.TrackState(*(t.cpu() for t in tracker.state.tensors()))
        C.check_frame(host, det["track_id"].flatten(), det["track_hits"].flatten(), out, loop.snapshot(), loop.M)
        det["next_id"] = host.next_id.item()
        seen.append(det)
    ids = seen[0]["track_id"].flatten()
    assert sorted(ids[:n].tolist()) == list(range(1, n + 1)) and not ids[n:].any()
    for k in (1, 2):
        assert torch.equal(seen[k]["track_id"], seen[0]["track_id"])
        assert seen[k]["track_hits"].flatten()[:n].tolist() == [k + 1] * n
    # after the first replay next_id stood still until the frame changed
    assert [d["next_id"] for d in seen[:3]] == [n + 1] * 3
    assert loop.births >= n and tracker.state.next_id.item() == 1 + loop.births
    assert loop.margins["iou"] >= 1e-3 and loop.margins["win"] >= 1e-3, loop.margins
    assert ref.n == 0
    live = tracker.tracks()
    print(f"[track] {'track_tiled (3, 2)' if tiled else 'track_image'} 97x131, one graph: {n} detections with stable "
          f"ids and hits 1, 2, 3 on the unchanged frame, {seen[3]['count'].item()} on the shifted one, "
          f"{loop.births - n} of them new; {len(live)} live tracks; outputs and state equal to the loop's on every "
          f"replay; margins {C.fmt(loop.margins)}")
    del graph
