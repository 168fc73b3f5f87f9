"""The appearance kernels on the GPU (``chip_features_k``, ``feature_overlap_k``, ``track_features_k`` of
``csrc/image_features.h`` and ``track_update_app_f32`` of ``csrc/image_track.h``) against the torch references of
``ops.image``. The rules are integers and the tracker scenes keep every fp32 operation exact (coordinates on a grid of
1/4 below 4096, ``velocity_gain`` 0.5), so every comparison is equality, and every one asserts that no reference was
taken by the op under test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RED, BLUE, GREEN = (224, 32, 32), (32, 32, 224), (32, 224, 32)
SIZE = (8, 4)           # the chips of the tracker scenes


@pytest.fixture(scope="module")
def I():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from walkai_nos_amd.ops import image, kernels
    assert image.hip_available(), "libnos_image.so must be built on a GPU box"
    kernels.set_backend("hip")
    return image


@pytest.fixture
def spies(I, monkeypatch):
    """The references, counted: ``spies()`` is the calls so far."""
    calls = []
    for name in ("chip_features_reference", "feature_overlap_reference", "track_update_reference",
                 "track_features_reference", "chips_reference"):
        fn = getattr(I, name)
        monkeypatch.setattr(I, name, lambda *a, _f=fn, **kw: (calls.append(_f.__name__), _f(*a, **kw))[1])
    return lambda: len(calls)


def some_chips(K, size, used, seed=0):
    """``K`` chips of random bytes — chip 0 all 255, chip 1 of two colours — with ``used`` slots, 0x7F behind them."""
    g = torch.Generator().manual_seed(seed)
    chips = torch.randint(0, 256, (K, *size, 3), generator=g, dtype=torch.uint8)
    chips[0] = 255
    if K > 1:
        chips[1, : size[0] // 2], chips[1, size[0] // 2:] = torch.tensor(RED, dtype=torch.uint8), 96
    chips[used:] = 0x7F
    rows = torch.where(torch.arange(K) < used, torch.arange(K) * 3, -1).to(torch.int32)
    return chips.cuda(), rows.cuda()


@pytest.mark.parametrize("size,stripes,K,used", (
    ((8, 1), 8, 3, 2), ((8, 1), 4, 1, 0), ((8, 1), 2, 1, 1), ((8, 1), 1, 3, 1), ((7, 5), 4, 3, 2), ((7, 5), 1, 256, 255),
    ((7, 5), 2, 3, 0), ((128, 64), 4, 256, 255), ((128, 64), 8, 3, 2), ((128, 64), 1, 1, 1), ((128, 64), 2, 3, 1),
    ((256, 256), 1, 3, 2), ((256, 256), 8, 3, 2)))
def test_chip_features(I, spies, size, stripes, K, used):
    chips, rows = some_chips(K, size, used)
    I.chip_features(chips, rows, None, stripes).fill_(0x7F7F7F7F)       # the cached buffer the next call writes
    got = I.chip_features(chips, rows, None, stripes)
    assert spies() == 0
    want = I.chip_features_reference(chips, rows, None, stripes)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    assert got.sum(1).tolist() == [I.feature_total(size)] * used + [0] * (K - used)
    # an unaligned view of the same bytes: the dword path's two ends
    if K == 3:
        shifted = torch.empty(chips.numel() + 1, dtype=torch.uint8, device="cuda")[1:].view(chips.shape).copy_(chips)
        assert torch.equal(I.chip_features(shifted, rows, None, stripes), want)


@pytest.mark.parametrize("K,T,D", ((1, 1, 64), (3, 65, 128), (33, 100, 512), (256, 1024, 512)))
def test_feature_overlap(I, spies, K, T, D):
    chips, rows = some_chips(K + T, SIZE, K + T, seed=K)
    f = I.chip_features_reference(chips, rows, None, D // 64)
    F, G = f[:K].clone(), f[K:].clone()
    G[T // 2] = 0
    F[K // 2] = 0 if K > 1 else F[0]
    G[T - 1] = F[0]                                                     # one identical pair
    before = spies()
    I.feature_overlap(F, G).fill_(0x7F7F7F7F)
    got = I.feature_overlap(F, G)
    assert spies() == before
    assert got.shape == (K, T) and torch.equal(got, I.feature_overlap_reference(F, G))
    assert got[0, T - 1].item() == I.feature_total(SIZE) and (T == 1 or not got[:, T // 2].any())


def lists_of(boxes, colours, K, N=None, labels=None):
    """One frame of a scene on the GPU: the lists (scores descending by row), flat-coloured chips for the first ``K``
    rows and their rows."""
    n, N = len(boxes), max(len(boxes), 1) if N is None else N
    pad = lambda t, fill: torch.cat((t, torch.full((N - n,) + t.shape[1:], fill, dtype=t.dtype)))      # noqa: E731
    scores = pad(0.9 - 0.5 * torch.arange(n) / max(n, 1), 0.0)
    labels = pad(torch.ones(n, dtype=torch.int32) if labels is None else labels, 0)
    boxes = pad(torch.tensor(boxes, dtype=torch.float32).view(-1, 4), 0.0)
    chips = torch.zeros((K, *SIZE, 3), dtype=torch.uint8)
    for k, c in enumerate(colours[:K]):
        chips[k] = torch.tensor(c, dtype=torch.uint8)
    rows = torch.where(torch.arange(K) < n, torch.arange(K), -1).to(torch.int32)
    return [t.cuda() for t in (torch.tensor([n], dtype=torch.int32), scores, labels, boxes, chips, rows)]


def run(I, spies, frames, T, K, kw, N=None):
    """The HIP route and the reference over ``frames`` on twin states: every field, ``track_id`` and ``track_hits``
    compared after each frame, and no reference taken by the HIP route. Returns the ids per frame and the final state."""
    kw = dict(velocity_gain=0.5, feature_total=I.feature_total(SIZE), **kw)
    a, b = I.track_state(T, "cuda", features=128), I.track_state(T, "cuda", features=128)
    ids = []
    for boxes, colours in frames:
        *lists, chips, rows = lists_of(boxes, colours, K, N)
        before = spies()
        f = I.chip_features(chips, rows, None, 2)
        got = I.track_update(a, *lists, features=f, feature_rows=rows, **kw)
        assert spies() == before
        want = I.track_update_reference(b, *lists, features=f, feature_rows=rows, **kw)
        for x, y in zip(got + a.tensors() + (a.feat, a.has, a.src), want + b.tensors() + (b.feat, b.has, b.src)):
            assert torch.equal(x, y), (len(ids), x, y)
        ids.append(got[0].tolist()[:len(boxes)])
    return ids, a


A, B, FAR = [0, 0, 40, 40], [10, 0, 50, 40], [500.25, 0, 540.25, 40]
CROSS = [([A, B], [RED, BLUE]), ([[8, 0, 48, 40], [2, 0, 42, 40]], [RED, BLUE])]       # IoU 2/3 with its own, 19/21
HIDDEN = [([A], [RED]), ([], []), ([], []), ([], [])]
TWO = [([A, [200, 0, 240, 40]], [RED, BLUE]), ([], [])]
SCENES = {
    # name: (frames, slots, chip capacity, parameters, the ids of every frame)
    "crossing boxes swap ids without a gate": (CROSS, 4, 4, dict(), [[1, 2], [2, 1]]),
    "and keep them with one": (CROSS, 4, 4, dict(appearance_gate=0.5), [[1, 2], [1, 2]]),
    "a hidden track reappears at IoU 0": (HIDDEN + [([FAR], [RED])], 4, 4, dict(reid_threshold=0.6),
                                          [[1], [], [], [], [1]]),
    "in other colours it is born anew": (HIDDEN + [([FAR], [BLUE])], 4, 4, dict(reid_threshold=0.6),
                                         [[1], [], [], [], [2]]),
    "no threshold, no re-identification": (HIDDEN + [([FAR], [RED])], 4, 4, dict(), [[1], [], [], [], [2]]),
    # only row 0 has a chip, so track 2 holds no descriptor and the gate cannot speak: the ids swap as without one
    "a candidate without a chip falls back to IoU": (CROSS, 4, 1, dict(appearance_gate=0.5), [[1, 2], [2, 1]]),
    # red at blue's place: blue's track overlaps (no gate), red's re-identifies with all of the descriptor
    "overlap beats a re-identification": (TWO + [([[204, 0, 244, 40]], [RED])], 4, 4, dict(reid_threshold=0.6),
                                          [[1, 2], [], [2]]),
    # two red tracks, both hidden; one red box far from both: the same sim, the lower slot
    "equal sim goes to the lower slot": ([([A, [200, 0, 240, 40]], [RED, RED]), ([], []), ([FAR], [RED])], 4, 4,
                                         dict(reid_threshold=0.6), [[1, 2], [], [1]]),
}


@pytest.mark.parametrize("name", SCENES)
def test_tracker_scenes(I, spies, name):
    frames, T, K, kw, want = SCENES[name]
    assert run(I, spies, frames, T, K, kw)[0] == want


@pytest.mark.parametrize("shift", (0, 2))
def test_descriptors_after_a_match_a_birth_and_a_death(I, spies, shift):
    # frame 1: the red track is matched by an orange box, green is born, blue (max_age 0) dies and frees slot 1
    frames = [([A, [200, 0, 240, 40]], [RED, BLUE]), ([[4, 0, 44, 40], [400, 0, 440, 40]], [(224, 96, 32), GREEN])]
    ids, st = run(I, spies, frames, 3, 4, dict(max_age=0, feature_shift=shift))
    assert ids == [[1, 2], [1, 3]] and st.src.tolist() == [0, 1, -1] and st.has.tolist() == [1, 1, 0]
    f = lambda c: I.chip_features_reference(torch.tensor(c, dtype=torch.uint8).expand(1, *SIZE, 3),       # noqa: E731
                                            torch.zeros(1, dtype=torch.int32), None, 2)[0].long()
    old, new = f(RED), f((224, 96, 32))
    assert st.feat[0].cpu().tolist() == (new if shift == 0 else old + ((new - old + 2) >> 2)).tolist()
    assert st.feat[1].cpu().tolist() == f(GREEN).tolist() and not st.feat[2].any()


def lattice(N, nframes=3, seed=0):
    """``N`` objects of random colours, 32 px in cells of 64, each moving by up to 1.5 px a frame in steps of 1/4 (an IoU
    of 0.7 or more with its own track, 0 with any other), rows shuffled in every frame, every fifth object hidden in
    frame 1."""
    g = torch.Generator().manual_seed(seed + N)
    cell = torch.arange(N)
    xy = torch.stack((64.0 * (cell % 32), 64.0 * (cell // 32)), 1) + 16.0
    colour = torch.randint(0, 256, (N, 3), generator=g)
    step = torch.randint(-6, 7, (N, 2), generator=g) / 4.0
    frames = []
    for k in range(nframes):
        who = torch.randperm(N, generator=g)
        who = who[who % 5 != 0] if k == 1 and N > 1 else who
        at = xy[who] + k * step[who]
        frames.append((torch.cat((at, at + 32.0), 1).tolist(), colour[who].tolist()))
    return frames


@pytest.mark.parametrize("N,T", ((1, 1), (65, 64), (1024, 1024)))
def test_tracker_rows_and_slots(I, spies, N, T):
    frames = lattice(N)
    ids, st = run(I, spies, frames, T, min(N, 256), dict(appearance_gate=0.5, reid_threshold=0.6, max_age=1), N=N)
    assert st.next_id.item() == min(N, T) + 1
    assert sorted(ids[2]) == sorted(ids[0])     # everything that fitted is found again, the hidden fifth included


def test_one_graph_of_the_four_launches(I, spies):
    kw = dict(velocity_gain=0.5, feature_total=I.feature_total(SIZE), appearance_gate=0.5, reid_threshold=0.6, max_age=1)
    state, twin = I.track_state(64, "cuda", features=128), I.track_state(64, "cuda", features=128)
    static = lists_of(*lattice(48)[0], 32, 48)
    I.track_update(state, *static[:4], features=I.chip_features(*static[4:], None, 2), feature_rows=static[5], **kw)
    state.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        held = I.track_update(state, *static[:4], features=I.chip_features(*static[4:], None, 2),
                              feature_rows=static[5], **kw)
    assert spies() == 0
    for seed in (1, 2):
        state.reset(), twin.reset()
        for frame in lattice(48, 10, seed):
            for dst, src in zip(static, lists_of(*frame, 32, 48)):
                dst.copy_(src)
            graph.replay()
            want = I.track_update_reference(twin, *static[:4], feature_rows=static[5], **kw,
                                            features=I.chip_features_reference(*static[4:], None, 2))
            for x, y in zip(held + state.tensors() + (state.feat, state.has, state.src),
                            want + twin.tensors() + (twin.feat, twin.has, twin.src)):
                assert torch.equal(x, y)
    assert state.next_id.item() > 48
    del graph


def test_track_image_with_an_appearance_is_the_composition_of_the_ops(I, spies):
    from yolos_reference import randomize
    from walkai_nos_amd.models.workload.processor import YolosProcessor
    from walkai_nos_amd.models.workload.tracker import Appearance, Tracker
    from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
    model = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=2, use_mid_position_embeddings=True)).eval()
    randomize(model)
    model.invalidate_cache()
    model.processor = YolosProcessor(80, 133)
    model = model.cuda()
    looks = Appearance(size=(16, 8), capacity=32, stripes=2, gate=0.25, reid_threshold=0.6)
    tracker, twin = (Tracker(capacity=64, device="cuda", appearance=looks) for _ in range(2))
    g = torch.Generator().manual_seed(13)
    frame = torch.randint(0, 256, (97, 131, 3), generator=g, dtype=torch.uint8)
    buf = frame.cuda()
    with torch.no_grad():
        s = model.detect_image(buf, 0.0)["scores"].flatten().sort().values
        thr = 0.5 * (s[-13] + s[-12]).item()
        model.track_image(buf, tracker, thr)
        tracker.reset()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
            held = model.track_image(buf, tracker, thr)
        tracker.reset()
        for k in range(4):
            if k == 2:
                buf.copy_(torch.roll(frame, (3, 5), (0, 1)))
            graph.replay()
            det = model.detect_image(buf, thr)
            lists = (det["count"], det["scores"], det["labels"], det["boxes"])
            chips, rows, _, n = I.chips(buf, *lists, size=(16, 8), select=looks.chips.select("cuda"), capacity=32)
            want = I.track_update(twin.state, *lists, **twin.params, **looks.params, feature_rows=rows,
                                  features=I.chip_features(chips, rows, n, 2))
            assert torch.equal(held["track_id"].flatten(), want[0]) and torch.equal(held["track_hits"].flatten(), want[1])
            a, b = tracker.state, twin.state
            assert all(torch.equal(x, y) for x, y in zip(a.tensors() + (a.feat, a.has, a.src),
                                                         b.tensors() + (b.feat, b.has, b.src)))
    assert spies() == 0 and tracker.state.has.any() and held["track_id"].max().item() >= 12
    del graph
