"""The appearance rules of ``ops.image`` on the CPU, on hand-made chips of a few pixels: the references of
``chip_features``, ``feature_overlap`` and ``track_update`` with features. Every comparison is equality."""
import pytest
import torch

from walkai_nos_amd.ops import image as I

ROW0 = torch.tensor([0], dtype=torch.int32)


def one_pixel(v):
    return torch.tensor([[[[v, 32, 32]]]], dtype=torch.uint8)


# value -> {red bin: weight of 16}: below the first centre, on the centres, between them, above the last
@pytest.mark.parametrize("v,bins", ((0, {0: 16}), (31, {0: 16}), (32, {0: 16}), (33, {0: 16}), (95, {0: 1, 1: 15}),
                                    (96, {1: 16}), (160, {2: 16}), (224, {3: 16}), (255, {3: 16}), (36, {0: 15, 1: 1})))
def test_a_channel_value_votes_into_two_bins(v, bins):
    f = I.chip_features_reference(one_pixel(v), ROW0, None, 1)[0]
    assert f.sum().item() == I.feature_total((1, 1)) == 4096
    assert {b // 16: w // 256 for b, w in enumerate(f.tolist()) if w} == bins   # green and blue sit in their bin 0


@pytest.mark.parametrize("size,stripes", (((7, 5), 4), ((7, 5), 1), ((8, 1), 8), ((3, 2), 2)))
def test_descriptors_sum_to_the_total_and_stripes_split_the_rows(size, stripes):
    g = torch.Generator().manual_seed(3)
    chips = torch.randint(0, 256, (3, *size, 3), generator=g, dtype=torch.uint8)
    rows = torch.tensor([4, -1, 0], dtype=torch.int32)
    f = I.chip_features_reference(chips, rows, None, stripes)
    assert f.dtype == torch.int32 and f.shape == (3, 64 * stripes)
    assert f.sum(1).tolist() == [I.feature_total(size), 0, I.feature_total(size)]
    heights = [(s + 1) * size[0] // stripes - s * size[0] // stripes for s in range(stripes)]
    assert (f[0].view(stripes, 64).sum(1) // (4096 * size[1])).tolist() == heights
    if (size, stripes) == ((7, 5), 4):
        assert heights == [1, 2, 2, 2]
    S = I.feature_overlap_reference(f, f)
    assert S.diagonal().tolist() == f.sum(1).tolist() and S[1].tolist() == [0, 0, 0] and torch.equal(S, S.t())


def test_track_reference_without_features_is_unchanged_and_with_them_follows_the_rule():
    g = torch.Generator().manual_seed(5)
    xy = torch.randint(0, 400, (12, 2), generator=g).float()
    lists = (torch.tensor([11], dtype=torch.int32), torch.rand(12, generator=g), torch.randint(0, 2, (12,),
             generator=g, dtype=torch.int32), torch.cat((xy, xy + 60.0), 1))
    a, b = I.track_state(16), I.track_state(16, features=64)
    for _ in range(3):
        plain = I.track_update_reference(a, *lists)
        more = I.track_update_reference(b, *lists, features=None, feature_rows=None, appearance_gate=0.5,
                                        reid_threshold=0.5, feature_shift=1)
        assert all(torch.equal(x, y) for x, y in zip(plain + a.tensors(), more + b.tensors()))
        lists = (lists[0], lists[1], lists[2], lists[3] + 4.0)
    assert not b.has.any() and not b.feat.any()
    # one red track; a frame without it; then red far away (the same track again) and blue further (a new one)
    st = I.track_state(2, features=64)
    red, blue = ((224, 32, 32), (32, 32, 224))
    kw = dict(reid_threshold=0.6, feature_total=4096, feature_shift=0)
    for boxes, colours, ids in (([[0, 0, 40, 40]], [red], [1]), ([], [], []), ([[500, 0, 540, 40]], [red], [1]),
                                ([[900, 0, 940, 40]], [blue], [2])):
        n = len(boxes)
        chips = torch.tensor(colours or [red], dtype=torch.uint8).view(-1, 1, 1, 3)
        rows = torch.arange(len(chips), dtype=torch.int32) if n else torch.tensor([-1], dtype=torch.int32)
        got = I.track_update(st, torch.tensor([n], dtype=torch.int32), torch.full((max(n, 1),), 0.9),
                             torch.ones(max(n, 1), dtype=torch.int32), torch.tensor(boxes or [[0.0] * 4]),
                             features=I.chip_features(chips, rows, None, 1), feature_rows=rows, **kw)
        assert got[0].tolist()[:n] == ids
    assert st.src.tolist() == [-1, 0] and st.has.tolist() == [1, 1] and st.misses.tolist() == [1, 0]
    st.reset()
    assert not any(t.any() for t in (st.feat, st.has, st.src, st.ids)) and len(st.tensors()) == 8
