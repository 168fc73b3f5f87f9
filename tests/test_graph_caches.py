"""The lifetime of the per-size device tensors that a captured graph reads by address (no GPU needed):
``YolosSmall.position_embeddings``, ``token_template``, ``_target_sizes`` and ``ops.image._device_tables``
all sit on ``ops.graph_cache.GraphCache``. What one of them hands out while the stream is capturing
stays the same object at the same address with the same contents, however many other sizes follow,
until ``invalidate_cache()`` or a parameter-version change; what was only used eagerly is bounded.

The capturing predicate is forced through ``graph_cache.is_capturing``, which every cache consults
per call, so the rule is tested on CPU tensors."""
import copy

import pytest
import torch

from walkai_nos_amd.models.workload.processor import YolosProcessor
from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
from walkai_nos_amd.ops import graph_cache
from walkai_nos_amd.ops import image as I

CPU = torch.device("cpu")
A_HW, A_SRC = (80, 96), (48, 64)
#: 20 other sizes: (resized H, W) in whole patches, and a source size of its own each
OTHERS = [((16 * (1 + n % 5), 16 * (2 + n // 5)), (11 + n, 23 + 2 * n)) for n in range(20)]


@pytest.fixture
def model():
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=1, use_mid_position_embeddings=True)).eval()
    m.processor = YolosProcessor(80, 133)
    return m


@pytest.fixture(autouse=True)
def clean_tables():
    I._tables.clear()
    yield
    I._tables.clear()


def fetch(m, hw, src):
    """Every per-size tensor of one image size, as ``detect_image`` fetches them."""
    pe, mid = m.position_embeddings(hw)
    tabs = I._device_tables(src[0], src[1], hw[0], hw[1], 16, CPU)
    return [pe, mid, m.token_template(hw), m._target_sizes(torch.zeros((1,) + src + (3,), dtype=torch.uint8))] \
        + list(tabs[:4])


def test_others_are_distinct_sizes():
    assert len(set(OTHERS)) == 20 and A_HW not in [o[0] for o in OTHERS] and A_SRC not in [o[1] for o in OTHERS]
    assert len({o[0] for o in OTHERS}) == 20 and len({o[1] for o in OTHERS}) == 20
    assert all(I.fusable(src, hw, 16) for hw, src in OTHERS)


def test_tensors_handed_out_under_capture_survive_other_sizes(model, monkeypatch):
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: True)
    held = fetch(model, A_HW, A_SRC)
    ptrs = [t.data_ptr() for t in held]
    copies = [t.clone() for t in held]
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: False)
    for hw, src in OTHERS:                      # eager traffic of 20 other sizes
        fetch(model, hw, src)
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: True)
    for hw, src in OTHERS[:3]:                  # and other captures
        fetch(model, hw, src)
    again = fetch(model, A_HW, A_SRC)
    for t, u, ptr, c in zip(held, again, ptrs, copies):
        assert u is t and u.data_ptr() == ptr and torch.equal(u, c)
    # the template is what the parameters say (not a block that was recycled)
    pe, _ = model.position_embeddings(A_HW)
    assert torch.equal(again[2][:, :1], model.cls_token + pe[:, :1])
    assert again[3].tolist() == [[48.0, 64.0]]


def test_an_eagerly_made_entry_is_pinned_when_a_capture_uses_it(model, monkeypatch):
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: False)
    held = fetch(model, A_HW, A_SRC)            # the warm-up run before a capture
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: True)
    assert all(u is t for t, u in zip(held, fetch(model, A_HW, A_SRC)))
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: False)
    for hw, src in OTHERS:
        fetch(model, hw, src)
    assert all(u is t for t, u in zip(held, fetch(model, A_HW, A_SRC)))


def test_unpinned_entries_are_bounded(model, monkeypatch):
    from walkai_nos_amd.models.workload.yolos import CACHED_SIZES
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: False)
    first = fetch(model, A_HW, A_SRC)
    for hw, src in OTHERS:
        fetch(model, hw, src)
    for cache in (model._pos_cache, model._tok_cache, model._ts_cache):
        assert cache.bound == CACHED_SIZES and len(cache) == cache.unpinned() == CACHED_SIZES
    assert I._tables.bound == 16 and len(I._tables) == I._tables.unpinned() == 16
    # the least recently used went first: A is made anew, the last size is still there
    assert all(u is not t for t, u in zip(first, fetch(model, A_HW, A_SRC)))
    last = fetch(model, *OTHERS[-1])
    assert all(u is t for t, u in zip(last, fetch(model, *OTHERS[-1])))
    # pinned entries do not count against the bound
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: True)
    for hw, src in OTHERS[:6]:
        fetch(model, hw, src)
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: False)
    for hw, src in OTHERS[6:]:
        fetch(model, hw, src)
    assert len(model._pos_cache) == 6 + CACHED_SIZES and model._pos_cache.unpinned() == CACHED_SIZES
    assert 14 <= I._tables.unpinned() <= 16 and len(I._tables) == 6 + I._tables.unpinned()
    key = (OTHERS[0][1] + OTHERS[0][0] + (16, "cpu"))
    assert I._tables.pinned(key) and not I._tables.pinned((OTHERS[19][1] + OTHERS[19][0] + (16, "cpu")))


def test_invalidate_cache_drops_pinned_entries(model, monkeypatch):
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: True)
    held = fetch(model, A_HW, A_SRC)
    model.invalidate_cache()
    I.invalidate_cache()
    for cache in (model._pos_cache, model._tok_cache, model._ts_cache, I._tables):
        assert len(cache) == 0
    again = fetch(model, A_HW, A_SRC)
    assert all(u is not t for t, u in zip(held, again)) and all(torch.equal(u, t) for t, u in zip(held, again))


def test_a_parameter_version_change_makes_pinned_entries_stale(model, monkeypatch):
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: True)
    pe, mid, tok = fetch(model, A_HW, A_SRC)[:3]
    fetch(model, *OTHERS[0])
    with torch.no_grad():
        model.pos_embed.add_(1.0)
    pe2, _, tok2 = fetch(model, A_HW, A_SRC)[:3]
    assert pe2 is not pe and torch.equal(pe2, pe + 1.0) and tok2 is not tok
    assert len(model._pos_cache) == 1 and len(model._tok_cache) == 1      # the other size's old version left too
    with torch.no_grad():
        model.det_tokens.add_(1.0)              # only the template reads the detection tokens
    pe3, _, tok3 = fetch(model, A_HW, A_SRC)[:3]
    assert pe3 is pe2 and tok3 is not tok2 and torch.equal(tok3[:, -100:], model.det_tokens + pe2[:, -100:])


def test_a_copied_model_starts_with_caches_of_its_own(model, monkeypatch):
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: True)
    held = fetch(model, A_HW, A_SRC)
    twin = copy.deepcopy(model)
    assert len(twin._pos_cache) == 0 and twin._pos_cache is not model._pos_cache
    assert all(u is not t for t, u in zip(held[:4], fetch(twin, A_HW, A_SRC)[:4]))
    assert all(u is t for t, u in zip(held, fetch(model, A_HW, A_SRC)))


def test_graph_cache_rules():
    flag = [False]
    c = graph_cache.GraphCache(2, capturing=lambda: flag[0])
    made = []

    def make(k):
        def f():
            made.append(k)
            return [k]
        return f
    a = c.get("a", make("a"))
    assert c.get("a", make("a")) is a and made == ["a"] and not c.pinned("a")
    c.get("b", make("b"))
    c.get("a", make("a"))                       # a is now the most recently used
    c.get("c", make("c"))                       # so b goes
    assert "a" in c and "b" not in c and "c" in c and len(c) == 2
    flag[0] = True
    assert c.get("a", make("a")) is a and c.pinned("a")
    flag[0] = False
    for k in "defgh":
        c.get(k, make(k))
    assert c.get("a", make("a")) is a and len(c) == 3 and c.unpinned() == 2
    c.get(("x", 1), make("x1"), stale=lambda k: k == "a")      # stale beats pinned
    assert "a" not in c and not c.pinned("a")
    assert c.get("none", lambda: None) is None and "none" in c   # None is a value like any other
    c.clear()
    assert len(c) == 0 and c.unpinned() == 0
    with pytest.raises(ValueError):
        graph_cache.GraphCache(0)
    # before the GPU is initialised the default predicate answers without touching it
    if not torch.cuda.is_initialized():
        assert graph_cache.is_capturing() is False and not torch.cuda.is_initialized()
