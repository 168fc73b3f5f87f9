"""The detection tail on the CPU: the last block computed on the detection rows only
(``YolosSmall.encode_detection``, ``_Block.forward_tail``) against the plain fp64 forward of
``tests/yolos_reference.py``, the shape rule that takes it, and its overrides. On the CPU the ops take
their torch form, so this covers the wiring: which rows feed the attention, the residuals and the heads.

The bound is the yardstick's: ``4 x own``, ``own`` being what the reference file's own formula loses
in plain fp32 against fp64 on the same input."""
import pytest
import torch

import yolos_reference as R
from walkai_nos_amd.models.workload import yolos as Y

NAMES = ("hidden", "logits", "boxes")
_own = {}


def own_error(layers, inp):
    """``(px, ref64, own per output)``: ``own`` the fp32 formula's max abs error against the fp64 one."""
    key = (layers,) + tuple(inp)
    if key not in _own:
        px, ref, _ = R.reference(layers, *inp)
        m = R.model(layers)
        f32 = R.forward(m.state_dict(), m.c, px, dtype=torch.float32)
        _own[key] = (px, ref, tuple((g.double() - r).abs().max().item() for g, r in zip(f32, ref)))
    return _own[key]


@pytest.fixture
def tail():
    """``set_detection_tail`` with the override taken back afterwards."""
    yield Y.set_detection_tail
    Y.set_detection_tail(None)


class Calls:
    def __init__(self, monkeypatch, owner, name):
        self.n = 0
        fn = getattr(owner, name)

        def spy(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        monkeypatch.setattr(owner, name, spy)


@pytest.mark.parametrize("inp", R.INPUTS, ids=lambda i: "x".join(map(str, i)))
@pytest.mark.parametrize("layers", R.LAYERS)
def test_forced_tail_matches_the_fp64_reference(tail, monkeypatch, layers, inp):
    px, ref, own = own_error(layers, inp)
    m = R.model(layers)
    nd = m.c.num_detection_tokens
    ran = Calls(monkeypatch, Y._Block, "forward_tail")
    tail(True)
    with torch.no_grad():
        logits, boxes = m(px)
        det = m.encode_detection(px)
        full = m.encode(px)
    assert ran.n == 2                      # forward and encode_detection took the tail; encode did not
    assert full.shape == ref[0].shape and det.shape == (inp[2], nd, m.c.hidden_size)
    for name, got, r, o in (("logits", logits, ref[1], own[1]), ("boxes", boxes, ref[2], own[2]),
                            ("tail rows", det, ref[0][:, -nd:], own[0]),
                            ("tail rows vs encode", det, full[:, -nd:].double(), own[0])):
        err = (got.double() - r).abs().max().item()
        print(f"[tail] L={layers} {inp} {name}: err {err:.3g}, own {o:.3g}")
        assert got.shape == r.shape and err <= 4.0 * o, (name, err, o)


def test_rule_truth_table():
    nd = R.config().num_detection_tokens
    assert nd == 100
    table = {128: False, 129: False, 224: False, 225: True, 257: True, 3401: True}
    assert {T: Y.detection_tail_rule(T, nd) for T in table} == table
    # the inputs of the wiring tests land on both sides
    assert not Y.detection_tail_rule(R.tokens(64, 112), nd) and Y.detection_tail_rule(R.tokens(192, 208), nd)


@pytest.mark.parametrize("inp,taken", [(R.INPUTS[1], False), (R.INPUTS[2], True)], ids=["T129", "T257"])
def test_rule_decides_without_an_override(monkeypatch, inp, taken):
    monkeypatch.delenv("NOS_DET_TAIL", raising=False)
    Y.set_detection_tail(None)
    px = R.pixels(*inp)
    m = R.model(2)
    ran = Calls(monkeypatch, Y._Block, "forward_tail")
    with torch.no_grad():
        logits, boxes = m(px)
        assert ran.n == (1 if taken else 0)
        want = m.detect(m.encode(px))
    assert ran.n == (1 if taken else 0)   # encode never takes it
    if not taken:  # forward is literally detect(encode(x))
        assert torch.equal(logits, want[0]) and torch.equal(boxes, want[1])


def test_env_override_off_is_detect_of_encode_bit_for_bit(monkeypatch):
    # read at every forward, not at import
    px = R.pixels(*R.INPUTS[2])
    m = R.model(3)
    ran = Calls(monkeypatch, Y._Block, "forward_tail")
    Y.set_detection_tail(None)
    monkeypatch.setenv("NOS_DET_TAIL", "0")
    with torch.no_grad():
        logits, boxes = m(px)
        want = m.detect(m.encode(px))
    assert ran.n == 0
    assert torch.equal(logits, want[0]) and torch.equal(boxes, want[1])
    monkeypatch.setenv("NOS_DET_TAIL", "1")
    with torch.no_grad():
        m(R.pixels(*R.INPUTS[1]))            # T = 129: forced on against the rule
    assert ran.n == 1


def test_setter_wins_over_the_environment(tail, monkeypatch):
    monkeypatch.setenv("NOS_DET_TAIL", "1")
    tail(False)
    assert not Y.detection_tail(3401, 100)
    tail(True)
    monkeypatch.setenv("NOS_DET_TAIL", "0")
    assert Y.detection_tail(129, 100)
    tail(None)
    assert not Y.detection_tail(3401, 100)
    monkeypatch.delenv("NOS_DET_TAIL")
    assert Y.detection_tail(3401, 100) and not Y.detection_tail(129, 100)


def test_attention_ref_window_is_the_rows_of_the_full_attention():
    from walkai_nos_amd.ops import kernels as K
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(2, 77, 3 * 2 * 64, generator=g)
    full = K.attention_ref(qkv, 2, 64, 0.125)
    for q0, n in ((0, 77), (5, 40), (76, 1)):
        win = K.attention_ref(qkv, 2, 64, 0.125, q0, n)
        assert win.shape == (2, n, 128)
        assert torch.allclose(win, full[:, q0:q0 + n], rtol=0, atol=1e-6)
        planes = K.attention_qkv_x3f(qkv, 2, 64, 0.125, q0=q0, q_rows=n)
        assert torch.equal(planes, K.split3(win))
        assert torch.equal(K.attention_qkv_x3(K.split3(qkv), 2, 64, 0.125, q0=q0, q_rows=n), planes)
    for q0, n in ((-1, 4), (3, 0), (70, 8)):
        with pytest.raises(ValueError):
            K.attention_ref(qkv, 2, 64, 0.125, q0, n)
