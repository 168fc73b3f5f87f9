"""The detection tail on the GPU: ``YolosSmall.forward`` / ``encode_detection`` / ``detect_image`` with
the last block on the detection rows only (windowed x3 attention, the three GEMMs at M = nd * B)
against the plain fp64 forward of ``tests/yolos_reference.py``. The conventions are those of
``tests/test_gpu_model_paths.py``: ``R.reference`` gives the input, the fp64 outputs and ``err_ref``
(the same model in plain fp32 on the CPU); a path passes within ``4 x err_ref``, floor
``2e-6 * max(1, |ref|max)``."""
import pytest
import torch

import yolos_reference as R
from kernel_inputs import Worst
from test_gpu_model_paths import CROSS, T129, T257, Calls, Forced, gpu_model, restore

from walkai_nos_amd.models.workload import yolos as Y

pytestmark = pytest.mark.gpu

NAMES = ("tail rows", "logits", "boxes")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from walkai_nos_amd.ops import kernels
    assert kernels.hip_available(), "libnos_kernels.so must be built on a GPU box"
    restore(kernels)
    yield kernels
    restore(kernels)
    Y.set_detection_tail(None)


class Windowed:
    """Counts the windowed calls (``q_rows`` given) of ``K.<name>``."""

    def __init__(self, monkeypatch, K, name):
        self.n = self.full = 0
        fn = getattr(K, name)

        def spy(*a, **kw):
            if kw.get("q_rows") is not None:
                self.n += 1
            else:
                self.full += 1
            return fn(*a, **kw)
        monkeypatch.setattr(K, name, spy)


def run_tail(m, px):
    with torch.no_grad():
        det = m.encode_detection(px)
        logits, boxes = m(px)
    torch.cuda.synchronize()
    return det, logits, boxes


def check_tail(wst, layers, inp, tag=()):
    px, ref, err_ref = R.reference(layers, *inp)
    m = gpu_model(layers)
    nd = m.c.num_detection_tokens
    got = run_tail(m, px.cuda())
    want = (ref[0][:, -nd:], ref[1], ref[2])
    for name, g, r, e in zip(NAMES, got, want, err_ref):
        assert g.shape == r.shape, (name, g.shape, r.shape)
        err = (g.double().cpu() - r).abs().max().item()   # NaN survives max(): it fails the bound
        wst.check(err, e, 2e-6 * max(1.0, r.abs().max().item()), (layers,) + tuple(inp) + tuple(tag) + (name,))


@pytest.mark.parametrize("inp", R.INPUTS, ids=lambda i: "x".join(map(str, i)))
@pytest.mark.parametrize("layers", R.LAYERS)
def test_forced_tail_default_path(K, monkeypatch, layers, inp):
    # the tail forced on at every input (T = 116 x 2 ... 257) and depth; 1 layer: no h3 handed in
    # Measured worst err/err_ref (bound 4) over the 18 cases: 2.01 (L = 1, T = 129, tail rows); the run is kept
    # in profiles/pytest_gpu_det_tail.log.
    monkeypatch.setenv("NOS_SPLITK", "0")
    win = Windowed(monkeypatch, K, "attention_qkv_x3f")
    wst = Worst(f"tail forced L={layers} {inp}", label="tail")
    try:
        Y.set_detection_tail(True)
        check_tail(wst, layers, inp)
        assert win.n == 2 and win.full == 2 * (layers - 1)   # encode_detection and forward, one window each
    finally:
        Y.set_detection_tail(None)
        restore(K)
    wst.done()


def test_forced_tail_with_timed_pipelines(K, monkeypatch):
    # NOS_SPLITK unset: the projection / fc2 timers run at M = nd too (split counts 6 and 8 on offer)
    from walkai_nos_amd.ops import gemm as G
    monkeypatch.delenv("NOS_SPLITK", raising=False)
    monkeypatch.setattr(G, "_fused_cache", {})
    wst = Worst("tail forced, timed pipelines", label="tail")
    try:
        Y.set_detection_tail(True)
        K.set_slice_cus(K.total_cus())
        check_tail(wst, 3, T257)
        print("[tail] the timer chose:", G.fused_table())
        assert {k[0] for k in G._fused_cache} == {257, 100}
    finally:
        Y.set_detection_tail(None)
        restore(K)
    wst.done()


@pytest.mark.parametrize("splits", [2, 8])
def test_forced_tail_with_forced_split_k(K, monkeypatch, splits):
    # split-K partials + combine-and-LayerNorm in every projection / fc2 step, the tail's included:
    # 2 splits for both depths, and the largest count each depth takes of those offered at M <= 128
    from walkai_nos_amd.ops import gemm as G
    choices = {}
    for Kd in (384, 1536):
        base = G.split_candidates(384, Kd)
        cands = base if splits == 2 else G.small_m_split_candidates(base, Kd)
        c, sp = cands[0] if splits == 2 else max(cands, key=lambda x: x[1])
        choices[Kd] = ("split", c, sp)
    assert splits == 2 or (choices[384][2], choices[1536][2]) == (6, 8)
    forced = Forced(choices)
    monkeypatch.setattr(G, "_fused_cache", forced)
    wst = Worst(f"tail forced, split-K {sorted(choices.values())}", label="tail")
    try:
        Y.set_detection_tail(True)
        K.set_slice_cus(K.total_cus())
        for inp in CROSS:
            check_tail(wst, 3, inp, (splits,))
        assert {k[2] for k in forced.keys} == {384, 1536} and len(forced.keys) == 2 * 6 * len(CROSS)
        assert {k[0] for k in forced.keys} >= {100, 200}
    finally:
        Y.set_detection_tail(None)
        restore(K)
    wst.done()


def test_forced_tail_planes_in_attention(K, monkeypatch):
    # NOS_ATTN_F32IN=0: the QKV GEMM writes planes and the planes-in kernel takes the window
    monkeypatch.setenv("NOS_ATTN_F32IN", "0")
    monkeypatch.setenv("NOS_SPLITK", "0")
    win = Windowed(monkeypatch, K, "attention_qkv_x3")
    wst = Worst("tail forced, planes-in attention", label="tail")
    try:
        Y.set_detection_tail(True)
        assert not K.attention_input_f32()
        for inp in CROSS:
            check_tail(wst, 3, inp)
        assert win.n == 2 * len(CROSS)
    finally:
        Y.set_detection_tail(None)
        restore(K)
    wst.done()


def test_rule_takes_the_tail_at_t257_and_not_at_t129(K, monkeypatch):
    monkeypatch.delenv("NOS_DET_TAIL", raising=False)
    monkeypatch.setenv("NOS_SPLITK", "0")
    Y.set_detection_tail(None)
    win = Windowed(monkeypatch, K, "attention_qkv_x3f")
    m = gpu_model(3)
    try:
        with torch.no_grad():
            m(R.reference(3, *T257)[0].cuda())
            assert (win.n, win.full) == (1, 2)
            m(R.reference(3, *T129)[0].cuda())
            assert (win.n, win.full) == (1, 5)
            # a setting the window does not cover runs the full block
            monkeypatch.setenv("NOS_ATTN_PROJ_FUSED", "1")
            m(R.reference(3, *T257)[0].cuda())
            assert win.n == 1
        torch.cuda.synchronize()
    finally:
        restore(K)


def test_graph_replay_of_forward_equals_the_eager_run(K, monkeypatch):
    monkeypatch.delenv("NOS_DET_TAIL", raising=False)
    Y.set_detection_tail(None)
    px, ref, err_ref = R.reference(3, *T257)
    m, x = gpu_model(3), px.cuda()
    win = Windowed(monkeypatch, K, "attention_qkv_x3f")
    wst = Worst("tail, graph replay", label="tail")
    try:
        with torch.no_grad():
            eager = [t.clone() for t in m(x)]
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            with torch.no_grad():
                held = m(x)
        assert win.n == 2
        for rep in range(2):
            for t in held:
                t.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            for name, h, e, r, er in zip(NAMES[1:], held, eager, ref[1:], err_ref[1:]):
                assert torch.equal(h, e), (name, rep)
                wst.check((h.double().cpu() - r).abs().max().item(), er, 2e-6 * max(1.0, r.abs().max().item()),
                          (name, rep))
        del graph
    finally:
        restore(K)
    wst.done()


def test_detect_image_is_the_model_on_the_kernel_pixels_with_the_tail(K, monkeypatch):
    # 96x104 -> 192x208 (T = 257, where the rule takes the tail): the fused image path and the model on
    # the kernel's pixels go through the same tail
    from walkai_nos_amd.models.workload.processor import YolosProcessor
    from walkai_nos_amd.ops import image as I
    monkeypatch.delenv("NOS_DET_TAIL", raising=False)
    Y.set_detection_tail(None)
    m = R.model(2)
    m.processor = YolosProcessor(192, 333)
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (96, 104, 3), generator=g, dtype=torch.uint8).cuda()
    assert m.processor.size((96, 104)) == (192, 208) and R.tokens(192, 208) == 257
    fused = Calls(monkeypatch, I, "image_patch_planes")
    win = Windowed(monkeypatch, K, "attention_qkv_x3f")
    try:
        with torch.no_grad():
            out = m.detect_image(img, 0.0)
            assert fused.n == 1 and win.n == 1
            px = m.processor.preprocess(img)
            logits, boxes = m(px)
            rows = m.encode_detection_image(img)
            every = m.encode_image(img)
        torch.cuda.synchronize()
        assert win.n == 3 and px.shape == (1, 3, 192, 208)
        assert torch.equal(out["logits"], logits) and torch.equal(out["pred_boxes"], boxes)
        assert rows.shape == (1, 100, 384) and every.shape == (1, 257, 384)
        assert not torch.isnan(logits).any() and out["count"].tolist() == [100]
    finally:
        restore(K)
