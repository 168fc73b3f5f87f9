"""The YOLOS forward on every path its dispatch can take (GPU only), with every parameter
distinguishable: no zero bias, no unit LayerNorm, mid position embeddings on, 1 / 2 / 3 layers of one
parameter set (``tests/yolos_reference.py``). Every check compares ``encode``'s full ``[B, T, D]``
output (the last block's class and patch rows included), the logits and the boxes with the plain fp64
forward of the same state dict.

The bound follows ``tests/test_gpu_kernel_edges.py``: ``err_ref`` is the error of the same model in
plain fp32 on the CPU against that reference, computed once per (layers, input); a path passes within
``factor * err_ref`` (factor 4 unless the test says why not), floor ``2e-6 * max(1, |ref|max)``.
The worst measured ``err / err_ref`` of each path stands beside its bound: the largest of three runs
on an MI355X, whose figures differ by a few tenths with the tiles the timers pick. The last of them is
kept in ``profiles/pytest_gpu_model_paths.log``, one ``[model]`` line per test, the tiles and
pipelines the timers chose at its end."""
import pytest
import torch

import yolos_reference as R
from kernel_inputs import Worst
from test_gpu_kernel_edges import restore_attention

pytestmark = pytest.mark.gpu

#: (H, W, batch) of ``R.INPUTS`` by what they are for
T128, T129, T257, CROPPED, ODD_WIDTH, BATCH2 = R.INPUTS
#: the reduced cross of paths (b)-(i): tile-exact, one past 128, one past 256, and the batch path
CROSS = (T128, T129, T257, BATCH2)
NAMES = ("hidden", "logits", "boxes")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from walkai_nos_amd.ops import gemm as G
    from walkai_nos_amd.ops import kernels
    assert kernels.hip_available(), "libnos_kernels.so must be built on a GPU box"
    restore(kernels)
    yield kernels
    restore(kernels)
    print("[model] x3 tiles:", G.x3_table())
    print("[model] projection / fc2 pipelines:", G.fused_table())


def restore(K):
    restore_attention(K)
    K.set_attention_head_block(None)
    K.set_fp32_matmul("x3")
    K.set_backend("hip")
    K.set_slice_pin(0)
    K.set_slice_cus(None)


_gpu_models = {}


def gpu_model(layers):
    if layers not in _gpu_models:
        _gpu_models[layers] = R.model(layers).cuda().eval()
    return _gpu_models[layers]


def run(m, px):
    with torch.no_grad():
        hidden = m.encode(px)
        logits, boxes = m.detect(hidden)
    torch.cuda.synchronize()
    return hidden, logits, boxes


def compare(wst, got, ref, err_ref, tag):
    for name, g, r, e in zip(NAMES, got, ref, err_ref):
        assert g.shape == r.shape, (tag, name, g.shape, r.shape)
        err = (g.double().cpu() - r).abs().max().item()   # NaN survives max(): it fails the bound
        wst.check(err, e, 2e-6 * max(1.0, r.abs().max().item()), tag + (name,))


def check(wst, layers, inp, tag=()):
    px, ref, err_ref = R.reference(layers, *inp)
    compare(wst, run(gpu_model(layers), px.cuda()), ref, err_ref, (layers,) + tuple(inp) + tuple(tag))


class Calls:
    """Counts the calls of ``owner.name`` (and keeps their results): that a path ran, not only passed."""

    def __init__(self, monkeypatch, owner, name):
        self.n, self.results = 0, []
        fn = getattr(owner, name)

        def spy(*a, **kw):
            self.n += 1
            out = fn(*a, **kw)
            self.results.append(out if out is None or isinstance(out, (bool, int)) else True)
            return out
        monkeypatch.setattr(owner, name, spy)


class Forced:
    """Stands in for ``gemm._fused_cache``: every key gets the pipeline forced for its K."""

    def __init__(self, by_k):
        self.by_k, self.keys = by_k, []

    def get(self, key, default=None):
        self.keys.append(key)
        return self.by_k[key[2]]


# ---- (a) the default x3 path, unsplit pipeline ----------------------------------------------------
@pytest.mark.parametrize("inp", R.INPUTS, ids=lambda i: "x".join(map(str, i)))
@pytest.mark.parametrize("layers", R.LAYERS)
def test_default_x3_unsplit(K, monkeypatch, layers, inp):
    # forward_x3 with the LayerNorms folded into the producing step; 1 layer: no h3 in and no next_ln
    # in one block; 2: apart; 3: a middle block with both. B = 1 runs the token template, the fused
    # heads and (even width) patch_planes; B = 2 torch.cat and the module heads; odd width im2col.
    # Measured worst err/err_ref (bound 4) over the 18 cases: 2.82 (L = 2, odd width, hidden).
    from walkai_nos_amd.ops import gemm as G
    monkeypatch.setenv("NOS_SPLITK", "0")
    monkeypatch.setattr(G, "_fused_cache", {})
    heads = Calls(monkeypatch, K, "detection_heads")
    planes = Calls(monkeypatch, K, "patch_planes")
    wst = Worst(f"(a) x3 unsplit L={layers} {inp}", label="model")
    try:
        check(wst, layers, inp)
        m = gpu_model(layers)
        assert K.x3_active(m.pos_embed) and not G._fused_cache   # nothing timed: ("unsplit",) every time
        assert heads.n == (1 if inp[2] == 1 else 0)
        assert planes.results == [None if inp[1] % 2 else True]
        if inp == T129:   # forward is encode + detect, bit for bit
            px = R.reference(layers, *inp)[0].cuda()
            with torch.no_grad():
                got, (logits, boxes) = run(m, px), m(px)
            assert torch.equal(got[1], logits) and torch.equal(got[2], boxes)
    finally:
        restore(K)
    wst.done()


# ---- (b), (c) forced projection / fc2 pipelines ---------------------------------------------------
def force(monkeypatch, choices):
    from walkai_nos_amd.ops import gemm as G
    forced = Forced(choices)
    monkeypatch.setattr(G, "_fused_cache", forced)
    return forced


@pytest.mark.parametrize("cus", [64, 256])
@pytest.mark.parametrize("which,splits", [("first", 2), ("last", 4)])
def test_forced_split_k(K, monkeypatch, which, splits, cus):
    # the split-K partial GEMM + combine-and-LayerNorm kernel in both steps of every block (with mid
    # as the second residual, broadcast by m % rows at B = 2): the first (64x64 tile, 2 splits) and
    # last (256x128 tile, 4 splits) candidate of each shape.
    # Measured worst err/err_ref (bound 4): 1.58 / 1.46 (2 splits, 64 / 256 CUs), 1.32 / 1.37 (4 splits).
    from walkai_nos_amd.ops import gemm as G
    choices = {}
    for Kd in (384, 1536):
        c, sp = G.split_candidates(384, Kd)[0 if which == "first" else -1]
        assert sp == splits
        choices[Kd] = ("split", c, sp)
    assert cus >= G.SPLITK_MIN_CUS
    forced = force(monkeypatch, choices)
    wst = Worst(f"(b) split-K {sorted(choices.values())} cus={cus}", label="model")
    try:
        K.set_slice_cus(cus)
        for inp in CROSS:
            check(wst, 3, inp, (which, cus))
        assert {k[2] for k in forced.keys} == {384, 1536} and len(forced.keys) == 6 * len(CROSS)
    finally:
        restore(K)
    wst.done()


@pytest.mark.parametrize("cus", [64, 256])
@pytest.mark.parametrize("which", ["slot_per_cu", "more_than_units"])
def test_forced_stream_k(K, monkeypatch, which, cus):
    # the stream-K partial GEMM + its combine-and-LayerNorm: 64x64 tiles with one workgroup per CU
    # (tiles cut across workgroups), and 128x128 tiles with more workgroups than some shapes have
    # units (P is clamped: every unit is a segment of its own).
    # Measured worst err/err_ref (bound 4): 1.51 / 1.43 (64x64, 64 / 256 CUs), 1.50 / 1.44 (128x128).
    from walkai_nos_amd.ops import gemm as G
    choices = {}
    for Kd in (384, 1536):
        cands = G.streamk_candidates(384, Kd, cus)
        c, P = [x for x in cands if x[1] == cus][0] if which == "slot_per_cu" else cands[-1]
        choices[Kd] = ("streamk", c, P)
    forced = force(monkeypatch, choices)
    wst = Worst(f"(c) stream-K {sorted(choices.values())} cus={cus}", label="model")
    try:
        K.set_slice_cus(cus)
        for inp in CROSS:
            check(wst, 3, inp, (which, cus))
        assert {k[2] for k in forced.keys} == {384, 1536} and len(forced.keys) == 6 * len(CROSS)
        clamped = {k: G.streamk_map(k[0], k[1], k[2], choices[k[2]][1], choices[k[2]][2])[0] < choices[k[2]][2]
                   for k in set(forced.keys)}
        # both kinds of launch ran: tiles cut across workgroups, and (128x128 tiles) P above the unit count
        assert not all(clamped.values()) and (which == "slot_per_cu" or any(clamped.values())), clamped
    finally:
        restore(K)
    wst.done()


# ---- (d) the timer left alone -------------------------------------------------------------------------
def test_timed_pipeline(K, monkeypatch):
    # whatever the projection / fc2 timer picks on the whole GPU at T = 257 (printed; in the kept run
    # unsplit for the projection, split-K for both fc2 shapes). Measured worst err/err_ref (bound 4): 1.49.
    from walkai_nos_amd.ops import gemm as G
    monkeypatch.delenv("NOS_SPLITK", raising=False)
    monkeypatch.setattr(G, "_fused_cache", {})
    wst = Worst("(d) timed pipeline", label="model")
    try:
        K.set_slice_cus(K.total_cus())
        check(wst, 3, T257)
        print("[model] (d) the timer chose:", G.fused_table())
        assert len(G._fused_cache) == 3   # projection, fc2 with mid, the last fc2 (no mid, no LayerNorm)
    finally:
        restore(K)
    wst.done()


# ---- (e) - (g) attention variants of the block ----------------------------------------------------
def test_fused_attention_projection(K, monkeypatch):
    # NOS_ATTN_PROJ_FUSED=1: attention partials, then merge + projection + residual + LN2 in one kernel.
    # Measured worst err/err_ref (bound 4): 2.24 (T = 257, hidden).
    monkeypatch.setenv("NOS_ATTN_PROJ_FUSED", "1")
    monkeypatch.setenv("NOS_SPLITK", "0")
    fused = Calls(monkeypatch, K, "attention_proj_ln_x3f")
    wst = Worst("(e) attention + projection fused", label="model")
    try:
        for inp in CROSS:
            check(wst, 3, inp)
        assert fused.n == 3 * len(CROSS)
    finally:
        restore(K)
    wst.done()


@pytest.mark.parametrize("group", [8, 4])
def test_planes_in_attention(K, monkeypatch, group):
    # NOS_ATTN_F32IN=0 (and 4 query tiles per workgroup, which implies it): the QKV GEMM writes x3
    # planes and the planes-in attention kernel reads them.
    # Measured worst err/err_ref (bound 4): 1.91, the same for both groups.
    monkeypatch.setenv("NOS_ATTN_F32IN", "0")
    monkeypatch.setenv("NOS_SPLITK", "0")
    planes_in = Calls(monkeypatch, K, "attention_qkv_x3")
    wst = Worst(f"(f) planes-in attention, group {group}", label="model")
    try:
        K.set_attention_x3_group(group)
        assert not K.attention_input_f32()
        for inp in CROSS:
            check(wst, 3, inp, (group,))
        assert planes_in.n == 3 * len(CROSS)
    finally:
        restore(K)
    wst.done()


def test_in_kernel_merge(K, monkeypatch):
    # the wide attention kernel merges split query tiles itself (row counters, no fixup launch).
    # Measured worst err/err_ref (bound 4): 1.91.
    monkeypatch.setenv("NOS_SPLITK", "0")
    wst = Worst("(g) in-kernel merge", label="model")
    try:
        K.set_attention_merge(True)
        assert K.attention_merge_in_kernel() and K.attention_x3_wide()
        for inp in CROSS:
            check(wst, 3, inp)
    finally:
        restore(K)
    wst.done()


# ---- (h) f32 mode -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 2, 3])
def test_f32_mode(K, variant):
    # the f32-input MFMA GEMMs (or hipBLASLt where the tuner finds it faster) and the f32 stream-K
    # attention kernels through _Block.forward's plain branch.
    # Measured worst err/err_ref (bound 4): 1.55 (variant 0), 1.41 (variants 2 and 3).
    wst = Worst(f"(h) f32 mode, attention variant {variant}", label="model")
    try:
        K.set_fp32_matmul("f32")
        K.set_attention_variant(variant)
        assert not K.x3_active(gpu_model(3).pos_embed)
        for inp in CROSS:
            check(wst, 3, inp, (variant,))
    finally:
        restore(K)
    wst.done()


# ---- (i) slice sizes and a pin ------------------------------------------------------------------------
@pytest.mark.parametrize("cus,pin", [(32, 0), (64, 0), (128, 0), (256, 0), (32, 1 << 5), (64, 0b0011)])
def test_slices_and_pins(K, monkeypatch, cus, pin):
    # the slice's CU count sizes the attention and LayerNorm grids, filters the tiles the timer
    # offers (large tiles below the whole GPU, persistent ones under a pin) and gates split-K
    # (SPLITK_MIN_CUS); the timers run as they do in production.
    # Measured worst err/err_ref (bound 4): 2.00 (32 CUs, pinned or not), 1.64 / 1.65 / 1.73 (64 / 128 /
    # 256 CUs), 1.55 (64 CUs on XCDs 0-1).
    from walkai_nos_amd.ops import gemm as G
    monkeypatch.delenv("NOS_SPLITK", raising=False)
    wst = Worst(f"(i) slice of {cus} CUs, pin {pin:#x}", label="model")
    try:
        K.set_slice_cus(cus)
        K.set_slice_pin(pin)
        for inp in CROSS:
            check(wst, 3, inp, (cus, pin))
        fused = [v for k, v in G._fused_cache.items() if k[5:] == (cus, pin)]
        assert bool(fused) == (cus >= G.SPLITK_MIN_CUS)
        if pin:
            tiles = {v for k, v in G._x3_cache.items() if k[5:] == (cus, pin)}
            assert tiles and tiles <= G.X3_PERSISTENT
    finally:
        restore(K)
    wst.done()


# ---- (j) graph capture --------------------------------------------------------------------------------
@pytest.mark.parametrize("inp", [T129, T257], ids=lambda i: "x".join(map(str, i)))
def test_graph_capture(K, monkeypatch, inp):
    # captured after a warm eager call (weights split, position embeddings cached) with empty tile
    # caches: under capture nothing can be timed, so x3_heuristic picks every tile and the
    # projection / fc2 steps take ("unsplit",). One stream, a straight-line graph, replayed twice.
    # Measured worst err/err_ref (bound 4): 1.58 (T = 129), 1.65 (T = 257).
    from walkai_nos_amd.ops import gemm as G
    monkeypatch.setenv("NOS_SPLITK", "0")
    heuristic = Calls(monkeypatch, G, "x3_heuristic")
    wst = Worst(f"(j) graph capture {inp}", label="model")
    try:
        px, ref, err_ref = R.reference(3, *inp)
        m, x = gpu_model(3), px.cuda()
        run(m, x)
        assert heuristic.n == 0
        monkeypatch.setattr(G, "_x3_cache", {})
        monkeypatch.setattr(G, "_fused_cache", {})
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            with torch.no_grad():
                hidden = m.encode(x)
                logits, boxes = m.detect(hidden)
        assert heuristic.n >= 5 and not G._fused_cache
        for rep in range(2):
            for t in (hidden, logits, boxes):
                t.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            compare(wst, (hidden, logits, boxes), ref, err_ref, (3,) + tuple(inp) + ("replay", rep))
        del graph
    finally:
        restore(K)
    wst.done()


# ---- (k) one block ------------------------------------------------------------------------------------
def test_block_level(K, monkeypatch):
    # the middle block alone on the model's own activations (the 1-layer model's hidden state):
    # _Block.forward's x3 branch (public, not reached from YolosSmall.forward) and forward_x3 with
    # nothing handed in or folded out, against that one block in fp64; the yardstick is the same
    # block in plain fp32 on the CPU. forward_x3's folded LayerNorm is checked against the next
    # block's LN1 of the fp64 output.
    # Measured worst err/err_ref (bound 4): 3.06 (T = 128, forward) - one block's err_ref is a single
    # small draw (3.6e-6 at |x| up to 15); the error, 1.1e-5, is a third of the floor.
    monkeypatch.setenv("NOS_SPLITK", "0")
    m, i = gpu_model(3), 1
    blk, nxt = m.blocks[i], m.blocks[i + 1].ln1
    sd32 = R.state_dict(3)
    sd64 = {k: v.double() for k, v in sd32.items()}
    wst = Worst("(k) block level", label="model")
    try:
        for inp in CROSS:
            h, w, b = inp
            x32 = R.reference(1, *inp)[1][0].float()
            mid64 = R.interpolate(sd64["mid_pos_embed"], m.c, h // 16, w // 16)[i]
            ref = R.block(x32.double(), sd64, i, m.c) + mid64
            err_ref = ((R.block(x32, sd32, i, m.c) + mid64.float()).double() - ref).abs().max().item()
            ln_ref = R._layernorm(ref, sd64["blocks.2.ln1.weight"], sd64["blocks.2.ln1.bias"], m.c.layer_norm_eps)
            ln_err = (R._layernorm(ref.float(), sd32["blocks.2.ln1.weight"], sd32["blocks.2.ln1.bias"],
                                   m.c.layer_norm_eps).double() - ln_ref).abs().max().item()
            mid = m.position_embeddings((h, w))[1][i]
            assert mid.shape == (1, R.tokens(h, w), 384)
            x = x32.cuda()
            assert K.x3_active(x)
            with torch.no_grad():
                outs = {"forward": blk(x, mid), "forward_x3": blk.forward_x3(x, mid, None, None)}
                folded = blk.forward_x3(x, mid, None, nxt)
            torch.cuda.synchronize()
            assert outs["forward_x3"][1] is None
            outs["forward_x3"] = outs["forward_x3"][0]
            outs["forward_x3 + next_ln"] = folded[0]
            floor = 2e-6 * max(1.0, ref.abs().max().item())
            for name, o in outs.items():
                assert o.shape == ref.shape
                wst.check((o.double().cpu() - ref).abs().max().item(), err_ref, floor, inp + (name,))
            # the planes of LN(x): x itself is off by up to err, which the LayerNorm passes on
            # scaled by |w| / std(x); the bound for the planes is the block's bound through that
            # gain, plus the LayerNorm's own fp32 error
            planes = folded[1].double().sum(0).cpu()
            assert planes.shape == ref.shape
            gain = (sd64["blocks.2.ln1.weight"].abs().max() / ref.std(-1, unbiased=False).min()).item()
            wst.check((planes - ln_ref).abs().max().item(), gain * err_ref + ln_err,
                      2e-6 * max(1.0, ln_ref.abs().max().item()), inp + ("next_ln planes",))
    finally:
        restore(K)
    wst.done()


# ---- which detection heads run --------------------------------------------------------------------
def test_module_heads_when_not_fusable(K, monkeypatch):
    # a 388-wide hidden layer in the heads fails heads_fusable: the hip backend takes K.layernorm and
    # the module heads at B = 1. Measured worst err/err_ref (bound 4): 1.53.
    from walkai_nos_amd.models.workload.yolos import _MLPHead
    monkeypatch.setenv("NOS_SPLITK", "0")
    cpu = R.model(3)
    cpu.cls_head, cpu.box_head = _MLPHead(384, 388, cpu.c.num_labels + 1), _MLPHead(384, 388, 4)
    R.randomize(cpu.cls_head, seed=3)
    R.randomize(cpu.box_head, seed=4)
    px = R.pixels(*T129)
    ref, err_ref = R.yardstick(cpu, px)
    assert torch.isfinite(ref[1]).all() and torch.isfinite(ref[2]).all()
    import copy
    m = copy.deepcopy(cpu).cuda().eval()
    heads = Calls(monkeypatch, K, "detection_heads")
    wst = Worst("388-wide heads (module path)", label="model")
    try:
        assert not m.heads_fusable() and gpu_model(3).heads_fusable()
        compare(wst, run(m, px.cuda()), ref, err_ref, T129 + (388,))
        assert heads.n == 0
    finally:
        restore(K)
    wst.done()
