"""The fp64 reference of the YOLOS architecture (``tests/yolos_reference.py``) checked on the CPU:
against ``transformers`` in fp64, against the project's own module in fp64 (its ops take their
torch form on the CPU), and the conditions the reference must satisfy to be a useful yardstick for
``tests/test_gpu_model_paths.py``. Also the fp32 parity of the module with ``transformers`` with mid
position embeddings, distinguishable 1-D parameters and inputs that are not ``image_size``."""
import pytest
import torch

import yolos_reference as R

from walkai_nos_amd.models.workload.yolos import YolosSmall


def _hf_pair(mid: bool, dtype):
    """``(transformers model, YolosSmall with its weights)``, every parameter drawn by ``R.randomize``."""
    transformers = pytest.importorskip("transformers")
    cfg = transformers.YolosConfig(hidden_size=384, num_hidden_layers=R.MAX_LAYERS, num_attention_heads=6,
                                   intermediate_size=1536, image_size=[64, 96], patch_size=16, num_labels=91,
                                   num_detection_tokens=100, use_mid_position_embeddings=mid)
    hf = transformers.YolosForObjectDetection(cfg).eval()
    R.randomize(hf, seed=2)
    m = YolosSmall(R.config(R.MAX_LAYERS, mid)).eval()
    m.load_hf_state_dict(hf.state_dict())
    return hf.to(dtype), m.to(dtype)


@pytest.mark.parametrize("mid", [False, True])
def test_reference_matches_transformers_fp64(mid):
    hf, m = _hf_pair(mid, torch.float64)
    sd = m.state_dict()
    for h, w, b in R.INPUTS:
        px = R.pixels(h, w, b).double()
        with torch.no_grad():
            out = hf(pixel_values=px)
        _, logits, boxes = R.forward(sd, m.c, px)
        assert (out.logits - logits).abs().max().item() < 1e-10, (h, w, b)
        assert (out.pred_boxes - boxes).abs().max().item() < 1e-10, (h, w, b)


@pytest.mark.parametrize("layers", R.LAYERS)
def test_reference_matches_module_fp64(layers):
    m = R.model(layers).double()
    for h, w, b in R.INPUTS:
        px = R.pixels(h, w, b).double()
        with torch.no_grad():
            hidden = m.encode(px)
            logits, boxes = m(px)
        ref = R.forward(R.state_dict(layers), m.c, px)
        assert hidden.shape == (b, R.tokens(h, w), 384)
        for name, got, want in zip(("hidden", "logits", "boxes"), (hidden, logits, boxes), ref):
            assert got.shape == want.shape
            assert (got - want).abs().max().item() < 1e-10, (name, h, w, b)


def test_reference_without_mid_matches_module_fp64():
    m = R.model(2, mid=False).double()
    px = R.pixels(64, 112).double()
    with torch.no_grad():
        logits, boxes = m(px)
    _, rl, rb = R.forward(R.state_dict(2, mid=False), m.c, px)
    assert (logits - rl).abs().max().item() < 1e-10 and (boxes - rb).abs().max().item() < 1e-10


@pytest.mark.parametrize("layers", R.LAYERS)
def test_reference_is_a_usable_yardstick(layers):
    # finite, no box in the sigmoid's saturated ends, the parameters do matter (no unit LayerNorm,
    # no zero bias, mid embeddings present), and plain fp32 sits where fp32 should
    sd = R.state_dict(layers)
    assert sd["mid_pos_embed"].shape[0] == layers - 1
    for k, v in sd.items():
        if v.dim() == 1:
            assert v.abs().min().item() > 0 and (v.numel() < 92 or v.std().item() > 0.2), k
    for h, w, b in R.INPUTS:
        px, (hidden, logits, boxes), err = R.reference(layers, h, w, b)
        assert px.shape == (b, 3, h, w) and hidden.shape == (b, R.tokens(h, w), 384)
        for t in (hidden, logits, boxes):
            assert t.dtype == torch.float64 and torch.isfinite(t).all()
        inside = ((boxes > 0.01) & (boxes < 0.99)).double().mean().item()
        assert inside >= 0.99, (h, w, b, inside)
        assert logits.abs().max().item() < 10.0
        assert 0 < err[1] < 2e-5 and 0 < err[2] < 5e-6, err
    # the same (layers, input) gives the same objects: computed once, shared
    assert R.reference(layers, 48, 144)[1][0] is R.reference(layers, 48, 144)[1][0]


def test_truncations_share_one_parameter_set():
    sd1, sd3 = R.state_dict(1), R.state_dict(3)
    assert "blocks.1.ln1.weight" not in sd1 and "blocks.2.ln1.weight" in sd3
    for k, v in sd1.items():
        if k != "mid_pos_embed":
            assert torch.equal(v, sd3[k]), k
    # the blocks differ from each other: a LayerNorm or bias taken from the wrong block shows
    assert not torch.equal(sd3["blocks.0.ln1.weight"], sd3["blocks.1.ln1.weight"])
    assert not torch.equal(sd3["mid_pos_embed"][0], sd3["mid_pos_embed"][1])


@pytest.mark.parametrize("mid", [False, True])
def test_yolos_matches_transformers_with_mid_embeddings_and_random_1d_parameters(mid):
    # the fp32 parity of tests/test_infra.py::test_yolos_matches_transformers_reference, at its bound,
    # with nothing trivial: inputs at, below and above image_size, an odd width, a batch
    hf, m = _hf_pair(mid, torch.float32)
    for h, w, b in ((64, 96, 1), (48, 80, 2), (80, 112, 1), (64, 98, 1), (70, 99, 1)):
        px = R.pixels(h, w, b)
        with torch.no_grad():
            ref = hf(pixel_values=px)
            logits, boxes = m(px)
        assert (ref.logits - logits).abs().max().item() < 1e-5, (h, w, b)
        assert (ref.pred_boxes - boxes).abs().max().item() < 1e-5, (h, w, b)
