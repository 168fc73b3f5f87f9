"""The staged-logit attention inputs (``tests/kernel_inputs.py``) do what they are for: replayed on
the CPU in fp64, every profile but ``spike_first`` fires the x3 attention kernels' lazy rescale rule
with a finite running max, and the suite's usual ``randn`` input never does."""
import pytest
import torch

import kernel_inputs as KI


@pytest.fixture(scope="module")
def replays():
    out = {}
    for profile, delta in KI.STAGED:
        qkv = KI.staged_qkv(profile, delta, 1, 257, 2)
        out[(profile, delta)] = (KI.rescale_replay(qkv, 2), KI.attention_reference(qkv, 2))
    return out


def test_staged_profiles_fire_the_rescale_rule(replays):
    assert set(replays) == set(KI.STAGED)
    for key, (r, _) in replays.items():
        print(key, r)
        if key[0] == "spike_first":
            assert r["fired"] == 0, (key, r)  # everything after the first block underflows
        else:
            assert r["fired"] > 0, (key, r)


def test_stairs_under_the_threshold_also_hold(replays):
    # a gap in (0, 8] leaves m where it is: P values above 1 reach the plane split
    for delta in (4.0, 7.5):
        r = replays[("stairs", delta)][0]
        assert r["held"] > 0 and 0 < r["largest_gap"], (delta, r)


def test_randn_never_fires_after_the_first_block():
    # the gap in the suite this construction closes: the workload-like input never moves m lazily
    r = KI.rescale_replay(KI.randn_qkv(1, 1024, 6, seed=0), 6)
    print("randn", r)
    assert r["fired"] == 0 and r["largest_gap"] < KI.RESCALE_GAP, r


def test_references_are_finite_and_fp32_formula_is_close(replays):
    for key, (_, (ref, err_ref, vmax)) in replays.items():
        assert torch.isfinite(ref).all(), key
        assert 0 < err_ref < 1e-3 and vmax > 1, (key, err_ref, vmax)


def test_a_kernel_without_the_rescale_is_caught_only_by_the_staged_inputs():
    # the lazy online softmax replayed in fp64: right, it is the reference on every input; with the
    # alpha rescale left out, every firing profile is off by far more than any bound the GPU tests
    # use, while the randn input cannot tell (m never moves after the first block)
    inputs = {key: KI.staged_qkv(key[0], key[1], 1, 257, 2) for key in KI.STAGED}
    inputs["randn"] = KI.randn_qkv(1, 1024, 6, seed=0)
    for key, qkv in inputs.items():
        H = 6 if key == "randn" else 2
        ref = KI.attention_formula(qkv.double(), H, 0.125)
        good = (KI.lazy_softmax_attention(qkv, H) - ref).abs().max().item()
        bad = (KI.lazy_softmax_attention(qkv, H, rescale=False) - ref).abs().max().item()
        print(key, good, bad)
        assert good < 1e-12, (key, good)
        if key == "randn" or key[0] == "spike_first":
            assert bad < 1e-12, (key, bad)
        else:
            assert bad > 1e-2, (key, bad)


def test_lane_pattern_and_gain():
    qkv = KI.staged_qkv("stairs", 8.5, 2, 70, 2).view(2, 70, 3, 2, 64)
    gain = 8.5 / (0.125 * KI.LOG2E)
    a = qkv[0, :, 0, 1, 0]
    assert torch.allclose(a[:8], gain * torch.tensor([1, -1, 0, 0.125] * 2))
    assert torch.equal(qkv[1, :, 1, 0, 0], (torch.arange(70) // 32).float())
    # one unit of c moves the score of an a = gain row by delta exp2 units
    assert abs(a[0].item() * 1.0 * 0.125 * KI.LOG2E - 8.5) < 1e-5
