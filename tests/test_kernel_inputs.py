"""The staged-logit attention inputs (``tests/kernel_inputs.py``) do what they are for: replayed on
the CPU in fp64, every profile but ``spike_first`` fires the x3 attention kernels' lazy rescale rule
with a finite running max, and the suite's usual ``randn`` input never does.

The exact-term x3 inputs (``term_case``, ``selector_qkv``) likewise: a plain emulation of the six-term
plane product (``x3_emulate``: per-term products in fp64, summed in fp32 in the kernels' order) is
bit-exact on every case, every single-term drop and every plane mutant changes bits on the case built
for it, and on ``randn`` the second-order drops stay under the bounds of the GPU suite."""
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


# ---- exact-term x3 inputs -------------------------------------------------------------------------
PROOF_M, PROOF_KD = 129, 64


@pytest.fixture(scope="module")
def proof_cases():
    return {kind: KI.term_case(kind, PROOF_M, PROOF_KD) for kind in KI.TERM_CASES}


def test_split3_cpu_is_the_librarys_split():
    from walkai_nos_amd.ops import kernels
    x = torch.cat([KI.split3_points(), KI.generic_f32(16, 64, seed=3).flatten()])
    assert torch.equal(KI.split3_cpu(x), kernels.split3(x))


def test_six_terms_are_bit_exact_on_every_case():
    # every case, depth and placement the GPU tests run (the smallest and the largest M), emulated with
    # both MFMA k-steps: the six-term product in the kernels' order is the fp64 product to the bit
    n = 0
    for Kd in KI.TERM_KDS:
        for kind in KI.TERM_CASES:
            for M in (65, 513):
                phases = KI.onehot_phases(M, Kd) if kind in ("a0b", "a1b1") else 1
                for phase in sorted({0, phases - 1}):
                    c = KI.term_case(kind, M, Kd, phase)
                    for kstep in (16, 32):
                        assert torch.equal(KI.x3_emulate(c["A"], c["W"], kstep=kstep), c["ref"]), (kind, M, Kd, phase, kstep)
                        n += 1
    assert n >= 2 * 2 * 4 * 4


def test_onehot_placement_covers_every_row_lane_and_k_group():
    for Kd in KI.TERM_KDS:
        want = 32 * (Kd // 8)
        for M in (65, 129, 257, 513):
            ks = [KI.onehot_k(M, Kd, p) for p in range(KI.onehot_phases(M, Kd))]
            assert all(int(k.max()) < Kd and int(k.min()) >= 0 for k in ks)
            assert len(KI.onehot_pairs(ks, Kd)) == want, (M, Kd)
            assert M % 32 == 1  # the last row block is partial for every BM
        assert KI.onehot_phases(KI.TERM_N, Kd) == 1 and len(KI.onehot_pairs([KI.onehot_k(KI.TERM_N, Kd)], Kd)) == want


def test_every_single_term_drop_changes_bits_on_the_case_built_for_it(proof_cases):
    # share of the outputs that change when one of the six products is left out, per case: a case
    # catches exactly the terms of KI.TERM_PINS. Among the one-hot cases only a1b1 catches a1b1;
    # dense2 catches it at full density. (PROOF_M x 768 outputs, Kd = 64.)
    share = {}
    for kind, c in proof_cases.items():
        for drop in KI.X3_TERMS:
            kept = tuple(t for t in KI.X3_TERMS if t != drop)
            share[(kind, drop)] = float((KI.x3_emulate(c["A"], c["W"], kept) != c["ref"]).float().mean())
    for drop in KI.X3_TERMS:
        print(drop, {kind: round(share[(kind, drop)], 4) for kind in KI.TERM_CASES})
    for kind in KI.TERM_CASES:
        caught = tuple(sorted(t for t in KI.X3_TERMS if share[(kind, t)] > 0))
        assert caught == tuple(sorted(KI.TERM_PINS[kind])), (kind, caught)
        assert all(share[(kind, t)] > 0.5 for t in KI.TERM_PINS[kind]), (kind, share)
    for drop in KI.X3_TERMS:
        assert any(drop in KI.TERM_PINS[kind] for kind in KI.TERM_CASES), drop
    assert [k for k in KI.TERM_CASES if share[(k, (1, 1))] > 0] == ["a1b1", "dense2"]
    assert [k for k in KI.TERM_CASES if share[(k, (2, 0))] > 0] == ["ab0"]
    assert [k for k in KI.TERM_CASES if share[(k, (0, 2))] > 0] == ["a0b"]


def test_plane_mutants_are_caught(proof_cases):
    # plane 2 read as zero, plane 2 read as plane 1, and W's planes swapped (each pair): every
    # mutant changes bits on some case
    def zero2(which):
        def f(pa, pw):
            pa, pw = pa.clone(), pw.clone()
            (pa if which == "a" else pw)[2] = 0
            return pa, pw
        return f

    def two_is_one(which):
        def f(pa, pw):
            pa, pw = pa.clone(), pw.clone()
            p = pa if which == "a" else pw
            p[2] = p[1]
            return pa, pw
        return f

    def swap(i, j):
        def f(pa, pw):
            order = [0, 1, 2]
            order[i], order[j] = j, i
            return pa, pw[order]
        return f
    mutants = {"a2=0": zero2("a"), "w2=0": zero2("w"), "a2=a1": two_is_one("a"), "w2=w1": two_is_one("w"),
               "w0<->w1": swap(0, 1), "w1<->w2": swap(1, 2), "w0<->w2": swap(0, 2)}
    for name, f in mutants.items():
        caught = [k for k, c in proof_cases.items() if not torch.equal(KI.x3_emulate(c["A"], c["W"], planes=f), c["ref"])]
        print(name, caught)
        assert caught, name


def test_second_order_drops_stay_under_the_randn_bounds():
    # why the exact inputs exist: on the suite's GEMM input (randn x 0.05 randn, N = 768) a missing
    # second-order product moves the result by less than the bounds of the edge tests (floor 1e-5 at
    # Kd <= 128) and of the split-K / stream-K / fused tests (1e-4), a missing first-order one by 1e-3.
    # (128 rows here. On the MI355X, with a1b1 taken out of every 32x32 tile, the edge test's 512 rows
    # reach 1.02e-5 at Kd = 128 - over its floor by 2% - and pass at Kd = 32 and 64.)
    for Kd, bound in ((32, 1e-5), (128, 1e-5), (384, 1e-4)):
        g = torch.Generator().manual_seed(100 + Kd)
        x = torch.randn(512, Kd, generator=g)[:128]
        w = torch.randn(768, Kd, generator=g) * 0.05
        ref = x.double() @ w.double().t()
        six = (KI.x3_emulate(x, w).double() - ref).abs().max().item()
        assert six < 4e-6, (Kd, six)  # the fp32 accumulator's own rounding over 6 Kd / 16 additions
        for drop in KI.X3_TERMS[:3]:
            err = (KI.x3_emulate(x, w, tuple(t for t in KI.X3_TERMS if t != drop)).double() - ref).abs().max().item()
            print(Kd, drop, six, err)
            assert 3 * six < err < bound, (Kd, drop, err)
        first = (KI.x3_emulate(x, w, tuple(t for t in KI.X3_TERMS if t != (0, 1))).double() - ref).abs().max().item()
        assert first > 1e-3, (Kd, first)


def test_selector_inputs():
    # the selected key leads by 2 G^2 against at most G^2; within the first 32-query tile the selected
    # keys fall in the first key block, a middle one (where there is one) and the tail key's block
    for T in KI.SELECT_PERM:
        qkv, exp = KI.selector_qkv(2, T, 2)
        pi = KI.selector_perm(T)
        nk = (T + 31) // 32
        blocks = set((pi[:32] // 32).tolist())
        assert 0 in blocks and (T - 1) // 32 in blocks and (nk <= 2 or blocks & set(range(1, nk - 1))), (T, blocks)
        ref = KI.attention_formula(qkv.double(), 2, 0.125)
        assert torch.equal(ref.float(), exp) and torch.equal(ref, exp.double()), T
        gap = KI.SELECT_GAIN ** 2 * 0.125 * KI.LOG2E
        assert gap > 700  # exp2(-gap) is zero in fp32; in the fp64 softmax above it is under the last bit


def test_lane_pattern_and_gain():
    qkv = KI.staged_qkv("stairs", 8.5, 2, 70, 2).view(2, 70, 3, 2, 64)
    gain = 8.5 / (0.125 * KI.LOG2E)
    a = qkv[0, :, 0, 1, 0]
    assert torch.allclose(a[:8], gain * torch.tensor([1, -1, 0, 0.125] * 2))
    assert torch.equal(qkv[1, :, 1, 0, 0], (torch.arange(70) // 32).float())
    # one unit of c moves the score of an a = gain row by delta exp2 units
    assert abs(a[0].item() * 1.0 * 0.125 * KI.LOG2E - 8.5) < 1e-5
