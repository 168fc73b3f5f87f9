"""The HIP kernels off their bulk path (GPU only): the attention kernels' lazy online-softmax rescale
on staged logits and at T edges, every GEMM tile at tile-exact M / one past / short K, the GELU
epilogues on exact pre-activations, LayerNorm over row counts, widths and value profiles, and
``split3`` / the detection heads at their edges. Inputs come from ``tests/kernel_inputs.py``; every
reference is fp64 of the same fp32 input, and every bound is a multiple of what the same formula
loses in plain fp32 on the CPU (``err_ref``), so it means the same at logits of +-330 as at
``randn``.

The worst measured ``err / err_ref`` of each kernel (MI355X; the run is kept in
``profiles/pytest_gpu_kernel_edges.log``, one ``[edges]`` line per test) stands beside its bound."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_inputs as KI
from kernel_inputs import Worst

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import erf_fit  # noqa: E402  (the CPU replay of the packed GELU)

pytestmark = pytest.mark.gpu

SCALE = 0.125
T_EDGES = (1, 31, 32, 33, 64, 255, 256, 257, 512)
T_STAGED = (33, 64, 256, 257)
KINDS = ["randn"] + [f"{p}:{d:g}" for p, d in KI.STAGED]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from walkai_nos_amd.ops import kernels
    assert kernels.hip_available(), "libnos_kernels.so must be built on a GPU box"
    kernels.set_backend("hip")
    return kernels


# ---- attention ----------------------------------------------------------------------------------
_cases = {}


def attn_case(kind, B, T, H):
    """``(qkv on the GPU, fp64 reference on the GPU, err_ref, floor)``, computed once per case."""
    key = (kind, B, T, H)
    if key not in _cases:
        if kind == "randn":
            qkv = KI.randn_qkv(B, T, H, seed=T)
        else:
            p, d = kind.split(":")
            qkv = KI.staged_qkv(p, float(d), B, T, H, SCALE, seed=T)
        ref, err_ref, vmax = KI.attention_reference(qkv, H, SCALE)
        assert torch.isfinite(ref).all()
        _cases[key] = (qkv.cuda(), ref.cuda(), err_ref, 2e-6 * vmax)
    return _cases[key]


def attn_cases(kind, shapes=((1, 1), (2, 2), (1, 2), (2, 1))):
    for T in (T_EDGES if kind == "randn" else T_STAGED):
        for B, H in shapes:
            yield (B, T, H) + attn_case(kind, B, T, H)


def grids(K, B, T, H, group=8):
    nk = (T + 31) // 32
    units = B * H * ((nk + group - 1) // group) * nk
    return (1, 3, 7, units + 5, K.attention_x3_waves(K.slice_cus(), B, T, H))


def nan_out(x3, B, T, H):
    if x3:
        return torch.full((3, B, T, H * 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    return torch.full((B, T, H * 64), float("nan"), device="cuda")


def as_f64(o):
    return o.double().sum(0) if o.dtype == torch.bfloat16 else o.double()


def attn_err(o, ref):
    # NaN survives max() on the GPU, so a NaN left from the prefill fails the bound
    return (as_f64(o) - ref).abs().max().item()


def restore_attention(K):
    K.set_attention_merge(None)
    K.set_attention_x3_pipelined(True)
    K.set_attention_x3_group(8)
    K.set_attention_x3_wide(K.attention_x3_wide_default())
    K.set_attention_variant(0)
    K._L().nos_attention_x3_set_flags(int(os.environ.get("NOS_ATTN_X3_FLAGS", "0")))


@pytest.mark.parametrize("kind", KINDS)
def test_attention_x3f_wide_and_two_wave(K, kind):
    # attn_fwd_x3w and attn_fwd_x3p<8> from fp32 QKV, fp32 and x3-plane outputs, heads in one launch
    # and one at a time: bit-identical to each other, the planes the exact split of the fp32 output,
    # and within 4x the fp32 formula's own error of fp64.
    # Measured worst err/err_ref (bound 4): randn 1.90; stairs 2.19 / 1.96 / 1.64 / 3.17 (delta 4 / 7.5 /
    # 8.5 / 30); spike_last 2.62; spike_first 1.21; saw 1.19 - the worst at T = 33, B = H = 1.
    wst = Worst("attention_x3f wide/two-wave")
    try:
        for B, T, H, qkv, ref, err_ref, floor in attn_cases(kind):
            for waves in grids(K, B, T, H):
                for hb in (None, 1):
                    f32 = None
                    for x3 in (False, True):
                        outs = []
                        for wide in (True, False):
                            K.set_attention_x3_wide(wide)
                            outs.append(K.attention_x3f(qkv, nan_out(x3, B, T, H), H, 64, SCALE, waves, head_block=hb))
                        tag = (kind, B, T, H, waves, hb, x3)
                        assert not torch.isnan(outs[0].float()).any(), tag
                        assert torch.equal(outs[0], outs[1]), tag
                        wst.check(attn_err(outs[0], ref), err_ref, floor, tag)
                        if x3:
                            assert torch.equal(outs[0], K.split3(f32)), tag
                        else:
                            f32 = outs[0]
    finally:
        restore_attention(K)
    wst.done()


@pytest.mark.parametrize("kind", KINDS)
def test_attention_x3_planes_in_kernels(K, kind):
    # the planes-in kernels: pipelined with 4 and 8 query tiles per workgroup, and block-at-a-time;
    # with 8 tiles the fp32-in kernel is the planes-in kernel bit for bit.
    # Measured worst err/err_ref (bound 4): the figures of the fp32-in kernels to the digit (randn 1.90,
    # stairs:30 3.17, spike_last 2.62), every variant.
    wst = Worst("attention_x3 planes-in")
    try:
        for B, T, H, qkv, ref, err_ref, floor in attn_cases(kind):
            planes = K.split3(qkv)
            for pipelined, group in ((True, 4), (True, 8), (False, 4)):
                K.set_attention_x3_pipelined(pipelined)
                K.set_attention_x3_group(group)
                for waves in grids(K, B, T, H, group):
                    tag = (kind, B, T, H, waves, pipelined, group)
                    out = K.attention_x3(planes, nan_out(False, B, T, H), H, 64, SCALE, waves)
                    wst.check(attn_err(out, ref), err_ref, floor, tag)
                    if pipelined and group == 8:
                        for hb in (None, 1):
                            a = K.attention_x3(planes, nan_out(True, B, T, H), H, 64, SCALE, waves, head_block=hb)
                            b = K.attention_x3f(qkv, nan_out(True, B, T, H), H, 64, SCALE, waves, head_block=hb)
                            assert torch.equal(a, b), tag
                            wst.check(attn_err(a, ref), err_ref, floor, tag + (hb, "x3 out"))
    finally:
        restore_attention(K)
    wst.done()


@pytest.mark.parametrize("kind", KINDS)
def test_attention_f32_kernels(K, kind):
    # the f32-input MFMA kernels: stream-K variants 0 (LDS-shared), 2 and 3 (one wave per tile), and
    # the unsplit kernel. They keep an eager running max, so the staged inputs exercise their alpha
    # rescale on every rising block.
    # Measured worst err/err_ref (bound 4): randn 2.34; stairs 3.19 / 1.41 / 2.65 / 1.82; spike_last
    # 3.25 (variant 2, 7 waves); spike_first 1.24; saw 0.84.
    wst = Worst("attention_sk / unsplit (f32 MFMA)")
    try:
        for B, T, H, qkv, ref, err_ref, floor in attn_cases(kind):
            for variant in (0, 2, 3):
                K.set_attention_variant(variant)
                for waves in grids(K, B, T, H):
                    out = K.attention_sk(qkv, nan_out(False, B, T, H), H, 64, SCALE, waves)
                    wst.check(attn_err(out, ref), err_ref, floor, (kind, B, T, H, waves, variant))
            wst.check(attn_err(K.attention_unsplit(qkv, H, 64, SCALE), ref), err_ref, floor, (kind, B, T, H, "unsplit"))
    finally:
        restore_attention(K)
    wst.done()


@pytest.mark.parametrize("kind", KINDS)
def test_attention_merge_and_bookkeeping_identities(K, kind):
    # in-kernel merge == the fixup launch (row counters left zero); reciprocal bookkeeping (flag 0)
    # == 64-bit bookkeeping (flag 8) == the fixup's XCD-local order (flag 64): all bit for bit, on
    # partials whose maxima differ by tens of exp2 units.
    # Measured worst err/err_ref (bound 4): as the fixup launch, 3.17 (stairs:30, T = 33).
    wst = Worst("attention_x3f in-kernel merge")
    L = K._L()
    try:
        K.set_attention_x3_wide(True)
        for B, T, H, qkv, ref, err_ref, floor in attn_cases(kind):
            for waves in grids(K, B, T, H):
                for x3 in (False, True):
                    fixup = {}
                    for hb in (None, 1):
                        tag = (kind, B, T, H, waves, x3, hb)
                        outs = []
                        for merge in (True, False, True):
                            K.set_attention_merge(merge)
                            outs.append(K.attention_x3f(qkv, nan_out(x3, B, T, H), H, 64, SCALE, waves, head_block=hb))
                        K.set_attention_merge(None)
                        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[1]), tag
                        wst.check(attn_err(outs[0], ref), err_ref, floor, tag)
                        fixup[hb] = outs[1]
                    for flags in (8, 64):
                        L.nos_attention_x3_set_flags(flags)
                        flagged = K.attention_x3f(qkv, nan_out(x3, B, T, H), H, 64, SCALE, waves)
                        L.nos_attention_x3_set_flags(0)
                        assert torch.equal(flagged, fixup[None]), (tag, flags)
            assert int(K._row_counters(qkv.device, 1).abs().sum().item()) == 0, (kind, B, T, H)
    finally:
        restore_attention(K)
    wst.done()


_proj = {}


def proj_case(kind, B, T):
    """The fused step's parameters and its fp64 / fp32-formula references (CPU), once per case."""
    key = (kind, B, T)
    if key not in _proj:
        H, D = 6, 384
        qkv, ref, _, _ = attn_case(kind, B, T, H)
        g = torch.Generator().manual_seed(12)
        w = torch.randn(D, D, generator=g) * 0.05
        b, lw, lb = (torch.randn(D, generator=g) for _ in range(3))
        r = torch.randn(B, T, D, generator=g)

        def chain(o, dt):
            x = o.to(dt) @ w.to(dt).t() + b.to(dt) + r.to(dt)
            return x, KI.layernorm_formula(x, lw.to(dt), lb.to(dt), 1e-12)
        x64, ln64 = chain(ref.cpu(), torch.float64)
        x32, ln32 = chain(KI.attention_formula(qkv.cpu(), H, SCALE), torch.float32)
        _proj[key] = ([t.cuda() for t in (w, b, r, lw, lb)], x64.cuda(), ln64.cuda(),
                      (x32.double() - x64).abs().max().item(), (ln32.double() - ln64).abs().max().item(),
                      2e-6 * max(1.0, x64.abs().max().item()), 2e-6 * max(1.0, ln64.abs().max().item()))
    return _proj[key]


@pytest.mark.parametrize("kind", KINDS)
def test_attention_merge_proj_layernorm_fused_edges(K, kind):
    # attention partials + csrc/attn_proj.hip's merge / projection / residual / LayerNorm (384-wide:
    # H = 6), B*T rows straddling its 32-row tiles. Yardstick: the same chain (attention, projection +
    # bias + residual, two-pass LayerNorm) in plain fp32 on the CPU against fp64; floor 2e-6 of the
    # output's scale, as for attention.
    # Measured worst err/err_ref (bound 4): x 1.71, LayerNorm planes 1.63 (both randn, T = 1, one
    # workgroup); staged inputs 0.97-1.57.
    wx, wl = Worst("attn_merge_proj_ln x"), Worst("attn_merge_proj_ln LayerNorm planes")
    for B, T, H, qkv, _, _, _ in attn_cases(kind, shapes=((1, 6), (2, 6))):
        (w, b, r, lw, lb), x64, ln64, ex, el, fx, fl = proj_case(kind, B, T)
        for waves in grids(K, B, T, H):
            x, h3 = K.attention_proj_ln_x3f(qkv, H, 64, SCALE, w, b, r, (lw, lb, 1e-12), waves=waves)
            assert x.shape == r.shape and h3.shape == (3,) + r.shape
            wx.check((x.double() - x64).abs().max().item(), ex, fx, (kind, B, T, waves))
            wl.check((h3.double().sum(0) - ln64).abs().max().item(), el, fl, (kind, B, T, waves))
    wx.done()
    wl.done()


# ---- GEMM ---------------------------------------------------------------------------------------
GEMM_N = 768
_gemm = {}


def gemm_case(Kd):
    """One 512-row problem per Kd: every M below takes its first M rows, so the fp64 products are
    computed once."""
    if Kd not in _gemm:
        g = torch.Generator().manual_seed(100 + Kd)
        x = torch.randn(512, Kd, generator=g).cuda()
        w = (torch.randn(GEMM_N, Kd, generator=g) * 0.05).cuda()
        b = torch.randn(GEMM_N, generator=g).cuda()
        r = torch.randn(512, GEMM_N, generator=g).cuda()
        r2 = torch.randn(1, 5, GEMM_N, generator=g).cuda()
        hb = x.double() @ w.double().t() + b.double()
        refs = {"bias": hb, "gelu": 0.5 * hb * (1 + torch.erf(hb / math.sqrt(2))),
                "res2": hb + r.double() + r2.double().reshape(5, GEMM_N)[torch.arange(512) % 5]}
        _gemm[Kd] = (x, w, b, r, r2, refs)
    return _gemm[Kd]


def epilogues(b, r, r2, M):
    return {"bias": {"bias": b}, "gelu": {"bias": b, "gelu": True},
            "res2": {"bias": b, "residual": r[:M], "residual2": r2}}


def m_edges(bm):
    return (bm - 1, bm, bm + 1, 2 * bm)


def guarded(M, fill):
    buf = torch.full((M + 7, GEMM_N), fill, device="cuda")
    return buf, buf[3:3 + M]


def guards_untouched(buf, fill):
    g = torch.cat([buf[:3], buf[-4:]])
    return bool(torch.isnan(g).all()) if math.isnan(fill) else bool((g == fill).all())


@pytest.mark.parametrize("Kd", [32, 64, 128])
def test_gemm_x3_every_tile_at_tile_edges(K, Kd, monkeypatch):
    # every x3 tile the table offers (persistent and the opt-in staggered one included) at a full
    # last row block, one row short, one past and two blocks; with Kd = 32 / 64 the 2-4-buffer
    # pipelines run fewer k-steps than they have LDS buffers. Bound: the suite's own (2x the f32
    # MFMA GEMM's error, floor 1e-5); the output lands in a NaN-guarded view.
    # Measured worst err/err_f32 (bound 2): 1.00 / 1.03 / 0.95 for Kd = 32 / 64 / 128; 40 / 50 / 50 tiles.
    from walkai_nos_amd.ops import gemm as G
    monkeypatch.setenv("NOS_X3_STAGGER", "1")
    x, w, b, r, r2, refs = gemm_case(Kd)
    x3 = K.split3(x)
    tiles = G.x3_eligible(GEMM_N, Kd)
    expect = [c for c, (bm, bn, _, kind) in G.X3_TILES.items()
              if GEMM_N % bn == 0 and (Kd % 64 == 0 or not kind.endswith("64"))]
    assert tiles == expect and len(tiles) >= 30 and any(c in G.X3_PERSISTENT for c in tiles) and 38 in tiles
    wst = Worst(f"gemm_x3 Kd={Kd}", factor=2.0)
    err_f32, ran = {}, 0
    for cfg in tiles:
        for M in m_edges(G.X3_TILES[cfg][0]):
            for name, kw in epilogues(b, r, r2, M).items():
                ref = refs[name][:M]
                if (M, name) not in err_f32:
                    f32 = G.gemm(x[:M], w, tile=G.eligible(M, GEMM_N, Kd)[0], **kw)
                    err_f32[(M, name)] = (f32.double() - ref).abs().max().item()
                buf, view = guarded(M, float("nan"))
                y, y3 = G.gemm_x3(x3[:, :M], w, tile=cfg, out_f32=True, out_x3=True, out=view, **kw)
                tag = (cfg, M, name)
                assert y.data_ptr() == view.data_ptr() and guards_untouched(buf, float("nan")), tag
                wst.check((y.double() - ref).abs().max().item(), err_f32[(M, name)], 1e-5, tag)
                assert torch.equal(y3.double().sum(0), y.double()), tag
                assert torch.equal(G.gemm_x3(x3[:, :M], w, tile=cfg, out_f32=False, out_x3=True, **kw), y3), tag
            ran += 1
    assert ran == 4 * len(tiles)
    wst.done()


@pytest.mark.parametrize("Kd", [32, 64, 128])
def test_gemm_f32_every_tile_at_tile_edges(K, Kd):
    from walkai_nos_amd.ops import gemm as G
    x, w, b, r, r2, refs = gemm_case(Kd)
    tiles = G.eligible(512, GEMM_N, Kd)
    assert tiles == [c for c, (_, bn, bk) in G.TILES.items() if GEMM_N % bn == 0 and Kd % bk == 0] and len(tiles) >= 7
    ran = 0
    for cfg in tiles:
        for M in m_edges(G.TILES[cfg][0]):
            assert cfg in G.eligible(M, GEMM_N, Kd)
            for name, kw in epilogues(b, r, r2, M).items():
                buf, view = guarded(M, 0.0)
                out = G.gemm(x[:M], w, tile=cfg, out=view, **kw)
                err = (out.double() - refs[name][:M]).abs().max().item()
                assert err < 2e-3 * max(1.0, Kd / 384), (cfg, M, name, err)
                assert guards_untouched(buf, 0.0), (cfg, M, name)
            ran += 1
    assert ran == 4 * len(tiles)


@pytest.mark.parametrize("Kd", [32, 64, 128])
def test_gemm_x3_f32a_at_tile_edges(K, Kd):
    # the fp32-activation kernel against the planes-in 16x16x32 8-wave tile of its shape: bit-identical
    from walkai_nos_amd.ops import gemm as G
    x, w, b, r, r2, _ = gemm_case(Kd)
    ran = 0
    for cfg, tile in ((0, 29), (1, 36)):
        assert G.X3A_TILES[cfg] == G.X3_TILES[tile][:2] and tile in G.x3_eligible(GEMM_N, Kd)
        for M in m_edges(G.X3A_TILES[cfg][0]):
            for name, kw in epilogues(b, r, r2, M).items():
                y, y3 = G.gemm_x3_f32a(x[:M], w, out_x3=True, cfg=cfg, **kw)
                t, t3 = G.gemm_x3(K.split3(x[:M].contiguous()), w, out_f32=True, out_x3=True, tile=tile, **kw)
                assert torch.equal(y, t) and torch.equal(y3, t3), (cfg, M, name, (y - t).abs().max().item())
            ran += 1
    assert ran == 8


def partial_refs(K, G, x, w, b, r, r2, M, lw, lb):
    hb = K.split3(x[:M].contiguous()).double().sum(0) @ G.weight_planes(w).double().sum(0).t()
    ref_x = hb + b.double() + r[:M].double() + r2.double().reshape(5, GEMM_N)[torch.arange(M) % 5]
    return hb, ref_x, F.layer_norm(ref_x, (GEMM_N,), lw.double(), lb.double(), 1e-12)


def test_splitk_partials_and_layernorm_at_tile_edges(K, monkeypatch):
    # split-K partials over every (tile, split) the table offers + the combine / LayerNorm kernel.
    # A split needs two stages per K range, so Kd = 32 and 64 offer none: ineligible by the table.
    from walkai_nos_amd.ops import gemm as G
    monkeypatch.setenv("NOS_X3_STAGGER", "1")
    g = torch.Generator().manual_seed(7)
    lw, lb = torch.randn(GEMM_N, generator=g).cuda(), torch.randn(GEMM_N, generator=g).cuda()
    ran = eligible = 0
    for Kd in (32, 64, 128):
        x, w, b, r, r2, _ = gemm_case(Kd)
        cands = G.split_candidates(GEMM_N, Kd)
        assert (len(cands) > 0) == (Kd == 128), (Kd, cands)
        refs = {}
        for cfg, sp in cands:
            for M in m_edges(G.X3_TILES[cfg][0]):
                eligible += 1
                if M not in refs:
                    refs[M] = partial_refs(K, G, x, w, b, r, r2, M, lw, lb)
                hb, ref_x, ref_ln = refs[M]
                a3 = K.split3(x[:M].contiguous())
                part = G.gemm_x3_partials(a3, w, cfg, sp, out=torch.full((sp, M, GEMM_N), float("nan"), device="cuda"))
                xo, planes = K.splitk_layernorm(part, b, r[:M].contiguous(), r2, (lw, lb, 1e-12))
                tag = (Kd, cfg, sp, M)
                assert (part.double().sum(0) - hb).abs().max().item() < 1e-4, tag
                assert (xo.double() - ref_x).abs().max().item() < 1e-4, tag
                assert (planes.double().sum(0) - ref_ln).abs().max().item() < 1e-4, tag
                x_only, none = K.splitk_layernorm(part, b, r[:M].contiguous(), None)
                assert none is None
                assert (x_only.double() - (hb + b.double() + r[:M].double())).abs().max().item() < 1e-4, tag
                ran += 1
    assert ran == eligible > 0


def test_streamk_partials_and_layernorm_at_tile_edges(K):
    # stream-K partials over every config the shape allows, P = 1, a prime and more workgroups than
    # units; planes a tile does not own stay NaN and the combine never reads them
    from walkai_nos_amd.ops import gemm as G
    g = torch.Generator().manual_seed(8)
    lw, lb = torch.randn(GEMM_N, generator=g).cuda(), torch.randn(GEMM_N, generator=g).cuda()
    ran = eligible = 0
    for Kd in (32, 64, 128):
        x, w, b, r, r2, _ = gemm_case(Kd)
        refs = {}
        for cfg, (bm, bn, bk, _) in G.X3K_TILES.items():
            if GEMM_N % bn or Kd % bk:
                continue
            for M in m_edges(bm):
                if M not in refs:
                    refs[M] = partial_refs(K, G, x, w, b, r, r2, M, lw, lb)
                _, ref_x, ref_ln = refs[M]
                a3 = K.split3(x[:M].contiguous())
                for P in (1, 7, 1 << 20):
                    eligible += 1
                    m = G.streamk_map(M, GEMM_N, Kd, cfg, P)
                    part, m2 = G.gemm_x3_streamk(a3, w, cfg, P, out=torch.full((m[6], M, GEMM_N), float("nan"), device="cuda"))
                    assert m2 == m
                    xo, planes = K.streamk_layernorm(part, m, b, r[:M].contiguous(), r2, (lw, lb, 1e-12))
                    assert (xo.double() - ref_x).abs().max().item() < 1e-4, (Kd, cfg, M, P, m)
                    assert (planes.double().sum(0) - ref_ln).abs().max().item() < 1e-4, (Kd, cfg, M, P, m)
                    ran += 1
    want = sum(12 for Kd in (32, 64, 128) for (_, bn, bk, _) in G.X3K_TILES.values() if GEMM_N % bn == 0 and Kd % bk == 0)
    assert ran == eligible == want and ran >= 12 * 9


# ---- epilogue tails -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gelu_pts():
    v = KI.gelu_points()
    ref = KI.gelu_reference(v)
    hc = erf_fit.header_coefficients()
    with np.errstate(over="ignore"):  # at |v| = 1e4 the unused |z| < 1 branch overflows; the replay selects the other
        replay = torch.from_numpy(erf_fit.gelu32(v.numpy(), hc["small"], hc["big"]))
    E = (replay.double() - ref).abs().max().item()
    assert 1e-8 < E < 1e-6, E
    x = torch.zeros(v.numel(), 32)
    x[:, 0] = v
    w = torch.zeros(128, 32)
    w[:, 0] = 1.0
    return {"v": v.cuda(), "ref": ref.cuda(), "E": E, "x": x.cuda(), "w": w.cuda(), "b": torch.zeros(128).cuda()}


def check_gelu(y, p, wst, tag):
    """``|err| <= max(2 E, 1e-7) + |v| 2^-23`` per element (E: the CPU replay's max error on these
    points; 2x for the hardware exp2's last bit), and the exact tails."""
    v, ref = p["v"], p["ref"]
    err = (y.double() - ref[:, None]).abs()
    allow = max(2 * p["E"], 1e-7) + v.double().abs()[:, None] * 2.0 ** -23
    over = err - allow
    wst.check(err.max().item(), p["E"], math.inf, tag)  # the figure for the log; the bound is per element
    assert not torch.isnan(y).any() and not bool((over > 0).any()), \
        (tag, err.max().item(), p["E"], v[over.max(1).values.argmax()].item())

    def rows(val, neg=False):
        sel = (v == val) & (torch.signbit(v) == neg)
        assert sel.any()
        return y[sel]
    assert (rows(0.0, True) == 0).all() and (rows(-1e4, True) == 0).all(), tag  # zeros of either sign
    assert (rows(0.0) == 0).all() and (rows(1e4) == 1e4).all(), tag


def test_gelu_epilogues_on_exact_preactivations(K, gelu_pts, monkeypatch):
    # x[m, 0] = v[m], w[n, 0] = 1, the rest 0, bias 0: every GEMM delivers h[m, n] = v[m] exactly
    # (asserted bit for bit on the plain-bias output first), so the epilogue is measured alone — the
    # |z| = 1 seam, the |z| = 4 clamp and the tails, one x3 tile of every kind, the fp32-activation
    # kernel and the f32 MFMA GEMM (erff).
    # Measured worst |err| / E (E = 2.93e-7, allowed 2 + the |v| 2^-23 term): packed GELU 1.00 on every
    # tile kind (the kernel is the CPU replay to the last bit at the worst point), erff 1.51.
    from walkai_nos_amd.ops import gemm as G
    monkeypatch.setenv("NOS_X3_STAGGER", "1")
    p = gelu_pts
    x, w, b, v = p["x"], p["w"], p["b"], p["v"]
    x3 = K.split3(x)
    tiles = G.x3_eligible(128, 32)
    kinds = {}
    for want in ("r", "d", "d2", "d8", "m16", "p", "t16w8"):
        kinds[want] = next(c for c in tiles if G.X3_TILES[c][3] == want)
    assert len(set(kinds.values())) == 7
    exact = v[:, None].expand(-1, 128).contiguous()
    nz = v != 0

    def injected(y):
        # bit for bit where v != 0; a signed zero comes out as a zero (the accumulator starts at +0)
        return torch.equal(y[nz].view(torch.int32), exact[nz].view(torch.int32)) and bool((y[~nz] == 0).all())
    wst = Worst("packed GELU (x3 epilogue) err / E", factor=math.inf)
    for kind, cfg in kinds.items():
        y, y3 = G.gemm_x3(x3, w, b, tile=cfg, out_f32=True, out_x3=True)
        assert injected(y) and torch.equal(y3.double().sum(0), exact.double()), (kind, cfg)
        y, y3 = G.gemm_x3(x3, w, b, gelu=True, tile=cfg, out_f32=True, out_x3=True)
        check_gelu(y, p, wst, (kind, cfg))
        assert torch.equal(y3.double().sum(0), y.double()), (kind, cfg)
    for cfg in G.X3A_TILES:
        assert injected(G.gemm_x3_f32a(x, w, b, cfg=cfg)), cfg
        check_gelu(G.gemm_x3_f32a(x, w, b, gelu=True, cfg=cfg), p, wst, ("f32a", cfg))
    wst.done()
    w32 = Worst("erff GELU (f32 GEMM epilogue) err / E", factor=math.inf)
    for cfg in G.eligible(v.numel(), 128, 32):
        assert injected(G.gemm(x, w, b, tile=cfg)), cfg
        check_gelu(G.gemm(x, w, b, gelu=True, tile=cfg), p, w32, ("f32", cfg))
    w32.done()


def test_bias_gelu_kernel_on_the_same_points(K, gelu_pts):
    # the in-place erff epilogue kernel: within 2x the error of torch's fp32 exact GELU on the CPU
    # (measured: 0.55x; 4.43e-7 against 8.09e-7)
    p = gelu_pts
    v = p["v"]
    e_torch = (F.gelu(v.cpu()).double() - p["ref"].cpu()).abs().max().item()
    y = v[:, None].repeat(1, 8).contiguous()
    K.bias_gelu_(y, torch.zeros(8, device="cuda"))
    wst = Worst("bias_gelu_ (erff) err / torch fp32 GELU err", factor=2.0)
    wst.check((y.double() - p["ref"][:, None]).abs().max().item(), e_torch, 0.0, "bias_gelu_")
    wst.done()
    assert (y[v == 0] == 0).all() and (y[v == -1e4] == 0).all() and (y[v == 1e4] == 1e4).all()


# ---- LayerNorm ----------------------------------------------------------------------------------
LN_ROWS = (1, 2, 3, 4, 5, 7, 8, 9, 17)
EPS = 1e-12
_ln = {}


def ln_case(profile, rows, D):
    key = (profile, rows, D)
    if key not in _ln:
        g = torch.Generator().manual_seed(D)
        w, b = torch.randn(D, generator=g), torch.randn(D, generator=g)
        x = KI.layernorm_rows(profile, rows, D, seed=rows)
        ref = KI.layernorm_formula(x.double(), w.double(), b.double(), EPS)
        err_ref = (KI.layernorm_formula(x, w, b, EPS).double() - ref).abs().max().item()
        assert torch.isfinite(ref).all()
        _ln[key] = (x.cuda(), w.cuda(), b.cuda(), ref.cuda(), err_ref, 1e-6 * max(1.0, w.abs().max().item()))
    return _ln[key]


def ln_launch(K, x, w, b, rows, D, wgs, x3):
    """``nos_layernorm_f32_grid`` into the middle of a NaN-filled buffer (fp32 rows, or the three
    dense x3 planes): returns the output view after checking the guard rows on both sides."""
    L = K._L()
    n = rows * D * (3 if x3 else 1)
    buf = torch.full((n + 4 * D,), float("nan"), dtype=torch.bfloat16 if x3 else torch.float32, device="cuda")
    view = buf[2 * D:2 * D + n]
    y, yp = (None, view.data_ptr()) if x3 else (view.data_ptr(), None)
    K._check(L.nos_layernorm_f32_grid(x.data_ptr(), w.data_ptr(), b.data_ptr(), y, yp, rows, D, EPS, wgs, K._stream()))
    assert torch.isnan(buf[:2 * D].float()).all() and torch.isnan(buf[2 * D + n:].float()).all(), (rows, D, wgs, x3)
    return view.view(3, rows, D) if x3 else view.view(rows, D)


@pytest.mark.parametrize("D", [384, 768, 1024, 1536, 2048])
def test_layernorm_rows_widths_and_values(K, D):
    # every width the launcher dispatches; row counts around the 4 waves x 2 rows in flight; one and
    # two workgroups, so one wave carries several iterations and the min(row, rows - 1) clamp and the
    # break both run; large-offset rows, an outlier, tiny and huge rows; a zero row gives the bias
    # back bit for bit. Bound: 4x the two-pass formula in plain fp32 on the CPU, floor 1e-6 max(1, |w|).
    # Measured worst err/err_ref (bound 4): 2.96 / 3.74 / 1.80 / 1.88 / 1.75 for D = 384 / 768 / 1024 /
    # 1536 / 2048. The two narrow widths peak on the 1e4-offset rows (2.2e-3 and 4.0e-3 absolute: the
    # mean of 1e4-sized values carries ~1e-3 of fp32 rounding either way, and with 3-4 rows the CPU
    # yardstick's own draw is small), the others on the outlier rows.
    wst = Worst(f"layernorm D={D}")
    for rows in LN_ROWS:
        for profile in KI.LN_PROFILES + ("zero",):
            x, w, b, ref, err_ref, floor = ln_case(profile, rows, D)
            for wgs in (0, 1, 2):
                y = ln_launch(K, x, w, b, rows, D, wgs, False)
                y3 = ln_launch(K, x, w, b, rows, D, wgs, True)
                tag = (profile, rows, D, wgs)
                assert not torch.isnan(y3.float()).any(), tag
                assert torch.equal(y3.double().sum(0), y.double()), tag
                if profile == "zero":
                    assert torch.equal(y, b.expand(rows, D)), tag
                else:
                    wst.check((y.double() - ref).abs().max().item(), err_ref, floor, tag)
            # the public wrappers (their own grid rule) give the same rows
            assert torch.equal(K.layernorm(x, w, b, EPS), y), tag
            assert torch.equal(K.layernorm_x3(x, w, b, EPS), y3), tag
    wst.done()


@pytest.mark.parametrize("D", [384, 768])
def test_splitk_layernorm_rows_and_values(K, D):
    # the combine kernel with one split of plain partials (x = part + 0 + 0 exactly), LayerNorm on and
    # off. Measured worst err/err_ref (bound 4): 2.96 / 3.74, layernorm_f32's figures to the digit.
    wst = Worst(f"splitk_layernorm D={D}")
    zero = torch.zeros(D, device="cuda")
    for rows in LN_ROWS:
        for profile in KI.LN_PROFILES + ("zero",):
            x, w, b, ref, err_ref, floor = ln_case(profile, rows, D)
            res = torch.zeros(rows, D, device="cuda")
            xo, planes = K.splitk_layernorm(x.view(1, rows, D), zero, res, None, (w, b, EPS))
            x_only, none = K.splitk_layernorm(x.view(1, rows, D), zero, res, None)
            tag = (profile, rows, D)
            assert none is None and torch.equal(xo, x) and torch.equal(x_only, x), tag
            assert not torch.isnan(planes.float()).any(), tag
            if profile == "zero":
                assert torch.equal(planes.double().sum(0), b.double().expand(rows, D)), tag
            else:
                wst.check((planes.double().sum(0) - ref).abs().max().item(), err_ref, floor, tag)
    wst.done()


# ---- companions ---------------------------------------------------------------------------------
def test_split3_special_values(K):
    x = KI.split3_points()
    p = K.split3(x.cuda())
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), K.split3(x)), "GPU planes != CPU split3"
    big = x.abs() >= 2.0 ** -100
    assert big.sum() > 400 and (~big).sum() > 40
    assert torch.isfinite(p.float()).all()
    recon = p.double().sum(0).cpu()
    assert torch.equal(recon[big], x.double()[big])
    zeros = x == 0
    assert (p[:, zeros.cuda()] == 0).all()


@pytest.mark.parametrize("rows", [1, 7, 33, 100, 129])
def test_detection_heads_row_counts(K, rows):
    from walkai_nos_amd.models.workload.yolos import YolosSmall
    torch.manual_seed(4)
    m = YolosSmall().cuda().eval()
    for prm in list(m.cls_head.parameters()) + list(m.box_head.parameters()) + list(m.ln_f.parameters()):
        prm.data.normal_(0, 0.05)
    det = torch.randn(rows, 384, device="cuda")
    with torch.no_grad():
        logits, boxes = K.detection_heads(det, m.ln_f, m.cls_head.layers, m.box_head.layers)
        h = F.layer_norm(det.double(), (384,), m.ln_f.weight.double(), m.ln_f.bias.double(), m.ln_f.eps)

        def mlp(layers, x):
            for i, l in enumerate(layers):
                x = x @ l.weight.double().t() + l.bias.double()
                if i < len(layers) - 1:
                    x = torch.relu(x)
            return x
        ref_l, ref_b = mlp(m.cls_head.layers, h), torch.sigmoid(mlp(m.box_head.layers, h))
    torch.cuda.synchronize()
    assert logits.shape == (rows, 92) and boxes.shape == (rows, 4)
    assert (logits.double() - ref_l).abs().max().item() < 1e-5
    assert (boxes.double() - ref_b).abs().max().item() < 1e-6
