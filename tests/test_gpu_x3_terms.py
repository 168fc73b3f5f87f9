"""Every kept product of the x3 plane product, pinned bit for bit on every kernel that holds a copy of
``mfma_x3`` (GPU only).

An fp32 product runs as six bf16 MFMA products (a2b0, a1b1, a0b2, a1b0, a0b1, a0b0). On ``randn`` a
missing second-order one moves the result by 2^-16 relative: under the suite's error bounds at
Kd <= 64 and in the split-K, stream-K and fused tests, and a fault in one buffer or stage under all.
The inputs of ``tests/kernel_inputs.py`` (``term_case``, ``selector_qkv``) have a six-term product
that is exact in fp32 in any order, so every comparison here is ``torch.equal`` against the fp64
product cast to fp32, and a dropped or misread plane, a stale ring buffer, a wrong key-block base or
merge slot is a changed bit. ``tests/test_kernel_inputs.py`` proves on the CPU which terms each case
pins (``a0b``: a0b0 a0b1 a0b2; ``ab0``: a0b0 a1b0 a2b0; ``a1b1`` and ``dense2``: a0b0 a0b1 a1b0 a1b1).
The second-order terms of the attention kernels' Q K^T product are not pinned: the selector's scores
are one-plane numbers.

The one-hot cases place row m's nonzero by ``onehot_k``; a tile of BM rows runs M = 2 BM + 1 rows (a
one-row last block) over as many placements as it takes to hit every (row mod 32, k div 8) pair,
which each test asserts from the index arrays it ran.

Every test prints one ``[terms]`` line: kernel family, launches, unequal outputs (0). The MI355X run
is kept in ``profiles/pytest_gpu_x3_terms.log``."""
import os

import pytest
import torch

import kernel_inputs as KI
from kernel_inputs import Exact
from test_gpu_gemm_stream import force_grid, free_grid
from test_gpu_kernel_edges import SCALE, grids, guarded, guards_untouched, nan_out, restore_attention

pytestmark = pytest.mark.gpu

N = KI.TERM_N
NAN = float("nan")
ONEHOT_A = ("a0b", "a1b1")  # the cases whose A rows hold one nonzero


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from walkai_nos_amd.ops import kernels
    assert kernels.hip_available(), "libnos_kernels.so must be built on a GPU box"
    kernels.set_backend("hip")
    yield kernels
    kernels.set_slice_cus(None)


@pytest.fixture(scope="module")
def G(K):
    from walkai_nos_amd.ops import gemm
    return gemm


@pytest.fixture
def launch_knobs(K, G, monkeypatch):
    """The staggered tile offered, and slice, grid slack and group back where they were."""
    monkeypatch.setenv("NOS_X3_STAGGER", "1")
    slack = os.environ.get("NOS_X3_PGRID_SLACK")
    yield
    K.set_slice_cus(None)
    if slack is None:
        os.environ.pop("NOS_X3_PGRID_SLACK", None)
    else:
        os.environ["NOS_X3_PGRID_SLACK"] = slack
    G.set_group_m(int(os.environ.get("NOS_X3_GROUP_M", G.X3_GROUP_M)))


_cases = {}


def case(K, kind, M, Kd, phase=0, n=N):
    """A ``term_case`` on the GPU with the activation's planes, built once."""
    key = (kind, M, Kd, phase, n)
    if key not in _cases:
        c = KI.term_case(kind, M, Kd, phase, n)
        g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items()}
        g["A3"] = K.split3(g["A"])
        g["ref64"] = g["ref"].double()
        _cases[key] = g
    return _cases[key]


def placements(kind, M, Kd, n=N):
    """The placements a one-hot case needs for full coverage: of A's M rows, or of W's n rows."""
    if kind == "dense2":
        return range(1)
    return range(KI.onehot_phases(M if kind in ONEHOT_A else n, Kd))


def every_case(K, M, Kd, n=N):
    """Every case and placement for M rows, after asserting from the index arrays that the one-hot
    placements hit every (row mod 32, k div 8) pair, rows of A and rows of W alike."""
    want = 32 * (Kd // 8)
    out = []
    for kind in KI.TERM_CASES:
        cs = [case(K, kind, M, Kd, p, n) for p in placements(kind, M, Kd, n)]
        if kind in ONEHOT_A:
            assert len(KI.onehot_pairs([c["ka"].cpu() for c in cs], Kd)) == want, (kind, M, Kd)
        elif kind == "ab0":
            assert len(KI.onehot_pairs([c["kw"].cpu() for c in cs], Kd)) == want, (kind, n, Kd)
        out += [(kind, p, c) for p, c in enumerate(cs)]
    return out


def x3_launch(G, c, M, cfg, ex, tag, **kw):
    """fp32 + planes into a NaN-guarded view against ``ref`` (default: the case's own)."""
    ref = kw.pop("ref", c["ref"])
    buf, view = guarded(M, NAN)
    y, y3 = G.gemm_x3(c["A3"], c["W"], tile=cfg, out_f32=True, out_x3=True, out=view, **kw)
    ex.launches += 1
    assert y.data_ptr() == view.data_ptr() and guards_untouched(buf, NAN), tag
    ex.check(y, ref, tag)
    ex.check(y3.double().sum(0), ref.double(), tag + ("planes",))


# ---- GEMM ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kd", KI.TERM_KDS)
def test_gemm_x3_every_tile_exact_terms(K, G, Kd, launch_knobs):
    # every tile of the table (persistent and staggered included), M = 2 BM + 1, every case and
    # placement; group 3 on the first placement; the persistent tiles at forced grids 1, 5 and one
    # workgroup per tile besides the slice's own
    tiles = G.x3_eligible(N, Kd)
    expect = [c for c, (bm, bn, _, kind) in G.X3_TILES.items()
              if N % bn == 0 and (Kd % 64 == 0 or not kind.endswith("64"))]
    assert tiles == expect and len(tiles) >= 30 and 38 in tiles
    ex = Exact(f"gemm_x3 Kd={Kd}")
    ran, forced = {}, set()
    try:
        for cfg in tiles:
            bm, bn = G.X3_TILES[cfg][:2]
            M = 2 * bm + 1
            n_tiles = 3 * (N // bn)
            gs = (None, 1, 5, n_tiles) if cfg in G.X3_PERSISTENT else (None,)
            for kind, p, c in every_case(K, M, Kd):
                for group in ((1, 3) if p == 0 else (1,)):
                    G.set_group_m(group)
                    for g in gs:
                        if g is None:
                            free_grid(K)
                        else:
                            force_grid(K, G, cfg, g)
                            forced.add((cfg, g))
                        x3_launch(G, c, M, cfg, ex, (cfg, kind, p, group, g))
                        ran[cfg] = ran.get(cfg, 0) + 1
    finally:
        free_grid(K)
    assert sorted(ran) == sorted(tiles) and all(v >= 6 for v in ran.values()), ran
    persistent = [c for c in tiles if c in G.X3_PERSISTENT]
    assert persistent and all(sum(1 for c, _ in forced if c == t) == 3 for t in persistent), forced
    assert ex.launches == sum(ran.values())
    ex.done(f", {len(tiles)} tiles ({len(persistent)} persistent, 3 forced grids each)")


@pytest.mark.parametrize("Kd", KI.TERM_KDS)
def test_gemm_x3_f32a_exact_terms(K, G, Kd, launch_knobs):
    # the fp32-activation kernel splits A in registers: against the exact product itself
    ex = Exact(f"gemm_x3_f32a Kd={Kd}")
    ran = 0
    for cfg, (bm, bn) in G.X3A_TILES.items():
        M = 2 * bm + 1
        for kind, p, c in every_case(K, M, Kd):
            for group in ((1, 3) if p == 0 else (1,)):
                G.set_group_m(group)
                y, y3 = G.gemm_x3_f32a(c["A"], c["W"], out_x3=True, cfg=cfg)
                ex.launches += 1
                ex.check(y, c["ref"], (cfg, kind, p, group))
                ex.check(y3.double().sum(0), c["ref64"], (cfg, kind, p, group, "planes"))
        ran += 1
    assert ran == len(G.X3A_TILES) == 2
    ex.done()


def owners(k, nk, bks, sp):
    """The split whose K stages [s nk / sp, (s + 1) nk / sp) hold column k (csrc/gemm_x3.hip)."""
    stage = k // bks
    own = torch.full_like(k, -1)
    for s in range(sp):
        own[(stage >= s * nk // sp) & (stage < (s + 1) * nk // sp)] = s
    assert int(own.min()) >= 0
    return own


def test_splitk_partials_exact_terms(K, G, launch_knobs):
    # gemm_x3_partials over every (tile, splits) of the table: the planes add up to the exact product,
    # a split whose K range holds no nonzero of a row (a column, for ab0) is exactly zero there, and
    # splitk_layernorm's x with zero bias and residual is the exact product
    ex = Exact("gemm_x3 split-K partials + splitk_layernorm")
    zero_b = torch.zeros(N, device="cuda")
    ran = eligible = zeros = 0
    counts, idle_splits, every_split = {}, set(), set()
    for Kd in KI.TERM_KDS:
        cands = G.split_candidates(N, Kd)
        every_split |= {(cfg, sp, s) for cfg, sp in cands for s in range(sp)}
        assert (len(cands) > 0) == (Kd >= 128), (Kd, cands)
        counts[Kd] = sorted({sp for _, sp in cands})
        for cfg, sp in cands:
            eligible += 1
            bm = G.X3_TILES[cfg][0]
            bks = 64 if G.X3_TILES[cfg][3].endswith("64") else 32
            M = 2 * bm + 1
            res = torch.zeros(M, N, device="cuda")
            for kind, p, c in every_case(K, M, Kd):
                tag = (Kd, cfg, sp, kind, p)
                part = G.gemm_x3_partials(c["A3"], c["W"], cfg, sp, out=torch.full((sp, M, N), NAN, device="cuda"))
                ex.launches += 1
                ex.check(part.double().sum(0), c["ref64"], tag)
                for k, rows in ((c["ka"], True), (c["kw"], False)):
                    if k is not None:
                        own = owners(k, Kd // bks, bks, sp)
                        for s in range(sp):
                            idle = part[s][own != s] if rows else part[s][:, own != s]
                            if idle.numel():  # one placement of a short M may put every row in one split
                                ex.check(idle, torch.zeros_like(idle), tag + ("idle split", s))
                                zeros += 1
                                idle_splits.add((cfg, sp, s))
                xo, none = K.splitk_layernorm(part, zero_b, res, None)
                assert none is None
                ex.check(xo, c["ref"], tag + ("splitk_layernorm",))
            ran += 1
    assert ran == eligible > 0 and zeros > 0 and idle_splits == every_split
    assert len(counts[192]) >= 2, counts  # the deepest K offers two split counts
    ex.done(f", {ran} (tile, splits) pairs, {zeros} idle-split checks, split counts {counts}")


def test_streamk_partials_exact_terms(K, G, launch_knobs):
    # gemm_x3_streamk over every config the shape allows, P = 1, a prime and one workgroup per unit,
    # into NaN-prefilled partials (a plane a tile does not own stays NaN and is never read)
    ex = Exact("gemm_x3 stream-K partials + streamk_layernorm")
    zero_b = torch.zeros(N, device="cuda")
    ran = 0
    for Kd in KI.TERM_KDS:
        for cfg, (bm, bn, bk, _) in G.X3K_TILES.items():
            if N % bn or Kd % bk:
                continue
            M = 2 * bm + 1
            res = torch.zeros(M, N, device="cuda")
            for P in (1, 7, 1 << 20):
                m = G.streamk_map(M, N, Kd, cfg, P)
                for kind, p, c in every_case(K, M, Kd):
                    part, m2 = G.gemm_x3_streamk(c["A3"], c["W"], cfg, P, out=torch.full((m[6], M, N), NAN, device="cuda"))
                    assert m2 == m
                    ex.launches += 1
                    xo, _ = K.streamk_layernorm(part, m, zero_b, res, None)
                    ex.check(xo, c["ref"], (Kd, cfg, P, kind, p))
                ran += 1
    want = sum(3 for Kd in KI.TERM_KDS for (_, bn, bk, _) in G.X3K_TILES.values() if N % bn == 0 and Kd % bk == 0)
    assert ran == want and ran >= 3 * 15, (ran, want)
    ex.done(f", {ran} (Kd, config, P) runs")


def test_epilogues_add_nothing_inexact(K, G, launch_knobs):
    # integer bias, residual and second residual on the integer accumulator of the a1b1 case: every
    # tile, the fp32-activation kernel and both combine kernels return the exact sum (no GELU here:
    # test_gelu_epilogues_on_exact_preactivations measures it on exact pre-activations)
    Kd = 64
    ex = Exact("x3 epilogues on an exact accumulator")
    n = torch.arange(N)
    b = ((n * 7) % 2001 - 1000).float().cuda()
    r2 = (((torch.arange(5)[:, None] * 11 + n[None, :] * 3) % 4001) - 2000).float().reshape(1, 5, N).cuda()
    ran = 0
    tiles = G.x3_eligible(N, Kd)
    for bm in sorted({G.X3_TILES[c][0] for c in tiles}):
        M = 2 * bm + 1
        c = case(K, "a1b1", M, Kd)
        m = torch.arange(M)
        r = (((m[:, None] * 13 + n[None, :] * 5) % 8001) - 4000).float().cuda()
        ref64 = c["ref64"] + b.double() + r.double() + r2.double().reshape(5, N)[m % 5]
        assert c["ref64"].abs().max().item() + 1000 + 4000 + 2000 < 2 ** 24  # every partial sum of the epilogue
        ref = ref64.float()
        kw = {"bias": b, "residual": r, "residual2": r2}
        for cfg in [t for t in tiles if G.X3_TILES[t][0] == bm]:
            x3_launch(G, c, M, cfg, ex, (cfg, "epilogue"), ref=ref, **kw)
            ran += 1
        for cfg, (abm, _) in G.X3A_TILES.items():
            if abm == bm:
                y = G.gemm_x3_f32a(c["A"], c["W"], cfg=cfg, **kw)
                ex.launches += 1
                ex.check(y, ref, ("f32a", cfg))
                ran += 1
        if bm == 128:
            deep = case(K, "a1b1", M, 128)  # two splits need four stages
            part = G.gemm_x3_partials(deep["A3"], deep["W"], 11, 2)
            ref128 = (deep["ref64"] + b.double() + r.double() + r2.double().reshape(5, N)[m % 5]).float()
            ex.launches += 1
            ex.check(K.splitk_layernorm(part, b, r, r2)[0], ref128, ("splitk_layernorm",))
            part, sk = G.gemm_x3_streamk(c["A3"], c["W"], 3, 7)
            ex.launches += 1
            ex.check(K.streamk_layernorm(part, sk, b, r, r2)[0], ref, ("streamk_layernorm",))
            ran += 2
    assert ran == len(tiles) + len(G.X3A_TILES) + 2
    ex.done(f", {len(tiles)} tiles")


# ---- attention ----------------------------------------------------------------------------------
SELECT_H = 2
_sel = {}


def selector(B, T, H=SELECT_H):
    if (B, T, H) not in _sel:
        qkv, exp = KI.selector_qkv(B, T, H)
        _sel[(B, T, H)] = (qkv.cuda(), exp.cuda())
    return _sel[(B, T, H)]


def check_attn(ex, out, exp, tag):
    ex.launches += 1
    if out.dtype == torch.bfloat16:
        ex.check(out.double().sum(0), exp.double(), tag)
    else:
        ex.check(out, exp, tag)


@pytest.mark.parametrize("T", sorted(KI.SELECT_PERM))
def test_attention_selects_one_value_row_bit_for_bit(K, T):
    # out[b, t, h] == V[b, pi(t), h]: every p, alpha and merge weight is exactly 1 or 0, so the P V
    # product (p0 v0 + p0 v1 + p0 v2 with V generic), the key-block base, the merges and the fixups of
    # every attention kernel are pinned to the bit. Within the first query tile the selected keys lie
    # in the first key block, a middle one (T = 257) and the tail key's block.
    pi = KI.selector_perm(T)
    nk = (T + 31) // 32
    blocks = set((pi[:32] // 32).tolist())
    assert 0 in blocks and (T - 1) // 32 in blocks and (nk <= 2 or blocks & set(range(1, nk - 1))), (T, blocks)
    H = SELECT_H
    ex = Exact(f"attention selector T={T}")
    L = K._L()
    seen = set()
    try:
        for B in (1, 2):
            qkv, exp = selector(B, T)
            planes = K.split3(qkv)
            # fp32 in: wide and two-wave, fixup launch / in-kernel merge / the XCD-local fixup order
            for wide in (True, False):
                K.set_attention_x3_wide(wide)
                for mode in ("fixup", "merge", "xcd-fixup"):
                    if mode == "merge" and not wide:
                        continue  # the in-kernel merge is the wide kernel's
                    K.set_attention_merge(mode == "merge")
                    L.nos_attention_x3_set_flags(64 if mode == "xcd-fixup" else 0)
                    for hb in (1, H):
                        for x3 in (False, True):
                            for waves in grids(K, B, T, H):
                                out = K.attention_x3f(qkv, nan_out(x3, B, T, H), H, 64, SCALE, waves, head_block=hb)
                                check_attn(ex, out, exp, ("x3f", B, wide, mode, hb, x3, waves))
                                seen.add(("x3f", wide, mode, hb, x3))
                K.set_attention_merge(None)
                L.nos_attention_x3_set_flags(0)
            assert int(K._row_counters(qkv.device, 1).abs().sum().item()) == 0, (B, T)
            # planes in: pipelined with 4 and 8 query tiles per workgroup, and block-at-a-time
            for pipelined, group in ((True, 4), (True, 8), (False, 4)):
                K.set_attention_x3_pipelined(pipelined)
                K.set_attention_x3_group(group)
                for hb in ((1, H) if pipelined else (H,)):  # head blocks are the pipelined kernel's
                    for x3 in (False, True):
                        for waves in grids(K, B, T, H, group):
                            out = K.attention_x3(planes, nan_out(x3, B, T, H), H, 64, SCALE, waves, head_block=hb)
                            check_attn(ex, out, exp, ("x3", B, pipelined, group, hb, x3, waves))
                            seen.add(("x3", pipelined, group, hb, x3))
            restore_attention(K)
            # the f32-input MFMA kernels
            for variant in (0, 2, 3):
                K.set_attention_variant(variant)
                for waves in grids(K, B, T, H):
                    out = K.attention_sk(qkv, nan_out(False, B, T, H), H, 64, SCALE, waves)
                    check_attn(ex, out, exp, ("f32 sk", B, variant, waves))
                    seen.add(("sk", variant))
            K.set_attention_variant(0)
            check_attn(ex, K.attention_unsplit(qkv, H, 64, SCALE), exp, ("f32 unsplit", B))
            seen.add(("unsplit",))
    finally:
        restore_attention(K)
    assert len([s for s in seen if s[0] == "x3f"]) == (3 + 2) * 2 * 2
    assert len([s for s in seen if s[0] == "x3"]) == (2 * 2 + 1) * 2
    assert {s for s in seen if s[0] in ("sk", "unsplit")} == {("sk", 0), ("sk", 2), ("sk", 3), ("unsplit",)}
    assert ex.launches == 2 * 5 * (20 + 10 + 3) + 2
    ex.done(f", {len(seen)} kernel / switch combinations x B 1, 2 x 5 grids")


# ---- attention partials + merge + projection + LayerNorm -----------------------------------------
def test_fused_merge_projection_exact_terms(K):
    # attention_proj_ln_x3f (csrc/attn_proj.hip), H = 6, D = 384: the selector QKV makes the projection's
    # activation the selected V rows to the bit, V and W are the four exact-term cases (dense2 at half
    # density: term_case), bias and residual zero, so x is the exact product. B T = 66 rows: two
    # 32-row tiles and a partial one; every placement of the one-hot cases.
    H, D, B, T = 6, 384, 2, 33
    M = B * T
    pi = KI.selector_perm(T)
    ex = Exact("attn_merge_proj_ln x")
    zero_b, ones = torch.zeros(D, device="cuda"), torch.ones(D, device="cuda")
    res = torch.zeros(B, T, D, device="cuda")
    want = 32 * (D // 8)
    ran = set()
    for kind in KI.TERM_CASES:
        ks = []
        for p in placements(kind, M, D, D):
            c = KI.term_case(kind, M, D, p, N=D)
            ks.append(c["ka"] if kind in ONEHOT_A else c["kw"])
            v = torch.empty(B, T, H, 64)
            v[:, pi] = c["A"].view(B, T, H, 64)
            qkv, exp = KI.selector_qkv(B, T, H, v)
            assert torch.equal(exp.view(M, D), c["A"])
            qkv, w, ref = qkv.cuda(), c["W"].cuda(), c["ref"].cuda().view(B, T, D)
            for waves in grids(K, B, T, H)[:: 2 if p else 1]:
                x, h3 = K.attention_proj_ln_x3f(qkv, H, 64, SCALE, w, zero_b, res, (ones, zero_b, 1e-12), waves=waves)
                ex.launches += 1
                ex.check(x, ref, (kind, p, waves))
                assert h3.shape == (3, B, T, D) and not torch.isnan(h3.float()).any(), (kind, p, waves)
            ran.add(kind)
        if ks[0] is not None:
            assert len(KI.onehot_pairs(ks, D)) == want, kind
    assert ran == set(KI.TERM_CASES)
    ex.done()
