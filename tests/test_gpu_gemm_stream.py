"""The persistent x3 GEMM stream (``gemm_x3s``, tiles 100-110) across tile boundaries and grids, and the
grouped tile order on every kernel family (GPU only).

One workgroup of the persistent kernel carries its DMA ring across tile boundaries: the next tile's
first stages load while the current tile's last MFMAs and its epilogue run. Here every persistent
tile runs at the smallest shapes where that can go wrong: N = 256 (2-8 tile columns), tile rows that
end in a one-row block, K stages nk = 1, 2, 3, 6, 12 (a boundary every stage, on every slot of the
S-stage ring), and grids from one workgroup that streams every tile to one workgroup per tile, forced
through the production launch path (``set_slice_cus`` + ``NOS_X3_PGRID_SLACK``). The library's own
walk of the schedule (``gemm.x3_schedule``) says which grid a launch uses and how long each
workgroup's stream is; the test asserts that both ``xcd_band`` branches, unequal per-workgroup tile
counts and the stream lengths 1, S-1, S, 2S-2, 2S-1, 2S and >= 3S+1 occurred.

References are fp64 of the same fp32 inputs, computed once per K. ``randn`` inputs are held to the
suite's bound for this kernel (2x the f32-input MFMA GEMM's error on the same rows, floor 1e-5); a
position-coded integer input (every product and partial sum an integer far below 2^24) must come
out exact, so a wrong tile, stage or a missed accumulator reset is a wrong integer. On top: the
result is the same bits whatever the grid, the group or the pin, the same bits as the
one-tile-per-workgroup twin of the same template arguments, and the same bits twice.

The issue's shapes (M = BM-1, 3 BM, 2 BM+1) give at most 6 tiles on the 128-wide tiles and no
workgroup 2S-1 tiles for S >= 3, so one more M (max(2S-1, 5) tile rows, the last of one row) and one
more grid (the tile columns) are added: with them every tile reaches both ``xcd_band`` branches and
a stream of 2S-1 one-stage tiles.

Worst measured figures (MI355X; ``profiles/pytest_gpu_gemm_stream.log``, one ``[stream]`` line per
test) stand beside each bound."""
import math
import os

import pytest
import torch

from kernel_inputs import Worst

pytestmark = pytest.mark.gpu

N = 256
KS = (32, 64, 96, 192, 384)
GRIDS = (1, 2, 3, 5, 8, 9, 16)
ROWS = 1280  # the most rows any shape below takes: 5 tile rows of 256
NAN = float("nan")
#: persistent tile -> the one-tile-per-workgroup tile of the same template arguments
TWINS = {100: 7, 101: 12, 102: 13, 103: 10, 104: 9, 105: 18, 106: 20, 107: 23, 108: 25, 109: 26, 110: 35}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from walkai_nos_amd.ops import kernels
    assert kernels.hip_available(), "libnos_kernels.so must be built on a GPU box"
    kernels.set_backend("hip")
    yield kernels
    kernels.set_slice_pin(0)
    kernels.set_slice_cus(None)


@pytest.fixture(scope="module")
def G(K):
    from walkai_nos_amd.ops import gemm
    return gemm


@pytest.fixture
def launch_knobs(K, G):
    """The knobs of the launch path back where they were: slice, pin, grid slack, group."""
    slack = os.environ.get("NOS_X3_PGRID_SLACK")
    yield
    K.set_slice_pin(0)
    K.set_slice_cus(None)
    if slack is None:
        os.environ.pop("NOS_X3_PGRID_SLACK", None)
    else:
        os.environ["NOS_X3_PGRID_SLACK"] = slack
    G.set_group_m(int(os.environ.get("NOS_X3_GROUP_M", G.X3_GROUP_M)))


def force_grid(K, G, cfg, g):
    """Make ``_launch_x3`` ask for ``g`` workgroups of persistent tile ``cfg``: a slice of
    ceil(g / slots) CUs and the slack that takes the rest off its resident slots."""
    slots = G.X3_SLOTS_PER_CU[cfg]
    cus = -(-g // slots)
    K.set_slice_cus(cus)
    os.environ["NOS_X3_PGRID_SLACK"] = str(slots * cus - g)
    asked = max(1, G.X3_SLOTS_PER_CU[cfg] * K.slice_cus() - int(os.environ["NOS_X3_PGRID_SLACK"]))
    assert asked == g, (cfg, g, asked)


def free_grid(K):
    K.set_slice_cus(None)
    os.environ.pop("NOS_X3_PGRID_SLACK", None)


def stage_depth(G, cfg):
    return 64 if G.X3_TILES[cfg][3].endswith("64") else 32


# ---- inputs and references ----------------------------------------------------------------------
_cases = {}


def randn_case(Kd, n=N):
    """One ROWS-row problem per Kd: every M takes its first M rows, the fp64 products computed once."""
    if ("randn", Kd, n) not in _cases:
        g = torch.Generator().manual_seed(300 + Kd + n)
        x = torch.randn(ROWS, Kd, generator=g).cuda()
        w = (torch.randn(n, Kd, generator=g) * 0.05).cuda()
        b = torch.randn(n, generator=g).cuda()
        r = torch.randn(ROWS, n, generator=g).cuda()
        r2 = torch.randn(1, 5, n, generator=g).cuda()
        hb = x.double() @ w.double().t() + b.double()
        refs = {"bias": hb, "gelu": 0.5 * hb * (1 + torch.erf(hb / math.sqrt(2))),
                "res2": hb + r.double() + r2.double().reshape(5, n)[torch.arange(ROWS) % 5]}
        _cases[("randn", Kd, n)] = (x, w, b, r, r2, refs)
    return _cases[("randn", Kd, n)]


def coded_case(Kd):
    """Position-coded integers: x[m, k] = ((7m + 3k) mod 13) - 6, w[n, k] = ((5n + k) mod 11) - 5,
    integer bias and residuals. Every row, column and K stage carries its own pattern, and every
    product and partial sum is an integer far below 2^24: fp32 accumulation in any order is exact.
    (Planes 1 and 2 of these operands are zero, which is why ``randn`` runs too.)"""
    if ("coded", Kd) not in _cases:
        m, n, k = torch.arange(ROWS)[:, None], torch.arange(N)[:, None], torch.arange(Kd)[None, :]
        x = (((7 * m + 3 * k) % 13) - 6).float()
        w = (((5 * n + k) % 11) - 5).float()
        b = ((torch.arange(N) % 7) - 3).float()
        r = (((3 * m + 2 * torch.arange(N)[None, :]) % 17) - 8).float()
        r2 = (((4 * torch.arange(5)[:, None] + torch.arange(N)[None, :]) % 9) - 4).float().reshape(1, 5, N)
        hb = x.double() @ w.double().t() + b.double()
        refs = {"bias": hb, "res2": hb + r.double() + r2.double().reshape(5, N)[torch.arange(ROWS) % 5]}
        bound = (x.double().abs() @ w.double().abs().t()).max().item() + 3 + 8 + 4  # every partial sum, any order
        for ref in refs.values():
            assert torch.equal(ref, ref.round()) and ref.abs().max().item() <= bound < 2 ** 24, (Kd, bound)
        _cases[("coded", Kd)] = tuple(t.cuda() for t in (x, w, b, r, r2)) + ({k_: v.cuda() for k_, v in refs.items()},)
    return _cases[("coded", Kd)]


def epilogues(b, r, r2, M, names=("bias", "gelu", "res2")):
    every = {"bias": {"bias": b}, "gelu": {"bias": b, "gelu": True},
             "res2": {"bias": b, "residual": r[:M], "residual2": r2}}
    return {n: every[n] for n in names}


_err_f32 = {}


def err_f32(G, Kd, M, name, x, w, kw, ref):
    """The yardstick: the f32-input MFMA GEMM's error on the same rows (as the tile-edge tests)."""
    key = (Kd, M, name, w.shape[0])
    if key not in _err_f32:
        f32 = G.gemm(x[:M], w, tile=G.eligible(M, w.shape[0], Kd)[0], **kw)
        _err_f32[key] = (f32.double() - ref).abs().max().item()
    return _err_f32[key]


def guarded(M, planes=None, n=N):
    """A NaN-filled buffer with 3 guard rows before and 4 after the ``[M, n]`` (or ``[planes, M, n]``) view."""
    rows = M * (planes or 1)
    buf = torch.full((rows + 7, n), NAN, device="cuda")
    view = buf[3:3 + rows]
    return buf, (view if planes is None else view.view(planes, M, n))


def guards_untouched(buf):
    return bool(torch.isnan(torch.cat([buf[:3], buf[-4:]])).all())


def run_x3(G, x3, M, w, cfg, kw):
    """fp32 + x3 planes into a guarded NaN view; returns them after the checks every launch gets."""
    buf, view = guarded(M)
    y, y3 = G.gemm_x3(x3[:, :M], w, tile=cfg, out_f32=True, out_x3=True, out=view, **kw)
    assert y.data_ptr() == view.data_ptr() and guards_untouched(buf), (cfg, M)
    assert not torch.isnan(y).any() and not torch.isnan(y3.float()).any(), (cfg, M)
    assert torch.equal(y3.double().sum(0), y.double()), (cfg, M)
    return y, y3


# ---- the plan: which (M, grid) a tile runs, read from the library's schedule -----------------------
def stream_plan(G, cfg):
    """``[(M, tiles_m, tiles_n, [(grid, schedule), ...]), ...]`` for a persistent tile: the issue's M
    (BM - 1, 3 BM, 2 BM + 1) and grids (1, 2, 3, 5, 8, 9, 16, tiles - 1, tiles; those above the tile
    count clamp to it and drop out as duplicates) plus the M and grid of the module docstring."""
    bm, bn, S, _ = G.X3_TILES[cfg]
    tiles_n = N // bn
    plan = []
    for M in (bm - 1, 3 * bm, 2 * bm + 1, (max(2 * S - 1, 5) - 1) * bm + 1):
        tiles_m = -(-M // bm)
        tiles = tiles_m * tiles_n
        grids = {}
        for g in GRIDS + (tiles_n, tiles - 1, tiles):
            if 1 <= g <= tiles:
                s = G.x3_schedule(tiles_m, tiles_n, 1, g, 0, True)
                assert s["P"] == g and s["nx"] == 8 and sum(c for c, _, _ in s["wg"]) == tiles, (cfg, M, g)
                grids[g] = s
        plan.append((M, tiles_m, tiles_n, sorted(grids.items())))
    return plan


def stream_lengths_wanted(S):
    return {1, S - 1, S, 2 * S - 2, 2 * S - 1, 2 * S}


def test_twin_table_matches_the_tile_table(G):
    assert set(TWINS) == set(G.X3_PERSISTENT) == set(range(100, 111))
    for p, d in TWINS.items():
        assert G.X3_TILES[p][:3] == G.X3_TILES[d][:3] and stage_depth(G, p) == stage_depth(G, d), (p, d)
        assert G.X3_TILES[p][3].startswith("p") and not G.X3_TILES[d][3].startswith("p"), (p, d)


@pytest.mark.parametrize("cfg", sorted(TWINS))
def test_persistent_stream_across_tile_boundaries_and_grids(K, G, cfg, launch_knobs):
    # Every persistent tile: M x K x grid x epilogue, randn (bound 2x the f32 MFMA GEMM's error) and
    # position-coded integers (exact), fp32 + planes into a NaN-guarded view, planes-only launch,
    # the same launch twice, every grid and the one-tile-per-workgroup twin bit for bit.
    # Measured worst err/err_f32 (bound 2): 1.30 on the 32-deep tiles (Kd = 32, M = BM - 1, residuals), 1.04 on
    # the 64-deep ones; 1425-2400 launches and 190-320 exact integer results per tile, 0.3-1.1 s each.
    bm, bn, S, _ = G.X3_TILES[cfg]
    bks = stage_depth(G, cfg)
    plan = stream_plan(G, cfg)
    wst = Worst(f"gemm_x3s tile {cfg} ({bm}x{bn} S{S} BK{bks}) stream", factor=2.0, label="stream")
    lengths, branches, unequal, launches, exact = set(), set(), 0, 0, 0
    try:
        for Kd in KS:
            if Kd % bks:
                continue
            nk = Kd // bks
            for kind in ("randn", "coded"):
                x, w, b, r, r2, refs = randn_case(Kd) if kind == "randn" else coded_case(Kd)
                x3 = K.split3(x)
                for M, tiles_m, tiles_n, grids in plan:
                    for name, kw in epilogues(b, r, r2, M, tuple(refs)).items():
                        ref = refs[name][:M]
                        free_grid(K)
                        twin = run_x3(G, x3, M, w, TWINS[cfg], kw)
                        for g, sched in grids:
                            tag = (cfg, kind, Kd, M, name, g)
                            force_grid(K, G, cfg, g)
                            y, y3 = run_x3(G, x3, M, w, cfg, kw)
                            again = run_x3(G, x3, M, w, cfg, kw)
                            only3 = G.gemm_x3(x3[:, :M], w, tile=cfg, out_f32=False, out_x3=True, **kw)
                            launches += 3
                            if kind == "randn":
                                wst.check((y.double() - ref).abs().max().item(),
                                          err_f32(G, Kd, M, name, x, w, kw, ref), 1e-5, tag)
                            else:
                                assert torch.equal(y.double(), ref), (tag, (y.double() - ref).abs().max().item())
                                exact += 1
                            assert torch.equal(again[0], y) and torch.equal(again[1], y3), tag
                            assert torch.equal(only3, y3), tag
                            assert torch.equal(y, twin[0]) and torch.equal(y3, twin[1]), \
                                (tag, (y - twin[0]).abs().max().item())
                            counts = [c for c, _, _ in sched["wg"]]
                            lengths |= {c * nk for c in counts}
                            branches.add("band" if sched["P"] % sched["nx"] == 0 else "sweep")
                            unequal += len(set(counts)) > 1
    finally:
        free_grid(K)
    print(f"[stream] tile {cfg}: {launches} persistent launches, {exact} exact integer results, "
          f"stream lengths {sorted(lengths)}, xcd_band branches {sorted(branches)}, {unequal} grids with unequal tile counts")
    assert branches == {"band", "sweep"} and unequal > 0, (cfg, branches, unequal)
    assert stream_lengths_wanted(S) <= lengths and max(lengths) >= 3 * S + 1, (cfg, S, sorted(lengths))
    assert exact > 0
    wst.done()


# ---- pins ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [100, 102, 107, 110])
def test_pinned_persistent_stream_bit_identical(K, G, cfg, launch_knobs):
    # the stream under a partition pin: P is whole rounds of the mask's XCDs (always the band branch,
    # workgroups past the tile count idle); grids 1, one that is no multiple of nx, and tiles
    # Measured worst err/err_f32 (bound 2): 0.53-1.00.
    bm, bn, S, _ = G.X3_TILES[cfg]
    Kd, M = 192, 2 * bm + 1
    tiles_m, tiles_n = 3, N // bn
    tiles = tiles_m * tiles_n
    x, w, b, r, r2, refs = randn_case(Kd)
    x3 = K.split3(x)
    kw = epilogues(b, r, r2, M)["res2"]
    wst = Worst(f"gemm_x3s tile {cfg} pinned", factor=2.0, label="stream")
    free_grid(K)
    base = run_x3(G, x3, M, w, cfg, kw)
    ran = 0
    try:
        for mask in (1 << 5, 0b0011, 0x0F):
            nx = bin(mask).count("1")
            odd = next(g for g in (3, 5, 7) if g % nx or nx == 1)
            assert odd < tiles
            for g in (1, odd, tiles):
                s = G.x3_schedule(tiles_m, tiles_n, 1, g, mask, True)
                assert s["nx"] == nx and s["P"] == nx * -(-g // nx) and s["phys"] == 8 * -(-g // nx), (cfg, mask, g, s["P"])
                assert sorted(u[0] for units in s["units"] for u in units) == list(range(tiles)), (cfg, mask, g)
                force_grid(K, G, cfg, g)
                K.set_slice_pin(mask)
                y, y3 = run_x3(G, x3, M, w, cfg, kw)
                K.set_slice_pin(0)
                tag = (cfg, mask, g)
                assert torch.equal(y, base[0]) and torch.equal(y3, base[1]), (tag, (y - base[0]).abs().max().item())
                wst.check((y.double() - refs["res2"][:M]).abs().max().item(),
                          err_f32(G, Kd, M, "res2", x, w, kw, refs["res2"][:M]), 1e-5, tag)
                ran += 1
    finally:
        K.set_slice_pin(0)
        free_grid(K)
    assert ran == 9
    wst.done()


# ---- grouped tile order -------------------------------------------------------------------------
GROUPS = (2, 3, 7, 255)
GROUP_K = 96
SPLITK_N = 384  # the narrowest width splitk_layernorm takes
TILE_ROWS = (1, 2, 3, 5)


def group_rows(bm):
    """M for 1, 2, 3 and 5 tile rows with a partial last block (31 rows or more of it left)."""
    return [tm * bm - 33 for tm in TILE_ROWS]


def f32a_guarded(G, x, M, w, cfg, b, r, r2):
    """``nos_gemm_x3_f32a`` (bias + residual + residual2) straight into guarded NaN views."""
    w3 = G.weight_planes(w)
    buf, view = guarded(M)
    o3 = torch.full((3, M, N), NAN, dtype=torch.bfloat16, device="cuda")
    xm, rm, r2m = x[:M].contiguous(), r[:M].contiguous(), r2.reshape(-1, N).contiguous()
    rc = G._lib_x3().nos_gemm_x3_f32a(xm.data_ptr(), w3.data_ptr(), w3[0].numel(), b.data_ptr(), rm.data_ptr(),
                                      r2m.data_ptr(), r2m.shape[0], view.data_ptr(), o3.data_ptr(), o3[0].numel(),
                                      M, N, x.shape[1], 1 | 4 | 8, cfg, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, G._lib_x3().nos_gemm_x3_last_error().decode()
    assert guards_untouched(buf) and not torch.isnan(view).any() and not torch.isnan(o3.float()).any(), (cfg, M)
    assert torch.equal(o3.double().sum(0), view.double()), (cfg, M)
    return view, o3


@pytest.mark.parametrize("family", ["x3-3", "x3-4", "x3d-11", "m16-29", "x3t-38", "f32a-0", "f32a-1",
                                    "splitk-11", "x3s-100", "x3s-102"])
def test_grouped_tile_order_on_every_kernel_family(K, G, family, launch_knobs, monkeypatch):
    # group > 1 (the last group short for groups 2 and 3 at 3 and 5 tile rows) on every template
    # family: a NaN-prefilled guarded output fully written, the fp64 bound, and the bits of group 1
    # Measured worst err/err_f32 (bound 2): 0.81 (split-K + splitk_layernorm) to 1.29 (128x128 tiles, 5 tile rows).
    monkeypatch.setenv("NOS_X3_STAGGER", "1")
    kind, cfg = family.split("-")
    cfg = int(cfg)
    bm = G.X3A_TILES[cfg][0] if kind == "f32a" else G.X3_TILES[cfg][0]
    x, w, b, r, r2, refs = randn_case(GROUP_K)
    x3 = K.split3(x)
    if kind == "splitk":
        x3w = K.split3(randn_case(GROUP_K, SPLITK_N)[0])
        g = torch.Generator().manual_seed(9)
        lnw, lnb = torch.randn(SPLITK_N, generator=g).cuda(), torch.randn(SPLITK_N, generator=g).cuda()
    wst = Worst(f"grouped order {family}", factor=2.0, label="stream")
    short, ran = 0, 0

    def launches(M):
        """name -> tensors to compare bit for bit with group 1; the fp64 checks are made on the way"""
        kw = epilogues(b, r, r2, M)["res2"]
        ref = refs["res2"][:M]
        e32 = err_f32(G, GROUP_K, M, "res2", x, w, kw, ref)
        out = {}
        if kind == "f32a":
            out["f32a"] = f32a_guarded(G, x, M, w, cfg, b, r, r2)
        elif kind == "splitk":
            # N = 256 has no combine kernel (splitk_layernorm: 384 and 768 wide): there the planes are
            # added here, and the same rows run again 384 wide through splitk_layernorm
            for sp in (2, 3):
                buf, view = guarded(M, planes=sp)
                part = G.gemm_x3_partials(x3[:, :M], w, cfg, sp, out=view)
                assert part.data_ptr() == view.data_ptr() and guards_untouched(buf) and not torch.isnan(part).any(), (M, sp)
                out[f"splits {sp}"] = (part, part.double().sum(0) + b.double() + ref - refs["bias"][:M])
                xw, ww, bw, rw, r2w, refs_w = randn_case(GROUP_K, SPLITK_N)
                buf, view = guarded(M, planes=sp, n=SPLITK_N)
                part = G.gemm_x3_partials(x3w[:, :M], ww, cfg, sp, out=view)
                assert part.data_ptr() == view.data_ptr() and guards_untouched(buf) and not torch.isnan(part).any(), (M, sp)
                xo, planes = K.splitk_layernorm(part, bw, rw[:M].contiguous(), r2w, (lnw, lnb, 1e-12))
                assert not torch.isnan(planes.float()).any(), (M, sp)
                kww = epilogues(bw, rw, r2w, M)["res2"]
                wst.check((xo.double() - refs_w["res2"][:M]).abs().max().item(),
                          err_f32(G, GROUP_K, M, "res2", xw, ww, kww, refs_w["res2"][:M]), 1e-5, (family, M, sp, SPLITK_N))
                out[f"splits {sp} x {SPLITK_N}"] = (part, xo, planes)
        else:
            for g in ((1, 5) if kind == "x3s" else (None,)):
                if g is not None:
                    force_grid(K, G, cfg, g)
                out[f"grid {g}"] = run_x3(G, x3, M, w, cfg, kw)
        for name, ts in out.items():
            if not name.endswith(str(SPLITK_N)):
                wst.check((ts[1 if kind == "splitk" else 0].double() - ref).abs().max().item(), e32, 1e-5, (family, M, name))
        return out

    try:
        for M in group_rows(bm):
            tiles_m = -(-M // bm)
            G.set_group_m(1)
            base = launches(M)
            for group in GROUPS:
                short += 0 < tiles_m % group < tiles_m
                G.set_group_m(group)
                got = launches(M)
                for name in base:
                    for u, v in zip(base[name], got[name]):
                        assert torch.equal(u, v), (family, M, group, name, (u.float() - v.float()).abs().max().item())
                ran += 1
    finally:
        G.set_group_m(int(os.environ.get("NOS_X3_GROUP_M", G.X3_GROUP_M)))
        free_grid(K)
    assert ran == len(TILE_ROWS) * len(GROUPS) and short > 0
    wst.done()
