"""The tile schedule of the x3 GEMMs (csrc/x3_schedule.h, csrc/pin.h), checked exhaustively on the
host through the library's own walk of it (``nos_gemm_x3_schedule`` runs the functions the kernels
run): for every tile grid up to 9 x 8, every grouped order, every persistent grid up to tiles + 9
and every kind of pin, each unit is run exactly once, inside the tile grid, by a workgroup that
takes its tiles in stream order; with whole XCD bands (P % nx == 0) each XCD's tiles are one
contiguous logical range; the grouped order is the one the kernel's comment promises. And the
launchers refuse bad arguments before any launch."""
import ctypes
import os

import pytest

from walkai_nos_amd.ops import build

TILES_M = range(1, 10)
TILES_N = range(1, 9)
GROUPS = (1, 2, 3, 4, 7, 255)
PINS = (0, 1 << 5, 0b0011, 0x0F, 0xFF)
SPLITS = (1, 2, 3)


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(build.OUT, "libnos_kernels.so")
    if not os.path.exists(path):
        pytest.skip("libnos_kernels.so not built")
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def schedule(lib):
    from walkai_nos_amd.ops import gemm as G
    return lambda *a, **kw: G.x3_schedule(*a, lib=lib, **kw)


def grouped_order(tiles_m, tiles_n, group):
    """What the comment at ``tile_rc`` promises, written as the walk itself: ``group`` tile rows (the
    last group: what is left) down a column, then the next column, then the next group of rows."""
    order = []
    for r0 in range(0, tiles_m, group):
        for nt in range(tiles_n):
            order += [(mt, nt) for mt in range(r0, min(r0 + group, tiles_m))]
    return order


def logical_workgroups(grid, tiles, pin):
    """(P, nx, physical grid) of a persistent launch: the clamp ``min(grid, tiles)`` and, under a
    pin, whole rounds of 8 physical workgroups of which the mask's XCDs keep theirs (csrc/pin.h)."""
    g = max(1, min(grid, tiles))
    if not pin:
        return g, 8, g
    nx = bin(pin).count("1")
    rounds = -(-g // nx)
    return rounds * nx, nx, 8 * rounds


@pytest.mark.parametrize("group", GROUPS)
def test_persistent_stream_runs_every_tile_once_in_stream_order(schedule, group):
    seen_branch = {"band": 0, "sweep": 0, "unequal": 0, "idle": 0}
    for tiles_m in TILES_M:
        for tiles_n in TILES_N:
            tiles = tiles_m * tiles_n
            order = grouped_order(tiles_m, tiles_n, group)
            assert sorted(order) == [(m, n) for m in range(tiles_m) for n in range(tiles_n)]
            for pin in PINS:
                for grid in range(1, tiles + 10):
                    s = schedule(tiles_m, tiles_n, group, grid, pin, True)
                    tag = (tiles_m, tiles_n, group, grid, pin)
                    P, nx = s["P"], s["nx"]
                    assert (P, nx, s["phys"]) == logical_workgroups(grid, tiles, pin), tag
                    assert s["want"] == tiles and len(s["wg"]) == P, tag
                    counts = [c for c, _, _ in s["wg"]]
                    assert min(counts) >= 0 and sum(counts) == s["ran"] == tiles, (tag, counts)
                    ran = []
                    for (count, base, stride), units in zip(s["wg"], s["units"]):
                        assert len(units) == count, tag
                        assert [u[0] for u in units] == [base + i * stride for i in range(count)], (tag, units)
                        assert count <= 1 or stride > 0, tag
                        ran += units
                    assert sorted(u[0] for u in ran) == list(range(tiles)), (tag, sorted(u[0] for u in ran))
                    for t, mt, nt, sp in ran:
                        assert 0 <= mt < tiles_m and 0 <= nt < tiles_n and sp == 0, (tag, t, mt, nt)
                        assert (mt, nt) == order[t], (tag, t, (mt, nt), order[t])
                    if P % nx == 0:
                        # every XCD's workgroups (w % nx) cover one contiguous logical range, the
                        # ranges in XCD order and as even as the tile count allows
                        at = 0
                        for x in range(nx):
                            mine = sorted(u[0] for w in range(x, P, nx) for u in s["units"][w])
                            assert mine == list(range(at, at + len(mine))), (tag, x, mine)
                            assert len(mine) == tiles // nx + (1 if x < tiles % nx else 0), (tag, x, mine)
                            at += len(mine)
                        assert at == tiles, tag
                    else:
                        assert pin == 0, tag  # a pinned launch is whole rounds: always bands
                    seen_branch["band" if P % nx == 0 else "sweep"] += 1
                    seen_branch["unequal"] += len(set(c for c in counts if c)) > 1
                    seen_branch["idle"] += 0 in counts
    assert all(v > 0 for v in seen_branch.values()), seen_branch


@pytest.mark.parametrize("group", GROUPS)
def test_one_unit_per_workgroup_covers_every_tile_and_split_once(schedule, group):
    for tiles_m in TILES_M:
        for tiles_n in TILES_N:
            tiles = tiles_m * tiles_n
            order = grouped_order(tiles_m, tiles_n, group)
            for pin in PINS:
                for splits in SPLITS:
                    s = schedule(tiles_m, tiles_n, group, 0, pin, False, splits)
                    tag = (tiles_m, tiles_n, group, pin, splits)
                    want = tiles * splits
                    nx = bin(pin).count("1") if pin else 8
                    rounds = -(-want // nx)
                    assert (s["P"], s["nx"], s["phys"]) == ((rounds * nx, nx, 8 * rounds) if pin else (want, 8, want)), tag
                    assert s["want"] == want == s["ran"] == sum(c for c, _, _ in s["wg"]), tag
                    ran = []
                    for (count, base, _), units in zip(s["wg"], s["units"]):
                        assert count in (0, 1) and len(units) == count, tag
                        for t, mt, nt, sp in units:
                            # a tile's splits are adjacent units: unit = tile * splits + split
                            assert (t, sp) == divmod(base, splits) and 0 <= sp < splits, (tag, base, t, sp)
                            assert 0 <= mt < tiles_m and 0 <= nt < tiles_n and (mt, nt) == order[t], (tag, t, mt, nt)
                            ran.append((t, sp))
                    assert sorted(ran) == [(t, sp) for t in range(tiles) for sp in range(splits)], tag


def test_schedule_refuses_bad_arguments(schedule):
    for args in ((0, 4, 1, 4, 0, True, 1), (4, 0, 1, 4, 0, True, 1), (4, 4, 0, 4, 0, True, 1), (4, 4, 256, 4, 0, True, 1),
                 (4, 4, 1, 4, 0x100, True, 1), (4, 4, 1, 4, 0, True, 2), (4, 4, 1, 4, 0, False, 9),
                 (4, 4, 1, 4, 0, False, 0)):
        with pytest.raises(ValueError, match="gemm_x3 schedule"):
            schedule(*args)
    assert schedule(4, 4, 1, 0, 0, True)["P"] == 1 and schedule(4, 4, 1, -3, 0, True)["P"] == 1  # never no workgroup


def test_python_tile_table_is_the_librarys(lib):
    """``gemm.X3_TILES`` is plain data the tuner and the tests index; the library's tables
    (``kTiles``, ``kPersistent`` in csrc/gemm_x3.hip) are what launches. They must agree."""
    from walkai_nos_amd.ops import gemm as G
    i32 = ctypes.c_int
    lib.nos_gemm_x3_tile.argtypes = [i32] + [ctypes.POINTER(i32)] * 3
    for cfg, tile in G.X3_TILES.items():
        bm, bn, nbuf = i32(), i32(), i32()
        assert lib.nos_gemm_x3_tile(cfg, bm, bn, nbuf) == 0, cfg
        assert (bm.value, bn.value, nbuf.value) == tile[:3], (cfg, tile)
    below = [c for c in G.X3_TILES if c < 100]
    assert lib.nos_gemm_x3_num_configs() == len(below) and sorted(below) == list(range(len(below)))
    assert set(G.X3_SLOTS_PER_CU) == set(G.X3_TILES)
    bm = i32()
    for cfg in (-1, len(below), 99, 100 + len(G.X3_PERSISTENT), 1 << 20):  # no id beside the tables answers
        assert lib.nos_gemm_x3_tile(cfg, bm, bm, bm) != 0, cfg
    assert G.X3_PERSISTENT == {100 + i for i in range(len(G.X3_PERSISTENT))}


def test_bad_arguments_are_refused_before_any_launch(lib):
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.nos_gemm_x3_persistent.argtypes = [vp, sz, vp, sz, vp, vp, vp, i32, vp, vp, sz, i32, i32, i32, i32, i32, i32, vp]
    lib.nos_gemm_x3.argtypes = [vp, sz, vp, sz, vp, vp, vp, i32, vp, vp, sz, i32, i32, i32, i32, i32, vp]
    lib.nos_gemm_x3_partials.argtypes = [vp, sz, vp, sz, vp, i32, i32, i32, i32, i32, vp]
    lib.nos_gemm_x3_streamk_map.argtypes = [i32, i32, i32, i32, i32, vp]
    lib.nos_gemm_x3_streamk.argtypes = [vp, sz, vp, sz, vp, i32, i32, i32, i32, i32, vp]
    lib.nos_gemm_x3_f32a.argtypes = [vp, vp, sz, vp, vp, vp, i32, vp, vp, sz, i32, i32, i32, i32, i32, vp]
    lib.nos_gemm_x3_set_group.argtypes = [i32]
    lib.nos_gemm_x3_last_error.restype = ctypes.c_char_p
    host = (ctypes.c_float * 64)()
    p = ctypes.addressof(host)  # never dereferenced: every case below returns before a launch
    skmap = (i32 * 7)()

    # M = 0: were a case ever let through, its workgroups would find no tile and touch nothing
    def persistent(N=128, Kd=64, epi=0, cfg=0, bias=None, R=None, R2=None, r2_rows=0, C=p, Cp=None, wp=None):
        return lib.nos_gemm_x3_persistent(p, 0, p, N * Kd if wp is None else wp, bias, R, R2, r2_rows, C, Cp, 0, 0, N,
                                          Kd, epi, cfg, 4, None)

    def x3(N=128, Kd=64, epi=0, cfg=7, bias=None, R=None, R2=None, r2_rows=0, C=p, Cp=None, ap=0, wp=None, cp=0):
        return lib.nos_gemm_x3(p, ap, p, N * Kd if wp is None else wp, bias, R, R2, r2_rows, C, Cp, cp, 0, N, Kd, epi,
                               cfg, None)

    def partials(N=128, Kd=128, cfg=7, splits=2, C=p, ap=0, wp=None):
        return lib.nos_gemm_x3_partials(p, ap, p, N * Kd if wp is None else wp, C, 0, N, Kd, cfg, splits, None)

    def sk_map(M=64, N=128, Kd=64, cfg=0, P=4):
        return lib.nos_gemm_x3_streamk_map(M, N, Kd, cfg, P, skmap)

    def streamk(M=64, N=128, Kd=64, cfg=0, P=4, C=p, ap=0, wp=None):  # every M > 0 here is refused for another reason
        return lib.nos_gemm_x3_streamk(p, ap, p, N * Kd if wp is None else wp, C, M, N, Kd, cfg, P, None)

    def f32a(N=128, Kd=64, epi=0, cfg=0, A=p, bias=None, R=None, R2=None, r2_rows=0, C=p, Cp=None, wp=None, cp=0):
        return lib.nos_gemm_x3_f32a(A, p, N * Kd if wp is None else wp, bias, R, R2, r2_rows, C, Cp, cp, 0, N, Kd, epi,
                                    cfg, None)

    x3_k32 = "gemm_x3: K must be a multiple of 32 and plane strides multiples of 8 elements"
    s_args = "gemm_x3s: K % 32 (K % 64 for 64-deep stages), plane strides % 8, and an output are required"
    p_args = "gemm_x3 partials: K % 32, plane strides % 8 and an output"
    p_cfg = "gemm_x3 partials: an LDS-DMA config (7..38) and 2..8 splits"
    k_cfg = "gemm_x3k: config 0..5, M > 0 and P > 0"
    k_p = "gemm_x3k: P must be the map's (clamped) P; plane strides % 8; an output"
    a_args = "gemm_x3a: an fp32 A, K % 32, plane strides % 8 and an output are required"
    cases = {"N not a multiple of BN": (lambda: persistent(N=96), "gemm_x3: N must be a multiple of the tile width 64"),
             "K % 64 on a 64-deep config": (lambda: persistent(Kd=96, cfg=5),
                                            "gemm_x3s: K must be a multiple of the stage depth 64"),
             "K % 32": (lambda: persistent(Kd=48), s_args),
             "bias missing": (lambda: persistent(epi=1), "gemm_x3s: epilogue operand missing"),
             "residual missing": (lambda: persistent(epi=1 | 4, bias=p), "gemm_x3s: epilogue operand missing"),
             "residual2 without rows": (lambda: persistent(epi=8, R2=p, r2_rows=0), "gemm_x3s: epilogue operand missing"),
             "no output": (lambda: persistent(C=None, Cp=None), s_args),
             "unknown config": (lambda: persistent(cfg=11), "gemm_x3s: unknown config"),
             "negative config": (lambda: persistent(cfg=-1), "gemm_x3s: unknown config"),
             "persistent: weight plane stride % 8": (lambda: persistent(wp=4), s_args),
             "persistent: K % 32 wins over a missing operand": (lambda: persistent(Kd=48, epi=1), s_args),
             "persistent: a missing operand wins over an unknown config":
                 (lambda: persistent(epi=4, cfg=11), "gemm_x3s: epilogue operand missing"),
             "persistent: an unknown config wins over N": (lambda: persistent(N=96, cfg=11), "gemm_x3s: unknown config"),
             "persistent: N wins over K % 64": (lambda: persistent(N=96, Kd=96, cfg=5), "tile width 64"),
             "group 0": (lambda: lib.nos_gemm_x3_set_group(0), "group must be 1..255"),
             "group 256": (lambda: lib.nos_gemm_x3_set_group(256), "group must be 1..255"),
             # nos_gemm_x3
             "x3: K % 32": (lambda: x3(Kd=48), x3_k32),
             "x3: activation plane stride % 8": (lambda: x3(ap=4), x3_k32),
             "x3: weight plane stride % 8": (lambda: x3(wp=12), x3_k32),
             "x3: output plane stride % 8": (lambda: x3(Cp=p, cp=2), x3_k32),
             "x3: no output": (lambda: x3(C=None), "gemm_x3: no output"),
             "x3: bias missing": (lambda: x3(epi=1), "gemm_x3: epilogue operand missing"),
             "x3: residual missing": (lambda: x3(epi=1 | 4, bias=p), "gemm_x3: epilogue operand missing"),
             "x3: residual2 missing": (lambda: x3(epi=8, r2_rows=3), "gemm_x3: epilogue operand missing"),
             "x3: residual2 without rows": (lambda: x3(epi=8, R2=p), "gemm_x3: epilogue operand missing"),
             "x3: unknown config": (lambda: x3(cfg=39), "gemm_x3: unknown tile config"),
             "x3: negative config": (lambda: x3(cfg=-1), "gemm_x3: unknown tile config"),
             "x3: a persistent id is no config here": (lambda: x3(cfg=100), "gemm_x3: unknown tile config"),
             "x3: N on a register-staged tile": (lambda: x3(N=96, cfg=0),
                                                 "gemm_x3: N must be a multiple of the tile width 64"),
             "x3: N on an LDS-DMA tile": (lambda: x3(N=128, cfg=32),
                                          "gemm_x3: N must be a multiple of the tile width 192"),
             "x3: K % 64 on a 64-deep tile": (lambda: x3(Kd=96, cfg=18),
                                              "gemm_x3: K must be a multiple of the stage depth 64"),
             "x3: N on the staggered tile": (lambda: x3(N=64, cfg=38), "gemm_x3t: N % 128 and K % 32 must be 0"),
             "x3: K % 32 wins over no output": (lambda: x3(Kd=48, C=None), x3_k32),
             "x3: no output wins over a missing operand": (lambda: x3(C=None, epi=1), "gemm_x3: no output"),
             "x3: a missing operand wins over an unknown config":
                 (lambda: x3(epi=4, cfg=39), "gemm_x3: epilogue operand missing"),
             "x3: an unknown config wins over N": (lambda: x3(N=96, cfg=39), "gemm_x3: unknown tile config"),
             "x3: N wins over K % 64": (lambda: x3(N=96, Kd=96, cfg=18), "tile width 64"),
             # nos_gemm_x3_partials
             "partials: K % 32": (lambda: partials(Kd=144), p_args),
             "partials: activation plane stride % 8": (lambda: partials(ap=4), p_args),
             "partials: weight plane stride % 8": (lambda: partials(wp=4), p_args),
             "partials: no output": (lambda: partials(C=None), p_args),
             "partials: a register-staged config": (lambda: partials(cfg=6), p_cfg),
             "partials: config past the table": (lambda: partials(cfg=39), p_cfg),
             "partials: one split": (lambda: partials(splits=1), p_cfg),
             "partials: nine splits": (lambda: partials(Kd=512, splits=9), p_cfg),
             "partials: more splits than stages": (lambda: partials(Kd=64, splits=3), p_cfg),
             "partials: N": (lambda: partials(N=96), "gemm_x3: N must be a multiple of the tile width 64"),
             "partials: K % 64 on a 64-deep tile": (lambda: partials(Kd=96, cfg=18),
                                                    "gemm_x3: K must be a multiple of the stage depth 64"),
             "partials: N on the staggered tile": (lambda: partials(N=64, cfg=38),
                                                   "gemm_x3t: N % 128 and K % 32 must be 0"),
             "partials: K % 32 wins over the config": (lambda: partials(Kd=144, cfg=3), p_args),
             "partials: the config wins over N": (lambda: partials(N=96, cfg=3), p_cfg),
             "partials: N wins over K % 64": (lambda: partials(N=96, Kd=96, cfg=18), "tile width 64"),
             # nos_gemm_x3_streamk_map and nos_gemm_x3_streamk through it
             "stream-K map: config 6": (lambda: sk_map(cfg=6), k_cfg),
             "stream-K map: negative config": (lambda: sk_map(cfg=-1), k_cfg),
             "stream-K map: M = 0": (lambda: sk_map(M=0), k_cfg),
             "stream-K map: P = 0": (lambda: sk_map(P=0), k_cfg),
             "stream-K map: N": (lambda: sk_map(N=96), "gemm_x3k: N % 64 and K % 32 must be 0"),
             "stream-K map: K % 64 on a 64-deep config": (lambda: sk_map(Kd=96, cfg=1),
                                                          "gemm_x3k: N % 64 and K % 64 must be 0"),
             "stream-K map: N on the 128-wide configs": (lambda: sk_map(N=64, cfg=2),
                                                         "gemm_x3k: N % 128 and K % 64 must be 0"),
             "stream-K map: too many units": (lambda: sk_map(M=1 << 25, N=64, Kd=32), "gemm_x3k: too many units"),
             "stream-K map: the config wins over N": (lambda: sk_map(N=96, cfg=6), k_cfg),
             "stream-K map: N wins over the unit count": (lambda: sk_map(M=1 << 25, N=96, Kd=32), "must be 0"),
             "stream-K: config 6": (lambda: streamk(cfg=6), k_cfg),
             "stream-K: N": (lambda: streamk(N=96), "gemm_x3k: N % 64 and K % 32 must be 0"),
             "stream-K: too many units": (lambda: streamk(M=1 << 25, N=64, Kd=32), "gemm_x3k: too many units"),
             "stream-K: P above the unit count": (lambda: streamk(P=5), k_p),  # 2 tiles x 2 stages
             "stream-K: activation plane stride % 8": (lambda: streamk(ap=4), k_p),
             "stream-K: weight plane stride % 8": (lambda: streamk(wp=4), k_p),
             "stream-K: no output": (lambda: streamk(C=None), k_p),
             "stream-K: the map's refusal wins over the strides": (lambda: streamk(N=96, ap=4, C=None),
                                                                   "gemm_x3k: N % 64 and K % 32 must be 0"),
             # nos_gemm_x3_f32a
             "fp32 A: no A": (lambda: f32a(A=None), a_args),
             "fp32 A: K % 32": (lambda: f32a(Kd=48), a_args),
             "fp32 A: weight plane stride % 8": (lambda: f32a(wp=4), a_args),
             "fp32 A: output plane stride % 8": (lambda: f32a(Cp=p, cp=4), a_args),
             "fp32 A: no output": (lambda: f32a(C=None), a_args),
             "fp32 A: bias missing": (lambda: f32a(epi=1), "gemm_x3a: epilogue operand missing"),
             "fp32 A: residual missing": (lambda: f32a(epi=1 | 4, bias=p), "gemm_x3a: epilogue operand missing"),
             "fp32 A: residual2 without rows": (lambda: f32a(epi=8, R2=p), "gemm_x3a: epilogue operand missing"),
             "fp32 A: unknown config": (lambda: f32a(cfg=2), "gemm_x3a: unknown config"),
             "fp32 A: negative config": (lambda: f32a(cfg=-1), "gemm_x3a: unknown config"),
             "fp32 A: N": (lambda: f32a(N=64), "gemm_x3a: N % 128 and K % 32 must be 0"),
             "fp32 A: no A wins over a missing operand": (lambda: f32a(A=None, epi=1), a_args),
             "fp32 A: a missing operand wins over an unknown config":
                 (lambda: f32a(epi=4, cfg=2), "gemm_x3a: epilogue operand missing"),
             "fp32 A: an unknown config wins over N": (lambda: f32a(N=64, cfg=2), "gemm_x3a: unknown config")}
    for name, (call, why) in cases.items():
        assert lib.nos_gemm_x3_set_group(1) == 0
        rc = call()
        err = lib.nos_gemm_x3_last_error().decode()
        assert rc != 0 and err and why in err, (name, rc, err)
    for g in (1, 255, int(os.environ.get("NOS_X3_GROUP_M", "1"))):  # the ends of the range; then the process's own
        assert lib.nos_gemm_x3_set_group(g) == 0, g
