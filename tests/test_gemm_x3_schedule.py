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


def test_bad_arguments_are_refused_before_any_launch(lib):
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.nos_gemm_x3_persistent.argtypes = [vp, sz, vp, sz, vp, vp, vp, i32, vp, vp, sz, i32, i32, i32, i32, i32, i32, vp]
    lib.nos_gemm_x3_set_group.argtypes = [i32]
    lib.nos_gemm_x3_last_error.restype = ctypes.c_char_p
    host = (ctypes.c_float * 64)()
    p = ctypes.addressof(host)  # never dereferenced: every case below returns before a launch

    def persistent(N=128, Kd=64, epi=0, cfg=0, bias=None, R=None, R2=None, r2_rows=0, C=p, Cp=None):
        # M = 0: were a case ever let through, its one workgroup would find no tile and touch nothing
        return lib.nos_gemm_x3_persistent(p, 0, p, N * Kd, bias, R, R2, r2_rows, C, Cp, 0, 0, N, Kd, epi, cfg, 4, None)

    cases = {"N not a multiple of BN": (lambda: persistent(N=96), "tile width"),
             "K % 64 on a 64-deep config": (lambda: persistent(Kd=96, cfg=5), "stage depth 64"),
             "K % 32": (lambda: persistent(Kd=48), "K % 32"),
             "bias missing": (lambda: persistent(epi=1), "operand missing"),
             "residual missing": (lambda: persistent(epi=1 | 4, bias=p), "operand missing"),
             "residual2 without rows": (lambda: persistent(epi=8, R2=p, r2_rows=0), "operand missing"),
             "no output": (lambda: persistent(C=None, Cp=None), "an output"),
             "unknown config": (lambda: persistent(cfg=11), "unknown config"),
             "negative config": (lambda: persistent(cfg=-1), "unknown config"),
             "group 0": (lambda: lib.nos_gemm_x3_set_group(0), "group must be 1..255"),
             "group 256": (lambda: lib.nos_gemm_x3_set_group(256), "group must be 1..255")}
    for name, (call, why) in cases.items():
        assert lib.nos_gemm_x3_set_group(1) == 0
        rc = call()
        err = lib.nos_gemm_x3_last_error().decode()
        assert rc != 0 and err and why in err, (name, rc, err)
    for g in (1, 255, int(os.environ.get("NOS_X3_GROUP_M", "1"))):  # the ends of the range; then the process's own
        assert lib.nos_gemm_x3_set_group(g) == 0, g
