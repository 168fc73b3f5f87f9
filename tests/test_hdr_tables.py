"""PQ and HLG frames tone-mapped to SDR, on the CPU: the tables (``ops.image.hdr_tables``) against the standards'
formulas written out again here in fp64, the integer definition (``ops.image.hdr_to_sdr`` behind ``yuv_to_rgb(...,
transfer=...)``, which is both what the kernel is tested against and the fallback) against a real-valued pipeline of
the same stages, the keyword on every entry point and frame class, and the launch descriptor against the header.

The integer pipeline against the real one: ``lut1`` rounds by at most 0.5 table steps (1 / 16383 of SDR white), the
gamut row with the largest absolute sum (6801 + 2407 + 298 = 9506, 2.32 x 4096) amplifies that to 1.16, and the shift
adds 0.5: under 1.7 table steps in front of ``lut2``. The sRGB curve is steepest in its linear part, 12.92 x 255 / 16383
= 0.2 bytes per table step, and ``lut2`` rounds by 0.5: under 0.84 bytes, plus what rounding the nine gamut
coefficients to 2^-12 moves (the real pipeline here keeps them in fp64). The bound asserted is one uint8 step; 200 000
random code triples per (transfer, depth, matrix) gave 0.57 to 0.89."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from walkai_nos_amd.models.workload import surfaces as S
from walkai_nos_amd.models.workload.processor import IMAGENET_MEAN, IMAGENET_STD, Nv12, Yuv420p
from walkai_nos_amd.ops import image as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = ("pq", "hlg")
DEPTHS = (10, 12)
MATRICES = ("bt601", "bt709", "bt2020")
BT2020_TO_709 = [[6801, -2407, -298], [-510, 4640, -34], [-74, -412, 4582]]


# ---- the standards, written out independently of ops.image ----------------------------------------
def pq_eotf(e):
    """SMPTE ST 2084: nits of the non-linear signal."""
    m1, m2 = 2610 / 16384, 2523 / 4096 * 128
    c1, c2, c3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
    p = np.asarray(e, dtype=np.float64) ** (1 / m2)
    return 10000 * (np.maximum(p - c1, 0) / (c2 - c3 * p)) ** (1 / m1)


def hlg_inverse_oetf(e):
    """BT.2100: scene light 0..1 of the non-linear signal."""
    a = 0.17883277
    b, c = 1 - 4 * a, 0.5 - a * np.log(4 * a)
    e = np.asarray(e, dtype=np.float64)
    return np.where(e <= 0.5, e * e / 3, (np.exp((e - c) / a) + b) / 12)


def nits(transfer, e):
    return pq_eotf(e) if transfer == "pq" else 1000 * hlg_inverse_oetf(e) ** 1.2


def reinhard(n, peak=1000.0):
    x, p = np.asarray(n, dtype=np.float64) / 203, peak / 203
    return np.clip(x * (1 + x / (p * p)) / (1 + x), 0, 1)


def srgb_oetf(lin):
    lin = np.asarray(lin, dtype=np.float64)
    return np.where(lin < 0.0031308, 12.92 * lin, 1.055 * np.maximum(lin, 1e-300) ** (1 / 2.4) - 0.055)


def to_xyz(primaries):
    m = np.array([[x / y, 1, (1 - x - y) / y] for x, y in primaries], dtype=np.float64).T
    xw, yw = 0.3127, 0.3290
    return m * np.linalg.solve(m, np.array([xw / yw, 1, (1 - xw - yw) / yw]))


REAL_GAMUT = np.linalg.solve(to_xyz(((0.640, 0.330), (0.300, 0.600), (0.150, 0.060))),
                             to_xyz(((0.708, 0.292), (0.170, 0.797), (0.131, 0.046))))


def signal(depth):
    return np.minimum(np.arange(1 << depth, dtype=np.float64) / (255.0 * (1 << (depth - 8))), 1.0)


# ---- anchors --------------------------------------------------------------------------------------
def test_anchors_of_the_two_transfer_functions():
    assert pq_eotf(0.508078) == pytest.approx(100.0, rel=1e-4)
    assert pq_eotf(0.751827) == pytest.approx(1000.0, rel=1e-4)
    assert hlg_inverse_oetf(0.5) == pytest.approx(1 / 12, rel=1e-12)
    assert hlg_inverse_oetf(1.0) == pytest.approx(1.0, rel=1e-7)
    # and the package's own fp64 functions are those
    e = np.linspace(0, 1, 1001)
    assert np.allclose(I.hdr_nits("pq", e), pq_eotf(e), rtol=1e-12, atol=0)
    assert np.allclose(I.hdr_nits("hlg", e), nits("hlg", e), rtol=1e-12, atol=0)
    assert I.hdr_tone_map(1000.0) == pytest.approx(1.0) and I.hdr_tone_map(0.0) == 0.0
    assert I.hdr_tone_map(203.0) == pytest.approx(0.5 * (1 + (203 / 1000) ** 2))
    assert I.TRANSFERS == ("sdr", "pq", "hlg")


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("transfer", HDR)
def test_lut1_is_the_rounded_formula_at_every_index(transfer, depth):
    for peak in (1000.0, 4000.0):
        lut1 = I.hdr_tables(transfer, depth, "bt2020", peak)[0]
        want = np.rint(16383 * reinhard(nits(transfer, signal(depth)), peak))
        assert lut1.dtype == np.uint16 and lut1.shape == (1 << depth,)
        assert np.array_equal(lut1.astype(np.int64), want.astype(np.int64))
    assert not np.array_equal(I.hdr_tables(transfer, depth, "bt2020", 1000.0)[0],
                              I.hdr_tables(transfer, depth, "bt2020", 4000.0)[0])


# ---- table shape ----------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("transfer", HDR)
def test_table_shape(transfer, depth):
    for matrix in MATRICES:
        lut1, gamut, lut2 = I.hdr_tables(transfer, depth, matrix)
        assert lut1[0] == 0 and lut1[-1] == 16383 and (np.diff(lut1.astype(np.int64)) >= 0).all()
        assert lut2.dtype == np.uint8 and lut2.shape == (16384,)
        assert (np.diff(lut2.astype(np.int64)) >= 0).all() and len(np.unique(lut2)) == 256
        assert np.array_equal(lut2.astype(np.int64), np.rint(255 * srgb_oetf(np.arange(16384) / 16383)).astype(np.int64))
        assert gamut.shape == (3, 3) and gamut.sum(axis=1).tolist() == [4096] * 3
        assert gamut.tolist() == (BT2020_TO_709 if matrix == "bt2020" else (4096 * np.eye(3, dtype=int)).tolist())
        # what the kernel's arithmetic needs: 24-bit operands, sums inside int32 with room
        assert np.abs(gamut).max() < 1 << 15 and np.abs(gamut).sum(axis=1).max() * 16383 + 2048 < 1 << 29
    # the nine integers are the fp64 derivation from the primaries, rounded
    assert np.array_equal(np.rint(REAL_GAMUT * 4096).astype(int), np.array(BT2020_TO_709))


def test_tables_are_shared_and_read_only():
    a, b = I.hdr_tables("pq", 10, "bt2020"), I.hdr_tables("pq", 10, "bt2020", 1000)
    assert all(x is y for x, y in zip(a, b))
    with pytest.raises(ValueError):
        a[0][0] = 1


# ---- the definition -------------------------------------------------------------------------------
def frame_444(codes, depth, **kw):
    """int32 ``[n, 3]`` (Y, U, V) codes as a one-row 4:4:4 frame's conversion ``[n, 3]``."""
    y, u, v = (codes[:, k].reshape(1, 1, -1).to(torch.int16) for k in range(3))
    return I.yuv_to_rgb(y, u, v, "444", depth, False, **kw).reshape(-1, 3)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("transfer", HDR)
def test_grey_stays_grey(transfer, depth):
    luma = torch.arange(1 << depth, dtype=torch.int32)
    codes = torch.stack((luma, torch.full_like(luma, 1 << (depth - 1)), torch.full_like(luma, 1 << (depth - 1))), dim=1)
    for matrix in MATRICES:
        for full in (False, True):
            rgb = frame_444(codes, depth, matrix=matrix, full_range=full, transfer=transfer)
            assert torch.equal(rgb[:, 0], rgb[:, 1]) and torch.equal(rgb[:, 1], rgb[:, 2]), (matrix, full)
            assert rgb[0, 0] == 0 and rgb[-1, 0] == 255 and (rgb[1:, 0] >= rgb[:-1, 0]).all()


def step1_codes(codes, depth, matrix, full_range):
    """Step 1 in numpy int64: the R'G'B' codes at the source's depth."""
    t = I.yuv_table(matrix, full_range, depth)
    d = codes.numpy().astype(np.int64) - np.array(t[9:])
    s = d @ np.array(t[:9]).reshape(3, 3).T + (1 << 15)
    return np.clip(s, 0, (1 << (16 + depth)) - 1) >> 16


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("transfer", HDR)
def test_agreement_with_a_real_valued_pipeline(transfer, depth):
    g = torch.Generator().manual_seed(depth * 31 + len(transfer))
    for matrix in ("bt2020", "bt709"):
        # random code triples, straight into steps 2 to 4 ...
        k = torch.randint(0, 1 << depth, (200_000, 3), generator=g, dtype=torch.int32)
        got = I.hdr_to_sdr(k, I.hdr_tables(transfer, depth, matrix)).numpy().astype(np.float64)
        light = reinhard(nits(transfer, np.minimum(k.numpy() / (255.0 * (1 << (depth - 8))), 1.0)))
        gamut = REAL_GAMUT if matrix == "bt2020" else np.eye(3)
        want = 255 * srgb_oetf(np.clip(light @ gamut.T, 0, 1))
        err = np.abs(got - want).max()
        print(f"{transfer} depth {depth} {matrix}: largest difference {err:.4f} bytes")
        assert err <= 1.0
        # ... and random YUV samples through all four, fed E' from step 1's codes
        yuv = torch.randint(0, 1 << depth, (50_000, 3), generator=g, dtype=torch.int32)
        rgb = frame_444(yuv, depth, matrix=matrix, transfer=transfer).numpy().astype(np.float64)
        k1 = step1_codes(yuv, depth, matrix, False)
        assert k1.min() == 0 and k1.max() == (1 << depth) - 1
        light = reinhard(nits(transfer, np.minimum(k1 / (255.0 * (1 << (depth - 8))), 1.0)))
        assert np.abs(rgb - 255 * srgb_oetf(np.clip(light @ gamut.T, 0, 1))).max() <= 1.0


def test_hdr_to_sdr_is_the_three_integer_steps():
    lut1, gamut, lut2 = I.hdr_tables("pq", 10, "bt2020")
    k = torch.randint(0, 1024, (4, 5, 3), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    light = lut1.astype(np.int64)[k.numpy()]
    s = np.clip((light @ gamut.astype(np.int64).T + 2048) >> 12, 0, 16383)
    got = I.hdr_to_sdr(k, (lut1, gamut, lut2))
    assert got.dtype == torch.uint8 and got.shape == k.shape and np.array_equal(got.numpy(), lut2[s])
    # tensors in place of the ndarrays, and the nine integers flat or by rows
    tens = (torch.from_numpy(lut1.astype(np.int16)), gamut.tolist(), torch.from_numpy(lut2.copy()))
    assert torch.equal(I.hdr_to_sdr(k, tens), got)
    assert torch.equal(I.hdr_to_sdr(k, I._hdr_device_tables("pq", 10, "bt2020", 1000.0, torch.device("cpu"))), got)
    for bad in (k.float(), k[..., :2], torch.tensor(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="hdr_to_sdr"):
            I.hdr_to_sdr(bad, (lut1, gamut, lut2))


# ---- defaults unchanged ---------------------------------------------------------------------------
def sdr_by_the_table(name, planes, h, w, matrix):
    """Today's conversion in numpy int64: nearest chroma, ``clip((sum + 2^(7+d)) >> (8+d), 0, 255)``."""
    _, sub, depth, _, _ = S.FORMATS[name]
    hs, vs = I.YUV_SUBSAMPLING[sub]
    t = I.yuv_table(matrix, False, depth)
    y, u, v = (p.numpy().astype(np.int64) for p in planes)
    rows, cols = np.arange(h) >> vs, np.arange(w) >> hs
    d = np.stack((y - t[9], u[rows][:, cols] - t[10], v[rows][:, cols] - t[11]), axis=-1)
    s = d @ np.array(t[:9]).reshape(3, 3).T + (1 << (7 + depth))
    return np.clip(s >> (8 + depth), 0, 255).astype(np.uint8)


def surface(name, h, w, seed=0):
    """A seeded picture of format ``name``: ``(codes y, u, v as int32 [rows, cols], the decoder's buffer)``."""
    kind, sub, depth, msb, swap = S.FORMATS[name]
    hs, vs = I.YUV_SUBSAMPLING[sub]
    g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w + depth)
    ch, cw = h >> vs, (w + (1 << hs) - 1) >> hs
    y, u, v = (torch.randint(0, 1 << depth, s, generator=g, dtype=torch.int32) for s in ((h, w), (ch, cw), (ch, cw)))
    if kind == "packed":
        yo, uo, vo = I.YUYV_ORDERS[{"yuy2": "yuyv"}.get(name, name)]
        data = torch.zeros(h, 4 * cw, dtype=torch.int32)
        data[:, yo::2][:, :w], data[:, uo::4], data[:, vo::4] = y, u, v
        return (y, u, v), data.to(torch.uint8).reshape(-1)

    def enc(t):
        if depth == 8:
            return t.to(torch.uint8).reshape(-1)
        word = t << (16 - depth) if msb else t
        return torch.stack((word & 255, word >> 8), dim=-1).to(torch.uint8).reshape(-1)
    first, second = (v, u) if swap else (u, v)
    chroma = [torch.stack((first, second), dim=-1)] if kind == "semiplanar" else [first, second]
    return (y, u, v), torch.cat([enc(y)] + [enc(c) for c in chroma])


@pytest.mark.parametrize("name", sorted(S.FORMATS))
def test_sdr_is_todays_conversion_and_the_transfers_are_not(name):
    h, w = 6, 9
    depth = S.FORMATS[name][2]
    codes, buf = surface(name, h, w)
    for matrix in ("bt709", "bt2020"):
        want = sdr_by_the_table(name, codes, h, w, matrix)
        plain = S.from_buffer(name, buf, h, w, matrix=matrix)
        said = S.from_buffer(name, buf, h, w, matrix=matrix, transfer="sdr", peak_nits=400.0)
        assert np.array_equal(plain.rgb()[0].numpy(), want) and np.array_equal(said.rgb()[0].numpy(), want)
        if depth == 8:
            continue
        assert (plain.transfer, plain.peak_nits) == ("sdr", 1000.0)
        pq = S.from_buffer(name, buf, h, w, matrix=matrix, transfer="pq").rgb()
        hlg = S.from_buffer(name, buf, h, w, matrix=matrix, transfer="hlg").rgb()
        dim = S.from_buffer(name, buf, h, w, matrix=matrix, transfer="pq", peak_nits=4000.0).rgb()
        assert pq.dtype == torch.uint8 and pq.shape == (1, h, w, 3)
        sdr = torch.from_numpy(want)[None]
        assert not torch.equal(pq, sdr) and not torch.equal(hlg, sdr) and not torch.equal(pq, hlg)
        assert not torch.equal(pq, dim)


def test_positional_calls_of_today_keep_working():
    y = torch.randint(0, 1024, (1, 4, 6), dtype=torch.int16)
    u = v = torch.randint(0, 1024, (1, 2, 3), dtype=torch.int16)
    uv = torch.stack((u, v), dim=-1)
    a = I.yuv_to_rgb(y, u, v, "420", 10, False, "bt2020", False, "bilinear", "topleft")
    assert torch.equal(a, I.yuv_to_rgb(y, u, v, "420", 10, False, "bt2020", False, "bilinear", "topleft", "sdr", 1000.0))
    assert torch.equal(a, I.yuv_semiplanar_to_rgb(y, uv, "420", 10, False, "bt2020", False, False, "bilinear", "topleft"))
    hdr = I.yuv_to_rgb(y, u, v, "420", 10, False, "bt2020", False, "bilinear", "topleft", "pq", 1000.0)
    assert torch.equal(hdr, I.yuv_semiplanar_to_rgb(y, uv, "420", 10, False, "bt2020", False, False, "bilinear",
                                                    "topleft", "pq", 1000.0))
    assert torch.equal(hdr, S.YuvPlanar(y, u, v, "420", 10, False, "bt2020", False, "bilinear", "topleft", "pq").rgb())
    f = S.YuvSemiPlanar(y, uv, "420", 10, False, "bt2020", False, False, "bilinear", "topleft", "pq", 1000.0)
    assert torch.equal(hdr, f.rgb()) and not torch.equal(hdr, a)
    # on the CPU the fused entry points are the RGB path on the definition
    for got in (f.patch_planes((16, 16), 16, IMAGENET_MEAN, IMAGENET_STD, True),
                I.yuv_planar_patch_planes(y, u, v, (16, 16), 16, IMAGENET_MEAN, IMAGENET_STD, "420", 10, False, "bt2020",
                                          False, True, "bilinear", "topleft", "pq", 1000.0)):
        want = I.image_patch_planes(hdr, (16, 16), 16, IMAGENET_MEAN, IMAGENET_STD, True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- errors ---------------------------------------------------------------------------------------
def entry_points(depth):
    """Every function and class that takes the keyword, as ``call(**kw)`` on a tiny frame of ``depth``."""
    dt = torch.uint8 if depth == 8 else torch.int16
    y, u, v = torch.zeros(1, 4, 4, dtype=dt), torch.zeros(1, 2, 2, dtype=dt), torch.zeros(1, 2, 2, dtype=dt)
    uv = torch.zeros(1, 2, 2, 2, dtype=dt)
    name, nbytes = ("nv16", 4 * 4 * 2) if depth == 8 else ("p010" if depth == 10 else "p012", 4 * 4 * 3)
    tail = ((16, 16), 16, IMAGENET_MEAN, IMAGENET_STD)
    return {
        "yuv_to_rgb": lambda **kw: I.yuv_to_rgb(y, u, v, "420", depth, **kw),
        "yuv_semiplanar_to_rgb": lambda **kw: I.yuv_semiplanar_to_rgb(y, uv, "420", depth, **kw),
        "yuv_planar_patch_planes": lambda **kw: I.yuv_planar_patch_planes(y, u, v, *tail, "420", depth, **kw),
        "yuv_semiplanar_patch_planes": lambda **kw: I.yuv_semiplanar_patch_planes(y, uv, *tail, "420", depth, **kw),
        "YuvPlanar": lambda **kw: S.YuvPlanar(y, u, v, "420", depth, **kw),
        "YuvSemiPlanar": lambda **kw: S.YuvSemiPlanar(y, uv, "420", depth, **kw),
        "from_buffer": lambda **kw: S.from_buffer(name, torch.zeros(nbytes, dtype=torch.uint8), 4, 4, **kw),
    }


@pytest.mark.parametrize("depth", (8, 10, 12))
def test_every_entry_point_refuses_by_the_arguments_name(depth):
    for who, call in entry_points(depth).items():
        call()
        call(transfer="sdr", peak_nits=203.5)
        with pytest.raises(ValueError, match="transfer 'srgb'"):
            call(transfer="srgb")
        for peak in (203.0, 100.0, 0.0, -1.0, float("nan")):
            for transfer in ("sdr", "pq"):
                with pytest.raises(ValueError, match="peak_nits"):
                    call(transfer=transfer, peak_nits=peak)
        for transfer in HDR:
            if depth == 8:
                with pytest.raises(ValueError, match="transfer .* depth 10 or 12"):
                    call(transfer=transfer)
            else:
                call(transfer=transfer)
                call(transfer=transfer, peak_nits=203.5)


def test_the_eight_bit_frame_classes_refuse_a_transfer():
    y, u, uv = (torch.zeros(s, dtype=torch.uint8) for s in ((4, 4), (2, 2), (2, 2, 2)))
    data = torch.zeros(4, 8, dtype=torch.uint8)
    for make in (lambda **kw: S.Yuyv(data, 4, **kw), lambda **kw: Nv12(y, uv, **kw), lambda **kw: Yuv420p(y, u, u, **kw),
                 lambda **kw: S.from_buffer("yuy2", data, 4, 4, **kw)):
        assert make().rgb().shape == (1, 4, 4, 3) and make(transfer="sdr").rgb().shape == (1, 4, 4, 3)
        for transfer in HDR:
            with pytest.raises(ValueError, match="transfer .* depth 10 or 12"):
                make(transfer=transfer)
        with pytest.raises(ValueError, match="transfer 'linear'"):
            make(transfer="linear")
    for bad in (("sdr", 10, "bt2020"), ("pq", 8, "bt2020"), ("pq", 10, "bt2020", 203.0), ("pq", 10, "bt470"),
                ("gamma", 10, "bt709")):
        with pytest.raises(ValueError):
            I.hdr_tables(*bad)


def test_the_pod_client_refuses_a_transfer_on_eight_bit_formats(capsys):
    from walkai_nos_amd.dataplane import client
    assert set(client.DEEP) == {n for n, f in S.FORMATS.items() if f[2] != 8}
    for fmt in ("rgb", "bgra", "nv12", "i420", "yuy2", "nv16", "i444"):
        for transfer in HDR:
            with pytest.raises(SystemExit) as e:
                client.main(["--end-to-end", "--pixel-format", fmt, "--transfer", transfer])
            assert e.value.code == 2 and "--transfer" in capsys.readouterr().err
    for peak in ("203", "100"):
        with pytest.raises(SystemExit) as e:
            client.main(["--end-to-end", "--pixel-format", "p010", "--transfer", "pq", "--peak-nits", peak])
        assert e.value.code == 2 and "--peak-nits" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        client.main(["--end-to-end", "--pixel-format", "p010", "--transfer", "linear"])


# ---- the device tables' cache ---------------------------------------------------------------------
def test_device_tables_are_cached_pinned_under_capture_and_dropped_by_invalidate_cache(monkeypatch):
    I.invalidate_cache()
    cpu = torch.device("cpu")
    a = I._hdr_device_tables("pq", 10, "bt2020", 1000.0, cpu)
    assert a is I._hdr_device_tables("pq", 10, "bt2020", 1000, cpu)
    lut1, gamut, lut2 = I.hdr_tables("pq", 10, "bt2020")
    assert a[0].dtype == torch.int16 and np.array_equal(a[0].numpy().view(np.uint16), lut1)
    assert a[1] == tuple(gamut.reshape(-1).tolist()) and np.array_equal(a[2].numpy(), lut2)
    hdr = I.yuv_hdr(*a)
    assert (hdr.size, hdr.entries, hdr.lut1, hdr.lut2) == (ctypes.sizeof(I.NosYuvHdr), 1024, a[0].data_ptr(),
                                                           a[2].data_ptr())
    assert list(hdr.gamut) == list(a[1])
    for other in (("hlg", 10, "bt2020", 1000.0), ("pq", 12, "bt2020", 1000.0), ("pq", 10, "bt709", 1000.0),
                  ("pq", 10, "bt2020", 600.0)):
        assert I._hdr_device_tables(*other, cpu) is not a
    key = ("pq", 10, "bt2020", 1000.0, "cpu")
    assert key in I._hdr_tables and not I._hdr_tables.pinned(key)
    # handed out while a graph is being captured: kept whatever comes after, until invalidate_cache
    from walkai_nos_amd.ops import graph_cache
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: True)
    assert I._hdr_device_tables(*key[:4], cpu) is a and I._hdr_tables.pinned(key)
    monkeypatch.setattr(graph_cache, "is_capturing", lambda: False)
    for peak in range(300, 300 + 2 * I._hdr_tables.bound):
        I._hdr_device_tables("hlg", 12, "bt709", float(peak), cpu)
    assert I._hdr_device_tables(*key[:4], cpu) is a and I._hdr_tables.unpinned() <= I._hdr_tables.bound
    I.invalidate_cache()
    assert len(I._hdr_tables) == 0 and I._hdr_device_tables(*key[:4], cpu) is not a
    I.invalidate_cache()


# ---- the descriptor -------------------------------------------------------------------------------
def test_the_descriptor_matches_the_header():
    text = open(os.path.join(ROOT, "csrc", "image_yuv.h")).read()
    body = re.search(r"typedef struct NosYuvHdr \{(.*?)\} NosYuvHdr;", text, re.S).group(1)
    fields = []
    for line in body.splitlines():
        decl = line.split("//")[0].strip().rstrip(";")
        if decl:
            m = re.fullmatch(r"(int|const void\*) (\w+)(?:\[(\d+)\])?", decl)
            assert m, decl
            fields.append((m.group(2), m.group(1), int(m.group(3) or 0)))
    assert [f[0] for f in fields] == ["size", "entries", "lut1", "lut2", "gamut"]
    ctype = {"int": ctypes.c_int, "const void*": ctypes.c_void_p}
    want = [(n, ctype[t] * k if k else ctype[t]) for n, t, k in fields]
    assert [(n, t) for n, t in I.NosYuvHdr._fields_] == want
    # two ints, two pointers, nine ints, padded to the pointers' alignment
    assert ctypes.sizeof(I.NosYuvHdr) == 64 and I.NosYuvHdr.lut1.offset == 8 and I.NosYuvHdr.gamut.offset == 24
    # and the source descriptor is what it was
    assert [f[0] for f in I.NosYuvSrc._fields_][-3:] == ["tab", "chroma", "siting"]
    assert ctypes.sizeof(I.NosYuvSrc) == 4 * 22 + 3 * 40
    assert "nos_image_patch_planes_yuv_hdr(const NosYuvSrc* src, const NosYuvHdr* hdr," in text
