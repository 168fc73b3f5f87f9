"""Bilinear chroma upsampling with siting (``ops.image.chroma_upsample`` and ``chroma="bilinear"`` on every
conversion and frame), on the CPU. The definition is in integers — two taps per subsampled axis, weights in quarters,
``(sum + 8) >> 4`` — and is held against two yardsticks that share no code with it: ``F.interpolate``'s bilinear at
scale 2 (which is the ``center`` siting) and a float64 interpolation at the luma sample's position on the chroma
grid, for all four sitings. Both are exact in float64 (the weights are multiples of 1/16 and the codes below 2^12),
so every comparison is ``torch.equal``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from walkai_nos_amd.models.workload import surfaces as S
from walkai_nos_amd.models.workload.processor import Nv12, Yuv420p
from walkai_nos_amd.ops import image as I

SIZES = ((1, 1), (2, 2), (3, 5), (37, 53))
#: (hs, vs) of 4:2:0 and 4:2:2
GEOMETRIES = {"420": (1, 1), "422": (1, 0)}
#: siting -> (horizontally co-sited, vertically co-sited), written out here on purpose
COSITED = {"left": (True, False), "center": (False, False), "topleft": (True, True), "top": (False, True)}


def codes(depth, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1 << depth, shape, generator=g, dtype=torch.int32)


def chroma_shape(h, w, hs, vs):
    return (h + (1 << vs) - 1) >> vs, (w + (1 << hs) - 1) >> hs


def by_position(c, h, w, hs, vs, siting):
    """Round-half-up of the float64 interpolation: luma ``x`` lies at chroma coordinate ``x / 2`` (co-sited) or
    ``(x - 0.5) / 2`` (centred), clamped to the plane, between the clamped neighbours."""
    c = c.double()

    def axis(n, nc, sub, cosited):
        x = torch.arange(n, dtype=torch.float64)
        pos = x if not sub else ((x - (0.0 if cosited else 0.5)) / 2.0).clamp(0.0, nc - 1.0)
        i0 = pos.floor().long()
        return i0, (i0 + 1).clamp(max=nc - 1), pos - i0
    hc, vc = COSITED[siting]
    y0, y1, fy = axis(h, c.shape[1], vs, vc)
    x0, x1, fx = axis(w, c.shape[2], hs, hc)
    rows = c[:, y0] * (1.0 - fy)[None, :, None] + c[:, y1] * fy[None, :, None]
    both = rows[:, :, x0] * (1.0 - fx) + rows[:, :, x1] * fx
    return (both + 0.5).floor().to(torch.int32)


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "{}x{}".format(*s))
@pytest.mark.parametrize("sub", sorted(GEOMETRIES))
@pytest.mark.parametrize("depth", (8, 12))
def test_upsample_against_the_position_formula_and_interpolate(depth, sub, hw):
    h, w = hw
    hs, vs = GEOMETRIES[sub]
    ch, cw = chroma_shape(h, w, hs, vs)
    c = codes(depth, (2, ch, cw), 100 * depth + h)
    seen = []
    for siting in I.SITINGS:
        got = I.chroma_upsample(c, h, w, hs, vs, siting)
        assert got.dtype == torch.int32 and tuple(got.shape) == (2, h, w)
        assert int(got.min()) >= int(c.min()) and int(got.max()) <= int(c.max())      # a code of the same depth
        assert torch.equal(got, by_position(c, h, w, hs, vs, siting)), siting
        seen.append(got)
    if min(hw) >= 3:
        nearest = c[:, torch.arange(h) >> vs][:, :, torch.arange(w) >> hs]
        # (co-sited 4:2:2 keeps the even columns: the two odd columns of five are what is left to differ)
        assert all((s != nearest).float().mean() > 0.3 for s in seen)
        # the sitings differ: all four on 4:2:0, the horizontal pair on 4:2:2
        assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2]) == (vs == 0)
    # "center" is torch's bilinear at scale 2 (half-pixel centres), rounded half up; on 4:2:2 along the rows only
    centre = I.chroma_upsample(c, h, w, hs, vs, "center")
    if vs:
        want = F.interpolate(c.double()[:, None], scale_factor=2, mode="bilinear", align_corners=False)[:, 0]
    else:
        want = F.interpolate(c.double().reshape(1, 2 * ch, cw), scale_factor=2, mode="linear",
                             align_corners=False).reshape(2, ch, 2 * cw)
    assert torch.equal(centre, (want + 0.5).floor().to(torch.int32)[:, :h, :w])


def test_a_constant_plane_stays_constant_and_a_ramp_is_linear():
    for sub, (hs, vs) in GEOMETRIES.items():
        for siting in I.SITINGS:
            c = torch.full((1,) + chroma_shape(9, 11, hs, vs), 777, dtype=torch.int32)
            want = torch.full((1, 9, 11), 777, dtype=torch.int32)
            assert torch.equal(I.chroma_upsample(c, 9, 11, hs, vs, siting), want)
    # C[i] = 4 i along a row: 2 x where chroma is co-sited with the even columns, 2 x - 1 where it is centred
    w, cw = 40, 20
    ramp = (4 * torch.arange(cw, dtype=torch.int32)).expand(1, 6, cw).contiguous()
    x = torch.arange(w, dtype=torch.int32)
    for siting, (hc, _) in COSITED.items():
        got = I.chroma_upsample(ramp, 6, w, 1, 0, siting)
        assert torch.equal(got[0, :, 1:-1], (2 * x - (0 if hc else 1))[1:-1].expand(6, -1)), siting
        # the edges clamp: the first column is C[0], the last C[cw - 1]
        assert got[0, 0, 0] == 0 and got[0, 0, -1] == 4 * (cw - 1)
    # the same down a column of 4:2:0
    col = (4 * torch.arange(cw, dtype=torch.int32))[None, :, None].expand(1, cw, 3).contiguous()
    for siting, (_, vc) in COSITED.items():
        got = I.chroma_upsample(col, w, 6, 1, 1, siting)
        assert torch.equal(got[0, 1:-1, 2], (2 * x - (0 if vc else 1))[1:-1]), siting


def typed(c, depth):
    return c.to(torch.uint8) if depth == 8 else c.to(torch.int16)


def words(c, depth, msb, seed):
    """int32 codes as 16-bit words with random ignored bits (``torch.int16``)."""
    junk = codes(16 - depth, c.shape, seed)
    w = (c << (16 - depth)) | junk if msb else c | (junk << depth)
    return w.to(torch.int16)        # (wraps: the same 16 bits)


def test_444_bilinear_is_nearest():
    y, u, v = (typed(codes(8, (1, 5, 7), s), 8) for s in (1, 2, 3))
    want = I.yuv_to_rgb(y, u, v, "444")
    for siting in I.SITINGS:
        assert torch.equal(I.yuv_to_rgb(y, u, v, "444", chroma="bilinear", siting=siting), want)
        assert torch.equal(S.YuvPlanar(y, u, v, "444", chroma="bilinear", siting=siting).rgb(), want)
    src = I.yuv_src(I.YUV_PLANAR, (y, u, v), "444", 8, False, 0, I.yuv_table(), "bilinear", "topleft")
    assert (src.chroma, src.siting) == (0, 0)           # the nearest instantiation is launched


def upsampled_444(y, u, v, sub, depth, msb, siting, **kw):
    """``yuv_to_rgb`` fed the upsampled planes as 4:4:4: the yardstick of every ``chroma="bilinear"`` conversion."""
    hs, vs = I.YUV_SUBSAMPLING[sub]
    h, w = y.shape[-2:]
    up = [typed(I.chroma_upsample(I.yuv_codes(t, depth, msb), h, w, hs, vs, siting), depth) for t in (u, v)]
    return I.yuv_to_rgb(typed(I.yuv_codes(y, depth, msb), depth), up[0], up[1], "444", depth, False, **kw)


@pytest.mark.parametrize("siting", sorted(COSITED))
def test_every_conversion_equals_yuv_to_rgb_of_the_upsampled_planes(siting):
    h, w = 6, 9
    kw = dict(chroma="bilinear", siting=siting)
    for sub, depth, msb in (("420", 8, False), ("422", 8, False), ("420", 10, True), ("422", 12, False)):
        hs, vs = I.YUV_SUBSAMPLING[sub]
        cs = (2,) + chroma_shape(h, w, hs, vs)
        yc, uc, vc = codes(depth, (2, h, w), 5), codes(depth, cs, 6), codes(depth, cs, 7)
        y, u, v = ((typed(t, 8) if depth == 8 else words(t, depth, msb, 8 + i)) for i, t in enumerate((yc, uc, vc)))
        for matrix, full in (("bt601", False), ("bt709", True)):
            want = upsampled_444(y, u, v, sub, depth, msb, siting, matrix=matrix, full_range=full)
            assert not torch.equal(want, I.yuv_to_rgb(y, u, v, sub, depth, msb, matrix, full))
            assert torch.equal(I.yuv_to_rgb(y, u, v, sub, depth, msb, matrix, full, **kw), want)
            uv, vu = torch.stack((u, v), dim=-1), torch.stack((v, u), dim=-1)
            assert torch.equal(I.yuv_semiplanar_to_rgb(y, uv, sub, depth, msb, matrix, full, **kw), want)
            assert torch.equal(I.yuv_semiplanar_to_rgb(y, vu, sub, depth, msb, matrix, full, True, **kw), want)
            if (sub, depth) == ("420", 8):
                assert torch.equal(I.yuv420_to_rgb(y, u, v, matrix, full, **kw), want)
                assert torch.equal(I.nv12_to_rgb(y, uv, matrix, full, **kw), want)
                assert torch.equal(I.nv12_to_rgb(y, vu, matrix, full, True, **kw), want)
            if (sub, depth) == ("422", 8):
                for order, (yo, uo, vo) in I.YUYV_ORDERS.items():
                    data = torch.zeros(2, h, 4 * cs[2], dtype=torch.uint8)
                    data[..., yo::2][..., :w] = y
                    data[..., uo::4], data[..., vo::4] = u, v
                    assert torch.equal(I.yuyv_to_rgb(data, w, order, matrix, full, **kw), want), order


def nearest_444(y, u, v, hs, vs):
    """Today's conversion, spelled out: every chroma sample repeated over its luma block, then 4:4:4."""
    h, w = y.shape[-2:]
    rep = [t.repeat_interleave(1 << vs, dim=-2).repeat_interleave(1 << hs, dim=-1)[..., :h, :w] for t in (u, v)]
    return I.yuv_to_rgb(y, rep[0], rep[1], "444")


def test_frames_carry_chroma_and_siting_and_the_defaults_are_todays():
    h, w = 6, 10
    y = typed(codes(8, (1, h, w), 11), 8)
    u, v = (typed(codes(8, (1, h // 2, w // 2), s), 8) for s in (12, 13))
    u2, v2 = (typed(codes(8, (1, h, w // 2), s), 8) for s in (14, 15))
    uv, uv2 = torch.stack((u, v), dim=-1), torch.stack((u2, v2), dim=-1)
    yuyv = torch.stack((y[..., 0::2], u2, y[..., 1::2], v2), dim=-1).flatten(2)
    p10 = [words(typed(t, 8).to(torch.int32) * 4, 10, True, 16 + i).view(torch.uint16) for i, t in enumerate((y, uv))]
    n420, n422 = nearest_444(y, u, v, 1, 1), nearest_444(y, u2, v2, 1, 0)
    #: (frame constructor taking the chroma keywords, the nearest RGB, the 4:4:4 yardstick's planes)
    cases = {
        "Nv12": (lambda **kw: Nv12(y, uv, **kw), n420, (y, u, v, "420", 8, False)),
        "Yuv420p": (lambda **kw: Yuv420p(y, u, v, **kw), n420, (y, u, v, "420", 8, False)),
        "YuvPlanar": (lambda **kw: S.YuvPlanar(y, u2, v2, "422", **kw), n422, (y, u2, v2, "422", 8, False)),
        "YuvSemiPlanar": (lambda **kw: S.YuvSemiPlanar(y, uv2, "422", **kw), n422, (y, u2, v2, "422", 8, False)),
        "Yuyv": (lambda **kw: S.Yuyv(yuyv, w, **kw), n422, (y, u2, v2, "422", 8, False)),
        "P010": (lambda **kw: S.YuvSemiPlanar(p10[0], p10[1], "420", 10, True, **kw), None,
                 (p10[0], p10[1][..., 0], p10[1][..., 1], "420", 10, True)),
    }
    for name, (make, nearest, planes) in cases.items():
        default = make()
        assert (default.chroma, default.siting) == ("nearest", "left")
        if nearest is not None:
            assert torch.equal(default.rgb(), nearest), name
        assert torch.equal(make(chroma="nearest", siting="center").rgb(), default.rgb())     # siting: bilinear's only
        for siting in I.SITINGS:
            f = make(chroma="bilinear", siting=siting)
            assert (f.chroma, f.siting) == ("bilinear", siting)
            assert torch.equal(f.rgb(), upsampled_444(*planes, siting)), (name, siting)
            assert not torch.equal(f.rgb(), default.rgb())
            assert f.to("cpu") is f and tuple(f.shape) == (1, h, w, 3)
        assert torch.equal(make(chroma="bilinear").rgb(), make(chroma="bilinear", siting="left").rgb())
    # the single-buffer constructors
    buf = torch.cat((y.flatten(), uv.flatten()))
    kw = dict(chroma="bilinear", siting="top")
    want = upsampled_444(y, u, v, "420", 8, False, "top")
    for f in (Nv12.from_buffer(buf, h, w, **kw), Yuv420p.from_buffer(torch.cat((y.flatten(), u.flatten(), v.flatten())),
                                                                      h, w, **kw)):
        assert (f.chroma, f.siting) == ("bilinear", "top") and torch.equal(f.rgb(), want)
    assert torch.equal(Nv12.from_buffer(buf, h, w).rgb(), n420)
    want = upsampled_444(y, u2, v2, "422", 8, False, "top")
    for name, data in (("yuy2", yuyv), ("nv16", torch.cat((y.flatten(), uv2.flatten()))),
                       ("i422", torch.cat((y.flatten(), u2.flatten(), v2.flatten())))):
        f = S.from_buffer(name, data.flatten().numpy() if name == "i422" else data.flatten(), h, w, **kw)
        assert (f.chroma, f.siting) == ("bilinear", "top") and torch.equal(f.rgb(), want), name
        assert torch.equal(S.from_buffer(name, data.flatten(), h, w).rgb(), n422), name


def test_unknown_names_raise():
    y = torch.zeros(1, 4, 4, dtype=torch.uint8)
    u = v = torch.zeros(1, 2, 2, dtype=torch.uint8)
    uv = torch.zeros(1, 2, 2, 2, dtype=torch.uint8)
    assert I.CHROMA == ("nearest", "bilinear") and set(I.SITINGS) == set(COSITED)
    # bit 0: horizontally co-sited, bit 1: vertically
    assert {k: (bool(b & 1), bool(b & 2)) for k, b in I.SITINGS.items()} == COSITED
    for bad in (dict(chroma="bicubic"), dict(chroma="bilinear", siting="bottom"), dict(siting="bottomleft"),
                dict(chroma=None), dict(siting=0)):
        for call in (lambda: I.yuv_to_rgb(y, u, v, **bad), lambda: I.yuv420_to_rgb(y, u, v, **bad),
                     lambda: I.nv12_to_rgb(y, uv, **bad), lambda: I.yuv_semiplanar_to_rgb(y, uv, **bad),
                     lambda: I.yuyv_to_rgb(torch.zeros(1, 4, 8, dtype=torch.uint8), 4, **bad),
                     lambda: I.yuv_planar_patch_planes(y, u, v, (16, 16), 16, (0.5,) * 3, (0.2,) * 3, **bad),
                     lambda: I.yuv_src(I.YUV_PLANAR, (y, u, v), "420", 8, False, 0, I.yuv_table(), **bad),
                     lambda: Nv12(y, uv, **bad), lambda: Yuv420p(y, u, v, **bad), lambda: S.YuvPlanar(y, u, v, **bad),
                     lambda: S.YuvSemiPlanar(y, uv, **bad),
                     lambda: S.Yuyv(torch.zeros(4, 8, dtype=torch.uint8), 4, **bad),
                     lambda: S.from_buffer("yuy2", torch.zeros(32, dtype=torch.uint8), 4, 4, **bad)):
            with pytest.raises(ValueError, match="chroma|siting"):
                call()
    with pytest.raises(ValueError, match="siting"):
        I.chroma_upsample(torch.zeros(1, 2, 2, dtype=torch.int32), 4, 4, 1, 1, "bottom")
    with pytest.raises(ValueError, match="chroma"):
        I.chroma_upsample(torch.zeros(1, 2, 3, dtype=torch.int32), 4, 4, 1, 1)


def test_the_descriptor_ends_with_chroma_and_siting():
    y = torch.zeros(1, 4, 4, dtype=torch.uint8)
    u = v = torch.zeros(1, 2, 2, dtype=torch.uint8)
    names = [f[0] for f in I.NosYuvSrc._fields_]
    assert names[-2:] == ["chroma", "siting"] and names[-3] == "tab"
    # the call the older tests make: seven positional arguments, today's behaviour
    src = I.yuv_src(I.YUV_PLANAR, (y, u, v), "420", 8, False, 0, I.yuv_table())
    assert (src.chroma, src.siting, src.size) == (0, 0, np.dtype(np.int32).itemsize * 22 + 3 * 40)
    for siting, (hc, vc) in COSITED.items():
        src = I.yuv_src(I.YUV_PLANAR, (y, u, v), "420", 8, False, 0, I.yuv_table(), "bilinear", siting)
        assert (src.chroma, src.siting) == (1, int(hc) + 2 * int(vc))
