"""4:2:2, 4:4:4, packed 4:2:2 and 10 / 12-bit surfaces on the CPU: the integer conversion at every depth
(``ops.image.yuv_to_rgb``, which is both the definition the kernel is tested against and the fallback) against the
real formula of the standards, its chroma geometry, the bits of a 16-bit word that do not count, the compositions
the ops are defined by, ``surfaces.from_buffer`` and the CPU path of the processor and the model.

The integer formula against fp64: a coefficient is ``rint(real * 2^(8 + depth))`` and a code is below ``2^depth``,
so the three products err by at most ``3 * 2^depth * 2^-(9 + depth) = 0.006`` together at every depth, and ``(sum +
2^(7 + depth)) >> (8 + depth)`` is ``floor(x + 0.5)`` of that sum. It can therefore differ from ``clip(rint(real))``
only where the real value is within 0.006 of a rounding tie, and then by 1.

The x4 law: in limited range the scale factors at depth ``d`` are those of depth 8 divided by ``k = 2^(d-8)`` and the
table is scaled by ``2^(8+d) = 2^16 k``, so the nine coefficients are the same integers; the offsets are ``k`` times
depth 8's. With codes ``k`` times an 8-bit frame's, the sum is ``k`` times depth 8's sum, the rounding constant
``2^(7+d) = k 2^15`` as well, and ``(k s + k 2^15) >> (16 + log2 k) == (s + 2^15) >> 16`` exactly."""
import itertools

import numpy as np
import pytest
import torch

from walkai_nos_amd.models.workload import processor as PR
from walkai_nos_amd.models.workload import surfaces as S
from walkai_nos_amd.models.workload.processor import IMAGENET_MEAN, IMAGENET_STD, Frame, Nv12, Packed, YolosProcessor, Yuv420p
from walkai_nos_amd.ops import image as I

KRKB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
TABLES = list(itertools.product((8, 10, 12), KRKB, (False, True)))
IDS = [f"{d}bit-{m}-{'full' if fr else 'limited'}" for d, m, fr in TABLES]
P = 16


def real_rgb(yv, u, v, matrix, full_range, depth=8):
    """The conversion as the standards state it for ``depth``-bit codes, in fp64 and independent of ``ops.image``:
    ``Y' = (Y - 16 k) / (219 k)`` and ``Pb, Pr = (U, V - 2^(depth-1)) / (224 k)`` with ``k = 2^(depth-8)`` (full
    range: ``Y / (2^depth - 1)`` and ``/ (2^depth - 1)``), ``R = Y' + 2 (1 - Kr) Pr``, ``B = Y' + 2 (1 - Kb) Pb``,
    ``G`` from ``Y' = Kr R + Kg G + Kb B``; times 255, unclipped."""
    kr, kb = KRKB[matrix]
    k, top, mid = float(1 << (depth - 8)), float((1 << depth) - 1), float(1 << (depth - 1))
    yv, u, v = (np.asarray(t, dtype=np.float64) for t in (yv, u, v))
    yp = yv / top if full_range else (yv - 16.0 * k) / (219.0 * k)
    pb, pr = ((u - mid) / top, (v - mid) / top) if full_range else ((u - mid) / (224.0 * k), (v - mid) / (224.0 * k))
    r, b = yp + 2.0 * (1.0 - kr) * pr, yp + 2.0 * (1.0 - kb) * pb
    g = (yp - kr * r - kb * b) / (1.0 - kr - kb)
    return 255.0 * r, 255.0 * g, 255.0 * b


def typed(codes, depth, dtype=torch.uint16):
    """int codes as a plane of ``depth``: uint8, or 16-bit words with the value in the low bits."""
    if depth == 8:
        return codes.to(torch.uint8)
    t = codes.to(torch.int16)
    return t if dtype == torch.int16 else t.view(torch.uint16)


def convert(triples, depth=8, matrix="bt601", full_range=False):
    t = torch.tensor(triples, dtype=torch.int32).reshape(-1, 3)
    y, u, v = (typed(t[:, k].reshape(-1, 1, 1), depth) for k in range(3))
    return I.yuv_to_rgb(y, u, v, "444", depth, False, matrix, full_range).reshape(-1, 3).tolist()


def planes(sub, depth, h, w, batch=None, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w + depth)
    hs, vs = I.YUV_SUBSAMPLING[sub]
    lead = () if batch is None else (batch,)
    shapes = ((h, w),) + (((h + (1 << vs) - 1) >> vs, (w + (1 << hs) - 1) >> hs),) * 2
    return tuple(torch.randint(0, 1 << depth, lead + s, generator=g, dtype=torch.int32) for s in shapes)


@pytest.mark.parametrize("depth,matrix,full_range", TABLES, ids=IDS)
def test_table_against_the_standard(depth, matrix, full_range):
    table = I.yuv_table(matrix, full_range, depth)
    m, off = I.yuv_real_matrix(matrix, full_range, depth)
    assert len(table) == 12 and all(isinstance(v, int) for v in table) and table[9:] == off
    assert off == (0 if full_range else 16 << (depth - 8), 1 << (depth - 1), 1 << (depth - 1))
    assert np.array_equal(np.array(table[:9]).reshape(3, 3), np.rint(m * 2.0 ** (8 + depth)))
    # what the kernel's arithmetic needs: 24-bit coefficients, sums inside int32 with room
    assert max(abs(v) for v in table[:9]) <= 140363
    top = (1 << depth) - 1
    reach = [max(table[9 + k], top - table[9 + k]) for k in range(3)]
    assert max(sum(abs(table[3 * c + k]) * reach[k] for k in range(3)) for c in range(3)) + (1 << (7 + depth)) < 5.81e8
    if depth == 8 and matrix != "bt2020":
        assert table == I.nv12_table(matrix, full_range)
    if not full_range:
        assert table[:9] == I.yuv_table(matrix, False, 8)[:9]
    kr, kb = KRKB[matrix]
    assert I.YUV_MATRICES[matrix] == (kr, kb)
    assert np.allclose(m[:, 0], m[0, 0]) and np.allclose(np.array([kr, 1 - kr - kb, kb]) @ m[:, 1:], 0.0, atol=1e-12)
    # the lattice: every Y code x 65 x 65 chroma codes (64 steps and the top code), as a 4:4:4 frame per luma value
    step = (1 << depth) // 64
    cc = np.concatenate((np.arange(0, 1 << depth, step), [top]))
    u, v = np.meshgrid(cc, cc, indexing="ij")
    up, vp = (typed(torch.from_numpy(t.astype(np.int32))[None], depth) for t in (u, v))
    worst, ties, total = 0, 0, 0
    chunk = 256
    for y0 in range(0, 1 << depth, chunk):
        yv = torch.arange(y0, y0 + chunk, dtype=torch.int32)
        yp = typed(yv.view(-1, 1, 1).expand(-1, 65, 65), depth)
        got = I.yuv_to_rgb(yp, up.expand(chunk, -1, -1), vp.expand(chunk, -1, -1), "444", depth, False, matrix,
                           full_range).numpy().astype(np.int64)
        for c, real in enumerate(real_rgb(yv.numpy()[:, None, None], u[None], v[None], matrix, full_range, depth)):
            diff = np.abs(got[..., c] - np.clip(np.rint(real), 0, 255).astype(np.int64))
            worst = max(worst, int(diff.max()))
            clear = np.abs(real - np.floor(real) - 0.5) > 0.01
            ties += int((~clear).sum())
            total += clear.size
            assert not diff[clear].any(), (y0, c)
    print(f"[yuv] {depth}-bit {matrix} {'full' if full_range else 'limited'}: worst |int - rint(real)| {worst} over "
          f"{total} values, {ties} ({100.0 * ties / total:.2f}%) within 0.01 of a tie")
    assert worst <= 1 and ties <= 0.05 * total


def test_anchor_values_at_depth_10():
    for matrix in KRKB:
        assert convert([(64, 512, 512), (940, 512, 512)], 10, matrix) == [[0, 0, 0], [255, 255, 255]]
        assert convert([(0, 512, 512), (1023, 512, 512)], 10, matrix, True) == [[0, 0, 0], [255, 255, 255]]
        # below black and above white clip in limited range
        assert convert([(0, 512, 512), (1023, 512, 512)], 10, matrix) == [[0, 0, 0], [255, 255, 255]]
        assert convert([(256, 2048, 2048), (3760, 2048, 2048)], 12, matrix) == [[0, 0, 0], [255, 255, 255]]
    # each channel clipping at 0 and at 255 while the luma is mid-grey: R by V, B by U, G by both
    r_lo, r_hi, b_lo, b_hi, g_lo, g_hi = convert([(512, 512, 0), (512, 512, 1023), (512, 0, 512), (512, 1023, 512),
                                                  (512, 1023, 1023), (512, 0, 0)], 10, "bt601", True)
    assert r_lo[0] == 0 and r_hi[0] == 255 and b_lo[2] == 0 and b_hi[2] == 255 and g_lo[1] == 0 and g_hi[1] == 255
    # (BT.2020's green takes 0.165 U + 0.571 V: from mid-grey it does not reach either end, red and blue do)
    r_lo, r_hi, b_lo, b_hi, g_lo, g_hi = convert([(512, 512, 0), (512, 512, 1023), (512, 0, 512), (512, 1023, 512),
                                                  (512, 1023, 1023), (512, 0, 0)], 10, "bt2020", True)
    assert r_lo[0] == 0 and r_hi[0] == 255 and b_lo[2] == 0 and b_hi[2] == 255 and 0 < g_lo[1] < g_hi[1] < 255
    # unclipped values by hand (BT.2020 full range, V = 812: R = (512 + 1.4746 * 300) * 255 / 1023 = 237.9,
    # G = (512 - 0.571353 * 300) * 255 / 1023 = 84.9, B = 512 * 255 / 1023 = 127.6)
    assert convert([(512, 512, 812)], 10, "bt2020", True) == [[238, 85, 128]]
    # one (Y, U, V) is another colour in each standard
    assert len({tuple(convert([(324, 360, 960)], 10, m)[0]) for m in KRKB}) == 3
    for bad in (dict(matrix="bt470"), dict(depth=16), dict(depth=9)):
        with pytest.raises(ValueError, match="yuv"):
            I.yuv_table(**bad)


@pytest.mark.parametrize("matrix", KRKB)
def test_codes_times_four_convert_to_the_8_bit_frame(matrix):
    y, u, v = planes("420", 8, 37, 53, batch=2)
    base = I.yuv_to_rgb(*(typed(t, 8) for t in (y, u, v)), "420", 8, False, matrix)
    if matrix != "bt2020":
        assert torch.equal(base, I.yuv420_to_rgb(*(typed(t, 8) for t in (y, u, v)), matrix))
    for depth, k in ((10, 4), (12, 16)):
        got = I.yuv_to_rgb(*(typed(t * k, depth) for t in (y, u, v)), "420", depth, False, matrix)
        assert torch.equal(got, base), depth
        high = I.yuv_to_rgb(*(typed(t * k << (16 - depth), depth) for t in (y, u, v)), "420", depth, True, matrix)
        assert torch.equal(high, base), depth
    # (not so in full range, whose scale is 255 / (2^d - 1))
    full8 = I.yuv_to_rgb(*(typed(t, 8) for t in (y, u, v)), "420", 8, False, matrix, True)
    assert not torch.equal(I.yuv_to_rgb(*(typed(t * 4, 10) for t in (y, u, v)), "420", 10, False, matrix, True), full8)


@pytest.mark.parametrize("sub", ("422", "444"))
def test_every_luma_pixel_takes_the_chroma_of_its_geometry(sub):
    h, w = 37, 53
    hs, vs = I.YUV_SUBSAMPLING[sub]
    ch, cw = (h + (1 << vs) - 1) >> vs, (w + (1 << hs) - 1) >> hs
    assert (ch, cw) == ((37, 27) if sub == "422" else (37, 53))
    # Y constant; U a ramp over the chroma index, V another (descending): a pixel's colour names its chroma sample
    base = torch.zeros(h, 64, dtype=torch.uint8)                      # pitch 64 > w, padding 0 ...
    base[:, :w] = 128
    y = base[:, :w]
    idx = torch.arange(ch * cw).reshape(ch, cw)
    u_ramp, v_ramp = (idx % 251).to(torch.uint8), (250 - idx % 241).to(torch.uint8)
    ubase, vbase = (torch.full((ch, cw + p), 255, dtype=torch.uint8) for p in (10, 7))   # ... chroma pitches, padding 255
    u, v = ubase[:, :cw], vbase[:, :cw]
    u.copy_(u_ramp), v.copy_(v_ramp)
    assert y.stride() == (64, 1) and u.stride() == (cw + 10, 1) and v.stride() == (cw + 7, 1)
    got = I.yuv_to_rgb(y, u, v, sub, 8, False, "bt601", True)
    assert got.shape == (1, h, w, 3) and got.dtype == torch.uint8
    rows, cols = torch.arange(h) >> vs, torch.arange(w) >> hs
    real = np.stack(real_rgb(128, u_ramp[rows][:, cols].numpy(), v_ramp[rows][:, cols].numpy(), "bt601", True), -1)
    clear = np.abs(real - np.floor(real) - 0.5) > 0.01
    assert clear.mean() > 0.95
    assert np.array_equal(got[0].numpy()[clear], np.clip(np.rint(real), 0, 255).astype(np.uint8)[clear])
    # the ramps make neighbours differ along both axes: a row or a column off by one, or halved where it is not, shows
    assert not torch.equal(got[0, :, :-2], got[0, :, 2:]) and not torch.equal(got[0, :-1], got[0, 1:])
    if sub == "444":
        assert not torch.equal(got[0, :, :-1], got[0, :, 1:])
    assert not torch.equal(I.yuv_to_rgb(y, v, u, sub, 8, False, "bt601", True), got)
    # a wrong geometry is refused, by its name
    with pytest.raises(ValueError, match="4:2:0"):
        I.yuv_to_rgb(y, u, v, "420")
    with pytest.raises(ValueError, match="subsampling"):
        I.yuv_to_rgb(y, u, v, "411")


def test_yuy2_odd_width_takes_the_last_macropixel():
    h, w = 5, 7
    g = torch.Generator().manual_seed(1)
    data = torch.randint(0, 256, (h, 4 * 4 + 3), generator=g, dtype=torch.uint8)    # 4 macropixels and 3 pad bytes
    y, u, v = I.yuyv_planes(data, w, "yuyv")
    assert y.shape == (1, h, 7) and u.shape == v.shape == (1, h, 4)
    assert torch.equal(y[0], data[:, 0:14:2]) and torch.equal(u[0], data[:, 1:16:4]) and torch.equal(v[0], data[:, 3:16:4])
    got = I.yuyv_to_rgb(data, w, "yuyv")
    assert got.shape == (1, h, 7, 3)
    # the last column: luma byte 12, and the last macropixel's U and V (bytes 13 and 15)
    last = I.yuv_to_rgb(data[:, 12:13], data[:, 13:14], data[:, 15:16], "444")
    assert torch.equal(got[0, :, 6], last[0, :, 0])
    # its second luma (byte 14) and the pad bytes are never shown
    other = data.clone()
    other[:, 14] = 255 - other[:, 14]
    other[:, 16:] = 255 - other[:, 16:]
    assert torch.equal(I.yuyv_to_rgb(other, w, "yuyv"), got)
    other[:, 15] = 255 - other[:, 15]
    assert not torch.equal(I.yuyv_to_rgb(other, w, "yuyv")[0, :, 6], got[0, :, 6])
    for bad, what in (((data[:, :15], w), "16 bytes"), ((data, w, "vyuy"), "order"), ((data.float(), w), "uint8"),
                      ((data.t(), 2), "contiguous")):
        with pytest.raises(ValueError, match=what):
            I.yuyv_planes(*bad)


@pytest.mark.parametrize("depth", (10, 12))
def test_bits_that_do_not_count(depth):
    y, u, v = planes("422", depth, 9, 11, batch=2, seed=2)
    g = torch.Generator().manual_seed(3)
    want = I.yuv_to_rgb(*(typed(t, depth) for t in (y, u, v)), "422", depth)
    for msb in (False, True):
        junk = [torch.randint(1, 1 << (16 - depth), t.shape, generator=g, dtype=torch.int32) for t in (y, u, v)]
        if msb:
            clean, noisy = [t << (16 - depth) for t in (y, u, v)], [t << (16 - depth) | j for t, j in zip((y, u, v), junk)]
        else:
            clean, noisy = [y, u, v], [t | j << depth for t, j in zip((y, u, v), junk)]
        for dtype in (torch.uint16, torch.int16):
            a = I.yuv_to_rgb(*(typed(t, depth, dtype) for t in clean), "422", depth, msb)
            b = I.yuv_to_rgb(*(typed(t, depth, dtype) for t in noisy), "422", depth, msb)
            assert a.dtype == torch.uint8 and torch.equal(a, want) and torch.equal(b, want), (msb, dtype)
        words = typed(noisy[0], depth)
        assert words.dtype == torch.uint16 and torch.equal(I.yuv_codes(words, depth, msb), y)
        assert torch.equal(I.yuv_codes(words.view(torch.int16), depth, msb), y)
        # read the other way round the noisy words are another picture
        assert not torch.equal(I.yuv_codes(words, depth, not msb), y)
    assert torch.equal(I.yuv_codes(typed(y & 255, 8)), y & 255)
    for bad in ((typed(y & 255, 8), depth), (typed(y, depth), 8), (y, depth)):
        with pytest.raises(ValueError, match="depth"):
            I.yuv_codes(*bad)


def semiplanar(u, v, vu=False):
    return torch.stack((v, u) if vu else (u, v), dim=-1)


def packed(y, u, v, order, pad=0):
    """uint8 planes ``[B, h, w]`` / ``[B, h, cw]`` as packed 4:2:2 rows with ``pad`` more bytes each."""
    B, h, w = y.shape
    cw = u.shape[2]
    data = torch.full((B, h, 4 * cw + pad), 77, dtype=torch.uint8)
    yo, uo, vo = I.YUYV_ORDERS[order]
    yy = torch.full((B, h, 2 * cw), 99, dtype=torch.uint8)
    yy[..., :w] = y
    data[..., yo:4 * cw:2], data[..., uo:4 * cw:4], data[..., vo:4 * cw:4] = yy, u, v
    return data


def test_compositions():
    out, ms = (80, 112), (IMAGENET_MEAN, IMAGENET_STD)
    y, u, v = (typed(t, 8) for t in planes("420", 8, 37, 53, batch=2, seed=4))
    for matrix, full in (("bt601", False), ("bt709", True)):
        assert torch.equal(I.yuv_to_rgb(y, u, v, "420", 8, False, matrix, full), I.yuv420_to_rgb(y, u, v, matrix, full))

    def same(got, rgb):
        want = I.image_patch_planes(rgb, out, P, *ms, True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])

    for sub, depth, msb in (("422", 8, False), ("444", 8, False), ("420", 10, True), ("422", 10, False),
                            ("444", 12, True)):
        y, u, v = planes(sub, depth, 37, 53, batch=2, seed=5)
        y, u, v = (typed(t << (16 - depth) if msb else t, depth) for t in (y, u, v))
        rgb = I.yuv_to_rgb(y, u, v, sub, depth, msb, "bt2020", True)
        assert not torch.equal(rgb, I.yuv_to_rgb(y, u, v, sub, depth, msb))
        same(I.yuv_planar_patch_planes(y, u, v, out, P, *ms, sub, depth, msb, "bt2020", True, True), rgb)
        only, none = I.yuv_planar_patch_planes(y, u, v, out, P, *ms, sub, depth, msb, "bt2020", True)
        assert none is None and torch.equal(only, I.image_patch_planes(rgb, out, P, *ms)[0])
        for vu in (False, True):
            uv = semiplanar(u, v, vu)
            assert torch.equal(I.yuv_semiplanar_to_rgb(y, uv, sub, depth, msb, "bt2020", True, vu), rgb)
            same(I.yuv_semiplanar_patch_planes(y, uv, out, P, *ms, sub, depth, msb, "bt2020", True, True, vu), rgb)
        assert not torch.equal(I.yuv_semiplanar_to_rgb(y, semiplanar(u, v, True), sub, depth, msb, "bt2020", True), rgb)
    y, u, v = (typed(t, 8) for t in planes("422", 8, 37, 53, batch=2, seed=6))
    rgb = I.yuv_to_rgb(y, u, v, "422", 8, False, "bt709")
    for order in I.YUYV_ORDERS:
        data = packed(y, u, v, order, pad=5)
        assert all(torch.equal(a, b) for a, b in zip(I.yuyv_planes(data, 53, order), (y, u, v)))
        assert torch.equal(I.yuyv_to_rgb(data, 53, order, "bt709"), rgb)
        same(I.yuyv_patch_planes(data, 53, order, out, P, *ms, "bt709", False, True), rgb)
    assert not torch.equal(I.yuyv_to_rgb(packed(y, u, v, "yuyv"), 53, "uyvy", "bt709"), rgb)


#: one name of each row of the name table: (h, w, pitch, chroma pitch) -> plane byte offsets, pitches (bytes)
BUFFERS = {"i422": (6, 10, 16, 12), "nv24": (6, 10, 16, 24), "uyvy": (6, 10, 24, None), "p210": (6, 10, 32, 28),
           "i010": (6, 10, 32, 14)}


@pytest.mark.parametrize("name", BUFFERS)
def test_from_buffer_views_one_buffer(name):
    h, w, pitch, cpitch = BUFFERS[name]
    kind, sub, depth, msb, swap = S.FORMATS[name]
    buf = torch.randint(0, 256, (2048,), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    f = S.from_buffer(name, buf, h, w, pitch, cpitch, matrix="bt2020", full_range=True)
    assert isinstance(f, Frame) and f.shape == (1, h, w, 3) and (f.matrix, f.full_range) == ("bt2020", True)
    base = buf.data_ptr()
    sb = 1 if depth == 8 else 2
    offs = {p: (getattr(f, p).data_ptr() - base, getattr(f, p).stride(0) * getattr(f, p).element_size()) for p in f.PLANES}
    ch = h // 2 if sub == "420" else h
    if kind == "packed":
        assert type(f) is S.Yuyv and offs == {"data": (0, pitch)} and f.data.shape == (h, 20) and f.order == "uyvy"
    elif kind == "semiplanar":
        assert type(f) is S.YuvSemiPlanar and offs == {"y": (0, pitch), "uv": (h * pitch, cpitch)}
        assert f.uv.shape == (ch, w if sub == "444" else w // 2, 2) and f.uv.stride()[1:] == (2, 1)
    else:
        assert type(f) is S.YuvPlanar
        assert offs == {"y": (0, pitch), "u": (h * pitch, cpitch), "v": (h * pitch + ch * cpitch, cpitch)}
    if kind != "packed":
        assert (f.subsampling, f.depth, f.msb) == (sub, depth, msb) and f.y.shape == (h, w)
        assert f.y.dtype == (torch.uint8 if depth == 8 else torch.uint16)
    # no copy: the planes live in the buffer, and a new frame written there is seen
    for p in f.PLANES:
        assert getattr(f, p).untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
    before = f.rgb()
    buf.copy_(255 - buf)
    assert not torch.equal(f.rgb(), before)
    y_bytes = buf[:h * pitch].reshape(h, pitch)[:, :f.y.shape[1] * sb] if kind != "packed" else None
    if kind != "packed":
        assert torch.equal(f.y.view(torch.uint8) if sb == 2 else f.y, y_bytes)
    # default pitches, an ndarray, and a buffer that ends with the last row's bytes
    arr = np.arange(2048, dtype=np.uint8)
    g = S.from_buffer(name, arr, h, w)
    assert np.shares_memory(getattr(g, g.PLANES[-1]).numpy(), arr) and g.shape == (1, h, w, 3)
    need = max(getattr(f, p).data_ptr() - base + (getattr(f, p).shape[0] - 1) * getattr(f, p).stride(0) * sb
               + getattr(f, p)[0].numel() * sb for p in f.PLANES)
    S.from_buffer(name, buf[:need], h, w, pitch, cpitch)
    row = 20 if kind == "packed" else w * sb
    for args, what in (((buf[:need - 1], h, w, pitch, cpitch), "bytes"), ((buf, h, w, row - 2, cpitch), "pitch"),
                       ((buf.float(), h, w, pitch, cpitch), "uint8"), ((buf, 0, w, pitch, cpitch), "positive")):
        with pytest.raises(ValueError, match=what) as e:
            S.from_buffer(name, *args)
        assert name in str(e.value)
    if sub == "420":
        with pytest.raises(ValueError, match="even height") as e:
            S.from_buffer(name, buf, h + 1, w, pitch, cpitch)
        assert name in str(e.value)
    if sb == 2:
        for args in ((buf, h, w, pitch + 1, cpitch), (buf, h, w, pitch, cpitch + 1), (buf[1:], h, w, pitch, cpitch)):
            with pytest.raises(ValueError, match="even") as e:
                S.from_buffer(name, *args)
            assert name in str(e.value)
    if kind == "planar":
        with pytest.raises(ValueError, match="chroma pitch"):
            S.from_buffer(name, buf, h, w, pitch, (w // 2) * sb - sb)


def test_from_buffer_names():
    from walkai_nos_amd.dataplane import client
    assert set(client.SURFACES) == set(S.FORMATS) and len(S.FORMATS) == 19
    with pytest.raises(ValueError, match="y210") as e:
        S.from_buffer("y210", torch.zeros(1024, dtype=torch.uint8), 4, 4)
    assert "unknown format" in str(e.value)
    buf = torch.randint(0, 256, (4096,), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    for a, b in (("i422", "yv16"), ("i444", "yv24"), ("nv16", "nv61"), ("nv24", "nv42")):
        fa, fb = S.from_buffer(a, buf, 6, 10), S.from_buffer(b, buf, 6, 10)
        if a[0] == "n":
            assert fb.vu and not fa.vu and fa.uv.data_ptr() == fb.uv.data_ptr()
        else:
            assert fa.u.data_ptr() == fb.v.data_ptr() and fa.v.data_ptr() == fb.u.data_ptr()
        assert not torch.equal(fa.rgb(), fb.rgb())
    # the same bytes by every name convert as the definition says, and each op on the CPU is the RGB op on that
    for name in S.FORMATS:
        f = S.from_buffer(name, buf, 6, 10)
        kind, sub, depth, msb, swap = S.FORMATS[name]
        if kind == "packed":
            want = I.yuv_to_rgb(*I.yuyv_planes(f.data, 10, f.order), "422")
        elif kind == "semiplanar":
            want = I.yuv_to_rgb(f.y, f.uv[..., int(swap)], f.uv[..., 1 - int(swap)], sub, depth, msb)
        else:
            want = I.yuv_to_rgb(f.y, f.u, f.v, sub, depth, msb)
        assert torch.equal(f.rgb(), want), name
        got = f.patch_planes((32, 48), P, IMAGENET_MEAN, IMAGENET_STD, True)
        ref = I.image_patch_planes(want, (32, 48), P, IMAGENET_MEAN, IMAGENET_STD, True)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), name


def test_frames_are_frames_and_the_older_ones_are_as_they_were():
    from walkai_nos_amd.models.workload import yolos
    buf = torch.randint(0, 256, (4096,), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    frames = [S.from_buffer(n, buf, 4, 6) for n in ("i444", "p010", "yuy2")]
    assert {type(f) for f in frames} == {S.YuvPlanar, S.YuvSemiPlanar, S.Yuyv}
    for f in frames:
        assert isinstance(f, Frame) and f.shape == (1, 4, 6, 3) and f.device == torch.device("cpu") and not f.is_cuda
        assert f.to("cpu") is f and f.to(None) is f and YolosProcessor.as_batch(f) is f
        moved = f.to("meta")
        assert type(moved) is type(f) and moved.device.type == "meta" and moved.shape == f.shape
        rgb = f.rgb()
        assert rgb.shape == (1, 4, 6, 3) and rgb.dtype == torch.uint8 and rgb.is_contiguous()
        for name in ("shape", "rgb", "patch_planes", "PLANES"):
            assert name in vars(type(f))
        with pytest.raises(Exception):
            f.depth = 8                                               # frozen
    # processor.py names the three older formats and nothing new; they still refuse BT.2020
    formats = {c for c in vars(PR).values() if isinstance(c, type) and issubclass(c, Frame) and c is not Frame}
    assert formats == {Nv12, Yuv420p, Packed}
    y = torch.zeros(4, 6, dtype=torch.uint8)
    c = torch.zeros(2, 3, dtype=torch.uint8)
    for refused in (lambda: I.nv12_table("bt2020"), lambda: Nv12(y, torch.stack((c, c), -1), "bt2020"),
                    lambda: Yuv420p(y, c, c, "bt2020")):
        with pytest.raises(ValueError, match="matrix"):
            refused()
    assert "bt2020" not in I.NV12_MATRICES and set(I.YUV_MATRICES) == set(I.NV12_MATRICES) | {"bt2020"}
    new = {S.YuvPlanar, S.YuvSemiPlanar, S.Yuyv}
    for name, obj in vars(yolos).items():
        assert not any(obj is c for c in new) and obj is not S, name
    assert not {"YuvPlanar", "YuvSemiPlanar", "Yuyv", "surfaces"} & set(vars(yolos))
    # a frame refuses what its op would: planes of the wrong geometry, dtype or matrix
    f = frames[0]
    for bad in (lambda: S.YuvPlanar(f.y, f.u[:-1], f.v), lambda: S.YuvPlanar(f.y, f.u, f.v, "444", 10),
                lambda: S.YuvPlanar(f.y, f.u, f.v, "444", matrix="bt470"), lambda: S.Yuyv(frames[2].data, 7),
                lambda: S.YuvSemiPlanar(frames[1].y, frames[1].uv[..., :1], "420", 10)):
        with pytest.raises(ValueError):
            bad()


def test_model_and_processor_take_the_new_frames_on_the_cpu():
    from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=1)).eval()
    m.processor = YolosProcessor(80, 133)
    buf = torch.randint(0, 256, (48 * 64 * 6,), generator=torch.Generator().manual_seed(10), dtype=torch.uint8)
    for name in ("p010", "nv16", "yuy2", "i444"):
        frame = S.from_buffer(name, buf, 48, 64, matrix="bt709")
        rgb = frame.rgb()
        assert m.processor.as_batch(frame) is frame
        assert torch.equal(m.processor.preprocess(frame), m.processor.preprocess(rgb))
        with torch.no_grad():
            got, want = m.detect_image(frame, 0.0), m.detect_image(rgb, 0.0)
        assert sorted(got) == sorted(want) and len(got) == 6
        for k in want:
            assert torch.equal(got[k], want[k]), (name, k)
        assert torch.equal(m._target_sizes(frame), torch.tensor([[48.0, 64.0]]))
