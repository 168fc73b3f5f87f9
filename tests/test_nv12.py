"""NV12 frames on the CPU: the integer colour conversion (``ops.image.nv12_to_rgb``, which is both the
definition the kernel is tested against and the fallback) against the real formula over every
``(Y, U, V)``, its plane addressing, ``processor.Nv12`` and the CPU path of the op and the model.

The integer formula against fp64: a coefficient is ``round(real * 2^16)``, so the three products err
by at most ``3 * 255 * 2^-17 = 0.006`` together, and ``(sum + 2^15) >> 16`` is ``floor(x + 0.5)`` of that
sum. It can therefore differ from ``clip(round(real))`` only where the real value is within 0.006 of a
rounding tie, and then by 1."""
import numpy as np
import pytest
import torch

from walkai_nos_amd.models.workload.processor import IMAGENET_MEAN, IMAGENET_STD, Nv12, YolosProcessor
from walkai_nos_amd.ops import image as I

COMBOS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]
IDS = [f"{m}-{'full' if fr else 'limited'}" for m, fr in COMBOS]


def convert(triples, matrix="bt601", full_range=False):
    """``nv12_to_rgb`` of single pixels: ``[(Y, U, V), ...]`` -> ``[[R, G, B], ...]``."""
    t = torch.tensor(triples, dtype=torch.uint8).reshape(-1, 3)
    return I.nv12_to_rgb(t[:, 0].reshape(-1, 1, 1), t[:, 1:].reshape(-1, 1, 1, 2), matrix, full_range) \
        .reshape(-1, 3).tolist()


def real_rgb(yv, u, v, matrix, full_range):
    """The conversion as the standards state it, in fp64 and independent of ``ops.image``: ``Y' = (Y - 16) / 219``
    and ``Pb, Pr = (U - 128, V - 128) / 224`` (full range: ``Y / 255`` and ``/ 255``), ``R = Y' + 2 (1 - Kr) Pr``,
    ``B = Y' + 2 (1 - Kb) Pb``, ``G`` from ``Y' = Kr R + Kg G + Kb B``; times 255, unclipped."""
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[matrix]
    yv, u, v = (np.asarray(t, dtype=np.float64) for t in (yv, u, v))
    yp = yv / 255.0 if full_range else (yv - 16.0) / 219.0
    pb, pr = ((u - 128.0) / 255.0, (v - 128.0) / 255.0) if full_range else ((u - 128.0) / 224.0, (v - 128.0) / 224.0)
    r, b = yp + 2.0 * (1.0 - kr) * pr, yp + 2.0 * (1.0 - kb) * pb
    g = (yp - kr * r - kb * b) / (1.0 - kr - kb)
    return 255.0 * r, 255.0 * g, 255.0 * b


def nv12_frame(h, w, batch=None, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + h * 1009 + w)
    lead = () if batch is None else (batch,)
    return (torch.randint(0, 256, lead + (h, w), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, lead + ((h + 1) // 2, (w + 1) // 2, 2), generator=g, dtype=torch.uint8))


@pytest.mark.parametrize("matrix,full_range", COMBOS, ids=IDS)
def test_integer_formula_against_fp64_over_every_triple(matrix, full_range):
    m, off = I.nv12_real_matrix(matrix, full_range)
    table = I.nv12_table(matrix, full_range)
    assert len(table) == 12 and all(isinstance(v, int) for v in table) and table[9:] == off
    assert np.array_equal(np.array(table[:9]).reshape(3, 3), np.rint(m * 65536.0))
    # the overflow argument of the comment in nv12_to_rgb: every term below 2^25
    # (luma is at most 255 off its offset, chroma at most 128)
    assert max(max(abs(v) for v in table[0:9:3]) * 255, max(abs(v) for v in table[:9]) * 128) < 2 ** 25
    # the rows of the real matrix are what (Kr, Kb) define: grey stays grey, luma is recovered
    kr, kb = I.NV12_MATRICES[matrix]
    assert np.allclose(m[:, 0], m[0, 0]) and np.allclose(np.array([kr, 1 - kr - kb, kb]) @ m[:, 1:], 0.0, atol=1e-12)
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    uv = torch.from_numpy(np.stack((u, v), -1).astype(np.uint8))[None]      # [1, 256, 256, 2]: U by row, V by column
    worst, ties = 0, 0
    for yv in range(256):
        # a 512 x 512 frame of one luma value whose chroma plane holds every (U, V): each 2 x 2 block one triple
        got = I.nv12_to_rgb(torch.full((1, 512, 512), yv, dtype=torch.uint8), uv, matrix, full_range)
        assert torch.equal(got[0, ::2, ::2], got[0, 1::2, 1::2])
        got = got[0, ::2, ::2].numpy().astype(np.int64)
        for c, real in enumerate(real_rgb(yv, u, v, matrix, full_range)):
            want = np.clip(np.rint(real), 0, 255).astype(np.int64)
            diff = np.abs(got[..., c] - want)
            worst = max(worst, int(diff.max()))
            clear = np.abs(real - np.floor(real) - 0.5) > 0.01
            ties += int((~clear).sum())
            assert not diff[clear].any(), (yv, c)
    print(f"[nv12] {matrix} {'full' if full_range else 'limited'}: worst |int - round(real)| {worst} over 256^3 x 3, "
          f"{ties} values within 0.01 of a tie")
    assert worst <= 1


def test_anchor_values():
    for matrix in ("bt601", "bt709"):
        assert convert([(16, 128, 128), (235, 128, 128)], matrix) == [[0, 0, 0], [255, 255, 255]]
        assert convert([(0, 128, 128), (255, 128, 128)], matrix, True) == [[0, 0, 0], [255, 255, 255]]
        # below black and above white clip in limited range
        assert convert([(0, 128, 128), (255, 128, 128)], matrix) == [[0, 0, 0], [255, 255, 255]]
    # each channel clipping at 0 and at 255 while the luma is mid-grey: R by V, B by U, G by both
    r_lo, r_hi, b_lo, b_hi, g_lo, g_hi = convert([(128, 128, 0), (128, 128, 255), (128, 0, 128), (128, 255, 128),
                                                  (128, 255, 255), (128, 0, 0)], "bt601", True)
    assert r_lo[0] == 0 and r_hi[0] == 255 and b_lo[2] == 0 and b_hi[2] == 255 and g_lo[1] == 0 and g_hi[1] == 255
    # unclipped values by hand (BT.601 full range, V = 200: R = 128 + 1.402 * 72 = 228.9, G = 128 - 0.714136 * 72 = 76.6)
    assert convert([(128, 128, 200)], "bt601", True) == [[229, 77, 128]]
    # a saturated red is another (Y, U, V) in each standard, and one (Y, U, V) another colour
    red601, red709 = convert([(81, 90, 240)], "bt601"), convert([(81, 90, 240)], "bt709")
    assert red601 != red709 and red601[0][0] >= 250 and red601[0][1] <= 5 and red601[0][2] <= 5
    with pytest.raises(ValueError, match="matrix"):
        I.nv12_table("bt2020")


def test_every_luma_pixel_takes_chroma_at_half_its_row_and_column():
    h, w, ch, cw = 37, 53, 19, 27
    # Y constant; U a ramp over the chroma index, V another (descending): a pixel's colour names its chroma sample
    base = torch.zeros(h, 64, dtype=torch.uint8)                      # pitch 64 > w, padding 0 ...
    base[:, :w] = 128
    y = base[:, :w]
    cbase = torch.full((ch, 2 * cw + 10), 255, dtype=torch.uint8)     # ... and a UV pitch with padding 255
    idx = torch.arange(ch * cw).reshape(ch, cw)
    u_ramp, v_ramp = (idx % 251).to(torch.uint8), (250 - idx % 241).to(torch.uint8)
    uv = cbase[:, :2 * cw].unflatten(1, (cw, 2))
    uv[..., 0], uv[..., 1] = u_ramp, v_ramp
    assert y.stride() == (64, 1) and uv.stride() == (2 * cw + 10, 2, 1)
    got = I.nv12_to_rgb(y, uv, "bt601", True)
    assert got.shape == (1, h, w, 3) and got.dtype == torch.uint8
    rows, cols = torch.arange(h) // 2, torch.arange(w) // 2
    # expected without ops.image: the real formula, where it is clear of a rounding tie (all but a few pixels)
    real = np.stack(real_rgb(128, u_ramp[rows][:, cols].numpy(), v_ramp[rows][:, cols].numpy(), "bt601", True), -1)
    clear = np.abs(real - np.floor(real) - 0.5) > 0.01
    assert clear.mean() > 0.95
    assert np.array_equal(got[0].numpy()[clear], np.clip(np.rint(real), 0, 255).astype(np.uint8)[clear])
    # the ramps make neighbours differ: a swap of U and V, a row or a column off by one would show
    assert not torch.equal(got[0, :, :-2], got[0, :, 2:]) and not torch.equal(got[0, :-2], got[0, 2:])
    swapped = I.nv12_to_rgb(y, uv.flip(-1).contiguous(), "bt601", True)
    assert not torch.equal(swapped, got)
    # a batch is converted frame by frame
    y2, uv2 = nv12_frame(h, w, batch=2)
    both = I.nv12_to_rgb(y2, uv2)
    assert torch.equal(both[1], I.nv12_to_rgb(y2[1], uv2[1])[0]) and not torch.equal(both[0], both[1])


def test_plane_checks():
    y, uv = nv12_frame(36, 52)
    for bad_y, bad_uv in ((y.float(), uv), (y, uv.to(torch.int16)), (y, uv[:-1]), (y, uv[:, :-1]), (y[None], uv),
                          (y, uv[..., :1]), (y.t(), uv), (y.numpy(), uv)):
        with pytest.raises(ValueError, match="nv12"):
            I.nv12_planes(bad_y, bad_uv)
        with pytest.raises(ValueError, match="nv12"):
            Nv12(bad_y, bad_uv)
    with pytest.raises(ValueError, match="matrix"):
        Nv12(y, uv, matrix="bt2020")
    # odd sizes: the UV plane rounds up
    I.nv12_planes(*nv12_frame(37, 53))
    with pytest.raises(ValueError, match="nv12"):
        I.nv12_planes(torch.zeros(37, 53, dtype=torch.uint8), torch.zeros(18, 26, 2, dtype=torch.uint8))


def test_from_buffer_views_one_surface():
    h, w, pitch = 36, 50, 64
    buf = torch.randint(0, 256, (pitch * (h + h // 2),), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    f = Nv12.from_buffer(buf, h, w, pitch, matrix="bt709", full_range=True)
    assert (f.matrix, f.full_range) == ("bt709", True) and f.shape == (1, h, w, 3) and not f.is_cuda
    rows = buf.reshape(-1, pitch)
    assert torch.equal(f.y, rows[:h, :w]) and torch.equal(f.uv, rows[h:, :w].reshape(h // 2, w // 2, 2))
    assert f.y.stride() == (pitch, 1) and f.uv.stride() == (pitch, 2, 1)
    # no copy: the planes live in the buffer, and a new frame written there is seen
    assert f.y.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr() == f.uv.untyped_storage().data_ptr()
    before = f.rgb()
    buf.copy_(255 - buf)
    assert torch.equal(f.y, rows[:h, :w]) and not torch.equal(f.rgb(), before)
    # the default pitch is the width; an ndarray is viewed too; the last row need not be padded
    arr = np.arange(h * 3 // 2 * w, dtype=np.uint8)
    g = Nv12.from_buffer(arr, h, w)
    assert g.y.stride() == (w, 1) and np.shares_memory(g.uv.numpy(), arr) and g.uv[0, 0, 0].item() == (h * w) % 256
    Nv12.from_buffer(buf[:(h * 3 // 2 - 1) * pitch + w], h, w, pitch)
    for args, what in (((buf, h + 1, w, pitch), "even"), ((buf[:-pitch], h, w, pitch), "bytes"),
                       ((buf.float(), h, w, pitch), "uint8"), ((buf, h, w, w - 2), "pitch")):
        with pytest.raises(ValueError, match=what):
            Nv12.from_buffer(*args)
    with pytest.raises(ValueError, match="UV plane of shape"):
        Nv12(f.y, f.uv[:-1])


@pytest.mark.parametrize("hw,out", (((48, 64), (80, 96)), ((37, 53), (80, 112)), ((260, 260), (64, 64))))
def test_cpu_op_is_the_rgb_op_on_the_converted_frame(hw, out):
    y, uv = nv12_frame(*hw, batch=2)
    for matrix, full_range in COMBOS[:1] + COMBOS[-1:]:
        want = I.image_patch_planes(I.nv12_to_rgb(y, uv, matrix, full_range), out, 16, IMAGENET_MEAN, IMAGENET_STD, True)
        got = I.nv12_patch_planes(y, uv, out, 16, IMAGENET_MEAN, IMAGENET_STD, matrix, full_range, want_pixels=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    only, none = I.nv12_patch_planes(y, uv, out, 16, IMAGENET_MEAN, IMAGENET_STD)
    assert none is None and torch.equal(only, I.image_patch_planes(I.nv12_to_rgb(y, uv), out, 16, IMAGENET_MEAN,
                                                                     IMAGENET_STD)[0])


def test_model_and_processor_take_an_nv12_frame_on_the_cpu():
    from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall
    m = YolosSmall(YolosConfig(image_size=(80, 96), num_layers=1)).eval()
    m.processor = YolosProcessor(80, 133)
    y, uv = nv12_frame(48, 64)
    frame = Nv12(y, uv, "bt709")
    rgb = I.nv12_to_rgb(y, uv, "bt709")
    assert torch.equal(frame.rgb(), rgb) and m.processor.as_batch(frame) is frame
    assert torch.equal(m.processor.preprocess(frame), m.processor.preprocess(rgb))
    with torch.no_grad():
        assert torch.equal(m.encode_image(frame), m.encode_image(rgb))
        got, want = m.detect_image(frame, 0.0), m.detect_image(rgb, 0.0)
    assert sorted(got) == sorted(want) and len(got) == 6
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # boxes are scaled to the Y plane's size
    assert got["boxes"].max().item() > 1.0 and torch.equal(m._target_sizes(frame), torch.tensor([[48.0, 64.0]]))
