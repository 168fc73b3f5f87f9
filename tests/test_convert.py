"""``ops.image.convert_reference`` on the CPU against the rule written out per pixel in Python integers, on the pitched,
offset and crop surfaces of ``overlay_case``: the whole allocation is compared, so nothing but the samples is written."""
import numpy as np
import pytest
import torch

import overlay_case as C
from walkai_nos_amd.models.workload.scaler import Scaler
from walkai_nos_amd.ops import image as I


def table(matrix, full, depth):
    """The 12 integers of the rule: ``rint(inv(M) 2^14)``, each chroma row's largest entry replaced so the row sums to 0."""
    m, off = I.yuv_real_matrix(matrix, full, depth)
    t = [[int(v) for v in row] for row in np.rint(np.linalg.inv(m) * 16384.0)]
    for row in t[1:]:
        k = max(range(3), key=lambda i: abs(row[i]))
        row[k] = -sum(v for i, v in enumerate(row) if i != k)
    return t, off


def rule(rgb, dst):
    """The bytes of ``dst``'s allocation after the rule has stored the ``h x w`` list ``rgb`` into it."""
    h, w, H, W = len(rgb), len(rgb[0]), dst.h, dst.w
    over = lambda j, s, n, m: max(min((s + 1) * m, (j + 1) * n) - max(s * m, j * n), 0)        # noqa: E731
    A = h * w
    R = [[[(sum(over(J, y, h, H) * over(X, x, w, W) * rgb[y][x][c] for y in range(h) for x in range(w)) + A // 2) // A
           for c in range(3)] for X in range(W)] for J in range(H)]
    out = bytearray(dst.storage.numpy().tobytes())
    if dst.name not in C.PACKED:
        t, off = table(dst.target.matrix, dst.target.full_range, dst.depth)
    for p in dst.planes:
        for cy in range((H + (1 << p.vs) - 1) >> p.vs):
            for cx in range((W + (1 << p.hs) - 1) >> p.hs):
                block = [R[y][x] for y in range(cy << p.vs, min((cy + 1) << p.vs, H))
                         for x in range(cx << p.hs, min((cx + 1) << p.hs, W))]
                S, k = [sum(px[c] for px in block) for c in range(3)], len(block).bit_length() - 1
                if dst.name in C.PACKED:
                    code = S[p.comp]
                else:
                    v = sum(a * b for a, b in zip(t[p.comp], S)) + (off[p.comp] << 14 << k) + (1 << 13 << k)
                    code = min(max(v >> (14 + k), 0), (1 << dst.depth) - 1)
                at = p.off + cy * p.pitch + cx * p.step
                out[at:at + p.sb] = (code << p.shift).to_bytes(p.sb, "little")
    return bytes(out)


@pytest.mark.parametrize("size", ((5, 7), (3, 4)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", ("nv12", "i444", "p010", "uyvy", "bgra"))
def test_the_reference_is_the_rule(layout, size):
    src, dst = C.surface("nv12", 5, 7, seed=3), C.surface(layout, *size, seed=4, matrix="bt709", full_range=layout == "i444")
    before = src.storage.clone()
    want = rule(src.target.rgb()[0].tolist(), dst)
    assert I.convert_reference(src.target, dst.target) is dst.target and I.convert(src.target, dst.target) is dst.target
    assert dst.storage.numpy().tobytes() == want and torch.equal(src.storage, before)


@pytest.mark.parametrize("layout", ("nv12", "p010", "yuy2", "i010"))
def test_grey_has_neutral_chroma(layout):
    for g, size in ((0, (5, 7)), (77, (4, 6)), (255, (5, 7))):
        dst = C.surface(layout, *size, seed=g)
        I.convert(torch.full((9, 5, 3), g, dtype=torch.uint8), dst.target)
        s = I.overlay_surface(dst.target)
        for view, comp, _, _ in s.samples[1:]:
            assert (I._plane_codes(view, s.shift, dst.depth)[1] == 1 << (dst.depth - 1)).all(), (layout, g, comp)


def test_equal_sizes_reproduce_rgb():
    g = torch.Generator().manual_seed(5)
    src = C.surface("i444", 6, 9, seed=6)
    for layout in ("rgb", "crop"):
        dst = C.surface(layout, 6, 9, seed=7)
        I.convert(src.target, dst.target)
        assert torch.equal(I._chip_source(dst.target)[6](), src.target.rgb())
    rgb = torch.randint(0, 256, (6, 9, 3), generator=g, dtype=torch.uint8)
    from walkai_nos_amd.models.workload.surfaces import YuvPlanar
    deep = YuvPlanar(*(torch.zeros(6, 9, dtype=torch.uint16) for _ in range(3)), "444", 12, True, "bt2020", True)
    for target in (C.surface("i444", 6, 9, seed=8, matrix="bt709").target, C.surface("nv24", 6, 9, full_range=True).target, deep):
        s = I.overlay_surface(I.convert(rgb, target))
        m, off = I.yuv_real_matrix(*s.colour)
        real = np.einsum("ij,hwj->hwi", np.linalg.inv(m), rgb.numpy().astype(np.float64)) + np.array(off, np.float64)
        for view, comp, _, _ in s.samples:
            codes = I._plane_codes(view, s.shift, s.colour[2])[1].numpy()
            assert np.abs(codes - np.clip(real[..., comp], 0, (1 << s.colour[2]) - 1)).max() <= 1.0, (s.colour, comp)


def test_refusals():
    src, dst = C.surface("nv12", 4, 6), C.surface("bgr", 4, 6)
    from walkai_nos_amd.models.workload import surfaces as S
    deep = C.surface("p010", 4, 6).target
    pq = S.YuvSemiPlanar(deep.y, deep.uv, "420", 10, True, "bt2020", transfer="pq")
    I.convert(pq, dst.target)       # a PQ frame is read
    for frame, target in ((src.target, src.target), (src.target, pq), (torch.zeros(2, 4, 6, 3, dtype=torch.uint8), dst.target),
                          (src.target, torch.zeros(2, 4, 6, 3, dtype=torch.uint8)),
                          (src.target, torch.zeros(4, 6, 3, dtype=torch.uint8, device="meta"))):
        for fn in (I.convert, I.convert_reference):
            with pytest.raises(ValueError):
                fn(frame, target)
    with pytest.raises(ValueError, match="nv13"):
        Scaler((4, 6), format="nv13")


def test_a_scaler_without_a_format_is_what_it_was():
    src, want = C.surface("nv12", 6, 10, seed=2), C.surface("nv12", 4, 6).target
    got = Scaler((4, 6)).scale(src.target)
    I.rescale_reference(src.target, want)
    assert type(got) is type(src.target) and torch.equal(got.y, want.y) and torch.equal(got.uv, want.uv)
    out = Scaler((4, 6), format="bgra").scale(src.target)
    assert out.order == "bgra" and out.data.shape == (4, 6, 4) and (out.data[..., 3] == 0xFF).all()
    assert torch.equal(out.rgb()[0], I.convert(src.target, torch.zeros(4, 6, 3, dtype=torch.uint8)))
