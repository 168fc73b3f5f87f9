"""``ops.image.rescale_reference`` on the CPU against the rule as a plain Python loop over the lattice (``loop`` reads
``overlay_case``'s surfaces byte by byte and shares no code with ``ops/image.py``), two properties of the rule, the
refusals, and ``Scaler``. There are no tolerances."""
import dataclasses

import pytest
import torch

import overlay_case as C
from walkai_nos_amd.models.workload.scaler import Scaler
from walkai_nos_amd.ops import image as I


def codes(surf: C.Surface, p: C.Plane):
    raw = bytes(surf.storage.numpy().tobytes())
    ph, pw = (surf.h + (1 << p.vs) - 1) >> p.vs, (surf.w + (1 << p.hs) - 1) >> p.hs
    at = lambda y, x: p.off + y * p.pitch + x * p.step      # noqa: E731
    return [[(int.from_bytes(raw[at(y, x):at(y, x) + p.sb], "little") >> p.shift) & ((1 << surf.depth) - 1)
             for x in range(pw)] for y in range(ph)]


def loop(src: C.Surface, dst: C.Surface) -> bytes:
    """``dst``'s allocation after rule 2, written out: every sample of every plane, and no other byte."""
    out = bytearray(dst.storage.numpy().tobytes())
    for p, q in zip(src.planes, dst.planes):
        code = codes(src, p)
        ph, pw = len(code), len(code[0])
        PH, PW = (dst.h + (1 << q.vs) - 1) >> q.vs, (dst.w + (1 << q.hs) - 1) >> q.hs
        for J in range(PH):
            for i in range(PW):
                total = 0
                for y in range(ph):
                    wy = max(min((y + 1) * PH, (J + 1) * ph) - max(y * PH, J * ph), 0)
                    for x in range(pw):
                        total += wy * max(min((x + 1) * PW, (i + 1) * pw) - max(x * PW, i * pw), 0) * code[y][x]
                at = q.off + J * q.pitch + i * q.step
                out[at:at + q.sb] = (((total + ph * pw // 2) // (ph * pw)) << q.shift).to_bytes(q.sb, "little")
    return bytes(out)


@pytest.mark.parametrize("size", ((4, 6), (9, 14)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", ("nv12", "p010", "yuy2", "crop"))
def test_reference_is_the_loop(layout, size):
    src, dst = C.surface(layout, 6, 10, seed=1), C.surface(layout, *size, seed=2)
    want, before = loop(src, dst), src.storage.clone()
    assert I.rescale_reference(src.target, dst.target) is dst.target
    assert bytes(dst.storage.numpy().tobytes()) == want and torch.equal(src.storage, before)


@pytest.mark.parametrize("layout", ("rgba", "p010", "uyvy"))
def test_equal_sizes_copy_and_two_to_one_is_the_block_mean(layout):
    src, same, half = (C.surface(layout, h, w, seed=s) for h, w, s in ((8, 12, 3), (8, 12, 4), (4, 6, 5)))
    I.rescale(src.target, same.target)      # (on the CPU rescale is the reference)
    I.rescale(src.target, half.target)
    for p, q, r in zip(src.planes, same.planes, half.planes):
        c = codes(src, p)
        assert codes(same, q) == c
        assert codes(half, r) == [[(c[y][x] + c[y][x + 1] + c[y + 1][x] + c[y + 1][x + 1] + 2) // 4
                                   for x in range(0, len(c[0]), 2)] for y in range(0, len(c), 2)]
    if layout == "p010":    # a word is stored whole: the six low bits are cleared
        low = lambda t: (t.y.view(torch.int16).to(torch.int32) & 0x3f).any()        # noqa: E731
        assert low(src.target) and not low(same.target)


def test_refusals_and_the_wide_sum():
    s = lambda name, h=4, w=6: C.surface(name, h, w).target     # noqa: E731
    whole, u8 = torch.zeros((8, 4, 3), dtype=torch.uint8), dict(dtype=torch.uint8)
    for frame, target in (
            (s("nv12"), s("nv21")), (s("nv12"), s("i420")), (s("nv12"), s("p010")), (s("i420"), s("yv12")),
            (s("yuy2"), s("uyvy")), (s("rgb"), s("bgr")), (s("rgb"), s("nv12")),        # layout, depth or order
            (whole[:4], whole[4:]),                                                     # one storage
            (dataclasses.replace(s("p010"), transfer="pq", matrix="bt2020"), s("p010", 6, 10)),
            (torch.zeros((2, 4, 4, 3), **u8), torch.zeros((4, 4, 3), **u8)),            # a batch
            (torch.zeros((4, 4, 3), **u8), torch.zeros((0, 4, 3), **u8))):              # a side of 0
        for f in (I.rescale, I.rescale_reference):
            with pytest.raises(ValueError):
                f(frame, target)
    for size in ((0, 4), (4, 8193), 7):
        with pytest.raises(ValueError):
            Scaler(size)
    # code 1023 everywhere at 2050 x 2050: the full sum passes 2^32, the reference's terms stay far below 2^53
    assert 2 ** 32 <= 2050 * 2050 * 1023 < 2 ** 53


@pytest.mark.parametrize("layout", ("rgb", "crop", "nv21", "yv12", "i010", "nv16", "yvyu"))
def test_scaler_returns_a_frame_of_the_same_kind(layout):
    src, scaler = C.surface(layout, 6, 10), Scaler((4, 7))
    out, again = scaler.scale(src.target), scaler.scale(src.target)
    want = I.rescale_reference(src.target, C.surface(layout, 4, 7, seed=9).target)
    assert type(out) is type(src.target)
    for (a, *_), (b, *_) in zip(I.overlay_surface(out).samples, I.overlay_surface(want).samples):
        assert torch.equal(a, b)
    if layout == "rgb":     # a plain [h, w, 3] tensor comes back as one
        assert out.shape == (4, 7, 3) and again is out
        return
    planes = set(out.PLANES) | {"width"}
    assert all(getattr(out, f.name) == getattr(src.target, f.name) for f in dataclasses.fields(out) if f.name not in planes)
    assert all(getattr(again, k) is getattr(out, k) for k in out.PLANES)
    assert getattr(out, "width", 7) == 7 and out.shape[:3] == (1, 4, 7)
    assert layout != "yv12" or (out.v.data_ptr() < out.u.data_ptr() and src.target.v.data_ptr() < src.target.u.data_ptr())
    assert layout != "crop" or (out.data[..., 3] == 0xFF).all()
