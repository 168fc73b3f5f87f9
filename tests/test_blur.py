"""``ops.image.blur_taps`` against the literal tables of the rule, ``ops.image.blur_reference`` against rule 4 of
``ops.image.blur`` as a loop per sample over the bytes of ``overlay_case``'s surfaces, the whole allocation compared byte
for byte, and ``Overlay``'s ``blur`` / ``blur_radius``."""
import math

import pytest
import torch

import overlay_case as C
from walkai_nos_amd.models.workload.overlay import Overlay
from walkai_nos_amd.ops import image as I

H, W = 10, 14
#: at the top-left corner; inside; ending one ulp past column 8 (columns 4..8); half outside at the bottom-right
BOXES = [[0.0, 0.0, 3.5, 2.5], [5.2, 5.1, 6.5, 6.9], [4.5, 4.5, C.ulp_up(8.0), 6.0], [11.5, 7.0, 20.0, 30.0]]


def test_taps():
    assert I.blur_taps(0).tolist() == [256] and I.blur_taps(1).tolist() == [27, 202, 27]
    assert I.blur_taps(2).tolist() == [14, 63, 102, 63, 14] and I.blur_taps(32)[32] == 6
    for rho in range(33):
        t = I.blur_taps(rho).tolist()
        assert len(t) == 2 * rho + 1 and sum(t) == 256 and t == t[::-1] and min(t) >= 1


def loop(storage: bytes, planes, depth: int, h: int, w: int, radius: int, painted) -> bytes:
    """``storage`` with every sample whose owner pixel is painted replaced by rule 4, read from ``storage``."""
    out = bytearray(storage)
    for p in planes:
        mask = (1 << depth) - 1 if p.sb == 2 else 255
        ph, pw = (h + (1 << p.vs) - 1) >> p.vs, (w + (1 << p.hs) - 1) >> p.hs
        rh, rv = radius >> p.hs, radius >> p.vs
        th, tv = I.blur_taps(rh).tolist(), I.blur_taps(rv).tolist()

        def code(cy, cx):
            at = p.off + min(max(cy, 0), ph - 1) * p.pitch + min(max(cx, 0), pw - 1) * p.step
            return (int.from_bytes(storage[at:at + p.sb], "little") >> p.shift) & mask
        for cy in range(ph):
            for cx in range(pw):
                if (cy << p.vs, cx << p.hs) in painted:
                    total = sum(tv[j + rv] * th[k + rh] * code(cy + j, cx + k)
                                for j in range(-rv, rv + 1) for k in range(-rh, rh + 1))
                    at = p.off + cy * p.pitch + cx * p.step
                    out[at:at + p.sb] = (((total + (1 << 15)) >> 16) << p.shift).to_bytes(p.sb, "little")
    return bytes(out)


@pytest.mark.parametrize("radius", (1, 5))
@pytest.mark.parametrize("layout", ("rgb", "nv12", "p010", "yuy2"))
def test_reference_is_the_loop(layout, radius):
    sc = C.Scene("blur", [0.9] * 4, [0, 1, 4, 5], BOXES)
    painted = {(y, x) for x0, y0, x1, y1 in sc.boxes for y in range(max(math.floor(y0), 0), min(math.ceil(y1), H))
               for x in range(max(math.floor(x0), 0), min(math.ceil(x1), W))}
    assert (5, 8) in painted and (5, 9) not in painted and (9, 13) in painted and len(painted) == 12 + 12 + 9
    surf = C.surface(layout, H, W)
    before = bytes(surf.storage.numpy().tobytes())
    I.blur_reference(surf.target, *sc.tensors(), select=torch.tensor(sc.modes, dtype=torch.uint8), radius=radius)
    got = bytes(surf.storage.numpy().tobytes())
    assert got == loop(before, surf.planes, surf.depth, H, W, radius, painted) and got != before


def test_overlay_blur_arguments():
    ov = Overlay(blur=(1, 2), modes={2: 1}, pixelate=(3,))
    assert [ov.radius_size(h, 2 * h) for h in (480, 1080, 2160)] == [7, 16, 32]
    assert ov.modes[1] == 0 and ov.modes[2] == 1 and ov.modes[3] == 0 and ov.modes[0] == 1
    assert Overlay(blur=(1,), blur_radius=5).radius_size(2160, 3840) == 5 and Overlay(blur=(1,)).radius_size(20, 20) == 1
    for bad in (dict(blur=(1,), redact=(1, 5)), dict(blur=(1,), pixelate=(1,)), dict(blur=(1,), modes={1: 2}),
                dict(blur=(1,), blur_radius=0), dict(blur=(1,), blur_radius=33), dict(blur=(91,))):
        with pytest.raises(ValueError):
            Overlay(**bad)
