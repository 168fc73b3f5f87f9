"""``ops.image.mosaic_reference`` against the rule of ``ops.image.mosaic`` as a loop per sample over the bytes of
``overlay_case``'s surfaces, the whole allocation compared byte for byte; and ``Overlay``'s ``pixelate`` / ``cell``."""
import pytest
import torch

import overlay_case as C
from walkai_nos_amd.models.workload.overlay import Overlay
from walkai_nos_amd.ops import image as I

H, W, CELL = 10, 14, 4
#: inside one cell; ending on a cell border (columns 4..7: not cell 2); one ulp past it (4..8); half outside the frame
BOXES = [[5.2, 5.1, 6.5, 6.9], [4.5, 0.5, 8.0, 2.0], [4.5, 4.5, C.ulp_up(8.0), 6.0], [11.5, 7.0, 20.0, 30.0]]
MARKED = {(0, 1), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3)}


def loop(storage: bytes, planes, depth: int, h: int, w: int, cell: int, marked) -> bytes:
    """``storage`` with every sample of every marked cell replaced by the cell's rounded mean, plane by plane."""
    out = bytearray(storage)
    for p in planes:
        mask = (1 << depth) - 1 if p.sb == 2 else 255
        for i, j in marked:
            at = [p.off + cy * p.pitch + cx * p.step
                  for cy in range((h + (1 << p.vs) - 1) >> p.vs) if (cy << p.vs) // cell == i
                  for cx in range((w + (1 << p.hs) - 1) >> p.hs) if (cx << p.hs) // cell == j]
            codes = [(int.from_bytes(storage[a:a + p.sb], "little") >> p.shift) & mask for a in at]
            m = (sum(codes) + len(codes) // 2) // len(codes)
            for a in at:
                out[a:a + p.sb] = (m << p.shift).to_bytes(p.sb, "little")
    return bytes(out)


@pytest.mark.parametrize("layout", ("rgb", "nv12", "p010", "yuy2"))
def test_reference_is_the_loop(layout):
    sc = C.Scene("mosaic", [0.9] * 4, [0, 1, 4, 5], BOXES)
    surf = C.surface(layout, H, W)
    before = bytes(surf.storage.numpy().tobytes())
    lists = sc.tensors()
    select = torch.tensor(sc.modes, dtype=torch.uint8)
    cells = I.mosaic_cells(H, W, *lists, 1, select, CELL)
    assert {tuple(k) for k in cells.nonzero().tolist()} == MARKED and cells.shape == (3, 4)
    I.mosaic_reference(surf.target, *lists, select=select, cell=CELL)
    got = bytes(surf.storage.numpy().tobytes())
    assert got == loop(before, surf.planes, surf.depth, H, W, CELL, MARKED) and got != before
    I.mosaic_reference(surf.target, *lists, select=select, cell=CELL)
    assert bytes(surf.storage.numpy().tobytes()) == got             # a second time changes nothing


def test_overlay_pixelate_arguments():
    ov = Overlay(pixelate=(1, 2), modes={2: 1})
    assert [ov.cell_size(h, 2 * h) for h in (96, 480, 1080, 2160)] == [4, 8, 32, 64]
    assert ov.modes[1] == 0 and ov.modes[2] == 1 and ov.modes[0] == 1 and Overlay(pixelate=(1,), cell=16).cell_size(96, 96) == 16
    for bad in (dict(pixelate=(1,), redact=(1, 5)), dict(pixelate=(1,), cell=6), dict(pixelate=(91,))):
        with pytest.raises(ValueError):
            Overlay(**bad)
