"""``bench.py --dump-outputs``: what the data plane's serving path returns, written per partition
slot (``bench_core.DataPlane.outputs`` / ``dump_outputs``)."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_dump_outputs_writes_every_partition_slots_inference(tmp_path):
    """Every pre-warmed slot's (logits, boxes) lands in ``<profile>_<k>_lane0_<name>.npy`` as float32,
    and is that slot's own inference: a slot no pod was put on serves once first (a captured graph's
    output buffer holds nothing of its own before the first replay), slots with different inputs give
    different arrays, and a slot's array equals the model run eagerly on the slot's input with the
    slot's CU count — the same kernels on the same tiles, so to a few fp32 roundings of outputs that
    are below 1 in magnitude (1e-5 absolute)."""
    from walkai_nos_amd.bench_core import BenchConfig, DataPlane, dump_outputs
    from walkai_nos_amd.ops import kernels as K
    cfg = BenchConfig(gpus=1, steps=1, warmup=0, dump_outputs=str(tmp_path / "dump"))
    data = DataPlane(cfg)
    try:
        served = data.slots[("dpx_nps1", 1)]
        served.submit()
        served.drain()
        rep = dump_outputs(cfg, data)
        names = sorted(os.listdir(cfg.dump_outputs))
        slots = [f"{p}_{k}" for p, n in (("spx_nps1", 1), ("dpx_nps1", 2), ("qpx_nps1", 4), ("cpx_nps1", 8))
                 for k in range(n)]
        assert names == sorted(f"{s}_lane0_{o}.npy" for s in slots for o in ("logits", "boxes"))
        assert rep["arrays"] == 30 and rep["dtype"] == "float32"
        assert sorted(rep["idle_in_window_served_once_for_the_dump"]) == sorted(set(slots) - {"dpx_nps1_1"})
        got = {n[:-4]: np.load(os.path.join(cfg.dump_outputs, n)) for n in names}
        for n, a in got.items():
            assert a.dtype == np.float32 and np.isfinite(a).all(), n
            assert a.shape == ((1, 100, 92) if n.endswith("logits") else (1, 100, 4)), (n, a.shape)
        assert rep["bytes"] == sum(a.nbytes for a in got.values()) <= 64 << 20
        # different inputs (seeds 1 and 2), the same weights and tiles: different outputs
        assert np.abs(got["cpx_nps1_1_lane0_logits"] - got["cpx_nps1_2_lane0_logits"]).max() > 1e-4
        for key in (("cpx_nps1", 3), ("dpx_nps1", 1), ("spx_nps1", 0)):
            slot = data.slots[key]
            lane = slot.lanes[0]
            K.set_slice_pin(slot.pin)
            K.set_slice_cus(lane.n_cus)
            with torch.no_grad(), torch.cuda.stream(lane.stream):
                logits, boxes = slot.model(lane.x)
            lane.stream.synchronize()
            for o, t in (("logits", logits), ("boxes", boxes)):
                err = np.abs(got[f"{key[0]}_{key[1]}_lane0_{o}"] - t.cpu().numpy()).max()
                print(key, o, "max abs difference to the eager run:", err)
                assert err <= 1e-5, (key, o, err)
    finally:
        data.close()
