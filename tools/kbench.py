"""Per-slice kernel microbenchmark on the GPU box: the YOLOS-small layer's hot ops timed on
CU-masked streams of 256/128/64/32 CUs (SPX/DPX/QPX/CPX-sized slices), one slice at a time.

    python tools/kbench.py [--iters N] [--out gpurun_out/kbench.json]

Reports microseconds per call and achieved TFLOP/s for: attention (unsplit one-wave-per-tile
baseline, stream-K LDS-shared workgroup kernel, stream-K one-wave kernel with 2 and 3
resident waves/SIMD, PyTorch SDPA), and the four fp32 GEMMs of a
layer (hipBLASLt via torch).

``--only image`` times the image pipeline instead (``csrc/image.hip``) on SPX- and CPX-sized slices:
the fused uint8 -> patch-planes kernel against the torch composition on the same GPU (``.float()``,
antialiased ``F.interpolate``, the affine, ``K.patch_planes``), the detections kernel against the
torch composition of the post-process, and ``detect_image`` against ``forward`` alone; the two sides
of each pair alternate within the run and the median of the rounds is reported. NV12 rows (a decoder
surface at a pitch of the width rounded up to 256, 480x640 and 1080x1920) time three ways to the same
planes, alternating: (a) the fused NV12 launch, (b) the RGB kernel alone on the converted frame, (c)
``nv12_to_rgb`` followed by the RGB kernel, which is what a pod without the fused path runs. The other
layouts of the same picture (``nv21_*``, ``i420_*``, ``bgr_*``, ``rgba_*``, ``bgra_*``, and ``rgbcrop_*``: RGB
rows at a padded pitch, read in place against ``.contiguous()`` first) are timed as the same triple, and so are
the surfaces of ``models/workload/surfaces.py``, one name per kernel instantiation (``i422_*``, ``i444_*``,
``nv16_*``, ``nv24_*``, ``yuy2_*``, ``p010_*``, ``i010_*``, ``p210_*``, ``i410_*``, ``i012_*``). Four of them
again with ``chroma="bilinear"`` (``i420_bilinear_*``, ``nv12_bilinear_*``, ``p010_bilinear_*``, ``yuy2_bilinear_*``):
there (c) interpolates the chroma in torch before the RGB kernel. Three more are the 10-bit surfaces as HDR frames
(BT.2020, peak 1000 nits: ``p010_pq_*``, ``p010_hlg_*``, ``i010_pq_bilinear_*``): (a) the fused launch through the
tables, (b) the same surface's nearest-chroma ``transfer="sdr"`` fused launch as the floor (``*_sdr_fused_us``), (c)
the frame's ``rgb()`` in torch on the GPU (table look-ups and the gamut matrix as tensor ops), then the RGB kernel.
Three rows time tiled detection (``--rows tiles`` runs them alone) on a 2160x3840 RGB frame at ``(2, 2)`` tiles, overlap
0.2 — tiles of 1200x2134 resized to 736x1328: ``tiles_planes_*``, the one tile launch against four
``packed_patch_planes`` launches on the crop views; ``merge_n400_*`` / ``merge_n900_*``, ``merge_detections`` of 4 and 9
tiles of 100 rows against its torch reference; and, on the whole GPU only, ``detect_tiled_ms`` against four
``detect_image`` calls on the crops (``detect_image_x4_ms``). Three more time the tiles of a YUV frame of that size
staged in place from its planes (``Frame.tile_planes``: ``*_hip_us``) against the route it replaces, the frame's
``rgb()`` followed by the packed tile launch (``*_torch_us``): ``yuv_tiles_nv12_*``, ``yuv_tiles_nv12_bilinear_*``
(siting ``left``) and ``yuv_tiles_p010_pq_*`` (BT.2020, peak 1000 nits); and, on the whole GPU only,
``detect_tiled_nv12_ms`` against ``detect_tiled`` of the converted frame, conversion included
(``detect_tiled_nv12_rgb_ms``).
Three rows time the tracker (``--rows track`` runs them alone): ``track_n100_t256_*``, ``track_n400_t256_*`` and
``track_n1000_t1024_*``, ``track_update`` of ``n`` rows on a state of ``t`` slots against its torch reference, on a
constructed scene in which about half the rows continue a track, a quarter start one and an eighth of the matched
number of tracks die. The state is restored from a saved copy inside the timed graph, so every replay does the same
work; ``*_restore_us`` is that copy alone, which both sides include. On the whole GPU ``track_image_ms`` stands beside
``detect_image_ms`` and ``track_tiled_ms`` beside ``detect_tiled_ms`` (the same calls with the tracker's launch).

Five rows time the overlay (``--rows overlay`` runs them alone): ``overlay_n100_1080p_nv12_*``, ``overlay_n400_2160p_nv12_*``,
``_rgb_*``, ``_p010_*`` and ``_nv12_redact_*`` (a quarter of the rows filled), ``ops.image.overlay`` of ``n`` rows with ids on
a lattice against ``overlay_reference``, the frame restored from a saved copy inside the timed graph on both sides
(``*_restore_us`` is that copy alone). ``*_scene`` gives the painted samples, their bytes, and those bytes over the
kernel's time (hip minus restore). On the whole GPU ``overlay_annotate_image_thr0_ms`` stands beside
``overlay_track_image_thr0_ms`` and ``overlay_annotate_tiled_thr0_ms`` beside ``overlay_track_tiled_thr0_ms``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from walkai_nos_amd.bench_core import slice_cus  # noqa: E402
from walkai_nos_amd.ops import gemm as G  # noqa: E402
from walkai_nos_amd.ops import kernels as K  # noqa: E402
from walkai_nos_amd.ops.probe import Stream  # noqa: E402

T, H, HD, D, FF = 3401, 6, 64, 384, 1536


def timeit(fn, stream, iters, warm=3):
    """GPU time per call: ``iters`` calls captured in one HIP graph on the slice's stream and
    replayed, so host-side launch overhead (ctypes, allocation) is not measured."""
    with torch.cuda.stream(stream):
        for _ in range(warm):
            fn()
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(iters):
                fn()
        g.replay()
        stream.synchronize()
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record(stream)
        g.replay()
        en.record(stream)
    en.synchronize()
    return st.elapsed_time(en) * 1000.0 / iters


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="gpurun_out/kbench.json")
    ap.add_argument("--only", choices=("all", "attn", "gemm", "model", "modes", "image"), default="all")
    ap.add_argument("--slices", default="spx,dpx,qpx,cpx")
    ap.add_argument("--rows", choices=("all", "tiles", "track", "overlay"), default="all",
                    help="image: every row, or the tiled-detection rows alone, or the tracker's, or the overlay's")
    ap.add_argument("--partitions", type=int, default=0, help="modes: run only this many partitions of each mode")
    ap.add_argument("--free-s", type=float, default=0.0,
                    help="modes: serve free-running (one thread per pod, as the bench) for this many seconds "
                         "instead of lock-step rounds")
    ap.add_argument("--lane-cus", type=int, default=0,
                    help="modes: serve partitions wider than this as request lanes of this many CUs (the bench's --lane-cus)")
    ap.add_argument("--emulation", default="spread", choices=("pinned", "spread", "landing"),
                    help="modes: compute-partition emulation (bench_core.EMULATION)")
    a = ap.parse_args()
    torch.manual_seed(0)
    if a.only == "modes":
        return modes_bench(a)
    if a.only == "image":
        return image_bench(a)
    qkv = torch.randn(1, T, 3 * D, device="cuda")
    out = torch.empty(1, T, D, device="cuda")
    x = torch.randn(T, D, device="cuda")
    h = torch.randn(T, FF, device="cuda")
    w_qkv, w_o = torch.randn(3 * D, D, device="cuda"), torch.randn(D, D, device="cuda")
    w_1, w_2 = torch.randn(FF, D, device="cuda"), torch.randn(D, FF, device="cuda")
    b_ff = torch.randn(FF, device="cuda")
    b_qkv, b_d = torch.randn(3 * D, device="cuda"), torch.randn(D, device="cuda")
    attn_flops = 4.0 * T * T * HD * H
    q, k, v = qkv.view(1, T, 3, H, HD).permute(2, 0, 3, 1, 4)
    results = []
    for prof, part, label in (("spx_nps1", 0, "spx"), ("dpx_nps1", 0, "dpx"), ("qpx_nps1", 0, "qpx"),
                              ("cpx_nps1", 0, "cpx")):
        if label not in a.slices.split(","):
            continue
        cus = slice_cus(prof, part)
        n = 256 if cus is None else len(cus)
        with Stream(0, cus) as hs:
            s = hs.torch_stream()
            r = {"slice": label, "cus": n}
            K.set_slice_cus(n)
            if a.only in ("all", "attn"):
                attn_bench(r, qkv, out, q, k, v, n, s, a.iters, attn_flops)
            if a.only in ("all", "gemm"):
                gemm_bench(r, x, h, w_qkv, w_o, w_1, w_2, b_ff, b_qkv, b_d, s, a.iters)
            if a.only in ("all", "model"):
                model_bench(r, s, max(3, a.iters // 4))
            r["layernorm_us"] = round(timeit(lambda: K.layernorm(x, w_o[0], w_o[1], 1e-12), s, a.iters), 1)
            r["layernorm_x3_us"] = round(timeit(lambda: K.layernorm_x3(x, w_o[0], w_o[1], 1e-12), s, a.iters), 1)
            for kname in list(r):
                if isinstance(r[kname], float):
                    r[kname] = round(r[kname], 2)
            print(json.dumps(r), flush=True)
            results.append(r)
    K.set_attention_variant(0)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
    return 0


def attn_bench(r, qkv, out, q, k, v, n, s, iters, attn_flops, variants=(0, 2, 3)):
    r["attn_unsplit_us"] = timeit(lambda: K.attention_unsplit(qkv, H, HD, 0.125), s, iters)
    for var in variants:
        K.set_attention_variant(var)
        wv = K.attention_waves(n)
        r[f"attn_sk{var}_us"] = timeit(lambda: K.attention_sk(qkv, out, H, HD, 0.125, wv), s, iters)
        r[f"attn_sk{var}_grid"] = wv
    K.set_attention_variant(0)
    for mult in (1, 2):  # LDS kernel with fewer persistent workgroups per CU than resident slots
        r[f"attn_sk0g{mult}_us"] = timeit(lambda: K.attention_sk(qkv, out, H, HD, 0.125, mult * n), s, iters)
    planes = K.split3(qkv)
    wx = K.attention_x3_waves(n, 1, T, H)
    r["attn_x3_us"] = timeit(lambda: K.attention_x3(planes, out, H, HD, 0.125, wx), s, iters)
    r["attn_x3_grid"] = wx
    for mult in (1, 2):
        r[f"attn_x3g{mult}_us"] = timeit(lambda: K.attention_x3(planes, out, H, HD, 0.125, mult * n), s, iters)
    K.set_attention_x3_group(4)  # the default is 8 query tiles per workgroup: time 4 as the A/B
    w4 = K.attention_x3_waves(n, 1, T, H)
    r["attn_x3q4_us"] = timeit(lambda: K.attention_x3(planes, out, H, HD, 0.125, w4), s, iters)
    r["attn_x3q4_grid"] = w4
    K.set_attention_x3_group(8)
    K.set_attention_x3_pipelined(False)
    wnp = K.attention_x3_waves(n, 1, T, H)
    r["attn_x3np_us"] = timeit(lambda: K.attention_x3(planes, out, H, HD, 0.125, wnp), s, iters)
    K.set_attention_x3_pipelined(True)
    r["split3_qkv_us"] = timeit(lambda: K.split3(qkv), s, iters)
    r["attn_sdpa_us"] = timeit(lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v), s, iters)
    for kname in [k_ for k_ in list(r) if k_.startswith("attn_") and k_.endswith("_us")
                  and not k_.startswith("split3")]:
        r[kname.replace("_us", "_tflops")] = round(attn_flops / r[kname] / 1e6, 2)


def modes_bench(a) -> int:
    """Whole-GPU throughput of each partition mode as the flagship bench runs it: every partition
    of the mode busy at once (its own CU-masked stream and graph-captured model replica), each
    running 8 x fraction inferences per round; inferences/s per GPU."""
    from walkai_nos_amd.bench_core import BenchConfig, Slot, slice_pin
    from walkai_nos_amd.models.workload.yolos import YolosSmall
    cfg = BenchConfig(lane_cus=a.lane_cus)
    template = YolosSmall()
    results = []
    for prof, n in (("spx_nps1", 1), ("dpx_nps1", 2), ("qpx_nps1", 4), ("cpx_nps1", 8)):
        if prof.split("_")[0] not in a.slices.split(","):
            continue
        n = min(n, a.partitions) if a.partitions else n
        slots = [Slot(slice_cus(prof, k, emulation=a.emulation), 0, cfg, template, seed=k,
                      pin=slice_pin(prof, k, a.emulation), split=a.lane_cus > 0) for k in range(n)]
        for sl in slots:
            sl.warm()
            sl.latency_ms.clear()
        torch.cuda.synchronize()
        work = 8 // n
        rounds = 6
        from walkai_nos_amd.bench_core import HwBusySampler
        sampler = HwBusySampler(0, period=0.02)
        sampler.start()
        t0 = time.perf_counter()
        if a.free_s > 0:
            # as the bench serves them: one thread per pod lane, each replaying its inference graph
            # and waiting for it before the next (the reference demo's loop), free-running
            done = free_running(slots, a.free_s)
        else:
            for _ in range(rounds):
                for sl in slots:
                    for _ in range(work):
                        sl.submit()
                for sl in slots:
                    sl.drain()
            done = rounds * work * n
        dt = time.perf_counter() - t0
        busy = sampler.stop()
        lat = [x for sl in slots for x in sl.latency_ms]
        r = {"mode": prof, "emulation": a.emulation, "partitions": n, "lanes_per_partition": len(slots[0].lanes),
             "serving": f"free-running threads, {a.free_s} s" if a.free_s > 0 else f"{rounds} lock-step rounds",
             "inf_per_s_per_gpu": round(done / dt, 1),
             "ms_per_round": round(1000 * dt / rounds, 2) if a.free_s <= 0 else None,
             "latency_ms_mean": round(sum(lat) / len(lat), 3) if lat else None,
             "hw_busy_pct": busy, **sampler.power_summary()}
        print(json.dumps(r), flush=True)
        results.append(r)
        for sl in slots:
            sl.close()
        torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
    return 0


def image_bench(a) -> int:
    """The image pipeline per slice: microseconds per call, fused kernel and torch composition
    interleaved (``rounds`` alternations, the median of each)."""
    import statistics

    import torch.nn.functional as F

    from walkai_nos_amd.models.workload.processor import IMAGENET_MEAN, IMAGENET_STD
    from walkai_nos_amd.models.workload.yolos import YolosSmall
    from walkai_nos_amd.ops import image as I
    out_hw, rounds = (800, 1056), 3
    ca, cb = I.affine(IMAGENET_MEAN, IMAGENET_STD)
    ca, cb = torch.tensor(ca, device="cuda").view(1, 3, 1, 1), torch.tensor(cb, device="cuda").view(1, 3, 1, 1)
    g = torch.Generator().manual_seed(0)
    imgs = {f"{h}x{w}": torch.randint(0, 256, (1, h, w, 3), generator=g, dtype=torch.uint8).cuda()
            for h, w in ((480, 640), (3024, 4032))}
    logits, boxes = 3.0 * torch.randn(1, 100, 92, device="cuda"), 0.2 + 0.6 * torch.rand(1, 100, 4, device="cuda")
    target = torch.tensor([[480.0, 640.0]], device="cuda")

    def torch_planes(img):
        x = F.interpolate(img.permute(0, 3, 1, 2).float(), size=out_hw, mode="bilinear", antialias=True,
                          align_corners=False)
        return K.patch_planes(x * ca + cb, 16)

    def pair(r, name, fused, composed, s, iters):
        t = {"hip": [], "torch": []}
        for _ in range(rounds):
            t["hip"].append(timeit(fused, s, iters))
            t["torch"].append(timeit(composed, s, iters))
        r[f"{name}_hip_us"] = round(statistics.median(t["hip"]), 1)
        r[f"{name}_torch_us"] = round(statistics.median(t["torch"]), 1)
        r[f"{name}_rounds_us"] = {k: [round(v, 1) for v in vs] for k, vs in t.items()}

    def triple(r, name, out, fused, rgb_only, convert_then_rgb, s, iters, second="rgb_kernel"):
        # five alternations: the spread of (b) within the run is what a difference (a) - (b) is read against
        t = {"fused": [], second: [], "convert_then_rgb": []}
        for _ in range(5):
            t["fused"].append(timeit(fused, s, iters))
            t[second].append(timeit(rgb_only, s, iters))
            t["convert_then_rgb"].append(timeit(convert_then_rgb, s, iters))
        r[f"{name}_target_hw"] = list(out)
        for k, vs in t.items():
            r[f"{name}_{k}_us"] = round(statistics.median(vs), 1)
        r[f"{name}_rounds_us"] = {k: [round(v, 1) for v in vs] for k, vs in t.items()}

    from walkai_nos_amd.models.workload.processor import Nv12, Packed, Yuv420p
    frames, layouts = {}, {}
    full = a.rows == "all"
    if not full:
        imgs = {}
    for h, w in ((480, 640), (1080, 1920)) if full else ():
        pitch = -(-w // 256) * 256
        surface = torch.randint(0, 256, (pitch * h * 3 // 2,), generator=g, dtype=torch.uint8).cuda()
        frames[f"{h}x{w}"] = Nv12.from_buffer(surface, h, w, pitch)
        # the other layouts: the same surface read as NV21 and as I420, and its picture as packed pixels (BGR
        # and RGBA rows side by side, BGRA and RGB in a buffer whose rows are padded to a multiple of 256 bytes)
        rgb = frames[f"{h}x{w}"].rgb()
        alpha = torch.randint(0, 256, (1, h, w, 1), generator=g, dtype=torch.uint8).cuda()

        def padded(img):
            rb = img.shape[2] * img.shape[3]
            buf = torch.zeros(h, -(-rb // 256) * 256, dtype=torch.uint8, device="cuda")
            view = buf[:, :rb].unflatten(1, img.shape[2:])[None]
            view.copy_(img)
            return view
        layouts[f"{h}x{w}"] = {"nv21": Nv12.from_buffer(surface, h, w, pitch, vu=True),
                               "i420": Yuv420p.from_buffer(surface, h, w, pitch),
                               "bgr": Packed(rgb[..., [2, 1, 0]].contiguous(), "bgr"),
                               "rgba": Packed(torch.cat((rgb, alpha), dim=-1), "rgba"),
                               "bgra": Packed(padded(torch.cat((rgb[..., [2, 1, 0]], alpha), dim=-1)), "bgra"),
                               "rgbcrop": Packed(padded(rgb), "rgb")}
        # 4:2:2, 4:4:4, packed 4:2:2 and 10 / 12-bit surfaces: one name per kernel instantiation, each a random
        # surface of its own at the same 256-byte row pitch rule
        from walkai_nos_amd.models.workload import surfaces
        for fmt in ("i422", "i444", "nv16", "nv24", "yuy2", "p010", "i010", "p210", "i410", "i012"):
            kind, _, depth = surfaces.FORMATS[fmt][:3]
            row = 4 * ((w + 1) // 2) if kind == "packed" else w * (1 if depth == 8 else 2)
            sp = -(-row // 256) * 256
            buf = torch.randint(0, 256, (3 * sp * h,), generator=g, dtype=torch.uint8).cuda()
            layouts[f"{h}x{w}"][fmt] = surfaces.from_buffer(fmt, buf, h, w, sp)
        # bilinear chroma (siting "left"): the same surfaces, one per layout and sample size, under keys of their own
        from dataclasses import replace
        fixed = layouts[f"{h}x{w}"]
        for fmt, fr in (("i420", fixed["i420"]), ("nv12", frames[f"{h}x{w}"]), ("p010", fixed["p010"]),
                        ("yuy2", fixed["yuy2"])):
            fixed[f"{fmt}_bilinear"] = replace(fr, chroma="bilinear")
        # PQ and HLG (BT.2020, peak 1000 nits): the 10-bit surfaces again, as HDR frames
        for key, fmt, kw in (("p010_pq", "p010", {"transfer": "pq"}), ("p010_hlg", "p010", {"transfer": "hlg"}),
                             ("i010_pq_bilinear", "i010", {"transfer": "pq", "chroma": "bilinear"})):
            fixed[key] = replace(fixed[fmt], matrix="bt2020", **kw)
    results = []
    for prof, label in (("spx_nps1", "spx"), ("cpx_nps1", "cpx")):
        if label not in a.slices.split(","):
            continue
        cus = slice_cus(prof, 0)
        n = 256 if cus is None else len(cus)
        with Stream(0, cus) as hs:
            s = hs.torch_stream()
            K.set_slice_cus(n)
            r = {"slice": label, "cus": n, "target_hw": list(out_hw), "iters": a.iters, "rounds": rounds}
            for name, img in imgs.items():
                pair(r, f"preprocess_{name}", lambda: I.image_patch_planes(img, out_hw, 16, IMAGENET_MEAN, IMAGENET_STD),
                     lambda: torch_planes(img), s, a.iters)
            for name, f in frames.items():
                out = I.resize_size(tuple(f.y.shape), 800, 1333)
                rgb = f.rgb()
                triple(r, f"nv12_{name}", out,
                       lambda: I.nv12_patch_planes(f.y, f.uv, out, 16, IMAGENET_MEAN, IMAGENET_STD),
                       lambda: I.image_patch_planes(rgb, out, 16, IMAGENET_MEAN, IMAGENET_STD),
                       lambda: I.image_patch_planes(I.nv12_to_rgb(f.y, f.uv), out, 16, IMAGENET_MEAN, IMAGENET_STD),
                       s, a.iters)
                for layout, fr in layouts[name].items():
                    if getattr(fr, "transfer", "sdr") != "sdr":
                        floor = replace(fr, transfer="sdr", chroma="nearest")
                        triple(r, f"{layout}_{name}", out,
                               lambda: fr.patch_planes(out, 16, IMAGENET_MEAN, IMAGENET_STD),
                               lambda: floor.patch_planes(out, 16, IMAGENET_MEAN, IMAGENET_STD),
                               lambda: I.image_patch_planes(fr.rgb(), out, 16, IMAGENET_MEAN, IMAGENET_STD),
                               s, a.iters, second="sdr_fused")
                        continue
                    conv = fr.rgb()
                    triple(r, f"{layout}_{name}", out,
                           lambda: fr.patch_planes(out, 16, IMAGENET_MEAN, IMAGENET_STD),
                           lambda: I.image_patch_planes(conv, out, 16, IMAGENET_MEAN, IMAGENET_STD),
                           lambda: I.image_patch_planes(fr.rgb(), out, 16, IMAGENET_MEAN, IMAGENET_STD),
                           s, a.iters)
            if a.rows in ("all", "tiles"):
                tiles_rows(r, pair, s, a.iters, rounds, whole_gpu=cus is None)
            if a.rows in ("all", "track"):
                track_rows(r, s, a.iters, rounds, whole_gpu=cus is None)
            if a.rows in ("all", "overlay"):
                overlay_rows(r, s, a.iters, rounds, whole_gpu=cus is None)
            if not full:
                print(json.dumps(r), flush=True)
                results.append(r)
                continue
            pair(r, "detections", lambda: I.detections(logits, boxes, target, 0.5),
                 lambda: I.detections_reference(logits, boxes, target, 0.5), s, a.iters)
            with torch.cuda.stream(s), torch.no_grad():
                m = YolosSmall().cuda().eval()
                img = imgs["480x640"][0]
                px = m.processor.preprocess(img)
                it = max(3, a.iters // 4)
                t = {"detect_image": [], "forward": []}
                for _ in range(rounds):
                    t["detect_image"].append(timeit(lambda: m.detect_image(img), s, it))
                    t["forward"].append(timeit(lambda: m(px), s, it))
            r["detect_image_ms"] = round(statistics.median(t["detect_image"]) / 1000.0, 3)
            r["forward_ms"] = round(statistics.median(t["forward"]) / 1000.0, 3)
            r["model_rounds_ms"] = {k: [round(v / 1000.0, 3) for v in vs] for k, vs in t.items()}
            print(json.dumps(r), flush=True)
            results.append(r)
    K.set_slice_cus(None)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
    return 0


def tiles_rows(r, pair, s, iters, rounds, whole_gpu):
    """Tiled detection of a 2160x3840 RGB frame at (2, 2) tiles, overlap 0.2 (see the module docstring): the pairs go
    into ``r`` as ``*_hip_us`` (the new launch) and ``*_torch_us`` (what it replaces)."""
    import statistics

    from walkai_nos_amd.models.workload.processor import IMAGENET_MEAN, IMAGENET_STD
    from walkai_nos_amd.models.workload.yolos import YolosSmall
    from walkai_nos_amd.ops import image as I
    g = torch.Generator().manual_seed(1)
    frame = torch.randint(0, 256, (2160, 3840, 3), generator=g, dtype=torch.uint8).cuda()
    th, tw, origins = I.tile_plan(2160, 3840, (2, 2), 0.2)
    out = I.resize_size((th, tw), 800, 1333)
    r["tiles"] = {"frame_hw": [2160, 3840], "tile_hw": [th, tw], "target_hw": list(out), "origins": origins}
    crops = [frame[None, y:y + th, x:x + tw] for y, x in origins]        # views: read in place
    pair(r, "tiles_planes", lambda: I.tiled_patch_planes(frame, "rgb", origins, (th, tw), out, 16, IMAGENET_MEAN,
                                                         IMAGENET_STD),
         lambda: [I.packed_patch_planes(c, "rgb", out, 16, IMAGENET_MEAN, IMAGENET_STD) for c in crops], s, iters)
    for B in (4, 9):
        lg = 3.0 * torch.randn(B, 100, 92, generator=g).cuda()
        bx = (0.2 + 0.6 * torch.rand(B, 100, 4, generator=g)).cuda()
        org = [(300 * (b // 3), 400 * (b % 3)) for b in range(B)]
        # (the reference is B * 100 steps of three launches: fewer calls per graph)
        t = {"hip": [], "torch": []}
        for _ in range(rounds):
            t["hip"].append(timeit(lambda: I.merge_detections(lg, bx, org, (th, tw), 0.1), s, iters))
            t["torch"].append(timeit(lambda: I.merge_detections_reference(lg, bx, org, (th, tw), 0.1), s, 2))
        r[f"merge_n{B * 100}_hip_us"] = round(statistics.median(t["hip"]), 1)
        r[f"merge_n{B * 100}_torch_us"] = round(statistics.median(t["torch"]), 1)
        r[f"merge_n{B * 100}_rounds_us"] = {k: [round(v, 1) for v in vs] for k, vs in t.items()}
        r[f"merge_n{B * 100}_kept"] = int(I.merge_detections(lg, bx, org, (th, tw), 0.1)[0].item())
    # the tiles of a YUV frame: staged from the planes by one launch, against rgb() and the packed tile launch
    from dataclasses import replace

    from walkai_nos_amd.models.workload import surfaces
    from walkai_nos_amd.models.workload.processor import Nv12
    nv12 = Nv12.from_buffer(torch.randint(0, 256, (3840 * 2160 * 3 // 2,), generator=g, dtype=torch.uint8).cuda(),
                            2160, 3840)
    p010 = surfaces.from_buffer("p010", torch.randint(0, 256, (3840 * 2160 * 3,), generator=g, dtype=torch.uint8).cuda(),
                                2160, 3840, matrix="bt2020", transfer="pq")
    for name, fr in (("nv12", nv12), ("nv12_bilinear", replace(nv12, chroma="bilinear")), ("p010_pq", p010)):
        pair(r, f"yuv_tiles_{name}", lambda: fr.tile_planes(origins, (th, tw), out, 16, IMAGENET_MEAN, IMAGENET_STD),
             lambda: I.tiled_patch_planes(fr.rgb(), "rgb", origins, (th, tw), out, 16, IMAGENET_MEAN, IMAGENET_STD),
             s, iters)
    if not whole_gpu:
        return
    with torch.cuda.stream(s), torch.no_grad():
        m = YolosSmall().cuda().eval()
        it = max(2, iters // 5)
        t = {"detect_tiled": [], "detect_image_x4": []}
        for _ in range(rounds):
            t["detect_tiled"].append(timeit(lambda: m.detect_tiled(frame, (2, 2), 0.2), s, it))
            t["detect_image_x4"].append(timeit(lambda: [m.detect_image(c) for c in crops], s, it))
    r["detect_tiled_ms"] = round(statistics.median(t["detect_tiled"]) / 1000.0, 3)
    r["detect_image_x4_ms"] = round(statistics.median(t["detect_image_x4"]) / 1000.0, 3)
    r["tiles_model_rounds_ms"] = {k: [round(v / 1000.0, 3) for v in vs] for k, vs in t.items()}
    with torch.cuda.stream(s), torch.no_grad():
        t = {"detect_tiled_nv12": [], "detect_tiled_nv12_rgb": []}
        for _ in range(rounds):
            t["detect_tiled_nv12"].append(timeit(lambda: m.detect_tiled(nv12, (2, 2), 0.2), s, it))
            t["detect_tiled_nv12_rgb"].append(timeit(lambda: m.detect_tiled(nv12.rgb()[0], (2, 2), 0.2), s, it))
    for k, vs in t.items():
        r[f"{k}_ms"] = round(statistics.median(vs) / 1000.0, 3)
    r["yuv_tiles_model_rounds_ms"] = {k: [round(v / 1000.0, 3) for v in vs] for k, vs in t.items()}


def track_scene(n: int, T: int, seed: int = 0):
    """``(state, lists, what)``: a tracker of ``T`` slots holding ``matched + dying`` tracks on a lattice of 64 px
    cells, and ``n`` rows of which ``matched = min(n, T) // 2`` continue a track (moved by its velocity and a pixel),
    ``n // 4`` start one and the rest lie behind ``count``; the ``matched // 8`` other tracks are at ``max_age``."""
    from walkai_nos_amd.ops import image as I
    g = torch.Generator().manual_seed(3000 + seed + n)
    matched, born = min(n, T) // 2, n // 4
    dying = matched // 8
    live = matched + dying
    cell = torch.arange(live + born)
    xy = torch.stack((64.0 * (cell % 40), 64.0 * (cell // 40)), dim=1) + 8.0
    state = I.track_state(T, "cpu")
    slots = torch.randperm(T, generator=g)[:live]
    state.boxes[slots] = torch.cat((xy[:live], xy[:live] + 32.0), dim=1)
    state.vel[slots] = torch.tensor([2.0, 1.0, 2.0, 1.0])
    state.labels[slots] = (cell[:live] % 16).to(torch.int32)
    state.ids[slots] = torch.arange(1, live + 1, dtype=torch.int32)
    state.hits[slots] = 3
    state.misses[slots[matched:]] = 30
    state.next_id.fill_(live + 1)
    seen = torch.cat((cell[:matched], cell[live:]))                    # the matched objects and the new ones
    rows = torch.arange(seen.shape[0])
    order = torch.randperm(seen.shape[0], generator=g)
    seen = seen[order]
    boxes = torch.zeros(n, 4)
    boxes[rows] = torch.cat((xy[seen] + 3.0, xy[seen] + 35.0), dim=1)
    scores = torch.zeros(n)
    scores[rows] = 0.25 + 0.7 * (torch.randperm(seen.shape[0], generator=g).float() + 1.0) / seen.shape[0]
    labels = torch.zeros(n, dtype=torch.int32)
    labels[rows] = (seen % 16).to(torch.int32)
    count = torch.tensor([seen.shape[0]], dtype=torch.int32)
    return state, (count, scores, labels, boxes), {"matched": matched, "born": born, "dying": dying}


def track_rows(r, s, iters, rounds, whole_gpu):
    """The tracker (see the module docstring): ``track_n*_t*_hip_us`` against ``*_torch_us``, both with the restore of
    the state that ``*_restore_us`` times alone."""
    import statistics

    from walkai_nos_amd.models.workload.tracker import Tracker
    from walkai_nos_amd.models.workload.yolos import YolosSmall
    from walkai_nos_amd.ops import image as I
    for n, T in ((100, 256), (400, 256), (1000, 1024)):
        saved, lists, what = track_scene(n, T)
        saved = [t.cuda() for t in saved.tensors()]
        lists = [t.cuda() for t in lists]
        state = I.track_state(T, "cuda")

        def restore():
            for dst, src in zip(state.tensors(), saved):
                dst.copy_(src)

        def hip():
            restore()
            return I.track_update(state, *lists)

        def composed():
            restore()
            return I.track_update_reference(state, *lists)
        with torch.cuda.stream(s):
            a, b = hip(), [t.clone() for t in state.tensors()]
            c, d = composed(), [t.clone() for t in state.tensors()]
            s.synchronize()
        same = all(torch.equal(x, y) for x, y in zip(a, c)) and all(
            torch.equal(x, y) for x, y in zip(b[2:], d[2:])) and all(
            torch.allclose(x, y, rtol=0, atol=1e-3) for x, y in zip(b[:2], d[:2]))
        ids = a[0].cpu()
        what.update(rows_with_a_track=int((ids > 0).sum()), live_after=int((b[3] != 0).sum()),
                    next_id=int(b[6].item()), dropped=int(b[7].item()), hip_equals_torch=bool(same))
        t = {"hip": [], "torch": [], "restore": []}
        for _ in range(rounds):
            t["hip"].append(timeit(hip, s, iters))
            t["torch"].append(timeit(composed, s, 2))           # n steps of several launches: fewer calls per graph
            t["restore"].append(timeit(restore, s, iters))
        name = f"track_n{n}_t{T}"
        for k, vs in t.items():
            r[f"{name}_{k}_us"] = round(statistics.median(vs), 1)
        r[f"{name}_rounds_us"] = {k: [round(v, 1) for v in vs] for k, vs in t.items()}
        r[f"{name}_scene"] = what
    if not whole_gpu:
        return
    g = torch.Generator().manual_seed(2)
    small = torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8).cuda()
    large = torch.randint(0, 256, (2160, 3840, 3), generator=g, dtype=torch.uint8).cuda()
    with torch.cuda.stream(s), torch.no_grad():
        m = YolosSmall().cuda().eval()
        # thresholds under which the random model keeps rows, so that the tracker has work: its state grows over
        # the replays of the timed graph until every row continues a track
        tr_i, tr_t = Tracker(capacity=256, device="cuda"), Tracker(capacity=1024, device="cuda")
        it = max(2, iters // 5)
        t = {"detect_image": [], "track_image": [], "detect_tiled": [], "track_tiled": []}
        for _ in range(rounds):
            t["detect_image"].append(timeit(lambda: m.detect_image(small, 0.0), s, it))
            t["track_image"].append(timeit(lambda: m.track_image(small, tr_i, 0.0), s, it))
            t["detect_tiled"].append(timeit(lambda: m.detect_tiled(large, (2, 2), 0.2, 0.0), s, it))
            t["track_tiled"].append(timeit(lambda: m.track_tiled(large, tr_t, (2, 2), 0.2, 0.0), s, it))
        s.synchronize()
    for k, vs in t.items():
        r[f"{k}_thr0_ms"] = round(statistics.median(vs) / 1000.0, 3)
    r["track_model_rounds_ms"] = {k: [round(v / 1000.0, 3) for v in vs] for k, vs in t.items()}
    r["track_model_live"] = {"track_image": len(tr_i.tracks()), "track_tiled": len(tr_t.tracks())}


def overlay_scene(n: int, h: int, w: int, redact: bool = False):
    """``n`` rows with ids on a lattice over an ``h x w`` frame, as ``track_scene`` lays its tracks out: a box of 55 to
    80 % of its cell, labels 0..7; with ``redact`` the rows of labels 0 and 1 (a quarter) are filled."""
    g = torch.Generator().manual_seed(n + h)
    cols = int((n * w / h) ** 0.5) + 1
    rows = -(-n // cols)
    cw, ch = w / cols, h / rows
    k = torch.arange(n)
    x0, y0 = (k % cols) * cw + 0.1 * cw, (k // cols) * ch + 0.15 * ch
    size = 0.55 + 0.25 * torch.rand(n, 2, generator=g)
    boxes = torch.stack((x0, y0, x0 + size[:, 0] * cw, y0 + size[:, 1] * ch), dim=1).float()
    i32 = torch.int32
    lists = (torch.tensor([n], dtype=i32), 0.5 + 0.5 * torch.rand(n, generator=g), (k % 8).to(i32), boxes,
             (7 * k + 1).to(i32), torch.full((n,), 3, dtype=i32))
    modes = torch.tensor([2 if redact and label < 2 else 1 for label in range(8)], dtype=torch.uint8)
    return lists, modes


def overlay_rows(r, s, iters, rounds, whole_gpu):
    """The overlay (see the module docstring): ``overlay_*_hip_us`` against ``*_torch_us``, both with the restore of
    the frame from a saved copy that ``*_restore_us`` times alone; ``*_scene`` says what was painted."""
    import statistics

    from walkai_nos_amd.models.workload import surfaces
    from walkai_nos_amd.models.workload.overlay import Overlay
    from walkai_nos_amd.models.workload.processor import Nv12
    from walkai_nos_amd.models.workload.tracker import Tracker
    from walkai_nos_amd.models.workload.yolos import YolosSmall
    from walkai_nos_amd.ops import image as I
    g = torch.Generator().manual_seed(3)
    for name, n, h, w, fmt, redact in (("n100_1080p_nv12", 100, 1080, 1920, "nv12", False),
                                       ("n400_2160p_nv12", 400, 2160, 3840, "nv12", False),
                                       ("n400_2160p_rgb", 400, 2160, 3840, "rgb", False),
                                       ("n400_2160p_p010", 400, 2160, 3840, "p010", False),
                                       ("n400_2160p_nv12_redact", 400, 2160, 3840, "nv12", True)):
        if fmt == "rgb":
            buf = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).cuda()
            frame = buf
        else:
            pitch = -(-w * (2 if fmt == "p010" else 1) // 256) * 256
            buf = torch.randint(0, 256, (pitch * h * 3 // 2,), generator=g, dtype=torch.uint8).cuda()
            frame = Nv12.from_buffer(buf, h, w, pitch) if fmt == "nv12" else surfaces.from_buffer(fmt, buf, h, w, pitch)
        saved = buf.clone()
        lists, modes = overlay_scene(n, h, w, redact)
        lists, modes = [t.cuda() for t in lists], modes.cuda()
        thickness, scale = Overlay().sizes(h, w)
        codes = I.overlay_codes(I.overlay_palette(), (0, 0, 0), frame)
        kw = dict(thickness=thickness, scale=scale, modes=modes, min_hits=1, codes=codes)

        def restore():
            buf.copy_(saved)

        def hip():
            restore()
            return I.overlay(frame, *lists, **kw)

        def composed():
            restore()
            return I.overlay_reference(frame, *lists, **kw)
        with torch.cuda.stream(s):
            hip()
            a = buf.clone()
            composed()
            same = torch.equal(a, buf)
            surf = I.overlay_surface(frame)
            slot = I.overlay_slots(h, w, *lists, thickness, scale, modes, 1, 16)
            sb = 1 if fmt != "p010" else 2
            samples = sum(int((slot[::1 << vs, ::1 << hs] >= 0).sum()) for _, _, hs, vs in surf.samples)
            s.synchronize()
        t = {"hip": [], "torch": [], "restore": []}
        for _ in range(rounds):
            t["hip"].append(timeit(hip, s, iters))
            t["torch"].append(timeit(composed, s, 1, warm=1))       # n steps of many launches: one call per graph
            t["restore"].append(timeit(restore, s, iters))
        for k, vs in t.items():
            r[f"overlay_{name}_{k}_us"] = round(statistics.median(vs), 1)
        r[f"overlay_{name}_rounds_us"] = {k: [round(v, 1) for v in vs] for k, vs in t.items()}
        print(f"[kbench] overlay_{name}: hip {t['hip']} torch {t['torch']} us", file=sys.stderr, flush=True)
        kernel_us = max(statistics.median(t["hip"]) - statistics.median(t["restore"]), 1e-3)
        r[f"overlay_{name}_scene"] = {"rows": n, "frame": [h, w], "thickness": thickness, "scale": scale,
                                      "painted_samples": samples, "painted_bytes": samples * sb,
                                      "frame_bytes": int(buf.numel()), "hip_equals_torch": bool(same),
                                      "painted_bytes_per_kernel_us": round(samples * sb / kernel_us, 1)}
    if not whole_gpu:
        return
    small = torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8).cuda()
    large = torch.randint(0, 256, (2160, 3840, 3), generator=g, dtype=torch.uint8).cuda()
    small_out, large_out = torch.empty_like(small), torch.empty_like(large)
    with torch.cuda.stream(s), torch.no_grad():
        m = YolosSmall().cuda().eval()
        tr = [Tracker(capacity=c, device="cuda") for c in (256, 256, 1024, 1024)]
        ov = Overlay()
        it = max(2, iters // 5)
        t = {"track_image": [], "annotate_image": [], "track_tiled": [], "annotate_tiled": []}
        for _ in range(rounds):
            t["track_image"].append(timeit(lambda: m.track_image(small, tr[0], 0.0), s, it))
            t["annotate_image"].append(timeit(lambda: m.annotate_image(small, ov, 0.0, tr[1], small_out), s, it))
            t["track_tiled"].append(timeit(lambda: m.track_tiled(large, tr[2], (2, 2), 0.2, 0.0), s, it))
            t["annotate_tiled"].append(timeit(lambda: m.annotate_tiled(large, ov, (2, 2), 0.2, 0.0, tracker=tr[3],
                                                                       target=large_out), s, it))
        s.synchronize()
    for k, vs in t.items():
        r[f"overlay_{k}_thr0_ms"] = round(statistics.median(vs) / 1000.0, 3)
    r["overlay_model_rounds_ms"] = {k: [round(v / 1000.0, 3) for v in vs] for k, vs in t.items()}


def free_running(slots, seconds: float) -> int:
    """Every lane of every slot on its own thread: replay, wait, replay ... until the deadline
    (``bench_core.NodeBench._serve_loops``); returns the inferences completed."""
    import threading
    deadline = time.perf_counter() + seconds
    counts = []

    def run(slot, lane):
        K.set_slice_cus(lane.n_cus)
        K.set_slice_pin(slot.pin)
        done = 0
        with torch.no_grad(), torch.cuda.stream(lane.stream):
            while time.perf_counter() < deadline:
                st = torch.cuda.Event(enable_timing=True)
                st.record(lane.stream)
                if lane.graph is not None:
                    lane.graph.replay()
                else:
                    lane.out = slot.model(lane.x)
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(lane.stream)
                ev.synchronize()
                slot.latency_ms.append(st.elapsed_time(ev))
                done += 1
        counts.append(done)
    threads = [threading.Thread(target=run, args=(sl, lane), daemon=True) for sl in slots for lane in sl.lanes]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return sum(counts)


def model_bench(r, s, iters):
    """One whole YOLOS-small inference (batch 1) on this slice, graph-replayed."""
    from walkai_nos_amd.models.workload.yolos import DEMO_INPUT_HW, YolosSmall, demo_input
    with torch.cuda.stream(s):
        m = YolosSmall().cuda().eval()
        xin = demo_input(1, DEMO_INPUT_HW, "cuda")
    for mode in ("x3", "f32"):
        K.set_fp32_matmul(mode)
        with torch.no_grad():
            us = timeit(lambda: m(xin), s, iters)
        sfx = "" if mode == "x3" else "_f32"
        r[f"model{sfx}_ms"] = round(us / 1000.0, 3)
        r[f"model{sfx}_tflops"] = round(m.flops_per_inference() / us / 1e6, 2)
        r[f"model{sfx}_inf_per_s_per_gpu"] = round(1e6 / us * 256 / r["cus"], 1)
    K.set_fp32_matmul("x3")


def gemm_bench(r, x, h, w_qkv, w_o, w_1, w_2, b_ff, b_qkv, b_d, s, iters):
    lib = {"qkv": (x, w_qkv, b_qkv, None, 0, 2.0 * T * D * 3 * D),
           "proj": (x, w_o, b_d, x, G.EPI_RES, 2.0 * T * D * D),
           "fc1": (x, w_1, b_ff, None, G.EPI_GELU, 2.0 * T * D * FF),
           "fc2": (h, w_2, b_d, x, G.EPI_RES, 2.0 * T * FF * D)}
    for gname, (xa, wa, ba, ra, epi, fl) in lib.items():
        o = torch.empty(xa.shape[0], wa.shape[0], device="cuda")
        us = timeit(lambda: G._library(xa, wa, ba, ra, o, G.EPI_BIAS | epi), s, iters)
        r[f"gemm_{gname}_us"] = round(us, 1)
        r[f"gemm_{gname}_tflops"] = round(fl / us / 1e6, 2)
        # hand-written MFMA GEMM, every tile, same fused epilogue
        kw = {"bias": ba, "gelu": bool(epi & G.EPI_GELU), "residual": ra}
        for cfg in G.eligible(xa.shape[0], wa.shape[0], xa.shape[1]):
            us = timeit(lambda: G.gemm(xa, wa, tile=cfg, **kw), s, iters)
            tag = "x".join(map(str, G.TILES[cfg][:2])) + f"k{G.TILES[cfg][2]}" + ("sb" if cfg >= 7 else "")
            r[f"mfma_{gname}_{tag}_us"] = round(us, 1)
            r[f"mfma_{gname}_{tag}_tflops"] = round(fl / us / 1e6, 2)
        # x3 GEMM (fp32-accurate on the bf16 matrix cores), every tile; planes out where the model
        # feeds another x3 consumer (qkv, fc1), fp32 out where it feeds the residual stream
        xa3 = K.split3(xa)
        x3_out = gname in ("qkv", "fc1")
        for cfg in G.x3_eligible(wa.shape[0], wa.shape[1]):
            us = timeit(lambda: G.gemm_x3(xa3, wa, tile=cfg, out_f32=not x3_out, out_x3=x3_out, **kw), s, iters)
            bm, bn, nb, kind = G.X3_TILES[cfg]
            r[f"x3_{gname}_{bm}x{bn}{kind}b{nb}_us"] = round(us, 1)
            r[f"x3_{gname}_{bm}x{bn}{kind}b{nb}_tflops"] = round(fl / us / 1e6, 2)


if __name__ == "__main__":
    sys.exit(main())
