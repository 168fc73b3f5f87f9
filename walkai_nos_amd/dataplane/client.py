"""One pod's inference process (the reference demo client, ref
``demos/gpu-sharing-comparison/client/main.py:19-35``: YOLOS-small, batch 1, one image, timed
inference in an endless loop), driven by :mod:`walkai_nos_amd.dataplane.procs`.

The process gets exactly what kubelet gives a container: ``HSA_CU_MASK`` (its CU set, applied by
the HSA runtime to every queue of the process), ``NOS_HBM_LIMIT_BYTES`` + ``LD_PRELOAD`` of the
HBM-budget shim, ``NOS_SLICE_IDS``.  It loads the model, warms up (and captures a HIP graph of one
inference), then prints ``READY`` and waits on stdin for ``GO <epoch>``; from that wall-clock
instant it runs one inference at a time — replay, synchronize, record the wall latency, exactly
the reference's loop — until ``epoch + seconds``.  A workgroup census (which physical CUs this
process's kernels run on) is taken while every pod is busy.  It prints one JSON line and exits.

    python -m walkai_nos_amd.dataplane.client --seconds 10 [--no-graph] [--census]

``--end-to-end`` makes one inference what a pod that is handed a photo does: a uint8 image (seeded,
synthetic, ``--image-hw``) through the fused preprocess, the model and the detections kernel
(``YolosSmall.detect_image``), all inside the warm-up and the captured graph; the JSON line then
carries ``"end_to_end": true`` and ``"detections"``, the number of boxes above ``--threshold``.
``--pixel-format nv12`` hands it what a video decoder does instead: one NV12 surface (Y rows, then UV
rows, ``--pitch`` bytes apart), converted inside the same preprocess launch. ``nv21`` is that with V first;
``i420`` / ``yv12`` a software decoder's planar surface (Y rows at ``--pitch``, then the two chroma planes at
half of it); ``bgr``, ``rgba`` and ``bgra`` packed pixels as OpenCV or a compositor hands them out. ``--pitch``
applies to every format (for the packed ones and ``rgb`` it is the bytes between rows of a padded buffer).
The names of ``models/workload/surfaces.py`` — ``i422``, ``nv16``, ``i444``, ``nv24``, ``yuy2`` / ``uyvy``, a 10-bit
decoder's ``p010`` / ``p210`` / ``p410``, ``i010`` (``yuv420p10le``) and their 12-bit forms — go the same way, and
``--matrix bt601|bt709|bt2020`` and ``--full-range`` say how any YUV format's codes are read, and ``--transfer
pq|hlg`` (with ``--peak-nits``) that a 10- or 12-bit format's codes are HDR and are tone-mapped to SDR in that launch.
``--tiles R,C`` runs a large frame as ``R x C`` overlapping tiles in one batch (``YolosSmall.detect_tiled``;
``--tile-overlap``, ``--match ios|iou``, ``--match-threshold``): the JSON line then carries ``"tiles"``, the tile count,
and ``"detections"`` counts the merged boxes. With a YUV ``--pixel-format`` (and ``--transfer``, ``--peak-nits``) the
tiles are staged straight from the surface's planes: no flag, the frame's own ``tile_planes``.
``--track`` gives every detection a stable id across the frames (``YolosSmall.track_image`` / ``track_tiled``, one more
launch inside the captured graph, whose replays advance the tracker; ``--track-iou``, ``--track-max-age``,
``--track-min-hits``, ``--track-capacity``, ``--track-motion``). The tracker is reset after the warm-ups and again after
the capture, so the timed loop starts at frame 0; the JSON line then carries a ``"track"`` block: the live tracks (and
those of them seen in ``--track-min-hits`` frames), the ids issued, the births dropped for lack of a slot, the frames.
``--annotate`` draws the detections into the frame (``YolosSmall.annotate_image`` / ``annotate_tiled``, one more launch
inside the captured graph; with ``--track`` the tags are the ids): boxes ``--annotate-thickness`` thick, tags of glyph
dots ``--annotate-scale`` pixels large or none with ``--no-tags``, the labels of ``--redact L1,L2,...`` filled instead.
The client builds a second surface of the same layout over a second buffer; inside the graph the source buffer is
copied there and painted there, so the synthetic frame stays the same from replay to replay. The JSON line then carries
``"annotate": {"changed_bytes": ...}``, the bytes of the second buffer that differ from the source, counted once on the
host after the loop. It is refused with ``--transfer pq|hlg``: an SDR colour has no code on such a surface.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time
from typing import Any, Dict, List


def _stats(v: List[float]) -> Dict[str, float]:
    if not v:
        return {"n": 0}
    s = sorted(v)
    return {"n": len(s), "mean": round(sum(s) / len(s), 3), "p50": round(s[len(s) // 2], 3),
            "p99": round(s[min(len(s) - 1, int(0.99 * len(s)))], 3), "max": round(s[-1], 3)}


def _census() -> Dict[str, Any]:
    from ..ops import probe as P
    pl = P.census(n_wg=4096, spin=4000)
    cus = sorted({(p["xcc"], p["se"], p["sh"], p["cu"]) for p in pl})
    return {"cus": len(cus), "xcds": sorted({c[0] for c in cus}), "ids": ["%d.%d.%d.%d" % c for c in cus]}


def _shim() -> Dict[str, Any]:
    try:
        lib = ctypes.CDLL(None)
        lib.nos_hbm_shim_loaded.restype = ctypes.c_int
        for f in ("nos_hbm_limit_bytes", "nos_hbm_peak_bytes", "nos_hbm_live_bytes"):
            getattr(lib, f).restype = ctypes.c_size_t
        if not lib.nos_hbm_shim_loaded():
            return {"loaded": False}
        return {"loaded": True, "limit_bytes": int(lib.nos_hbm_limit_bytes()),
                "peak_bytes": int(lib.nos_hbm_peak_bytes()), "live_bytes": int(lib.nos_hbm_live_bytes())}
    except (AttributeError, OSError):
        return {"loaded": False}


#: the names of models/workload/surfaces.py's FORMATS (spelled out: this module imports torch only after its arguments)
SURFACES = ("i422", "yv16", "i444", "yv24", "nv16", "nv61", "nv24", "nv42", "yuy2", "uyvy", "yvyu",
            "p010", "p012", "p210", "p410", "i010", "i012", "i210", "i410")


#: those of them with 10- or 12-bit samples: the ones that take --transfer pq|hlg
DEEP = tuple(n for n in SURFACES if n[1:] in ("010", "012", "210", "410"))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser("nos pod client")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--census", action="store_true")
    ap.add_argument("--hw", default="800,1066")
    ap.add_argument("--streams", type=int, default=int(os.environ.get("NOS_POD_STREAMS", "1")),
                    help="HIP streams the inference loop rotates over (one inference at a time)")
    ap.add_argument("--end-to-end", action="store_true",
                    help="time image in, detections out (uint8 image -> preprocess -> model -> post-process)")
    ap.add_argument("--image-hw", default="480,640", help="--end-to-end: the synthetic source image's height,width")
    ap.add_argument("--size", default="800,1333", help="--end-to-end: the processor's shortest,longest edge")
    ap.add_argument("--threshold", type=float, default=0.5, help="--end-to-end: detection score threshold")
    ap.add_argument("--pixel-format", choices=("rgb", "bgr", "rgba", "bgra", "nv12", "nv21", "i420", "yv12")
                    + tuple(SURFACES), default="rgb",
                    help="--end-to-end: packed pixels, a decoder's 4:2:0 surface (even height), or a 4:2:2 / 4:4:4 / "
                         "packed 4:2:2 / 10- or 12-bit surface (models/workload/surfaces.py)")
    ap.add_argument("--pitch", type=int, default=0,
                    help="--end-to-end: bytes between rows of the surface (default: a luma row's bytes rounded up to "
                         "256 for the YUV formats, rows side by side for the packed RGB ones)")
    ap.add_argument("--matrix", choices=("bt601", "bt709", "bt2020"), default="bt601",
                    help="--end-to-end: the YUV formats' colour matrix (bt2020 with the surfaces.py formats only)")
    ap.add_argument("--full-range", action="store_true", help="--end-to-end: full-range YUV codes (default: limited)")
    ap.add_argument("--transfer", choices=("sdr", "pq", "hlg"), default="sdr",
                    help="--end-to-end: the codes' transfer function; pq and hlg (10- and 12-bit formats only) are "
                         "tone-mapped to SDR")
    ap.add_argument("--peak-nits", type=float, default=1000.0,
                    help="--end-to-end: with --transfer pq|hlg, the luminance that is mapped to SDR white (above 203)")
    ap.add_argument("--tiles", default="", help="--end-to-end: R,C overlapping tiles of the frame, run as one batch and merged")
    ap.add_argument("--tile-overlap", type=float, default=0.2, help="--tiles: the overlap of neighbouring tiles, of a tile")
    ap.add_argument("--match", choices=("ios", "iou"), default="ios",
                    help="--tiles: how two tiles' boxes are compared: intersection over the smaller area, or over the union")
    ap.add_argument("--match-threshold", type=float, default=0.5,
                    help="--tiles: a box is dropped when a kept box of the same label from another tile overlaps it by more")
    ap.add_argument("--track", action="store_true", help="--end-to-end: stable ids across frames (a tracker in the graph)")
    ap.add_argument("--track-iou", type=float, default=0.3, help="--track: the IoU a detection must exceed to continue a track")
    ap.add_argument("--track-max-age", type=int, default=30, help="--track: frames a track survives unmatched")
    ap.add_argument("--track-min-hits", type=int, default=1, help="--track: frames a track is seen in before it is counted as confirmed")
    ap.add_argument("--track-capacity", type=int, default=256, help="--track: slots of the tracker (1..1024 run in HIP)")
    ap.add_argument("--track-motion", choices=("constant", "none"), default="constant",
                    help="--track: compare a track one frame along its velocity, or where it was")
    ap.add_argument("--annotate", action="store_true",
                    help="--end-to-end: draw the detections into a copy of the frame (an overlay launch in the graph)")
    ap.add_argument("--annotate-thickness", type=int, default=None, help="--annotate: a box outline's pixels (default: twice the scale)")
    ap.add_argument("--annotate-scale", type=int, default=None,
                    help="--annotate: the pixels of a glyph's dot (default: the frame's shorter side / 360, at least 1)")
    ap.add_argument("--redact", default="", help="--annotate: L1,L2,... labels that are filled, not outlined")
    ap.add_argument("--no-tags", action="store_true", help="--annotate: boxes without id tags")
    args = ap.parse_args(argv)
    redact = ()
    if args.annotate:
        if not args.end_to_end:
            ap.error("--annotate takes --end-to-end")
        if args.transfer != "sdr":
            ap.error(f"--annotate draws SDR colours: it is not offered with --transfer {args.transfer}")
        if args.annotate_thickness is not None and args.annotate_thickness < 1:
            ap.error(f"--annotate-thickness {args.annotate_thickness} is not a number of pixels from 1 up")
        if args.annotate_scale is not None and args.annotate_scale < 1:
            ap.error(f"--annotate-scale {args.annotate_scale} is not a number of pixels from 1 up (--no-tags draws none)")
        try:
            redact = tuple(int(v) for v in args.redact.split(",")) if args.redact else ()
        except ValueError:
            redact = (-1,)
        if any(not 0 <= v < 91 for v in redact):
            ap.error(f"--redact {args.redact!r} is not L1,L2,... with labels in 0..90")
    elif args.annotate_thickness is not None or args.annotate_scale is not None or args.redact or args.no_tags:
        ap.error("--annotate-thickness, --annotate-scale, --redact and --no-tags take --annotate")
    if args.track:
        if not args.end_to_end:
            ap.error("--track takes --end-to-end")
        if not args.track_iou >= 0.0:
            ap.error(f"--track-iou {args.track_iou!r} is not a number from 0 up")
        if args.track_max_age < 0:
            ap.error(f"--track-max-age {args.track_max_age} is negative")
        if args.track_min_hits < 1:
            ap.error(f"--track-min-hits {args.track_min_hits} is not a number of frames from 1 up")
        if not 1 <= args.track_capacity <= 1024:
            ap.error(f"--track-capacity {args.track_capacity} is not in 1..1024")
    tiles = None
    if args.tiles:
        if not args.end_to_end:
            ap.error("--tiles takes --end-to-end")
        try:
            tiles = tuple(int(v) for v in args.tiles.split(","))
        except ValueError:
            tiles = ()
        if len(tiles) != 2 or min(tiles) < 1:
            ap.error(f"--tiles {args.tiles!r} is not R,C with R, C >= 1")
    if args.transfer != "sdr" and args.pixel_format not in DEEP:
        ap.error(f"--transfer {args.transfer} takes a 10- or 12-bit --pixel-format ({', '.join(DEEP)}), "
                 f"not {args.pixel_format}")
    if not args.peak_nits > 203.0:
        ap.error(f"--peak-nits {args.peak_nits:g} must exceed 203, the reference white")
    t_boot = time.perf_counter()
    import torch

    from ..models.workload.yolos import YolosSmall, demo_input
    from ..ops import kernels as K
    K.set_backend("hip")
    hw = tuple(int(x) for x in args.hw.split(","))
    dev = "cuda:0"
    model = YolosSmall().to(dev).eval()
    seed = int(os.environ.get("NOS_POD_SEED", "0"))
    tracker = None
    if args.end_to_end:
        from ..models.workload.processor import Nv12, Packed, YolosProcessor, Yuv420p
        ih, iw = (int(v) for v in args.image_hw.split(","))
        shortest, longest = (int(v) for v in args.size.split(","))
        model.processor = YolosProcessor(shortest, longest, patch=model.c.patch_size)
        gen = torch.Generator().manual_seed(seed)
        fmt = args.pixel_format
        if fmt in SURFACES:
            from ..models.workload import surfaces
            kind, sub, depth = surfaces.FORMATS[fmt][:3]
            row = 4 * ((iw + 1) // 2) if kind == "packed" else iw * (1 if depth == 8 else 2)
            pitch = args.pitch or -(-row // 256) * 256
            if pitch < row:
                ap.error(f"--pitch {pitch} is smaller than a row of {iw} {fmt} pixels ({row} bytes)")
            # luma rows, then at most twice as many bytes of chroma (4:4:4)
            buf = torch.randint(0, 256, (3 * pitch * ih,), generator=gen, dtype=torch.uint8).to(dev)

            def surface(b):
                return surfaces.from_buffer(fmt, b, ih, iw, pitch, matrix=args.matrix, full_range=args.full_range,
                                            transfer=args.transfer, peak_nits=args.peak_nits)
        elif fmt in ("nv12", "nv21", "i420", "yv12"):
            if args.matrix == "bt2020":
                ap.error(f"--matrix bt2020 is not offered for {fmt}")
            pitch = args.pitch or -(-iw // 256) * 256
            buf = torch.randint(0, 256, (pitch * (ih + ih // 2),), generator=gen, dtype=torch.uint8).to(dev)

            def surface(b):
                if fmt in ("nv12", "nv21"):
                    return Nv12.from_buffer(b, ih, iw, pitch, args.matrix, args.full_range, vu=fmt == "nv21")
                return Yuv420p.from_buffer(b, ih, iw, pitch, order=fmt, matrix=args.matrix, full_range=args.full_range)
        elif fmt == "rgb" and not args.pitch:
            buf = torch.randint(0, 256, (ih, iw, 3), generator=gen, dtype=torch.uint8).to(dev)

            def surface(b):
                return b
        else:
            C = len(fmt)
            pitch = args.pitch or iw * C
            if pitch < iw * C:
                ap.error(f"--pitch {pitch} is smaller than a row of {iw} {fmt} pixels")
            buf = torch.randint(0, 256, (ih * pitch,), generator=gen, dtype=torch.uint8).to(dev)

            def surface(b):
                return Packed(b.as_strided((ih, iw, C), (pitch, C, 1)), fmt)
        img = surface(buf)      # the frame over its buffer, in place
        hw = model.processor.size((ih, iw))
        if tiles is not None:
            th, tw, origins = model.processor.tile_plan((ih, iw), tiles, args.tile_overlap, model.c.num_detection_tokens)
            hw = model.processor.size((th, tw))
        if args.track:
            from ..models.workload.tracker import Tracker
            tracker = Tracker(args.track_capacity, args.track_iou, args.track_max_age, motion=args.track_motion,
                              min_hits=args.track_min_hits, device=dev)
        overlay = painted = None
        if args.annotate:
            from ..models.workload.overlay import Overlay
            overlay = Overlay(thickness=args.annotate_thickness, scale=args.annotate_scale, tags=not args.no_tags,
                              redact=redact, min_hits=args.track_min_hits if args.track else 1,
                              num_labels=model.c.num_labels)
            painted = torch.empty_like(buf)     # a second surface of the same layout over a second buffer
            target = surface(painted)

        def infer():
            if overlay is not None:
                painted.copy_(buf)
                if tiles is not None:
                    return model.annotate_tiled(img, overlay, tiles, args.tile_overlap, args.threshold, args.match,
                                                args.match_threshold, tracker, target)
                return model.annotate_image(img, overlay, args.threshold, tracker, target)
            if tracker is not None:
                if tiles is not None:
                    return model.track_tiled(img, tracker, tiles, args.tile_overlap, args.threshold, args.match,
                                             args.match_threshold)
                return model.track_image(img, tracker, args.threshold)
            if tiles is not None:
                return model.detect_tiled(img, tiles, args.tile_overlap, args.threshold, args.match, args.match_threshold)
            return model.detect_image(img, args.threshold)
    else:
        x = demo_input(1, hw, dev, seed=seed)

        def infer():
            return model(x)
    streams = [torch.cuda.Stream() for _ in range(max(1, args.streams))]
    if os.environ.get("NOS_POD_EAGER_QUEUES", "0") == "1":
        # touch every stream back to back before anything else: HIP creates the process's hardware
        # queues at first use, so they are created together (consecutive queues of one process)
        for st in streams:
            with torch.cuda.stream(st):
                torch.zeros(1, device=dev).add_(1)
        torch.cuda.synchronize()
    stream = streams[0]
    with torch.no_grad(), torch.cuda.stream(stream):
        for _ in range(2):
            res = infer()
        if tracker is not None:
            tracker.reset()     # the warm-ups were no frames of the stream
    stream.synchronize()
    graph = None
    if not args.no_graph:
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph, stream=stream):
            res = infer()
        if tracker is not None:
            with torch.cuda.stream(stream):
                tracker.reset()     # nor was the capture, where the launch may have run
        stream.synchronize()
    out: Dict[str, Any] = {"pid": os.getpid(), "slice_ids": os.environ.get("NOS_SLICE_IDS", ""),
                           "hsa_cu_mask": os.environ.get("HSA_CU_MASK", ""), "slice_cus": K.slice_cus(),
                           "boot_s": round(time.perf_counter() - t_boot, 2), "streams": len(streams),
                           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "")}
    print("READY", flush=True)
    line = sys.stdin.readline().split()
    if not line or line[0] != "GO":
        return 3
    start = float(line[1])
    end = start + args.seconds
    while time.time() < start:
        time.sleep(0.0005)
    lat: List[float] = []
    census_at = start + 0.25 * args.seconds if args.census else None
    census = None
    k = 0
    with torch.no_grad():
        while True:
            now = time.time()
            if now >= end:
                break
            if census_at is not None and now >= census_at:
                census = _census()  # every other pod is mid-loop now
                census_at = None
            s = streams[k % len(streams)]  # one inference at a time, rotated over the process's queues
            k += 1
            t0 = time.perf_counter()
            with torch.cuda.stream(s):
                if graph is not None:
                    graph.replay()
                else:
                    res = infer()
            s.synchronize()
            lat.append(1e3 * (time.perf_counter() - t0))
    out["window_s"] = round(time.time() - start, 3)
    out["inferences"] = len(lat)
    out["latency_ms"] = _stats(lat)
    if args.end_to_end:
        out["end_to_end"] = True
        out["input_hw"] = list(hw)
        out["pixel_format"] = args.pixel_format
        out["transfer"] = args.transfer
        if tiles is not None:
            out["tiles"] = len(origins)
            out["tile_hw"] = [th, tw]
        out["detections"] = int(res["count"].sum().item())   # of the last inference
        if tracker is not None:
            live = tracker.tracks()
            out["track"] = {"live": len(live), "confirmed": sum(1 for t in live if t["hits"] >= tracker.min_hits),
                            "ids_issued": int(tracker.state.next_id.item()) - 1,
                            "dropped": int(tracker.state.dropped.item()), "frames": len(lat),
                            "capacity": tracker.capacity, "motion": args.track_motion}
        if overlay is not None:
            out["annotate"] = {"changed_bytes": int((painted != buf).sum().item())}
    if census is not None:
        out["census"] = census
    out["hbm"] = _shim()
    out["torch_max_reserved_bytes"] = int(torch.cuda.max_memory_reserved())
    print(json.dumps(out), flush=True)
    del graph
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
