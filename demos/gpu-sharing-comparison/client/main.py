"""GPU-sharing comparison client (reference demo ``demos/gpu-sharing-comparison/client/main.py``).

Endless YOLOS-small object-detection inference, batch 1, on whatever slice of an MI355X this pod
was given (a compute partition, a CU-mask slice, or a time-sliced whole GPU). Each call is timed
into the Prometheus Summary ``inference_time_seconds`` served on :8000, which the comparison
dashboards scrape through a PodMonitor.

Weights: if ``YOLOS_WEIGHTS`` points at a local safetensors file of ``hustvl/yolos-small`` they are
loaded (safetensors only, nothing executable); otherwise the architecture runs with random-init
weights, which has identical cost. Input: an 800x1066 image (``YOLOS_IMAGE`` = path to a .npy
float32 CHW array, else a synthetic one of the same shape). ``YOLOS_IMAGE`` may also be a photo: a
uint8 HWC ``.npy`` or an image file (when PIL is installed). Each inference is then image in,
detections out (``YolosSmall.detect_image``: resize, normalise, model, score threshold
``YOLOS_THRESHOLD``, boxes in pixels of the photo), and the detections are printed with the timing.
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch
from prometheus_client import Summary, start_http_server

from walkai_nos_amd.models.workload.yolos import DEMO_INPUT_HW, YolosSmall, demo_input

INFERENCE_TIME = Summary("inference_time_seconds", "Time spent running one YOLOS-small inference")


def load_model(device: str) -> YolosSmall:
    m = YolosSmall()
    path = os.environ.get("YOLOS_WEIGHTS", "")
    if path:
        from safetensors.torch import load_file
        m.load_hf_state_dict(load_file(path))
    return m.to(device).eval()


def load_image(device: str) -> torch.Tensor:
    """A float32 ``[1, 3, H, W]`` tensor of normalised pixels, or a uint8 ``[h, w, 3]`` photo."""
    path = os.environ.get("YOLOS_IMAGE", "")
    if not path:
        return demo_input(1, DEMO_INPUT_HW, device)
    if path.endswith(".npy"):
        arr = np.load(path, allow_pickle=False)
        if arr.dtype == np.uint8 and arr.ndim == 3 and arr.shape[-1] == 3:
            return torch.from_numpy(arr).to(device)
        return torch.from_numpy(arr.astype(np.float32)).unsqueeze(0).to(device)
    try:
        from PIL import Image
    except ImportError as e:
        raise SystemExit(f"YOLOS_IMAGE={path}: an image file needs PIL (or pass a uint8 HWC .npy): {e}")
    return torch.from_numpy(np.array(Image.open(path).convert("RGB"))).to(device)


def main() -> None:
    device = "cuda" if torch.cuda.is_available() else "cpu"
    start_http_server(int(os.environ.get("METRICS_PORT", "8000")))
    model, x = load_model(device), load_image(device)
    photo = x.dtype == torch.uint8
    threshold = float(os.environ.get("YOLOS_THRESHOLD", "0.5"))
    n = 0
    while True:
        t0 = time.perf_counter()
        with torch.no_grad():
            out = model.detect_image(x, threshold) if photo else model(x)
        if device == "cuda":
            torch.cuda.synchronize()
        INFERENCE_TIME.observe(time.perf_counter() - t0)
        n += 1
        if n % 100 == 0:
            print(f"{n} inferences, last {1000 * (time.perf_counter() - t0):.1f} ms", flush=True)
            if photo:
                det = model.processor.results(out["count"], out["scores"], out["labels"], out["boxes"])[0]
                for s, l, b in zip(det["scores"].tolist(), det["labels"].tolist(), det["boxes"].tolist()):
                    print(f"  label {l} at ({b[0]:.0f}, {b[1]:.0f}, {b[2]:.0f}, {b[3]:.0f}), {s:.2f}", flush=True)


if __name__ == "__main__":
    main()
