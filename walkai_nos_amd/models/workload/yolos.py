"""YOLOS-small: the fractional-GPU benchmark workload.

The reference's only published performance numbers come from its GPU-sharing demo, in which every
Pod runs ``hustvl/yolos-small`` inference at batch 1 on one COCO image in a loop
(``demos/gpu-sharing-comparison/client/main.py:6-35``).  This module is an
independent implementation of that architecture (ViT-S/16 encoder with 100 detection tokens and
DETR-style MLP heads) built for the MI355X inference path:

* fp32 end to end (the reference demo runs fp32 PyTorch; no precision is given up): on the GPU every
  product runs in the x3 format — fp32 operands split exactly into three bf16 planes, six bf16
  MFMAs per block, fp32-accurate (``ops/kernels.py: set_fp32_matmul``); ``f32`` mode uses the
  f32-input MFMA instead;
* the interpolated position embeddings are computed once per input resolution and cached (the
  upstream implementation re-interpolates on every forward);
* the hot ops dispatch to hand-written HIP kernels (:mod:`walkai_nos_amd.ops.kernels`) on the GPU:
  LayerNorm that emits x3 planes, x3 GEMMs with bias / exact GELU / residuals fused into the store
  (the QKV projection leaves as fp32, which the x3 flash attention splits in-kernel), and the
  stream-K x3 flash attention; the detection heads (100 tokens) stay on ``torch`` / hipBLASLt;
* ``encode_image`` / ``detect_image`` take a uint8 photo instead of ready pixels: the processor's
  resize and normalisation fused with the patch GEMM's x3 split, and the post-process, one HIP
  launch each (:mod:`walkai_nos_amd.ops.image`, :mod:`.processor`);
* ``detect_tiled`` runs a frame too large for one input as ``R x C`` overlapping tiles in one batch — one tile-staging
  launch, one patch GEMM, the fused heads on all ``B x nd`` rows — and merges the tiles' detections in frame pixels by
  one more launch (``ops.image.tiled_patch_planes`` / ``merge_detections``), still without a host synchronisation; a
  YUV frame's tiles are staged straight from its planes (``Frame.tile_planes``), not from its ``rgb()``;
* the last block runs on the detection rows only ("detection tail"). ``detect`` reads nothing but
  the last ``nd`` = 100 rows, and a row of a block's output depends on the other rows only through K
  and V: so in the last block the attention queries, the projection, LN2, fc1, GELU and fc2 of the
  class/patch rows (3301 of 3401 at the demo's size) feed nothing and are skipped —
  ``forward`` / ``detect_image`` go through ``encode_detection``: the QKV GEMM on every row, the x3
  attention with a query window (``q0 = T - nd``, ``Tq = nd``), then the three GEMMs at M = nd. The
  Q third of that QKV GEMM is still computed for the pruned rows (about 9 us on the whole GPU; left
  for later). The rule is one of shapes only: the tail is taken when it at least halves the block's
  32-row query tiles, ``2*ceil(nd/32) <= ceil(T/32)`` (taken at T = 3401 and 257, not at T <= 224);
  ``NOS_DET_TAIL=0/1`` or ``set_detection_tail`` override it. Where it is taken, ``forward`` equals
  ``detect(encode(x))`` to fp32 rounding, not bit for bit (the lazy softmax rescale is decided per
  32-row tile, and the stream-K split points and tuned tiles follow the shape); ``encode`` /
  ``encode_image`` keep returning every row. Measured: ``docs/benchmark.md``, "Round 7";
* ``load_hf_state_dict`` maps a ``transformers`` ``YolosForObjectDetection`` state dict onto this
  module, which is how numerical parity is tested
  (``tests/test_infra.py::test_yolos_matches_transformers_reference``) — there is no network, so
  weights are random-init of the same architecture.

Config (hustvl/yolos-small): hidden 384, 12 layers, 6 heads, MLP 1536, patch 16, 100 detection
tokens, pre-training image size 800x1333, 91 COCO labels (+1 "no object").  The demo's 640x480
image is resized by the YOLOS processor to 800x1066 (shortest edge 800) -> 50x66 patches ->
3401 tokens.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ...ops import image as I
from ...ops import kernels as K
from ...ops.graph_cache import GraphCache
from .processor import YolosProcessor


@dataclass
class YolosConfig:
    hidden_size: int = 384
    num_layers: int = 12
    num_heads: int = 6
    intermediate_size: int = 1536
    patch_size: int = 16
    num_channels: int = 3
    num_detection_tokens: int = 100
    image_size: Tuple[int, int] = (800, 1333)
    num_labels: int = 91
    layer_norm_eps: float = 1e-12
    use_mid_position_embeddings: bool = False

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_heads


#: eagerly used input sizes whose position embeddings, token template and target sizes stay cached
#: (sizes used under graph capture are kept besides): with mid position embeddings one size is 12
#: tensors of T x 384 fp32, 63 MB at the demo's 3401 tokens, so 4 bound a server that sees every size
#: eagerly to about 250 MB, while a handful of sizes in rotation never re-interpolates
CACHED_SIZES = 4

#: the demo's input after YolosImageProcessor (640x480 COCO image -> shortest edge 800)
DEMO_INPUT_HW = (800, 1066)


_det_tail: Optional[bool] = None


def set_detection_tail(on: Optional[bool]) -> None:
    """Force the last block onto the detection rows only (True) or onto every row (False); None:
    ``NOS_DET_TAIL`` (``0`` / ``1``), else the shape rule of :func:`detection_tail_rule`. For A/B runs
    and for tests at small T; read at every forward."""
    global _det_tail
    _det_tail = on


def detection_tail_rule(T: int, nd: int) -> bool:
    """The last block runs on the ``nd`` detection rows when that at least halves its 32-row query
    tiles. Below that there is one query group and one or two GEMM row tiles either way."""
    return 2 * ((nd + 31) // 32) <= (T + 31) // 32


def detection_tail(T: int, nd: int) -> bool:
    """:func:`detection_tail_rule` unless overridden (:func:`set_detection_tail`, ``NOS_DET_TAIL``)."""
    if _det_tail is not None:
        return _det_tail
    env = os.environ.get("NOS_DET_TAIL", "").strip()
    if env in ("0", "1"):
        return env == "1"
    return detection_tail_rule(T, nd)


class _Block(nn.Module):
    def __init__(self, c: YolosConfig):
        super().__init__()
        d, f = c.hidden_size, c.intermediate_size
        self.c = c
        self.ln1 = nn.LayerNorm(d, eps=c.layer_norm_eps)
        self.qkv = nn.Linear(d, 3 * d)            # fused q|k|v projection
        self.proj = nn.Linear(d, d)
        self.ln2 = nn.LayerNorm(d, eps=c.layer_norm_eps)
        self.fc1 = nn.Linear(d, f)
        self.fc2 = nn.Linear(f, d)

    def attention_x3(self, h3: torch.Tensor, q0: int = 0, q_rows: Optional[int] = None) -> torch.Tensor:
        """QKV GEMM + attention on LN1(x) as planes; the output as planes, of every row or of the
        rows ``q0 .. q0+q_rows-1``. QKV leaves the GEMM as fp32 (4 B per element; the attention splits
        it in-kernel) or as planes (:func:`K.attention_input_f32`)."""
        H, Dh = self.c.num_heads, self.c.head_dim
        if K.attention_input_f32():
            qkv = K.linear_x3(h3, self.qkv.weight, self.qkv.bias)
            return K.attention_qkv_x3f(qkv, H, Dh, 1.0 / math.sqrt(Dh), q0=q0, q_rows=q_rows)
        qkv3 = K.linear_x3(h3, self.qkv.weight, self.qkv.bias, out_x3=True)
        return K.attention_qkv_x3(qkv3, H, Dh, 1.0 / math.sqrt(Dh), q0=q0, q_rows=q_rows)

    def forward_x3(self, x: torch.Tensor, mid: Optional[torch.Tensor], h3: Optional[torch.Tensor],
                   next_ln: Optional[nn.LayerNorm]) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """The x3 path with the LayerNorms folded into the producing step: ``h3`` is LN1(x) as planes
        when the previous block already made it; the projection step returns x and LN2(x), the fc2
        step x and ``next_ln``(x) (the next block's LN1) — each either the fused-epilogue GEMM + a
        LayerNorm kernel or a split-K GEMM + one combine-and-LayerNorm kernel, whichever is faster
        on the slice (``ops.gemm.linear_residual_ln_x3``)."""
        H, Dh = self.c.num_heads, self.c.head_dim
        eps = self.c.layer_norm_eps
        if h3 is None:
            h3 = K.layernorm_x3(x, self.ln1.weight, self.ln1.bias, eps)
        if K.attention_input_f32() and K.attn_proj_fusable(H, Dh):
            # attention partials -> one merge + projection + residual + LN2 kernel
            qkv = K.linear_x3(h3, self.qkv.weight, self.qkv.bias)
            x, h3 = K.attention_proj_ln_x3f(qkv, H, Dh, 1.0 / math.sqrt(Dh), self.proj.weight, self.proj.bias,
                                            x, (self.ln2.weight, self.ln2.bias, eps))
        else:
            x, h3 = K.linear_residual_ln_x3(self.attention_x3(h3), self.proj.weight, self.proj.bias, x,
                                            ln=(self.ln2.weight, self.ln2.bias, eps))
        f3 = K.linear_x3(h3, self.fc1.weight, self.fc1.bias, gelu=True, out_x3=True)
        nl = (next_ln.weight, next_ln.bias, next_ln.eps) if next_ln is not None else None
        return K.linear_residual_ln_x3(f3, self.fc2.weight, self.fc2.bias, x, residual2=mid, ln=nl)

    def tail_supported(self, x: torch.Tensor) -> bool:
        """The attention that would run on ``x`` takes a query window: the reference math (CPU,
        ``torch`` backend) and the pipelined x3 kernels do; the fused attention + projection kernel
        (``NOS_ATTN_PROJ_FUSED=1``), the block-at-a-time x3 kernel and the f32-MFMA attention do not."""
        if K.x3_active(x):
            return K.attention_x3_windowed() and not (K.attention_input_f32()
                                                      and K.attn_proj_fusable(self.c.num_heads, self.c.head_dim))
        return not (x.is_cuda and K.get_backend() == "hip")

    def forward_tail(self, x: torch.Tensor, h3: Optional[torch.Tensor], nd: int) -> torch.Tensor:
        """The block for a caller that reads only the last ``nd`` rows: ``[B, nd, D]``, the same rows
        :meth:`forward` / :meth:`forward_x3` give to fp32 rounding. K and V need every row, so the QKV
        GEMM runs on all of ``x``; the attention takes the last ``nd`` rows as its queries, and the
        projection, LN2, fc1 + GELU and fc2 run on those rows alone (``h3``: LN1(x) as planes when
        the previous block made it, as for :meth:`forward_x3`)."""
        T = x.shape[1]
        H, Dh = self.c.num_heads, self.c.head_dim
        eps, scale = self.c.layer_norm_eps, 1.0 / math.sqrt(self.c.head_dim)
        xd = x[:, T - nd:].contiguous()   # a view for B = 1
        if K.x3_active(x):
            if h3 is None:
                h3 = K.layernorm_x3(x, self.ln1.weight, self.ln1.bias, eps)
            o3 = self.attention_x3(h3, q0=T - nd, q_rows=nd)
            xd, h3 = K.linear_residual_ln_x3(o3, self.proj.weight, self.proj.bias, xd,
                                             ln=(self.ln2.weight, self.ln2.bias, eps))
            f3 = K.linear_x3(h3, self.fc1.weight, self.fc1.bias, gelu=True, out_x3=True)
            return K.linear_residual_ln_x3(f3, self.fc2.weight, self.fc2.bias, xd, ln=None)[0]
        h = K.layernorm(x, self.ln1.weight, self.ln1.bias, eps)
        qkv = K.linear(h, self.qkv.weight, self.qkv.bias)
        o = K.attention_ref(qkv, H, Dh, scale, T - nd, nd)                  # [B, nd, D]
        xd = K.linear_residual(o, self.proj.weight, self.proj.bias, xd)
        h = K.layernorm(xd, self.ln2.weight, self.ln2.bias, eps)
        h = K.linear_gelu(h, self.fc1.weight, self.fc1.bias)
        return K.linear_residual(h, self.fc2.weight, self.fc2.bias, xd)

    def forward(self, x: torch.Tensor, mid: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, T, D = x.shape
        H, Dh = self.c.num_heads, self.c.head_dim
        if K.x3_active(x):
            # every fp32 product on the bf16 matrix cores in x3 form: activations leave their
            # producer as three exact bf16 planes; the residual stream stays fp32
            h3 = K.layernorm_x3(x, self.ln1.weight, self.ln1.bias, self.c.layer_norm_eps)
            o3 = self.attention_x3(h3)
            x = K.linear_x3(o3, self.proj.weight, self.proj.bias, residual=x)
            h3 = K.layernorm_x3(x, self.ln2.weight, self.ln2.bias, self.c.layer_norm_eps)
            f3 = K.linear_x3(h3, self.fc1.weight, self.fc1.bias, gelu=True, out_x3=True)
            return K.linear_x3(f3, self.fc2.weight, self.fc2.bias, residual=x, residual2=mid)
        h = K.layernorm(x, self.ln1.weight, self.ln1.bias, self.c.layer_norm_eps)
        qkv = K.linear(h, self.qkv.weight, self.qkv.bias)                  # [B, T, 3D]
        o = K.attention_qkv(qkv, H, Dh, 1.0 / math.sqrt(Dh))               # [B, T, D]
        x = K.linear_residual(o, self.proj.weight, self.proj.bias, x)      # x + o @ Wp^T + bp
        h = K.layernorm(x, self.ln2.weight, self.ln2.bias, self.c.layer_norm_eps)
        h = K.linear_gelu(h, self.fc1.weight, self.fc1.bias)               # gelu(h @ W1^T + b1)
        return K.linear_residual(h, self.fc2.weight, self.fc2.bias, x, mid)   # (+ mid pos-embed, fused)


class _MLPHead(nn.Module):
    def __init__(self, d_in: int, d_hidden: int, d_out: int, n_layers: int = 3):
        super().__init__()
        dims = [d_in] + [d_hidden] * (n_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims, dims[1:] + [d_out]))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        for i, l in enumerate(self.layers):
            x = l(x)
            if i < len(self.layers) - 1:
                x = F.relu(x)
        return x


class YolosSmall(nn.Module):
    def __init__(self, c: Optional[YolosConfig] = None):
        super().__init__()
        c = c or YolosConfig()
        self.c = c
        d = c.hidden_size
        gh, gw = c.image_size[0] // c.patch_size, c.image_size[1] // c.patch_size
        self.cls_token = nn.Parameter(torch.zeros(1, 1, d))
        self.det_tokens = nn.Parameter(torch.zeros(1, c.num_detection_tokens, d))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + gh * gw + c.num_detection_tokens, d))
        self.patch = nn.Conv2d(c.num_channels, d, kernel_size=c.patch_size, stride=c.patch_size)
        self.mid_pos_embed = (nn.Parameter(torch.zeros(c.num_layers - 1, 1, 1 + gh * gw + c.num_detection_tokens, d))
                              if c.use_mid_position_embeddings else None)
        self.blocks = nn.ModuleList(_Block(c) for _ in range(c.num_layers))
        self.ln_f = nn.LayerNorm(d, eps=c.layer_norm_eps)
        self.cls_head = _MLPHead(d, d, c.num_labels + 1)
        self.box_head = _MLPHead(d, d, 4)
        # per-size device tensors that a captured graph reads by address (ops/graph_cache.py): what is
        # handed out under capture stays until invalidate_cache() or a parameter-version change; of the
        # sizes only run eagerly the CACHED_SIZES most recently used are kept
        self._pos_cache = GraphCache(CACHED_SIZES)
        self._tok_cache = GraphCache(CACHED_SIZES)
        self._ts_cache = GraphCache(CACHED_SIZES)
        #: the image processor of :meth:`encode_image` / :meth:`detect_image` (replace it for another size rule)
        self.processor = YolosProcessor(patch=c.patch_size)
        self.reset_parameters()

    def reset_parameters(self, seed: int = 0) -> None:
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                if p.dim() >= 2:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.02)
                else:
                    p.zero_()
            for m in self.modules():
                if isinstance(m, nn.LayerNorm):
                    m.weight.fill_(1.0)

    # -- position embeddings ---------------------------------------------------------------
    def _interp(self, pe: torch.Tensor, hw: Tuple[int, int]) -> torch.Tensor:
        c = self.c
        nd = c.num_detection_tokens
        gh, gw = c.image_size[0] // c.patch_size, c.image_size[1] // c.patch_size
        cls_pe, patch_pe, det_pe = pe[..., :1, :], pe[..., 1:-nd, :], pe[..., -nd:, :]
        lead = patch_pe.shape[:-2]
        patch_pe = patch_pe.reshape(-1, gh, gw, c.hidden_size).permute(0, 3, 1, 2)
        nh, nw = hw[0] // c.patch_size, hw[1] // c.patch_size
        patch_pe = F.interpolate(patch_pe, size=(nh, nw), mode="bicubic", align_corners=False)
        patch_pe = patch_pe.flatten(2).transpose(1, 2).reshape(*lead, nh * nw, c.hidden_size)
        return torch.cat((cls_pe, patch_pe, det_pe), dim=-2)

    def position_embeddings(self, hw: Tuple[int, int]) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        key = (hw[0], hw[1], str(self.pos_embed.device), self.pos_embed._version)

        def make():
            with torch.no_grad():
                pe = self._interp(self.pos_embed, hw).contiguous()
                mid = self._interp(self.mid_pos_embed, hw).contiguous() if self.mid_pos_embed is not None else None
            return pe, mid
        # entries of another device or parameter version are stale: they leave, pinned or not
        return self._pos_cache.get(key, make, lambda k: k[2:] != key[2:])

    def invalidate_cache(self) -> None:
        """Drop every cached per-size tensor (after the parameters changed in place in a way their
        version counters miss, e.g. through ``.data``). Graphs captured before must be captured again."""
        self._pos_cache.clear()
        self._tok_cache.clear()
        self._ts_cache.clear()

    # -- forward -------------------------------------------------------------------------
    def forward(self, pixels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.detect(self.encode_detection(pixels))

    def encode(self, pixels: torch.Tensor) -> torch.Tensor:
        """Tokens after the last block, ``[B, T, D]`` (before ``ln_f``): every row, not only the
        detection rows the heads read — the last block runs in full here, whatever the detection
        tail's rule says (:meth:`encode_detection` is the form that skips the other rows)."""
        return self._run_blocks(*self._embed(pixels))

    def encode_detection(self, pixels: torch.Tensor) -> torch.Tensor:
        """The detection rows after the last block, ``[B, nd, D]`` (before ``ln_f``): what
        :meth:`detect` reads of :meth:`encode`'s tokens. Where the detection tail is taken
        (:func:`detection_tail`) the last block computes these rows only, equal to
        ``encode(pixels)[:, -nd:]`` to fp32 rounding; elsewhere they are that slice itself."""
        return self._run_blocks(*self._embed(pixels), det_only=True)

    def _embed(self, pixels: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """The token rows before the first block (patches + class / detection tokens + position
        embeddings) and the mid position embeddings."""
        B, _, Hh, Ww = pixels.shape
        pe, mid = self.position_embeddings((Hh, Ww))
        nd = self.c.num_detection_tokens
        hip = B == 1 and pixels.is_cuda and K.get_backend() == "hip"
        if hip:
            # one copy of the token template (class/detection token rows already + pos), then the
            # patch rows written straight into it by the GEMM (bias + pos fused)
            P = (Hh // self.c.patch_size) * (Ww // self.c.patch_size)
            x = self.token_template((Hh, Ww)).clone()
            K.patch_embed(pixels, self.patch.weight, self.patch.bias, self.c.patch_size, pe[0, 1:1 + P],
                          out=x[0, 1:1 + P])
        else:
            xp = K.patch_embed(pixels, self.patch.weight, self.patch.bias, self.c.patch_size)   # [B, P, D]
            x = torch.cat((self.cls_token.expand(B, -1, -1), xp, self.det_tokens.expand(B, -1, -1)), dim=1) + pe
        return x, mid

    def _run_blocks(self, x: torch.Tensor, mid: Optional[torch.Tensor], det_only: bool = False) -> torch.Tensor:
        """Every block on ``x``: ``[B, T, D]`` — or, with ``det_only``, the detection rows
        ``[B, nd, D]``, the last block running on those rows alone where the detection tail is taken."""
        nd = self.c.num_detection_tokens
        last = len(self.blocks) - 1
        tail = det_only and detection_tail(x.shape[1], nd) and self.blocks[last].tail_supported(x)
        if K.x3_active(x):
            h3 = None
            for i, blk in enumerate(self.blocks):
                if tail and i == last:
                    return blk.forward_tail(x, h3, nd)
                nxt = self.blocks[i + 1].ln1 if i + 1 < len(self.blocks) else None
                x, h3 = blk.forward_x3(x, mid[i] if mid is not None and i < self.c.num_layers - 1 else None, h3, nxt)
        else:
            for i, blk in enumerate(self.blocks):
                if tail and i == last:
                    return blk.forward_tail(x, None, nd)
                x = blk(x, mid[i] if mid is not None and i < self.c.num_layers - 1 else None)
        return x[:, -nd:] if det_only else x

    # -- image in, detections out ----------------------------------------------------------
    def _image_fused(self, img: torch.Tensor, hw: Tuple[int, int]) -> bool:
        """The uint8 image can go straight to the patch GEMM's planes: batch 1 on the GPU in x3 mode,
        and a resize the kernel takes (``ops.image.fusable``)."""
        p = self.c.patch_size
        return (img.shape[0] == 1 and img.is_cuda and K.x3_active(self.pos_embed) and self.c.num_channels == 3
                and (3 * p * p) % 32 == 0 and I.fusable(tuple(img.shape[1:3]), hw, p))

    def encode_image(self, image_u8, det_only: bool = False) -> torch.Tensor:
        """:meth:`encode` (every row, ``[B, T, D]``; with ``det_only`` :meth:`encode_detection`, the
        detection rows ``[B, nd, D]``) from a uint8 HWC image (tensor, ndarray or PIL) or a
        ``processor.Frame`` (NV12 / NV21, planar 4:2:0, BGR / RGBA / BGRA, pitched views: converted inside the same kernel): resized by
        ``self.processor``'s rule, normalised and split into the patch GEMM's x3 planes by one kernel
        (``ops.image.image_patch_planes``) — no fp32 image is materialised. In ``f32`` mode, off the GPU
        or for a batch it is ``encode(processor.preprocess(image))``."""
        img = self.processor.as_batch(image_u8, self.pos_embed.device)
        hw = self.processor.size(tuple(img.shape[1:3]))
        if not self._image_fused(img, hw):
            px = self.processor.preprocess(img)
            return self.encode_detection(px) if det_only else self.encode(px)
        from ...ops.gemm import gemm_x3
        pe, mid = self.position_embeddings(hw)
        p = self.c.patch_size
        P = (hw[0] // p) * (hw[1] // p)
        x = self.token_template(hw).clone()
        planes, _ = self.processor.patch_planes(img, hw, patch=p)
        gemm_x3(planes, self.patch.weight.reshape(self.patch.weight.shape[0], -1), self.patch.bias,
                residual2=pe[0, 1:1 + P], out=x[0, 1:1 + P])
        return self._run_blocks(x, mid, det_only=det_only)

    def encode_detection_image(self, image_u8) -> torch.Tensor:
        """:meth:`encode_detection` from an image: ``encode_image``'s input, the detection rows out."""
        return self.encode_image(image_u8, det_only=True)

    def detect_image(self, image_u8, threshold: float = 0.5) -> Dict[str, torch.Tensor]:
        """Image in, detections out, with no host synchronisation (so it can be captured in a graph):
        ``{"logits", "pred_boxes"}`` of the model and ``{"count", "scores", "labels", "boxes"}`` of
        ``ops.image.detections`` — survivors first, in token order, boxes in pixels of the original
        image as it was passed (of a YUV frame: of its Y plane; of a crop: of the crop; a captured graph reads the frame's buffers by address, so a
        new frame written into them is what the next replay detects on).
        ``self.processor.results(count, scores, labels, boxes)`` gives the per-image lists."""
        img = self.processor.as_batch(image_u8, self.pos_embed.device)
        logits, boxes = self.detect(self.encode_detection_image(img))
        count, scores, labels, xyxy = I.detections(logits, boxes, self._target_sizes(img), threshold)
        return {"logits": logits, "pred_boxes": boxes, "count": count, "scores": scores, "labels": labels,
                "boxes": xyxy}

    def detect_tiled(self, image_u8, tiles: Tuple[int, int] = (2, 2), overlap: float = 0.2, threshold: float = 0.5,
                     match: str = "ios", match_threshold: float = 0.5) -> Dict[str, object]:
        """Tiled ("sliced") detection of one large frame, with no host synchronisation (capturable as one graph, which
        reads the frame's buffer by address as :meth:`detect_image`'s does): the frame is cut into ``tiles = (R, C)``
        overlapping tiles of one size (``processor.tile_plan``), the ``B = R * C`` tiles run as one batch at the
        model size ``processor.size(tile_hw)``, and their detections are mapped to frame pixels and merged
        (``ops.image.merge_detections``: a box is dropped when a kept box of the same label from *another* tile
        overlaps it by more than ``match_threshold``, ``match`` ``"ios"`` or ``"iou"``). Returns ``logits [B, nd, L+1]``
        and ``pred_boxes [B, nd, 4]`` per tile, ``origins [B, 2]`` int32 ``(y0, x0)`` on the device, ``tile_hw``, and
        the merged ``count [1]``, ``scores``, ``labels``, ``boxes`` (frame pixels) and ``tile`` ``[B * nd]``, kept rows
        first by score; ``self.processor.results(count, scores, labels, boxes)`` gives the list.

        On the GPU in x3 mode, for a resize the kernel takes, the tiles are staged by one launch
        (``ops.image.tiled_patch_planes``), one patch GEMM at ``M = B * P`` writes a temporary (bias and the position
        rows fused, broadcast over the tiles) that one copy puts into the patch rows of ``B`` token templates, the
        blocks run with the detection tail, and the final LayerNorm and both heads run fused on the ``B * nd`` rows.
        Elsewhere it is ``detect(encode_detection(processor.preprocess(stacked crops)))`` and the merge. On that fused
        route a ``processor.Frame`` other than ``Packed`` (NV12, P010, YUY2 ...) is not converted: its
        ``tile_planes`` stages the tiles straight from the planes, bit-equal to the packed launch on its ``rgb()``;
        elsewhere it is converted once by its ``rgb()`` and then tiled."""
        img = self.processor.as_batch(image_u8, self.pos_embed.device)
        if img.shape[0] != 1:
            raise ValueError(f"tiles are cut from one frame, not from a batch of {img.shape[0]}")
        nd, p = self.c.num_detection_tokens, self.c.patch_size
        th, tw, origins = self.processor.tile_plan(tuple(img.shape[1:3]), tiles, overlap, nd)
        hw = self.processor.size((th, tw))
        B = len(origins)
        fused = (img.is_cuda and K.x3_active(self.pos_embed) and self.c.num_channels == 3 and (3 * p * p) % 32 == 0
                 and I.fusable((th, tw), hw, p))
        in_place = fused and self.processor.tiles_in_place(img)
        if not in_place:
            data, order = self.processor.as_packed(img)
        if fused:
            from ...ops.gemm import gemm_x3
            pe, mid = self.position_embeddings(hw)
            P = (hw[0] // p) * (hw[1] // p)
            if in_place:
                planes, _ = self.processor.frame_tile_planes(img, origins, (th, tw), hw, patch=p)
            else:
                planes, _ = self.processor.tile_planes(data, order, origins, (th, tw), hw, patch=p)
            rows = gemm_x3(planes, self.patch.weight.reshape(self.patch.weight.shape[0], -1), self.patch.bias,
                           residual2=pe[0, 1:1 + P])
            x = self.token_template(hw).repeat(B, 1, 1)
            x[:, 1:1 + P] = rows.view(B, P, -1)
            det = self._run_blocks(x, mid, det_only=True).contiguous()
            if self.heads_fusable():
                logits, boxes = K.detection_heads(det.view(B * nd, -1), self.ln_f, self.cls_head.layers,
                                                  self.box_head.layers)
                logits, boxes = logits.view(B, nd, -1), boxes.view(B, nd, -1)
            else:
                det = K.layernorm(det, self.ln_f.weight, self.ln_f.bias, self.c.layer_norm_eps)
                logits, boxes = self.cls_head(det), torch.sigmoid(self.box_head(det))
        else:
            crops = I.tile_crops(data, origins, (th, tw))
            if order != "rgb":
                crops = I.packed_to_rgb(crops, order)
            logits, boxes = self.detect(self.encode_detection(self.processor.preprocess(crops)))
        org = I.origin_tensor(origins, img.device)
        count, scores, labels, xyxy, tile = I.merge_detections(logits, boxes, org, (th, tw), threshold, match,
                                                               match_threshold)
        return {"logits": logits, "pred_boxes": boxes, "origins": org.clone(), "tile_hw": (th, tw), "count": count,
                "scores": scores, "labels": labels, "boxes": xyxy, "tile": tile}

    def track_image(self, image_u8, tracker, threshold: float = 0.5) -> Dict[str, torch.Tensor]:
        """:meth:`detect_image` and ``tracker.update`` (``tracker.Tracker``): the same dict with ``track_id`` and
        ``track_hits`` ``[1, nd]`` int32 beside ``labels`` — the id of each row's track and the frames it has been
        seen in, 0 behind ``count``. No host synchronisation either: captured as one graph, each replay detects on the
        frame then in the buffers and advances the tracker by one frame."""
        return tracker.update(self.detect_image(image_u8, threshold))

    def track_tiled(self, image_u8, tracker, tiles: Tuple[int, int] = (2, 2), overlap: float = 0.2,
                    threshold: float = 0.5, match: str = "ios", match_threshold: float = 0.5) -> Dict[str, object]:
        """:meth:`detect_tiled` and ``tracker.update``: the merged list with ``track_id`` and ``track_hits``
        ``[B * nd]`` int32 beside it, capturable as :meth:`track_image` is. (``match`` and ``match_threshold`` are the
        cross-tile merge's; the tracker's own are set on the tracker.)"""
        return tracker.update(self.detect_tiled(image_u8, tiles, overlap, threshold, match, match_threshold))

    def annotate_image(self, frame, overlay, threshold: float = 0.5, tracker=None, target=None) -> Dict[str, object]:
        """:meth:`detect_image` — :meth:`track_image` with a ``tracker`` — and ``overlay.draw`` (``overlay.Overlay``)
        into ``target``: the same dict with ``"frame"``, the painted target, added. One more launch and no host
        synchronisation: frame in, annotated (or redacted) frame out is still one capturable graph. ``target`` is a
        surface of the frame's size (the boxes are in the frame's pixels) and defaults to ``frame`` itself, painted in
        place: a decoder writes the next frame over it before the next replay. With ``target=None`` a replay on an
        unchanged buffer therefore detects on the annotated frame, not on the one that was put there."""
        det = self.detect_image(frame, threshold) if tracker is None else self.track_image(frame, tracker, threshold)
        return {**det, "frame": overlay.draw(det, frame if target is None else target)}

    def annotate_tiled(self, frame, overlay, tiles: Tuple[int, int] = (2, 2), overlap: float = 0.2,
                       threshold: float = 0.5, match: str = "ios", match_threshold: float = 0.5, tracker=None,
                       target=None) -> Dict[str, object]:
        """:meth:`detect_tiled` — :meth:`track_tiled` with a ``tracker`` — and ``overlay.draw`` of the merged list into
        ``target``, as :meth:`annotate_image`: with ``target=None`` the frame itself is painted, and a replay on an
        unchanged buffer detects on the annotated frame."""
        if tracker is None:
            det = self.detect_tiled(frame, tiles, overlap, threshold, match, match_threshold)
        else:
            det = self.track_tiled(frame, tracker, tiles, overlap, threshold, match, match_threshold)
        return {**det, "frame": overlay.draw(det, frame if target is None else target)}

    def _target_sizes(self, img: torch.Tensor) -> torch.Tensor:
        """``[B, 2]`` fp32 (height, width) of the original images on their device, cached: a captured
        graph must not copy from the host."""
        B, h, w = img.shape[:3]
        return self._ts_cache.get((B, h, w, str(img.device)),
                                  lambda: torch.tensor([[h, w]] * B, dtype=torch.float32).to(img.device))

    def detect(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(logits, boxes)`` from :meth:`encode`'s tokens or :meth:`encode_detection`'s rows:
        ``ln_f`` and the two MLP heads on the last ``nd`` rows."""
        hip = x.shape[0] == 1 and x.is_cuda and K.get_backend() == "hip"
        det = x[:, -self.c.num_detection_tokens:, :]
        if hip and x.is_contiguous() and self.heads_fusable():
            # final LayerNorm + both MLP heads in three launches (csrc/head.hip)
            logits, boxes = K.detection_heads(det[0], self.ln_f, self.cls_head.layers, self.box_head.layers)
            return logits[None], boxes[None]
        det = K.layernorm(det.contiguous(), self.ln_f.weight, self.ln_f.bias, self.c.layer_norm_eps)
        return self.cls_head(det), torch.sigmoid(self.box_head(det))

    def heads_fusable(self) -> bool:
        """Both heads are 3-layer MLPs of one shape with rows of at most 384 (a multiple of 4) —
        what the fused kernel stages in LDS (``csrc/head.hip``); otherwise the module path runs."""
        ch, bh = self.cls_head.layers, self.box_head.layers
        d, hid = self.c.hidden_size, ch[0].weight.shape[0]
        return (len(ch) == 3 and len(bh) == 3 and ch[0].weight.shape == bh[0].weight.shape
                and ch[1].weight.shape == bh[1].weight.shape and d <= 384 and hid <= 384
                and d % 4 == 0 and hid % 4 == 0)

    def token_template(self, hw: Tuple[int, int]) -> torch.Tensor:
        """[1, T, D]: the class-token row + its position embedding, zero patch rows, the detection-token
        rows + theirs — cached per parameter versions (every forward copies it once)."""
        key = (tuple(hw), str(self.pos_embed.device), self.pos_embed._version, self.cls_token._version,
               self.det_tokens._version)

        def make():
            pe, _ = self.position_embeddings(hw)
            nd = self.c.num_detection_tokens
            with torch.no_grad():
                t = torch.zeros_like(pe)
                t[:, :1] = self.cls_token + pe[:, :1]
                t[:, -nd:] = self.det_tokens + pe[:, -nd:]
            return t
        return self._tok_cache.get(key, make, lambda k: k[1:] != key[1:])

    def flops_per_inference(self, hw: Tuple[int, int] = DEMO_INPUT_HW) -> float:
        c = self.c
        T = 1 + (hw[0] // c.patch_size) * (hw[1] // c.patch_size) + c.num_detection_tokens
        d, f = c.hidden_size, c.intermediate_size
        per_layer = 2 * T * (3 * d * d + d * d + 2 * d * f) + 4 * T * T * d
        patch = 2 * (T - 1 - c.num_detection_tokens) * d * c.num_channels * c.patch_size ** 2
        return float(c.num_layers * per_layer + patch)

    # -- weights ------------------------------------------------------------------------
    def load_hf_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Map ``transformers`` YolosForObjectDetection weights onto this module."""
        own: Dict[str, torch.Tensor] = {
            "cls_token": sd["vit.embeddings.cls_token"],
            "det_tokens": sd["vit.embeddings.detection_tokens"],
            "pos_embed": sd["vit.embeddings.position_embeddings"],
            "patch.weight": sd["vit.embeddings.patch_embeddings.projection.weight"],
            "patch.bias": sd["vit.embeddings.patch_embeddings.projection.bias"],
            "ln_f.weight": sd["vit.layernorm.weight"],
            "ln_f.bias": sd["vit.layernorm.bias"],
        }
        if self.mid_pos_embed is not None:
            own["mid_pos_embed"] = sd["vit.encoder.mid_position_embeddings"]
        for i in range(self.c.num_layers):
            p = f"vit.encoder.layer.{i}."
            a = p + "attention."
            own[f"blocks.{i}.qkv.weight"] = torch.cat([sd[a + f"attention.{n}.weight"] for n in ("query", "key", "value")])
            own[f"blocks.{i}.qkv.bias"] = torch.cat([sd[a + f"attention.{n}.bias"] for n in ("query", "key", "value")])
            own[f"blocks.{i}.proj.weight"] = sd[a + "output.dense.weight"]
            own[f"blocks.{i}.proj.bias"] = sd[a + "output.dense.bias"]
            own[f"blocks.{i}.ln1.weight"] = sd[p + "layernorm_before.weight"]
            own[f"blocks.{i}.ln1.bias"] = sd[p + "layernorm_before.bias"]
            own[f"blocks.{i}.ln2.weight"] = sd[p + "layernorm_after.weight"]
            own[f"blocks.{i}.ln2.bias"] = sd[p + "layernorm_after.bias"]
            own[f"blocks.{i}.fc1.weight"] = sd[p + "intermediate.dense.weight"]
            own[f"blocks.{i}.fc1.bias"] = sd[p + "intermediate.dense.bias"]
            own[f"blocks.{i}.fc2.weight"] = sd[p + "output.dense.weight"]
            own[f"blocks.{i}.fc2.bias"] = sd[p + "output.dense.bias"]
        for head, hf in (("cls_head", "class_labels_classifier"), ("box_head", "bbox_predictor")):
            for j in range(3):
                own[f"{head}.layers.{j}.weight"] = sd[f"{hf}.layers.{j}.weight"]
                own[f"{head}.layers.{j}.bias"] = sd[f"{hf}.layers.{j}.bias"]
        missing, unexpected = self.load_state_dict(own, strict=True), None
        del missing, unexpected
        self.invalidate_cache()


def demo_input(batch: int = 1, hw: Tuple[int, int] = DEMO_INPUT_HW, device: str = "cpu", seed: int = 0) -> torch.Tensor:
    """A normalised image tensor of the demo's processed shape (synthetic; no dataset access)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 3, hw[0], hw[1], generator=g).to(device)
