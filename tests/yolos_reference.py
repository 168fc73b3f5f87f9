"""A plain fp64 forward of the YOLOS architecture, written from the architecture with ``torch`` on the
CPU (no call into ``walkai_nos_amd.ops``), and the model the wiring tests run it against
(``tests/test_yolos_reference.py`` on the CPU, ``tests/test_gpu_model_paths.py`` on the GPU).

The model under test has every parameter distinguishable (:func:`randomize`): no zero bias, no unit
LayerNorm, mid position embeddings on, a 4x6 pre-training grid so that every input is
interpolated. One parameter set (drawn for three layers) serves the 1-, 2- and 3-layer models
(:func:`truncate`), so each truncation makes another block's rows observable."""
import math
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from walkai_nos_amd.models.workload.yolos import YolosConfig, YolosSmall

LAYERS = (1, 2, 3)
MAX_LAYERS = 3
#: (H, W, batch) -> T = 101 + (H // 16) * (W // 16): tile-exact 128, one past (129), one past 256
#: (257), both dimensions cropped to whole patches (125), odd width (125), the batch path (2 x 116)
INPUTS = ((48, 144, 1), (64, 112, 1), (192, 208, 1), (70, 98, 1), (64, 99, 1), (48, 80, 2))


def config(num_layers: int = MAX_LAYERS, mid: bool = True) -> YolosConfig:
    return YolosConfig(hidden_size=384, num_layers=num_layers, num_heads=6, intermediate_size=1536, patch_size=16,
                       num_detection_tokens=100, image_size=(64, 96), use_mid_position_embeddings=mid)


def tokens(h: int, w: int, cfg: YolosConfig = None) -> int:
    cfg = cfg or config()
    return 1 + cfg.num_detection_tokens + (h // cfg.patch_size) * (w // cfg.patch_size)


def randomize(module: torch.nn.Module, seed: int = 1) -> None:
    """Every parameter distinguishable, drawn in sorted name order from one seeded CPU generator:
    tensors of two or more dimensions ``randn * 0.05``, 1-D tensors ``randn * 0.5``, LayerNorm
    weights ``1 + randn * 0.5``."""
    g = torch.Generator().manual_seed(seed)
    ln_weights = {id(m.weight) for m in module.modules() if isinstance(m, torch.nn.LayerNorm)}
    with torch.no_grad():
        for _, p in sorted(module.named_parameters()):
            r = torch.randn(p.shape, generator=g, dtype=torch.float32)
            if id(p) in ln_weights:
                r = 1.0 + r * 0.5
            else:
                r = r * (0.05 if p.dim() >= 2 else 0.5)
            p.copy_(r)


_sd3: Dict[Tuple[bool, int], Dict[str, torch.Tensor]] = {}


def state_dict(num_layers: int = MAX_LAYERS, mid: bool = True, seed: int = 1) -> Dict[str, torch.Tensor]:
    """The fp32 CPU state dict of the ``num_layers``-layer model: the three-layer draw, truncated."""
    if (mid, seed) not in _sd3:
        m = YolosSmall(config(MAX_LAYERS, mid))
        randomize(m, seed)
        _sd3[(mid, seed)] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return truncate(_sd3[(mid, seed)], num_layers)


def truncate(sd: Dict[str, torch.Tensor], num_layers: int) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in sd.items():
        if k.startswith("blocks.") and int(k.split(".")[1]) >= num_layers:
            continue
        out[k] = v[:num_layers - 1].clone() if k == "mid_pos_embed" else v.clone()
    return out


def model(num_layers: int = MAX_LAYERS, mid: bool = True, seed: int = 1) -> YolosSmall:
    m = YolosSmall(config(num_layers, mid)).eval()
    m.load_state_dict(state_dict(num_layers, mid, seed), strict=True)
    m.invalidate_cache()
    return m


def pixels(h: int, w: int, batch: int = 1, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed * 1000003 + h * 1009 + w)
    return torch.randn(batch, 3, h, w, generator=g)


# ---- the fp64 forward ---------------------------------------------------------------------------
def _layernorm(x, w, b, eps):
    c = x - x.mean(-1, keepdim=True)
    return c / torch.sqrt((c * c).mean(-1, keepdim=True) + eps) * w + b


def interpolate(pe, cfg, nh, nw):
    """[..., 1 + gh*gw + nd, D] -> [..., 1 + nh*nw + nd, D]: the patch rows resampled bicubically."""
    nd, D = cfg.num_detection_tokens, cfg.hidden_size
    gh, gw = cfg.image_size[0] // cfg.patch_size, cfg.image_size[1] // cfg.patch_size
    lead = pe.shape[:-2]
    grid = pe[..., 1:1 + gh * gw, :].reshape(-1, gh, gw, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(nh, nw), mode="bicubic", align_corners=False) if grid.shape[0] else \
        grid.new_zeros(0, D, nh, nw)
    grid = grid.permute(0, 2, 3, 1).reshape(*lead, nh * nw, D)
    return torch.cat((pe[..., :1, :], grid, pe[..., 1 + gh * gw:, :]), dim=-2)


def _mlp(x, sd, head):
    n = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith(head + ".layers."))
    for j in range(n):
        x = x @ sd[f"{head}.layers.{j}.weight"].t() + sd[f"{head}.layers.{j}.bias"]
        if j < n - 1:
            x = torch.relu(x)
    return x


def block(x, sd, i, cfg):
    """One pre-LN transformer block (without the mid position embedding) in ``x``'s precision."""
    p = f"blocks.{i}."
    B, T, D = x.shape
    H, Dh, eps = cfg.num_heads, cfg.head_dim, cfg.layer_norm_eps
    h = _layernorm(x, sd[p + "ln1.weight"], sd[p + "ln1.bias"], eps)
    q, k, v = (h @ sd[p + "qkv.weight"].t() + sd[p + "qkv.bias"]).split(D, dim=-1)   # packed q | k | v
    q, k, v = (t.reshape(B, T, H, Dh).transpose(1, 2) for t in (q, k, v))
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(Dh), dim=-1) @ v
    x = x + a.transpose(1, 2).reshape(B, T, D) @ sd[p + "proj.weight"].t() + sd[p + "proj.bias"]
    h = _layernorm(x, sd[p + "ln2.weight"], sd[p + "ln2.bias"], eps)
    h = h @ sd[p + "fc1.weight"].t() + sd[p + "fc1.bias"]
    h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return x + h @ sd[p + "fc2.weight"].t() + sd[p + "fc2.bias"]


def forward(sd: Dict[str, torch.Tensor], cfg: YolosConfig, px: torch.Tensor, dtype=torch.float64):
    """``(hidden [B, T, D] before ln_f, logits, boxes)`` of the state dict ``sd`` on ``px``."""
    sd = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}
    px = px.detach().cpu().to(dtype)
    B, _, Hh, Ww = px.shape
    nh, nw = Hh // cfg.patch_size, Ww // cfg.patch_size
    nd = cfg.num_detection_tokens
    x = F.conv2d(px, sd["patch.weight"], sd["patch.bias"], stride=cfg.patch_size)   # crops to whole patches
    assert x.shape[-2:] == (nh, nw)
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), x, sd["det_tokens"].expand(B, -1, -1)), dim=1)
    x = x + interpolate(sd["pos_embed"], cfg, nh, nw)
    mid = interpolate(sd["mid_pos_embed"], cfg, nh, nw) if "mid_pos_embed" in sd else None
    for i in range(cfg.num_layers):
        x = block(x, sd, i, cfg)
        if mid is not None and i < cfg.num_layers - 1:
            x = x + mid[i]
    det = _layernorm(x[:, -nd:], sd["ln_f.weight"], sd["ln_f.bias"], cfg.layer_norm_eps)
    return x, _mlp(det, sd, "cls_head"), torch.sigmoid(_mlp(det, sd, "box_head"))


def yardstick(m: YolosSmall, px: torch.Tensor):
    """``((hidden, logits, boxes) in fp64, err_ref per output)`` for a CPU fp32 module ``m``: the fp64
    forward of its state dict, and the max abs error against it of ``m`` itself in plain fp32 on the
    CPU (its ops take their torch form there) — the suite's yardstick. The module shares its glue
    with the GPU paths, so a wiring mistake would inflate the yardstick along with the error it
    measures: it must stay within 4x of what this file's own formula loses in fp32."""
    ref = forward(m.state_dict(), m.c, px)
    with torch.no_grad():
        got = (m.encode(px),) + tuple(m(px))
    err = tuple((g.double() - r).abs().max().item() for g, r in zip(got, ref))
    own = tuple((g.double() - r).abs().max().item()
                for g, r in zip(forward(m.state_dict(), m.c, px, dtype=torch.float32), ref))
    assert all(e <= 4.0 * o for e, o in zip(err, own)), ("the fp32 module is off the fp32 formula", err, own)
    return ref, err


_refs: dict = {}


def reference(num_layers: int, h: int, w: int, batch: int = 1):
    """``(px, (hidden, logits, boxes) in fp64, err_ref per output)`` of the ``num_layers``-layer model,
    computed once per (layers, input) and left unchanged."""
    key = (num_layers, h, w, batch)
    if key not in _refs:
        px = pixels(h, w, batch)
        _refs[key] = (px,) + yardstick(model(num_layers), px)
    return _refs[key]
