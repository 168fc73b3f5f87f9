"""Inputs that drive the HIP kernels off their bulk path, built on the CPU and shared by the GPU edge
tests (``tests/test_gpu_kernel_edges.py``) and the CPU test of the construction itself
(``tests/test_kernel_inputs.py``).

Staged-logit attention inputs. The x3 attention kernels move a row's running max ``m`` lazily: only
when a key block's max exceeds it by more than 8 in exp2 units. On ``randn`` inputs that never
happens after the first block, so the ``alpha`` rescale, P values above 1 and stream-K partials
whose maxima differ widely are never run. :func:`staged_qkv` plants a known logit profile in
dimension 0 of every head: ``Q[..., q, 0] = a[q]`` and ``K[..., key, 0] = c[key]`` with
``a[q] = gain * (1, -1, 0, 1/8)[q % 4]`` (neighbouring lanes of one wave disagree, so the
wave-uniform ballot is mixed) and ``gain = delta / (scale * log2 e)`` (one unit of ``c`` moves the
score by ``delta`` exp2 units). The other 63 dimensions stay ``randn * 0.5`` and V ``randn``."""
import math

import numpy as np
import torch

LOG2E = 1.4426950408889634
HD = 64
#: the lazy-rescale threshold of the x3 attention kernels, exp2 units
RESCALE_GAP = 8.0
#: (profile, delta) pairs of the staged inputs
STAGED = (("stairs", 4.0), ("stairs", 7.5), ("stairs", 8.5), ("stairs", 30.0),
          ("spike_last", 60.0), ("spike_first", 60.0), ("saw", 12.0))
_LANE_GAIN = (1.0, -1.0, 0.0, 0.125)


def key_profile(profile: str, T: int) -> torch.Tensor:
    key = torch.arange(T)
    if profile == "stairs":
        return (key // 32).float()
    if profile == "saw":
        return ((key // 32) % 2).float()
    c = torch.zeros(T)
    if profile == "spike_last":
        c[T - 1] = 1.0
    elif profile == "spike_first":
        c[0] = 1.0
    else:
        raise ValueError(profile)
    return c


def randn_qkv(B: int, T: int, H: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, 3 * H * HD, generator=g)


def staged_qkv(profile: str, delta: float, B: int, T: int, H: int, scale: float = 0.125, seed: int = 0) -> torch.Tensor:
    """Packed fp32 ``[B, T, 3*H*64]`` QKV with the staged logit profile (module docstring)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3, H, HD, generator=g)
    qkv[:, :, :2] *= 0.5
    gain = delta / (scale * LOG2E)
    a = gain * torch.tensor(_LANE_GAIN)[torch.arange(T) % 4]
    qkv[:, :, 0, :, 0] = a[None, :, None]
    qkv[:, :, 1, :, 0] = key_profile(profile, T)[None, :, None]
    return qkv.reshape(B, T, 3 * H * HD).contiguous()


def _heads(qkv: torch.Tensor, H: int):
    B, T, _ = qkv.shape
    return qkv.view(B, T, 3, H, HD).permute(2, 0, 3, 1, 4)


def attention_formula(qkv: torch.Tensor, H: int, scale: float) -> torch.Tensor:
    """``softmax(q k^T * scale) v`` in ``qkv``'s own precision with plain torch ops: fp64 input gives
    the reference, fp32 input on the CPU the fp32 yardstick (``err_ref``)."""
    B, T, _ = qkv.shape
    q, k, v = _heads(qkv, H)
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, T, H * HD)


def attention_reference(qkv: torch.Tensor, H: int, scale: float = 0.125):
    """``(ref64, err_ref, vmax)``: the fp64 output, the max abs error of the fp32 formula on the CPU
    against it, and ``max |V|``."""
    cpu = qkv.detach().cpu()
    ref = attention_formula(cpu.double(), H, scale)
    err_ref = (attention_formula(cpu, H, scale).double() - ref).abs().max().item()
    vmax = _heads(cpu, H)[2].abs().max().item()
    return ref, err_ref, vmax


def rescale_replay(qkv: torch.Tensor, H: int, scale: float = 0.125, gap: float = RESCALE_GAP) -> dict:
    """The kernels' lazy running-max rule replayed per query row in fp64 over 32-key blocks: ``m``
    moves to ``max(m, mx)`` only where ``mx - m > gap`` (exp2 units). Returns the number of
    (row, block) events that ``fired`` with a finite ``m``, that were ``held`` (a gap in (0, gap]
    that did not fire), and the ``largest_gap`` seen with a finite ``m``."""
    B, T, _ = qkv.shape
    q, k, _ = _heads(qkv.detach().cpu().double(), H)
    s = (q @ k.transpose(-1, -2)) * (scale * LOG2E)
    nk = (T + 31) // 32
    pad = torch.full((B, H, T, nk * 32 - T), -math.inf, dtype=s.dtype)
    mx = torch.cat([s, pad], -1).view(B, H, T, nk, 32).max(-1).values
    m = mx[..., 0].clone()  # the first block always moves m (from -inf)
    fired = held = 0
    largest = 0.0
    for i in range(1, nk):
        d = mx[..., i] - m
        fire = d > gap
        fired += int(fire.sum())
        held += int(((d > 0) & ~fire).sum())
        largest = max(largest, float(d.max()))
        m = torch.where(fire, torch.maximum(m, mx[..., i]), m)
    return {"fired": fired, "held": held, "largest_gap": largest}


def lazy_softmax_attention(qkv: torch.Tensor, H: int, scale: float = 0.125, gap: float = RESCALE_GAP,
                           rescale: bool = True) -> torch.Tensor:
    """The kernels' online softmax replayed in fp64 over 32-key blocks with the lazy running max
    (decided per row). ``rescale=False`` leaves out the ``alpha`` rescale of ``l`` and ``o`` when
    ``m`` moves: a deliberately wrong kernel, to show which inputs can tell the difference."""
    B, T, _ = qkv.shape
    q, k, v = _heads(qkv.detach().cpu().double(), H)
    s = (q @ k.transpose(-1, -2)) * (scale * LOG2E)
    m = torch.full((B, H, T), -math.inf, dtype=s.dtype)
    l = torch.zeros(B, H, T, dtype=s.dtype)
    o = torch.zeros(B, H, T, HD, dtype=s.dtype)
    for k0 in range(0, T, 32):
        sb = s[..., k0:k0 + 32]
        mx = sb.max(-1).values
        m_new = torch.where(mx - m > gap, torch.maximum(m, mx), m)
        if rescale:
            alpha = torch.exp2(m - m_new)
            l, o = l * alpha, o * alpha[..., None]
        m = m_new
        p = torch.exp2(sb - m[..., None])
        l = l + p.sum(-1)
        o = o + p @ v[..., k0:k0 + 32, :]
    return (o / l[..., None]).transpose(1, 2).reshape(B, T, H * HD)


# ---- epilogue points ----------------------------------------------------------------------------
def gelu_points() -> torch.Tensor:
    """Pre-activations for the GELU epilogues: a 4097-point linspace over [-12, 12], +-sqrt 2 and
    +-4 sqrt 2 with their fp32 neighbours (the packed erf's branch seam |z| = 1 and its clamp
    |z| = 4), +-0, +-1e-30, +-30 and +-1e4."""
    f32 = np.float32
    pts = [np.linspace(-12.0, 12.0, 4097).astype(f32)]
    for c in (math.sqrt(2.0), 4.0 * math.sqrt(2.0)):
        x = f32(c)
        near = [x]
        lo = hi = x
        for _ in range(3):
            lo, hi = np.nextafter(lo, f32(0)), np.nextafter(hi, f32(np.inf))
            near += [lo, hi]
        near = np.array(near, f32)
        pts += [near, -near]
    pts.append(np.array([0.0, -0.0, 1e-30, -1e-30, 30.0, -30.0, 1e4, -1e4], f32))
    return torch.from_numpy(np.concatenate(pts))


def gelu_reference(v: torch.Tensor) -> torch.Tensor:
    x = v.detach().cpu().double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ---- LayerNorm rows -----------------------------------------------------------------------------
LN_PROFILES = ("randn", "offset", "outlier", "tiny", "huge")


def layernorm_rows(profile: str, rows: int, D: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g)
    if profile == "randn":
        return x
    if profile == "offset":
        return x + 1e4
    if profile == "outlier":
        x[torch.arange(rows), (torch.arange(rows) * 131 + 5) % D] = 1e4
        return x
    if profile == "tiny":
        return x * 1e-20
    if profile == "huge":
        return x * 1e15
    if profile == "zero":
        return torch.zeros(rows, D)
    raise ValueError(profile)


def layernorm_formula(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    """The two-pass LayerNorm written out in ``x``'s precision (fp64: the reference; fp32 on the CPU:
    the yardstick)."""
    D = x.shape[-1]
    c = x - x.sum(-1, keepdim=True) / D
    var = (c * c).sum(-1, keepdim=True) / D
    return c * torch.rsqrt(var + eps) * w + b


# ---- split3 -------------------------------------------------------------------------------------
#: the largest fp32 whose bf16 rounding stays finite: 0x7F7F7FFF (one below the tie to 2^128)
SPLIT3_MAX_BITS = 0x7F7F7FFF


def split3_points() -> torch.Tensor:
    """+-0, mantissa-all-ones values around 1.0 (0x3F7FFFFF and neighbours: the bf16 rounding
    carries into the exponent), every power of two from 2^-126 to 2^127, and the largest value
    whose bf16 rounding stays finite with its neighbours below; length a multiple of 4."""
    bits = [0x00000000, 0x80000000]
    for base in (0x3F7FFFFF, 0x3FFFFFFF, 0x3F7F7FFF, 0x3F7F8000, 0x3F7F8001, 0x3F807FFF, 0x3F808000):
        bits += [base - 1, base, base + 1]
    bits += [(e << 23) for e in range(1, 255)]
    bits += [SPLIT3_MAX_BITS - 2, SPLIT3_MAX_BITS - 1, SPLIT3_MAX_BITS, 0x7F7F0000, 0x7F000001]
    bits += [b | 0x80000000 for b in bits[2:]]
    while len(bits) % 4:
        bits.append(0x3F800000)
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


# ---- the collector of the GPU tests' figures --------------------------------------------------------
class Worst:
    """Collects ``err`` against ``max(factor * err_ref, floor)``, prints the worst ratio, then asserts:
    the figures reach the log whether or not the bound holds."""

    def __init__(self, name, factor=4.0, label="edges"):
        self.label = label
        self.name, self.factor, self.ratio, self.at, self.n, self.fail = name, factor, 0.0, None, 0, []

    def check(self, err, err_ref, floor, tag):
        self.n += 1
        ratio = err / err_ref if err_ref > 0 else (0.0 if err == 0 else math.inf)
        if not ratio <= self.ratio:  # NaN counts
            self.ratio, self.at = ratio, (tag, err, err_ref)
        if not err <= max(self.factor * err_ref, floor):
            self.fail.append((tag, err, err_ref, floor))

    def done(self):
        print(f"[{self.label}] {self.name}: {self.n} checks, worst err/err_ref {self.ratio:.3g} at {self.at}, "
              f"{len(self.fail)} over the bound")
        assert self.n > 0
        assert not self.fail, (self.name, len(self.fail), self.fail[:6])
