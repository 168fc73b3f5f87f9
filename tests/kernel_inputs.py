"""Inputs that drive the HIP kernels off their bulk path, built on the CPU and shared by the GPU edge
tests (``tests/test_gpu_kernel_edges.py``), the exact-term tests (``tests/test_gpu_x3_terms.py``, see
"exact-term x3 inputs" below) and the CPU test of the constructions themselves
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


# ---- exact-term x3 inputs ------------------------------------------------------------------------
# The x3 kernels compute an fp32 product as six bf16 plane products (``mfma_x3``): with a = a0 + a1 + a2
# and b = b0 + b1 + b2 (``split3``), in this order: a2b0, a1b1, a0b2, a1b0, a0b1, a0b0. On ``randn`` a
# missing second-order term moves the result by 2^-16 relative: under the suite's error bounds at
# Kd <= 64 and in the split-K, stream-K and fused tests, and a fault in one buffer or stage under all.
# The cases below have a six-term product that is exact in fp32 whatever the order of the sums, so the
# check is ``torch.equal`` and a missing term is a changed bit.
#: the kept plane products (plane of a, plane of b) in the kernels' order
X3_TERMS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
TERM_N = 768
TERM_KDS = (32, 64, 128, 192)
TERM_CASES = ("a0b", "ab0", "a1b1", "dense2")
#: the deepest K at which 287^2 Kd < 2^24 (203); deeper problems get W at half density (Kd <= 384)
DENSE2_MAX_KD = 192
#: the terms a case pins: dropping any of them changes output bits (tests/test_kernel_inputs.py)
TERM_PINS = {"a0b": ((0, 0), (0, 1), (0, 2)), "ab0": ((0, 0), (1, 0), (2, 0)), "a1b1": ((0, 0), (0, 1), (1, 0), (1, 1)),
             "dense2": ((0, 0), (0, 1), (1, 0), (1, 1))}


def split3_cpu(x: torch.Tensor) -> torch.Tensor:
    """``[3, *x.shape]`` bf16 planes: round-to-nearest-even bf16 of x, then of each exact residual
    (what ``kernels.split3`` and the kernels' in-register split compute)."""
    out, r = [], x.float()
    for _ in range(3):
        out.append(r.to(torch.bfloat16))
        r = r - out[-1].float()
    return torch.stack(out)


def onehot_phases(rows: int, Kd: int) -> int:
    """Placements (:func:`onehot_k`) it takes until every (row mod 32, k div 8) pair has occurred."""
    return -(-(Kd // 8) // max(1, rows // 32))


def onehot_k(rows: int, Kd: int, phase: int = 0) -> torch.Tensor:
    """Column of the single nonzero of each row. The 32-row group ``r = row div 32`` of placement
    ``phase`` lands in the 8-column group ``(r + phase * (rows div 32)) mod (Kd / 8)``, so the full
    groups of ``onehot_phases`` placements cover every (row mod 32, k div 8) pair; within the group
    the column moves with the row."""
    m = torch.arange(rows)
    full = max(1, rows // 32)
    kg = (m // 32 + phase * full) % (Kd // 8)
    return kg * 8 + (3 * (m % 32) + m // 32 + phase) % 8


def onehot_pairs(ks, Kd: int) -> set:
    """The (row mod 32, k div 8) pairs a list of placements covers."""
    pairs = set()
    for k in ks:
        m = torch.arange(k.numel())
        pairs |= set(zip((m % 32).tolist(), (k // 8).tolist()))
    return pairs


def generic_f32(rows: int, cols: int, seed: int) -> torch.Tensor:
    """``randn`` with column c scaled by 2^e(c), e over -20 ... 20: all three planes nonzero."""
    g = torch.Generator().manual_seed(seed)
    e = (torch.arange(cols) * 17 + seed) % 41 - 20
    x = torch.randn(rows, cols, generator=g) * torch.exp2(e.float())
    planes = split3_cpu(x)
    assert all(float((p != 0).float().mean()) > 0.95 for p in planes), "generic_f32: a plane is mostly zero"
    return x


def _pow2(n: int, seed: int) -> torch.Tensor:
    i = torch.arange(n)
    return torch.exp2(((i * 5 + seed) % 7 - 3).float()) * (1 - 2 * ((i * 3 + seed) % 2)).float()


def _two_plane_ints(rows: int, cols: int, seed: int, lo: int, hi: int) -> torch.Tensor:
    """Dense odd integers of either sign with lo <= |x| <= hi inside [257, 511]: planes (even, +-1, 0)."""
    g = torch.Generator().manual_seed(seed)
    mag = 2 * torch.randint(lo // 2, (hi - 1) // 2 + 1, (rows, cols), generator=g) + 1
    return (mag * (1 - 2 * torch.randint(0, 2, (rows, cols), generator=g))).float()


def term_case(kind: str, M: int, Kd: int, phase: int = 0, N: int = TERM_N) -> dict:
    """One exact-term GEMM problem ``C = A W^T`` (``A`` [M, Kd], ``W`` [N, Kd], fp32 on the CPU):
    ``ref`` is the fp64 product cast to fp32, asserted exact; ``ka`` / ``kw`` hold the column of the
    single nonzero of each row of A / W (or None).

    ``a0b``: A one +-2^e per row (planes a1 = a2 = 0), W generic: pins a0b0, a0b1, a0b2.
    ``ab0``: the mirror (W one +-2^e per row, A generic): pins a0b0, a1b0, a2b0.
    ``a1b1``: A one +-(384 + d), d = +-1, per row (planes 384, d, 0: both neighbours of 384 are ties
    that round to the even 384, where 256 - 1 = 255 would be a bf16 number itself); W dense +-(128 j0 + j1) with
    j0 in [129, 255] (at j0 = 128 a negative j1 drops a binade, where the bf16 step is 64), j1 in
    [-63, 63] less 0 (planes 128 j0, j1, 0): every product an integer below 2^24; without a1b1 it is
    off by d j1.
    ``dense2``: both operands dense odd integers of either sign in [257, 287] (planes even, +-1, 0)
    with sum_k |a||w| < 2^24, so every partial sum is exact in any order: a1b1, a0b1 and a1b0 at full
    density in every k-step."""
    g = torch.Generator().manual_seed(1000 * Kd + 10 * phase + TERM_CASES.index(kind))
    ka = kw = None
    if kind == "a0b":
        ka = onehot_k(M, Kd, phase)
        A = torch.zeros(M, Kd)
        A[torch.arange(M), ka] = _pow2(M, phase)
        W = generic_f32(N, Kd, seed=Kd + 1)
    elif kind == "ab0":
        kw = onehot_k(N, Kd, phase)
        W = torch.zeros(N, Kd)
        W[torch.arange(N), kw] = _pow2(N, phase + 1)
        A = generic_f32(M, Kd, seed=Kd + 2 + M)
    elif kind == "a1b1":
        ka = onehot_k(M, Kd, phase)
        m = torch.arange(M)
        A = torch.zeros(M, Kd)
        A[m, ka] = ((384 + (1 - 2 * ((m // 2 + phase) % 2))) * (1 - 2 * (m % 2))).float()
        j0 = torch.randint(129, 256, (N, Kd), generator=g)
        j1 = torch.randint(1, 64, (N, Kd), generator=g) * (1 - 2 * torch.randint(0, 2, (N, Kd), generator=g))
        W = ((128 * j0 + j1) * (1 - 2 * torch.randint(0, 2, (N, Kd), generator=g))).float()
        pa, pw = split3_cpu(A), split3_cpu(W)
        assert torch.equal(pa[0].float().abs()[m, ka], torch.full((M,), 384.0)) and bool((pa[1].float().abs()[m, ka] == 1).all())
        assert (pa[1].float()[m, ka] * pa[0].float()[m, ka]).unique().numel() == 2, "a1b1: d of one sign only"
        assert torch.equal(pw[0].float().abs(), (128 * j0).float()) and torch.equal(pw[1].float().abs(), j1.abs().float())
        assert not pa[2].any() and not pw[2].any()
        assert A.abs().max().item() * W.abs().max().item() < 2 ** 24
    elif kind == "dense2":
        A = _two_plane_ints(M, Kd, 7 + Kd, 257, 287)
        W = _two_plane_ints(N, Kd, 8 + Kd, 257, 287)
        if Kd > DENSE2_MAX_KD:  # half density, a checkerboard: every k-step of every row keeps nonzeros
            W = W * ((torch.arange(N)[:, None] + torch.arange(Kd)[None, :]) % 2 == 0)
        pa, pw = split3_cpu(A), split3_cpu(W)
        assert bool((pa[1].float().abs() == 1).all()) and bool((pw[1].float().abs() == (W != 0)).all())
        assert not pa[2].any() and not pw[2].any()
        assert (A.double().abs() @ W.double().abs().t()).max().item() < 2 ** 24, ("dense2: Kd too deep", Kd)
    else:
        raise ValueError(kind)
    ref64 = A.double() @ W.double().t()
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), (kind, M, Kd, "the fp64 product is not exact in fp32")
    return {"kind": kind, "A": A, "W": W, "ref": ref, "ka": ka, "kw": kw}


def x3_emulate(A: torch.Tensor, W: torch.Tensor, terms=X3_TERMS, kstep: int = 16, planes=None) -> torch.Tensor:
    """The plane product on the CPU: per k-step of ``kstep`` columns and per kept ``(i, j)`` term, in
    the kernels' order, the product of plane i of A and plane j of W in fp64, added to an fp32
    accumulator. ``planes``: a function ``(pa, pw) -> (pa, pw)`` that misreads the planes (mutants)."""
    pa, pw = split3_cpu(A), split3_cpu(W)
    if planes is not None:
        pa, pw = planes(pa, pw)
    pa, pw = pa.double(), pw.double()
    acc = torch.zeros(A.shape[0], W.shape[0])
    for k0 in range(0, A.shape[1], kstep):
        for i, j in terms:
            acc = (acc.double() + pa[i][:, k0:k0 + kstep] @ pw[j][:, k0:k0 + kstep].t()).float()
    return acc


# ---- the attention selector ----------------------------------------------------------------------
SELECT_GAIN = 64.0
#: T -> (a, c) of the permutation pi(t) = (a t + c) mod T
SELECT_PERM = {33: (2, 32), 64: (5, 63), 257: (37, 256)}


def selector_perm(T: int) -> torch.Tensor:
    a, c = SELECT_PERM[T]
    assert math.gcd(a, T) == 1
    pi = (a * torch.arange(T) + c) % T
    assert sorted(pi.tolist()) == list(range(T))
    return pi


def selector_qkv(B: int, T: int, H: int, v: torch.Tensor = None, seed: int = 0):
    """``(qkv [B, T, 3*H*64], expected [B, T, H*64])``: key j carries the code
    ``G (e_{j mod 32} + e_{32 + j div 32})``, query t the code of key pi(t), G = 64, so a raw score is
    0, G^2 or 2 G^2 — powers of two, exact under the kernels' ``scale * log2 e`` — and the selected key
    leads every other by at least G^2 * 0.125 * log2 e = 738 exp2 units: every p, alpha and merge
    weight is exactly 1 or 0 and ``out[b, t, h] == V[b, pi(t), h]`` bit for bit. V (``v``
    [B, T, H, 64], default generic fp32 over 2^-20 ... 2^20) keeps all three planes."""
    assert T <= 32 * 32
    pi = selector_perm(T)
    j = torch.arange(T)
    code = torch.zeros(T, HD)
    code[j, j % 32] = SELECT_GAIN
    code[j, 32 + j // 32] = SELECT_GAIN
    if v is None:
        v = generic_f32(B * T * H, HD, seed=seed + T).view(B, T, H, HD)
    qkv = torch.zeros(B, T, 3, H, HD)
    qkv[:, :, 0] = code[pi][None, :, None, :]
    qkv[:, :, 1] = code[None, :, None, :]
    qkv[:, :, 2] = v
    s = code[pi].double() @ code.double().t()
    assert torch.equal(s.argmax(1), pi) and bool((s.max(1).values == 2 * SELECT_GAIN ** 2).all())
    assert (s.sort(1).values[:, -2] <= SELECT_GAIN ** 2).all()
    expected = v[:, pi].reshape(B, T, H * HD).contiguous()
    return qkv.reshape(B, T, 3 * H * HD).contiguous(), expected


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


class Exact:
    """Collects bit-for-bit comparisons (``torch.equal``), prints the launches and the count of unequal
    outputs, then asserts that there are none: the figures reach the log whether or not they hold."""

    def __init__(self, name, label="terms"):
        self.label, self.name, self.launches, self.n, self.unequal, self.fail = label, name, 0, 0, 0, []

    def check(self, out, ref, tag):
        self.n += 1
        if not torch.equal(out, ref):  # NaN is unequal to everything
            bad = int((out != ref).sum()) if out.shape == ref.shape else out.numel()
            self.unequal += bad
            if len(self.fail) < 8:
                self.fail.append((tag, bad))

    def done(self, extra=""):
        print(f"[{self.label}] {self.name}: {self.launches} launches, {self.n} comparisons, "
              f"{self.unequal} unequal outputs{extra}")
        assert self.n > 0 and self.launches > 0
        assert self.unequal == 0 and not self.fail, (self.name, self.unequal, self.fail)
