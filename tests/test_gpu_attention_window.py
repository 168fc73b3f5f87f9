"""The query window of the x3 stream-K attention (GPU only): queries are rows ``q0 .. q0+Tq-1`` of the
packed QKV tensor, keys and values all ``T`` rows, the output compact (``[B, Tq, H*64]`` or its
planes). Inputs and ``Worst`` come from ``tests/kernel_inputs.py``; the reference is the fp64 attention
of the same input on the window's rows and the bound that of ``test_gpu_kernel_edges.py``:
``4 x err_ref`` (what the plain fp32 formula loses on those rows), floor ``2e-6 |V|max``.

Every launch writes into a NaN-filled buffer with NaN guard rows before and after the output: the
guards must come back untouched and no NaN may be left inside."""
import ctypes
import os

import pytest
import torch

import kernel_inputs as KI
from kernel_inputs import Worst

pytestmark = pytest.mark.gpu

SCALE = 0.125
#: (T, q0, Tq): an unaligned window; one query in the key-tail block; the last row alone; the model's
#: form (four tiles, half a group, key tail of one); two query groups, the second partial; identity
CASES = ((33, 1, 32), (33, 32, 1), (77, 76, 1), (257, 157, 100), (333, 40, 293), (64, 0, 64))
SHAPES = ((1, 1), (2, 2))
KINDS = ("randn", "stairs:30")
GUARD = 3


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from walkai_nos_amd.ops import kernels
    assert kernels.hip_available(), "libnos_kernels.so must be built on a GPU box"
    kernels.set_backend("hip")
    return kernels


_inputs = {}


def attn_input(kind, B, T, H):
    """``(qkv on the GPU, fp64 reference, fp32-formula output, |V|max)`` — the last three on the CPU,
    every row; computed once per input and left unchanged."""
    key = (kind, B, T, H)
    if key not in _inputs:
        if kind == "randn":
            qkv = KI.randn_qkv(B, T, H, seed=T)
        else:
            p, d = kind.split(":")
            qkv = KI.staged_qkv(p, float(d), B, T, H, SCALE, seed=T)
        ref = KI.attention_formula(qkv.double(), H, SCALE)
        own = KI.attention_formula(qkv, H, SCALE).double()
        assert torch.isfinite(ref).all()
        vmax = qkv.view(B, T, 3, H, KI.HD)[:, :, 2].abs().max().item()
        _inputs[key] = (qkv.cuda(), ref, own, vmax)
    return _inputs[key]


def window_case(kind, B, T, H, q0, Tq):
    """``(qkv, ref64 of the window's rows on the GPU, err_ref over those rows, floor)``"""
    qkv, ref, own, vmax = attn_input(kind, B, T, H)
    r = ref[:, q0:q0 + Tq]
    err_ref = (own[:, q0:q0 + Tq] - r).abs().max().item()
    return qkv, r.cuda(), err_ref, 2e-6 * vmax


def window_grids(K, B, T, H, Tq, group=8):
    units = B * H * (((Tq + 31) // 32 + group - 1) // group) * ((T + 31) // 32)
    return (1, 3, 7, units + 5, K.attention_window_waves(K.slice_cus(), B, T, H, Tq))


def guarded(x3, B, Tq, H):
    """A NaN-filled buffer with GUARD rows before and after the output and the output's view of it."""
    D = H * 64
    rows = (3 if x3 else 1) * B * Tq
    buf = torch.full((rows + 2 * GUARD, D), float("nan"), dtype=torch.bfloat16 if x3 else torch.float32,
                     device="cuda")
    out = buf[GUARD:GUARD + rows].view((3, B, Tq, D) if x3 else (B, Tq, D))
    assert out.is_contiguous() and out.data_ptr() % 16 == 0
    return buf, out


def guards_untouched(buf):
    return bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all())


def as_f64(o):
    return o.double().sum(0) if o.dtype == torch.bfloat16 else o.double()


def restore_attention(K):
    K.set_attention_merge(None)
    K.set_slice_pin(0)
    K.set_attention_x3_group(8)
    K.set_attention_x3_wide(K.attention_x3_wide_default())
    K._L().nos_attention_x3_set_flags(int(os.environ.get("NOS_ATTN_X3_FLAGS", "0")))


@pytest.mark.parametrize("T,q0,Tq", CASES)
def test_window_fp32_in_wide_and_two_wave(K, T, q0, Tq):
    # attn_fwd_x3w and attn_fwd_x3p<8> on the window: bit-identical to each other, the plane output
    # split3 of the fp32 output, the planes-in kernel equal to the fp32-in one, inside the bound, the
    # guard rows untouched and no NaN left.
    # Measured worst err/err_ref (bound 4): 3.17 / 3.16 (T = 33, stairs:30, as the full launch there), 0.98 (T = 77),
    # 1.23 (257, 157, 100), 1.21 (333, 40, 293), 1.08 (64, 0, 64); kept in profiles/pytest_gpu_attention_window.log.
    wst = Worst("attention window", label="window")
    try:
        for kind in KINDS:
            for B, H in SHAPES:
                qkv, ref, err_ref, floor = window_case(kind, B, T, H, q0, Tq)
                planes = K.split3(qkv)
                for waves in window_grids(K, B, T, H, Tq):
                    for hb in (None, 1):
                        f32 = None
                        for x3 in (False, True):
                            outs = []
                            for wide in (True, False):
                                K.set_attention_x3_wide(wide)
                                buf, out = guarded(x3, B, Tq, H)
                                K.attention_x3f(qkv, out, H, 64, SCALE, waves, head_block=hb, q0=q0, q_rows=Tq)
                                tag = (kind, B, T, H, q0, Tq, waves, hb, x3, wide)
                                assert guards_untouched(buf), tag
                                assert not torch.isnan(out.float()).any(), tag
                                outs.append(out)
                            assert torch.equal(outs[0], outs[1]), tag
                            wst.check((as_f64(outs[0]) - ref).abs().max().item(), err_ref, floor, tag)
                            if x3:
                                assert torch.equal(outs[0], K.split3(f32)), tag
                                buf, out = guarded(True, B, Tq, H)
                                K.attention_x3(planes, out, H, 64, SCALE, waves, head_block=hb, q0=q0, q_rows=Tq)
                                assert guards_untouched(buf), tag
                                assert torch.equal(out, outs[0]), tag
                            else:
                                f32 = outs[0]
    finally:
        restore_attention(K)
    wst.done()


@pytest.mark.parametrize("T,q0,Tq", CASES)
def test_window_planes_in_four_tile_group(K, T, q0, Tq):
    # attn_fwd_x3p<4> (planes in, four query tiles per workgroup) and attn_sk_lds_fixup<4> on the window
    # Measured worst err/err_ref (bound 4): the 8-tile kernels' figures, 1.23 at (333, 40, 293).
    wst = Worst("attention window, 4-tile group", label="window")
    try:
        K.set_attention_x3_group(4)
        for kind in KINDS:
            for B, H in SHAPES:
                qkv, ref, err_ref, floor = window_case(kind, B, T, H, q0, Tq)
                planes = K.split3(qkv)
                for waves in window_grids(K, B, T, H, Tq, group=4):
                    for x3 in (False, True):
                        buf, out = guarded(x3, B, Tq, H)
                        K.attention_x3(planes, out, H, 64, SCALE, waves, q0=q0, q_rows=Tq)
                        tag = (kind, B, T, H, q0, Tq, waves, x3)
                        assert guards_untouched(buf), tag
                        assert not torch.isnan(out.float()).any(), tag
                        wst.check((as_f64(out) - ref).abs().max().item(), err_ref, floor, tag)
    finally:
        restore_attention(K)
    wst.done()


@pytest.mark.parametrize("T,q0,Tq", [(257, 157, 100), (333, 40, 293)])
def test_window_switches_and_pins_change_no_bit(K, T, q0, Tq):
    # every instantiation the launcher can reach besides the defaults — the explicit vmcnt wait
    # (flag 1, planes in), the static priority (2, fp32 in, two-wave), dispatch order (4), 64-bit
    # bookkeeping (8), the fixup's 2-byte stores (32) and XCD-local order (64) — pinned launches, and
    # the in-kernel-merge setting (a windowed launch keeps the fixup launch): the default's bits
    L = K._L()
    try:
        for kind in KINDS:
            for B, H in SHAPES:
                qkv = window_case(kind, B, T, H, q0, Tq)[0]
                planes = K.split3(qkv)

                def launch(waves, x3, wide, f32in):
                    K.set_attention_x3_wide(wide)
                    buf, out = guarded(x3, B, Tq, H)
                    if f32in:
                        K.attention_x3f(qkv, out, H, 64, SCALE, waves, q0=q0, q_rows=Tq)
                    else:
                        K.attention_x3(planes, out, H, 64, SCALE, waves, q0=q0, q_rows=Tq)
                    assert guards_untouched(buf) and not torch.isnan(out.float()).any()
                    return out
                for waves in window_grids(K, B, T, H, Tq):
                    for x3 in (False, True):
                        want = launch(waves, x3, True, True)
                        for flags in (1, 2, 4, 8, 32, 64):
                            L.nos_attention_x3_set_flags(flags)
                            got = [launch(waves, x3, True, True), launch(waves, x3, False, True),
                                   launch(waves, x3, False, False)]
                            L.nos_attention_x3_set_flags(0)
                            assert all(torch.equal(g, want) for g in got), (kind, B, T, H, waves, x3, flags)
                        for pin in (0b00000001, 0b00110000, 0b11111111):
                            K.set_slice_pin(pin)
                            got = [launch(waves, x3, True, True), launch(waves, x3, False, True),
                                   launch(waves, x3, False, False)]
                            K.set_slice_pin(0)
                            assert all(torch.equal(g, want) for g in got), (kind, B, T, H, waves, x3, pin)
                        K.set_attention_merge(True)
                        got = launch(waves, x3, True, True)
                        K.set_attention_merge(None)
                        assert torch.equal(got, want), (kind, B, T, H, waves, x3, "merge setting")
    finally:
        restore_attention(K)


@pytest.mark.parametrize("T", sorted({c[0] for c in CASES}))
def test_identity_window_is_the_old_entry_point(K, T):
    # q0 = 0, Tq = T through the windowed entry points: torch.equal to the entry points without a window
    try:
        for kind in KINDS:
            for B, H in SHAPES:
                qkv = attn_input(kind, B, T, H)[0]
                planes = K.split3(qkv)
                for waves in window_grids(K, B, T, H, T):
                    for x3 in (False, True):
                        for wide in (True, False):
                            K.set_attention_x3_wide(wide)
                            old = K.attention_x3f(qkv, guarded(x3, B, T, H)[1], H, 64, SCALE, waves)
                            new = K.attention_x3f(qkv, guarded(x3, B, T, H)[1], H, 64, SCALE, waves, q0=0, q_rows=T)
                            assert torch.equal(old, new), (kind, B, T, H, waves, x3, wide)
                        old = K.attention_x3(planes, guarded(x3, B, T, H)[1], H, 64, SCALE, waves)
                        new = K.attention_x3(planes, guarded(x3, B, T, H)[1], H, 64, SCALE, waves, q0=0, q_rows=T)
                        assert torch.equal(old, new), (kind, B, T, H, waves, x3, "planes in")
    finally:
        restore_attention(K)


@pytest.mark.parametrize("q0,Tq", [(-1, 8), (4, 0), (30, 4)])
def test_bad_windows_are_refused_on_the_host(K, q0, Tq):
    # q0 < 0, Tq <= 0 and q0 + Tq > T: an error from the launcher's host check, before any launch, and
    # the output as it was
    B, T, H = 1, 33, 1
    qkv = attn_input("randn", B, T, H)[0]
    planes = K.split3(qkv)
    rows = max(Tq, 1)
    ws = torch.zeros(4 * 2 * (64 * 32 + 64) * 8, device="cuda")
    L = K._L()
    for x3 in (False, True):
        buf, out = guarded(x3, B, rows, H)
        o, op = (None, out.data_ptr()) if x3 else (out.data_ptr(), None)
        common = dict(out=o, outp=op, ws=ws.data_ptr(), B=B, T=T, H=H, head_dim=64, scale=SCALE, waves=4, q0=q0, Tq=Tq)
        d = K._x3_desc(qkv=qkv.data_ptr(), f32in=1, **common)
        rc = L.nos_attention_x3(ctypes.byref(d), K._stream())
        assert rc != 0 and "query window" in L.nos_kernels_last_error().decode()
        d = K._x3_desc(qkv=planes.data_ptr(), f32in=0, plane_stride=planes[0].numel(), **common)
        rc = L.nos_attention_x3(ctypes.byref(d), K._stream())
        assert rc != 0 and "query window" in L.nos_kernels_last_error().decode()
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf.float()).all())
        if Tq > 0:  # the wrappers pass the error on
            with pytest.raises(RuntimeError, match="query window"):
                K.attention_x3f(qkv, out, H, 64, SCALE, 4, q0=q0, q_rows=Tq)
            with pytest.raises(RuntimeError, match="query window"):
                K.attention_x3(planes, out, H, 64, SCALE, 4, q0=q0, q_rows=Tq)
            torch.cuda.synchronize()
            assert bool(torch.isnan(buf.float()).all())
    assert not torch.isnan(ws).any() and not ws.any()  # the workspace too: nothing ran
    with pytest.raises(ValueError):
        K.attention_qkv_x3f(qkv, H, 64, SCALE, q0=q0, q_rows=Tq)
