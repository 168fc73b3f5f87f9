"""The host checks of the x3 attention's one entry point (``nos_attention_x3``, ``csrc/attn_x3.hip``),
without a device: descriptors built with the ``Structure`` class and the filler ``ops/kernels.py``
itself uses, one invalid field each, every one refused with its own message. The messages differ by
field, so a field read at another offset than Python wrote it answers with the wrong message (or
none). Every pointer is a small host buffer: nothing here may pass validation, so there is no valid
descriptor, and the module does not run where a GPU could take a launch."""
import ctypes
import os

import pytest
import torch

from walkai_nos_amd.ops import build
from walkai_nos_amd.ops import kernels as K

if torch.cuda.is_available():
    pytest.skip("host-pointer descriptors must never reach a device", allow_module_level=True)

HOST = (ctypes.c_float * 16)()
P = ctypes.addressof(HOST)
B, T, H = 2, 33, 2   # one query group of 8 tiles per (batch, head): B*H*QG = 4 row counters


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(build.OUT, "libnos_kernels.so")
    if not os.path.exists(path):
        pytest.skip("libnos_kernels.so not built")
    L = ctypes.CDLL(path)
    L.nos_attention_x3.argtypes = [ctypes.POINTER(K.NosAttnX3), ctypes.c_void_p]
    L.nos_kernels_last_error.restype = ctypes.c_char_p
    return L


def desc(**change) -> K.NosAttnX3:
    """fp32 QKV in, fp32 out, every head and row, 4 workgroups — with ``change`` applied."""
    fields = dict(qkv=P, f32in=1, out=P, outp=None, ws=P, B=B, T=T, H=H, head_dim=64, scale=0.125, waves=4)
    return K._x3_desc(**{**fields, **change})


WINDOW = "query window out of range"
NEEDS_FIXUP = "a query window needs the pipelined kernel and the separate fixup launch"
ONE_OUT = "exactly one of out / outp"
WS = "needs waves > 0 and a workspace"
CASES = {
    "window q0 < 0": (dict(q0=-1, Tq=8), WINDOW),
    "window Tq = 0": (dict(q0=4, Tq=0), WINDOW),
    "window past T": (dict(q0=30, Tq=4), WINDOW),
    "out and outp": (dict(outp=P), ONE_OUT),
    "no out, no outp": (dict(out=None), ONE_OUT),
    "head_dim 32": (dict(head_dim=32), "head_dim must be 64"),
    "ws null": (dict(ws=None), WS),
    "waves 0": (dict(waves=0), WS),
    "waves 2^22": (dict(waves=1 << 22), "at most 2^22 workgroups"),
    "plane stride 4": (dict(f32in=0, plane_stride=4), "plane stride must be a multiple of 8"),
    "heads past H": (dict(h0=1, hn=2), "head block out of range"),
    "counters one short": (dict(cnt=P, ncnt=B * H * 1 - 1), "needs B*hn*QG row counters"),
    "counters and a window": (dict(cnt=P, ncnt=64, q0=1, Tq=8), NEEDS_FIXUP),
    "no fixup and a window": (dict(fixup=0, q0=1, Tq=8), NEEDS_FIXUP),
    "no fixup, out null": (dict(fixup=0, out=None, outp=P), "partials: needs the fp32 direct-output buffer"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_bad_field_is_refused_with_its_message(lib, name):
    change, message = CASES[name]
    rc = lib.nos_attention_x3(ctypes.byref(desc(**change)), None)
    assert rc != 0 and message in lib.nos_kernels_last_error().decode(), (name, rc)


def test_a_descriptor_of_another_size_is_refused_first(lib):
    d = desc(q0=-1, Tq=8)   # also a bad window: the size is what is reported
    d.size += 4
    rc = lib.nos_attention_x3(ctypes.byref(d), None)
    assert rc != 0 and "descriptor of another size" in lib.nos_kernels_last_error().decode()
