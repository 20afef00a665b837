"""CPU suite: the control-block optimizer entry points (include/dana_hip.h "optimizer scalars in device memory") refuse
bad arguments before any HIP call -- -1 and a message that names the entry point -- and the host-side packing of the
control block forms Adam's bias corrections like dana_adam. No GPU: every call here returns before its launch."""
import ctypes

import numpy as np
import pytest
import torch

from dana_amd import _lib, ops
from dana_amd.trainer import Trainer

A16 = 0x1000   # fake device addresses: 16-byte aligned, never dereferenced (the argument checks come first)
ODD = 0x1004   # 4-byte aligned only
ODD2 = 0x1002  # not even 4-byte aligned


def _err(name, *args):
    """-> (return code, dana_last_error()) of a raw call"""
    L = _lib.lib()
    rc = L.fn[name](*args)
    return rc, L.cdll.dana_last_error().decode()


def _refused(name, *args):
    rc, msg = _err(name, *args)
    assert rc == -1, (name, rc, msg)
    assert msg.startswith(name + ":"), msg
    with pytest.raises(_lib.DanaError, match=name):
        _lib.lib().call(name, *args)
    return msg


def test_grad_sqnorm_argument_errors():
    assert "multiple of 4" in _refused("dana_grad_sqnorm", A16, 6, A16, 1 << 20, None)
    assert "multiple of 4" in _refused("dana_grad_sqnorm", A16, -4, A16, 1 << 20, None)
    assert "null" in _refused("dana_grad_sqnorm", None, 8, A16, 1 << 20, None)
    assert "null" in _refused("dana_grad_sqnorm", A16, 8, None, 1 << 20, None)
    assert "aligned" in _refused("dana_grad_sqnorm", ODD, 8, A16, 1 << 20, None)
    assert "aligned" in _refused("dana_grad_sqnorm", A16, 8, ODD, 1 << 20, None)
    rc, msg = _err("dana_grad_sqnorm", A16, 4096, A16, 8, None)  # 4 workgroups need 32 bytes
    assert rc == -3 and msg.startswith("dana_grad_sqnorm: workspace")
    # an empty segment is accepted, whatever the pointers: it contributes nothing
    _lib.lib().call("dana_grad_sqnorm", None, 0, None, 0, None)


def test_grad_sqnorm_workspace_is_monotone_and_positive():
    q = lambda n: _lib.lib().query("dana_grad_sqnorm_workspace_bytes", n)
    assert q(0) == 0 and q(-4) == 0
    sizes = [1, 4, 8, 1020, 1024, 1028, 2048, 4096, 1 << 16, 1 << 20, (1 << 21) - 4, 1 << 21, (1 << 21) + 4, 37_000_000,
             1 << 28, 1 << 31]
    vals = [q(n) for n in sizes]
    assert all(v > 0 and v % 8 == 0 for v in vals)
    assert all(a <= b for a, b in zip(vals, vals[1:]))
    assert q(4) == 8 and q(1024) == 8 and q(1028) == 16      # one double per workgroup, 256 float4 per workgroup pass
    assert q(1 << 31) == q(1 << 21)                          # the grid is capped: partial counts stay small
    assert ops.grad_sqnorm_workspace(4096) == 4


def test_optim_prepare_argument_errors():
    assert "null" in _refused("dana_optim_prepare", None, 4, A16, A16, None)
    assert "count" in _refused("dana_optim_prepare", A16, -1, A16, A16, None)
    assert "null" in _refused("dana_optim_prepare", A16, 4, None, A16, None)
    assert "null" in _refused("dana_optim_prepare", A16, 4, A16, None, None)
    assert "aligned" in _refused("dana_optim_prepare", ODD, 4, A16, A16, None)   # partials are doubles
    assert "aligned" in _refused("dana_optim_prepare", A16, 4, ODD2, A16, None)
    assert "aligned" in _refused("dana_optim_prepare", A16, 4, A16, ODD2, None)


@pytest.mark.parametrize("name,tail", [("dana_sgd_momentum_ctl", (0.9, 1e-4, 0, None)),
                                       ("dana_adam_ctl", (0.9, 0.999, 1e-8, 0.0, None))])
def test_ctl_update_argument_errors(name, tail):
    nbuf = 3 if name == "dana_sgd_momentum_ctl" else 4

    def args(bufs=None, n=8, hyper=A16, state=A16, group=0):
        return tuple(bufs if bufs is not None else [A16] * nbuf) + (n, hyper, state, group) + tail

    assert "multiple of 4" in _refused(name, *args(n=6))
    assert "multiple of 4" in _refused(name, *args(n=-4))
    for k in range(nbuf):
        assert "null" in _refused(name, *args(bufs=[None if j == k else A16 for j in range(nbuf)]))
        assert "aligned" in _refused(name, *args(bufs=[ODD if j == k else A16 for j in range(nbuf)]))
    assert "null" in _refused(name, *args(hyper=None))
    assert "null" in _refused(name, *args(state=None))
    assert "aligned" in _refused(name, *args(hyper=ODD2))
    assert "aligned" in _refused(name, *args(state=ODD2))
    for g in (-1, ops.OPTIM_MAX_GROUPS, 1000):
        assert "group" in _refused(name, *args(group=g))
    assert "group" in _refused(name, *args(n=0, group=ops.OPTIM_MAX_GROUPS))  # checked even for an empty segment
    _lib.lib().call(name, *args(bufs=[None] * nbuf, n=0, hyper=None, state=None, group=ops.OPTIM_MAX_GROUPS - 1))


def test_pack_hyper_argument_errors_and_layout():
    h = np.zeros(ops.OPTIM_HYPER_FLOATS, dtype=np.float32)
    lrs = (ctypes.c_float * 4)(0.01, 0.02, 0.03, 0.04)
    hp, lp = h.ctypes.data, ctypes.cast(lrs, ctypes.c_void_p)
    assert "clip_norm" in _refused("dana_optim_pack_hyper", hp, lp, 2, 1.0, -1.0, 0.0, 0.0, 1)
    assert "null" in _refused("dana_optim_pack_hyper", None, lp, 2, 1.0, 0.0, 0.0, 0.0, 1)
    assert "null" in _refused("dana_optim_pack_hyper", hp, None, 2, 1.0, 0.0, 0.0, 0.0, 1)
    assert "groups" in _refused("dana_optim_pack_hyper", hp, lp, 0, 1.0, 0.0, 0.0, 0.0, 1)
    assert "groups" in _refused("dana_optim_pack_hyper", hp, lp, ops.OPTIM_MAX_GROUPS + 1, 1.0, 0.0, 0.0, 0.0, 1)
    assert "step" in _refused("dana_optim_pack_hyper", hp, lp, 2, 1.0, 0.0, 0.9, 0.999, 0)
    assert "grad_scale" in _refused("dana_optim_pack_hyper", hp, lp, 2, 0.0, 0.0, 0.9, 0.999, 1)
    assert not h.any()  # a refused call writes nothing
    with pytest.raises(_lib.DanaError, match="clip_norm"):
        ops.optim_pack_hyper(torch.zeros(8), [0.01, 0.02], 1.0, clip_norm=-0.5)

    t = torch.zeros(ops.OPTIM_HYPER_FLOATS)
    for step in (1, 2, 10, 1000, 100000):
        ops.optim_pack_hyper(t, [0.01, 0.02], 1.0 / 8, clip_norm=10.0, betas=(0.9, 0.999), step=step)
        got = t.numpy()
        # the layout of include/dana_hip.h; the rates and 1 / world are the floats a launch parameter would have carried
        assert got[0] == np.float32(0.01) and got[1] == np.float32(0.02) and got[2] == 0 and got[3] == 0
        assert got[4] == np.float32(0.125) and got[5] == np.float32(10.0)
        # dana_adam: 1.0 - pow((double)beta, step) with the FLOAT beta, rounded to float
        for slot, beta in ((6, 0.9), (7, 0.999)):
            assert got[slot] == np.float32(1.0 - float(np.float32(beta)) ** step), (step, slot)
    ops.optim_pack_hyper(t, [0.5], 1.0, step=7)  # SGD: no betas -> the bias corrections are 1
    assert t[6] == 1.0 and t[7] == 1.0 and t[5] == 0.0 and t[1] == 0.0


def test_trainer_rejects_negative_clip_norm():
    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(4, 4)

    for bad in (-1.0, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="clip_norm"):
            Trainer(Tiny(), 0.01, clip_norm=bad)
