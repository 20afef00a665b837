"""`dana.resolve_query_batch`: the host-side validation of a query-bank batch's index, and the C declaration of the gather it
feeds (no device)."""
import numpy as np
import pytest
import torch

from dana_amd import _lib
from dana_amd.dana import resolve_query_batch


def test_accepted_forms():
    for B in (1, 2, 5):
        idx = (np.arange(B) * 3) % 4
        for given in (idx.tolist(), idx.astype(np.int32), idx.astype(np.int64), torch.from_numpy(idx)):
            out = resolve_query_batch(given, 4, B)
            assert isinstance(out, np.ndarray) and out.dtype == np.int32 and out.flags["C_CONTIGUOUS"]
            assert out.shape == (B,) and np.array_equal(out, idx)
    # B None: any batch size
    assert resolve_query_batch([3, 0, 2], 4).shape == (3,)
    # a non-contiguous view comes back contiguous
    wide = np.arange(8) % 5
    out = resolve_query_batch(wide[::2], 5, 4)
    assert out.flags["C_CONTIGUOUS"] and np.array_equal(out, wide[::2])


def test_the_result_is_a_fresh_int32_copy():
    idx = np.array([0, 1, 2], dtype=np.int32)  # (already what comes back: still not the caller's array)
    out = resolve_query_batch(idx, 4, 3)
    assert out is not idx and not np.shares_memory(out, idx)
    idx[0] = 3
    assert out[0] == 0


def test_repeats_and_any_order_are_kept():
    idx = [3, 3, 0, 3, 1]
    assert resolve_query_batch(idx, 4, 5).tolist() == idx


@pytest.mark.parametrize("index", [
    [[0, 1]],                      # 2-D
    3,                             # a scalar
    [0, 1, 2],                     # B = 2 expected
    np.zeros((0,), dtype=np.int64),  # no image
    [0.0, 1.0],                    # floats
    [True, False],                 # booleans
], ids=["2d", "scalar", "batch", "empty", "float", "bool"])
def test_value_errors(index):
    with pytest.raises(ValueError):
        resolve_query_batch(index, 4, 2)


def test_a_device_tensor_is_a_value_error():
    class Dev(torch.Tensor):  # (this test runs without a GPU: a stand-in whose is_cuda is True takes the same branch)
        @property
        def is_cuda(self):
            return True

    t = torch.zeros((2,), dtype=torch.int64).as_subclass(Dev)
    with pytest.raises(ValueError, match="host"):
        resolve_query_batch(t, 4, 2)


@pytest.mark.parametrize("bad", [-1, 4, 1 << 20])
def test_index_errors(bad):
    with pytest.raises(IndexError, match=r"\[0, 4\)"):
        resolve_query_batch([0, bad], 4, 2)
    # ... and a value that would wrap to a valid row as int32 is still outside
    with pytest.raises(IndexError):
        resolve_query_batch(np.array([(1 << 32) + 1], dtype=np.int64), 4, 1)


def test_the_header_declares_the_gather_with_c_scalars_and_raw_pointers():
    protos = _lib.parse_header()
    assert "dana_qbank_gather" in protos
    ret, args = protos["dana_qbank_gather"]
    assert ret == "int"
    assert args == [("const float*", "maps"), ("const int*", "index"), ("int", "n_bank"), ("int", "B"), ("int", "rows"),
                    ("int", "channels"), ("float*", "out"), ("int", "ld_out"), ("dana_stream_t", "stream")]


def test_the_gather_reports_argument_errors_without_a_gpu():
    L = _lib.lib()
    for n_bank, B, rows, C, ld in ((4, 2, 8, 6, 8),      # channels no multiple of 4
                                   (4, 2, 8, 8, 10),     # ld_out no multiple of 4
                                   (4, 2, 8, 8, 4),      # ld_out < channels
                                   (4, 65536, 8, 8, 8),  # more images than grid rows
                                   (-1, 2, 8, 8, 8)):
        with pytest.raises(_lib.DanaError, match="bad shape"):
            L.call("dana_qbank_gather", None, None, n_bank, B, rows, C, None, ld, None)
    with pytest.raises(_lib.DanaError, match="null pointer"):
        L.call("dana_qbank_gather", None, None, 4, 2, 8, 8, None, 8, None)
    with pytest.raises(_lib.DanaError, match="16-byte aligned"):
        L.call("dana_qbank_gather", 4096 + 4, 4096, 4, 2, 8, 8, 8192, 8, None)
    with pytest.raises(_lib.DanaError, match="16-byte units per image"):  # (the kernel numbers an image's units in 32 bits)
        L.call("dana_qbank_gather", 4096, 4096, 4, 2, (1 << 31) - 1, 8, 8192, 8, None)
    # an empty batch or an empty image is a no-op
    L.call("dana_qbank_gather", None, None, 4, 0, 8, 8, None, 8, None)
    L.call("dana_qbank_gather", None, None, 4, 2, 0, 8, None, 8, None)
