"""`dana.resolve_bank_episode`: the host-side validation of a support-bank episode's index (no device, no library)."""
import numpy as np
import pytest
import torch

from dana_amd.dana import resolve_bank_episode


def test_accepted_shapes_and_types():
    for B, way, shot in ((1, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 3)):
        idx = np.arange(B * way * shot).reshape(B, way * shot) % 5
        for given in (idx, idx.tolist(), torch.from_numpy(idx), idx.astype(np.int64), idx.astype(np.uint8)):
            out = resolve_bank_episode(given, 5, B, way, shot)
            assert isinstance(out, np.ndarray) and out.dtype == np.int32 and out.flags["C_CONTIGUOUS"]
            assert out.shape == (B, way * shot) and np.array_equal(out, idx)
    # B None: any batch size
    assert resolve_bank_episode([[0, 1], [2, 3], [4, 0]], 5, None, 2, 1).shape == (3, 2)
    # a non-contiguous view comes back contiguous
    wide = np.arange(16).reshape(2, 8) % 6
    out = resolve_bank_episode(wide[:, ::2], 6, 2, 2, 2)
    assert out.flags["C_CONTIGUOUS"] and np.array_equal(out, wide[:, ::2])


def test_the_result_is_a_copy():
    idx = np.array([[0, 1, 2, 3]], dtype=np.int32)
    out = resolve_bank_episode(idx, 4, 1, 2, 2)
    idx[0, 0] = 3
    assert out[0, 0] == 0


def test_positives_first_layout_is_preserved():
    # image b's row is [its shot positives | the negatives], exactly as given: nothing is sorted or regrouped
    idx = [[5, 1, 0, 3], [2, 4, 5, 1]]
    out = resolve_bank_episode(idx, 6, 2, 2, 2)
    assert out.tolist() == idx
    assert out[:, :2].tolist() == [[5, 1], [2, 4]] and out[:, 2:].tolist() == [[0, 3], [5, 1]]


def test_repeats_are_kept():
    # the same exemplar twice in a row, and as a positive of one image and a negative of the other
    idx = [[3, 3, 0, 0], [0, 1, 3, 3]]
    assert resolve_bank_episode(idx, 4, 2, 2, 2).tolist() == idx


@pytest.mark.parametrize("index", [
    [0, 1, 2, 3],                         # flat
    [[0, 1, 2]],                          # way*shot = 4 columns expected
    [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3]],  # B = 2 expected
    [[[0, 1, 2, 3]], [[0, 1, 2, 3]]],     # 3-D
    np.zeros((0, 4), dtype=np.int64),     # no image
    [[0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0, 3.0]],  # floats
    [[True, False, True, False], [True, False, True, False]],  # booleans
], ids=["flat", "columns", "batch", "3d", "empty", "float", "bool"])
def test_value_errors(index):
    with pytest.raises(ValueError):
        resolve_bank_episode(index, 4, 2, 2, 2)


def test_a_device_tensor_is_a_value_error():
    class Dev(torch.Tensor):  # (this test runs without a GPU: a stand-in whose is_cuda is True takes the same branch)
        @property
        def is_cuda(self):
            return True

    t = torch.zeros((2, 4), dtype=torch.int64).as_subclass(Dev)
    with pytest.raises(ValueError, match="host"):
        resolve_bank_episode(t, 4, 2, 2, 2)


@pytest.mark.parametrize("bad", [-1, 4, 1 << 20])
def test_index_errors(bad):
    idx = [[0, 1, 2, 3], [0, 1, bad, 3]]
    with pytest.raises(IndexError, match=r"\[0, 4\)"):
        resolve_bank_episode(idx, 4, 2, 2, 2)
    # ... and a value that would wrap to a valid row as int32 is still outside
    with pytest.raises(IndexError):
        resolve_bank_episode(np.array([[(1 << 32) + 1, 0, 0, 0]], dtype=np.int64), 4, 1, 2, 2)
