"""CPU suite: `dana.resolve_shot_views`, the pure function that turns the `shots=` spec of `SupportCache.select` /
`SupportCache.sweep` into one ordered tuple of shot indices per problem (no device involved), and the declarations of the
three entry points the shot views add."""
import pytest
import torch

from dana_amd import _lib
from dana_amd.dana import resolve_shot_views

COUNTS = (3, 2, 1, 3)  # real shots of sets 0..3 (shot = 3; sets 1 and 2 are ragged)


def test_default_views_come_from_the_counts():
    sets, views = resolve_shot_views(None, [0, 1, 2, 1], COUNTS)
    assert sets == [0, 1, 2, 1]
    assert views == [(0, 1, 2), (0, 1), (0,), (0, 1)]


def test_int_spec_is_the_nested_k_shot_subset():
    assert resolve_shot_views(1, [0, 1, 2], COUNTS)[1] == [(0,), (0,), (0,)]
    assert resolve_shot_views(2, [0, 1], COUNTS)[1] == [(0, 1), (0, 1)]
    assert resolve_shot_views(3, [0, 3], COUNTS)[1] == [(0, 1, 2), (0, 1, 2)]
    with pytest.raises(IndexError):
        resolve_shot_views(2, [0, 2], COUNTS)  # set 2 has one shot
    with pytest.raises(ValueError):
        resolve_shot_views(0, [0], COUNTS)


def test_sequence_spec_one_for_all_and_one_per_problem():
    # a flat sequence of ints is ONE view, for every problem; order is kept
    assert resolve_shot_views([2, 0], [0, 3], COUNTS)[1] == [(2, 0), (2, 0)]
    assert resolve_shot_views((1,), [0, 1], COUNTS)[1] == [(1,), (1,)]
    assert resolve_shot_views(torch.tensor([1, 0]), [0, 1], COUNTS)[1] == [(1, 0), (1, 0)]
    # a sequence holding a sequence (or None) is one spec per problem; each of them may be None, an int or a sequence
    assert resolve_shot_views([(2,)], [0], COUNTS)[1] == [(2,)]
    assert resolve_shot_views([(1,), None, 1, [2, 0]], [0, 1, 2, 3], COUNTS)[1] == [(1,), (0, 1), (0,), (2, 0)]
    with pytest.raises(ValueError, match="per-problem"):
        resolve_shot_views([(0,), (1,)], [0, 1, 3], COUNTS)


def test_each_expands_every_class_into_its_one_shot_views():
    sets, views = resolve_shot_views("each", [3, 0], COUNTS, each=True)
    assert sets == [3, 3, 3, 0, 0, 0]  # problem c*S + s = shot s of class c
    assert views == [(0,), (1,), (2,), (0,), (1,), (2,)]
    sets, views = resolve_shot_views("each", [1], COUNTS, each=True)
    assert (sets, views) == ([1, 1], [(0,), (1,)])
    with pytest.raises(ValueError, match="different shot counts"):
        resolve_shot_views("each", [0, 1], COUNTS, each=True)
    with pytest.raises(ValueError):
        resolve_shot_views("each", [0], COUNTS)  # a selection has no "each"
    with pytest.raises(ValueError):
        resolve_shot_views("all", [0], COUNTS, each=True)


def test_errors():
    with pytest.raises(ValueError, match="empty"):
        resolve_shot_views([()], [0], COUNTS)
    with pytest.raises(ValueError, match="empty"):
        resolve_shot_views([], [0], COUNTS)
    with pytest.raises(ValueError, match="twice"):
        resolve_shot_views([1, 1], [0], COUNTS)
    with pytest.raises(ValueError, match="twice"):
        resolve_shot_views([(0, 2, 0)], [0], COUNTS)
    with pytest.raises(IndexError):
        resolve_shot_views([(2,)], [1], COUNTS)  # shot 2 of the 2-shot set
    with pytest.raises(IndexError):
        resolve_shot_views([3], [0], COUNTS)
    with pytest.raises(IndexError):
        resolve_shot_views([-1], [0], COUNTS)
    with pytest.raises(ValueError):
        resolve_shot_views([0.5], [0], COUNTS)
    with pytest.raises(ValueError):
        resolve_shot_views([True], [0], COUNTS)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="device"):
            resolve_shot_views(torch.tensor([0]).cuda(), [0], COUNTS)


def test_device_tensor_spec_is_refused_without_a_device():
    class FakeCuda(torch.Tensor):  # (is_cuda is all the resolver looks at before it refuses)
        is_cuda = True

    with pytest.raises(ValueError, match="device"):
        resolve_shot_views(torch.tensor([0]).as_subclass(FakeCuda), [0], COUNTS)


def test_new_entry_points_are_declared():
    protos = _lib.parse_header()
    g = protos["dana_gather_shot_blocks"][1]
    assert [n for _, n in g] == ["src_ptrs", "dst_ptrs", "rows", "block_bytes", "n_tensors", "index", "view", "w", "n_sets",
                                 "shot", "m", "P", "stream"]
    for name, ref in (("dana_attn_softmax_unary_w", "dana_attn_softmax_unary"),
                      ("dana_attn_softmax_unary_sweep_w", "dana_attn_softmax_unary_sweep")):
        args, ref_args = protos[name][1], protos[ref][1]
        # the scalar out_scale gives way to (seg_scale, its per-problem stride); everything else is the same
        i = [n for _, n in ref_args].index("out_scale")
        assert args[:i] == ref_args[:i] and args[i + 2:] == ref_args[i + 1:]
        assert args[i][0] == "const float*" and args[i][1] == "seg_scale" and args[i + 1][0] == "long"
