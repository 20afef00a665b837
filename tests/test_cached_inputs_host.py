"""`dana_amd.cached_inputs` on the host (no device, no call into the library): the index validator through its four
callers, the reader of a forward's inputs on stub handles, and the host-mirrored device index on a CPU "device"."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dana_amd import _lib
from dana_amd import cached_inputs as CI

N, SHOT = 4, 2  # sets of the cache / rows of the banks; shots per set


@pytest.fixture(autouse=True)
def no_capture(monkeypatch):
    """an index write asks torch whether the current stream is capturing, which needs a GPU to answer: here it is not"""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)


class _Model:
    """what a handle asks of its model"""
    training, n_way, n_shot = False, 1, SHOT

    def _cache_layout(self, shot, sup_map):
        return dict(kp=(shot * 4, 2))

    def _cache_shot_blocks(self, sup_map):
        return dict(kp=(1, 8))

    def _state(self, dev):
        return ("state", str(dev))

    _cache_state = _bank_state = _qbank_state = _state


MODEL = _Model()


def _cache():
    return CI.SupportCache(MODEL, dict(kp=torch.zeros(N, SHOT * 8)), SHOT, (2, 2), None, MODEL._state("cpu"), "cpu")


def _qbank():
    return CI.QueryBank(MODEL, torch.zeros(N, 1, 1), (16, 16), (1, 1), MODEL._state("cpu"), "cpu")


def _select(index):
    cache = _cache()
    cache.select(index)
    return cache._sel


CALLERS = {
    "select": _select,
    "sweep": lambda index: list(_cache().sweep(index).classes),
    "episode": lambda index: CI.resolve_bank_episode(index, N, None, 1, SHOT).tolist(),
    "batch": lambda index: CI.resolve_query_batch(index, N).tolist(),
}

# caller, index -> the exception and what its text must name; None: accepted, with these values
ROWS = [
    # float dtype: refused where an index is an array; select / sweep take anything int() accepts
    ("select", torch.tensor([1.0, 2.0]), None, [1, 2]),
    ("sweep", np.array([3.0, 0.0]), None, [3, 0]),
    ("episode", np.array([[0.0, 1.0]]), ValueError, ["float64"]),
    ("batch", torch.tensor([0.0, 1.0]), ValueError, ["float32"]),
    # bool dtype
    ("select", [True, False], None, [1, 0]),
    ("sweep", torch.tensor([True]), None, [1]),
    ("episode", np.array([[True, False]]), ValueError, ["bool"]),
    ("batch", [True, False], ValueError, ["bool"]),
    # empty
    ("select", [], ValueError, ["empty selection"]),
    ("sweep", torch.zeros(0, dtype=torch.int64), ValueError, ["empty class list"]),
    ("episode", np.zeros((0, SHOT), dtype=np.int64), ValueError, ["(0, 2)"]),
    ("batch", np.zeros((0,), dtype=np.int64), ValueError, ["(0,)"]),
    # negative
    ("select", [0, -1, 2, -3], IndexError, ["[-1, -3]", "[0, 4)"]),
    ("sweep", [-2], IndexError, ["[-2]", "[0, 4)"]),
    ("episode", [[0, -1], [-5, -1]], IndexError, ["[-5, -1]", "[0, 4)"]),
    ("batch", [3, -1], IndexError, ["[-1]", "[0, 4)"]),
    # too large
    ("select", [4, 0, 7], IndexError, ["[4, 7]", "[0, 4)"]),
    ("sweep", torch.tensor([9, 3]), IndexError, ["[9]", "[0, 4)"]),
    ("episode", np.array([[3, 4], [11, 4]]), IndexError, ["[4, 11]", "[0, 4)"]),
    ("batch", torch.tensor([4, 4, 1]), IndexError, ["[4]", "[0, 4)"]),
    # wrong shape (select / sweep flatten what they are given: they have no shape rule besides "not empty")
    ("episode", [0, 1], ValueError, ["way*shot = 2", "(2,)"]),
    ("episode", [[0, 1, 2]], ValueError, ["way*shot = 2", "(1, 3)"]),
    ("batch", [[0, 1], [2, 3]], ValueError, ["[B]", "(2, 2)"]),
    ("select", torch.tensor([[0, 1], [2, 3]]), None, [0, 1, 2, 3]),
]


@pytest.mark.parametrize("caller,index,exc,expect", ROWS, ids=["%s-%d" % (r[0], i) for i, r in enumerate(ROWS)])
def test_index_validation_through_every_caller(caller, index, exc, expect):
    if exc is None:
        assert CALLERS[caller](index) == expect
        return
    with pytest.raises(exc) as err:
        CALLERS[caller](index)
    assert type(err.value) is exc
    for text in expect:
        assert text in str(err.value)


def test_a_fixed_batch_size_is_part_of_the_shape_rule():
    with pytest.raises(ValueError, match=r"\[3, way\*shot = 2\]"):
        CI.resolve_bank_episode([[0, 1]], N, 3, 1, SHOT)
    with pytest.raises(ValueError, match=r"must be \[3\]"):
        CI.resolve_query_batch([0, 1], N, 3)
    # a wrong shape is reported before an entry out of range, a wrong dtype before both
    with pytest.raises(ValueError, match="must be"):
        CI.resolve_query_batch([[9]], N)
    with pytest.raises(ValueError, match="integers"):
        CI.resolve_query_batch([[9.5]], N)


def _stub(cls, **attrs):
    handle = object.__new__(cls)  # (no bank, no model: the reader looks at types only)
    for k, v in attrs.items():
        setattr(handle, k, v)
    return handle


def _supports():
    cache = _cache()
    sweep = cache.sweep([2, 0])
    return {"images": (torch.zeros(1, 2, 3, 4, 4), None, None, None), "cache": (cache, cache, None, None),
            "sweep": (sweep, cache, sweep, None), "episode": (_stub(CI.BankEpisode),) + (None, None, "self")}


@pytest.mark.parametrize("query", ["images", "qbatch"])
@pytest.mark.parametrize("support", ["images", "cache", "sweep", "episode"])
def test_read_inputs(query, support):
    im_data = torch.zeros(3, 3, 8, 8) if query == "images" else _stub(
        CI.QueryBatch, B=5, bank=SimpleNamespace(device=torch.device("cpu")))
    given, cache, sweep, episode = _supports()[support]
    got = CI.read_inputs(im_data, given)
    assert got.qbatch is (im_data if query == "qbatch" else None)
    assert got.cache is cache and got.sweep is sweep
    assert got.episode is (given if episode == "self" else None)
    assert tuple(got) == (got.qbatch, got.cache, got.sweep, got.episode)
    assert CI.query_device(im_data) == torch.device("cpu")
    assert CI.query_batch_size(im_data) == (3 if query == "images" else 5)


def test_read_inputs_without_a_fifth_argument():
    inputs = [torch.zeros(1, 3, 8, 8)] * 4  # (the plain Faster R-CNN takes four)
    assert tuple(CI.read_inputs(inputs[0], *inputs[4:5])) == (None, None, None, None)


REFUSAL = "the index changed inside a recording"


def _write(buf, held, rows, **kw):
    return CI.write_device_index(buf, held, rows, torch.device("cpu"), REFUSAL, **kw)


@pytest.mark.parametrize("rows,other,kw", [
    (np.array([[1, 2], [3, 0]], dtype=np.int32), np.array([[1, 2], [3, 1]], dtype=np.int32), {}),
    ([1, 2, 3], [1, 2, 0], dict(grow=(N, (), 0))),
    ([[0, -1], [1, 0]], [[0, 1], [1, 0]], dict(grow=(N, (SHOT,), -1))),
], ids=["bank", "cache-index", "cache-views"])
def test_device_index_uploads_only_what_changed(rows, other, kw, monkeypatch):
    buf, held = _write(None, None, rows, **kw)
    flat = np.asarray(rows).reshape(-1).tolist()
    assert buf.dtype == torch.int32 and buf.reshape(-1)[:len(flat)].tolist() == flat
    if kw:  # one growing buffer: capacity max(len, least rows, 16), the rest filled
        assert buf.shape == (16,) + kw["grow"][1] and set(buf[len(rows):].reshape(-1).tolist()) == {kw["grow"][2]}
    else:
        assert buf.shape == (4,)
    # equal mirror: no second upload -- a value scribbled into the buffer survives, the objects are the same
    buf.fill_(7)
    same = rows.copy() if isinstance(rows, np.ndarray) else [list(r) if isinstance(r, list) else r for r in rows]
    buf2, held2 = _write(buf, held, same, **kw)
    assert buf2 is buf and held2 is held and set(buf.reshape(-1).tolist()) == {7}
    # under a recorder: an equal index passes, a changed one is refused and nothing is written
    monkeypatch.setattr(_lib, "RECORDER", object())
    assert _write(buf, held, same, **kw)[0] is buf
    with pytest.raises(RuntimeError, match=REFUSAL):
        _write(buf, held, other, **kw)
    assert set(buf.reshape(-1).tolist()) == {7}
    monkeypatch.setattr(_lib, "RECORDER", None)
    buf3, held3 = _write(buf, held, other, **kw)
    assert buf3 is buf and buf.reshape(-1)[:len(flat)].tolist() == np.asarray(other).reshape(-1).tolist()
    assert np.array_equal(held3, other)


def test_the_mirror_is_a_copy_of_the_callers_array():
    rows = np.array([0, 1], dtype=np.int32)
    buf, held = _write(None, None, rows)
    rows[0] = 3  # (the caller goes on writing its array: the mirror must not follow)
    buf.fill_(7)
    assert _write(buf, held, rows)[0].tolist() == [3, 1]


def test_a_bank_keeps_one_index_buffer_per_key():
    bank = _qbank()
    two, three = bank.batch([0, 1]), bank.batch([3, 2, 1])
    b2, b3 = bank._index[2], bank._index[3]
    assert b2 is not b3 and b2.tolist() == [0, 1] and b3.tolist() == [3, 2, 1]
    two.set([1, 1])
    other = bank.batch([2, 3])  # (another batch of that size shares the buffer)
    assert bank._index[2] is b2 and bank._index[3] is b3 and b2.tolist() == [2, 3]
    two._check(MODEL, "cpu")    # (... and a forward of the first one uploads its index again)
    assert bank._index[2] is b2 and b2.tolist() == [1, 1] and other.index.tolist() == [2, 3]
    sbank = CI.SupportBank(MODEL, torch.zeros(N, 1, 1), torch.zeros(N, 1, 1), (1, 1), None, MODEL._state("cpu"), "cpu")
    ep = sbank.episode([[0, 1], [2, 3]])
    buf = sbank._index[(2, 2)]
    ep.set([[3, 3], [0, 0]])
    assert sbank._index[(2, 2)] is buf and buf.tolist() == [3, 3, 0, 0] and list(sbank._index) == [(2, 2)]


def test_a_cache_keeps_one_growing_index_buffer():
    cache = _cache()
    cache.select([1, 0])
    buf = cache._index
    cache.select([3] * 16)
    assert cache._index is buf and buf.tolist() == [3] * 16
    cache.select([2] * 17)  # (past the capacity: a new buffer, which a recorded program notices by identity)
    assert cache._index is not buf and cache._index.shape == (17,)
    cache.select([0, 1], shots=[[1], [0, 1]])
    assert cache._sel_views == [(1,), (0, 1)] and cache._view[:2].tolist() == [[1, -1], [0, 1]] and cache._view.shape == (16, 2)


@pytest.mark.parametrize("make,noun,advice", [(_cache, "SupportCache", "re-encode the supports"),
                                              (_qbank, "QueryBank", "re-encode the images")])
def test_one_staleness_check_words_every_handle(make, noun, advice, monkeypatch):
    handle = make()
    handle._check(MODEL, "cpu")
    with pytest.raises(RuntimeError, match="this %s was encoded by another model: %s with this one" % (noun, advice)):
        handle._check(_Model(), "cpu")
    with pytest.raises(RuntimeError, match="this %s lives on cpu, the .* on meta: %s there" % (noun, advice)):
        handle._check(MODEL, "meta")
    monkeypatch.setattr(_Model, handle._STATE, lambda self, dev: ("moved",))
    with pytest.raises(RuntimeError, match=r"the model changed since %s \(.*\): %s$" % (handle._ENCODER, advice)):
        handle._check(MODEL, "cpu")
