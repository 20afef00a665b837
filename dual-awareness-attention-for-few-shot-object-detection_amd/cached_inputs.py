"""What a forward takes in place of images: the handles of encoded inputs, and the host-side code they share.

  SupportCache / ClassSweep   model.encode_supports: the support side of C sets, for eval forwards (5th argument)
  SupportBank / BankEpisode   model.encode_support_bank: support maps of a pool, for training over a frozen trunk (5th)
  QueryBank / QueryBatch      model.encode_query_bank: query trunk maps of a pool (1st argument)

A leaf module: it imports ops, _lib and config, never a model; a handle reaches its model's `_*_state`, `_cache_layout` and
`_cache_shot_blocks` through the model object it was encoded by. dana.py re-exports every name here.
(`SupportCache.nbytes` is a property, the banks' `nbytes` a method: public API, left as it is.)"""
import weakref
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import ops
from .config import cfg


def active_recording():
    """inside a launch-program recording or a hipGraph capture: what a replay points at must not be (re)made here"""
    return _lib.RECORDER is not None or torch.cuda.is_current_stream_capturing()


class _Encoded:
    """A handle over tensors a model encoded: it remembers the model, the device and `getattr(model, _STATE)(dev)` of that
    moment, and `_check` refuses a forward after any of them changed. The subclasses say in data what the messages name."""

    def _check(self, model, dev):
        noun = type(self).__name__
        if self._model() is not model:
            raise RuntimeError("this %s was encoded by another model: %s with this one" % (noun, self._ADVICE))
        if torch.device(dev) != self.device:
            raise RuntimeError("this %s lives on %s, the %s on %s: %s there" % (noun, self.device, self._FORWARD, dev, self._ADVICE))
        if getattr(model, self._STATE)(dev) != self._state:
            raise RuntimeError("the model changed since %s (%s): %s" % (self._ENCODER, self._DEPENDS, self._ADVICE))


def host_index(index, n, device_tensor, wrong_shape, outside, wrong_dtype=None):
    """The rules of every index a caller hands to a handle, host only: a sequence, a numpy array or a CPU tensor of integers
    in [0, n). The callers bring their wording and their shape rule: device_tensor, the ValueError text for a device tensor;
    wrong_dtype, the ValueError text (%s: the dtype) for a bool or non-integer array -> the index as an array -- None
    (SupportCache.select / sweep): anything int() accepts, flattened -> a list of ints; wrong_shape(values) -> the ValueError
    text or None (an empty index is a wrong shape); outside, the IndexError text (%s: the offenders)."""
    if torch.is_tensor(index):
        if index.is_cuda:
            raise ValueError(device_tensor)
        index = index.numpy() if wrong_dtype is not None else index.reshape(-1).tolist()
    if wrong_dtype is None:
        values = [int(i) for i in index]
    else:
        values = np.asarray(index)
        if values.dtype == np.bool_ or not np.issubdtype(values.dtype, np.integer):
            raise ValueError(wrong_dtype % values.dtype)
    shape_text = wrong_shape(values)
    if shape_text is not None:
        raise ValueError(shape_text)
    if wrong_dtype is None:
        bad = [i for i in values if i < 0 or i >= n]
    else:
        bad = sorted(set(int(v) for v in values[(values < 0) | (values >= int(n))].reshape(-1)))[:8]
    if bad:
        raise IndexError(outside % (bad,))
    return values


def write_device_index(buf, held, rows, device, refusal, grow=None):
    """rows into the device int32 index a gather reads, mirrored on the host -> (buf, held) for the owner to keep: nothing to
    do when the mirror is equal; RuntimeError(refusal) inside a recording or capture, whose replay reads the buffer; else
    allocate (once: a recording points at the buffer), upload, remember.
    grow None (the banks): rows is an int32 array, the buffer has its size (the owner keeps one per key), pinned upload.
    grow (least rows, row shape, fill) (SupportCache): rows is a list; ONE buffer of max(len(rows), least rows, 16) rows,
    which ProgramDAnA compares by identity after a recording; a plain copy from a pageable tensor."""
    if held is not None and (held == rows if grow is not None else np.array_equal(held, rows)):
        return buf, held
    if active_recording():
        raise RuntimeError(refusal)
    if grow is not None:
        least, row, fill = grow
        if buf is None or buf.size(0) < len(rows):
            buf = torch.full((max(len(rows), least, 16),) + tuple(row), fill, dtype=torch.int32, device=device)
        buf[:len(rows)].copy_(torch.tensor(rows, dtype=torch.int32))
        return buf, list(rows)
    if buf is None:
        buf = torch.zeros((rows.size,), dtype=torch.int32, device=device)
    # one asynchronous copy on the current stream, as Trainer.upload_hyper's: a pageable source would hold the host
    # until the stream has drained, once per iteration. The pinned block comes from torch's host allocator, which
    # does not hand it out again before the copy that read it has finished. The gather runs behind an event of this
    # stream (the forward's inputs_ready), and every side stream of a step is joined before the next set()
    staged = torch.empty((rows.size,), dtype=torch.int32, pin_memory=buf.is_cuda)
    staged.copy_(torch.from_numpy(rows).reshape(-1))
    buf.copy_(staged, non_blocking=True)
    return buf, rows.copy()


ForwardInputs = namedtuple("ForwardInputs", "qbatch cache sweep episode")


def read_inputs(im_data, support_ims=None):
    """The handles among a forward's 1st and 5th argument (`read_inputs(inputs[0], *inputs[4:5])` of an argument list) ->
    (qbatch, cache, sweep, episode), each None when the forward was given images there. A ClassSweep brings its cache."""
    qbatch = im_data if isinstance(im_data, QueryBatch) else None
    sweep = support_ims if isinstance(support_ims, ClassSweep) else None
    cache = sweep.cache if sweep is not None else (support_ims if isinstance(support_ims, SupportCache) else None)
    episode = support_ims if isinstance(support_ims, BankEpisode) else None
    return ForwardInputs(qbatch, cache, sweep, episode)


def query_device(im_data):
    """the device of a forward's 1st argument: query images or a QueryBatch"""
    return im_data.bank.device if isinstance(im_data, QueryBatch) else im_data.device


def query_batch_size(im_data):
    """B of a forward's 1st argument: query images or a QueryBatch"""
    return im_data.B if isinstance(im_data, QueryBatch) else im_data.size(0)


def check_cached_forward(model, dev, cache, sweep):
    """the rules of a forward from a SupportCache (or a ClassSweep of one), DAnA's and the siblings' alike"""
    if model.training:
        raise RuntimeError("a SupportCache serves eval-mode forwards only (model.eval()); training recomputes the "
                           "support side from support images")
    cache._check(model, dev)
    if sweep is not None and cfg.POOLING_MODE != "align":
        raise NotImplementedError("a ClassSweep forward pools with RoIAlign (the grouped NHWC kernel); POOLING_MODE "
                                  "'%s' is not supported there: sweep with cache.select per class instead" % cfg.POOLING_MODE)


def _is_shot_spec_leaf(x):
    return x is None or isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def resolve_shot_views(shots, sets, counts, each=False):
    """The shot views of a call, host only (no device): -> (sets, views), views[p] an ordered tuple of distinct shot
    indices of set sets[p], each < counts[sets[p]] (the set's real shots).
    shots: ONE spec for every problem -- None (all real shots of the set), an int k (shots 0..k-1: the nested K-shot
    subsets) or a flat sequence of shot indices -- or a sequence of len(sets) specs, one per problem (recognised by an
    element that is itself None or a sequence; per-problem ints k go as range(k)). "each" (each=True callers: a sweep)
    expands every listed set into its S one-shot views, problem c*S + s = shot s of sets[c]; the listed sets must have
    equal counts. ValueError: empty view, duplicates, device tensors, a bad spec; IndexError: a shot >= counts[set]."""
    sets = [int(c) for c in sets]

    def host_list(x):
        if torch.is_tensor(x):
            if x.is_cuda:
                raise ValueError("shots= takes host values (ints, sequences or CPU tensors), not device tensors")
            return x.reshape(-1).tolist()
        return x

    def one(spec, c):
        n = int(counts[c])
        spec = host_list(spec)
        if spec is None:
            return tuple(range(n))
        if _is_shot_spec_leaf(spec):
            k = int(spec)
            if k < 1:
                raise ValueError("shots=%d: a view needs at least one shot" % k)
            if k > n:
                raise IndexError("shots=%d: set %d has %d shots" % (k, c, n))
            return tuple(range(k))
        if isinstance(spec, str) or not hasattr(spec, "__iter__"):
            raise ValueError("shots: %r is not a view (None, an int or a sequence of shot indices)" % (spec,))
        view = []
        for v in spec:
            if v is None or not _is_shot_spec_leaf(v):
                raise ValueError("shots: %r is not a shot index" % (v,))
            view.append(int(v))
        if not view:
            raise ValueError("shots: empty view for set %d" % c)
        if len(set(view)) != len(view):
            raise ValueError("shots: view %s of set %d names a shot twice" % (view, c))
        bad = [v for v in view if v < 0 or v >= n]
        if bad:
            raise IndexError("shots: %s outside the %d shots of set %d" % (bad, n, c))
        return tuple(view)

    shots = host_list(shots)
    if isinstance(shots, str):
        if shots != "each" or not each:
            raise ValueError("shots=%r: %s" % (shots, "only a sweep takes shots='each'" if shots == "each" else
                                               "the only string spec is 'each'"))
        ns = sorted({int(counts[c]) for c in sets})
        if len(ns) != 1:
            raise ValueError("shots='each': the listed sets have different shot counts %s; sweep them by count" % ns)
        return [c for c in sets for _ in range(ns[0])], [(s_,) for _ in sets for s_ in range(ns[0])]
    per_problem = (not _is_shot_spec_leaf(shots) and hasattr(shots, "__iter__")
                   and any(v is None or (hasattr(v, "__iter__") and not isinstance(v, str)) for v in shots))
    if per_problem:
        shots = list(shots)
        if len(shots) != len(sets):
            raise ValueError("shots: %d per-problem specs for %d problems" % (len(shots), len(sets)))
        return sets, [one(sp, c) for sp, c in zip(shots, sets)]
    return sets, [one(shots, c) for c in sets]


class SupportCache(_Encoded):
    """The query-independent support tensors of C support sets (encode_supports), per set as the model's
    `_cache_layout` names them. DAnA:
    RPN level  kp [shot*L][d] (column mean subtracted), unary [shot][L] (softmaxed), s_t [1024][shot*L];
    RoI level  k2 [shot*49][dq], un2 [shot][49], and sw [shot*49][64] (folded S.Wt^T) or sp_pe [shot*49][1024]
               (product attention or fold_roi_attn off).
    The sibling detectors' layouts are in frcnn.py (meta), fsod.py and fgn.py.
    `model(im_data, im_info, gt_boxes, num_boxes, cache)`: query image b uses set index[b] -- `select(indices)`, else the
    identity when C == B and a broadcast when C == 1. The forward gathers the selected sets into B-batched buffers the cache
    owns (one launch, dana_gather_blocks, index read on the device: a recorded replay follows later `select` calls).
    Every tensor is `shot` independent blocks, so `select(indices, shots=)` / `sweep(classes, shots=)` serve shot VIEWS of a
    set (`resolve_shot_views`: K-shot subsets, single shots, ragged sets encoded with `num_shots=`): problems whose view is
    not range(shot) are gathered by dana_gather_shot_blocks into m-shot buffers (m = the longest view of the call; padding
    slots zeroed, w [P][m] = 1/len(view) or 0) and the query side runs with shot = m; views of unequal length scale the
    attention per segment by w (dana_attn_softmax_unary_w / _sweep_w). Needs the model's `_cache_shot_blocks`.
    The cache records what it was built under; a forward after any of it changed raises ("re-encode")."""

    _ADVICE, _STATE, _FORWARD, _ENCODER = "re-encode the supports", "_cache_state", "query", "encode_supports"
    _DEPENDS = "weights, MFMA mode, Winograd settings, attention_type, semantic_enhance, fold_roi_attn or num_shot"

    def __init__(self, model, tensors, shot, sup_map, pool, state, dev, counts=None):
        self._model = weakref.ref(model)
        self._t = {k: v for k, v in tensors.items() if v is not None}
        self.shot, self.sup_map, self.pool, self.device = shot, tuple(sup_map), pool, torch.device(dev)
        self._state = state
        self._C = next(iter(self._t.values())).size(0)
        # the shapes the forward's consumers expect, per image (B of them stacked on the first axis)
        self._shapes = model._cache_layout(shot, sup_map)
        self.FIELDS = tuple(self._shapes)
        self._sel = None        # host list of the last select(), or None
        self._index = None      # device int32 [capacity]: what dana_gather_blocks reads
        self._index_host = None  # what the device index holds
        self._bufs = {}         # B -> (gathered tensors, device tables)
        # shot views. _blocks: name -> (rows, floats per shot block) of a set's [rows][shot][block] tensor, or None when
        # the model's cached tensors are not per-shot blocks (_no_shot_views says why)
        self._blocks = model._cache_shot_blocks(sup_map)
        self._no_shot_views = getattr(model, "_no_shot_views", None)
        self._counts = tuple(int(n) for n in counts) if counts is not None else (shot,) * self._C
        if len(self._counts) != self._C or any(n < 1 or n > shot for n in self._counts):
            raise ValueError("SupportCache: shot counts %s for %d sets of %d shots" % (list(self._counts), self._C, shot))
        self._sel_views = None   # the views of the last select(), or None: every selected set's real shots
        self._view = None        # device int32 [capacity][shot], -1 padded: what dana_gather_shot_blocks reads
        self._view_host = None   # what the device view table holds
        self._vbufs = {}         # (P, m) -> (gathered m-shot tensors, device tables, n tensors, w [P][m])
        self._mode = None        # the last prepared forward: None (identity views) or (m, weighted)

    def __len__(self):
        return self._C

    @property
    def shot_counts(self):
        """the number of real shots of every set (encode_supports' num_shots; `shot` each without it)"""
        return self._counts

    def _views(self, shots, sets, each=False):
        """-> (sets, views or None): `resolve_shot_views`, None when every view is the identity range(shot)"""
        if self._blocks is None and (shots is not None or self._counts != (self.shot,) * self._C):
            raise NotImplementedError("shot views (shots=, num_shots=): " + (self._no_shot_views or "not declared by the model"))
        if shots is None and all(self._counts[c] == self.shot for c in sets):
            return list(sets), None
        sets, views = resolve_shot_views(shots, sets, self._counts, each=each)
        ident = tuple(range(self.shot))
        return sets, (None if all(v == ident for v in views) else views)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self._t.values())

    def _sets(self, indices, who, empty):
        """a host sequence or a CPU tensor of set indices -> a list of ints in [0, C)"""
        return host_index(indices, self._C, "SupportCache.%s takes host indices (a sequence or a CPU tensor)" % who,
                          lambda idx: None if idx else "SupportCache.%s: empty %s" % (who, empty),
                          "SupportCache.%s: indices %%s outside [0, %d)" % (who, self._C))

    def select(self, indices, shots=None):
        """query image b of the next forwards uses support set indices[b] (a host sequence or a CPU tensor of length B),
        and of it the shots `shots` names (`resolve_shot_views`; default: all real shots). Validated on the host, written
        into the device index (and view table) the gather reads."""
        idx = self._sets(indices, "select", "selection")
        _, views = self._views(shots, idx)
        self._sel, self._sel_views = idx, views
        self._write_index(idx)
        if views is not None:
            self._write_views(views)

    def sweep(self, classes=None, shots=None):
        """-> ClassSweep: `model(im_data, im_info, gt_boxes, num_boxes, cache.sweep(classes))` runs every query image
        against each listed set (default: all C, in order). classes: a host sequence or a CPU tensor of set indices.
        shots: the view of every class, or one per class (`resolve_shot_views`); "each" expands every class into its S
        one-shot views, problem c*S + s of an image = shot s of class c (postprocess.ensemble_shots' layout)."""
        idx = self._sets(range(self._C) if classes is None else classes, "sweep", "class list")
        idx, views = self._views(shots, idx, each=True)
        return ClassSweep(self, idx, views)

    def _resolve(self, B):
        if self._sel is not None:
            if len(self._sel) != B:
                raise RuntimeError("SupportCache: %d selected sets for a batch of %d query images" % (len(self._sel), B))
            return self._sel
        if self._C == B:
            return list(range(B))
        if self._C == 1:
            return [0] * B
        raise RuntimeError("SupportCache of %d sets for a batch of %d query images: call cache.select(indices) "
                           "(without it C == B means set b for image b, C == 1 one set for every image)" % (self._C, B))

    def _write_index(self, idx):
        self._index, self._index_host = write_device_index(
            self._index, self._index_host, idx, self.device,
            "SupportCache: the selection changed inside a recording / capture: select before it", grow=(self._C, (), 0))

    def _write_views(self, views):
        """the view table of the next gather: row p = views[p], -1 padded to `shot`"""
        rows = [list(v) + [-1] * (self.shot - len(v)) for v in views]
        self._view, self._view_host = write_device_index(
            self._view, self._view_host, rows, self.device,
            "SupportCache: the shot views changed inside a recording / capture: select before it",
            grow=(self._C, (self.shot,), -1))

    def _prepare(self, B, idx=None, views=None):
        """host-side set-up of a forward that gathers B sets (selection written, gathered buffers + pointer tables
        allocated): what a recording or capture must find done. idx, views: the B set indices and their shot views (a
        class sweep's), else the selection / default for B images. Sets self._mode: None (identity views: the whole-set
        buffers) or (m, weighted)"""
        if idx is None:
            idx = self._resolve(B)
            views = self._sel_views if self._sel is not None else self._views(None, idx)[1]
        self._write_index(idx)
        if views is not None:
            return self._prepare_views(B, views)
        self._mode = None
        if (self._C == 1 and B == 1) or B in self._bufs:
            return
        if active_recording():
            raise RuntimeError("SupportCache: first B = %d forward inside a recording / capture: run one eagerly first" % B)
        names = [k for k in self.FIELDS if k in self._t]
        dst = {k: torch.empty((B,) + self._shapes[k], dtype=torch.float32, device=self.device) for k in names}
        for k in names:
            if self._t[k][0].numel() != dst[k][0].numel():
                raise RuntimeError("SupportCache: tensor %s has %d elements per set, expected %d"
                                   % (k, self._t[k][0].numel(), dst[k][0].numel()))
        tab = torch.tensor([[self._t[k].data_ptr() for k in names], [dst[k].data_ptr() for k in names],
                            [self._t[k][0].numel() * 4 for k in names]], dtype=torch.int64).to(self.device)
        self._bufs[B] = (dst, tab, len(names))

    def _prepare_views(self, P, views):
        if len(views) != P:
            raise RuntimeError("SupportCache: %d shot views for %d problems" % (len(views), P))
        self._write_views(views)
        m = max(len(v) for v in views)
        self._mode = (m, any(len(v) != m for v in views))
        if (P, m) in self._vbufs:
            return
        if active_recording():
            raise RuntimeError("SupportCache: first (P, m) = (%d, %d) view forward inside a recording / capture: run one "
                               "eagerly first" % (P, m))
        names = [k for k in self.FIELDS if k in self._t]
        shapes = self._model()._cache_layout(m, self.sup_map)
        dst = {k: torch.empty((P,) + shapes[k], dtype=torch.float32, device=self.device) for k in names}
        for k in names:
            rows, block = self._blocks[k]
            if self._t[k][0].numel() != rows * self.shot * block or dst[k][0].numel() != rows * m * block:
                raise RuntimeError("SupportCache: tensor %s is not [%d][shot][%d] per set" % (k, rows, block))
        tab = torch.tensor([[self._t[k].data_ptr() for k in names], [dst[k].data_ptr() for k in names],
                            [self._blocks[k][0] for k in names], [self._blocks[k][1] * 4 for k in names]],
                           dtype=torch.int64).to(self.device)
        self._vbufs[(P, m)] = (dst, tab, len(names), torch.zeros((P, m), dtype=torch.float32, device=self.device))

    def _gather_views(self, P, idx=None, views=None):
        """-> ({name: the P problems' tensors}, m, w): `_gather` when every view is the identity (m = shot, w None), else
        one dana_gather_shot_blocks launch into the (P, m) buffers; w [P][m] when the views' lengths differ, else None"""
        self._prepare(P, idx, views)
        if self._mode is None:
            return self._gather(P, idx, prepared=True), self.shot, None
        m, weighted = self._mode
        dst, tab, n, w = self._vbufs[(P, m)]
        _lib.lib().call("dana_gather_shot_blocks", tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(),
                        n, self._index.data_ptr(), self._view.data_ptr(), w.data_ptr(), self._C, self.shot, m, P, ops._stream())
        return {k: dst.get(k) for k in self.FIELDS}, m, (w if weighted else None)

    def _gather(self, B, idx=None, prepared=False):
        """-> {name: the B selected sets in the forward's layout}, gathered by one launch (none for one set, one image)"""
        if not prepared:
            self._prepare(B, idx)
            if self._mode is not None:
                raise NotImplementedError("shot views: " + (self._no_shot_views or "this forward does not take them"))
        if self._C == 1 and B == 1:
            return {k: (self._t[k].view(self._shapes[k]) if k in self._t else None) for k in self.FIELDS}
        dst, tab, n = self._bufs[B]
        _lib.lib().call("dana_gather_blocks", tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), n,
                        self._index.data_ptr(), self._C, B, ops._stream())
        return {k: dst.get(k) for k in self.FIELDS}


class ClassSweep:
    """SupportCache.sweep(classes): as the 5th argument of an eval-mode forward, each of the B query images runs against
    each of the C listed sets -- B*C problems p = b*C + c, each the cached forward of image b with set classes[c]
    (dana.py:87-220 per class, as inference.py:70-140 fills all_boxes[j][i]). The query trunk runs once per image; the
    outputs are laid out as the replicated call `model(im.repeat_interleave(C, 0), ..., cache)` after
    `cache.select(classes * B)` lays them out: rois [B*C, R, 5] (column 0 = p), cls_prob [B*C*R, 2], bbox_pred [B*C*R, 4]."""

    __slots__ = ("cache", "classes", "views")

    def __init__(self, cache, classes, views=None):
        # views: the shot view of every listed problem (SupportCache.sweep's shots=), None: every set whole
        self.cache, self.classes, self.views = cache, tuple(classes), (None if views is None else tuple(views))

    def __len__(self):
        return len(self.classes)

    def _index(self, B):
        """the gather index of a B-image forward: the class list repeated for every image"""
        return list(self.classes) * B

    def _views(self, B):
        """the shot views of a B-image forward, or None"""
        return None if self.views is None else list(self.views) * B

    def __repr__(self):
        return "ClassSweep(%d sets: %s)" % (len(self.classes), list(self.classes))


def _bank_rows(index, n_bank, what, forms, rows, shape_text):
    """a bank handle's host index -> a C-contiguous int32 array. what: "a bank episode" / "a query batch"; forms: the host
    forms its device-tensor refusal lists; rows: its noun in the IndexError; shape_text(arr): see `host_index`"""
    arr = host_index(index, n_bank, "%s takes a host index (%s), not a device tensor: it is validated on the host and "
                     "uploaded once" % (what, forms), shape_text, "%s: rows %%s outside [0, %d)" % (rows, int(n_bank)),
                     wrong_dtype="%s's index holds integers (bank rows), got dtype %%s" % what)
    return np.array(arr, dtype=np.int32, order="C")  # (always a copy: the caller may go on writing its array)


def resolve_bank_episode(index, n_bank, B, way, shot):
    """The support rows of one training episode, host only (no device): index [B, way*shot] integers, row b the bank rows of
    query image b's supports with its `shot` positives first (dana.py:103-104: the layout of support_ims) -> a C-contiguous
    int32 array of that shape. Repeats are fine: one exemplar may be positive for one image and negative for another.
    B None: any batch size >= 1. ValueError: a device tensor, a non-integer dtype, a wrong shape; IndexError: an entry
    outside [0, n_bank)."""
    ws = int(way) * int(shot)

    def shape_text(arr):
        if arr.ndim != 2 or arr.shape[1] != ws or arr.shape[0] < 1 or (B is not None and arr.shape[0] != int(B)):
            return ("a bank episode's index must be [%s, way*shot = %d] (per query image its %d positive supports, then "
                    "the negatives), got %s" % ("B" if B is None else int(B), ws, int(shot), arr.shape))

    return _bank_rows(index, n_bank, "a bank episode", "a numpy array, nested lists or a CPU tensor", "bank episode", shape_text)


class SupportBank(_Encoded):
    """The weight-independent support tensors of a pool of N images (DAnARCNN.encode_support_bank), for fine-tuning over a
    frozen trunk (cfg.RESNET.FIXED_BLOCKS = 3): map_pe [N][L][1024], the trunk map + PE, and pool_pe [N][49][1024], its
    average pool + PE -- everything on the support side in front of the first trained weight. (A SupportCache stores the
    K / unary / S.Wt^T chain behind those weights, which is why it serves inference only.)
    `ep = bank.episode(index)` names the B*way*shot supports of an iteration by bank row; `model(im_data, im_info, gt_boxes,
    num_boxes, ep)` in train mode gathers them (one launch, dana_bank_gather_episode, index read on the device) and runs the
    query trunk only; `ep.set(index)` names the next iteration's -- a recorded replay (program.ProgramTrainer) follows it.
    The bank records what it was built under (the trunk's parameters and buffers, the MFMA and Winograd settings, the
    device); using it after any of that changed raises ("re-encode")."""

    _ADVICE, _STATE, _FORWARD, _ENCODER = "re-encode the pool", "_bank_state", "query", "encode_support_bank"
    _DEPENDS = "the trunk's weights or buffers, the MFMA mode or the Winograd settings"

    def __init__(self, model, map_pe, pool_pe, sup_map, pool, state, dev):
        self._model = weakref.ref(model)
        self.map_pe, self.pool_pe = map_pe, pool_pe
        self.sup_map, self.pool, self.device = tuple(sup_map), pool, torch.device(dev)
        self._state = state
        self._index = {}       # (B, way*shot) -> device int32 [B*way*shot]: what dana_bank_gather_episode reads
        self._index_host = {}  # ... and what it holds

    def __len__(self):
        return self.map_pe.size(0)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.map_pe, self.pool_pe))

    def episode(self, index):
        """-> BankEpisode over index [B, way*shot] (`resolve_bank_episode`; way and shot are the model's)"""
        return BankEpisode(self, index)

    def _write_index(self, arr):
        """arr into the device index of its shape (allocated once per shape: a recording points at it)"""
        key = arr.shape
        self._index[key], self._index_host[key] = write_device_index(
            self._index.get(key), self._index_host.get(key), arr, self.device,
            "SupportBank: the episode changed inside a recording / capture: ep.set(index) before it")


class BankEpisode:
    """SupportBank.episode(index): the 5th argument of a train-mode forward over a frozen trunk, in place of support_ims
    [B, way*shot, 3, S, S] -- image b's supports are the bank rows index[b], positives first. The index lives in a device
    buffer the bank owns (one per episode shape, shared by the bank's episodes of that shape: the forward uploads an
    episode's index when the buffer holds another); `set(index)` rewrites it for the next iteration."""

    __slots__ = ("bank", "B", "way", "shot", "_host")

    def __init__(self, bank, index):
        model = bank._model()
        if model is None:
            raise RuntimeError("the model of this SupportBank is gone")
        self.bank, self.way, self.shot = bank, int(model.n_way), int(model.n_shot)
        self._host = resolve_bank_episode(index, len(bank), None, self.way, self.shot)
        self.B = self._host.shape[0]
        bank._write_index(self._host)

    def set(self, index):
        """the supports of the next forwards (same shape), validated on the host and written into the device index"""
        self._host = resolve_bank_episode(index, len(self.bank), self.B, self.way, self.shot)
        self.bank._write_index(self._host)

    @property
    def index(self):
        """the episode's host index [B, way*shot] (a copy)"""
        return self._host.copy()

    def _check(self, model, dev, B):
        self.bank._check(model, dev)
        if (self.way, self.shot) != (int(model.n_way), int(model.n_shot)):
            raise RuntimeError("this episode was laid out for way %d, shot %d; the model now has way %d, shot %d: make a new "
                               "one (bank.episode)" % (self.way, self.shot, model.n_way, model.n_shot))
        if B != self.B:
            raise RuntimeError("a bank episode of %d query images for a batch of %d" % (self.B, B))
        self.bank._write_index(self._host)  # (a no-op unless another episode of this shape used the buffer since)

    def _gather(self, shot):
        """-> (s_pe [B][shot*L][1024], sp_pe [B*way*shot*49][1024]) of the episode, fresh buffers on the current stream,
        written by ONE launch"""
        bank = self.bank
        return ops.bank_gather_episode(bank.map_pe, bank.pool_pe, bank._index[self._host.shape], self.B, self.way, shot)


def resolve_query_batch(index, n_bank, B=None):
    """The query rows of one batch, host only (no device): index [B] integers, entry b the bank row of query image b -> a
    C-contiguous int32 array of that shape. Repeats are fine. B None: any batch size >= 1. ValueError: a device tensor, a
    non-integer dtype, a wrong shape; IndexError: an entry outside [0, n_bank)."""
    def shape_text(arr):
        if arr.ndim != 1 or arr.shape[0] < 1 or (B is not None and arr.shape[0] != int(B)):
            return ("a query batch's index must be [%s] (per query image its bank row), got %s"
                    % ("B" if B is None else int(B), arr.shape))

    return _bank_rows(index, n_bank, "a query batch", "a numpy array, a list or a CPU tensor", "query batch", shape_text)


class QueryBank(_Encoded):
    """The trunk maps of a pool of N query images of one H x W (DAnARCNN.encode_query_bank): maps [N][fh*fw][1024], what the
    query trunk writes into the first half of corr. Over a frozen trunk (cfg.RESNET.FIXED_BLOCKS = 3) they are constants of a
    fine-tuning run, as a SupportBank's rows are. `qb = bank.batch(index)` names the B images of a forward by bank row;
    `model(qb, im_info, gt_boxes, num_boxes, support)` gathers them (one launch, dana_qbank_gather, index read on the device)
    and runs no query trunk -- in train mode with support images or a BankEpisode, in eval mode with support images, a
    SupportCache or a ClassSweep; `qb.set(index)` names the next forward's -- a recorded replay (program.ProgramTrainer)
    follows it. The bank records what it was built under (the trunk's parameters and buffers, the MFMA and Winograd
    settings, the device); using it after any of that changed raises ("re-encode"). Layer4, the RPN and the heads may move.
    A trunk with stages that train (FIXED_BLOCKS < 3: eval-mode use only) is written by the fused optimizers through raw
    pointers, which no tensor version shows, so there the bank also records the model's weight epoch: it is stale after every
    optimizer step (and after a ProgramTrainer recording), i.e. it serves the forwards between two steps only."""

    _ADVICE, _STATE, _FORWARD, _ENCODER = "re-encode the images", "_qbank_state", "forward runs", "encode_query_bank"
    _DEPENDS = ("the trunk's weights or buffers, the MFMA mode or the Winograd settings; over a trunk with stages that train, "
                "any optimizer step or re-recording")

    def __init__(self, model, maps, image_hw, map_hw, state, dev):
        self._model = weakref.ref(model)
        self.maps = maps
        self.image_hw, self.map_hw, self.device = tuple(image_hw), tuple(map_hw), torch.device(dev)
        self._state = state
        self._index = {}       # B -> device int32 [B]: what dana_qbank_gather reads
        self._index_host = {}  # ... and what it holds

    def __len__(self):
        return self.maps.size(0)

    def nbytes(self):
        return self.maps.numel() * self.maps.element_size()

    def batch(self, index):
        """-> QueryBatch over index [B] (`resolve_query_batch`)"""
        return QueryBatch(self, index)

    def _write_index(self, arr):
        """arr into the device index of its B (allocated once per B: a recording points at it); one small asynchronous
        upload on the current stream, as SupportBank._write_index's"""
        key = arr.shape[0]
        self._index[key], self._index_host[key] = write_device_index(
            self._index.get(key), self._index_host.get(key), arr, self.device,
            "QueryBank: the batch changed inside a recording / capture: batch.set(index) before it")


class QueryBatch:
    """QueryBank.batch(index): the 1st argument of a forward, in place of im_data [B, 3, H, W] -- query image b is bank row
    index[b]. B, the device and H x W come from the batch. The index lives in a device buffer the bank owns (one per B, shared
    by the bank's batches of that size: the forward uploads a batch's index when the buffer holds another); `set(index)`
    rewrites it for the next forward."""

    __slots__ = ("bank", "B", "_host")

    def __init__(self, bank, index):
        self.bank = bank
        self._host = resolve_query_batch(index, len(bank))
        self.B = self._host.shape[0]
        bank._write_index(self._host)

    def set(self, index):
        """the query images of the next forwards (same B), validated on the host and written into the device index"""
        self._host = resolve_query_batch(index, len(self.bank), self.B)
        self.bank._write_index(self._host)

    @property
    def index(self):
        """the batch's host index [B] (a copy)"""
        return self._host.copy()

    def _check(self, model, dev):
        self.bank._check(model, dev)
        self.bank._write_index(self._host)  # (a no-op unless another batch of this size used the buffer since)

    def _gather(self, corr):
        """the batch's trunk maps into the first 1024 columns of corr [B*fh*fw][2048], ONE launch on the current stream"""
        bank = self.bank
        return ops.qbank_gather(bank.maps, bank._index[self.B], self.B, out=corr, ld_out=corr.size(1))
