"""Shot views of a cached support set: `cache.select(indices, shots=)`, `cache.sweep(classes, shots=)`, ragged sets
(`encode_supports(..., num_shots=)`) and shot ensembles (`shots="each"`), with the kernels under them
(dana_gather_shot_blocks, dana_attn_softmax_unary_w, dana_attn_softmax_unary_sweep_w) and the launch-program replay.

Bars. The gather is a move: bits. The `_w` softmax meets test_gpu_forward_ops.py's float64 bar (|err| <= 1e-6 * the summed
term magnitudes) and equals the scalar-scale kernels bit for bit where the scales are equal. A view forward issues the
launches an m-shot model issues on the same blocks, so it equals that model's cached forward bit for bit. Against
UNCACHED forwards of 1- and 2-shot models (other support-side launch shapes) and between the per-segment-scale path and
the scalar one, the bars are test_gpu_support_cache.py's end-to-end ones: IoU >= 1 - 1e-3 for >= 99 % of the rois (a
condition, met by the seeded episodes below as it is by that file's cached-vs-uncached tests, which use the same model
and episodes), cls_prob / bbox_pred within 1e-4 on the matched rois.
Queries are 192 x 256, supports 320 x 320, shot 3; the helpers are those of test_gpu_support_cache.py, copied."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TINY = float(np.finfo(np.float32).tiny)


# ---- helpers of test_gpu_support_cache.py / test_gpu_backward_ops.py (copies) ---------------------------------------
def _model(dev, shot=3, use_ba=True):
    import dana_amd
    from dana_amd import synthetic as S
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=use_ba, way=1, shot=shot, classes=["fg", "bg"])
    sd = S.fill_state_dict(m.state_dict(), seed=11, profile="test")
    m.load_state_dict(sd)
    return m.to(dev).eval(), sd


def _episode(dev, B, shot=3, H=192, W=256, seed=1996):
    from dana_amd import synthetic as S
    return [t.to(dev) for t in S.episode_inputs(B, 1, shot, H, W, seed=seed)]


def _sets(sup):
    """[B, shot, 3, S, S] episode supports -> B support sets"""
    return sup.reshape(sup.size(0), -1, 3, sup.size(-2), sup.size(-1))


def _iou(a, b):
    x1, y1 = np.maximum(a[:, 0], b[:, 0]), np.maximum(a[:, 1], b[:, 1])
    x2, y2 = np.minimum(a[:, 2], b[:, 2]), np.minimum(a[:, 3], b[:, 3])
    inter = np.clip(x2 - x1 + 1, 0, None) * np.clip(y2 - y1 + 1, 0, None)
    aa = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    ab = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    return inter / (aa + ab - inter)


def _close(out, ref):
    """test_gpu_model.py's end-to-end bar between two output tuples"""
    r, rg = out[0].cpu().numpy().reshape(-1, 5), ref[0].cpu().numpy().reshape(-1, 5)
    assert r.shape == rg.shape and np.array_equal(r[:, 0], rg[:, 0])
    matched = _iou(r[:, 1:], rg[:, 1:]) >= 1 - 1e-3
    print("matched %.2f%%" % (100 * matched.mean()))
    assert matched.mean() >= 0.99, "only %.1f%% of rois match by position" % (100 * matched.mean())
    d1 = np.abs(out[1].cpu().numpy() - ref[1].cpu().numpy())[matched].max()
    d2 = np.abs(out[2].cpu().numpy() - ref[2].cpu().numpy())[matched].max()
    print("max |d cls_prob| %.3e  max |d bbox_pred| %.3e" % (d1, d2))
    assert d1 <= 1e-4 and d2 <= 1e-4


def _same(out, ref):
    for a, b, name in zip(out[:3], ref[:3], ("rois", "cls_prob", "bbox_pred")):
        assert torch.equal(a, b), "%s differs (max |d| %.3e)" % (name, (a - b).abs().max().item())


def _clone(out):
    return tuple(t.clone() if torch.is_tensor(t) else t for t in out)


def _check(got, ref, mag, what, tiny=0.0):
    """|got - ref| <= 1e-6 * mag + tiny per element; prints and reports the worst err / bound"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), "%s: non-finite result" % what
    err = (got - ref).abs()
    bound = 1e-6 * mag.expand_as(ref) + tiny
    inexact = torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err))  # (a zero bound asks for equality)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), inexact)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("ERR/BOUND %-44s %.4f" % (what, worst))
    assert worst <= 1.0, "%s: worst err / bound = %.3f (max err %.3e)" % (what, worst, float(err.max()))


def _wide(t, ld, fill):
    buf = torch.full((t.size(0), ld), fill, dtype=t.dtype)
    buf[:, :t.size(1)] = t
    return buf


def _block(out, p, R):
    """problem p of a sweep's outputs as a one-problem output tuple (rois' column 0 = 0)"""
    rois = out[0][p:p + 1].clone()
    rois[:, :, 0] = 0
    return rois, out[1][p * R:(p + 1) * R], out[2][p * R:(p + 1) * R]


# ---- shared state: one 3-shot model, one cache of 3 sets, one query image, built once. The cache's tensors never change;
# its selection does, so every test selects what it needs before it runs a forward.
_SHARED = {}


def _shared(dev):
    if not _SHARED:
        m, sd = _model(dev)
        sets = _sets(_episode(dev, 3, seed=7)[4])
        with torch.no_grad():
            cache = m.encode_supports(sets)
        _SHARED.update(m=m, sd=sd, sets=sets, cache=cache, q=_episode(dev, 1)[:4])
    return _SHARED


# ---- 1. the gather ----------------------------------------------------------------------------------------------------
GATHER_VIEWS = {  # P = 5 problems over C = 3 sets (set 1 has 2 real shots: its shot 2 is NaN in the source)
    3: ([0, 2, 2, 1, 0], [(0, 1, 2), (2, 0), (1,), (1, 0), (0, 2, 1)]),
    2: ([0, 2, 2, 1, 0], [(2, 0), (1,), (0, 1), (1,), (1, 2)]),
    1: ([0, 2, 2, 1, 0], [(2,), (0,), (1,), (0,), (0,)]),
}


@pytest.mark.parametrize("m", [1, 2, 3])
def test_gather_shot_blocks_equals_torch_indexing(dev, m):
    """(rows 1, block 8 floats): 16-byte copies; (rows 1, block 49 floats): un2's 4-byte tier; (rows 5, block 12 floats):
    a row axis outside the shot axis, as s_t has. Out-of-order view (2, 0), a repeated set, padding slots."""
    import dana_amd
    ops = dana_amd.ops
    C, shot, P = 3, 3, 5
    index, views = GATHER_VIEWS[m]
    gen = torch.Generator().manual_seed(40 + m)
    rows, blocks = [1, 1, 5], [8, 49, 12]
    srcs = []
    for r, b in zip(rows, blocks):
        t = torch.randn(C, r, shot, b, generator=gen)
        t[1, :, 2, :] = float("nan")  # the unused slot of the 2-shot set
        srcs.append(t.to(dev))
    view = torch.full((P, shot), -1, dtype=torch.int32)
    for p, v in enumerate(views):
        view[p, :len(v)] = torch.tensor(v, dtype=torch.int32)
    dsts, w = ops.gather_shot_blocks(srcs, rows, blocks, torch.tensor(index, dtype=torch.int32, device=dev), view.to(dev), m)
    for t, d in zip(srcs, dsts):
        ref = torch.zeros_like(d)
        for p, (c, v) in enumerate(zip(index, views)):
            ref[p, :, :len(v), :] = t[c][:, list(v), :]
        assert torch.isfinite(d).all()
        assert torch.equal(d, ref)
        assert (d.view(torch.int32)[ref == 0] == 0).all()  # (+0.0 in the padding slots)
    w_ref = torch.zeros(P, m)
    for p, v in enumerate(views):
        w_ref[p, :len(v)] = torch.tensor(1.0) / len(v)  # float32 1.0f / n
    assert torch.equal(w.cpu(), w_ref)


def test_gather_shot_blocks_byte_tier_and_bad_indices(dev):
    """a 13-byte block from an odd address takes the byte copies; a set index outside [0, n_sets) writes nothing, a shot
    index outside [0, shot) is a padding slot"""
    from dana_amd._lib import lib
    import dana_amd
    ops = dana_amd.ops
    C, shot, P, m, rows, nb = 2, 3, 3, 2, 2, 13
    gen = torch.Generator().manual_seed(5)
    raw = torch.randint(1, 255, (1 + C * rows * shot * nb,), generator=gen, dtype=torch.uint8).to(dev)
    src = raw[1:]  # (odd address)
    dst = torch.full((P * rows * m * nb,), 77, dtype=torch.uint8, device=dev)
    w = torch.full((P, m), 9.0, device=dev)
    index = torch.tensor([1, 5, 0], dtype=torch.int32, device=dev)  # problem 1: no such set
    view = torch.tensor([[2, 0, -1], [0, 1, -1], [1, 7, -1]], dtype=torch.int32, device=dev)  # problem 2: shot 7
    tab = torch.tensor([[src.data_ptr()], [dst.data_ptr()], [rows], [nb]], dtype=torch.int64).to(dev)
    lib().call("dana_gather_shot_blocks", tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(), 1,
               index.data_ptr(), view.data_ptr(), w.data_ptr(), C, shot, m, P, ops._stream())
    s4 = src.view(C, rows, shot, nb).cpu()
    ref = torch.full((P, rows, m, nb), 77, dtype=torch.uint8)
    ref[0] = s4[1][:, [2, 0], :]
    ref[2, :, 0] = s4[0][:, 1, :]
    ref[2, :, 1] = 0
    assert torch.equal(dst.view(P, rows, m, nb).cpu(), ref)
    assert torch.equal(w.cpu(), torch.tensor([[0.5, 0.5], [9.0, 9.0], [1.0, 0.0]]))


# ---- 2. the per-segment-scale softmax -----------------------------------------------------------------------------------
def _softmax_mag(x, p, dim):
    return p * (1 + (x - x.max(dim, keepdim=True)[0]).abs())


SCALES = {1: [[0.25], [0.0]], 3: [[0.5, 0.0, 0.5], [1.0, 0.0, 0.0]]}  # per batch; 0: a padding slot


@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("L", [49, 400, 520])  # 520 > 512: the loop path, else a segment stays in registers
def test_attn_softmax_unary_w_vs_fp64(dev, L, nseg):
    """A = (softmax_seg(S) + ugamma * u) * scale[batch][seg] in place on rows ld apart, 10 rows in batches of 5, kpad >
    nseg * L. mag = (p (1 + |x - max|) + |ugamma u|) * scale (test_attn_softmax_unary_vs_fp64's). Zero-scale segments hold
    NaN scores and NaN unary terms: they are not read and come back as +0.0. Equal scales: the scalar kernel's bits."""
    import dana_amd
    ops = dana_amd.ops
    gen = torch.Generator().manual_seed(300 + 7 * L + nseg)
    rows, rpb = 10, 5
    K = nseg * L
    kpad = (K + 7) // 8 * 8 + 8
    ld, ubs, sbs = kpad + 8, K + 5, nseg + 2
    ug = float(np.float32(0.1))
    sc = torch.tensor(SCALES[nseg], dtype=torch.float32)  # [2][nseg]
    x = torch.randn(rows, nseg, L, generator=gen) * 2
    u = torch.rand(rows // rpb, ubs, generator=gen)
    dead = (sc == 0)[:, None, :].expand(-1, rpb, -1).reshape(rows, nseg)  # [rows][nseg]
    xn = x.clone()
    xn[dead] = float("nan")
    un = u.clone()
    for b_ in range(sc.size(0)):
        for s_ in range(nseg):
            if sc[b_, s_] == 0:
                un[b_, s_ * L:(s_ + 1) * L] = float("nan")
    xb = _wide(xn.view(rows, K), ld, 9.0).to(dev)
    scb = _wide(sc, sbs, float("nan")).to(dev)
    ops.attn_softmax_unary_w_(xb, un.to(dev), rows, rpb, nseg, L, ld, kpad, 0.1, scb, unary_batch_stride=ubs,
                              scale_batch_stride=sbs)
    xd = x.double()
    p = F.softmax(xd, 2)
    ud = u[:, :K].double().reshape(rows // rpb, 1, nseg, L).expand(-1, rpb, -1, -1).reshape(rows, nseg, L)
    scd = sc.double()[:, None, :, None].expand(-1, rpb, -1, L).reshape(rows, nseg, L)
    ref = (p + ug * ud) * scd
    mag = (_softmax_mag(xd, p, 2) + (ug * ud).abs()) * scd
    _check(xb[:, :K], ref.view(rows, K), mag.view(rows, K), "attn_softmax_unary_w_ L %d nseg %d" % (L, nseg), TINY)
    got = xb[:, :K].view(rows, nseg, L).cpu()
    assert (got[dead].view(torch.int32) == 0).all()  # exact +0.0 over NaN input
    assert (xb[:, K:kpad] == 0).all() and (xb[:, kpad:] == 9.0).all()
    # equal scales: the bits of the scalar-scale kernel
    osc = 1.0 / nseg
    a = _wide(x.view(rows, K), ld, 9.0).to(dev)
    b = a.clone()
    ops.attn_softmax_unary_(a, u.to(dev), rows, rpb, nseg, L, ld, kpad, 0.1, osc, unary_batch_stride=ubs)
    ops.attn_softmax_unary_w_(b, u.to(dev), rows, rpb, nseg, L, ld, kpad, 0.1,
                              torch.full((rows // rpb, nseg), osc, dtype=torch.float32, device=dev), unary_batch_stride=ubs)
    assert torch.equal(a, b)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("L", [400, 520])
def test_sweep_w_softmax_equals_plain_w(dev, C, L):
    """the sweep form moves row (b, i, c) to problem b*C + c: row for row the plain form's bits, scales and NaN-filled
    zero-scale segments included; with equal scales the scalar sweep kernel's bits"""
    import dana_amd
    ops = dana_amd.ops
    B, hw, shot = 2, 37, 3
    K1 = shot * L
    gen = torch.Generator().manual_seed(10 * C + L)
    sc = torch.tensor([[1.0 / 3] * 3, [0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.5, 0.5, 0.0], [1.0 / 3] * 3, [1.0, 0.0, 0.0]])[:B * C]
    by_problem = torch.randn(B * C, hw, shot, L, generator=gen) * 4
    unary = torch.softmax(torch.randn(B * C, shot, L, generator=gen), -1)
    dead = sc == 0  # [B*C][shot]
    unary[dead] = float("nan")
    by_problem[dead[:, None, :].expand(-1, hw, -1)] = float("nan")
    scores = by_problem.view(B, C, hw, K1).permute(0, 2, 1, 3).reshape(B, hw, C * K1).contiguous()
    assert torch.isnan(scores).any() == bool(dead.any())
    scores, unary, sc = scores.to(dev), unary.to(dev), sc.contiguous().to(dev)
    out = torch.full((B * C, hw, K1), 7.0, device=dev)
    ops.attn_softmax_unary_sweep_w(scores, out, unary, B, C, hw, shot, L, K1, K1, K1, 0.1, sc)
    ref = scores.view(B, hw, C, K1).permute(0, 2, 1, 3).contiguous()  # problem-major copy: [B*C][hw][K1]
    ops.attn_softmax_unary_w_(ref, unary, B * C * hw, hw, shot, L, K1, K1, 0.1, sc)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref.view(B * C, hw, K1))
    clean = torch.nan_to_num(scores, nan=0.5)
    u_clean = torch.nan_to_num(unary, nan=0.25)
    a = torch.empty_like(out)
    b = torch.empty_like(out)
    ops.attn_softmax_unary_sweep(clean, a, u_clean, B, C, hw, shot, L, K1, K1, K1, 0.1, 1.0 / shot)
    ops.attn_softmax_unary_sweep_w(clean, b, u_clean, B, C, hw, shot, L, K1, K1, K1, 0.1,
                                   torch.full((B * C, shot), 1.0 / shot, dtype=torch.float32, device=dev))
    assert torch.equal(a, b)


# ---- 3. exactness of the plumbing ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", [(1,), (2, 0), (0, 1, 2)], ids=str)
def test_view_forward_equals_m_shot_model_on_sliced_cache(dev, view):
    """an m-shot model with the same weights and a SupportCache built from torch slices of the 3-shot cache's tensors
    issues the launches of the 3-shot model's view forward, on the same numbers -> the same bits on all three outputs"""
    from dana_amd.dana import SupportCache
    sh = _shared(dev)
    m3, cache3 = sh["m"], sh["cache"]
    mk, _ = _model(dev, shot=len(view))
    mk.load_state_dict(sh["sd"])
    blocks = m3._cache_shot_blocks(cache3.sup_map)
    C = len(cache3)
    tensors = {k: t.view(C, blocks[k][0], 3, blocks[k][1])[:, :, list(view), :].reshape(C, -1).contiguous()
               for k, t in cache3._t.items()}
    cache_k = SupportCache(mk, tensors, len(view), cache3.sup_map, cache3.pool, mk._cache_state(dev), dev)
    with torch.no_grad():
        ref = _clone(mk(*sh["q"], cache_k.sweep([2, 0])))
        out = m3(*sh["q"], cache3.sweep([2, 0], shots=view))
    assert out[0].shape == ref[0].shape and out[0].size(0) == 2
    _same(out, ref)


# ---- 4. meaning -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", [(0,), (1,), (2,), (0, 1)], ids=str)
def test_view_matches_uncached_forward_of_a_smaller_model(dev, view):
    """view (s,) is the 1-shot model's forward on shot s alone, view (0, 1) the 2-shot model's on the first two shots --
    UNCACHED forwards of models built with that num_shot, from the support images. Episode: the seeded B = 2 episode
    (seed 1996) of test_gpu_support_cache.py's cached-vs-uncached tests, which meet the 99 % condition on it."""
    m3, sd = _model(dev)
    mk, _ = _model(dev, shot=len(view))
    mk.load_state_dict(sd)
    im, info, gt, nb, sup = _episode(dev, 2)
    sets = _sets(sup)
    with torch.no_grad():
        cache = m3.encode_supports(sets)
        cache.select([0, 1], shots=view)
        out = _clone(m3(im, info, gt, nb, cache))
        ref = mk(im, info, gt, nb, sets[:, list(view)].contiguous())
    _close(out, ref)


# ---- 5. mixed lengths and ragged sets -----------------------------------------------------------------------------------
def test_mixed_length_sweep_matches_each_view_alone(dev):
    """views of lengths 1, 2 and 3 in one sweep (m = 3: per-segment scales, padding slots) against each view run alone
    on the scalar-scale path with m = its own length"""
    sh = _shared(dev)
    m, cache = sh["m"], sh["cache"]
    views = [(1,), (2, 0), (0, 1, 2)]
    classes = [2, 0, 1]
    with torch.no_grad():
        out = _clone(m(*sh["q"], cache.sweep(classes, shots=views)))
        assert cache._mode == (3, True)
        R = out[0].size(1)
        assert out[0].shape == (3, R, 5) and all(torch.isfinite(t).all() for t in out[:3])
        for p, (c, v) in enumerate(zip(classes, views)):
            ref = m(*sh["q"], cache.sweep([c], shots=[v]))
            assert cache._mode in (None, (len(v), False))
            _close(_block(out, p, R), ref)
        # ... and the plain (no sweep) forward over a selection with views of unequal length
        im, info, gt, nb = _episode(dev, 2)[:4]
        cache.select([1, 2], shots=[(2,), (1, 0)])
        both = _clone(m(im, info, gt, nb, cache))
        assert cache._mode == (2, True)
        for b, (c, v) in enumerate([(1, (2,)), (2, (1, 0))]):
            cache.select([c], shots=[v])
            ref = m(im[b:b + 1], info[b:b + 1], gt[b:b + 1], nb[b:b + 1], cache)
            _close(_block(both, b, R), ref)


def test_ragged_sets(dev):
    """num_shots = [3, 2, 1]: the unused slots hold NaN images, their encoded blocks stay in the cache and never reach a
    forward -- the outputs are finite and equal, bit for bit, the same call with zero images there"""
    sh = _shared(dev)
    m = sh["m"]
    nan_sets, zero_sets = sh["sets"].clone(), sh["sets"].clone()
    for c, n in enumerate([3, 2, 1]):
        nan_sets[c, n:] = float("nan")
        zero_sets[c, n:] = 0
    with torch.no_grad():
        cache = m.encode_supports(nan_sets, num_shots=[3, 2, 1])
        assert cache.shot_counts == (3, 2, 1) and sh["cache"].shot_counts == (3, 3, 3)
        out = _clone(m(*sh["q"], cache.sweep()))
        assert cache._mode == (3, True)
        assert all(torch.isfinite(t).all() for t in out[:3])
        zcache = m.encode_supports(zero_sets, num_shots=torch.tensor([3, 2, 1]))
        _same(m(*sh["q"], zcache.sweep()), out)
        # the default selection of a ragged cache takes each set's real shots too
        cache.select([1])
        one = _clone(m(*sh["q"], cache))
        assert cache._mode == (2, False) and all(torch.isfinite(t).all() for t in one[:3])
        _close(m(*sh["q"], cache.sweep([1])), one)  # (a one-class sweep splits the RPN conv: other launches)
    with pytest.raises(IndexError):
        cache.sweep([1], shots=[(2,)])  # shot 2 of the 2-shot set
    with pytest.raises(IndexError):
        cache.select([2], shots=2)
    with pytest.raises(ValueError):
        m.encode_supports(nan_sets, num_shots=[3, 2])
    with pytest.raises(ValueError):
        m.encode_supports(nan_sets, num_shots=[3, 4, 1])
    with pytest.raises(ValueError):
        m.encode_supports(nan_sets, num_shots=[3, 0, 1])


# ---- 6. ensemble --------------------------------------------------------------------------------------------------------
def test_each_is_the_list_of_one_shot_views(dev):
    from dana_amd import postprocess as PP
    sh = _shared(dev)
    m, cache = sh["m"], sh["cache"]
    im, info = sh["q"][0], sh["q"][1]
    with torch.no_grad():
        sw = cache.sweep([2, 0], shots="each")
        assert len(sw) == 6 and sw.classes == (2, 2, 2, 0, 0, 0) and sw.views == ((0,), (1,), (2,)) * 2
        out = _clone(m(*sh["q"], sw))
        assert cache._mode == (1, False)
        ref = m(*sh["q"], cache.sweep([2, 2, 2, 0, 0, 0], shots=[(0,), (1,), (2,), (0,), (1,), (2,)]))
        _same(out, ref)
        cd = PP.detections_by_class(out[0], out[1], out[2], info, 6, with_layout=True)
        ens = PP.ensemble_shots(cd, 3)
        assert len(ens) == 1 and len(ens[0]) == 2 and ens.num_classes == 2
        ragged = m.encode_supports(sh["sets"], num_shots=[3, 2, 3])
    assert len(ragged.sweep([0, 2], shots="each")) == 6
    with pytest.raises(ValueError, match="different shot counts"):
        ragged.sweep(shots="each")
    with pytest.raises(ValueError):
        cache.select([0], shots="each")
    with pytest.raises(ValueError):
        cache.sweep([0], shots=torch.tensor([0], device=dev))
    with pytest.raises(ValueError, match="twice"):
        cache.sweep([0], shots=[(1, 1)])
    with pytest.raises(ValueError, match="empty"):
        cache.select([0], shots=[()])


# ---- 7. replay ----------------------------------------------------------------------------------------------------------
def test_program_replay_follows_views(dev):
    from dana_amd.graphs import GraphedDAnA
    from dana_amd.program import ProgramDAnA
    sh = _shared(dev)
    m, cache = sh["m"], sh["cache"]
    q = sh["q"]
    with torch.no_grad():
        cache.select([1], shots=[(0,)])
        eager = _clone(m(*q, cache))
        prog = ProgramDAnA(m, *q, cache)
        _same(prog(*q, cache), eager)
        cache.select([2], shots=[(2,)])  # between replays: the recorded gather reads index and view table on the device
        eager = _clone(m(*q, cache))
        _same(prog(*q, cache), eager)
        cache.select([0], shots=[(1, 0)])
        with pytest.raises(RuntimeError, match="record a new runner"):
            prog(*q, cache)
        cache.select([0])
        with pytest.raises(RuntimeError, match="record a new runner"):
            prog(*q, cache)
        cache.select([0], shots=1)
        _same(prog(*q, cache), _clone(m(*q, cache)))
        # a sweep of views, recorded weighted; replayed with other views of the same (m, weighted)
        sw = cache.sweep([0, 1], shots=[(0,), (2, 1)])
        eager = _clone(m(*q, sw))
        sprog = ProgramDAnA(m, *q, sw)
        _same(sprog(*q, sw), eager)
        sw2 = cache.sweep([2, 0], shots=[(1, 2), (1,)])
        eager = _clone(m(*q, sw2))
        _same(sprog(*q, sw2), eager)
        with pytest.raises(RuntimeError, match="record a new runner"):
            sprog(*q, cache.sweep([2, 0], shots=2))
        with pytest.raises(NotImplementedError):
            GraphedDAnA(m, *q, cache.sweep([0], shots=1))


def test_views_cannot_change_inside_a_recording(dev):
    from dana_amd import _lib
    sh = _shared(dev)
    m, cache = sh["m"], sh["cache"]
    with torch.no_grad():
        cache.select([1], shots=[(0,)])
        m(*sh["q"], cache)

        class Names:
            def add_call(self, fn, name, args):
                pass

        _lib.RECORDER = Names()
        try:
            with pytest.raises(RuntimeError, match="inside a recording"):
                cache.select([1], shots=[(1,)])
        finally:
            _lib.RECORDER = None


def _launch_names(m, q, arg):
    """the forward's launch list through the launch recorder (_lib.RECORDER, what program.LaunchProgram records from)"""
    from dana_amd import _lib

    class Names:
        def __init__(self):
            self.names = []

        def add_call(self, fn, name, args):
            self.names.append(name)

    with torch.no_grad():
        m(*q, arg)  # (eagerly first: buffers allocated, selection written)
        rec = Names()
        _lib.RECORDER = rec
        try:
            m(*q, arg)
        finally:
            _lib.RECORDER = None
    torch.cuda.synchronize()
    return rec.names


def test_identity_views_issue_the_parent_launch_list(dev):
    sh = _shared(dev)
    m, cache = sh["m"], sh["cache"]
    q = sh["q"]
    m._single_stream = True
    try:
        cache.select([1])
        plain = _launch_names(m, q, cache)
        assert plain.count("dana_gather_blocks") == 1 and "dana_gather_shot_blocks" not in plain
        for shots in (None, 3, (0, 1, 2), [(0, 1, 2)], [None]):
            cache.select([1], shots=shots)
            assert cache._sel_views is None
            assert _launch_names(m, q, cache) == plain, shots
        sweep = _launch_names(m, q, cache.sweep([0, 2]))
        assert sweep.count("dana_gather_blocks") == 1 and "dana_gather_shot_blocks" not in sweep
        assert _launch_names(m, q, cache.sweep([0, 2], shots=[(0, 1, 2), 3])) == sweep
        # a real view: the shot gather in place of the set gather, scalar softmax launches while the lengths are equal
        cache.select([1], shots=[(2, 0)])
        viewed = _launch_names(m, q, cache)
        assert viewed.count("dana_gather_shot_blocks") == 1 and "dana_gather_blocks" not in viewed
        assert not any(n.endswith("_w") for n in viewed) and len(viewed) == len(plain)
        mixed = _launch_names(m, q, cache.sweep([0, 2], shots=[(1,), (2, 0)]))
        assert mixed.count("dana_gather_shot_blocks") == 1 and "dana_gather_blocks" not in mixed
        assert mixed.count("dana_attn_softmax_unary_sweep_w") == 1 and mixed.count("dana_attn_softmax_unary_w") == 1
        assert "dana_attn_softmax_unary" not in mixed and "dana_attn_softmax_unary_sweep" not in mixed
        assert len(mixed) == len(sweep)
        # one set, one image, whole set: still no gather at all
        one = m.encode_supports(sh["sets"][:1])
        alone = _launch_names(m, q, one)
        assert "dana_gather_blocks" not in alone and "dana_gather_shot_blocks" not in alone
    finally:
        m._single_stream = False
        cache.select([0])


# ---- 8. siblings --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["meta", "fsod", "fgn"])
def test_siblings_refuse_shot_views(dev, name):
    """meta, fsod and fgn average over the shots while encoding: no per-shot blocks in their caches"""
    import dana_amd
    from dana_amd import synthetic as S
    m = dana_amd.get_model(name, pretrained=False, way=1, shot=3, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=11, profile="test"))
    m.to(dev).eval()
    sets = _shared(dev)["sets"]
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="averages over"):
            m.encode_supports(sets, num_shots=[3, 2, 1])
        cache = m.encode_supports(sets)
    assert cache.shot_counts == (3, 3, 3)
    with pytest.raises(NotImplementedError, match="averages over"):
        cache.select([0], shots=1)
    with pytest.raises(NotImplementedError, match="averages over"):
        cache.sweep(shots="each")
    with pytest.raises(NotImplementedError, match="averages over"):
        cache.sweep([0, 1], shots=[(0,), (1, 2)])
    cache.select([0])  # (whole sets: as before)
    assert len(cache.sweep()) == 3
