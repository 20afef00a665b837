"""Cached support sets: DAnARCNN.encode_supports -> SupportCache, the cached eval forward
`model(im_data, im_info, gt_boxes, num_boxes, cache)` (one dana_gather_blocks launch for the selected sets), its launch-program
replay, and the batched detection post-processing (dana_detect_postprocess_batched).

Tolerances where the shapes of the support-side launches differ from the uncached forward's (the reference goldens, and
selections / broadcasts at B > 1, whose uncached forward runs the support trunk over all B * shot images at once) are
test_gpu_model.py's: IoU >= 1 - 1e-3 for >= 99 % of the rois, cls_prob / bbox_pred within 1e-4 on the matched rois."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _load(golden_dir, tag):
    return np.load(os.path.join(golden_dir, "e2e_%s.npz" % tag))


def _build(meta, dev):
    import dana_amd
    from dana_amd import synthetic as S
    use_ba, training, B, way, shot, H, W, wseed, iseed, nseed = [int(v) for v in meta[:10]]
    if len(meta) > 10 and int(meta[10]):  # attention_type='product'
        from dana_amd.dana import DAnARCNN
        m = DAnARCNN(["fg", "bg"], "product", 256, 256, pretrained=False, semantic_enhance=bool(use_ba), num_way=way,
                     num_shot=shot)
        m.create_architecture()
        tame = S.tame_product_weights
    else:
        m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=bool(use_ba), way=way, shot=shot,
                               classes=["fg", "bg"])
        tame = lambda sd_: sd_  # noqa: E731
    sd = tame(S.fill_state_dict(m.state_dict(), seed=wseed, profile="test"))
    m.load_state_dict(sd)
    m.to(dev)
    m.nms_inclusive = True  # the golden vectors come from the reference's CPU path (nms_cpu.cpp:60: >=)
    m.eval()
    inputs = S.episode_inputs(B, 1, shot, H, W, seed=iseed)
    return m, sd, [t.to(dev) for t in inputs]


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


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _close(out, ref):
    """test_gpu_model.py's end-to-end bar between two 8-tuples"""
    r, rg = out[0].cpu().numpy().reshape(-1, 5), ref[0].cpu().numpy().reshape(-1, 5)
    assert r.shape == rg.shape and np.array_equal(r[:, 0], rg[:, 0])
    matched = _iou(r[:, 1:], rg[:, 1:]) >= 1 - 1e-3
    assert matched.mean() >= 0.99, "only %.1f%% of rois match by position" % (100 * matched.mean())
    assert np.abs(out[1].cpu().numpy() - ref[1].cpu().numpy())[matched].max() <= 1e-4
    assert np.abs(out[2].cpu().numpy() - ref[2].cpu().numpy())[matched].max() <= 1e-4


def _same(out, ref):
    for a, b, name in zip(out[:3], ref[:3], ("rois", "cls_prob", "bbox_pred")):
        assert torch.equal(a, b), "%s differs (max |d| %.3e)" % (name, (a - b).abs().max().item())


def _clone(out):
    return tuple(t.clone() if torch.is_tensor(t) else t for t in out)


@pytest.fixture(params=[1, 0], ids=["bf16x6", "f32mfma"])
def mfma_mode(request):
    import dana_amd
    prev = dana_amd.ops.set_mfma_mode(request.param)
    yield request.param
    dana_amd.ops.set_mfma_mode(prev)


@pytest.mark.parametrize("tag", ["eval_small_cisa", "eval_small_ba", "eval_full_ba", "eval_small_product"])
def test_cached_forward_matches_reference_golden(golden_dir, dev, tag, mfma_mode):
    """the reference's own eval outputs, with the support side encoded once into a cache"""
    import dana_amd
    ops = dana_amd.ops
    g = _load(golden_dir, tag)
    m, _, din = _build(g["meta"], dev)
    with torch.no_grad():
        cache = m.encode_supports(_sets(din[4]))
        m._capture = {}
        rois, cls_prob, bbox_pred, l1, l2, l3, l4, lab = m(*din[:4], cache)
    assert (l1, l2, l3, l4, lab) == (0, 0, 0, 0, None)
    if "base_feat_s" in g:
        corr, B, fh, fw = m._capture["corr"]
        corr_nchw = ops.nhwc_to_nchw(corr, B, 2048, fh, fw).cpu().numpy()
        assert _rel(corr_nchw[:, :1024][:, ::16], g["base_feat_s"]) < 2e-4
        assert _rel(corr_nchw[:, 1024:][:, ::16], g["dense_s"]) < 2e-4
        heads = m._capture["rpn_heads"].view(B, fh, fw, 72).permute(0, 3, 1, 2).cpu().numpy()
        assert _rel(heads[:, :24], g["rpn_cls_score"]) < 2e-4
        assert _rel(heads[:, 24:], g["rpn_bbox_pred"]) < 2e-4
    assert m._capture["pooled"] is not None
    r, rg = rois.cpu().numpy().reshape(-1, 5), g["rois"].reshape(-1, 5)
    assert r.shape == rg.shape and np.array_equal(r[:, 0], rg[:, 0])
    matched = _iou(r[:, 1:], rg[:, 1:]) >= 1 - 1e-3
    assert matched.mean() >= 0.99, "only %.1f%% of rois match the reference by position" % (100 * matched.mean())
    assert np.abs(cls_prob.cpu().numpy() - g["cls_prob"])[matched].max() <= 1e-4
    assert np.abs(bbox_pred.cpu().numpy() - g["bbox_pred"])[matched].max() <= 1e-4


@pytest.mark.parametrize("use_ba", [True, False], ids=["ba", "cisa"])
def test_cached_forward_b1_is_bit_identical_to_uncached(dev, use_ba):
    """B = 1, C = 1: encode_supports issues exactly the support-side launches of the uncached B = 1 forward (same kernels,
    same shapes, no atomics in the forward contractions) and the cached forward hands their results to the same query-side
    launches (no gather at C = B = 1) -> the same bits"""
    m, _ = _model(dev, use_ba=use_ba)
    im, info, gt, nb, sup = _episode(dev, 1)
    with torch.no_grad():
        ref = _clone(m(im, info, gt, nb, sup))
        cache = m.encode_supports(_sets(sup))
        out = m(im, info, gt, nb, cache)
    assert len(cache) == 1 and cache.nbytes > 0
    _same(out, ref)


def test_selection_and_broadcast(dev):
    m, _ = _model(dev)
    im, info, gt, nb, sup = _episode(dev, 3)
    sets = _sets(sup)
    with torch.no_grad():
        cache = m.encode_supports(sets)
        assert len(cache) == 3
        # shot 3, L = 400, d = dq = 256: kp + unary + s_t + k2 + un2 + sw per set
        per_set = 4 * (1200 * 256 + 3 * 400 + 1024 * 1200 + 147 * 256 + 3 * 49 + 147 * 64)
        assert cache.nbytes == 3 * per_set
        cache.select([2, 0, 2])
        out = _clone(m(im, info, gt, nb, cache))
        ref = m(im, info, gt, nb, sets[[2, 0, 2]].reshape(3, 3, 3, 320, 320))
        _close(out, ref)
        # a CPU tensor selects too, and the identity is C == B's default for a fresh cache
        cache.select(torch.tensor([0, 1, 2]))
        _close(_clone(m(im, info, gt, nb, cache)), m(im, info, gt, nb, sup))
        # C = 1 broadcasts to every image
        one = m.encode_supports(sets[1:2])
        out = _clone(m(im[:2], info[:2], gt[:2], nb[:2], one))
        ref = m(im[:2], info[:2], gt[:2], nb[:2], sets[[1, 1]].reshape(2, 3, 3, 320, 320))
        _close(out, ref)
        with pytest.raises(IndexError):
            cache.select([0, 3, 1])
        with pytest.raises(IndexError):
            cache.select([-1, 0, 0])
        fresh = m.encode_supports(sets)
        with pytest.raises(RuntimeError, match="select"):
            m(im[:2], info[:2], gt[:2], nb[:2], fresh)  # C = 3, B = 2, no selection
        fresh.select([0, 1])
        with pytest.raises(RuntimeError, match="batch of 3"):
            m(im, info, gt, nb, fresh)  # two selected sets for three images


def test_cached_forward_issues_no_support_trunk_launches(dev):
    import dana_amd
    ops = dana_amd.ops
    m, _ = _model(dev)
    im, info, gt, nb, sup = _episode(dev, 1)
    m._single_stream = True
    try:
        with torch.no_grad():
            cache = m.encode_supports(_sets(sup))
            m(im, info, gt, nb, sup)  # (warm: plan and constants)
            ops.PROFILE = []
            m(im, info, gt, nb, sup)
            uncached = [e[0] for e in ops.PROFILE]
            ops.PROFILE = []
            m(im, info, gt, nb, cache)
            cached = [e[0] for e in ops.PROFILE]
            torch.cuda.synchronize()
    finally:
        ops.PROFILE = None
        m._single_stream = False
    stem = "conv7x7 M=%d " % (3 * 160 * 160)
    assert any(n.startswith(stem) for n in uncached)
    assert not any(n.startswith(stem) for n in cached), [n for n in cached if n.startswith("conv7x7")]
    assert len(uncached) - len(cached) >= 38, (len(uncached), len(cached))


def test_cache_invalidation(dev):
    import dana_amd
    ops = dana_amd.ops
    m, sd = _model(dev)
    im, info, gt, nb, sup = _episode(dev, 1)
    with torch.no_grad():
        cache = m.encode_supports(_sets(sup))
        m(im, info, gt, nb, cache)
        sd2 = dict(sd)
        sd2["rpn_unary_layer.weight"] = sd["rpn_unary_layer.weight"] * 1.5
        m.load_state_dict(sd2)
        with pytest.raises(RuntimeError, match="re-encode"):
            m(im, info, gt, nb, cache)
        cache = m.encode_supports(_sets(sup))
        ref = _clone(m(im, info, gt, nb, sup))
        _same(m(im, info, gt, nb, cache), ref)
        prev = ops.set_mfma_mode(1 - ops.get_mfma_mode())
        try:
            with pytest.raises(RuntimeError, match="re-encode"):
                m(im, info, gt, nb, cache)
        finally:
            ops.set_mfma_mode(prev)
        m(im, info, gt, nb, cache)  # (back to the mode it was encoded under)
        m.fold_roi_attn = False
        try:
            with pytest.raises(RuntimeError, match="re-encode"):
                m(im, info, gt, nb, cache)
            unfolded = m.encode_supports(_sets(sup))  # sp_pe instead of the folded table
            _close(m(im, info, gt, nb, unfolded), ref)
        finally:
            m.fold_roi_attn = True
        m.train()
        try:
            with pytest.raises(RuntimeError, match="eval"):
                m.encode_supports(_sets(sup))
            with pytest.raises(RuntimeError, match="eval"):
                m(im, info, gt, nb, cache)
        finally:
            m.eval()
        _same(m(im, info, gt, nb, cache), ref)


def test_program_replay_of_the_cached_forward(dev):
    from dana_amd.graphs import GraphedDAnA
    from dana_amd.program import ProgramDAnA
    m, _ = _model(dev)
    im, info, gt, nb, sup = _episode(dev, 2)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    with torch.no_grad():
        cache = m.encode_supports(sets)
        cache.select([2, 0])
        eager = _clone(m(im, info, gt, nb, cache))
        prog = ProgramDAnA(m, im, info, gt, nb, cache)
        _same(prog(im, info, gt, nb, cache), eager)
        cache.select([1, 1])  # between replays: the recorded gather reads the new index from device memory
        eager = _clone(m(im, info, gt, nb, cache))
        _same(prog(im, info, gt, nb, cache), eager)
        cache.select([0, 2])
        eager = _clone(m(im, info, gt, nb, cache))
        _same(prog(im, info, gt, nb, cache), eager)
        other = m.encode_supports(sets)
        other.select([0, 2])
        with pytest.raises(RuntimeError, match="different SupportCache"):
            prog(im, info, gt, nb, other)
        with pytest.raises(RuntimeError):
            prog(im, info, gt, nb, sup)
        cache.select([0, 1, 2])
        with pytest.raises(RuntimeError, match="batch of 2"):
            prog(im, info, gt, nb, cache)
        with pytest.raises(NotImplementedError):
            GraphedDAnA(m, im, info, gt, nb, cache)


def test_detections_batched_equals_per_image_loop(dev):
    from dana_amd import postprocess as PP
    m, _ = _model(dev)
    im, info, gt, nb, sup = _episode(dev, 3)
    with torch.no_grad():
        rois, cls_prob, bbox_pred = m(im, info, gt, nb, sup)[:3]
    B, R = rois.size(0), rois.size(1)
    cls_prob = cls_prob.clone()
    cls_prob[R:2 * R, 1] = 0.01  # image 1: every score below the 0.05 threshold -> no detection
    cls_prob[R:2 * R, 0] = 0.99
    loop = [PP.detections(rois[b:b + 1], cls_prob[b * R:(b + 1) * R], bbox_pred[b * R:(b + 1) * R], info[b:b + 1])
            for b in range(B)]
    batched, counts, offsets = PP.detections_batched(rois, cls_prob, bbox_pred, info, with_layout=True)
    assert len(batched) == B
    assert loop[1].shape == (0, 5) and batched[1].shape == (0, 5)
    assert loop[0].size(0) > 0 and loop[2].size(0) > 0
    for b in range(B):
        assert torch.equal(batched[b], loop[b]), b
    assert counts.tolist() == [t.size(0) for t in loop]
    assert offsets.tolist() == [0, loop[0].size(0), loop[0].size(0), loop[0].size(0) + loop[2].size(0)]
    plain = PP.detections_batched(rois, cls_prob, bbox_pred, info)  # (the plain form: the list only)
    assert all(torch.equal(a, b) for a, b in zip(plain, loop))
    # inclusive NMS (IoU >= thr) agrees as well
    loop_i = [PP.detections(rois[b:b + 1], cls_prob[b * R:(b + 1) * R], bbox_pred[b * R:(b + 1) * R], info[b:b + 1],
                            nms_inclusive=True) for b in range(B)]
    for a, b in zip(PP.detections_batched(rois, cls_prob, bbox_pred, info, nms_inclusive=True), loop_i):
        assert torch.equal(a, b)
