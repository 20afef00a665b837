"""Cached support sets and class sweeps of the support-conditioned siblings (`get_model('meta' | 'fsod' | 'fgn')`):
`encode_supports` -> SupportCache with the model's own per-set layout, the cached forward (one dana_gather_blocks launch
in place of the support trunk and chain), `cache.sweep(classes)` through `FasterRCNN._stages(group=C)`, and the three
kernels behind it (grouped depth-wise correlation, grouped channel scaling, Meta R-CNN's class head over a sweep).

End-to-end bars are test_gpu_support_cache.py's; the reference goldens' are test_gpu_model.py's sibling-golden bar
(every roi matched at IoU >= 1 - 1e-3, cls_prob / bbox_pred within 1e-4)."""
import numpy as np
import pytest
import torch

from test_gpu_support_cache import _clone, _close, _episode, _iou, _same, _sets

pytestmark = pytest.mark.gpu

MODELS = ["meta", "fsod", "fgn"]
CLASSES = [2, 0, 1]


@pytest.fixture(params=[1, 0], ids=["bf16x6", "f32mfma"])
def mfma_mode(request):
    import dana_amd
    prev = dana_amd.ops.set_mfma_mode(request.param)
    yield request.param
    dana_amd.ops.set_mfma_mode(prev)


def _tame(name):
    from dana_amd import synthetic as S
    return {"fsod": S.tame_fsod_weights, "fgn": S.tame_fgn_weights}.get(name, lambda sd_: sd_)


def _sibling(dev, name, shot=3, seed=11, way=1):
    """the sibling with test_gpu_model.py's golden-test weights"""
    import dana_amd
    from dana_amd import synthetic as S
    m = dana_amd.get_model(name, pretrained=False, way=way, shot=shot, classes=["fg", "bg"])
    sd = _tame(name)(S.fill_state_dict(m.state_dict(), seed=seed, profile="test"))
    m.load_state_dict(sd)
    return m.to(dev).eval(), sd


def _fwd(m, im, info, gt, nb, sup):
    """the model's forward; meta's anchor targets take every class's boxes as its 6th argument (meta.py:48,65)"""
    if type(m).__name__ == "MetaRCNN":
        return m(im, info, gt, nb, sup, gt)
    return m(im, info, gt, nb, sup)


def _replicated(m, cache, classes, im, info, gt, nb):
    """the per-class forward a sweep is defined by: every image repeated C times, set classes[c] for copy c"""
    C = len(classes)
    cache.select(list(classes) * im.size(0))
    rep = [t.repeat_interleave(C, 0) for t in (im, info, gt, nb)]
    return _fwd(m, *rep, cache)


def _profiled(m, fn):
    import dana_amd
    ops = dana_amd.ops
    fn()  # (warm: plan, constants, gathered buffers)
    ops.PROFILE = []
    try:
        fn()
        torch.cuda.synchronize()
        return [e[0] for e in ops.PROFILE]
    finally:
        ops.PROFILE = None


@pytest.mark.parametrize("name", MODELS)
def test_cached_b1_is_bit_identical_to_uncached(dev, name, mfma_mode):
    """B = 1, C = 1: encode_supports issues the uncached B = 1 forward's support-side launches, the cached forward hands
    their results to the same query-side launches (no gather) -> the same bits, and no support-trunk launch"""
    m, _ = _sibling(dev, name)
    im, info, gt, nb, sup = _episode(dev, 1)
    with torch.no_grad():
        ref = _clone(_fwd(m, im, info, gt, nb, sup))
        cache = m.encode_supports(_sets(sup))
        out = _fwd(m, im, info, gt, nb, cache)
        assert len(cache) == 1 and cache.nbytes > 0
        assert out[3:] == (0, 0, 0, 0, None)
        _same(out, ref)
        uncached = _profiled(m, lambda: _fwd(m, im, info, gt, nb, sup))
        cached = _profiled(m, lambda: _fwd(m, im, info, gt, nb, cache))
    stem = "conv7x7 M=%d " % (3 * 160 * 160)  # the support trunk's stem: shot 320 x 320 images
    assert any(n.startswith(stem) for n in uncached)
    assert not any(n.startswith(stem) for n in cached), [n for n in cached if n.startswith("conv7x7")]
    assert len(uncached) - len(cached) >= 38, (len(uncached), len(cached))


def _golden(golden_dir, dev, name):
    import dana_amd
    from dana_amd import synthetic as S
    g = np.load("%s/e2e_%s_eval_small.npz" % (golden_dir, name))
    training, B, way, shot, H, W, wseed, iseed, nseed = [int(v) for v in g["meta"]]
    assert not training
    m = dana_amd.get_model(name, pretrained=False, way=way, shot=shot, classes=["fg", "bg"])
    m.load_state_dict(_tame(name)(S.fill_state_dict(m.state_dict(), seed=wseed, profile="test")))
    m.to(dev)
    m.nms_inclusive = True  # the golden vectors come from the reference's CPU path (nms_cpu.cpp:60: >=)
    m.eval()
    return g, m, [t.to(dev) for t in S.episode_inputs(B, 1, shot, H, W, seed=iseed)]


@pytest.mark.parametrize("name", MODELS)
def test_cached_forward_matches_reference_golden(golden_dir, dev, name, mfma_mode):
    g, m, din = _golden(golden_dir, dev, name)
    with torch.no_grad():
        cache = m.encode_supports(_sets(din[4]))
        out = _fwd(m, *din[:4], cache)
    r, rg = out[0].cpu().numpy().reshape(-1, 5), g["rois"].reshape(-1, 5)
    assert r.shape == rg.shape and np.array_equal(r[:, 0], rg[:, 0])
    matched = _iou(r[:, 1:], rg[:, 1:]) >= 1 - 1e-3
    assert matched.all(), "only %.1f%% of rois match the reference by position" % (100 * matched.mean())
    assert np.abs(out[1].cpu().numpy() - g["cls_prob"]).max() <= 1e-4
    assert np.abs(out[2].cpu().numpy() - g["bbox_pred"]).max() <= 1e-4


@pytest.mark.parametrize("name", MODELS)
def test_sweep_matches_reference_golden(golden_dir, dev, name, mfma_mode):
    """the golden's support set encoded as set k = 1 of 3 (the others synthetic): block k of the sweep is the reference's
    own eval output"""
    g, m, din = _golden(golden_dir, dev, name)
    assert din[0].size(0) == 1
    shot = m.n_shot
    other = _sets(_episode(dev, 2, shot=shot, seed=5)[4])
    k = 1
    with torch.no_grad():
        cache = m.encode_supports(torch.cat([other[:1], _sets(din[4])[:1], other[1:]], 0))
        rois, cls_prob, bbox_pred = _fwd(m, *din[:4], cache.sweep())[:3]
    assert rois.size(0) == 3
    R = rois.size(1)
    r, rg = rois[k].cpu().numpy(), g["rois"].reshape(-1, 5)
    assert r.shape == rg.shape and (r[:, 0] == k).all()
    matched = _iou(r[:, 1:], rg[:, 1:]) >= 1 - 1e-3
    assert matched.mean() >= 0.99, "only %.1f%% of rois match the reference by position" % (100 * matched.mean())
    assert np.abs(cls_prob[k * R:(k + 1) * R].cpu().numpy() - g["cls_prob"])[matched].max() <= 1e-4
    assert np.abs(bbox_pred[k * R:(k + 1) * R].cpu().numpy() - g["bbox_pred"])[matched].max() <= 1e-4


@pytest.mark.parametrize("name", MODELS)
def test_selection_at_b4(dev, name, mfma_mode):
    m, _ = _sibling(dev, name)
    im, info, gt, nb, _ = _episode(dev, 4)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    idx = [2, 0, 2, 1]
    with torch.no_grad():
        cache = m.encode_supports(sets)
        assert len(cache) == 3
        cache.select(idx)
        out = _clone(_fwd(m, im, info, gt, nb, cache))
        ref = _fwd(m, im, info, gt, nb, sets[idx].reshape(4, 3, 3, 320, 320))
    assert out[3:] == (0, 0, 0, 0, None)
    _close(out, ref)


@pytest.mark.parametrize("name", MODELS)
def test_sweep_equals_replicated_cached_forward(dev, name, mfma_mode):
    m, _ = _sibling(dev, name)
    im, info, gt, nb, _ = _episode(dev, 2)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    with torch.no_grad():
        cache = m.encode_supports(sets)
        out = _clone(_fwd(m, im, info, gt, nb, cache.sweep(CLASSES)))
        ref = _replicated(m, cache, CLASSES, im, info, gt, nb)
        B, C, R = 2, len(CLASSES), out[0].size(1)
        assert out[0].shape == (B * C, R, 5) and out[1].shape == (B * C * R, 2) and out[2].shape == (B * C * R, 4)
        assert out[3:] == (0, 0, 0, 0, None)
        assert torch.equal(out[0][:, :, 0].cpu(), torch.arange(B * C).float().view(-1, 1).expand(B * C, R))
        _close(out, ref)
        # C = 1: one set for every image, as cache.select([c] * B)
        one = _clone(_fwd(m, im, info, gt, nb, cache.sweep([1])))
        cache.select([1, 1])
        _close(one, _fwd(m, im, info, gt, nb, cache))


@pytest.mark.parametrize("name", MODELS)
def test_sweep_launches_do_not_depend_on_classes(dev, name):
    m, _ = _sibling(dev, name)
    im, info, gt, nb, _ = _episode(dev, 2)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    counts = {}
    with torch.no_grad():
        cache = m.encode_supports(sets)
        for cl in ([0], CLASSES):
            counts[len(cl)] = _profiled(m, lambda: _fwd(m, im, info, gt, nb, cache.sweep(cl)))
    assert len(counts[3]) == len(counts[1]), (len(counts[3]), len(counts[1]))
    stems = [n for n in counts[3] if n.startswith("conv7x7")]
    assert len(stems) == 1 and stems[0].startswith("conv7x7 M=%d " % (2 * 96 * 128)), stems  # B images, not B*C
    if name == "meta":
        # RPN, proposals, RoIAlign, layer4 and the box head run once per image (B*R rois): every contraction is C's = 1
        assert counts[3] == counts[1]


@pytest.mark.parametrize("ragged", [False, True], ids=["even", "ragged"])
def test_grouped_depthwise_corr_equals_replicated_map(dev, ragged):
    import dana_amd
    ops = dana_amd.ops
    gen = torch.Generator().manual_seed(5)
    group, n_maps, H, W, ch, kh, kw, ld = (3, 6, 38, 63, 1024, 7, 7, 1024) if not ragged else (3, 5, 11, 15, 36, 3, 5, 44)
    n_img = (n_maps + group - 1) // group
    feat = torch.randn(n_img * H * W, ld, generator=gen).to(dev)
    kern = torch.randn(n_maps, kh * kw, ch, generator=gen).to(dev)
    got, oh, ow = ops.depthwise_corr_grouped(feat, kern, n_maps, H, W, ch, kh, kw, group, feat_stride=ld)
    assert (oh, ow) == (H - kh + 1, W - kw + 1)
    rep = feat.view(n_img, H * W, ld).repeat_interleave(group, 0)[:n_maps].reshape(-1, ld).contiguous()
    ref, _, _ = ops.depthwise_corr(rep, kern, n_maps, H, W, ch, kh, kw, feat_stride=ld)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("ragged", [False, True], ids=["even", "ragged"])
def test_grouped_scale_rows_equals_replicated_rows(dev, ragged):
    import dana_amd
    ops = dana_amd.ops
    gen = torch.Generator().manual_seed(6)
    group, n_blocks, rows, ch, ld = (3, 6, 38 * 63, 1024, 1024) if not ragged else (3, 5, 37, 20, 28)
    n_img = (n_blocks + group - 1) // group
    x = torch.randn(n_img * rows, ld, generator=gen).to(dev)
    vec = torch.rand(n_blocks, ch, generator=gen).to(dev)
    got = ops.scale_rows_grouped(x, vec, rows, ch, group, n_blocks, ld_x=ld)
    rep = x.view(n_img, rows, ld)[:, :, :ch].repeat_interleave(group, 0)[:n_blocks].reshape(-1, ch).contiguous()
    ref = ops.scale_rows_by_group(rep, vec, n_blocks * rows, rows, ch)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("C", [1, 3])
def test_meta_class_head_vs_float64(dev, C):
    import dana_amd
    ops = dana_amd.ops
    gen = torch.Generator().manual_seed(C)
    B, R, K = 2, 37, 2048
    fc7 = torch.rand(B * R, K, generator=gen) * 2
    vec = torch.sigmoid(torch.randn(B * C, K, generator=gen))
    w = torch.randn(2, K, generator=gen) * 0.05
    bias = torch.randn(2, generator=gen) * 0.1
    rois = torch.rand(B, R, 5, generator=gen) * 500
    rois[:, :, 0] = torch.arange(B).float().view(-1, 1)
    bbox = torch.randn(B * R, 4, generator=gen)
    rois_o, prob, bbox_o = ops.meta_class_head(fc7.to(dev), vec.to(dev), w.to(dev), bias.to(dev), rois.to(dev),
                                               bbox.to(dev), B, C, R, K)
    rois_o, prob, bbox_o = rois_o.cpu(), prob.cpu(), bbox_o.cpu()
    assert rois_o.shape == (B * C, R, 5) and prob.shape == (B * C * R, 2) and bbox_o.shape == (B * C * R, 4)
    for b in range(B):
        for c in range(C):
            p = b * C + c
            comb = (fc7[b * R:(b + 1) * R] * vec[p]).double()  # (the product rounded to fp32, as the cached head's)
            ref = torch.softmax(comb @ w.double().t() + bias.double(), 1)
            got = prob[p * R:(p + 1) * R].double()
            assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), (b, c)
            assert torch.equal(rois_o[p, :, 1:], rois[b, :, 1:]) and (rois_o[p, :, 0] == p).all()
            assert torch.equal(bbox_o[p * R:(p + 1) * R], bbox[b * R:(b + 1) * R])


@pytest.mark.parametrize("name", MODELS)
def test_detections_by_class_on_a_sibling_sweep(dev, name):
    from dana_amd import postprocess as PP
    m, _ = _sibling(dev, name)
    im, info, gt, nb, _ = _episode(dev, 2)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    with torch.no_grad():
        cache = m.encode_supports(sets)
        rois, cls_prob, bbox_pred = _fwd(m, im, info, gt, nb, cache.sweep(CLASSES))[:3]
    B, C, R = 2, 3, rois.size(1)
    dets = PP.detections_by_class(rois, cls_prob, bbox_pred, info, C)
    assert len(dets) == B and all(len(d) == C for d in dets)
    for b in range(B):
        for c in range(C):
            p = b * C + c
            ref = PP.detections(rois[p:p + 1], cls_prob[p * R:(p + 1) * R], bbox_pred[p * R:(p + 1) * R], info[b:b + 1])
            assert torch.equal(dets[b][c], ref), (b, c)


@pytest.mark.parametrize("name", MODELS)
def test_sibling_cache_validation(dev, name):
    import dana_amd
    from dana_amd import synthetic as S
    from dana_amd.config import cfg
    m, sd = _sibling(dev, name)
    im, info, gt, nb, sup = _episode(dev, 1)
    sets = _sets(_episode(dev, 2, seed=7)[4])
    with torch.no_grad():
        cache = m.encode_supports(sets)
        _fwd(m, im, info, gt, nb, cache.sweep([0, 1]))
        m.train()
        try:
            with pytest.raises(RuntimeError, match="eval"):
                m.encode_supports(sets)
            with pytest.raises(RuntimeError, match="eval"):
                _fwd(m, im, info, gt, nb, cache.sweep([0, 1]))
        finally:
            m.eval()
        # another model: a second instance of the same kind, a DAnA model, and a DAnA cache here
        other, _ = _sibling(dev, name)
        with pytest.raises(RuntimeError, match="another model"):
            _fwd(other, im, info, gt, nb, cache)
        dana = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=3, classes=["fg", "bg"])
        dana.load_state_dict(S.fill_state_dict(dana.state_dict(), seed=11, profile="test"))
        dana.to(dev).eval()
        with pytest.raises(RuntimeError, match="another model"):
            dana(im, info, gt, nb, cache)
        with pytest.raises(RuntimeError, match="another model"):
            _fwd(m, im, info, gt, nb, dana.encode_supports(sets[:1]))
        with pytest.raises(ValueError):
            m.encode_supports(sets[:, :2])  # 2 shots for a 3-shot model
        small = _sets(S.episode_inputs(1, 1, 3, 64, 64, seed=3, support_size=224)[4].to(dev))
        with pytest.raises(RuntimeError, match="320x320"):
            m.encode_supports(small)
        prev = cfg.POOLING_MODE
        cfg.POOLING_MODE = "pool"
        try:
            with pytest.raises(NotImplementedError):
                _fwd(m, im, info, gt, nb, cache.sweep([0, 1]))
        finally:
            cfg.POOLING_MODE = prev
        sd2 = dict(sd)
        k = next(k for k in sd if k.startswith("RCNN_bbox_pred.weight"))
        sd2[k] = sd[k] * 1.5
        m.load_state_dict(sd2)
        with pytest.raises(RuntimeError, match="re-encode"):
            _fwd(m, im, info, gt, nb, cache)
        with pytest.raises(RuntimeError, match="re-encode"):
            _fwd(m, im, info, gt, nb, cache.sweep([0, 1]))


def test_frcnn_has_no_support_sets_to_encode(dev):
    import dana_amd
    m = dana_amd.get_model("frcnn", pretrained=False, classes=["fg", "bg"]).to(dev).eval()
    sets = _sets(_episode(dev, 1, seed=7)[4])
    with pytest.raises(TypeError, match="no support branch"):
        m.encode_supports(sets)
