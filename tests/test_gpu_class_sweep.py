"""Class sweep: `model(im_data, im_info, gt_boxes, num_boxes, cache.sweep(classes))` runs each of B query images against each
of C cached support sets (B*C problems p = b*C + c, the query trunk once per image), its kernels (class-interleaved
softmax, RPN conv split by input channels with a grouped residual, RoIAlign with a group divisor), its launch-program
replay and `postprocess.detections_by_class`.

End-to-end bars are test_gpu_support_cache.py's (IoU >= 1 - 1e-3 for >= 99 % of the rois, cls_prob / bbox_pred within
1e-4 on the matched rois); the split conv's is test_gpu_contractions.py's test_winograd_3x3_vs_torch bar."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_support_cache import _build, _clone, _close, _episode, _iou, _load, _model, _same, _sets

pytestmark = pytest.mark.gpu

CLASSES = [2, 0, 1]
_CONV_REF = {}


@pytest.fixture(params=[1, 0], ids=["bf16x6", "f32mfma"])
def mfma_mode(request):
    import dana_amd
    prev = dana_amd.ops.set_mfma_mode(request.param)
    yield request.param
    dana_amd.ops.set_mfma_mode(prev)


def _variant(dev, kind):
    if kind == "product":  # the product golden's configuration (test_gpu_support_cache._build): BA on, tamed weights
        m, _, _ = _build(np.array([1, 0, 1, 1, 3, 192, 256, 11, 1996, 7, 1]), dev)
        m.nms_inclusive = False
        return m
    return _model(dev, use_ba=(kind == "concat_ba"))[0]


def _replicated(m, cache, classes, im, info, gt, nb):
    """the per-class forward the sweep is defined by: every image repeated C times, set classes[c] for copy c"""
    C = len(classes)
    cache.select(list(classes) * im.size(0))
    return m(im.repeat_interleave(C, 0), info.repeat_interleave(C, 0), gt.repeat_interleave(C, 0),
             nb.repeat_interleave(C, 0), cache)


@pytest.mark.parametrize("kind", ["concat_ba", "concat_cisa", "product"])
def test_sweep_matches_per_class_forward(dev, kind, mfma_mode):
    m = _variant(dev, kind)
    im, info, gt, nb, _ = _episode(dev, 2)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    with torch.no_grad():
        cache = m.encode_supports(sets)
        out = _clone(m(im, info, gt, nb, cache.sweep(CLASSES)))
        ref = _replicated(m, cache, CLASSES, im, info, gt, nb)
        B, C, R = 2, len(CLASSES), out[0].size(1)
        assert out[0].shape == (B * C, R, 5) and out[1].shape == (B * C * R, 2) and out[2].shape == (B * C * R, 4)
        assert out[3:] == (0, 0, 0, 0, None)
        assert torch.equal(out[0][:, :, 0].cpu(), torch.arange(B * C).float().view(-1, 1).expand(B * C, R))
        _close(out, ref)
        # C = 1: one set for every image, as cache.select([c] * B)
        one = _clone(m(im, info, gt, nb, cache.sweep([1])))
        cache.select([1, 1])
        _close(one, m(im, info, gt, nb, cache))


@pytest.mark.parametrize("tag", ["eval_small_cisa", "eval_small_ba", "eval_full_ba", "eval_small_product"])
def test_sweep_matches_reference_golden(golden_dir, dev, tag, mfma_mode):
    """the golden's support set encoded as set k = 1 of 3 (the others synthetic): block k of the sweep is the reference's
    own eval output"""
    g = _load(golden_dir, tag)
    m, _, din = _build(g["meta"], dev)
    shot = int(g["meta"][4])
    other = _sets(_episode(dev, 2, shot=shot, seed=5)[4])
    k = 1
    with torch.no_grad():
        sets = torch.cat([other[:1], _sets(din[4])[:1], other[1:]], 0)
        cache = m.encode_supports(sets)
        rois, cls_prob, bbox_pred = m(*din[:4], cache.sweep())[:3]
    assert rois.size(0) == 3
    R = rois.size(1)
    r, rg = rois[k].cpu().numpy(), g["rois"].reshape(-1, 5)
    assert r.shape == rg.shape and (r[:, 0] == k).all()
    matched = _iou(r[:, 1:], rg[:, 1:]) >= 1 - 1e-3
    assert matched.mean() >= 0.99, "only %.1f%% of rois match the reference by position" % (100 * matched.mean())
    assert np.abs(cls_prob[k * R:(k + 1) * R].cpu().numpy() - g["cls_prob"])[matched].max() <= 1e-4
    assert np.abs(bbox_pred[k * R:(k + 1) * R].cpu().numpy() - g["bbox_pred"])[matched].max() <= 1e-4


def test_grouped_roi_align_equals_replicated_map(dev):
    import dana_amd
    ops = dana_amd.ops
    B, C, H, W, ch, R = 2, 3, 38, 63, 1024, 200
    gen = torch.Generator().manual_seed(3)
    feat = torch.randn(B * H * W, 2048, generator=gen).to(dev)
    x1 = torch.rand(R, generator=gen) * 900
    y1 = torch.rand(R, generator=gen) * 500
    rois = torch.stack([torch.randint(0, B * C, (R,), generator=gen).float(), x1, y1,
                        x1 + torch.rand(R, generator=gen) * 300, y1 + torch.rand(R, generator=gen) * 200], 1).to(dev)
    rep = feat.view(B, H * W, 2048).repeat_interleave(C, 0).reshape(-1, 2048).contiguous()
    pe = torch.randn(49, ch, generator=gen).to(dev)
    for kw in ({}, {"pe": pe}):
        got = ops.roi_align_forward_nhwc(feat, B, H, W, ch, 2048, rois, 1.0 / 16.0, 7, 0, group=C, **kw)
        ref = ops.roi_align_forward_nhwc(rep, B * C, H, W, ch, 2048, rois, 1.0 / 16.0, 7, 0, **kw)
        for a, b in zip(got, ref):
            assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("C", [1, 3])
def test_sweep_softmax_equals_attn_softmax_unary(dev, C):
    import dana_amd
    ops = dana_amd.ops
    B, hw, shot, L = 2, 150, 3, 400
    K1 = shot * L
    gen = torch.Generator().manual_seed(C)
    scores = (torch.randn(B, hw, C * K1, generator=gen) * 4).to(dev)
    unary = torch.softmax(torch.randn(B * C, shot, L, generator=gen), -1).to(dev)
    out = torch.full((B * C, hw, K1), 7.0, device=dev)
    ops.attn_softmax_unary_sweep(scores, out, unary, B, C, hw, shot, L, K1, K1, K1, 0.1, 1.0 / shot)
    ref = scores.view(B, hw, C, K1).permute(0, 2, 1, 3).contiguous()  # problem-major copy: [B*C][hw][K1]
    ops.attn_softmax_unary_(ref, unary, B * C * hw, hw, shot, L, K1, K1, 0.1, 1.0 / shot)
    assert torch.equal(out, ref.view(B * C, hw, K1))


@pytest.mark.parametrize("winograd", [True, False], ids=["winograd", "igemm"])
def test_split_rpn_conv_with_grouped_residual_vs_torch(dev, winograd, mfma_mode):
    """RPN shape: cin 2048 = [base_feat | attended], cout 512, a 38 x 63 map, B = 2 images x C = 3 problems"""
    import dana_amd
    ops = dana_amd.ops
    m = _model(dev)[0]
    m.use_winograd = winograd
    B, C, fh, fw = 2, 3, 38, 63
    hw = fh * fw
    gen = torch.Generator().manual_seed(17)
    base = torch.randn(B, hw, 1024, generator=gen)
    att = torch.randn(B * C, hw, 1024, generator=gen)
    with torch.no_grad():
        plan = m._get_plan()
        assert (plan["rpn_conv_u"] is not None) == winograd
        corr = torch.cat([base, torch.zeros_like(base)], 2).reshape(-1, 2048).to(dev)
        x = m._rpn_conv_sweep(plan, corr, att.reshape(-1, 1024).to(dev), B, C, fh, fw, False)
        got = ops.nhwc_to_nchw(x, B * C, 512, fh, fw).cpu()
        w = m.RCNN_rpn.RPN_Conv.weight.detach().cpu()
        bias = m.RCNN_rpn.RPN_Conv.bias.detach().cpu()
    key = (B, C, fh, fw)
    if key not in _CONV_REF:  # (the same weights and inputs for every parametrisation: one CPU conv)
        full = torch.cat([base.repeat_interleave(C, 0), att], 2).view(B * C, fh, fw, 2048).permute(0, 3, 1, 2)
        _CONV_REF[key] = F.relu(F.conv2d(full, w, bias, padding=1))
    a, b = got.double(), _CONV_REF[key].double()
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert err <= 1e-4 * scale, "max err %.3e vs scale %.3e" % (err, scale)


def test_sweep_launches_do_not_depend_on_classes(dev):
    import dana_amd
    ops = dana_amd.ops
    m, _ = _model(dev)
    im, info, gt, nb, _ = _episode(dev, 2)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    counts = {}
    m._single_stream = True
    try:
        with torch.no_grad():
            cache = m.encode_supports(sets)
            for cl in ([0], CLASSES):
                m(im, info, gt, nb, cache.sweep(cl))  # (warm: plan, split filters, gathered buffers)
                ops.PROFILE = []
                m(im, info, gt, nb, cache.sweep(cl))
                counts[len(cl)] = [e[0] for e in ops.PROFILE]
                torch.cuda.synchronize()
    finally:
        ops.PROFILE = None
        m._single_stream = False
    assert len(counts[3]) == len(counts[1]), (len(counts[3]), len(counts[1]))
    stems = [n for n in counts[3] if n.startswith("conv7x7")]
    assert len(stems) == 1 and stems[0].startswith("conv7x7 M=%d " % (2 * 96 * 128)), stems  # B images, not B*C


def test_program_replay_of_a_sweep(dev):
    from dana_amd.graphs import GraphedDAnA
    from dana_amd.program import ProgramDAnA
    m, _ = _model(dev)
    im, info, gt, nb, _ = _episode(dev, 2)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    with torch.no_grad():
        cache = m.encode_supports(sets)
        sw = cache.sweep(CLASSES)
        eager = _clone(m(im, info, gt, nb, sw))
        prog = ProgramDAnA(m, im, info, gt, nb, sw)
        _same(prog(im, info, gt, nb, sw), eager)
        sw2 = cache.sweep([1, 2, 2])  # same C, other sets: the recorded gather reads the new index
        eager2 = _clone(m(im, info, gt, nb, sw2))
        _same(prog(im, info, gt, nb, sw2), eager2)
        assert not torch.equal(eager2[1], eager[1])
        with pytest.raises(RuntimeError, match="re-record"):
            prog(im, info, gt, nb, cache.sweep([0, 1]))
        with pytest.raises(RuntimeError, match="re-record"):
            prog(im, info, gt, nb, m.encode_supports(sets).sweep(CLASSES))
        with pytest.raises(RuntimeError, match="re-record"):
            prog(im, info, gt, nb, cache)
        with pytest.raises(NotImplementedError):
            GraphedDAnA(m, im, info, gt, nb, sw)


def test_detections_by_class_equals_per_problem_detections(dev):
    from dana_amd import postprocess as PP
    m, _ = _model(dev)
    im, info, gt, nb, _ = _episode(dev, 2)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    with torch.no_grad():
        cache = m.encode_supports(sets)
        rois, cls_prob, bbox_pred = m(im, info, gt, nb, cache.sweep(CLASSES))[:3]
    B, C, R = 2, 3, rois.size(1)
    dets = PP.detections_by_class(rois, cls_prob, bbox_pred, info, C)
    assert len(dets) == B and all(len(d) == C for d in dets)
    for b in range(B):
        for c in range(C):
            p = b * C + c
            ref = PP.detections(rois[p:p + 1], cls_prob[p * R:(p + 1) * R], bbox_pred[p * R:(p + 1) * R], info[b:b + 1])
            assert torch.equal(dets[b][c], ref), (b, c)
    with pytest.raises(ValueError):
        PP.detections_by_class(rois, cls_prob, bbox_pred, info, 2)


def test_sweep_validation(dev):
    m, sd = _model(dev)
    im, info, gt, nb, _ = _episode(dev, 1)
    sets = _sets(_episode(dev, 3, seed=7)[4])
    with torch.no_grad():
        cache = m.encode_supports(sets)
        assert len(cache.sweep()) == 3 and cache.sweep(torch.tensor([2, 0])).classes == (2, 0)
        with pytest.raises(ValueError):
            cache.sweep([])
        with pytest.raises(IndexError):
            cache.sweep([0, 3])
        with pytest.raises(IndexError):
            cache.sweep([-1])
        with pytest.raises(ValueError):
            cache.sweep(torch.tensor([0, 1], device=dev))
        m.train()
        try:
            with pytest.raises(RuntimeError, match="eval"):
                m(im, info, gt, nb, cache.sweep([0, 1]))
        finally:
            m.eval()
        sd2 = dict(sd)
        sd2["rpn_unary_layer.weight"] = sd["rpn_unary_layer.weight"] * 1.5
        m.load_state_dict(sd2)
        with pytest.raises(RuntimeError, match="re-encode"):
            m(im, info, gt, nb, cache.sweep([0, 1]))
