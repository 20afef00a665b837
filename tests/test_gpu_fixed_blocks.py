"""Training with cfg.RESNET.FIXED_BLOCKS 0, 2 and 3 (1 is what every other training test runs): the saving forward, the HIP
backward, Trainer and the launch-program replay follow the trunk's freeze prefix, for DAnA and the four siblings.
Small shape throughout: B 2, way 2, shot 1, query 128x160, supports 320x320, `test` weight profile, nms_inclusive."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, WAY, SHOT, H, W = 2, 2, 1, 128, 160
WEIGHTS = (1.0, 0.5, 2.0, 1.5)
SEEDS = (23, 24, 26, 27, 29, 30)
N_COMPARED = {0: 80, 1: 70, 2: 57, 3: 38}  # DAnA with the BA block: trainable tensors per FIXED_BLOCKS


@pytest.fixture(params=[1, 0], ids=["bf16x6", "f32mfma"])
def mfma_mode(request):
    from dana_amd import ops
    prev = ops.set_mfma_mode(request.param)
    yield request.param
    ops.set_mfma_mode(prev)


def _build(name, k, dev, sd_seed=21, way=WAY, shot=SHOT, **kw):
    """the model built under cfg.RESNET.FIXED_BLOCKS = k (restored behind the constructor) -> (model on dev in train mode, sd)"""
    import dana_amd
    from dana_amd import synthetic as S
    from dana_amd.config import cfg
    prev = cfg.RESNET.FIXED_BLOCKS
    cfg.RESNET.FIXED_BLOCKS = k
    try:
        m = dana_amd.get_model(name, pretrained=False, way=way, shot=shot, classes=["fg", "bg"], **kw)
    finally:
        cfg.RESNET.FIXED_BLOCKS = prev
    sd = S.fill_state_dict(m.state_dict(), seed=sd_seed, profile="test")
    if name == "fsod":
        sd = S.tame_fsod_weights(sd)
    m.load_state_dict(sd)
    m.to(dev).train()
    m.nms_inclusive = True
    return m, sd


def _trainable(key, k):
    """the oracle's state-dict tensors that train under FIXED_BLOCKS = k (dana.py:350-385)"""
    if key in ("bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias"):
        return True  # fgn's head BatchNorms are ordinary, trainable layers (fgn.py:31-36)
    if "bn" in key or "downsample.1" in key or "running_" in key or "num_batches" in key:
        return False
    frozen = ("RCNN_base.0", "RCNN_base.1") + tuple("RCNN_base.%d." % (4 + li) for li in range(k))
    return not key.startswith(frozen)


def _episode(name, seed):
    from dana_amd import synthetic as S
    e = S.episode_inputs(B, WAY, SHOT, H, W, seed=seed)
    if name in ("DAnA", "fgn", "fsod"):
        return list(e)
    return list(e[:4]) if name == "frcnn" else list(e) + [e[2].clone()]  # meta.py:39,48: all_cls_gt_boxes


def _oracle(name, state, inputs, **kw):
    from oracle import model_ref as O
    if name == "DAnA":
        return O.forward(state, *inputs, training=True, n_way=WAY, n_shot=SHOT, use_ba=True, nms_inclusive=True, **kw)
    if name == "frcnn":
        return O.frcnn_forward(state, *inputs, training=True, nms_inclusive=True, **kw)
    fwd = dict(fgn=O.fgn_forward, fsod=O.fsod_forward, meta=O.meta_forward)[name]
    return fwd(state, *inputs, training=True, n_way=WAY, n_shot=SHOT, nms_inclusive=True, **kw)


_PROBE, _GRADS = {}, {}  # the oracle's CPU runs depend on neither the MFMA mode nor (the forward) on k: once per process


def _forward_on_agreeing_seed(name, m, sd, dev):
    """the first input seed on which the HIP forward and the oracle sample the same rois (test_gpu_backward.py: near ties
    in this tiny model's proposal ranking are decided by fp32 round-off) -> (seed, inputs, HIP outputs); the forward saved"""
    m.save_for_backward = True
    for seed in SEEDS:
        inputs = _episode(name, seed)
        np.random.seed(33)
        with torch.no_grad():
            res = m(*[t.to(dev) for t in inputs])
        if (name, seed) not in _PROBE:
            np.random.seed(33)
            with torch.no_grad():
                _PROBE[(name, seed)] = _oracle(name, sd, inputs)
        probe = _PROBE[(name, seed)]
        if np.array_equal(res[7].cpu().numpy(), probe[7].numpy()) and (res[0].cpu() - probe[0]).abs().max().item() < 0.05:
            return seed, inputs, res
    pytest.fail("no seed on which the HIP forward and the oracle sample the same rois")


def _oracle_grads(name, k, seed, sd, inputs):
    key = (name, k, seed)
    if key not in _GRADS:
        osd = {n: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and _trainable(n, k) else v.clone())
               for n, v in sd.items()}
        np.random.seed(33)
        out = _oracle(name, osd, inputs, differentiable=True)
        sum(wt * l for wt, l in zip(WEIGHTS, out[3:7])).backward()
        _GRADS[key] = (osd, out)
    return _GRADS[key]


def _compare(m, osd, l2_bound=None):
    """test_gpu_backward.py:194-215: max relative error with the 1e-3 * gmax floor (biases in front of a mean subtraction /
    softmax have an exactly-zero gradient), and the relative L2 error -> the number of tensors compared"""
    params = dict(m.named_parameters())
    ref = {n: v.grad for n, v in osd.items() if v.dtype.is_floating_point and v.requires_grad}
    gmax = max(g.abs().max().item() for g in ref.values())
    worst, worst_l2 = [], []
    for n, gr in ref.items():
        g = params[n].grad
        assert g is not None, "no HIP gradient for %s" % n
        scale = gr.abs().max().item() + 1e-3 * gmax
        worst.append(((g.cpu() - gr).abs().max().item() / scale, n))
        worst_l2.append(((g.cpu() - gr).double().norm().item()
                         / (gr.double().norm().item() + 1e-3 * gmax * gr.numel() ** 0.5), n))
    worst.sort(reverse=True)
    worst_l2.sort(reverse=True)
    print("largest relative gradient errors: max %s, L2 %s" % (worst[:3], worst_l2[:3]))
    assert worst[0][0] <= 5e-3, "largest relative gradient errors: %s" % (worst[:8],)
    if l2_bound is not None:
        assert worst_l2[0][0] <= l2_bound, "largest relative L2 gradient errors: %s" % (worst_l2[:8],)
    return len(ref)


@pytest.mark.parametrize("k", [0, 2, 3])
def test_dana_backward_vs_oracle_autograd(dev, mfma_mode, k):
    """every trainable parameter's gradient under FIXED_BLOCKS = k against autograd through the oracle at the bounds of
    test_gpu_backward.py (5e-3 max relative with the 1e-3 * gmax floor, 1.5e-3 relative L2); frozen ones keep grad None"""
    from dana_amd import backward as BW
    m, sd = _build("DAnA", k, dev, use_BA_block=True)
    seed, inputs, res = _forward_on_agreeing_seed("DAnA", m, sd, dev)
    ctx = m._ctx
    assert ctx["t"] == k
    assert [s["key"] for s in ctx["q_saved"]] == [s["key"] for s in ctx["s_saved"]] == [
        "RCNN_base.%d.%d" % (4 + li, bi) for li in range(k, 3) for bi in range(len(m.RCNN_base[4 + li]))]
    osd, out = _oracle_grads("DAnA", k, seed, sd, inputs)
    for a, b in zip(res[3:7], out[3:7]):
        assert abs(float(a) - float(b.detach())) <= 1e-4 * max(1.0, abs(float(b.detach())))
    BW.model_backward(m, WEIGHTS)
    torch.cuda.synchronize()
    assert m._ctx is None and ctx.get("consumed")
    assert _compare(m, osd, l2_bound=1.5e-3) == N_COMPARED[k]
    for n, p in m.named_parameters():
        assert (p.grad is None) == (not p.requires_grad), n
    if k == 0:
        assert max(m.get_parameter("RCNN_base.4.%d.conv2.weight" % b).grad.abs().max().item() for b in range(3)) > 0


_HIP_GRADS = {}


def _hip_grads(dev, k, mode):
    """DAnA's gradients under FIXED_BLOCKS = k on the inputs of seed 23 (one run per k and MFMA mode)"""
    from dana_amd import backward as BW
    if (k, mode) not in _HIP_GRADS:
        m, _ = _build("DAnA", k, dev, use_BA_block=True)
        m.save_for_backward = True
        np.random.seed(33)
        with torch.no_grad():
            m(*[t.to(dev) for t in _episode("DAnA", 23)])
        BW.model_backward(m, WEIGHTS)
        torch.cuda.synchronize()
        _HIP_GRADS[(k, mode)] = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return _HIP_GRADS[(k, mode)]


@pytest.mark.parametrize("k", [2, 3])
def test_freezing_more_only_removes_launches(dev, mfma_mode, k):
    """FIXED_BLOCKS = k against 1 on the same inputs: the gradients of the parameters trainable in both are torch.equal --
    the launches that are left are the same launches on the same operands (the weight gradients reduce in a fixed slice
    order and RoIAlign's adjoint is the deterministic gather form). No surviving launch was shrunk, so no parameter is
    exempt."""
    one, got = _hip_grads(dev, 1, mfma_mode), _hip_grads(dev, k, mfma_mode)
    assert len(one) == N_COMPARED[1] and len(got) == N_COMPARED[k] and set(got) < set(one)
    unequal = [n for n in got if not torch.equal(got[n], one[n])]
    print("k = %d: %d of %d shared gradients differ from k = 1: %s" % (k, len(unequal), len(got), unequal[:6]))
    assert not unequal


def _backward_launches(m, dev, inputs):
    """(C-ABI entry points the backward of one saved forward issues, keys of its conv weight-gradient launch groups, ctx)"""
    from dana_amd import _lib, backward as BW

    class Names:
        names = []

        def add_call(self, fn, name, args):
            self.names.append(name)

    m.save_for_backward = True
    np.random.seed(33)
    with torch.no_grad():
        m(*[t.to(dev) for t in inputs])
    ctx, keys, add_conv = m._ctx, [], BW.WeightGrads.add_conv

    def spy(self, key, *a, **kw):
        keys.append(key)
        return add_conv(self, key, *a, **kw)

    saved = {k_: len(ctx[k_]) for k_ in ("q_saved", "s_saved", "m_saved", "l4_saved")}
    rec = Names()
    rec.names = []
    BW.WeightGrads.add_conv, _lib.RECORDER = spy, rec
    try:
        BW.model_backward(m, WEIGHTS)
    finally:
        BW.WeightGrads.add_conv, _lib.RECORDER = add_conv, None
    torch.cuda.synchronize()
    return rec.names, keys, saved


@pytest.mark.parametrize("merged", [False, True], ids=["two-buffer", "trainer-merged"])
def test_frozen_trunk_backward_issues_nothing_for_the_trunk(dev, merged):
    """FIXED_BLOCKS = 3: no RoI-pooling adjoint, no support-map average-pool adjoint, exactly layer4's ten conv weight
    gradients and RPN_Conv's, nothing saved below layer4 -- and every head / RPN / layer4 launch of k = 1 that writes a
    weight gradient is still there (the gradients are checked against the oracle above)"""
    m, _ = _build("DAnA", 3, dev, use_BA_block=True)
    if merged:
        m._train_merge = (True, 3)  # what a Trainer sets for its saving forwards
    names, keys, saved = _backward_launches(m, dev, _episode("DAnA", 23))
    assert saved == dict(q_saved=0, s_saved=0, m_saved=0, l4_saved=3)
    assert not [n for n in names if "roi_align_backward" in n or "roi_pool_backward" in n], names
    assert "dana_avgpool_backward_nhwc" not in names
    assert "dana_upsample_scatter_nhwc" not in names  # layer4's first block: no input gradient either
    want = ["RCNN_top.0.%d.%s" % (b, c) for b in (2, 1, 0) for c in ("conv3", "conv2", "conv1")] + ["RCNN_top.0.0.downsample.0"]
    assert sorted(keys) == sorted(want + ["RCNN_rpn.RPN_Conv"]) and len(keys) == 11
    m1, _ = _build("DAnA", 1, dev, use_BA_block=True)
    names1, keys1, saved1 = _backward_launches(m1, dev, _episode("DAnA", 23))
    assert saved1["q_saved"] == saved1["s_saved"] == 10 and len(keys1) > 11
    assert any("roi_align_backward" in n for n in names1) and "dana_avgpool_backward_nhwc" in names1
    assert len(names) < len(names1)
    print("backward launches: k = 3 %d, k = 1 %d" % (len(names), len(names1)))


def test_frozen_trunk_without_the_ba_block(dev):
    """FIXED_BLOCKS = 3 with semantic_enhance off: nothing reads the gradient into the positive supports' PE-added maps,
    so the RPN chain makes no such buffer (its attention adjoint and the unary term's run without a value / input
    gradient). Same launch conditions as with the block, and every gradient bit-equal to the k = 1 run's, whose path
    test_gpu_backward.py checks against the oracle"""
    m, _ = _build("DAnA", 3, dev, use_BA_block=False)
    names, keys, saved = _backward_launches(m, dev, _episode("DAnA", 23))
    assert saved == dict(q_saved=0, s_saved=0, m_saved=0, l4_saved=3) and len(keys) == 11
    assert not [n for n in names if "roi_align_backward" in n or "roi_pool_backward" in n or "avgpool_backward" in n]
    assert "dana_ba_backward" not in names
    m1, _ = _build("DAnA", 1, dev, use_BA_block=False)
    names1, _, _ = _backward_launches(m1, dev, _episode("DAnA", 23))
    got = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    one = {n: p.grad for n, p in m1.named_parameters() if p.grad is not None}
    assert len(got) == N_COMPARED[3] - 2 and len(one) == N_COMPARED[1] - 2 and set(got) < set(one)
    assert not [n for n in got if not torch.equal(got[n], one[n])]
    assert len(names) < len(names1)
    print("backward launches, BA off: k = 3 %d, k = 1 %d" % (len(names), len(names1)))


def test_two_frozen_stages_leave_no_layer2_launch(dev):
    m, _ = _build("DAnA", 2, dev, use_BA_block=True)
    names, keys, saved = _backward_launches(m, dev, _episode("DAnA", 23))
    assert saved["q_saved"] == saved["s_saved"] == 6
    assert not [k_ for k_ in keys if k_.startswith("RCNN_base.5")]
    assert sorted(set(k_ for k_ in keys if k_.startswith("RCNN_base."))) == sorted(
        ["RCNN_base.6.%d.%s" % (b, c) for b in range(6) for c in ("conv1", "conv2", "conv3")] + ["RCNN_base.6.0.downsample.0"])
    assert any("roi_align_backward" in n for n in names)


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("shape", ["small", "reference"])
def test_trainer_step_matches_reference_loop_with_torch_sgd(dev, k, shape):
    """two iterations of train.py:125-143 through the autograd bridge + torch.optim.SGD against Trainer.step, by the criterion
    of test_gpu_backward.py's test of that name; frozen tensors stay bit-identical, and the freeze decides what moves.
    `reference`: that test's own inputs -- B 2, way 2, shot 2, 160x224, lr 0.01 -- and its criterion unchanged, the count of
    moved tensors included.
    `small`: this file's shape at lr 1e-3, the rate of the siblings' Trainer.step test. At lr 0.01 one step throws the tiny
    random-weight model out at this shape (rpn losses 1.20 / 0.76 -> 15.1 / 45.8, largest gradient 0.6 -> 7.8), and the
    second iteration amplifies the first one's round-off (the two loops' gradients agree to 8e-7 relative) until the
    parameters part by 17x the bound at the DEFAULT freeze k = 1 and 7.6x at k = 0 (profiles/fixed_blocks.md): a
    property of the shape, not of the freeze. The seven biases in front of a mean subtraction / softmax have gradients
    that are zero up to fp32 round-off; at this shape two of them move by it, so here they may move or stay."""
    from dana_amd import synthetic as S
    from dana_amd.config import cfg
    from dana_amd.trainer import Trainer
    (b_, way, shot, h_, w_), lr = ((B, WAY, SHOT, H, W), 1e-3) if shape == "small" else ((2, 2, 2, 160, 224), 0.01)
    ma, sd0 = _build("DAnA", k, dev, sd_seed=5, way=way, shot=shot, use_BA_block=True)
    mb, _ = _build("DAnA", k, dev, sd_seed=5, way=way, shot=shot, use_BA_block=True)
    ma.nms_inclusive = mb.nms_inclusive = shape == "small"  # (the reference test runs the default)
    inputs = [t.to(dev) for t in S.episode_inputs(b_, way, shot, h_, w_, seed=6)]
    groups = []
    for key, value in dict(ma.named_parameters()).items():
        if value.requires_grad:
            if "bias" in key:
                groups.append({"params": [value], "lr": lr * (cfg.TRAIN.DOUBLE_BIAS + 1),
                               "weight_decay": cfg.TRAIN.BIAS_DECAY and cfg.TRAIN.WEIGHT_DECAY or 0})
            else:
                groups.append({"params": [value], "lr": lr, "weight_decay": cfg.TRAIN.WEIGHT_DECAY})
    opt = torch.optim.SGD(groups, momentum=cfg.TRAIN.MOMENTUM)
    tr = Trainer(mb, lr)
    flat = set(tr.weights.names) | set(tr.biases.names)
    assert flat == {n for n, p in mb.named_parameters() if p.requires_grad} and len(flat) == N_COMPARED[k]
    losses_a, losses_b = [], []
    for it in range(2):
        np.random.seed(40 + it)
        ma.zero_grad()
        out = ma(*inputs)
        loss = out[3].mean() + out[4].mean() + out[5].mean() + out[6].mean()
        opt.zero_grad()
        loss.backward()
        assert all((p.grad is None) == (not p.requires_grad) for p in ma.parameters())
        opt.step()
        losses_a.append([float(x.detach()) for x in out[3:7]])
        np.random.seed(40 + it)
        outb = tr.step(*inputs)
        losses_b.append([float(x.detach()) for x in outb[3:7]])
    torch.cuda.synchronize()
    assert losses_a[0] == losses_b[0]
    assert losses_a[0] != losses_a[1], "the second forward must see the updated weights"
    for x, y in zip(losses_a[1], losses_b[1]):
        assert abs(x - y) <= 1e-5 * max(1.0, abs(x))
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    for n in pa:
        d = (pa[n].detach() - pb[n].detach()).abs().max().item()
        assert d <= 1e-6 + 1e-5 * pa[n].detach().abs().max().item(), (n, d)
    for mod in (ma, mb):
        for n, v in mod.state_dict().items():
            if n not in flat:
                assert torch.equal(v.cpu(), sd0[n]), "frozen tensor %s changed" % n
    moved = [n for n in pb if not torch.equal(pb[n].detach().cpu(), sd0[n])]
    if k == 0:
        assert any(n.startswith("RCNN_base.4.") and "conv" in n for n in moved)
    else:
        assert not [n for n in moved if n.startswith("RCNN_base.")]
        assert all(p.grad is None for n, p in pb.items() if n.startswith("RCNN_base."))
    assert set(moved) <= flat
    if shape == "reference":
        assert len(moved) == len(flat) - 7  # (the 7 biases in front of a mean subtraction / softmax have zero gradient)
    else:
        assert len(moved) >= len(flat) - 7


def test_program_trainer_over_a_frozen_trunk_equals_the_eager_trainer(dev):
    """FIXED_BLOCKS = 3: iterations replayed from launch programs == eager Trainer.step calls, by the criterion of
    test_gpu_program.py::test_program_training_iteration_equals_trainer_step"""
    from dana_amd import synthetic as S
    from dana_amd.program import ProgramTrainer
    from dana_amd.trainer import Trainer

    def params(m):
        return np.concatenate([p.detach().float().cpu().numpy().ravel() for _, p in sorted(m.named_parameters())])

    inputs = [t.to(dev) for t in S.episode_inputs(B, WAY, SHOT, H, W, seed=6)]
    (m0, _), (m1, _) = _build("DAnA", 3, dev, sd_seed=5, use_BA_block=True), _build("DAnA", 3, dev, sd_seed=5, use_BA_block=True)
    t0, t1 = Trainer(m0, 0.01), Trainer(m1, 0.01)
    for it in range(5):
        np.random.seed(40 + it)
        ref_out = t0.step(*inputs)
    torch.cuda.synchronize()
    ref, ref_losses = params(m0), [float(x) for x in ref_out[3:7]]
    for it in range(2):
        np.random.seed(40 + it)
        t1.step(*inputs)
    before = params(m1)
    pt = ProgramTrainer(t1, *inputs, warmup=0)
    torch.cuda.synchronize()
    assert np.array_equal(params(m1), before) and t1.steps == 2
    for it in range(2, 5):
        np.random.seed(40 + it)
        out = pt.step(*inputs)
    torch.cuda.synchronize()
    got = params(m1)
    d = np.abs(got - ref).max()
    assert d <= 1e-6 + 1e-4 * np.abs(ref).max(), d
    for a, b in zip([float(x) for x in out[3:7]], ref_losses):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b))
    assert t1.steps == 5 and not np.array_equal(got, before)


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("name", ["frcnn", "meta", "fgn", "fsod"])
def test_sibling_backward_vs_oracle_autograd_and_trainer_step(dev, mfma_mode, name, k):
    """the pattern of test_gpu_backward.py's test of this name under FIXED_BLOCKS = k: every trainable parameter's gradient
    against autograd through the oracle's forward of that model (5e-3), frozen ones keep grad None, then one Trainer.step"""
    from dana_amd import backward as BW
    from dana_amd.trainer import Trainer
    m, sd = _build(name, k, dev)
    seed, inputs, res = _forward_on_agreeing_seed(name, m, sd, dev)
    assert m._ctx["t"] == k and len(m._ctx["q_saved"]) == sum(len(m.RCNN_base[4 + li]) for li in range(k, 3))
    osd, out = _oracle_grads(name, k, seed, sd, inputs)
    for a, b in zip(res[3:7], out[3:7]):
        assert abs(float(a) - float(b.detach())) <= 1e-4 * max(1.0, abs(float(b.detach())))
    BW.model_backward(m, WEIGHTS)
    torch.cuda.synchronize()
    assert _compare(m, osd) == sum(1 for p in m.parameters() if p.requires_grad)
    for n, p in m.named_parameters():
        assert (p.grad is None) == (not p.requires_grad), n

    m.save_for_backward = False
    for p in m.parameters():
        p.grad = None
    tr = Trainer(m, lr=1e-3)
    before = {n: v.detach().clone() for n, v in m.named_parameters()}
    np.random.seed(33)
    o = tr.step(*[t.to(dev) for t in inputs])
    torch.cuda.synchronize()
    assert all(np.isfinite(float(x.detach())) for x in o[3:7])
    trainable = [n for n, v in m.named_parameters() if v.requires_grad]
    moved = [n for n, v in m.named_parameters() if not torch.equal(v.detach(), before[n])]
    assert set(moved) <= set(trainable)
    assert len(moved) >= len(trainable) - 2, "only %d of %d trainable tensors moved" % (len(moved), len(trainable))
    if k == 0:
        assert any(n.startswith("RCNN_base.4.") for n in moved)
    else:
        assert not [n for n in moved if n.startswith("RCNN_base.")]


def test_bottleneck_backward_of_layer1s_first_block_vs_autograd(dev, mfma_mode):
    """layer1's first block -- stride 1, 64 -> 64 1x1, 64 -> 64 3x3 direct (below winograd_min_cin), 64 -> 256 1x1 and a
    stride-1 downsample conv -- at 13x17: dL/dx and dL/dW against float64 autograd of the oracle's functional bottleneck,
    with test_gpu_backward.py's `_close` tolerances (1e-4 of the scale forward, 2e-4 backward); and without the input
    gradient, as the block runs at FIXED_BLOCKS = 0 (the stem in front of it is frozen)"""
    import torch.nn as nn
    from dana_amd import ops, backward as BW
    from dana_amd.dana import Bottleneck, DAnARCNN
    from oracle import model_ref as O

    def close(a, b, tol=2e-4):
        a, b = a.double(), b.double()
        scale = b.abs().max().item() + 1e-12
        err = (a - b).abs().max().item()
        assert err <= tol * scale, "max err %.3e vs scale %.3e" % (err, scale)

    stride, inplanes, planes, (Hh, Ww), N = 1, 64, 64, (13, 17), 2
    torch.manual_seed(164)
    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
    blk = Bottleneck(inplanes, planes, stride, ds)
    for mod in blk.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.1)
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    blk.eval()
    x = torch.randn(N, inplanes, Hh, Ww)
    sd = {"b." + n: v.detach().double().requires_grad_(v.dtype.is_floating_point and "conv" in n or "downsample.0" in n)
          for n, v in blk.state_dict().items()}
    xr = x.double().requires_grad_(True)
    y = O.bottleneck(xr, sd, "b", stride)
    gy = torch.randn(y.shape, dtype=torch.double)
    y.backward(gy)
    blk.to(dev)
    helper = DAnARCNN(["fg", "bg"], num_shot=1)
    bp = helper._block_plan(blk)
    assert bp["c2"]["u"] is None, "64 input channels are below winograd_min_cin: the direct 3x3"
    xd = ops.nchw_to_nhwc(x.to(dev)).view(-1, inplanes)
    names = [("conv1", bp["c1"], blk.conv1), ("conv2", bp["c2"], blk.conv2), ("conv3", bp["c3"], blk.conv3),
             ("downsample.0", bp["ds"], blk.downsample[0])]
    for need_dx in (True, False):
        saved = []
        o3, h1, w1 = helper._bottleneck(xd, N, Hh, Ww, bp, save=saved)
        assert len(saved) == 1
        close(ops.nhwc_to_nchw(o3, N, planes * 4, h1, w1).cpu(), y.detach(), 1e-4)
        g = ops.nchw_to_nhwc(gy.float().to(dev)).view(-1, planes * 4).contiguous()
        grads = BW.WeightGrads()
        dx = BW.bottleneck_backward(g, saved[0], N, Hh, Ww, bp, grads, "b", need_dx=need_dx, mask_dx=False)
        if need_dx:
            close(ops.nhwc_to_nchw(dx, N, inplanes, Hh, Ww).cpu(), xr.grad)
        else:
            assert dx is None
        for nm, c, mod in names:
            mod.weight.grad = None
            grads.finish_conv("b." + nm, c, mod.weight)
            close(mod.weight.grad.cpu(), sd["b.%s.weight" % nm].grad)
        assert not grads.packed


def test_a_freeze_that_is_no_prefix_is_refused_at_the_forward_and_by_the_trainer(dev):
    from dana_amd.trainer import Trainer
    m, _ = _build("DAnA", 1, dev, use_BA_block=True)
    for p in m.RCNN_base[6].parameters():
        p.requires_grad = False
    with pytest.raises(ValueError, match=r"RCNN_base\.6\.0\.conv1\.weight"):
        m(*[t.to(dev) for t in _episode("DAnA", 23)])
    with pytest.raises(ValueError, match=r"RCNN_base\.6\.0\.conv1\.weight"):
        Trainer(m, 0.01)
