"""cfg.RESNET.FIXED_BLOCKS 0..3 on the host: the gradient stages follow the trunk's freeze prefix for DAnA and its four
siblings, in the backward's finishing order, and a freeze that is not a prefix is refused by name. (The stub plan holds
what `_block_convs` reads, as in test_abi_and_host.py.)"""
import re

import pytest

import dana_amd
from dana_amd import backward as BW
from dana_amd.config import cfg

MODELS = ("DAnA", "frcnn", "meta", "fgn", "fsod")
# trainable tensors per model at FIXED_BLOCKS = 1 (test_abi_and_host.py) and the conv weights of layer1 / layer2 / layer3
AT_ONE = dict(DAnA=70, frcnn=52, meta=52, fgn=58, fsod=64)
STAGE_CONVS = (10, 13, 19)


def _model(name, k):
    prev = cfg.RESNET.FIXED_BLOCKS
    cfg.RESNET.FIXED_BLOCKS = k
    try:
        return dana_amd.get_model(name, pretrained=False, use_BA_block=True, way=2, shot=2, classes=["bg", "fg"])
    finally:
        cfg.RESNET.FIXED_BLOCKS = prev


def _stub_plan(m):
    blocks = lambda layer: [{"ds": True if blk.downsample is not None else None} for blk in layer]  # noqa: E731
    return dict(layer4=blocks(m.RCNN_top[0]), layers=[blocks(m.RCNN_base[i]) for i in (4, 5, 6)])


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_grad_stages_name_exactly_the_trainable_parameters(name, k):
    m = _model(name, k)
    assert BW.first_trainable_stage(m) == k
    names = [n for _, stage in BW.grad_stages(m, _stub_plan(m)) for n in stage]
    count = AT_ONE[name] + (STAGE_CONVS[0] if k == 0 else -sum(STAGE_CONVS[1:k]))
    assert len(names) == len(set(names)) == count
    assert sorted(names) == sorted(n for n, p in m.named_parameters() if p.requires_grad)


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_trunk_stages_finish_layer3_first_and_each_layer_from_its_last_block(name, k):
    m = _model(name, k)
    stages = BW.grad_stages(m, _stub_plan(m))
    trunk = [(s, names) for s, names in stages if s.startswith("RCNN_base.")]
    assert [s for s, _ in stages[len(stages) - len(trunk):]] == [s for s, _ in trunk], "the trunk's stages come last"
    want = ["RCNN_base.%d.%d" % (4 + li, bi) for li in range(2, k - 1, -1)
            for bi in reversed(range(len(m.RCNN_base[4 + li])))]
    assert [s for s, _ in trunk] == want
    for s, names in trunk:
        tail = [re.sub(r"^%s\." % re.escape(s), "", n) for n in names]
        assert tail[:3] == ["conv3.weight", "conv2.weight", "conv1.weight"] and tail[3:] in ([], ["downsample.0.weight"])


@pytest.mark.parametrize("name", MODELS)
def test_default_freeze_gives_the_list_a_plan_without_layer1_gives(name):
    """k = 1 is today's list: the stages in front of t are never looked at (the stub plan of test_abi_and_host.py has
    None for layer1), and passing t explicitly -- as the backward does from its context -- equals deriving it"""
    m = _model(name, 1)
    plan = _stub_plan(m)
    plan["layers"][0] = None
    got = BW.grad_stages(m, plan)
    assert got == BW.grad_stages(m, plan, 1)
    trunk = [s for s, _ in got if s.startswith("RCNN_base.")]
    assert trunk == ["RCNN_base.6.%d" % b for b in (5, 4, 3, 2, 1, 0)] + ["RCNN_base.5.%d" % b for b in (3, 2, 1, 0)]
    assert sum(len(n) for _, n in got) == AT_ONE[name]


def test_a_freeze_that_is_no_prefix_is_refused_by_parameter_name():
    m = _model("DAnA", 1)
    for p in m.RCNN_base[6].parameters():  # layer3 frozen by hand behind a trainable layer2
        p.requires_grad = False
    with pytest.raises(ValueError, match=r"RCNN_base\.6\.0\.conv1\.weight"):
        BW.first_trainable_stage(m)
    with pytest.raises(ValueError, match=r"RCNN_base\.6\.0\.conv1\.weight"):
        BW.grad_stages(m, _stub_plan(m))


def test_conv_weights_of_one_stage_must_agree():
    m = _model("frcnn", 1)
    m.RCNN_base[5][2].conv2.weight.requires_grad = False
    with pytest.raises(ValueError, match=r"RCNN_base\.5\.2\.conv2\.weight"):
        BW.first_trainable_stage(m)
