"""Attention maps, the parts that need no device: argument validation of `attention_maps` / `render` / `upsample`, the
colour table, and the cell-rectangle rule (`attention.cell_rect`, the Python statement of what dana_attn_box_mean does in
its kernel) on hand-worked boxes."""
import pytest
import torch


def _model(use_ba=True):
    import dana_amd
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=use_ba, way=1, shot=2, classes=["fg", "bg"])
    return m.eval()


def _inputs(B=1):
    return torch.zeros(B, 3, 96, 128), torch.tensor([[96.0, 128.0, 1.0]] * B), torch.zeros(B, 2, 3, 320, 320)


def test_module_and_method_exist():
    import dana_amd
    from dana_amd import attention
    assert attention.AttentionMaps._fields == ("ba", "rpn", "roi")
    assert callable(dana_amd.DAnARCNN.attention_maps)
    assert attention.ATTENTION_LEVELS == ("ba", "rpn", "roi")


def test_train_mode_raises_runtime_error():
    m = _model().train()
    im, info, sup = _inputs()
    with pytest.raises(RuntimeError, match="eval"):
        m.attention_maps(im, info, torch.zeros(1, 1, 4), sup)


@pytest.mark.parametrize("boxes, what", [
    (torch.zeros(1, 4), "rank"),                              # [n][4]: no batch axis
    (torch.zeros(1, 3, 5), "rank"),                           # rois with the index column
    (torch.zeros(1, 3, 4, dtype=torch.float64), "float32"),
    (torch.zeros(1, 3, 4, dtype=torch.int32), "float32"),
    (torch.zeros(1, 0, 4), "n >= 1"),
    (torch.zeros(2, 3, 4), "images"),                         # B = 2 boxes for a B = 1 im_data
    (torch.zeros(1, 3, 4), "HIP"),                            # right shape, on the host
    ([[0.0, 0.0, 1.0, 1.0]], "rank"),                         # not a tensor
])
def test_boxes_are_validated_on_the_host(boxes, what):
    m = _model()
    im, info, sup = _inputs()
    with pytest.raises(ValueError):
        m.attention_maps(im, info, boxes, sup)


def test_levels_are_validated():
    from dana_amd import attention
    m = _model()
    im, info, sup = _inputs()
    for bad in (("rpn", "layer4"), (), "head"):
        with pytest.raises(ValueError, match="levels"):
            m.attention_maps(im, info, torch.zeros(1, 1, 4), sup, levels=bad)
    assert attention.check_levels("rpn") == ("rpn",)
    assert attention.check_levels(["roi", "rpn"]) == ("roi", "rpn")


def test_explicit_ba_without_the_ba_block_raises():
    # (the default levels give ba = None there; that needs a device -- tests/test_gpu_attention_maps.py)
    m = _model(use_ba=False)
    im, info, sup = _inputs()
    with pytest.raises(ValueError, match="'ba'"):
        m.attention_maps(im, info, torch.zeros(1, 1, 4), sup, levels=("ba", "rpn"))


def test_color_table_shape_and_endpoints():
    from dana_amd.attention import COLOR_TABLE
    assert len(COLOR_TABLE) == 256 and all(len(c) == 3 for c in COLOR_TABLE)
    assert all(isinstance(v, int) and 0 <= v <= 255 for c in COLOR_TABLE for v in c)
    assert COLOR_TABLE[0] == (0, 0, 255) and COLOR_TABLE[255] == (255, 0, 0)       # blue -> red
    assert COLOR_TABLE[64][1] == 255 and COLOR_TABLE[128][1] == 255 and COLOR_TABLE[191][1] == 255  # through green
    # red never falls and blue never rises along the table; neighbours differ by at most 4 in any channel
    for a, b in zip(COLOR_TABLE[:-1], COLOR_TABLE[1:]):
        assert b[0] >= a[0] and b[2] <= a[2]
        assert max(abs(x - y) for x, y in zip(a, b)) <= 4
    assert len(set(COLOR_TABLE)) == 256


@pytest.mark.parametrize("box, rect", [
    # 96 x 128 query: grid fh = 6, fw = 8, cells of 16 pixels. (x1, y1, x2, y2) -> (x_lo, y_lo, x_hi, y_hi)
    ((20.0, 36.0, 30.0, 44.0), (1, 2, 1, 2)),          # inside one cell: x 16..31 is cell 1, y 32..47 is cell 2
    ((0.0, 0.0, 127.0, 95.0), (0, 0, 7, 5)),           # the whole image
    ((100.0, 70.0, 400.0, 300.0), (6, 4, 7, 5)),       # past the right and bottom edges: clamped to the last cells
    ((90.0, 20.0, 40.0, 60.0), (5, 1, 5, 3)),          # x2 < x1: x_hi is clamped up to x_lo, one column
    ((15.99, 31.5, 16.0, 32.0), (0, 1, 1, 2)),         # the cell boundary: 16 belongs to cell 1, 15.99 to cell 0
    ((-40.0, -3.0, -20.0, 5.0), (0, 0, 0, 0)),         # left of the image: floor(-40 / 16) = -3 clamps to cell 0
    ((300.0, 200.0, 310.0, 210.0), (7, 5, 7, 5)),      # outside altogether: the corner cell
    ((0.0, 0.0, 0.0, 0.0), (0, 0, 0, 0)),
])
def test_cell_rect_on_hand_worked_boxes(box, rect):
    from dana_amd.attention import cell_rect
    got = cell_rect(box, 6, 8)
    assert got == rect
    x_lo, y_lo, x_hi, y_hi = got
    assert 0 <= x_lo <= x_hi <= 7 and 0 <= y_lo <= y_hi <= 5  # never empty, never outside


def test_cell_rect_other_stride_and_grid():
    from dana_amd.attention import cell_rect
    assert cell_rect((10.0, 10.0, 50.0, 20.0), 4, 4, stride=8) == (1, 1, 3, 2)
    assert cell_rect((0.0, 0.0, 1e9, 1e9), 38, 63) == (0, 0, 62, 37)  # the 600 x 1000 grid


def test_render_and_upsample_refuse_host_tensors_and_bad_shapes():
    from dana_amd import attention
    with pytest.raises(ValueError, match="HIP"):
        attention.upsample(torch.zeros(2, 20, 20), 320)
    with pytest.raises(ValueError):
        attention.upsample(torch.zeros(20), 320)
    with pytest.raises(ValueError):
        attention.upsample(torch.zeros(2, 20, 20, dtype=torch.float64), 320)
    with pytest.raises(ValueError, match="HIP"):
        attention.render(torch.zeros(2, 20, 20), torch.zeros(2, 3, 320, 320))


def test_config_carries_the_pixel_means():
    from dana_amd import cfg
    assert [round(v, 4) for v in torch.as_tensor(cfg.PIXEL_MEANS).reshape(-1).tolist()] == [102.9801, 115.9465, 122.7717]
