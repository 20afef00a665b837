"""CPU suite, part 2: the C-ABI library loads and exports every symbol include/dana_hip.h declares
(no compute without a GPU), argument errors surface as DanaError with a message, and the host-side
logic of the product package (module API, state_dict contract, config, target assignment, synthetic
generator) behaves like the reference / the oracle."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import dana_amd
from dana_amd import _lib, ops, synthetic as S, targets as T
from dana_amd.config import cfg, cfg_from_list
from oracle import model_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    protos = _lib.parse_header()
    assert len(protos) >= 35
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), "libdana_hip.so does not export %s" % name
    # and nothing torch-typed leaks into the boundary: only C scalars and raw pointers
    allowed = {"int", "long", "float", "double", "size_t", "dana_stream_t", "const float*", "float*", "const int*",
               "int*", "const unsigned char*", "unsigned long long", "void*", "const unsigned long long*",
               "unsigned long long*", "long long*", "const long long*", "void**", "const char*", "const void*"}
    for name, (ret, args) in protos.items():
        assert ret in ("int", "size_t", "const char*"), (name, ret)
        for ty, _ in args:
            assert ty in allowed, "%s: parameter type %r is not a plain C scalar / raw pointer" % (name, ty)
    assert _lib.lib().query("dana_abi_version") == 1
    # the debug / tuning switches live in their own header (include/dana_hip_debug.h), are exported too, and none of them
    # is declared by the drop-in ABI
    dbg = _lib.parse_header(_lib.DEBUG_HEADER)
    assert {"dana_set_epilogue_mode", "dana_set_sort_mode", "dana_set_igemm_trace", "dana_debug_force_tile",
            "dana_debug_stream_create_cumask", "dana_debug_set_dma_kernel", "dana_debug_get_dma_kernel",
            "dana_debug_set_pp_stages", "dana_debug_get_pp_stages", "dana_debug_last_igemm_form", "dana_debug_force_wgrad",
            "dana_debug_last_wgrad_form", "dana_debug_last_roi_align_backward_form"} <= set(dbg)
    assert not set(dbg) & set(protos)
    for name in dbg:
        assert hasattr(cdll, name), "libdana_hip.so does not export %s" % name


def test_argument_errors_are_reported_without_a_gpu():
    L = _lib.lib()
    with pytest.raises(_lib.DanaError, match="bad shape"):
        L.call("dana_roi_align_forward", None, None, None, 1, 0, 8, 8, 1, 1.0, 7, 7, 0, 0, 0, 0, None, None, 0, None)
    with pytest.raises(_lib.DanaError, match="multiples of 4"):
        L.call("dana_gemm_nt", 16, 16, 16, None, None, None, 8, 8, 6, 6, 6, 8, 0, 1, 0, 0, 0, 1.0, 0, None)
    with pytest.raises(_lib.DanaError, match="workspace"):
        L.call("dana_nms", 16, 100, 1, 0.7, 0, 0, 16, 100, 16, None, 0, None)
    # mask words + kept-row / folded-column words + state + the transposed diagonal / first three super-diagonal words
    assert L.query("dana_nms_workspace_bytes", 12000, 4) == 4 * 12000 * 188 * 8 + 4 * (2 * 188 * 8 + 16) + 4 * 4 * 12000 * 8
    # empty inputs are a no-op, like the reference (nms.h:17-18, ROIAlign_cuda.cu:278-281)
    L.call("dana_roi_align_forward", None, None, None, 1, 8, 8, 8, 0, 1.0, 7, 7, 0, 0, 0, 0, None, None, 0, None)


def test_launch_program_executor_reissues_recorded_calls_without_a_gpu():
    """include/dana_hip.h "launch programs" (csrc/program.hip): recorded C-ABI calls are re-issued by one C loop through
    libffi -- exercised here on entry points that need no GPU: a configuration call, the empty-input no-op of
    dana_roi_align_forward (19 arguments, a float in the middle, five null pointers) and its argument-error path"""
    import struct
    from dana_amd.program import LaunchProgram
    L = _lib.lib()
    h = ctypes.c_void_p()
    L.call("dana_program_create", ctypes.cast(ctypes.byref(h), ctypes.c_void_p))

    def add(name, *args):
        fn = L.fn[name]
        sig = "".join(LaunchProgram._SIG[t] for t in fn.argtypes)
        assert len(sig) == len(args)
        words = (ctypes.c_ulonglong * len(args))()
        for k, (c, a) in enumerate(zip(sig, args)):
            if c == "f":
                words[k] = struct.unpack("<I", struct.pack("<f", a))[0]
            elif c == "d":
                words[k] = struct.unpack("<Q", struct.pack("<d", a))[0]
            else:
                words[k] = (0 if a is None else int(a)) & 0xFFFFFFFFFFFFFFFF
        L.call("dana_program_add_call", h, ctypes.cast(fn, ctypes.c_void_p), sig.encode(), ctypes.cast(words, ctypes.c_void_p),
               len(args))

    prev = ops.get_mfma_mode()
    add("dana_set_mfma_mode", 0)
    add("dana_roi_align_forward", None, None, None, 1, 8, 8, 8, 0, 1.0, 7, 7, 0, 0, 0, 0, None, None, 0, None)  # R = 0: no-op
    add("dana_set_mfma_mode", 1)
    add("dana_roi_align_forward", None, None, None, 1, 0, 8, 8, 1, 1.0, 7, 7, 0, 0, 0, 0, None, None, 0, None)  # C = 0: refused
    add("dana_set_mfma_mode", 0)  # (never reached)
    assert L.query("dana_program_size", h) == 5
    ops.set_mfma_mode(1)
    assert L.query("dana_program_run", h, 0, 2) == 0 and ops.get_mfma_mode() == 0
    assert L.query("dana_program_run", h, 2, 5) == -1 and ops.get_mfma_mode() == 1  # stopped at the failing entry
    assert b"bad shape" in L.cdll.dana_last_error()
    with pytest.raises(_lib.DanaError, match="bad range"):
        L.call("dana_program_run", h, 3, 9)
    with pytest.raises(_lib.DanaError, match="signature character"):
        L.call("dana_program_add_call", h, ctypes.cast(L.fn["dana_set_mfma_mode"], ctypes.c_void_p), b"q",
               ctypes.cast((ctypes.c_ulonglong * 1)(0), ctypes.c_void_p), 1)
    L.call("dana_program_destroy", h)
    ops.set_mfma_mode(prev)


def test_launch_trace_formatter_masks_pointers_and_numbers_streams_and_events():
    """tools/launch_trace.py: the text form of a launch sequence that two commits are diffed by -- pointers as 0 / p (their
    values change from run to run), every other argument as it is, streams and events as ordinals by first appearance"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        from launch_trace import Trace
    finally:
        sys.path.pop(0)
    protos = _lib.parse_header()
    t = Trace(protos)
    st_a, st_b = type("St", (), dict(cuda_stream=0x7f00))(), type("St", (), dict(cuda_stream=0x9f00))()
    ev_a, ev_b = object(), object()
    t.add_call(None, "dana_maxpool3x3s2_ceil_nhwc", (0x1000, 0x2000, 2, 35, 50, 64, 0x9f00))
    t.event("rec", ev_a, st_b)
    t.event("wait", ev_a, st_a)
    t.add_call(None, "dana_conv2d_nhwc", (0x1000, 0x3000, 0x4000, 0x5000, ctypes.c_void_p(0x6000), None, 2, 9, 13, 128, 512, 1, 1,
                                          1, 0, 0, 2048, 0, 257, 0x7f00))
    t.add_call(None, "dana_roi_align_forward", (None, ctypes.c_void_p(None), 0x10, 1, 8, 8, 8, 0, 0.0625, 7, 7, 0, 0, 0, 0, None,
                                                None, 0, None))
    t.event("rec", ev_b, st_a)
    assert t.lines == [
        "dana_maxpool3x3s2_ceil_nhwc p p 2 35 50 64 s0",
        "rec e0 s0",
        "wait e0 s1",
        "dana_conv2d_nhwc p p p p p 0 2 9 13 128 512 1 1 1 0 0 2048 0 257 s1",
        "dana_roi_align_forward 0 0 p 1 8 8 8 0 0.0625 7 7 0 0 0 0 0 0 0 s2",  # (the null stream is a stream of its own)
        "rec e1 s1",
    ]


def test_mfma_mode_switch_roundtrip_and_errors():
    """dana_set_mfma_mode / dana_get_mfma_mode (host-side state only: no GPU needed)"""
    L = _lib.lib()
    prev = ops.get_mfma_mode()
    assert prev in (0, 1)
    assert ops.set_mfma_mode(0) == prev and ops.get_mfma_mode() == 0
    assert ops.set_mfma_mode(1) == 0 and ops.get_mfma_mode() == 1
    with pytest.raises(_lib.DanaError, match="mode must be"):
        L.call("dana_set_mfma_mode", 7)
    with pytest.raises(_lib.DanaError, match="mode must be"):
        L.call("dana_set_mfma_mode", 2)  # forced tiles are a debug switch now (dana_debug_force_tile)
    ops.force_tile(3)
    assert ops.get_mfma_mode() == 1
    ops.force_tile(0)
    # a CU mask that leaves an XCD without CUs is refused before any HIP call (bit i = CU i // 8 of XCD i % 8)
    mask, out = (ctypes.c_uint * 8)(*([0x0f0f0f0f] * 8)), ctypes.c_void_p()
    with pytest.raises(_lib.DanaError, match="every XCD needs"):
        L.call("dana_debug_stream_create_cumask", ctypes.cast(mask, ctypes.c_void_p), 8, 8,
               ctypes.cast(ctypes.byref(out), ctypes.c_void_p))
    assert ops.get_mfma_mode() == 1
    ops.set_mfma_mode(prev)


def _selectors_in_a_child(**env):
    """(dma kernel, pp stages, stderr) as a fresh process started with `env` reports them"""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from dana_amd import ops; "
            "print(ops.get_dma_kernel(), ops.get_pp_stages())" % ROOT)
    clean = {k: v for k, v in os.environ.items() if k not in ("DANA_DMA_KERNEL", "DANA_PP_STAGES")}
    pr = subprocess.run([sys.executable, "-c", code], env=dict(clean, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                        timeout=120)
    assert pr.returncode == 0, pr.stderr.decode()
    dm, pp = pr.stdout.split()
    return int(dm), int(pp), pr.stderr.decode()


def test_contraction_form_selectors_roundtrip_errors_and_environment():
    """dana_debug_set_dma_kernel / dana_debug_set_pp_stages (host-side state only): the setters change what the getters
    report, refuse values the environment variables would not accept either, -1 returns to the value the process started
    with; DANA_DMA_KERNEL / DANA_PP_STAGES give a fresh process its initial values, an unknown one is reported and ignored"""
    L = _lib.lib()
    dm0, pp0 = ops.get_dma_kernel(), ops.get_pp_stages()
    try:
        for v in (0, 1, 2):
            prev = ops.get_dma_kernel()
            assert ops.set_dma_kernel(v) == prev and ops.get_dma_kernel() == v
        for v in (2, 3, 4, 6, 13, 14):
            prev = ops.get_pp_stages()
            assert ops.set_pp_stages(v) == prev and ops.get_pp_stages() == v
        for bad in (3, -2, 13):
            with pytest.raises(_lib.DanaError, match="dana_debug_set_dma_kernel"):
                L.call("dana_debug_set_dma_kernel", bad)
        for bad in (5, 0, 1, -2, 7, 15):
            with pytest.raises(_lib.DanaError, match="dana_debug_set_pp_stages"):
                L.call("dana_debug_set_pp_stages", bad)
        assert (ops.get_dma_kernel(), ops.get_pp_stages()) == (2, 14)  # a refused value changes nothing
        ops.set_dma_kernel(-1)
        ops.set_pp_stages(-1)
        assert (ops.get_dma_kernel(), ops.get_pp_stages()) == (dm0, pp0)
        with ops.igemm_forms(dma=0, pp=13, epilogue=1):
            assert (ops.get_dma_kernel(), ops.get_pp_stages(), L.query("dana_get_epilogue_mode")) == (0, 13, 1)
        assert (ops.get_dma_kernel(), ops.get_pp_stages(), L.query("dana_get_epilogue_mode")) == (dm0, pp0, 0)
    finally:
        ops.set_dma_kernel(-1)
        ops.set_pp_stages(-1)
    f = ops.decode_igemm_form(4 | 2 << 4 | 1 << 6 | 1 << 9 | 3 << 12 | 1 << 16 | 1 << 17)
    assert f == ops.IgemmForm("dma", 128, 64, 0, 1, 0, 0, 3, 1, 1)
    assert ops.decode_igemm_form(3 | 2 << 4 | 2 << 6 | 1 << 11).family == "split_128"
    assert _selectors_in_a_child()[:2] == (-1, -1)
    assert _selectors_in_a_child(DANA_DMA_KERNEL="2", DANA_PP_STAGES="13")[:2] == (2, 13)
    dm, pp, err = _selectors_in_a_child(DANA_PP_STAGES="5")
    assert (dm, pp) == (-1, -1) and "DANA_PP_STAGES=5 is not one of the accepted values; ignored" in err


def test_wgrad_selector_refusals_and_decoding():
    """dana_debug_force_wgrad (host-side state only): tile 0 / 64 / 128 and slices 0..64, anything else is an argument error
    that changes nothing (seen through the workspace size, which follows the forced slice count); the launch records decode"""
    L = _lib.lib()
    size = lambda: L.query("dana_conv2d_wgrad_workspace_bytes", 1, 19, 23, 64, 64, 3, 3, 1, 1)  # noqa: E731  (M = 437, K = 576)
    unit = 64 * 576 * 4
    try:
        ops.force_wgrad(0, 0)
        s0 = size()
        assert s0 % unit == 0 and 1 <= s0 // unit <= 2  # the cost model: at most ceil(M / 256) slices
        ops.force_wgrad(64, 5)
        assert size() == 5 * unit
        for tile, slices in ((32, 0), (1, 1), (256, 0), (-64, 0), (129, 2), (64, -1), (128, 65), (0, 1000)):
            with pytest.raises(_lib.DanaError, match="dana_debug_force_wgrad"):
                L.call("dana_debug_force_wgrad", tile, slices)
            assert size() == 5 * unit, (tile, slices)
        with ops.wgrad_forms(tile=128, slices=2):
            assert size() == 2 * unit
        assert size() == s0  # the context manager leaves (0, 0) behind
    finally:
        ops.force_wgrad(0, 0)
    assert ops.decode_wgrad_form(0) == ops.WgradForm(None, 0, 0)
    assert ops.decode_wgrad_form(4 | 5 << 4 | 36 << 12) == ops.WgradForm("split_128p", 5, 36)
    assert ops.decode_wgrad_form(1 | 64 << 4 | 65535 << 12) == ops.WgradForm("f32_64", 64, 65535)
    assert [ops.decode_wgrad_form(k).kernel for k in (2, 3)] == ["f32_128", "split_128"]
    assert ops.last_roi_align_backward_form() in (None, "gather", "bins", "scatter_nhwc", "scatter_nchw", "memset")


def test_wgrad_workspace_sizes_follow_a_forced_slice_count():
    """the override sits in wgrad_shape(), so dana_conv2d_wgrad_workspace_bytes / dana_gemm_tn_batched_workspace_bytes (and
    through the latter's internal twin the Winograd-domain weight gradient) size for the forced S, clamped to ceil(M / 32),
    to a last slice that is not empty and to planes * S <= 65535; a forced tile alone leaves the cost model's S"""
    L = _lib.lib()
    conv = lambda b, h, w: L.query("dana_conv2d_wgrad_workspace_bytes", b, h, w, 64, 64, 3, 3, 1, 1) // (64 * 576 * 4)  # noqa: E731
    tn = lambda planes, m: L.query("dana_gemm_tn_batched_workspace_bytes", planes, m, 8, 64) // (planes * 8 * 64 * 4)  # noqa: E731
    wino = lambda: L.query("dana_conv3x3_wgrad_winograd4_workspace_bytes", 2, 17, 20, 64, 8)  # noqa: E731  (50 tiles of 4x4)
    try:
        ops.force_wgrad(0, 0)
        assert conv(1, 19, 23) in (1, 2) and tn(3, 49) == 1
        w0 = wino()
        for tile in (64, 128):
            ops.force_wgrad(tile, 1)
            assert (conv(1, 19, 23), tn(3, 49), tn(3, 1)) == (1, 1, 1)
            w1 = wino()
            ops.force_wgrad(tile, 2)
            assert (conv(1, 19, 23), tn(3, 49), tn(3, 33), tn(3, 32), tn(3, 1)) == (2, 2, 2, 1, 1)
            assert wino() == w1 + 36 * 2 * 8 * 64 * 4  # S = 1 needs no partial tiles, S = 2 two per plane
            ops.force_wgrad(tile, 5)
            assert (conv(1, 19, 23), conv(1, 5, 7), conv(1, 1, 1), tn(3, 49), tn(30000, 437)) == (5, 2, 1, 2, 2)
            ops.force_wgrad(tile, 64)
            assert (conv(1, 19, 23), conv(1, 15, 20)) == (14, 10)  # ceil(437 / 32), ceil(300 / 32)
            # M = 300 in 9 slices: chunks of 64 pixels, of which only five are not empty (6, 7 and 8 slices likewise) -> 5
            ops.force_wgrad(tile, 9)
            assert conv(1, 15, 20) == 5
            ops.force_wgrad(tile, 0)
            assert (conv(1, 19, 23), tn(3, 49)) in ((1, 1), (2, 1)) and wino() in (w0, w1)
    finally:
        ops.force_wgrad(0, 0)


def test_wgrad_refuses_pixel_strides_below_the_channel_count():
    """dana_conv2d_wgrad_nhwc: in_pix_stride < cin or grad_pix_stride < cout is an argument error before the workspace is
    looked at and before any launch (dana_gemm_tn_batched checks ldy >= n / ldx >= k the same way)"""
    L = _lib.lib()
    for in_stride, grad_stride in ((60, 0), (0, 4), (60, 4)):
        with pytest.raises(_lib.DanaError, match="in_pix_stride < cin or grad_pix_stride < cout"):
            L.call("dana_conv2d_wgrad_nhwc", 16, 16, 16, 1, 5, 7, 64, 8, 1, 1, 1, 0, in_stride, grad_stride, None, 0, None, 0, None)
    with pytest.raises(_lib.DanaError, match="workspace"):  # strides at the channel counts pass the check
        L.call("dana_conv2d_wgrad_nhwc", 16, 16, 16, 1, 5, 7, 64, 8, 1, 1, 1, 0, 64, 8, None, 0, None, 0, None)
    with pytest.raises(_lib.DanaError, match="16-byte aligned"):
        L.call("dana_gemm_tn_batched", 16, 16, 16, 1, 5, 8, 64, 4, 64, 0, 0, 0, 8, 0, None, 0, None)


def test_ops_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.roi_align_forward(torch.zeros(1, 4, 8, 8), torch.zeros(1, 5), 1.0, 7, 7, 0)
    with pytest.raises(RuntimeError):
        dana_amd._C.nms(torch.zeros(3, 4), torch.zeros(3), 0.5)


def test_module_api_and_state_dict_contract():
    """346 entries (344 without the BA layer), 70 trainable tensors / 37 113 489 params."""
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=2, shot=3, classes=["fg", "bg"])
    sd = m.state_dict()
    assert len(sd) == 346
    assert sum(k.startswith("RCNN_base.") for k in sd) == 258 and sum(k.startswith("RCNN_top.") for k in sd) == 60
    for k in ("rpn_unary_layer.weight", "rcnn_adapt_q_layer.bias", "rpn_channel_k_layer.weight",
              "RCNN_rpn.RPN_Conv.weight", "RCNN_rpn.RPN_cls_score.bias", "rcnn_transform_layer.weight",
              "output_score_layer.linear1.weight", "RCNN_bbox_pred.bias", "RCNN_base.6.5.bn3.running_var",
              "RCNN_top.0.0.downsample.0.weight"):
        assert k in sd, k
    assert tuple(sd["RCNN_rpn.RPN_Conv.weight"].shape) == (512, 2048, 3, 3)
    assert tuple(sd["RCNN_rpn.RPN_cls_score.weight"].shape) == (24, 512, 1, 1)
    assert tuple(sd["output_score_layer.linear1.weight"].shape) == (1024, 3136)
    trainable = [p for p in m.parameters() if p.requires_grad]
    assert len(trainable) == 70 and sum(p.numel() for p in trainable) == 37113489
    assert sum(p.numel() for p in m.parameters()) == 37389009
    assert "bias" in "".join(n for n, _ in m.named_parameters())  # train.py:79-85 keys off 'bias' in name
    m.train()
    assert not m.RCNN_base[4].training and m.RCNN_base[5].training  # dana.py:370-385
    assert all(not mod.training for mod in m.RCNN_base.modules() if isinstance(mod, torch.nn.BatchNorm2d))
    assert len(dana_amd.get_model("DAnA", pretrained=False, use_BA_block=False).state_dict()) == 344
    with pytest.raises(Exception):
        dana_amd.get_model("cisa")  # undefined in the reference too (utils.py:117-118)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.eval()(*S.episode_inputs(1, 1, 3, 64, 64))


@pytest.mark.parametrize("name,count", [("DAnA", 70), ("frcnn", 52), ("meta", 52), ("fgn", 58), ("fsod", 64)])
def test_grad_stages_name_every_trainable_parameter_once(name, count):
    """backward.grad_stages finds each model's stage list through its class; together the stages are exactly the
    requires_grad parameters, each once (Trainer.__init__ only notices a MISSING name, not a duplicate). The stub plan
    holds what `_block_convs` reads: whether a block has a downsample conv."""
    from dana_amd import backward as BW
    m = dana_amd.get_model(name, pretrained=False, use_BA_block=True, way=2, shot=2, classes=["bg", "fg"])
    blocks = lambda layer: [{"ds": True if blk.downsample is not None else None} for blk in layer]  # noqa: E731
    plan = dict(layer4=blocks(m.RCNN_top[0]), layers=[None, blocks(m.RCNN_base[5]), blocks(m.RCNN_base[6])])
    names = [n for _, stage in BW.grad_stages(m, plan) for n in stage]
    assert len(names) == len(set(names)) == count
    assert sorted(names) == sorted(n for n, p in m.named_parameters() if p.requires_grad)


def test_config_overrides():
    assert cfg.ANCHOR_SCALES == [4, 8, 16, 32] and cfg.MAX_NUM_GT_BOXES == 50 and cfg.TRAIN.BATCH_SIZE == 128
    cfg_from_list(["TRAIN.RPN_POST_NMS_TOP_N", "1000"])
    assert cfg.TRAIN.RPN_POST_NMS_TOP_N == 1000
    cfg_from_list(["TRAIN.RPN_POST_NMS_TOP_N", "2000"])
    with pytest.raises(AssertionError):
        cfg_from_list(["NOT_A_KEY", "1"])


def test_synthetic_generator_is_portable_and_seeded():
    a, b = S.normal("x", (4, 5), 2.0, 1.0, seed=3), S.normal("x", (4, 5), 2.0, 1.0, seed=3)
    assert torch.equal(a, b) and not torch.equal(a, S.normal("y", (4, 5), 2.0, 1.0, seed=3))
    big = S.normal("z", (200000,), 1.0, 0.0, seed=1)
    assert abs(float(big.mean())) < 0.01 and abs(float(big.std()) - 1.0) < 0.01
    im, info, gt, nb, sup = S.episode_inputs(2, 2, 3, 64, 96)
    assert sup.shape == (2, 6, 3, 320, 320) and gt.shape == (2, 50, 5) and (gt[:, :3, 4] == 1).all()


def test_anchor_table_matches_the_oracle():
    assert np.array_equal(T.generate_anchors(scales=np.array([4, 8, 16, 32])), O.generate_anchors(scales=[4, 8, 16, 32]))


def test_torch_ops_registration_of_the_five_C_operators():
    """the reference's pybind `model._C` (vision.cpp:7-13) as PyTorch custom operators: csrc/torch_ops.cpp
    registers them with TORCH_LIBRARY over the C ABI; dana_amd._C binds to them when the shim library is built"""
    assert dana_amd._C.BINDING == "torch.ops.dana", dana_amd._C.BINDING
    for name in ("nms", "roi_align_forward", "roi_align_backward", "roi_pool_forward", "roi_pool_backward", "roi_align",
                 "roi_pool"):
        assert hasattr(torch.ops.dana, name)
    schema = str(torch.ops.dana.roi_align_forward.default._schema)
    assert "Tensor input, Tensor rois, float spatial_scale, int pooled_height, int pooled_width, int sampling_ratio" in schema
    # CPU tensors are refused with the reference's wording; empty input -> empty result without a launch (nms.h:17-18)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        torch.ops.dana.roi_align_forward(torch.zeros(1, 4, 8, 8), torch.zeros(1, 5), 1.0, 7, 7, 0)
    with pytest.raises(RuntimeError, match="Not compiled with CPU support"):
        dana_amd._C.roi_pool_forward(torch.zeros(1, 4, 8, 8), torch.zeros(1, 5), 1.0, 7, 7)
    assert dana_amd._C.nms(torch.zeros(0, 4), torch.zeros(0), 0.5).shape == (0,)


def test_C_module_installs_as_the_reference_model_C():
    """`sys.modules['model._C'] = dana_amd._C` is the whole binding a reference caller needs -- the
    roi_layers wrappers of lib/model/roi_layers/*.py import `from model import _C` and call these five names"""
    import sys
    import types
    stub = types.ModuleType("model")
    stub._C = dana_amd._C
    saved = {k: sys.modules.get(k) for k in ("model", "model._C")}
    sys.modules["model"], sys.modules["model._C"] = stub, dana_amd._C
    try:
        ns = {}
        exec("from model import _C\nnames = [_C.nms, _C.roi_align_forward, _C.roi_align_backward, _C.roi_pool_forward, "
             "_C.roi_pool_backward]", ns)
        assert all(callable(f) for f in ns["names"])
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_bench_rejects_a_launcher_whose_world_size_is_not_gpus():
    """bench.py's launch contract: under an external launcher WORLD_SIZE must equal --gpus; a mismatch
    exits non-zero before any device work (it would otherwise print a line whose n_gpus is not what was asked for)."""
    import subprocess
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0"],
                        env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert pr.returncode != 0 and b"WORLD_SIZE=2" in pr.stderr and not pr.stdout.strip()


def test_bench_dump_outputs_dtypes_and_byte_budget(tmp_path):
    """bench.py --dump-outputs: floating point as float32 (float64 kept), integers and numbers as float64, None skipped;
    arrays over the byte budget are replaced by a sample of their elements at fixed, sorted positions, the same on every
    call (two builds compare element for element)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("dana_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    named = {"rois": torch.ones(2, 5), "rois_label": torch.tensor([1, 0, 2]), "loss": torch.tensor(0.5, dtype=torch.float64),
             "half": torch.ones(3, dtype=torch.float16), "skipped": None, "zero": 0, "big": torch.arange(10000.0)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), named, limit=4096)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n, v in named.items() if v is not None)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert {n: a.dtype for n, a in got.items()} == {"rois": np.float32, "rois_label": np.float64, "loss": np.float64,
                                                    "half": np.float32, "zero": np.float64, "big": np.float32}
    assert np.array_equal(got["rois_label"], [1, 0, 2]) and np.array_equal(got["rois"], np.ones((2, 5)))
    assert sum(a.nbytes for a in got.values()) <= 4096
    assert 0 < got["big"].size < 10000 and np.all(np.diff(got["big"]) > 0)  # sorted positions of an arange
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))
