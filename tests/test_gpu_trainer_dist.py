"""The data-parallel training iteration end to end with a REAL world size of 2: two processes share the one GPU of the
test box and exchange gradients over gloo (RCCL refuses two ranks on one device; on the 8-GPU node the same code runs
over RCCL/xGMI). Checks the bucketed asynchronous all-reduce inside the HIP backward, the 1/world scaling in the fused
SGD launch and the initial parameter broadcast."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, same_inputs, q, name="DAnA", replay=False):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    import dana_amd
    from dana_amd import synthetic as S
    from dana_amd.trainer import Trainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        if world > 1:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        dev = torch.device("cuda:0")
        m = dana_amd.get_model(name, pretrained=False, use_BA_block=False, way=2, shot=2, classes=["fg", "bg"])
        # rank 1 starts from DIFFERENT weights: the trainer's broadcast must overwrite them with rank 0's
        m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=5 + rank, profile="test"))
        m.to(dev).train()
        tr = Trainer(m, 0.01, bucket_bytes=8 << 20)
        seed = 6 if same_inputs else 6 + rank
        inputs = [t.to(dev) for t in S.episode_inputs(1, 2, 2, 160, 224, seed=seed)]
        if name == "frcnn":
            inputs = inputs[:4]  # faster_rcnn.py:35: no supports
        step = tr.step
        if replay:
            # the same two iterations replayed from launch programs (program.ProgramTrainer): every bucket's all-reduce is a
            # host callback inside the second program -- a REAL exchange between the two processes at every replay
            from dana_amd.program import ProgramTrainer
            pt = ProgramTrainer(tr, *inputs, warmup=0)
            assert pt.p2.stats["host_callbacks"] == 1 + sum(len(fb.buckets) for fb, _, _ in tr.groups)
            step = pt.step
        for it in range(2):
            np.random.seed(40 + it)
            step(*inputs)
        torch.cuda.synchronize()
        vec = torch.cat([p.detach().reshape(-1)[::97] for p in m.parameters() if p.requires_grad]).cpu()
        nb = sum(len(fb.buckets) for fb, _, _ in tr.groups)
        q.put((rank, "ok", vec.numpy(), nb))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "error: %r\n%s" % (e, traceback.format_exc()), None, 0))
    finally:
        if world > 1:
            dist.destroy_process_group()


def _run(world, same_inputs, name="DAnA", replay=False):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, same_inputs, q, name, replay)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
    for r in res:
        assert r[1] == "ok", r[1]
    return res


def test_two_rank_training_iteration_over_gloo_on_one_gpu(dev):
    single = _run(1, True)[0]
    same = _run(2, True)
    assert same[0][3] >= 3  # several buckets: the exchange really was bucketed
    # identical shards on both ranks: the averaged gradient IS the single-rank gradient (and rank 1's different
    # initial weights were replaced by rank 0's)
    for r in same:  # (up to the order of the RoIAlign-backward atomics; a missing 1/world would be >= 1e-2)
        d = np.abs(r[2] - single[2]).max()
        assert d <= 1e-6 + 1e-4 * np.abs(single[2]).max(), d
    diff = _run(2, False)
    assert np.array_equal(diff[0][2], diff[1][2])  # different shards: replicas stay bit-identical
    assert np.abs(diff[0][2] - single[2]).max() > 0  # and the other shard's gradient did arrive


def test_two_rank_training_iteration_replayed_from_launch_programs(dev):
    """world size 2 over gloo on one GPU, the iteration replayed from launch programs: the bucket all-reduces are re-issued
    by the programs' host callbacks, the replicas stay bit-identical and equal the eager single-rank trajectory"""
    single = _run(1, True)[0]
    same = _run(2, True, replay=True)
    assert np.array_equal(same[0][2], same[1][2])
    for r in same:
        d = np.abs(r[2] - single[2]).max()
        assert d <= 1e-6 + 1e-4 * np.abs(single[2]).max(), d
    diff = _run(2, False, replay=True)
    assert np.array_equal(diff[0][2], diff[1][2]) and np.abs(diff[0][2] - single[2]).max() > 0


def test_two_rank_training_iteration_of_the_frcnn_sibling(dev):
    """the same exchange for the plain Faster R-CNN sibling (FasterRCNN._backward marks its own gradient stages)"""
    single = _run(1, True, "frcnn")[0]
    same = _run(2, True, "frcnn")
    assert np.array_equal(same[0][2], same[1][2])  # the replicas stay bit-identical
    for r in same:
        # identical shards: the averaged gradient is the single-rank gradient up to the order of the RoIAlign-backward
        # atomics (run-to-run ~1e-5 after two steps at lr 0.01; a missing 1/world or a lost bucket would be >= 1e-2)
        d = np.abs(r[2] - single[2]).max()
        assert d <= 5e-4 * np.abs(single[2]).max(), d
    assert same[0][3] >= 2


# ---- RCCL (backend "nccl" on ROCm): the path the 8-GPU runs take -------------------------------------------------
def _rccl_worker(rank, world, port, q, always_reduce, replay=False):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    import dana_amd
    from dana_amd import synthetic as S
    from dana_amd.trainer import Trainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    inited = False
    try:
        torch.cuda.set_device(rank)
        dev = torch.device("cuda", rank)
        if world > 1 or always_reduce:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            inited = True
        m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=2, shot=2, classes=["fg", "bg"])
        m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=5 + rank, profile="test"))
        m.to(dev).train()
        tr = Trainer(m, 0.01, bucket_bytes=8 << 20, always_reduce=always_reduce)
        inputs = [t.to(dev) for t in S.episode_inputs(1, 2, 2, 160, 224, seed=6 + rank)]
        step = tr.step
        if replay:
            # the same two iterations replayed from launch programs (program.ProgramTrainer): every bucket's all-reduce is a
            # host callback inside the second program -- a REAL exchange between the two processes at every replay
            from dana_amd.program import ProgramTrainer
            pt = ProgramTrainer(tr, *inputs, warmup=0)
            assert pt.p2.stats["host_callbacks"] == 1 + sum(len(fb.buckets) for fb, _, _ in tr.groups)
            step = pt.step
        for it in range(2):
            np.random.seed(40 + it)
            step(*inputs)
        torch.cuda.synchronize()
        vec = torch.cat([p.detach().reshape(-1)[::97] for p in m.parameters() if p.requires_grad]).cpu()
        seen = dist.get_world_size() if inited else 0
        backend = dist.get_backend() if inited else "none"
        q.put((rank, "ok", vec.numpy(), sum(len(fb.launch_order) for fb, _, _ in tr.groups), seen, backend))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "error: %r\n%s" % (e, traceback.format_exc()), None, 0, 0, ""))
    finally:
        if inited:
            dist.destroy_process_group()


def _run_rccl(world, always_reduce, replay=False):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rccl_worker, args=(r, world, port, q, always_reduce, replay)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=900) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
    for r in res:
        assert r[1] == "ok", r[1]
    return res


def test_training_iteration_over_rccl_single_rank_group(dev):
    """init_process_group("nccl") + the bucketed asynchronous all_reduce issued from the trainer's exchange stream while
    the HIP backward still runs on the model's side streams, on the ONE GPU every test box has: a 1-rank RCCL group
    (always_reduce=True keeps the collectives although world == 1). The sum over one rank is the identity, so the result
    must equal the no-process-group run up to the order of the RoIAlign-backward atomics."""
    plain = _run_rccl(1, False)[0]
    rccl = _run_rccl(1, True)[0]
    assert rccl[5] == "nccl" and rccl[4] == 1
    assert rccl[3] >= 3  # several buckets left through RCCL
    d = np.abs(rccl[2] - plain[2]).max()
    assert d <= 1e-6 + 1e-4 * np.abs(plain[2]).max(), d
    # ... and with the iteration replayed from launch programs: the RCCL all-reduces are re-issued by the host callbacks
    prog = _run_rccl(1, True, replay=True)[0]
    d = np.abs(prog[2] - plain[2]).max()
    assert d <= 1e-6 + 1e-4 * np.abs(plain[2]).max(), d


def test_two_rank_training_iteration_over_rccl():
    """two ranks, one GPU each, RCCL over xGMI (train.py:104-105,138-139 as one process per GPU): different shards leave
    the replicas bit-identical and differ from the single-rank result; rank 1's initial weights are replaced by rank 0's"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs: RCCL refuses two ranks on one device (the 1-rank RCCL test above and the 2-rank "
                    "gloo tests cover this box)")
    single = _run_rccl(1, False)[0]
    two = _run_rccl(2, False)
    assert two[0][4] == 2 and two[0][5] == "nccl"
    assert np.array_equal(two[0][2], two[1][2])
    assert np.abs(two[0][2] - single[2]).max() > 0
    rep = _run_rccl(2, False, replay=True)  # the same two iterations replayed from launch programs
    assert np.array_equal(rep[0][2], rep[1][2])
    d = np.abs(rep[0][2] - two[0][2]).max()
    assert d <= 1e-6 + 1e-4 * np.abs(two[0][2]).max(), d
