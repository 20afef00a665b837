"""The replayed fine-tuning iteration over a frozen trunk (cfg.RESNET.FIXED_BLOCKS = 3) at the BASELINE configs[2] shape
(res50, BA on, way 2, shot 3, bs 4, 600x1000, weights seed 11, inputs seed 1996), from support images or from a support bank.

    python tools/support_bank_bench.py --supports images|bank [--queries images|bank] [--pool 64] [--steps 100]

One run per process (the role streams take their hardware queues once per process). Prints one JSON line: ms per iteration
timed as bench.py's trial() (3 warm steps, then the median GPU-side interval between consecutive iteration ends; two rounds,
the better one counts), the host enqueue time per iteration (blocked time in the forward's one D2H read excluded) and how
many launches the two programs hold.
`--supports images`: tools/fixed_blocks_bench.py at k = 3; it uses nothing this feature added, so it runs on older checkouts.
`--supports bank`: a pool of `--pool` images (seed 1997) is encoded once (time and bytes reported); every timed iteration
draws its B x way*shot bank rows with np.random (a cycle of 16 draws made in advance, so the training forward's own
np.random stream is not moved), `ep.set(draw)`, then the replayed step: the loop of INTEGRATION.md.
`--queries bank`: a pool of `--qpool` query images (seed 1998) is encoded once as a QueryBank (time and bytes reported, the
gather alone timed into a corr-shaped buffer); every timed iteration draws its B bank rows from a cycle of 16 draws,
`batch.set(draw)`, then the step. `--queries images` (the default) is the behaviour before the query bank.
profiles/support_bank.md and profiles/query_bank.md were made with it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cached_inference import trial  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--supports", default="images", choices=["images", "bank"])
    ap.add_argument("--queries", default="images", choices=["images", "bank"])
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("--qpool", type=int, default=64)
    ap.add_argument("--launch", default="program", choices=["program", "eager"])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import dana_amd
    from dana_amd import ops, synthetic as S
    from dana_amd.config import cfg, cfg_from_list
    from dana_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    way, shot = 2, 3
    cfg_from_list(["RESNET.FIXED_BLOCKS", "3"])  # (as the reference's --set; BEFORE the model is built)
    model = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=way, shot=shot, classes=["fg", "bg"])
    model.load_state_dict(S.fill_state_dict(model.state_dict(), seed=11, profile="test"))
    model.to(dev).train()
    inputs = [t.to(dev) for t in S.episode_inputs(args.batch, way, shot, args.height, args.width, seed=1996)]
    bank_info, ep, draws = None, None, None
    if args.supports == "bank":
        pool = S.normal("support_pool", (args.pool, 3, 320, 320), 64.0, 0.0, 1997).to(dev)
        model.encode_support_bank(pool[:16])  # (warm: the weight plan, the allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bank = model.encode_support_bank(pool)
        torch.cuda.synchronize()
        bank_info = {"pool": len(bank), "encode_ms": round((time.perf_counter() - t0) * 1e3, 2), "nbytes": bank.nbytes()}
        rng = np.random.RandomState(1996)
        draws = [rng.randint(0, len(bank), size=(args.batch, way * shot)) for _ in range(16)]
        ep = bank.episode(draws[0])
        # the gather alone, back to back on one stream (fresh destinations from the allocator's pool each time)
        idx = bank._index[draws[0].shape]
        gather = lambda: ops.bank_gather_episode(bank.map_pe, bank.pool_pe, idx, args.batch, way, shot)  # noqa: E731
        for _ in range(10):
            gather()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            gather()
        e1.record()
        torch.cuda.synchronize()
        moved = (args.batch * shot * bank.map_pe[0].numel() + args.batch * way * shot * bank.pool_pe[0].numel()) * 4
        bank_info.update(gather_us=round(e0.elapsed_time(e1) * 1e3 / 200, 2), gather_bytes_copied=moved)
        inputs = inputs[:4] + [ep]
        del pool
    qbank_info, qb, qdraws = None, None, None
    if args.queries == "bank":
        qpool = S.normal("query_pool", (args.qpool, 3, args.height, args.width), 64.0, 0.0, 1998).to(dev)
        model.encode_query_bank(qpool[:4])  # (warm: the weight plan, the allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        qbank = model.encode_query_bank(qpool)
        torch.cuda.synchronize()
        qbank_info = {"pool": len(qbank), "encode_ms": round((time.perf_counter() - t0) * 1e3, 2), "nbytes": qbank.nbytes()}
        del qpool
        rng = np.random.RandomState(1998)
        qdraws = [rng.randint(0, len(qbank), size=(args.batch,)) for _ in range(16)]
        qb = qbank.batch(qdraws[0])
        # the gather alone, back to back on one stream, into one corr-shaped buffer
        corr = torch.empty((args.batch * qbank.maps.size(1), 2048), dtype=torch.float32, device=dev)
        qgather = lambda: ops.qbank_gather(qbank.maps, qbank._index[args.batch], args.batch, out=corr, ld_out=2048)  # noqa: E731
        for _ in range(10):
            qgather()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            qgather()
        e1.record()
        torch.cuda.synchronize()
        qbank_info.update(gather_us=round(e0.elapsed_time(e1) * 1e3 / 200, 2),
                          gather_bytes_copied=args.batch * qbank.maps[0].numel() * 4)
        del corr
        inputs = [qb] + inputs[1:]
    trainer = Trainer(model, lr=1e-5)
    np.random.seed(1996)
    trainer.step(*inputs)
    launches = None
    if args.launch == "program":
        from dana_amd.program import ProgramTrainer
        runner = ProgramTrainer(trainer, *inputs)
        run = lambda: runner.step(*runner.inputs)  # noqa: E731
        launches = [p.stats["launches"] for p in (runner.p1, runner.p2) if p is not None]
    else:
        run = lambda: trainer.step(*inputs)  # noqa: E731
    count = [0]

    def step():
        if ep is not None:
            ep.set(draws[count[0] % len(draws)])
        if qb is not None:
            qb.set(qdraws[count[0] % len(qdraws)])
        if ep is not None or qb is not None:
            count[0] += 1
        return run()

    np.random.seed(1996)
    rounds = [trial(step, args.steps) for _ in range(2)]
    k = min(20, args.steps)
    torch.cuda.synchronize()
    ops.HOST_WAIT[0] = 0.0
    t0 = time.perf_counter()
    for _ in range(k):
        step()
    host = (time.perf_counter() - t0 - ops.HOST_WAIT[0]) / k * 1e3
    torch.cuda.synchronize()
    print(json.dumps({"label": args.label, "supports": args.supports, "queries": args.queries, "fixed_blocks": cfg.RESNET.FIXED_BLOCKS,
                      "launch": args.launch, "steps": args.steps,
                      "shape": "%dx%d, B %d, way %d, shot %d" % (args.height, args.width, args.batch, way, shot),
                      "trainable_tensors": sum(p.requires_grad for p in model.parameters()),
                      "ms_per_step": round(min(rounds), 3), "ms_per_step_rounds": [round(r, 3) for r in rounds],
                      "host_enqueue_ms_per_step": round(host, 3), "program_launches": launches, "bank": bank_info, "query_bank": qbank_info}))


if __name__ == "__main__":
    main()
