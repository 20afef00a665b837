"""The replayed training iteration of `bench.py --mode step` (res50, way 2, shot 3, bs 4, 600x1000, seed 11) with the
trainer's options bench.py does not expose: gradient-norm clipping on / off, SGD / Adam. Prints one JSON line: the median
GPU-side interval between iteration ends, the wall-clock mean and the host enqueue time per iteration (blocked time in the
forward's one D2H read excluded), as bench.py measures them. profiles/optimizer_ctl.md was made with

    python tools/optimizer_ctl_bench.py --launch program                      # clipping off
    python tools/optimizer_ctl_bench.py --launch program --clip-norm 10       # clipping on (the reference's threshold)
    rocprofv3 --kernel-trace --stats ... -- python tools/optimizer_ctl_bench.py --launch program --clip-norm 10 --steps 10

--clip-norm 0 passes no clip_norm at all, so the same script times a build that does not know the keyword."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch", default="program", choices=["program", "graph", "eager"])
    ap.add_argument("--clip-norm", type=float, default=0.0)
    ap.add_argument("--optimizer", default="sgd", choices=["sgd", "adam"])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1000)
    args = ap.parse_args()
    import dana_amd
    from dana_amd import ops, synthetic as S
    from dana_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    model = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=2, shot=3, classes=["fg", "bg"])
    model.load_state_dict(S.fill_state_dict(model.state_dict(), seed=11, profile="test"))
    model.to(dev).train()
    inputs = [t.to(dev) for t in S.episode_inputs(args.batch, 2, 3, args.height, args.width, seed=1996)]
    kw = {"clip_norm": args.clip_norm} if args.clip_norm > 0 else {}
    if args.optimizer != "sgd":
        kw["optimizer"] = args.optimizer
    trainer = Trainer(model, lr=1e-5, **kw)
    np.random.seed(1996)
    trainer.step(*inputs)
    if args.launch == "program":
        from dana_amd.program import ProgramTrainer
        runner = ProgramTrainer(trainer, *inputs)
        step = lambda: runner.step(*runner.inputs)  # noqa: E731
    elif args.launch == "graph":
        from dana_amd.graphs import GraphedTrainer
        runner = GraphedTrainer(trainer, *inputs)
        step = lambda: runner.step(*runner.inputs)  # noqa: E731
    else:
        step = lambda: trainer.step(*inputs)  # noqa: E731
    for _ in range(args.warmup):
        step()
    np.random.seed(1996)
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True)]
    marks[0].record()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.steps * 1e3
    iv = sorted(a.elapsed_time(b) for a, b in zip(marks, marks[1:]))
    k = min(20, args.steps)
    ops.HOST_WAIT[0] = 0.0
    t0 = time.perf_counter()
    for _ in range(k):
        step()
    host = (time.perf_counter() - t0 - ops.HOST_WAIT[0]) / k * 1e3
    torch.cuda.synchronize()
    out = {"launch": args.launch, "optimizer": args.optimizer, "clip_norm": args.clip_norm, "steps": args.steps,
           "ms_per_step": round(wall, 3), "ms_per_step_median": round(iv[len(iv) // 2], 3),
           "host_enqueue_ms_per_step": round(host, 3)}
    if hasattr(trainer, "grad_norm") and args.clip_norm > 0:
        out["grad_norm_last"] = float(trainer.grad_norm().item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
