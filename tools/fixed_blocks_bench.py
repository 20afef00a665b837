"""The replayed training iteration of `bench.py --mode step` (BASELINE configs[2]: res50, BA on, way 2, shot 3, bs 4,
600x1000, weights seed 11, inputs seed 1996) under cfg.RESNET.FIXED_BLOCKS = k: which trunk stages train.

    python tools/fixed_blocks_bench.py --fixed-blocks 3 [--launch program|eager] [--steps 100]

One k per process (the key is read when the model is built, and the role streams take their hardware queues once per
process). Prints one JSON line: ms per iteration timed as bench.py's trial() (3 warm steps, then the median GPU-side
interval between consecutive iteration ends; two rounds, the better one counts), the host enqueue time per iteration
(blocked time in the forward's one D2H read excluded), how many tensors train and how many launches the two programs
hold. The script uses nothing this feature added, so it runs on older checkouts too: there k = 2 and 3 train the right
parameters at the full price of k = 1 and k = 0 is refused by the Trainer. profiles/fixed_blocks.md was made with it."""
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
    ap.add_argument("--fixed-blocks", type=int, default=1, choices=[0, 1, 2, 3])
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
    cfg_from_list(["RESNET.FIXED_BLOCKS", str(args.fixed_blocks)])  # (as the reference's --set; BEFORE the model is built)
    model = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=2, shot=3, classes=["fg", "bg"])
    model.load_state_dict(S.fill_state_dict(model.state_dict(), seed=11, profile="test"))
    model.to(dev).train()
    inputs = [t.to(dev) for t in S.episode_inputs(args.batch, 2, 3, args.height, args.width, seed=1996)]
    trainer = Trainer(model, lr=1e-5)
    np.random.seed(1996)
    trainer.step(*inputs)
    launches = None
    if args.launch == "program":
        from dana_amd.program import ProgramTrainer
        runner = ProgramTrainer(trainer, *inputs)
        step = lambda: runner.step(*runner.inputs)  # noqa: E731
        launches = [p.stats["launches"] for p in (runner.p1, runner.p2) if p is not None]
    else:
        step = lambda: trainer.step(*inputs)  # noqa: E731
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
    print(json.dumps({"label": args.label, "fixed_blocks": cfg.RESNET.FIXED_BLOCKS, "launch": args.launch, "steps": args.steps,
                      "shape": "%dx%d, B %d, way 2, shot 3" % (args.height, args.width, args.batch),
                      "trainable_tensors": sum(p.requires_grad for p in model.parameters()),
                      "ms_per_step": round(min(rounds), 3), "ms_per_step_rounds": [round(r, 3) for r in rounds],
                      "host_enqueue_ms_per_step": round(host, 3), "program_launches": launches}))


if __name__ == "__main__":
    main()
