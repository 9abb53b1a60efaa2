#!/usr/bin/env python3
"""Co-evolution precision record: one generation of the SAME seeded
populations through MultiAgentGpuEngine in bf16 and in fp32 member rows, both
in rollout mode "episode" (es_tag_episode against es_tag_episode_f32), and
through the pair form (pair_rollout=True, es_tag_pair_episode, which evaluates
bf16(theta) +- bf16(sigma*eps)), again against fp32.

Prints, per policy, the Spearman rank correlation of the 2*pairs member
fitnesses and the cosine of the two reconstructed gradients (``st.grad``),
bf16 against fp32 and pair against fp32. The numbers are a record (profiles/README.md), not an
assertion: a catch is a threshold, so one-ulp weight differences can end a
game a step apart and the gap grows with the horizon.

  python tools/ma_precision.py --nets 32,32 256,256 --max-steps 200
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.ma_bench import make_engine  # noqa: E402
from tools.precision_ladder import spearman  # noqa: E402


def one_generation(dev, wdtype, ppg, layers, max_steps, seed, mode="episode"):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng = make_engine(dev, mode, ppg, layers, max_steps, seed, wdtype)
    eng.step([CenteredRanker(), CenteredRanker()])
    fits = eng.rew_total[:ppg].cpu().numpy().astype(np.float64)     # (2*pairs, agent)
    grads = [st.grad.cpu().numpy().astype(np.float64) for st in eng.states]
    steps = eng.member_steps[:ppg].cpu().numpy()
    return fits, grads, steps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ppg", type=int, default=1024)
    p.add_argument("--nets", nargs="+", default=["32,32", "256,256"],
                   help="hidden layer sizes, comma separated, one net per item")
    p.add_argument("--max-steps", type=int, default=200)
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--json", type=str, default=None, help="also write the rows here")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ma_precision needs a GPU: both modes run the fused tag kernel")
    dev = torch.device("cuda", 0)

    rows = []
    print(f"{'net':>9} {'ppg':>5} {'rows':>5} {'policy':>6} {'spearman':>9} {'grad cosine':>11} "
          f"{'games ending apart':>18}")
    for net in args.nets:
        layers = [int(x) for x in net.split(",")]
        f16, g16, s16 = one_generation(dev, "bf16", args.ppg, layers, args.max_steps,
                                       args.seed)
        f32, g32, s32 = one_generation(dev, "fp32", args.ppg, layers, args.max_steps,
                                       args.seed)
        fpr, gpr, spr = one_generation(dev, "bf16", args.ppg, layers, args.max_steps,
                                       args.seed, mode="pair")
        for name, (fl, gl, sl) in (("bf16", (f16, g16, s16)), ("pair", (fpr, gpr, spr))):
            apart = int((sl != s32).sum())
            for i in range(2):
                cos = float(np.dot(gl[i], g32[i]) /
                            np.sqrt(np.dot(gl[i], gl[i]) * np.dot(g32[i], g32[i])))
                row = {"net": layers, "ppg": args.ppg, "max_steps": args.max_steps,
                       "rows": name, "policy": i,
                       "spearman": spearman(fl[:, i], f32[:, i]),
                       "grad_cosine": cos, "games_ending_apart": apart}
                rows.append(row)
                print(f"{net:>9} {args.ppg:>5} {name:>5} {i:>6} {row['spearman']:>9.5f} "
                      f"{cos:>11.5f} {apart:>18}", flush=True)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
