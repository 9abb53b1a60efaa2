#!/usr/bin/env python3
"""Co-evolution rollout bench: MultiAgentGpuEngine.step per generation in
rollout mode "step" (per-step launches) against "episode" (one fused
es_tag_episode launch), on one box.

For every grid point two engines are built from the same seeds, one per mode,
and their generations ALTERNATE (step, episode, step, ...) after a warm-up,
so both see the same machine state. Each generation ends in a device
synchronise inside engine.step; rollout_s and gen_s are the engine's own
timings. --weights-dtype bf16 fp32 adds the member-row dtype as another
alternating axis (one engine per mode and dtype). Games that end stop early
in episode mode, so the mean episode
length is printed with every row: it is part of the answer.

Mode "pair" is episode mode with pair_rollout=True (es_tag_pair_episode: one
workgroup plays both games of an antithetic pair on shared theta and
sigma*eps rows; bf16 only). It alternates with the others and gets a verdict
of its own against "episode": a pair block lasts as long as the longer of its
two episodes and the grid has half as many blocks, so small points may lose.

The project's bar for a speed claim: the SLOWEST run of the new mode must
lead the FASTEST run of the old one by at least three times the run-to-run
spread (max - min within a mode, the larger of the two).

  python tools/ma_bench.py                      # the whole grid, both modes
  python tools/ma_bench.py --modes step         # baseline only
  python tools/ma_bench.py --modes episode pair # pair sharing against per-game rows
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def make_engine(dev, mode, ppg, layers, max_steps, seed, wdtype="bf16"):
    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.ma_engine import MultiAgentGpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs.multiagent import BatchedPursuitTag
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import Comm

    torch.manual_seed(seed)
    comm = Comm(dev)
    cfg = AttrDict({"env": {"name": "PursuitTag", "max_steps": max_steps},
                    "noise": {"tbl_size": 2_000_000, "std": 0.05},
                    "policy": {"layer_sizes": layers, "ac_std": 0.01, "l2coeff": 0.005,
                               "lr": 0.02, "ob_clip": 5, "save_obs_chance": 0.1},
                    "general": {"policies_per_gen": ppg, "batch_size": 500, "seed": seed}})
    env = BatchedPursuitTag(ppg + 1, dev, max_steps=max_steps)

    class _View:
        def __init__(self, i):
            self.observation_space = env.observation_space[i]
            self.action_space = env.action_space[i]

    policies = []
    for i in range(2):
        nn = FeedForward(layers, torch.nn.Tanh(), _View(i), 0.01, 5)
        policies.append(Policy(nn, 0.05, Adam(len(Policy.get_flat(nn)), 0.02)))
    nt = NoiseTable.create_shared(comm, 2_000_000, len(policies[0]), seed=seed, device=dev)
    rs = np.random.RandomState(seed + 1)
    # "step" is the constructor's default: built without the keyword, so the
    # same script times a revision from before the keyword existed
    kw = {} if mode == "step" else {"rollout_mode": "episode"}
    if mode == "pair":
        kw["pair_rollout"] = True
    # likewise "bf16": a revision from before weights_dtype ran bf16 rows
    if wdtype != "bf16":
        kw["weights_dtype"] = wdtype
    eng = MultiAgentGpuEngine(cfg, comm, policies, nt, env, rs, **kw)
    assert getattr(eng, "rollout_mode", "step") == ("episode" if mode == "pair" else mode)
    assert getattr(eng, "pair_rollout", False) == (mode == "pair")
    assert getattr(eng, "weights_dtype", "bf16") == wdtype
    return eng


def one_gen(eng):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    _, obstats = eng.step([CenteredRanker(), CenteredRanker()])
    eng.update_obstats(obstats)
    t = dict(eng.timings)
    t["ep_len"] = float(eng.member_steps.mean().item())
    return t


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--modes", nargs="+", default=["step", "episode"],
                   choices=["step", "episode", "pair"])
    p.add_argument("--weights-dtype", nargs="+", default=["bf16"],
                   choices=["bf16", "fp32"], help="member-row dtypes to alternate")
    p.add_argument("--ppg", type=int, nargs="+", default=[32, 1024, 4096])
    p.add_argument("--nets", nargs="+", default=["32,32", "256,256"],
                   help="hidden layer sizes, comma separated, one net per item")
    p.add_argument("--max-steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--gens", type=int, default=5, help="timed generations per mode")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--json", type=str, default=None, help="also write the rows here")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ma_bench needs a GPU: a CPU timing says nothing about this path")
    dev = torch.device("cuda", 0)

    rows = []
    variants = [(m, w) for m in args.modes for w in args.weights_dtype
                if not (m == "pair" and w != "bf16")]      # pair has no fp32 form
    if not variants:
        sys.exit("mode pair runs bf16 rows only: add bf16 to --weights-dtype")
    print(f"{'ppg':>5} {'net':>9} {'mode':>8} {'dtype':>5} {'rollout_s med':>13} {'min':>9} "
          f"{'max':>9} {'gen_s med':>10} {'env-steps/s':>12} {'ep_len':>7}")
    for ppg in args.ppg:
        for net in args.nets:
            layers = [int(x) for x in net.split(",")]
            engs = {k: make_engine(dev, k[0], ppg, layers, args.max_steps, args.seed, k[1])
                    for k in variants}
            runs = {k: [] for k in variants}
            for g in range(args.warmup + args.gens):
                for k in variants:              # alternate the modes and dtypes
                    t = one_gen(engs[k])
                    if g >= args.warmup:
                        runs[k].append(t)
            point = {}
            for k in variants:
                m, w = k
                ro = np.array([t["rollout_s"] for t in runs[k]])
                row = {"ppg": ppg, "net": layers, "mode": m, "weights_dtype": w,
                       "max_steps": args.max_steps,
                       "rollout_s": ro.tolist(),
                       "rollout_s_med": float(np.median(ro)),
                       "gen_s_med": float(np.median([t["gen_s"] for t in runs[k]])),
                       "env_steps_per_s": float(np.median(
                           [t["env_steps"] / t["rollout_s"] for t in runs[k]])),
                       "ep_len": float(np.mean([t["ep_len"] for t in runs[k]]))}
                point[k] = row
                rows.append(row)
                print(f"{ppg:>5} {net:>9} {m:>8} {w:>5} {row['rollout_s_med']:>13.5f} "
                      f"{ro.min():>9.5f} {ro.max():>9.5f} {row['gen_s_med']:>10.5f} "
                      f"{row['env_steps_per_s']:>12.4g} {row['ep_len']:>7.1f}", flush=True)
            for w in args.weights_dtype:
                if not all((m, w) in point for m in ("step", "episode")):
                    continue
                s, e = (np.array(point[m, w]["rollout_s"]) for m in ("step", "episode"))
                spread = max(s.max() - s.min(), e.max() - e.min())
                lead = s.min() - e.max()
                verdict = {"ppg": ppg, "net": layers, "weights_dtype": w,
                           "lead_s": float(lead),
                           "spread_s": float(spread), "clears_bar": bool(lead >= 3 * spread),
                           "speedup_med": float(np.median(s) / np.median(e))}
                rows.append(verdict)
                print(f"      fastest step - slowest episode = {lead:.5f} s, spread "
                      f"{spread:.5f} s, bar (3x spread) "
                      f"{'cleared' if verdict['clears_bar'] else 'NOT cleared'}, "
                      f"median rollout speed-up {verdict['speedup_med']:.1f}x", flush=True)
            if ("episode", "bf16") in point and ("pair", "bf16") in point:
                e, q = (np.array(point[m, "bf16"]["rollout_s"]) for m in ("episode", "pair"))
                spread = max(e.max() - e.min(), q.max() - q.min())
                lead = e.min() - q.max()
                verdict = {"ppg": ppg, "net": layers, "weights_dtype": "bf16",
                           "pair_vs_episode": True, "lead_s": float(lead),
                           "spread_s": float(spread), "clears_bar": bool(lead > 3 * spread),
                           "speedup_med": float(np.median(e) / np.median(q))}
                rows.append(verdict)
                print(f"      fastest episode - slowest pair = {lead:.5f} s, spread "
                      f"{spread:.5f} s, bar (3x spread) "
                      f"{'cleared' if verdict['clears_bar'] else 'NOT cleared'}, "
                      f"median rollout episode / pair {verdict['speedup_med']:.2f}x",
                      flush=True)
            for m in args.modes:
                if (m, "bf16") in point and (m, "fp32") in point:
                    r = point[m, "fp32"]["rollout_s_med"] / point[m, "bf16"]["rollout_s_med"]
                    rows.append({"ppg": ppg, "net": layers, "mode": m,
                                 "fp32_over_bf16_rollout_med": float(r)})
                    print(f"      {m}: fp32 / bf16 median rollout_s = {r:.2f}", flush=True)
            del engs
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
