#!/usr/bin/env python3
"""Classic-control rollout bench: GpuEngine.step per generation on the generic
path under hipGraph (one es_mlp_fwd launch plus a dozen torch kernels per env
step) against classic_fused (one es_classic_episode launch), on one box.

For every grid point two engines are built from the same seeds, one per mode,
and their generations ALTERNATE (generic, fused, generic, ...) after a
warm-up, so both see the same machine state. Each generation ends in a device
synchronise inside engine.step; rollout_s and gen_s are the engine's own
timings. CartPole slots whose episode ends leave the fused kernel's loop while
the generic path steps every slot max_steps times, so the mean episode length
is printed with every row: it is part of the answer. Pendulum never ends
early, so it isolates launch overhead from early exit.

The project's bar for a speed claim: the SLOWEST run of the new mode must
lead the FASTEST run of the old one by more than three times the run-to-run
spread (max - min within a mode, the larger of the two).

  python tools/classic_bench.py                     # the whole grid, both modes
  python tools/classic_bench.py --modes generic     # baseline only
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ENVS = {"cartpole": ("CartPole-v1", 500), "pendulum": ("Pendulum-v1", 200)}


def make_engine(dev, mode, env_name, ppg, layers, max_steps, seed):
    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.engine import GpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs import make_batched
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import Comm

    torch.manual_seed(seed)
    comm = Comm(dev)
    cfg = AttrDict({"env": {"name": env_name, "max_steps": max_steps},
                    "noise": {"tbl_size": 5_000_000, "std": 0.05},
                    "policy": {"layer_sizes": layers, "ac_std": 0.01, "l2coeff": 0.005,
                               "lr": 0.02, "ob_clip": 5, "save_obs_chance": 0.1},
                    "general": {"policies_per_gen": ppg, "batch_size": 500, "seed": seed}})
    env = make_batched(env_name, ppg + 1, dev)
    nn = FeedForward(layers, torch.nn.Tanh(), env, 0.01, 5)
    policy = Policy(nn, 0.05, Adam(len(Policy.get_flat(nn)), 0.02))
    nt = NoiseTable.create_shared(comm, 5_000_000, len(policy), seed=seed, device=dev)
    rs = np.random.RandomState(seed + 1)
    # "generic" is the constructor's default: built without the keyword, so
    # the same script times a revision from before the keyword existed
    kw = {} if mode == "generic" else {"classic_fused": True}
    eng = GpuEngine(cfg, comm, policy, nt, env, rs, use_graph=True, **kw)
    assert eng.numerics["path"] == ("generic" if mode == "generic" else "classic")
    return eng


def one_gen(eng):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    _, obstat = eng.step(CenteredRanker())
    eng.update_obstat(obstat)
    t = dict(eng.timings)
    t["ep_len"] = float(eng.member_steps.mean().item())
    return t


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--modes", nargs="+", default=["generic", "fused"],
                   choices=["generic", "fused"])
    p.add_argument("--envs", nargs="+", default=["cartpole", "pendulum"], choices=list(ENVS))
    p.add_argument("--ppg", type=int, nargs="+", default=[64, 1024, 4096])
    p.add_argument("--net", default="32,32", help="hidden layer sizes, comma separated")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--gens", type=int, default=5, help="timed generations per mode")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--json", type=str, default=None, help="also write the rows here")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("classic_bench needs a GPU: a CPU timing says nothing about this path")
    dev = torch.device("cuda", 0)
    layers = [int(x) for x in args.net.split(",")]

    rows = []
    print(f"{'env':>9} {'ppg':>5} {'mode':>8} {'rollout_s med':>13} {'min':>9} {'max':>9} "
          f"{'gen_s med':>10} {'env-steps/s':>12} {'ep_len':>7}")
    for env_key in args.envs:
        env_name, max_steps = ENVS[env_key]
        for ppg in args.ppg:
            engs = {m: make_engine(dev, m, env_name, ppg, layers, max_steps, args.seed)
                    for m in args.modes}
            runs = {m: [] for m in args.modes}
            for g in range(args.warmup + args.gens):
                for m in args.modes:            # alternate the modes
                    t = one_gen(engs[m])
                    if g >= args.warmup:
                        runs[m].append(t)
            point = {}
            for m in args.modes:
                ro = np.array([t["rollout_s"] for t in runs[m]])
                row = {"env": env_key, "ppg": ppg, "net": layers, "mode": m,
                       "max_steps": max_steps, "rollout_s": ro.tolist(),
                       "rollout_s_med": float(np.median(ro)),
                       "gen_s_med": float(np.median([t["gen_s"] for t in runs[m]])),
                       "env_steps_per_s": float(np.median(
                           [t["env_steps"] / t["rollout_s"] for t in runs[m]])),
                       "ep_len": float(np.mean([t["ep_len"] for t in runs[m]]))}
                point[m] = row
                rows.append(row)
                print(f"{env_key:>9} {ppg:>5} {m:>8} {row['rollout_s_med']:>13.5f} "
                      f"{ro.min():>9.5f} {ro.max():>9.5f} {row['gen_s_med']:>10.5f} "
                      f"{row['env_steps_per_s']:>12.4g} {row['ep_len']:>7.1f}", flush=True)
            if len(point) == 2:
                s, e = (np.array(point[m]["rollout_s"]) for m in ("generic", "fused"))
                spread = max(s.max() - s.min(), e.max() - e.min())
                lead = s.min() - e.max()
                verdict = {"env": env_key, "ppg": ppg, "net": layers, "lead_s": float(lead),
                           "spread_s": float(spread), "clears_bar": bool(lead > 3 * spread),
                           "speedup_med": float(np.median(s) / np.median(e))}
                rows.append(verdict)
                print(f"      fastest generic - slowest fused = {lead:.5f} s, spread "
                      f"{spread:.5f} s, bar (3x spread) "
                      f"{'cleared' if verdict['clears_bar'] else 'NOT cleared'}, "
                      f"median rollout speed-up {verdict['speedup_med']:.1f}x", flush=True)
            del engs
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
