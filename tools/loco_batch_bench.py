#!/usr/bin/env python3
"""Locomotion rollout bench for eps_per_policy > 1: the rollout of one
generation with loco_batch=True (es_loco_batch_episode, a block per member,
its episodes as MFMA columns) against the engine's existing paths at the same
eps on the same tree:

  default  the config path of configs/flagrun.json (pair_rollout + eps_fp8 in
           the config, so the engine's own gate picks pair / fp8 where it
           applies), replayed from its hipGraph
  episode  rollout_mode="episode" (es_loco_episode, a block per slot)
  wave     loco_wave=True (es_loco_wave_episode, a wave per slot; nets at most
           64 wide)
  batch    loco_batch=True
  wave_batch  loco_wave_batch=True (es_loco_wave_batch_episode, a wave per
           member, its episodes as MFMA columns; nets at most 64 wide)

Method and bar are tools/loco_wave_bench.py's: same seeds, fixed parameters,
rollouts ALTERNATE between the modes after a warm-up, each ends in a device
synchronise; a speed claim needs the SLOWEST run of the new mode (wave_batch
where it runs, batch otherwise) to lead the FASTEST run of the other mode by
more than three times the larger max - min spread.

  python tools/loco_batch_bench.py
  python tools/loco_batch_bench.py --modes default episode   # also runs on a
                                        # library from before the batch kernel
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loco_wave_bench import one_rollout  # noqa: E402

ENVS = {"humanoidflagrun": "HumanoidFlagrunBulletEnv-v0", "antflagrun": "AntFlagrun-v3",
        "hopper": "Hopper-v3"}
NETS = {"humanoidflagrun": [256, 256], "antflagrun": [64, 64], "hopper": [64, 64]}
MODES = ("default", "episode", "wave", "batch", "wave_batch")
MODE_KW = {"default": dict(use_graph=True),
           "episode": dict(use_graph=False, rollout_mode="episode", pair_rollout=False),
           "wave": dict(use_graph=False, loco_wave=True),
           "batch": dict(use_graph=False, loco_batch=True),
           "wave_batch": dict(use_graph=False, loco_wave_batch=True)}
PATHS = {"wave": "loco_wave", "batch": "loco_batch", "wave_batch": "loco_wave_batch"}


def make_engine(dev, mode, env_name, ppg, eps, layers, max_steps, seed, wdt):
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
    general = {"policies_per_gen": ppg, "eps_per_policy": eps, "batch_size": 500,
               "seed": seed, "weights_dtype": wdt}
    if mode == "default":
        general.update(pair_rollout=True, eps_fp8=True)
    cfg = AttrDict({"env": {"name": env_name, "max_steps": max_steps},
                    "noise": {"tbl_size": 5_000_000, "std": 0.02},
                    "policy": {"layer_sizes": layers, "ac_std": 0.01, "l2coeff": 0.005,
                               "lr": 0.01, "ob_clip": 5, "save_obs_chance": 0.01},
                    "general": general})
    env = make_batched(env_name, (ppg + 1) * eps, dev, max_steps=max_steps, matrix_seed=seed)
    nn = FeedForward(layers, torch.nn.Tanh(), env, 0.01, 5)
    policy = Policy(nn, 0.02, Adam(len(Policy.get_flat(nn)), 0.01))
    nt = NoiseTable.create_shared(comm, 5_000_000, len(policy), seed=seed, device=dev)
    eng = GpuEngine(cfg, comm, policy, nt, env, np.random.RandomState(seed + 1),
                    **MODE_KW[mode])
    if mode in PATHS:
        assert eng.numerics["path"] == PATHS[mode]
    eng._upload_offsets()               # one draw: the same members every run
    eng.seed_dev.fill_(seed)
    eng.acstd_dev.fill_(0.01)
    return eng


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--modes", nargs="+", default=["default", "episode", "batch"],
                   choices=MODES)
    p.add_argument("--envs", nargs="+", default=["humanoidflagrun", "antflagrun"],
                   choices=list(ENVS))
    p.add_argument("--ppg", type=int, nargs="+", default=[256, 1280])
    p.add_argument("--eps", type=int, nargs="+", default=[4, 10])
    p.add_argument("--max-steps", type=int, default=1000)
    p.add_argument("--weights-dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--runs", type=int, default=5, help="timed rollouts per mode")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--json", type=str, default=None, help="also write the rows here")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loco_batch_bench needs a GPU: a CPU timing says nothing about this path")
    dev = torch.device("cuda", 0)

    rows = []
    print(f"{'env':>16} {'ppg':>5} {'eps':>3} {'mode':>10} {'path':>16} {'rollout_s med':>13} "
          f"{'min':>9} {'max':>9} {'ep_len':>7}")
    for env_key in args.envs:
        for ppg in args.ppg:
            for eps in args.eps:
                engs = {m: make_engine(dev, m, ENVS[env_key], ppg, eps, NETS[env_key],
                                       args.max_steps, args.seed, args.weights_dtype)
                        for m in args.modes}
                runs = {m: [] for m in args.modes}
                for g in range(args.warmup + args.runs):
                    for m in args.modes:            # alternate the modes
                        r = one_rollout(engs[m])
                        if g >= args.warmup:
                            runs[m].append(r)
                point = {}
                for m in args.modes:
                    ro = np.array([r[0] for r in runs[m]])
                    num = engs[m].numerics
                    path = f"{num['path']}/{num['eps_encoding']}/{num['rollout_mode']}"
                    point[m] = {"env": env_key, "ppg": ppg, "eps": eps, "mode": m, "path": path,
                                "weights": args.weights_dtype, "max_steps": args.max_steps,
                                "rollout_s": ro.tolist(), "rollout_s_med": float(np.median(ro)),
                                "ep_len": float(np.mean([r[1] for r in runs[m]]))}
                    rows.append(point[m])
                    print(f"{env_key:>16} {ppg:>5} {eps:>3} {m:>10} {path:>16} "
                          f"{np.median(ro):>13.5f} {ro.min():>9.5f} {ro.max():>9.5f} "
                          f"{point[m]['ep_len']:>7.1f}", flush=True)
                new = "wave_batch" if "wave_batch" in point else "batch"
                if new in point:
                    b = np.array(point[new]["rollout_s"])
                    for m in args.modes:
                        if m == new:
                            continue
                        o = np.array(point[m]["rollout_s"])
                        spread = max(o.max() - o.min(), b.max() - b.min())
                        lead = o.min() - b.max()
                        v = {"env": env_key, "ppg": ppg, "eps": eps, "new": new, "against": m,
                             "lead_s": float(lead), "spread_s": float(spread),
                             "clears_bar": bool(lead > 3 * spread),
                             "speedup_med": float(np.median(o) / np.median(b))}
                        rows.append(v)
                        print(f"      fastest {m} - slowest {new} = {lead:.5f} s, spread "
                              f"{spread:.5f} s, bar (3x spread) "
                              f"{'cleared' if v['clears_bar'] else 'NOT cleared'}, median "
                              f"rollout speed-up {v['speedup_med']:.2f}x", flush=True)
                del engs
                torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
