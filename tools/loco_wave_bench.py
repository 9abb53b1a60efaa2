#!/usr/bin/env python3
"""Locomotion rollout bench for small envs and nets: the rollout of one
generation in rollout_mode="episode" (es_loco_episode, a workgroup per slot,
plus the noiseless side launch) and with loco_wave=True (es_loco_wave_episode,
a wavefront per slot, all slots in one launch), on one box.

For every grid point both engines are built from the same seeds and their
rollouts ALTERNATE (episode, wave, episode, ...) after a warm-up, so both see
the same machine state. The parameters stay fixed - pheno, reset and rollout
only, no optimizer step - so that episode length does not drift between rows;
each rollout ends in a device synchronise and is timed with the host clock
around it. Slots that fall leave the wave kernel's loop while the block kernel
steps every slot max_steps times, so the mean episode length is printed with
every row: it is part of the answer.

The project's bar for a speed claim: the SLOWEST wave run must lead the
FASTEST episode run by more than three times the run-to-run spread (max - min
within a mode, the larger of the two).

  python tools/loco_wave_bench.py                      # the whole grid
  python tools/loco_wave_bench.py --modes episode      # block kernel only (also
                                                       # runs on a library from
                                                       # before the wave kernel)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ENVS = {"hopper": "Hopper-v3", "ant": "Ant-v3", "walker": "Walker2d-v3",
        "swimmer": "Swimmer-v3"}
MODES = ("episode", "wave")      # old -> new


def make_engine(dev, mode, env_name, ppg, layers, max_steps, seed, wdt):
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
                    "noise": {"tbl_size": 5_000_000, "std": 0.02},
                    "policy": {"layer_sizes": layers, "ac_std": 0.01, "l2coeff": 0.005,
                               "lr": 0.01, "ob_clip": 5, "save_obs_chance": 0.01},
                    "general": {"policies_per_gen": ppg, "batch_size": 500, "seed": seed,
                                "weights_dtype": wdt}})
    # matrix_seed: both engines get the same env matrices in every process
    env = make_batched(env_name, ppg + 1, dev, max_steps=max_steps, matrix_seed=seed)
    nn = FeedForward(layers, torch.nn.Tanh(), env, 0.01, 5)
    policy = Policy(nn, 0.02, Adam(len(Policy.get_flat(nn)), 0.01))
    nt = NoiseTable.create_shared(comm, 5_000_000, len(policy), seed=seed, device=dev)
    # "episode" is built without the new keyword, so the same script times a
    # revision from before it existed
    kw = {"episode": {"rollout_mode": "episode"}, "wave": {"loco_wave": True}}[mode]
    eng = GpuEngine(cfg, comm, policy, nt, env, np.random.RandomState(seed + 1),
                    use_graph=False, **kw)
    assert eng.numerics["path"] == {"episode": "fused", "wave": "loco_wave"}[mode]
    assert eng.rollout_mode == "episode"
    eng._upload_offsets()               # one draw: the same members every run
    eng.seed_dev.fill_(seed)
    eng.acstd_dev.fill_(0.01)
    return eng


def one_rollout(eng):
    """(rollout seconds, mean episode length) of one generation's rollout."""
    eng._pheno()
    eng._reset_rollout_state()
    eng.obs_buf.copy_(eng.env.reset(0))
    torch.cuda.synchronize(eng.device)
    t0 = time.perf_counter()
    eng._rollout()
    torch.cuda.synchronize(eng.device)
    return time.perf_counter() - t0, float(eng.member_steps.mean().item())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--modes", nargs="+", default=list(MODES), choices=MODES)
    p.add_argument("--envs", nargs="+", default=["hopper", "ant"], choices=list(ENVS))
    p.add_argument("--ppg", type=int, nargs="+", default=[256, 1024, 4096])
    p.add_argument("--nets", nargs="+", default=["32,32", "64,64"],
                   help="hidden layer sizes, comma separated, one entry per net")
    p.add_argument("--max-steps", type=int, default=1000)
    p.add_argument("--weights-dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--runs", type=int, default=5, help="timed rollouts per mode")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--json", type=str, default=None, help="also write the rows here")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loco_wave_bench needs a GPU: a CPU timing says nothing about this path")
    dev = torch.device("cuda", 0)

    rows = []
    print(f"{'env':>8} {'net':>7} {'ppg':>5} {'mode':>8} {'rollout_s med':>13} {'min':>9} "
          f"{'max':>9} {'env-steps/s':>12} {'ep_len':>7}")
    for env_key in args.envs:
        for net in args.nets:
            layers = [int(x) for x in net.split(",")]
            for ppg in args.ppg:
                engs = {m: make_engine(dev, m, ENVS[env_key], ppg, layers, args.max_steps,
                                       args.seed, args.weights_dtype) for m in args.modes}
                runs = {m: [] for m in args.modes}
                for g in range(args.warmup + args.runs):
                    for m in args.modes:            # alternate the modes
                        r = one_rollout(engs[m])
                        if g >= args.warmup:
                            runs[m].append(r)
                point = {}
                for m in args.modes:
                    ro = np.array([r[0] for r in runs[m]])
                    ep_len = float(np.mean([r[1] for r in runs[m]]))
                    row = {"env": env_key, "net": layers, "ppg": ppg, "mode": m,
                           "weights": args.weights_dtype, "max_steps": args.max_steps,
                           "rollout_s": ro.tolist(), "rollout_s_med": float(np.median(ro)),
                           "env_steps_per_s": ep_len * (ppg + 1) / float(np.median(ro)),
                           "ep_len": ep_len}
                    point[m] = row
                    rows.append(row)
                    print(f"{env_key:>8} {net:>7} {ppg:>5} {m:>8} {row['rollout_s_med']:>13.5f} "
                          f"{ro.min():>9.5f} {ro.max():>9.5f} {row['env_steps_per_s']:>12.4g} "
                          f"{ep_len:>7.1f}", flush=True)
                if len(point) == 2:
                    s, e = (np.array(point[m]["rollout_s"]) for m in MODES)
                    spread = max(s.max() - s.min(), e.max() - e.min())
                    lead = s.min() - e.max()
                    verdict = {"env": env_key, "net": layers, "ppg": ppg, "lead_s": float(lead),
                               "spread_s": float(spread), "clears_bar": bool(lead > 3 * spread),
                               "speedup_med": float(np.median(s) / np.median(e))}
                    rows.append(verdict)
                    print(f"      fastest episode - slowest wave = {lead:.5f} s, spread "
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
