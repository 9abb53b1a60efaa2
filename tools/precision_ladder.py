#!/usr/bin/env python3
"""Precision ladder: one generation of the SAME seeded population through
every numerics variant of the engine, each compared with the fp32-weights
mode (the reference's precision):

  fp32       float32(theta +- sigma*eps) rows, fp32-weight forward
  bf16-blob  bf16(theta +- sigma*eps) rows
  bf16-pair  bf16(theta) +- bf16(sigma*eps)
  e4m3-pair  bf16(theta) +- e4m3(sigma*eps)

Prints, per variant, the Spearman rank correlation of the 2*pairs member
fitnesses and the cosine of the reconstructed gradients against fp32. The
numbers are a record (profiles/README.md), not an assertion: chaotic rollouts
amplify one-ulp weight differences with the horizon.

  python tools/precision_ladder.py --horizon 100 --pop 1280
"""
import argparse
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

VARIANTS = [
    ("fp32", dict(weights_dtype="fp32")),
    ("bf16-blob", dict(weights_dtype="bf16", pair_rollout=False)),
    ("bf16-pair", dict(weights_dtype="bf16", pair_rollout=True, eps_fp8=False)),
    ("e4m3-pair", dict(weights_dtype="bf16", pair_rollout=True, eps_fp8=True)),
]


def spearman(a, b):
    """Spearman rank correlation (average ranks for ties), numpy only."""
    def ranks(x):
        order = np.argsort(x, kind="stable")
        r = np.empty(len(x), dtype=np.float64)
        r[order] = np.arange(len(x), dtype=np.float64)
        xs = x[order]
        i = 0
        while i < len(xs):          # average the ranks of tied runs
            j = i
            while j + 1 < len(xs) and xs[j + 1] == xs[i]:
                j += 1
            if j > i:
                r[order[i:j + 1]] = 0.5 * (i + j)
            i = j + 1
        return r
    ra, rb = ranks(np.asarray(a, np.float64)), ranks(np.asarray(b, np.float64))
    ra -= ra.mean()
    rb -= rb.mean()
    return float(np.dot(ra, rb) / np.sqrt(np.dot(ra, ra) * np.dot(rb, rb)))


def run_variant(args, kw):
    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.engine import GpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs import make_batched
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import Comm
    from es_pytorch_amd.utils.rankers import CenteredRanker

    torch.manual_seed(99)
    comm = Comm(torch.device("cuda", 0))
    cfg = AttrDict({"env": {"name": args.env, "max_steps": args.horizon},
                    "noise": {"tbl_size": args.tbl, "std": args.std},
                    "policy": {"layer_sizes": list(args.layers), "ac_std": 0.01,
                               "l2coeff": 0.005, "lr": 0.01, "ob_clip": 5,
                               "save_obs_chance": 0.01},
                    "general": {"policies_per_gen": args.pop, "batch_size": 500,
                                "seed": 9}})
    # fixed env matrices in every process (the default seed depends on the
    # per-process str hash salt), derived as bench.py derives them
    env = make_batched(args.env, args.pop + 1, comm.device, max_steps=args.horizon,
                       terminate_on_fall=True,
                       matrix_seed=0xE5 + zlib.crc32(args.env.encode()) % 100000)
    nn = FeedForward(list(args.layers), torch.nn.Tanh(), env, 0.01, 5)
    policy = Policy(nn, args.std, Adam(len(Policy.get_flat(nn)), 0.01))
    nt = NoiseTable.create_shared(comm, args.tbl, len(policy), seed=9, device=comm.device)
    eng = GpuEngine(cfg, comm, policy, nt, env, np.random.RandomState(100),
                    use_graph=False, **kw)
    ranker = CenteredRanker()
    eng.step(ranker)
    torch.cuda.synchronize()
    fits = np.concatenate([ranker.fits_pos, ranker.fits_neg]).ravel()
    return fits, eng.grad.cpu().numpy().copy(), eng.numerics


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--env", default="Humanoid-v2")
    p.add_argument("--layers", type=int, nargs="*", default=[256, 256])
    p.add_argument("--pop", type=int, default=1280)
    p.add_argument("--horizon", type=int, nargs="*", default=[100])
    p.add_argument("--std", type=float, default=0.02)
    p.add_argument("--tbl", type=int, default=50_000_000)
    args = p.parse_args()
    horizons = list(args.horizon)
    for h in horizons:
        args.horizon = h
        base = None
        print(f"# {args.env} pop {args.pop} layers {args.layers} sigma {args.std} "
              f"horizon {h}", flush=True)
        print(f"{'variant':<10} {'fitness spearman':>17} {'grad cosine':>12}  numerics")
        for name, kw in VARIANTS:
            fits, grad, numerics = run_variant(args, kw)
            if base is None:
                base = (fits, grad)
            rho = spearman(base[0], fits)
            cos = float(np.dot(base[1], grad) /
                        (np.linalg.norm(base[1]) * np.linalg.norm(grad)))
            print(f"{name:<10} {rho:>17.4f} {cos:>12.4f}  {numerics}", flush=True)


if __name__ == "__main__":
    main()
