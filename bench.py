#!/usr/bin/env python3
"""Flagship benchmark: Humanoid-v2 MLP(256,256) objective-ES (BASELINE.json).

Measures whole-job env-steps/sec (and generations/sec) of the GPU engine:
population-batched synthetic Humanoid rollouts, HBM noise table, HIP kernels,
RCCL all-gather across ranks. Weak scaling: policies_per_gen = 1280 per GPU
(10240 at 8 GPUs = the BASELINE "pop=10k on 8 GPUs" config).

Launch (driver contract):
  python bench.py --gpus 1 --steps K --warmup W                 # single GPU
  python bench.py ... --dump-outputs DIR    # + last timed step's outputs (.npy)
  python bench.py ... --full                # + per-phase breakdown in the JSON
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N ...             # one rank/GPU

A plain run does only what the headline figure needs: set up, warm up, time
the K generations, print one JSON line. With the same arguments every input
(noise table, initial weights, env matrices, per-generation draws) is
identical from run to run, so --dump-outputs of two builds compare output
for output.

A "step" is one ES generation. Data is synthetic (seeded latent-dynamics env
of Humanoid-v2's 376-obs/17-action shape; no physics engine or datasets exist
offline) with random-init weights; compute dtype bf16 (theta/forward, fp32
accumulation, fp32 master params, fp64 fitness exchange). The perturbation
sigma*eps rows are encoded e4m3 by default (reported as config.eps_encoding;
--no-fp8 reverts to bf16): the gradient gather re-quantizes through the same
hardware converters, so the update is estimator-exact ES on the quantized
perturbation distribution — fidelity, learning and TCC evidence in
profiles/README.md.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5, help="timed generations")
    p.add_argument("--warmup", type=int, default=2, help="untimed warmup generations")
    p.add_argument("--pop-per-gpu", type=int, default=1280)
    p.add_argument("--max-steps", type=int, default=1000, help="env steps per episode")
    p.add_argument("--env", type=str, default="Humanoid-v2")
    p.add_argument("--objective", type=str, default="reward",
                   choices=["reward", "nsr"],
                   help="nsr = NSR-A style [reward, novelty] 2-objective ES")
    p.add_argument("--layers", type=int, nargs="*", default=[256, 256])
    p.add_argument("--tbl-size", type=int, default=250_000_000)
    p.add_argument("--no-graph", action="store_true")
    p.add_argument("--no-pair", action="store_true",
                   help="disable the antithetic-pair rollout (pair is the "
                        "default: one sigma*eps HBM stream + L2-resident "
                        "shared theta serve both members of a pair — "
                        "measured 1.27x over per-member weight blobs, and "
                        "the perturbation keeps MORE bf16 mantissa)")
    p.add_argument("--cpu", action="store_true", help="debug: run the engine on CPU")
    p.add_argument("--no-fp8", action="store_true",
                   help="disable the fp8 (e4m3) sigma*eps stream (the "
                        "flagship default: halves the dominant HBM weight "
                        "bytes AND load count; the gradient gather re-"
                        "quantizes through the same e4m3 hardware so the "
                        "update is estimator-exact ES on the quantized "
                        "perturbation distribution; fidelity + learning "
                        "evidence in profiles/)")
    p.add_argument("--mode", type=str, default="step", choices=["step", "episode"],
                   help="rollout launch shape: per-step graph-replayed grid, or "
                        "one whole-episode launch per generation (blocks drift; "
                        "phases overlap chip-wide)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "generation returned (fitnesses, noise indices, "
                        "shaped ranks, noiseless evaluation, observation "
                        "statistics, updated parameters) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="everything beyond the headline figure: adds the "
                        "last generation's per-phase wall-time breakdown to "
                        "the result line (off by default; a plain run only "
                        "sets up, warms up, times the steps and reports)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be >= 1")

    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.engine import GpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs import make_batched
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import init_comm, seed_all
    from es_pytorch_amd.utils.rankers import CenteredRanker

    use_cuda = torch.cuda.is_available() and not args.cpu
    if not args.cpu and not use_cuda:
        # never silently emit CPU-stand-in numbers as if they were measured
        raise SystemExit("bench.py: no GPU visible — pass --cpu explicitly for "
                         "the debug stand-in path")
    if args.objective == "nsr" and not use_cuda:
        raise SystemExit("--objective nsr requires the GPU engine")
    comm = init_comm()
    world = comm.size
    if world > 1 and args.gpus != world:
        args.gpus = world
    device = comm.device if use_cuda else torch.device("cpu")

    rs, my_seed, global_seed = seed_all(comm, [1000 + r for r in range(world)])

    ppg = args.pop_per_gpu * world
    cfg = AttrDict({
        "env": {"name": args.env, "max_steps": args.max_steps},
        "noise": {"tbl_size": args.tbl_size, "std": 0.02},
        "policy": {"layer_sizes": list(args.layers), "ac_std": 0.01, "l2coeff": 0.005,
                   "lr": 0.01, "ob_clip": 5, "save_obs_chance": 0.01},
        "general": {"name": "bench", "policies_per_gen": ppg, "batch_size": 500,
                    "seed": global_seed, "pair_rollout": not args.no_pair},
    })

    B = 2 * (ppg // world // 2) + 1
    # fixed-horizon synthetic rollouts: every counted env step is a fully
    # computed batched forward + dynamics step (stable, honest throughput)
    env_kwargs = dict(max_steps=args.max_steps, terminate_on_fall=False)
    if os.environ.get("PYTHONHASHSEED", "random") == "random":
        # the env's default matrix seed goes through hash(name), salted per
        # process: pin it so every run (and every rank) sees the same
        # dynamics. An interpreter with a pinned hash seed already does, and
        # keeps the matrices it always had.
        env_kwargs["matrix_seed"] = 0xE5 + zlib.crc32(args.env.encode()) % 100000
    env = make_batched(cfg.env.name, B, device, **env_kwargs)
    nn = FeedForward(cfg.policy.layer_sizes, torch.nn.Tanh(), env, cfg.policy.ac_std,
                     cfg.policy.ob_clip)
    policy = Policy(nn, cfg.noise.std, Adam(len(Policy.get_flat(nn)), cfg.policy.lr))

    if use_cuda and not os.path.exists(os.path.join(os.path.dirname(
            os.path.abspath(__file__)), "es_pytorch_amd", "ops", "_hip_ops.so")):
        raise RuntimeError("HIP ops library missing on a GPU machine — build first")

    tbl = args.tbl_size if use_cuda else min(args.tbl_size, 2_000_000)
    nt = NoiseTable.create_shared(comm, tbl, len(policy), seed=cfg.general.seed,
                                  device=device)

    if use_cuda:
        # pair_rollout arrives via cfg so the engine's grid-size gate can
        # fall back to the fused per-member path for tiny populations
        engine = GpuEngine(cfg, comm, policy, nt, env, rs, objective=args.objective,
                           use_graph=not args.no_graph, rollout_mode=args.mode,
                           pair_rollout=False if args.no_pair else None,
                           eps_fp8=not (args.no_fp8 or args.no_pair))
        if args.objective == "nsr":
            # seeded starter archive on device (NSR-A semantics: novelty vs
            # the behaviour archive, grown per generation)
            engine.archive = torch.randn(16, 2, dtype=torch.float64,
                                         device=device) * 5.0
    else:
        engine = _CpuRefEngine(cfg, comm, policy, nt, env, rs)
    if args.objective == "nsr":
        from es_pytorch_amd.utils.rankers import MultiObjectiveRanker
        ranker = MultiObjectiveRanker(CenteredRanker(), 0.5)
    else:
        ranker = CenteredRanker()

    for _ in range(args.warmup):
        engine.step(ranker)

    comm.barrier()
    if use_cuda:
        torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    steps_done = 0
    last = None
    for _ in range(args.steps):
        last = engine.step(ranker)
        if args.objective == "nsr" and use_cuda:
            # on-device archive growth inside the timed region (reference
            # nsra.py:130-135): ONE 2-float broadcast + device cdist re-score
            engine.grow_archive()
        steps_done += engine.timings["env_steps"]
    comm.barrier()
    if use_cuda:
        torch.cuda.synchronize(device)
    elapsed = time.perf_counter() - t0

    # per-rank diagnostics to stderr (the driver parses stdout JSON only)
    print(f"[bench rank {comm.rank}/{world}] elapsed={elapsed:.3f}s "
          f"timings={getattr(engine, 'timings', {})}", file=sys.stderr, flush=True)

    # MAX elapsed over ranks = whole-job wall time
    elapsed = comm.allreduce_scalar(elapsed) if world == 1 else max(
        comm.allgather_obj(elapsed))
    # env_steps from engine are already whole-job (allreduced per gen)
    env_steps_per_sec = steps_done / elapsed
    gens_per_sec = args.steps / elapsed

    if args.dump_outputs and comm.rank == 0:
        # after the clock stopped: every rank holds identical outputs
        # (redundant ranking/update), so rank 0's copy is the job's
        _dump_outputs(args.dump_outputs, last, ranker, policy)

    if comm.rank == 0:
        out = {
            "metric": (f"env-steps/sec (whole node), {args.env} "
                       f"{'NSR-A' if args.objective == 'nsr' else 'objective-ES'}"),
            "value": round(env_steps_per_sec, 1),
            "unit": "env-steps/s",
            "n_gpus": args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1000.0 * elapsed / args.steps, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "model": f"MLP{tuple(args.layers)}",
                "env": args.env,
                "global_batch": ppg,
                "policies_per_gen": ppg,
                "episode_len": args.max_steps,
                "seq_len": args.max_steps,
                "objective": args.objective,
                "parallelism": f"dp{args.gpus}",
                "pair_rollout": bool(getattr(engine, "pair_rollout", False)),
                "eps_encoding": ("e4m3" if getattr(engine, "eps_fp8", False)
                                 else "bf16"),
                "gens_per_sec": round(gens_per_sec, 3),
                "noise_table_elems": tbl,
                "n_params": len(policy),
            },
        }
        if args.full:
            out["config"]["last_step_timings"] = {
                k: round(float(v), 6) for k, v in engine.timings.items()}
        print(json.dumps(out))
    return 0


def _dump_outputs(folder, last, ranker, policy):
    """Write what a caller of the timed path holds after its last step: the
    (noiseless result, generation ObStat) pair engine.step returned, the
    ranker it filled and the parameters it updated — one .npy each, fp64
    except the fp32 parameters (well under 1 MB in all at flagship size)."""
    os.makedirs(folder, exist_ok=True)
    arrays = {
        "fits_pos": np.asarray(ranker.fits_pos, dtype=np.float64),
        "fits_neg": np.asarray(ranker.fits_neg, dtype=np.float64),
        "noise_inds": np.asarray(ranker.noise_inds, dtype=np.float64),
        "ranked_fits": np.asarray(ranker.ranked_fits, dtype=np.float64),
        "flat_params": np.asarray(policy.flat_params, dtype=np.float32),
    }
    if last is not None:  # the CPU stand-in returns nothing
        noiseless, obstat = last
        arrays.update({
            "noiseless_result": np.asarray(noiseless.result, dtype=np.float64),
            "noiseless_behaviour": np.asarray(noiseless.behaviour, dtype=np.float64),
            "env_steps": np.asarray([noiseless.steps], dtype=np.float64),
            "obstat_sum": np.asarray(obstat.sum, dtype=np.float64),
            "obstat_sumsq": np.asarray(obstat.sumsq, dtype=np.float64),
            "obstat_count": np.asarray([obstat.count], dtype=np.float64),
        })
    for name, arr in arrays.items():
        np.save(os.path.join(folder, name + ".npy"), arr)


class _CpuRefEngine:
    """Tiny CPU stand-in so bench.py --cpu runs without a GPU (debug only)."""

    def __init__(self, cfg, comm, policy, nt, env, rs):
        from es_pytorch_amd.core import engine as _e
        self.cfg, self.comm, self.policy, self.nt, self.env, self.rs = \
            cfg, comm, policy, nt, env, rs
        self.timings = {}
        self.pairs = cfg.general.policies_per_gen // comm.size // 2
        self.B = env.batch
        self.perm = _e.forward_perm(policy._module.layer_dims())

    def step(self, ranker):
        import torch as T
        t0 = time.perf_counter()
        cfg, env, policy = self.cfg, self.env, self.policy
        offs = self.nt.sample_idxs(self.rs, self.pairs)
        n = len(policy)
        theta = T.from_numpy(policy.flat_params)
        signs = np.concatenate([np.ones(self.pairs), -np.ones(self.pairs), [0.0]])
        offs_full = np.concatenate([offs, offs, [0]]).astype(np.int64)
        W = T.stack([theta + float(s) * policy.std * self.nt.noise[o:o + n]
                     for s, o in zip(signs, offs_full)])
        obs = env.reset(0)
        rew_tot = T.zeros(self.B)
        alive = T.ones(self.B)
        steps = T.zeros(())
        dims = policy._module.layer_dims()
        mean = T.zeros(env.ob_dim)
        std = T.ones(env.ob_dim)
        for t in range(cfg.env.max_steps):
            x = T.clamp((obs - mean) / std, -5, 5)
            off = 0
            for li, (I, O) in enumerate(zip(dims[:-1], dims[1:])):
                w = W[:, off:off + I * O].reshape(self.B, O, I)
                b = W[:, off + I * O:off + I * O + O]
                x = T.tanh(T.einsum("boi,bi->bo", w, x) + b)
                off += I * O + O
            obs, rew, done = env.step(x)
            rew_tot += rew * alive
            steps += alive.sum()
            alive *= (1 - done.float())
        rows = np.zeros((self.pairs, 3))
        rows[:, 0] = rew_tot[:self.pairs].numpy()
        rows[:, 1] = rew_tot[self.pairs:2 * self.pairs].numpy()
        rows[:, 2] = offs
        allr = self.comm.allgather_rows(T.from_numpy(rows)).numpy()
        ranker.rank(allr[:, :1], allr[:, 1:2], allr[:, 2])
        from es_pytorch_amd.utils.utils import scale_noise
        g = scale_noise(ranker.ranked_fits, ranker.noise_inds, self.nt, n,
                        cfg.general.batch_size).numpy() / ranker.n_fits_ranked
        policy.optim_step(cfg.policy.l2coeff * policy.flat_params - g)
        total = float(self.comm.allreduce_scalar(float(steps.item())))
        self.timings = {"env_steps": total, "gen_s": time.perf_counter() - t0}


if __name__ == "__main__":
    sys.exit(main())
