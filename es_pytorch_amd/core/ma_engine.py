"""MultiAgentGpuEngine — GPU-batched co-evolution (beyond reference parity).

The reference evaluates co-evolving policies in ONE Unity sim per CPU rank,
sequentially (``multi_agent.py:33-67``). Here N policies' perturbations play
against each other in B batched env instances per generation: env instance b
is a joint game between perturbation b of EVERY policy. Per env step each
policy's population forward runs as one HIP kernel (``mlp_fwd.hip``) over
its agents' observations, the batched multi-agent env consumes the action
list, and per-agent rewards accumulate under a shared alive mask.

Per-policy updates mirror the single-policy engine: RCCL all_gather of that
policy's (fit+, fit-, idx) triples, redundant host ranking, gather-GEMV
gradient from the shared noise table, fused Adam — all per policy, from its
own fitness column (reference ``multi_agent.py:110-125``).

Unlike the reference (which evaluates the SAME +noise phenotypes twice —
``multi_agent.py:48-49``, a documented quirk), this engine uses true
antithetic pairs: instance slots [0, pairs) carry +noise for every policy
and [pairs, 2*pairs) carry -noise; slot 2*pairs is the all-noiseless game.

Two rollout modes. ``"step"`` (the default) is the loop described above.
``"episode"`` (``rollout_mode=`` or ``general.ma_rollout_mode``) plays the
whole rollout of a generation in ONE launch of the fused tag kernel
(``rollout_tag.hip``): both policies' forwards, the env step and the
bookkeeping per game, with games that end leaving early. It draws the same
action noise as the step loop and needs the ``BatchedPursuitTag`` env on a GPU.

Two weight dtypes, for both policies alike (``weights_dtype=`` or
``general.weights_dtype``, the single-policy engine's key). ``"bf16"`` (the
default) evaluates the members on bf16 rows. ``"fp32"`` materializes
``float32(theta + s*eps)`` rows (``es_pheno_f32``) and runs the fp32-weight
forward in either rollout mode (``es_mlp_fwd_f32`` per step,
``es_tag_episode_f32`` per episode): the reference's numerics, and what ties
a generation to ``theta`` and the noise table in the oracle tests.

``pair_rollout=True`` (or ``general.ma_pair_rollout``; bf16, episode mode
only) shares the rows across the two games of an antithetic pair: no member
blob is materialized, one workgroup of ``es_tag_pair_episode`` plays games p
and pairs + p on ``bf16(theta) +- bf16(sigma*eps_p)``, streaming ONE
sigma*eps row per policy plus the theta row the whole grid shares. Two bf16
roundings instead of one; the gradient uses the unquantized noise, as on the
single-policy bf16 pair path. Off by default.
"""
from __future__ import annotations

import time
from typing import List, Optional, Tuple

import numpy as np
import torch

from es_pytorch_amd import ops
from es_pytorch_amd.core.engine import forward_perm
from es_pytorch_amd.core.noisetable import NoiseTable
from es_pytorch_amd.core.policy import Policy
from es_pytorch_amd.envs.multiagent import BatchedPursuitTag
from es_pytorch_amd.nn.obstat import ObStat
from es_pytorch_amd.nn.optimizers import Adam
from es_pytorch_amd.parallel.comm import Comm
from es_pytorch_amd.utils.rankers import Ranker


class _PolicyState:
    """Per-policy device state (theta, moments, member weight blobs)."""

    def __init__(self, policy: Policy, device, pairs: int, ob_dim: int,
                 weights_dtype: torch.dtype = torch.bfloat16, pair: bool = False):
        self.policy = policy
        d = device
        self.dims = policy._module.layer_dims()
        self.n = len(policy)
        self.perm = forward_perm(self.dims).to(d)
        self.dims_arr = np.array(self.dims, dtype=np.int32)
        flat = torch.from_numpy(policy.flat_params).to(d)
        self.theta = flat[self.perm].contiguous()
        self.m = torch.zeros(self.n, dtype=torch.float32, device=d)
        self.v = torch.zeros(self.n, dtype=torch.float32, device=d)
        self.row_stride = (self.n + 7) // 8 * 8
        M = 2 * pairs + 1
        if pair:
            # no member blob: one theta row and `pairs` sigma*eps rows, the
            # row behind them zero for the noiseless block; one guard row
            # each, as the single-policy engine keeps for the pair forward
            self._theta_blob = torch.zeros((2, self.row_stride), dtype=torch.bfloat16,
                                           device=d)
            self.theta_row = self._theta_blob[:1]
            self._eps_blob = torch.zeros((pairs + 2, self.row_stride),
                                         dtype=torch.bfloat16, device=d)
            self.eps_rows = self._eps_blob[:pairs]
            self._zeros_n = torch.zeros(self.n, dtype=torch.float32, device=d)
            self._zero_off = torch.zeros(1, dtype=torch.int64, device=d)
            self._zero_sign = torch.zeros(1, dtype=torch.float32, device=d)
            self._one_signs = torch.ones(pairs, dtype=torch.float32, device=d)
        else:
            self.weights = torch.empty((M, self.row_stride), dtype=weights_dtype,
                                       device=d)
        self.offsets = torch.zeros(M, dtype=torch.int64, device=d)
        self.signs = torch.cat([torch.ones(pairs), -torch.ones(pairs),
                                torch.zeros(1)]).to(d)
        self.acstd_dev = torch.zeros(1, dtype=torch.float32, device=d)
        self.grad = torch.empty(self.n, dtype=torch.float32, device=d)
        self.obmean = torch.zeros(ob_dim, dtype=torch.float32, device=d)
        self.obstd = torch.ones(ob_dim, dtype=torch.float32, device=d)
        self.push_obstat()

    def push_obstat(self):
        self.obmean.copy_(torch.from_numpy(
            np.asarray(self.policy.obstat.mean, dtype=np.float32)))
        self.obstd.copy_(torch.from_numpy(
            np.asarray(self.policy.obstat.std, dtype=np.float32)))

    def sync_host(self):
        flat = torch.empty(self.n, dtype=torch.float32, device=self.theta.device)
        flat[self.perm] = self.theta
        self.policy.flat_params[:] = flat.cpu().numpy()
        if not np.isfinite(self.policy.flat_params).all():
            raise FloatingPointError("non-finite parameters in co-evolution update")


class MultiAgentGpuEngine:
    def __init__(self, cfg, comm: Comm, policies: List[Policy], nt: NoiseTable, env,
                 rs: np.random.RandomState, rollout_mode: Optional[str] = None,
                 weights_dtype: Optional[str] = None,
                 pair_rollout: Optional[bool] = None):
        self.cfg = cfg
        self.comm = comm
        self.nt = nt
        self.env = env
        self.rs = rs
        self.device = nt.noise.device
        self.n_agents = len(policies)
        assert env.N_AGENTS == self.n_agents
        if rollout_mode is None:
            rollout_mode = cfg.general.get("ma_rollout_mode", "step")
        if rollout_mode not in ("step", "episode"):
            raise ValueError(f"ma_rollout_mode must be 'step' or 'episode', got "
                             f"{rollout_mode!r}")
        if rollout_mode == "episode":
            # the fused kernel IS the tag game: fail here, not mid-generation
            if not isinstance(env, BatchedPursuitTag):
                raise ValueError(
                    f"ma_rollout_mode='episode' runs the fused PursuitTag kernel "
                    f"(ops/csrc/hip/rollout_tag.hip) and needs a BatchedPursuitTag "
                    f"env, got {type(env).__name__} - use ma_rollout_mode='step'")
            if self.device.type != "cuda" or env.device.type != "cuda":
                raise ValueError(
                    f"ma_rollout_mode='episode' needs the noise table and the env "
                    f"on a GPU, got {self.device.type!r} and {env.device.type!r} - "
                    f"use ma_rollout_mode='step'")
        self.rollout_mode = rollout_mode
        if weights_dtype is None:
            weights_dtype = cfg.general.get("weights_dtype", "bf16")
        if weights_dtype not in ("bf16", "fp32"):
            raise ValueError(f"weights_dtype must be 'bf16' or 'fp32', got "
                             f"{weights_dtype!r}")
        self.weights_dtype = weights_dtype
        self.fp32 = weights_dtype == "fp32"
        if self.fp32 and rollout_mode == "episode" and \
                not hasattr(ops.hip(), "es_tag_episode_f32"):
            raise RuntimeError(
                "weights_dtype='fp32' with ma_rollout_mode='episode' needs "
                "es_tag_episode_f32, which the loaded HIP library does not have "
                "(an earlier revision's library?) - use ma_rollout_mode='step' or "
                "rebuild the library")
        # general.ma_pair_rollout, NOT the single-policy engine's pair_rollout:
        # that key is size-gated and sits in most configs users copy from
        if pair_rollout is None:
            pair_rollout = cfg.general.get("ma_pair_rollout", False)
        if not isinstance(pair_rollout, bool):
            raise ValueError(f"ma_pair_rollout must be true or false, got "
                             f"{pair_rollout!r}")
        if pair_rollout and self.fp32:
            raise ValueError(
                "ma_pair_rollout evaluates bf16(theta) +- bf16(sigma*eps) and has no "
                "fp32 form - use weights_dtype='bf16' or leave ma_pair_rollout off")
        if pair_rollout and rollout_mode != "episode":
            raise ValueError(
                f"ma_pair_rollout shares the rows of an antithetic pair inside the "
                f"fused kernel and needs ma_rollout_mode='episode', got "
                f"{rollout_mode!r} - set ma_rollout_mode='episode' or leave "
                f"ma_pair_rollout off")
        if pair_rollout and not hasattr(ops.hip(), "es_tag_pair_episode"):
            raise RuntimeError(
                "ma_pair_rollout needs es_tag_pair_episode, which the loaded HIP "
                "library does not have (an earlier revision's library?) - leave "
                "ma_pair_rollout off or rebuild the library")
        self.pair_rollout = pair_rollout

        ppg = cfg.general.policies_per_gen
        assert ppg % comm.size == 0 and (ppg / comm.size) % 2 == 0
        self.pairs = int(ppg // comm.size // 2)
        self.B = 2 * self.pairs + 1
        assert env.batch == self.B, f"env batch {env.batch} != {self.B}"

        wdt = torch.float32 if self.fp32 else torch.bfloat16
        self.states = [_PolicyState(p, self.device, self.pairs, env.ob_dims[i], wdt,
                                    pair=self.pair_rollout)
                       for i, p in enumerate(policies)]
        self.actions = [torch.empty((self.B, env.ac_dims[i]), dtype=torch.float32,
                                    device=self.device) for i in range(self.n_agents)]
        self.alive = torch.ones(self.B, dtype=torch.float32, device=self.device)
        self.rew_total = torch.zeros((self.B, self.n_agents), dtype=torch.float32,
                                     device=self.device)
        self.member_steps = torch.zeros(self.B, dtype=torch.float32, device=self.device)
        self.seed_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.max_steps = int(cfg.env.max_steps)
        if rollout_mode == "episode":
            # per-game fp64 observation moments, (game, agent, ob)
            self.ep_ob_sum = torch.zeros((self.B, self.n_agents, env.ob_dims[0]),
                                         dtype=torch.float64, device=self.device)
            self.ep_ob_sumsq = torch.zeros_like(self.ep_ob_sum)
        self.gen = 0
        self.timings = {}

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream if \
            self.device.type == "cuda" else None

    @property
    def numerics(self) -> dict:
        """What the rollout evaluates with (the keys of ``GpuEngine.numerics``)."""
        if self.pair_rollout:
            return {"weights": "bf16", "eps_encoding": "bf16", "path": "tag_pair",
                    "rollout_mode": "episode"}
        return {"weights": self.weights_dtype, "eps_encoding": "none", "path": "tag",
                "rollout_mode": self.rollout_mode}

    def _forward(self, i: int, obs: torch.Tensor, salt: int):
        st = self.states[i]
        fn, name = (ops.hip().es_mlp_fwd_f32, "es_mlp_fwd_f32") if self.fp32 else \
            (ops.hip().es_mlp_fwd, "es_mlp_fwd")
        ops.check(fn(
            self.actions[i].data_ptr(), obs.contiguous().data_ptr(),
            st.weights.data_ptr(), st.obmean.data_ptr(), st.obstd.data_ptr(),
            st.dims_arr.ctypes.data, len(st.dims_arr), self.seed_dev.data_ptr(),
            salt * self.n_agents + i, self.B,
            float(st.policy._module.ob_clip), st.acstd_dev.data_ptr(),
            st.row_stride, 1, self.B - 1, 0, 1, 0, None, None,
            self._stream()), name)
        return self.actions[i]

    def _rollout_episode(self):
        """The whole rollout in one launch, on the env's own p/v tensors."""
        s0, s1 = self.states
        env = self.env
        assert env.p.is_contiguous() and env.v.is_contiguous()
        self.ep_ob_sum.zero_()
        self.ep_ob_sumsq.zero_()
        if self.pair_rollout:
            ops.check(ops.hip().es_tag_pair_episode(
                env.p.data_ptr(), env.v.data_ptr(), self.alive.data_ptr(),
                self.member_steps.data_ptr(), self.rew_total.data_ptr(),
                self.ep_ob_sum.data_ptr(), self.ep_ob_sumsq.data_ptr(),
                s0.theta_row.data_ptr(), s1.theta_row.data_ptr(),
                s0.eps_rows.data_ptr(), s1.eps_rows.data_ptr(), s0.obmean.data_ptr(),
                s1.obmean.data_ptr(), s0.obstd.data_ptr(), s1.obstd.data_ptr(),
                s0.dims_arr.ctypes.data, len(s0.dims_arr), s1.dims_arr.ctypes.data,
                len(s1.dims_arr), s0.row_stride, s1.row_stride,
                float(s0.policy._module.ob_clip), float(s1.policy._module.ob_clip),
                s0.acstd_dev.data_ptr(), s1.acstd_dev.data_ptr(),
                self.seed_dev.data_ptr(), 0, self.n_agents, env.ob_dims[0], self.pairs, 1,
                self.max_steps, 1, self.B - 1, self._stream()), "es_tag_pair_episode")
            return self._episode_sums()
        fn, name = (ops.hip().es_tag_episode_f32, "es_tag_episode_f32") if self.fp32 \
            else (ops.hip().es_tag_episode, "es_tag_episode")
        ops.check(fn(
            env.p.data_ptr(), env.v.data_ptr(), self.alive.data_ptr(),
            self.member_steps.data_ptr(), self.rew_total.data_ptr(),
            self.ep_ob_sum.data_ptr(), self.ep_ob_sumsq.data_ptr(),
            s0.weights.data_ptr(), s1.weights.data_ptr(), s0.obmean.data_ptr(),
            s1.obmean.data_ptr(), s0.obstd.data_ptr(), s1.obstd.data_ptr(),
            s0.dims_arr.ctypes.data, len(s0.dims_arr), s1.dims_arr.ctypes.data,
            len(s1.dims_arr), s0.row_stride, s1.row_stride,
            float(s0.policy._module.ob_clip), float(s1.policy._module.ob_clip),
            s0.acstd_dev.data_ptr(), s1.acstd_dev.data_ptr(), self.seed_dev.data_ptr(),
            0, self.n_agents, env.ob_dims[0], self.B, self.max_steps, 1, self.B - 1,
            self._stream()), name)
        return self._episode_sums()

    def _episode_sums(self):
        ob_sums = [self.ep_ob_sum[:, i].sum(0) for i in range(self.n_agents)]
        ob_sumsqs = [self.ep_ob_sumsq[:, i].sum(0) for i in range(self.n_agents)]
        return ob_sums, ob_sumsqs, self.member_steps.sum().double()

    def _pheno_pair(self, st: _PolicyState):
        """GpuEngine._pheno's pair form: sign 0 gives the bf16(theta) row, zero
        theta and sign +1 the bf16(sigma*noise[off_p:]) rows."""
        fn = ops.hip().es_pheno_bf16
        ops.check(fn(
            st.theta_row.data_ptr(), st.theta.data_ptr(), self.nt.noise.data_ptr(),
            st._zero_off.data_ptr(), st._zero_sign.data_ptr(), 1, st.n, st.row_stride,
            0.0, self._stream()), "es_pheno_bf16")
        ops.check(fn(
            st.eps_rows.data_ptr(), st._zeros_n.data_ptr(), self.nt.noise.data_ptr(),
            st.offsets.data_ptr(), st._one_signs.data_ptr(), self.pairs, st.n,
            st.row_stride, float(st.policy.std), self._stream()), "es_pheno_bf16")

    def step(self, rankers: List[Ranker]) -> Tuple[List[float], List[ObStat]]:
        """One co-evolution generation; every policy updated from its own
        fitness column. :returns: (noiseless rewards per agent, obstats)."""
        t0 = time.perf_counter()
        for i, st in enumerate(self.states):
            offs = self.nt.sample_idxs(self.rs, self.pairs)  # one draw per policy
            st.offsets[:self.pairs].copy_(torch.from_numpy(offs).to(self.device))
            st.offsets[self.pairs:2 * self.pairs].copy_(st.offsets[:self.pairs])
            st.acstd_dev.fill_(float(getattr(st.policy._module, "_action_std", 0.0)))
            if self.pair_rollout:
                self._pheno_pair(st)
                continue
            fn, name = (ops.hip().es_pheno_f32, "es_pheno_f32") if self.fp32 else \
                (ops.hip().es_pheno_bf16, "es_pheno_bf16")
            ops.check(fn(
                st.weights.data_ptr(), st.theta.data_ptr(), self.nt.noise.data_ptr(),
                st.offsets.data_ptr(), st.signs.data_ptr(), self.B, st.n,
                st.row_stride, float(st.policy.std), self._stream()), name)
        self.seed_dev.fill_(int(self.rs.randint(0, 2 ** 31)))

        self.alive.fill_(1.0)
        self.rew_total.zero_()
        self.member_steps.zero_()
        obs = self.env.reset((self.gen * 1000003 + self.comm.rank * 7919) & 0x7FFFFFFF)
        ob_sums = [torch.zeros(self.env.ob_dims[i], dtype=torch.float64,
                               device=self.device) for i in range(self.n_agents)]
        ob_sumsqs = [torch.zeros_like(s) for s in ob_sums]
        ob_count = torch.zeros((), dtype=torch.float64, device=self.device)

        if self.rollout_mode == "episode":
            ob_sums, ob_sumsqs, ob_count = self._rollout_episode()
        else:
            for t in range(self.max_steps):
                acts = [self._forward(i, obs[i], t + 1) for i in range(self.n_agents)]
                obs, rews, done = self.env.step(acts)
                self.rew_total.add_(rews * self.alive.unsqueeze(1))
                self.member_steps.add_(self.alive)
                w = self.alive.unsqueeze(1)
                for i in range(self.n_agents):
                    ob_sums[i].add_((obs[i] * w).sum(0).double())
                    ob_sumsqs[i].add_((obs[i] * obs[i] * w).sum(0).double())
                ob_count.add_(self.alive.sum().double())
                self.alive.mul_(1.0 - done.float())

        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()

        # per-policy: share triples, rank, reconstruct gradient, update
        noiseless = []
        obstats = []
        for i, st in enumerate(self.states):
            fits = self.rew_total[:, i]
            rows = torch.empty((self.pairs, 3), dtype=torch.float64, device=self.device)
            rows[:, 0] = fits[:self.pairs].double()
            rows[:, 1] = fits[self.pairs:2 * self.pairs].double()
            rows[:, 2] = st.offsets[:self.pairs].double()
            all_rows = self.comm.allgather_rows(rows).cpu().numpy()
            rankers[i].rank(all_rows[:, :1], all_rows[:, 1:2], all_rows[:, 2])
            rf = torch.from_numpy(np.ascontiguousarray(
                rankers[i].ranked_fits, dtype=np.float32)).to(self.device)
            ri = torch.from_numpy(np.ascontiguousarray(
                rankers[i].noise_inds, dtype=np.int64)).to(self.device)
            ops.check(ops.hip().es_grad_gather(
                st.grad.data_ptr(), self.nt.noise.data_ptr(), rf.data_ptr(),
                ri.data_ptr(), rf.numel(), st.n, 0.0, self._stream()), "es_grad_gather")
            opt = st.policy.optim
            assert isinstance(opt, Adam)
            opt.t += 1
            a = opt.lr * np.sqrt(1 - opt.beta2 ** opt.t) / (1 - opt.beta1 ** opt.t)
            ops.check(ops.hip().es_adam_step(
                st.theta.data_ptr(), st.m.data_ptr(), st.v.data_ptr(),
                st.grad.data_ptr(), st.n, float(a), float(opt.beta1), float(opt.beta2),
                float(opt.epsilon), float(self.cfg.policy.l2coeff),
                1.0 / rankers[i].n_fits_ranked, self._stream()), "es_adam_step")
            st.sync_host()

            ob = ObStat((self.env.ob_dims[i],), 0)
            ob.inc(ob_sums[i].cpu().numpy(), ob_sumsqs[i].cpu().numpy(),
                   float(ob_count.item()))
            ob.dist_inc(self.comm)
            obstats.append(ob)
            noiseless.append(float(fits[-1].item()))

        self.gen += 1
        self.timings = {"rollout_s": t1 - t0, "gen_s": time.perf_counter() - t0,
                        "env_steps": float(self.member_steps[:2 * self.pairs].sum().item())
                        * self.n_agents}
        return noiseless, obstats

    def update_obstats(self, obstats: List[ObStat]):
        for st, ob in zip(self.states, obstats):
            st.policy.update_obstat(ob)
            st.push_obstat()
