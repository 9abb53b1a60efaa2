"""Pins tests/oracle64_classic.py to the envs that define the games.

The oracle is run in float32 and ``BatchedCartPole`` / ``BatchedPendulum`` are
driven on the CPU with the oracle's own actions, under the bookkeeping of
``GpuEngine._step_body`` (alive mask, terminal observation counted), kept per
slot. Both sides then do the same float32 operations in the same order: end
steps and alive flags must agree exactly, and state, rewards and moments to a
few ulp of their magnitude. Their only freedom is how ``sin``, ``cos`` and
``atan2`` round, numpy's float32 routines against torch's, which may land an
ulp apart; the dynamics carry such a difference forward.

Measured here (the ENV-SLACK figures the test prints, in ulp of each buffer's
largest magnitude): the largest over all cases is 0.77 ulp (ob_sum of
cartpole_base), then 0.61 (Pendulum rew_total), 0.59 (thdot) and 0.50 (th);
CartPole's state stays within 0.19 ulp. The bound is ULPS = 4, five times the
largest figure, the same few ulp tests/test_oracle64_tag_cpu.py allows.

The CPU test of the engine's constructor check and the input conditions of
the GPU cases (tests/test_kernel_oracle_classic.py) live here too: neither
needs a GPU.
"""
import numpy as np
import pytest
import torch

from es_pytorch_amd.envs.classic import BatchedCartPole, BatchedPendulum
from tests.oracle64_classic import CARTPOLE_KEYS, PENDULUM_KEYS, cartpole_state
from tests.test_kernel_oracle_classic import (ALL_CASES, CASES, MARGIN_MIN, build_case,
                                              case_id, case_noise, float_keys, oracle,
                                              rollout_fn, state_keys)

EPS32 = 2.0 ** -23
ULPS = 4.0


def drive_env(c, actions):
    """_step_body's loop on the CPU env, fed `actions` (T, B); totals and
    moments are kept per slot, and so is the state of a slot's last live
    step (the env itself goes on stepping a slot that is done)."""
    B, n, kind = c["B"], c["n_steps"], c["kind"]
    if kind == "cartpole":
        env = BatchedCartPole(B, "cpu")
        env.state.copy_(torch.from_numpy(c["state"]["state"]))
        D = 4
    else:
        env = BatchedPendulum(B, "cpu")
        env.th.copy_(torch.from_numpy(c["state"]["th"]))
        env.thdot.copy_(torch.from_numpy(c["state"]["thdot"]))
        D = 3
    env._steps.copy_(torch.from_numpy(c["state"]["env_steps"]))
    alive = torch.ones(B)
    rew_total = torch.zeros(B)
    member_steps = torch.zeros(B)
    ob_sum = torch.zeros(B, D, dtype=torch.float64)
    ob_sumsq = torch.zeros(B, D, dtype=torch.float64)
    held = {k: torch.from_numpy(c["state"][k]).clone()
            for k in (("state",) if kind == "cartpole" else ("th", "thdot"))}
    held["env_steps"] = env._steps.clone()
    end_step = torch.zeros(B, dtype=torch.int64)
    for t in range(n):
        a = torch.from_numpy(np.ascontiguousarray(actions[t])).unsqueeze(1)
        ob, rew, done = env.step(a)
        live = alive > 0
        rew_total.add_(rew * alive)
        member_steps.add_(alive)
        w = alive.unsqueeze(1)
        ob_sum.add_((ob * w).double())
        ob_sumsq.add_((ob * ob * w).double())
        for k in held:
            src = env._steps if k == "env_steps" else getattr(env, k)
            held[k][live] = src[live]
        end_step[live & done] = t + 1
        alive.mul_(1.0 - done.float())
    out = {k: v.numpy() for k, v in held.items()}
    out.update(alive=alive.numpy(), member_steps=member_steps.numpy(),
               rew_total=rew_total.numpy(), ob_sum=ob_sum.numpy(),
               ob_sumsq=ob_sumsq.numpy(), end_step=end_step.numpy())
    return out


def ulps(a, b, scale):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) / \
        (EPS32 * scale)


@pytest.mark.parametrize("name,noise_on", [("cartpole_base", False),
                                           ("cartpole_base", True),
                                           ("cartpole_eps2", False),
                                           ("pendulum_base", False),
                                           ("pendulum_base", True),
                                           ("pendulum_time_limit", False)])
def test_oracle_f32_plays_the_env(name, noise_on):
    c = build_case(name)
    noise = case_noise(c) if noise_on else None
    y32, info = rollout_fn(c["kind"])(c["state"], c["net"], c["n_steps"],
                                      dtype=np.float32, noise=noise)
    assert y32["rew_total"].dtype == np.float32 and info["actions"].dtype == np.float32
    env = drive_env(c, info["actions"])
    assert np.array_equal(env["member_steps"], y32["member_steps"])
    assert np.array_equal(env["env_steps"], y32["env_steps"])
    assert np.array_equal(env["end_step"], info["end_step"])
    assert np.array_equal(env["alive"], y32["alive"])
    if name != "pendulum_base":
        assert (info["end_step"] > 0).any() and (info["end_step"] == 0).any()
    for k in float_keys(c["kind"]):
        # a few ulp of the buffer's largest value: the running sums round at
        # the total's magnitude, the env side squares in float32 (a relative
        # 2^-24 per positive term)
        u = ulps(env[k], y32[k], max(1.0, float(np.abs(y32[k]).max())))
        print(f"ENV-SLACK {name} noise={noise_on} {k} {u:.2f} ulp")
        assert u <= ULPS, (k, u)


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
@pytest.mark.parametrize("noise_on", [False, True], ids=["noise_off", "noise_on"])
def test_gpu_cases_meet_their_input_conditions(case, noise_on):
    """No GPU: no slot on a decision's rounding edge and float32 plays the
    float64 game (asserted inside oracle()), for every case the GPU tests run."""
    name, f32 = case
    y64, e32, info = oracle(name, f32, noise_on)
    for m in info["margins"].values():
        assert np.isfinite(m).all() and (m >= MARGIN_MIN).all()
    for k in float_keys(CASES[name][0]):
        assert e32[k] > 0 and np.isfinite(y64[k]).all()


def test_oracle_endings_and_freeze():
    """An ended slot is frozen, so a rollout cut in two gives the same float64
    state; end_step, member_steps and alive tell one story."""
    for name in ("cartpole_base", "pendulum_time_limit"):
        c = build_case(name)
        fn, n = rollout_fn(c["kind"]), c["n_steps"]
        y, info = fn(c["state"], c["net"], n)
        es = info["end_step"]
        assert np.array_equal(y["member_steps"], np.where(es > 0, es, n))
        assert np.array_equal(y["alive"], (es == 0).astype(np.float64))
        assert np.array_equal(y["env_steps"], c["state"]["env_steps"] + y["member_steps"])
        if c["kind"] == "cartpole":
            assert np.array_equal(y["rew_total"], y["member_steps"])
            out = (np.abs(y["state"][:, 0]) > 2.4) | (np.abs(y["state"][:, 2]) > 0.2094395)
            assert np.array_equal(out | (y["env_steps"] >= 500), es > 0)
        noise = case_noise(c)
        mid, _ = fn(c["state"], c["net"], 5, noise=dict(noise, salt_base=0))
        two, _ = fn(mid, c["net"], n - 5, noise=dict(noise, salt_base=5))
        one, _ = fn(c["state"], c["net"], n, noise=noise)
        for k in state_keys(c["kind"]):
            assert np.array_equal(one[k], two[k]), (name, k)


def test_oracle_noise_is_per_slot():
    """Slots >= noiseless_from draw nothing; ac_std 0 draws nothing."""
    c = build_case("pendulum_base")
    fn = rollout_fn("pendulum")
    off, _ = fn(c["state"], c["net"], 1)
    noise = dict(case_noise(c), noiseless_from=6)
    on, _ = fn(c["state"], c["net"], 1, noise=noise)
    assert np.array_equal(on["thdot"][6:], off["thdot"][6:])
    assert (on["thdot"][:6] != off["thdot"][:6]).all()
    zero, _ = fn(c["state"], c["net"], 1, noise=dict(noise, ac_std=0.0))
    assert np.array_equal(zero["thdot"], off["thdot"])
    other, _ = fn(c["state"], c["net"], 1, noise=dict(noise, salt_base=1))
    assert (other["thdot"][:6] != on["thdot"][:6]).all()
    assert set(cartpole_state(np.zeros((2, 4)))) == set(CARTPOLE_KEYS)
    assert set(c["state"]) == set(PENDULUM_KEYS)


def test_classic_fused_on_cpu_is_rejected_at_construction():
    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.engine import GpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs import make_batched
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import Comm

    def setup(general=None):
        comm = Comm(torch.device("cpu"))
        cfg = AttrDict({"env": {"name": "CartPole-v1", "max_steps": 8},
                        "noise": {"tbl_size": 10000, "std": 0.02},
                        "policy": {"layer_sizes": [16], "ac_std": 0.0, "l2coeff": 0.005,
                                   "lr": 0.01, "ob_clip": 5},
                        "general": dict({"name": "t", "policies_per_gen": 4,
                                         "batch_size": 100}, **(general or {}))})
        env = make_batched("CartPole-v1", 5, torch.device("cpu"))
        nn = FeedForward([16], torch.nn.Tanh(), env, 0.0, 5)
        policy = Policy(nn, 0.02, Adam(len(Policy.get_flat(nn)), 0.01))
        nt = NoiseTable.create_shared(comm, 10000, len(policy), seed=1)
        return cfg, comm, policy, nt, env, np.random.RandomState(0)

    with pytest.raises(ValueError, match="GPU"):
        GpuEngine(*setup(), use_graph=False, classic_fused=True)
    with pytest.raises(ValueError, match="GPU"):
        GpuEngine(*setup({"classic_fused": True}), use_graph=False)
    # off by default, and the argument overrides the config
    eng = GpuEngine(*setup(), use_graph=False)
    assert not eng.classic_fused and eng.numerics["path"] == "generic"
    eng = GpuEngine(*setup({"classic_fused": True}), use_graph=False, classic_fused=False)
    assert not eng.classic_fused and eng.numerics["path"] == "generic"
