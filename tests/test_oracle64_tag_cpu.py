"""Pins tests/oracle64_tag.py to the env that defines the game.

The oracle is run in float32 and ``BatchedPursuitTag`` is driven on the CPU
with the oracle's own actions, under the bookkeeping of
``MultiAgentGpuEngine.step``'s loop (alive mask, terminal observation
counted). Both sides then do the same float32 operations in the same order:
positions and velocities must agree to a few ulp, and so must the rewards,
whose only freedom is how the 2-norm is rounded (torch's norm against
sqrt(dx*dx + dy*dy)).
"""
import numpy as np
import pytest
import torch

from es_pytorch_amd.envs.multiagent import BatchedPursuitTag
from tests.oracle64_tag import TAG_KEYS, tag_rollout, tag_state
from tests.test_kernel_oracle_tag import MARGIN_MIN, NOISE, build_case

EPS32 = 2.0 ** -23
ULPS = 4.0


def drive_env(c, actions):
    """The engine's step loop on the CPU env, fed `actions` (T, B, 2, 2);
    totals are kept per game."""
    B, n = c["B"], c["n_steps"]
    env = BatchedPursuitTag(B, "cpu", max_steps=10 ** 6)
    env.p.copy_(torch.from_numpy(c["state"]["p"]))
    env.v.copy_(torch.from_numpy(c["state"]["v"]))
    alive = torch.ones(B)
    rew_total = torch.zeros(B, 2)
    member_steps = torch.zeros(B)
    ob_sum = torch.zeros(B, 2, 8, dtype=torch.float64)
    ob_sumsq = torch.zeros(B, 2, 8, dtype=torch.float64)
    p_end, v_end = env.p.clone(), env.v.clone()
    catch_step = torch.zeros(B, dtype=torch.int64)
    for t in range(n):
        acts = [torch.from_numpy(np.ascontiguousarray(actions[t, :, i])) for i in range(2)]
        obs, rews, done = env.step(acts)
        live = alive > 0
        rew_total.add_(rews * alive.unsqueeze(1))
        member_steps.add_(alive)
        w = alive.unsqueeze(1)
        for i in range(2):
            ob_sum[:, i].add_((obs[i] * w).double())
            ob_sumsq[:, i].add_((obs[i] * obs[i] * w).double())
        p_end[live] = env.p[live]
        v_end[live] = env.v[live]
        catch_step[live & done] = t + 1
        alive.mul_(1.0 - done.float())
    return {"p": p_end.numpy(), "v": v_end.numpy(), "alive": alive.numpy(),
            "steps": member_steps.numpy(), "rew_total": rew_total.numpy(),
            "ob_sum": ob_sum.numpy(), "ob_sumsq": ob_sumsq.numpy(),
            "catch_step": catch_step.numpy()}


def close(a, b, scale):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() <= \
        ULPS * EPS32 * scale


@pytest.mark.parametrize("name,noise", [("base", None), ("base", NOISE),
                                        ("asymmetric", None)])
def test_oracle_f32_plays_the_env(name, noise):
    c = build_case(name)
    y32, info = tag_rollout(c["state"], c["nets"], c["n_steps"], dtype=np.float32,
                            noise=noise)
    assert y32["p"].dtype == np.float32 and info["actions"].dtype == np.float32
    env = drive_env(c, info["actions"])
    assert np.array_equal(env["steps"], y32["steps"])
    assert np.array_equal(env["catch_step"], info["catch_step"])
    assert np.array_equal(env["alive"], y32["alive"])
    assert (info["catch_step"] > 0).any() and (info["catch_step"] == 0).any()
    assert close(env["p"], y32["p"], 5.0)            # |p| <= ARENA
    assert close(env["v"], y32["v"], 2.5)            # |v| <= 0.5 / (1 - 0.8)
    # a few ulp of the largest total: a step's d may round an ulp apart, and
    # the running float32 sum then rounds at the total's magnitude
    assert close(env["rew_total"], y32["rew_total"], np.abs(y32["rew_total"]).max())
    # moments: the same float32 observations summed in float64; the env side
    # squares in float32, a relative 2^-24 per (positive) term
    for k in ("ob_sum", "ob_sumsq"):
        assert close(env[k], y32[k], max(1.0, np.abs(y32[k]).max()))


def test_oracle_catch_margin_and_freeze():
    """margin is the closest the live game came to the threshold; an ended
    game is frozen, so a rollout cut in two gives the same float64 state."""
    c = build_case("base")
    n = c["n_steps"]
    y, info = tag_rollout(c["state"], c["nets"], n)
    assert (info["margin"] >= MARGIN_MIN).all() and np.isfinite(info["margin"]).all()
    cs = info["catch_step"]
    assert np.array_equal(y["steps"], np.where(cs > 0, cs, n))
    assert np.array_equal(y["alive"], (cs == 0).astype(np.float64))
    d = np.linalg.norm(y["p"][:, 0] - y["p"][:, 1], axis=1)
    assert ((d < 0.3) == (cs > 0)).all()
    # the game that ends at step 1 took one reward, -d + 10 and d - 10
    b = int(np.nonzero(cs == 1)[0][0])
    assert abs(y["rew_total"][b, 0] - (10.0 - d[b])) < 1e-12
    assert abs(y["rew_total"][b, 0] + y["rew_total"][b, 1]) < 1e-12
    mid, _ = tag_rollout(c["state"], c["nets"], 5, noise=dict(NOISE, salt_base=0))
    two, _ = tag_rollout(mid, c["nets"], n - 5, noise=dict(NOISE, salt_base=5))
    one, _ = tag_rollout(c["state"], c["nets"], n, noise=NOISE)
    for k in TAG_KEYS:
        assert np.array_equal(one[k], two[k]), k


def test_oracle_noise_is_per_agent_and_per_slot():
    """Slots >= noiseless_from draw nothing; an agent with ac_std 0 draws
    nothing either."""
    c = build_case("base")
    off, _ = tag_rollout(c["state"], c["nets"], 1)
    on, _ = tag_rollout(c["state"], c["nets"], 1, noise=NOISE)
    k = NOISE["noiseless_from"]
    assert np.array_equal(on["v"][k:], off["v"][k:])
    assert (on["v"][:k] != off["v"][:k]).any()
    half, _ = tag_rollout(c["state"], c["nets"], 1, noise=dict(NOISE, ac_std=(0.0, 0.05)))
    assert np.array_equal(half["v"][:, 0], off["v"][:, 0])
    assert (half["v"][:k, 1] != off["v"][:k, 1]).any()
    assert set(tag_state(c["state"]["p"])) == set(TAG_KEYS)
