"""Float64 numpy oracle for the whole-episode tag rollout (es_tag_episode).

Written out from the documented semantics, like tests/oracle64.py whose
forward and Philox noise it builds on: the game is
``envs/multiagent.py::BatchedPursuitTag`` (pinned to it on the CPU by
tests/test_oracle64_tag_cpu.py), the bookkeeping is the step loop of
``MultiAgentGpuEngine.step`` for a game that is still alive.

Per step, for every game that is alive:
  agent i = 0, 1 sees (own p, own v, other p, other v) of the PRE-step state,
  its policy (member row b of its own blob) gives a raw action, plus
  ac_std_i * z when ac_std_i != 0 and b < noiseless_from, z drawn with key
  seed + (salt_base + t + 1) * 2 + i at counter b * odim_i + o;
  v_i = 0.8 v_i + clamp(a_i[:2], +-1) * 0.1 * 5,  p = clamp(p + 0.1 v, +-5);
  d = |p_0 - p_1|, caught = d < 0.3, rewards (-d + bonus, d - bonus) with
  bonus 10 when caught; rew_total += r, steps += 1, the observation moments
  take both agents' POST-step observations (the terminal one too), then
  alive = not caught. A game that is not alive does not change.

The scalar constants are float32 values, as the kernel and the env have them.
The observation moments are float64 sums of the `dtype` observations whatever
`dtype` is: that is what the kernel and the engine accumulate in.
"""
import numpy as np

from tests.oracle64 import policy_actions

ARENA = 5.0
CATCH = 0.3
TAG_KEYS = ("p", "v", "alive", "steps", "rew_total", "ob_sum", "ob_sumsq")


def tag_state(p, v=None):
    """Fresh state for start positions p (B, 2, 2): all alive, totals zero."""
    p = np.asarray(p, dtype=np.float32)
    B = p.shape[0]
    return {"p": p.copy(),
            "v": np.zeros_like(p) if v is None else np.asarray(v, np.float32).copy(),
            "alive": np.ones(B, np.float32), "steps": np.zeros(B, np.float32),
            "rew_total": np.zeros((B, 2), np.float32),
            "ob_sum": np.zeros((B, 2, 8), np.float64),
            "ob_sumsq": np.zeros((B, 2, 8), np.float64)}


def tag_obs(p, v):
    """[obs of agent 0, obs of agent 1], each (B, 8)."""
    return [np.concatenate([p[:, i], v[:, i], p[:, 1 - i], v[:, 1 - i]], axis=1)
            for i in range(2)]


def tag_rollout(state, nets, n_steps, dtype=np.float64, noise=None):
    """n_steps of the tag game from `state` (not modified).

    state: dict of TAG_KEYS, (B, ...) arrays (see tag_state).
    nets: two dicts of policy_actions keywords (dims, weight_rows, obmean,
    obstd, ob_clip, optionally act_final); game b uses weight row b of each.
    noise: None or a dict of seed (None: no seed_dev), ac_std (one value per
    agent), noiseless_from and optionally salt_base (default 0).
    Returns (state, info). info: margin (B,), the smallest |d - 0.3| seen
    while the game was alive (inf if it never stepped); catch_step (B,), the
    1-based step of this call at which the game ended, 0 if it did not;
    actions (n_steps, B, 2, 2), the raw actions [t, b, agent], 0 where the
    game was not alive.
    """
    f = lambda x: dtype(np.float32(x))
    p = np.asarray(state["p"]).astype(dtype)
    v = np.asarray(state["v"]).astype(dtype)
    alive = np.asarray(state["alive"]).astype(np.float64) > 0
    steps = np.asarray(state["steps"]).astype(np.float64)
    rew = np.asarray(state["rew_total"]).astype(dtype)
    ob_sum = np.asarray(state["ob_sum"]).astype(np.float64)
    ob_sumsq = np.asarray(state["ob_sumsq"]).astype(np.float64)
    B = p.shape[0]
    margin = np.full(B, np.inf)
    catch_step = np.zeros(B, np.int64)
    actions = np.zeros((n_steps, B, 2, 2), dtype=dtype)
    salt_base = 0 if noise is None else int(noise.get("salt_base", 0))

    for t in range(n_steps):
        if not alive.any():
            break
        obs = tag_obs(p, v)
        act = []
        for i in range(2):
            nz = None
            if noise is not None:
                nz = dict(seed=noise["seed"], salt=(salt_base + t + 1) * 2 + i,
                          ac_std=noise["ac_std"][i],
                          noiseless_from=noise["noiseless_from"])
            a, _ = policy_actions(obs=obs[i], dtype=dtype, noise=nz, **nets[i])
            act.append(a[:, :2])
        a = np.stack(act, axis=1)                                   # (B, agent, 2)
        actions[t] = np.where(alive[:, None, None], a, dtype(0.0))
        a = np.minimum(np.maximum(a, dtype(-1.0)), dtype(1.0))
        vn = f(0.8) * v + a * f(0.1) * f(5.0)
        pn = np.minimum(np.maximum(p + vn * f(0.1), -f(ARENA)), f(ARENA))
        dx = pn[:, 0, 0] - pn[:, 1, 0]
        dy = pn[:, 0, 1] - pn[:, 1, 1]
        d = np.sqrt(dx * dx + dy * dy)
        caught = d < f(CATCH)
        bonus = np.where(caught, f(10.0), dtype(0.0))
        r = np.stack([-d + bonus, d - bonus], axis=1)

        live = alive
        p = np.where(live[:, None, None], pn, p)
        v = np.where(live[:, None, None], vn, v)
        rew = np.where(live[:, None], rew + r, rew)
        steps = steps + live
        ob = np.stack(tag_obs(p, v), axis=1).astype(np.float64)     # (B, agent, 8)
        ob_sum = np.where(live[:, None, None], ob_sum + ob, ob_sum)
        ob_sumsq = np.where(live[:, None, None], ob_sumsq + ob * ob, ob_sumsq)
        m = np.abs(d.astype(np.float64) - float(np.float32(CATCH)))
        margin = np.where(live, np.minimum(margin, m), margin)
        catch_step = np.where(live & caught, t + 1, catch_step)
        alive = live & ~caught

    out = {"p": p, "v": v, "alive": alive.astype(np.float64), "steps": steps,
           "rew_total": rew, "ob_sum": ob_sum, "ob_sumsq": ob_sumsq}
    return out, {"margin": margin, "catch_step": catch_step, "actions": actions}
