"""Float64 numpy oracle for the whole-episode classic-control rollout
(es_classic_episode, es_classic_episode_f32).

Written out from the documented semantics, like tests/oracle64.py whose
forward and Philox noise it builds on: the envs are
``envs/classic.py::BatchedCartPole`` and ``BatchedPendulum`` (pinned to them
on the CPU by tests/test_oracle64_classic_cpu.py), the bookkeeping is
``GpuEngine._step_body`` for a slot that is still alive.

Per step, for every slot b that is alive:
  the observation of the PRE-step state (CartPole: x, x_dot, theta, theta_dot;
  Pendulum: cos th, sin th, thdot) goes through the policy on weight row
  b // eps; output 0 is the raw action a, plus ac_std * z when ac_std != 0 and
  b < noiseless_from, z drawn with key seed + salt_base + t + 1 at counter
  b * odim;
  CartPole: force = +-10 by a > 0, then
    temp     = (force + pml * theta_dot^2 * sin) / total_mass
    thetaacc = (g sin - cos temp) / (l (4/3 - mp cos^2 / total_mass))
    xacc     = temp - pml thetaacc cos / total_mass
    x += tau x_dot, x_dot += tau xacc, theta += tau theta_dot,
    theta_dot += tau thetaacc (all from the old values), reward 1,
    done = |x| > 2.4 or |theta| > 12 deg or env_steps >= max_env_steps;
  Pendulum: u = clamp(a, +-2), cost = atan2(sin th, cos th)^2 + 0.1 thdot^2 +
    0.001 u^2 of the pre-step state, thdot = clamp(thdot + (15 sin th + 3 u)
    * 0.05, +-8), th += thdot * 0.05, reward -cost,
    done = env_steps >= max_env_steps;
  rew_total += r, member_steps += 1, env_steps += 1, the observation moments
  take the POST-step observation (the terminal one too), then alive = not
  done. A slot that is not alive does not change.

The scalar constants are the float32 values of the Python doubles the envs
hold. The observation moments are float64 sums of the `dtype` observations
whatever `dtype` is: that is what the kernel accumulates in.
"""
import math

import numpy as np

from tests.oracle64 import policy_actions

CP_MAX_STEPS = 500
PD_MAX_STEPS = 200
X_THRESHOLD = 2.4
THETA_THRESHOLD = 12 * 2 * math.pi / 360
COMMON_KEYS = ("env_steps", "alive", "member_steps", "rew_total", "ob_sum", "ob_sumsq")
CARTPOLE_KEYS = ("state",) + COMMON_KEYS
PENDULUM_KEYS = ("th", "thdot") + COMMON_KEYS


def _totals(B, D):
    return {"env_steps": np.zeros(B, np.float32), "alive": np.ones(B, np.float32),
            "member_steps": np.zeros(B, np.float32), "rew_total": np.zeros(B, np.float32),
            "ob_sum": np.zeros((B, D), np.float64), "ob_sumsq": np.zeros((B, D), np.float64)}


def cartpole_state(state, env_steps=None):
    """Fresh state for starts (B, 4): all alive, totals zero."""
    s = np.asarray(state, dtype=np.float32)
    out = dict(state=s.copy(), **_totals(s.shape[0], 4))
    if env_steps is not None:
        out["env_steps"] = np.asarray(env_steps, np.float32).copy()
    return out


def pendulum_state(th, thdot, env_steps=None):
    th = np.asarray(th, dtype=np.float32)
    out = dict(th=th.copy(), thdot=np.asarray(thdot, np.float32).copy(),
               **_totals(th.shape[0], 3))
    if env_steps is not None:
        out["env_steps"] = np.asarray(env_steps, np.float32).copy()
    return out


def _rollout(kind, state, net, n_steps, dtype, noise, max_env_steps):
    f = lambda x: dtype(np.float32(x))
    cart = kind == "cartpole"
    if cart:
        s = np.asarray(state["state"]).astype(dtype)
        x, x_dot, theta, theta_dot = (s[:, k].copy() for k in range(4))
    else:
        th = np.asarray(state["th"]).astype(dtype)
        thdot = np.asarray(state["thdot"]).astype(dtype)
    alive = np.asarray(state["alive"]).astype(np.float64) > 0
    env_steps = np.asarray(state["env_steps"]).astype(np.float64)
    msteps = np.asarray(state["member_steps"]).astype(np.float64)
    rew = np.asarray(state["rew_total"]).astype(dtype)
    ob_sum = np.asarray(state["ob_sum"]).astype(np.float64)
    ob_sumsq = np.asarray(state["ob_sumsq"]).astype(np.float64)
    B = alive.shape[0]
    end_step = np.zeros(B, np.int64)
    actions = np.zeros((n_steps, B), dtype=dtype)
    margins = {k: np.full(B, np.inf) for k in (("a", "x", "theta") if cart else ())}
    salt_base = 0 if noise is None else int(noise.get("salt_base", 0))

    def obs():
        if cart:
            return np.stack([x, x_dot, theta, theta_dot], axis=1)
        return np.stack([np.cos(th), np.sin(th), thdot], axis=1)

    for t in range(n_steps):
        if not alive.any():
            break
        nz = None
        if noise is not None:
            nz = dict(seed=noise["seed"], salt=salt_base + t + 1, ac_std=noise["ac_std"],
                      noiseless_from=noise["noiseless_from"])
        ob = obs()
        a, _ = policy_actions(obs=ob, dtype=dtype, noise=nz, **net)
        a = a[:, 0]
        actions[t] = np.where(alive, a, dtype(0.0))
        live = alive
        if cart:
            force = np.where(a > 0, f(10.0), -f(10.0))
            cos, sin = np.cos(theta), np.sin(theta)
            pml, tm = f(0.1 * 0.5), f(0.1 + 1.0)
            temp = (force + pml * (theta_dot * theta_dot) * sin) / tm
            thetaacc = (f(9.8) * sin - cos * temp) / \
                (f(0.5) * (f(4.0 / 3.0) - f(0.1) * (cos * cos) / tm))
            xacc = temp - pml * thetaacc * cos / tm
            tau = f(0.02)
            xn = x + tau * x_dot
            x_dotn = x_dot + tau * xacc
            thetan = theta + tau * theta_dot
            theta_dotn = theta_dot + tau * thetaacc
            x = np.where(live, xn, x)
            x_dot = np.where(live, x_dotn, x_dot)
            theta = np.where(live, thetan, theta)
            theta_dot = np.where(live, theta_dotn, theta_dot)
            r = np.ones(B, dtype=dtype)
            done = (np.abs(xn) > f(X_THRESHOLD)) | (np.abs(thetan) > f(THETA_THRESHOLD))
            for k, v in (("a", np.abs(a)),
                         ("x", np.abs(np.abs(xn) - f(X_THRESHOLD))),
                         ("theta", np.abs(np.abs(thetan) - f(THETA_THRESHOLD)))):
                margins[k] = np.where(live, np.minimum(margins[k], v.astype(np.float64)),
                                      margins[k])
        else:
            u = np.minimum(np.maximum(a, -f(2.0)), f(2.0))
            sin, cos = np.sin(th), np.cos(th)
            th_norm = np.arctan2(sin, cos)
            cost = th_norm * th_norm + f(0.1) * (thdot * thdot) + f(0.001) * (u * u)
            nd = thdot + (f(3 * 10.0 / (2 * 1.0)) * sin + f(3.0) * u) * f(0.05)
            nd = np.minimum(np.maximum(nd, -f(8.0)), f(8.0))
            th = np.where(live, th + nd * f(0.05), th)
            thdot = np.where(live, nd, thdot)
            r = -cost
            done = np.zeros(B, bool)
        rew = np.where(live, rew + r, rew)
        msteps = msteps + live
        env_steps = env_steps + live
        done = done | (env_steps >= max_env_steps)
        ob = obs().astype(np.float64)
        ob_sum = np.where(live[:, None], ob_sum + ob, ob_sum)
        ob_sumsq = np.where(live[:, None], ob_sumsq + ob * ob, ob_sumsq)
        end_step = np.where(live & done, t + 1, end_step)
        alive = live & ~done

    out = {"env_steps": env_steps, "alive": alive.astype(np.float64),
           "member_steps": msteps, "rew_total": rew, "ob_sum": ob_sum,
           "ob_sumsq": ob_sumsq}
    if cart:
        out["state"] = np.stack([x, x_dot, theta, theta_dot], axis=1)
    else:
        out["th"], out["thdot"] = th, thdot
    return out, {"end_step": end_step, "actions": actions, "margins": margins}


def cartpole_rollout(state, net, n_steps, dtype=np.float64, noise=None,
                     max_env_steps=CP_MAX_STEPS):
    """n_steps of CartPole from `state` (not modified).

    state: dict of CARTPOLE_KEYS, (B, ...) arrays (see cartpole_state).
    net: dict of policy_actions keywords (dims, weight_rows, obmean, obstd,
    ob_clip, optionally eps and act_final); slot b uses weight row b // eps.
    noise: None or a dict of seed (None: no seed_dev), ac_std, noiseless_from
    and optionally salt_base (default 0).
    Returns (state, info). info: end_step (B,), the 1-based step of this call
    at which the slot's episode ended, 0 if it did not; actions (n_steps, B),
    the raw actions, 0 where the slot was not alive; margins, a dict of (B,)
    arrays, the smallest value seen while the slot was alive of |a| ("a": the
    force is a sign), ||x| - 2.4| ("x") and ||theta| - 12 deg| ("theta"), inf
    for a slot that never stepped.
    """
    return _rollout("cartpole", state, net, n_steps, dtype, noise, max_env_steps)


def pendulum_rollout(state, net, n_steps, dtype=np.float64, noise=None,
                     max_env_steps=PD_MAX_STEPS):
    """n_steps of Pendulum from `state` (dict of PENDULUM_KEYS, see
    pendulum_state); arguments and returns as cartpole_rollout. Pendulum has
    no threshold on a float, so info["margins"] is empty."""
    return _rollout("pendulum", state, net, n_steps, dtype, noise, max_env_steps)
