"""GpuEngine(loco_wave=True): one generation on es_loco_wave_episode (all B
slots in one launch), replayed through the float64 oracle from what the engine
itself consumed, and the construction errors of the mode. The engine builder is
tests/test_fp32_engine.py's (env matrices pinned); FALL_THR makes slots fall
inside the short episode with every live h more than 1e-3 away from it.
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import ERR_FACTOR, bf16_bits_to_f64, err_scale, loco_rollout, max_ratio
from tests.test_fp32_engine import _bits, _engine

pytestmark = pytest.mark.gpu

PPG, MAX_STEPS, FALL_THR = 6, 10, -0.25


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def make_engine(dev, name="Swimmer-v3", eps=1, layers=(16,), wdt="bf16", **kw):
    eng = _engine(dev, name, list(layers), PPG, eps, MAX_STEPS, wdt, **kw)
    eng.env.fall_threshold = FALL_THR
    eng.policy._module._action_std = 0.01        # action noise on
    return eng


def replay(eng, dtype, thr=FALL_THR):
    """(state, infos) of generation 0 from the engine's own buffers."""
    env, B, D = eng.env, eng.B, eng.env.ob_dim
    w = eng.weights[:, :eng.n]
    rows = w.cpu().numpy().astype(np.float64) if eng.fp32 else bf16_bits_to_f64(_bits(w))
    num = lambda t: t.cpu().numpy()
    goal = num(env.goal) if env.goal_conditioned else None
    env.reset(0)                         # generation 0, rank 0 -> reset seed 0
    z = lambda *shape: np.zeros(shape, dtype=np.float32)
    state = dict(s=num(env.s), pos=z(B, 3), goal=goal, alive=z(B) + 1, rew_total=z(B),
                 member_steps=z(B), behv=z(B, 3), mo_sum=z(B, D), mo_sumsq=z(B, D))
    policy = dict(dims=list(eng.dims), weight_rows=rows, obmean=num(eng.obmean),
                  obstd=num(eng.obstd), ob_clip=5.0, eps=eng.eps, wrow0=0, act_mode=0, bins=0)
    envd = dict(A=bf16_bits_to_f64(_bits(env.A_bf16)), B=num(env.B), b0=num(env.b0),
                wv=num(env.wv), wa=num(env.wa), wy=num(env.wy), wh=num(env.wh),
                leak=env.leak, ctrl=env.ctrl_cost, alive_bonus=env.alive_bonus, dt=env.dt,
                terminate=1, goal=int(env.goal_conditioned), fall_thr=thr)
    noise = dict(seed=int(eng.seed_dev.item()), ac_std=float(eng.acstd_dev.item()),
                 noiseless_from=(eng.M - 1) * eng.eps)
    return loco_rollout(state, envd, policy, MAX_STEPS, None, dtype, noise)


@pytest.mark.parametrize("name,eps", [("Swimmer-v3", 2), ("AntFlagrun-v3", 1)])
@pytest.mark.parametrize("wdt", ["bf16", "fp32"])
def test_loco_wave_generation_matches_oracle(dev, name, eps, wdt):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng = make_engine(dev, name, eps, wdt=wdt, loco_wave=True, use_graph=True)
    assert eng.loco_wave and eng.fused and not eng.pair_rollout
    assert eng.numerics == {"weights": wdt, "eps_encoding": "none", "path": "loco_wave",
                            "rollout_mode": "episode"}
    flat0 = eng.policy.flat_params.copy()
    noiseless, _ = eng.step(CenteredRanker())
    assert eng._graph is None            # one launch: no hipGraph on this path
    rew, steps, alive = (t.cpu().numpy() for t in (eng.rew_total, eng.member_steps,
                                                   eng.alive))
    (y64, infos), (y32, _) = replay(eng, np.float64), replay(eng, np.float32)
    assert float(eng.acstd_dev.item()) == np.float32(0.01)
    for info in infos:
        live = info["alive_before"]
        assert (np.abs(info["h"][live] - FALL_THR) > 1e-3).all(), "h on the threshold"
    assert np.array_equal(y64["member_steps"], y32["member_steps"])
    assert 0 < y64["alive"].sum() < eng.B, "need fallen and surviving slots"
    e32 = err_scale(y32["rew_total"], y64["rew_total"])
    r = max_ratio(rew, y64["rew_total"], e32)
    print(f"ORACLE-RATIO loco wave engine {name} {wdt} rew_total ratio={r:.2f} E32={e32:.3g}")
    assert np.array_equal(steps, y64["member_steps"])
    assert np.array_equal(alive, y64["alive"])
    assert np.isfinite(rew).all() and r <= ERR_FACTOR, (r, e32)
    assert noiseless.reward == float(rew[(eng.M - 1) * eng.eps:].mean())
    assert not np.array_equal(eng.policy.flat_params, flat0)


def test_loco_wave_plumbing_and_rejections(dev, monkeypatch):
    from es_pytorch_amd import ops
    assert not make_engine(dev).loco_wave                      # default off
    eng = make_engine(dev, general={"loco_wave": True, "pair_rollout": True})
    assert eng.loco_wave and not eng.pair_rollout and eng.numerics["path"] == "loco_wave"
    eng = make_engine(dev, general={"loco_wave": True}, loco_wave=False)
    assert not eng.loco_wave and eng.numerics["path"] == "fused"

    for kw in (dict(loco_wave=1), dict(general={"loco_wave": "yes"})):
        with pytest.raises(ValueError, match="loco_wave must be true or false"):
            make_engine(dev, **kw)
    for flag in ("pair_rollout", "eps_fp8", "split_dyn"):
        with pytest.raises(ValueError, match=f"{flag}=True is not available"):
            make_engine(dev, loco_wave=True, **{flag: True})
    with pytest.raises(ValueError, match="steps_per_launch"):
        make_engine(dev, loco_wave=True, general={"steps_per_launch": 5})
    with pytest.raises(ValueError, match=r"at most 64 wide.*returned -116"):
        make_engine(dev, loco_wave=True, layers=(256,))
    with pytest.raises(ValueError, match="SyntheticLocomotion"):
        make_engine(dev, loco_wave=True, fused=False)
    # a library of an earlier revision: no fallback to the block kernel
    real = ops.hip()
    old = type("OldLib", (), {"__getattr__": lambda self, k: getattr(real, k)
                              if "loco_wave" not in k else object.__getattribute__(self, k)})()
    monkeypatch.setattr(ops, "hip", lambda: old)
    with pytest.raises(RuntimeError, match="es_loco_wave_episode"):
        make_engine(dev, loco_wave=True)
