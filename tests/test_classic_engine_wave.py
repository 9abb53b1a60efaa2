"""GpuEngine(classic_wave=True): the generation of
tests/test_classic_engine_fused.py on the wave-per-slot kernel
(es_classic_wave_episode), against the float64 oracle on what the engine
itself consumed. Same seeds as there, so generation 0 reads the same inputs,
whose margins (no CartPole slot within 1e-3 of a decision) are asserted again.
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import ERR_FACTOR, fp32_error_scale, max_ratio
from tests.test_classic_engine_fused import (MARGIN_MIN, MAX_STEPS, PPG, SEEDS,
                                             consumed_inputs, make_engine)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("env_name,wdt", list(SEEDS), ids=lambda v: str(v))
def test_classic_wave_generation_matches_oracle(dev, env_name, wdt):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng, policy = make_engine(dev, env_name, SEEDS[(env_name, wdt)], classic_wave=True,
                              weights_dtype=wdt)
    assert eng.classic_wave and eng.classic_fused and not eng.fused
    assert eng.numerics == {"weights": wdt, "eps_encoding": "none", "path": "classic_wave",
                            "rollout_mode": "step"}
    flat0 = policy.flat_params.copy()
    noiseless, obstat = eng.step(CenteredRanker())
    assert eng._graph is None
    fn, state, net, noise = consumed_inputs(eng, dev, env_name)
    y64, e32 = fp32_error_scale(fn, state, net, MAX_STEPS, noise=noise)
    _, info = fn(state, net, MAX_STEPS, noise=noise)
    _, info32 = fn(state, net, MAX_STEPS, dtype=np.float32, noise=noise)
    for k, m in info["margins"].items():
        assert int((m < MARGIN_MIN).sum()) == 0, (k, m)
    assert np.array_equal(info["end_step"], info32["end_step"])

    rew = eng.rew_total.cpu().numpy()
    steps = eng.member_steps.cpu().numpy()
    r = max_ratio(rew, y64["rew_total"], e32["rew_total"])
    print(f"ORACLE-RATIO classic wave engine {env_name} {wdt} rew_total ratio={r:.2f} "
          f"E32={e32['rew_total']:.3g}")
    assert np.array_equal(steps, y64["member_steps"])
    assert np.array_equal(eng.alive.cpu().numpy(), y64["alive"])
    assert np.isfinite(rew).all() and r <= ERR_FACTOR, (r, e32["rew_total"])

    mask = eng.save_mask.cpu().numpy()
    assert mask.tolist() == [1.0] * PPG + [0.0]
    assert obstat.count == float((y64["member_steps"] * mask).sum()) > 0
    for got, key in ((obstat.sum, "ob_sum"), (obstat.sumsq, "ob_sumsq")):
        want = (y64[key] * mask[:, None]).sum(0)
        assert np.abs(got - want).max() <= eng.B * ERR_FACTOR * e32[key], key
    assert noiseless.reward == float(rew[-1])
    assert torch.equal(eng.behv, eng.env.positions)

    eng.update_obstat(obstat)
    eng.step(CenteredRanker())
    assert not np.array_equal(policy.flat_params, flat0)
    assert np.isfinite(policy.flat_params).all()


def test_classic_wave_plumbing_and_rejections(dev):
    from es_pytorch_amd.envs import make_batched
    from es_pytorch_amd.nn.nn import FeedForward

    eng, _ = make_engine(dev, classic_fused=True)           # default off
    assert not eng.classic_wave and eng.numerics["path"] == "classic"
    eng, _ = make_engine(dev, general={"classic_wave": True})
    assert eng.classic_wave and eng.classic_fused
    assert eng.numerics["path"] == "classic_wave"
    eng, _ = make_engine(dev, general={"classic_wave": True}, classic_wave=False)
    assert not eng.classic_wave and eng.numerics["path"] == "generic"
    eng, _ = make_engine(dev, general={"classic_wave": False}, classic_wave=True)
    assert eng.numerics["path"] == "classic_wave"

    with pytest.raises(ValueError, match="classic_fused=False"):
        make_engine(dev, classic_wave=True, classic_fused=False)
    with pytest.raises(ValueError, match="at most 64 wide"):
        make_engine(dev, classic_wave=True,
                    module=lambda env: FeedForward([256], torch.nn.Tanh(), env, 0.01, 5))
    with pytest.raises(ValueError, match="BatchedCartPole"):
        make_engine(dev, "Hopper-v2", env=make_batched("Hopper-v2", PPG + 1, dev),
                    classic_wave=True, fused=False)
