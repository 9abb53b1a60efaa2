"""GpuEngine(loco_wave_batch=True): one generation with eps_per_policy = 3 on
es_loco_wave_batch_episode (all members in one launch), replayed through the
float64 oracle from what the engine itself consumed, and the construction
errors of the mode. Builder and replay are tests/test_loco_engine_wave.py's,
the fall thresholds tests/test_loco_engine_batch.py's.
"""
import numpy as np
import pytest

from tests.oracle64 import ERR_FACTOR, err_scale, max_ratio
from tests.test_loco_engine_batch import FALL_THRS
from tests.test_loco_engine_wave import dev, make_engine, replay  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["Swimmer-v3", "AntFlagrun-v3"])
@pytest.mark.parametrize("wdt", ["bf16", "fp32"])
def test_loco_wave_batch_generation_matches_oracle(dev, name, wdt):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng = make_engine(dev, name, 3, wdt=wdt, loco_wave_batch=True, use_graph=True)
    FALL_THR = FALL_THRS[name]
    eng.env.fall_threshold = FALL_THR
    assert eng.loco_wave_batch and eng.fused and not eng.pair_rollout and eng.eps == 3
    assert eng.numerics == {"weights": wdt, "eps_encoding": "none",
                            "path": "loco_wave_batch", "rollout_mode": "episode"}
    flat0 = eng.policy.flat_params.copy()
    noiseless, _ = eng.step(CenteredRanker())
    assert eng._graph is None            # one launch: no hipGraph on this path
    rew, steps, alive = (t.cpu().numpy() for t in (eng.rew_total, eng.member_steps,
                                                   eng.alive))
    (y64, infos), (y32, _) = (replay(eng, np.float64, FALL_THR),
                             replay(eng, np.float32, FALL_THR))
    for info in infos:
        live = info["alive_before"]
        assert (np.abs(info["h"][live] - FALL_THR) > 1e-3).all(), "h on the threshold"
    assert np.array_equal(y64["member_steps"], y32["member_steps"])
    assert 0 < y64["alive"].sum() < eng.B, "need fallen and surviving slots"
    e32 = err_scale(y32["rew_total"], y64["rew_total"])
    r = max_ratio(rew, y64["rew_total"], e32)
    print(f"ORACLE-RATIO loco wave batch engine {name} {wdt} rew_total ratio={r:.2f} "
          f"E32={e32:.3g}")
    assert np.array_equal(steps, y64["member_steps"])
    assert np.array_equal(alive, y64["alive"])
    assert np.isfinite(rew).all() and r <= ERR_FACTOR, (r, e32)
    # the mean of the noiseless member's float32 rewards as the engine takes it,
    # on the device (numpy's mean of the same three rounds an ulp apart)
    assert noiseless.reward == float(eng.rew_total[(eng.M - 1) * eng.eps:].mean().item())
    assert not np.array_equal(eng.policy.flat_params, flat0)


def test_loco_wave_batch_plumbing_and_rejections(dev, monkeypatch):
    from es_pytorch_amd import ops
    assert not make_engine(dev).loco_wave_batch                # default off
    eng = make_engine(dev, general={"loco_wave_batch": True, "pair_rollout": True})
    assert eng.loco_wave_batch and not eng.pair_rollout
    assert eng.numerics["path"] == "loco_wave_batch"
    eng = make_engine(dev, general={"loco_wave_batch": True}, loco_wave_batch=False)
    assert not eng.loco_wave_batch and eng.numerics["path"] == "fused"

    for kw in (dict(loco_wave_batch=1), dict(general={"loco_wave_batch": "yes"})):
        with pytest.raises(ValueError, match="loco_wave_batch must be true or false"):
            make_engine(dev, **kw)
    for flag in ("pair_rollout", "eps_fp8", "split_dyn"):
        with pytest.raises(ValueError, match=f"{flag}=True is not available"):
            make_engine(dev, loco_wave_batch=True, **{flag: True})
    with pytest.raises(ValueError, match="steps_per_launch"):
        make_engine(dev, loco_wave_batch=True, general={"steps_per_launch": 5})
    for other in ("loco_wave", "loco_batch"):
        with pytest.raises(ValueError, match=f"loco_wave_batch and {other} select"):
            make_engine(dev, loco_wave_batch=True, **{other: True})
    with pytest.raises(ValueError, match=r"eps_per_policy 17.*returned -118"):
        make_engine(dev, eps=17, loco_wave_batch=True)
    with pytest.raises(ValueError, match=r"at most 64 wide.*returned -118"):
        make_engine(dev, eps=3, loco_wave_batch=True, layers=(256,))
    with pytest.raises(ValueError, match="SyntheticLocomotion"):
        make_engine(dev, loco_wave_batch=True, fused=False)
    # a library of an earlier revision: no fallback to another kernel
    real = ops.hip()
    old = type("OldLib", (), {"__getattr__": lambda self, k: getattr(real, k)
                              if "loco_wave_batch" not in k
                              else object.__getattribute__(self, k)})()
    monkeypatch.setattr(ops, "hip", lambda: old)
    with pytest.raises(RuntimeError, match="es_loco_wave_batch_episode"):
        make_engine(dev, loco_wave_batch=True)
