"""MultiAgentGpuEngine with tag_wave=True (es_tag_wave_episode): the interface
(CPU), one fp32 generation tied to the float64 oracle from ``theta`` and the
noise table (helpers and seeds of tests/test_ma_engine_fp32.py), one bf16
generation replayed from the member rows the engine holds (as
tests/test_ma_engine_fused.py). ``rew_total`` within ``16 * E32``, steps and
``alive`` exact; the margins of these seeds are asserted where they come from.
Measured on MI355X: ratio 1.00 (fp32), 1.09 (bf16).
"""
import os

import pytest
import torch

from tests.oracle64 import ERR_FACTOR, fp32_error_scale
from tests.oracle64_tag import tag_rollout
from tests.test_ma_engine_fp32 import MAX_STEPS, make_engine, run_generation, shared_oracle, tie
from tests.test_ma_engine_fused import consumed_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS_GPU = "ma_rollout_mode='episode' needs the noise table and the env on a GPU"


# ---- the interface, on a CPU noise table ------------------------------------

def cpu_engine(**kw):
    return make_engine("cpu", tbl=20_000, **kw)[0]


def test_keyword_and_config_key_imply_episode_mode():
    # on the CPU the implied episode mode is what refuses: the key was read
    for kw in (dict(tag_wave=True), dict(general={"ma_tag_wave": True}),
               dict(general={"ma_tag_wave": False}, tag_wave=True),
               dict(tag_wave=True, weights_dtype="fp32")):
        with pytest.raises(ValueError, match=NEEDS_GPU):
            cpu_engine(**kw)
    # the keyword beats the config; with nothing set nothing changes
    for kw in (dict(general={"ma_tag_wave": True}, tag_wave=False), dict()):
        eng = cpu_engine(**kw)
        assert eng.tag_wave is False
        assert eng.numerics == {"weights": "bf16", "eps_encoding": "none", "path": "tag",
                                "rollout_mode": "step"}


def test_non_bool_raises():
    for kw in (dict(tag_wave=1), dict(tag_wave="true"), dict(general={"ma_tag_wave": "yes"})):
        with pytest.raises(ValueError, match="ma_tag_wave must be true or false"):
            cpu_engine(**kw)


def test_step_mode_and_pair_conflict():
    for kw in (dict(tag_wave=True, rollout_mode="step"),
               dict(tag_wave=True, general={"ma_rollout_mode": "step"})):
        with pytest.raises(ValueError, match="ma_tag_wave.*implies ma_rollout_mode='episode'"):
            cpu_engine(**kw)
    for kw in (dict(tag_wave=True, pair_rollout=True),
               dict(general={"ma_tag_wave": True, "ma_pair_rollout": True})):
        with pytest.raises(ValueError, match="ma_tag_wave and ma_pair_rollout"):
            cpu_engine(**kw)


def test_wave_config_loads():
    from es_pytorch_amd.config import load_config
    cfg = load_config(os.path.join(ROOT, "configs", "multi_agent_wave.json"))
    want = load_config(os.path.join(ROOT, "configs", "multi_agent_fused.json")).to_dict()
    want["general"]["ma_tag_wave"] = True
    assert cfg.general.ma_tag_wave is True and cfg.to_dict() == want


dev = torch.device("cuda", 0)


@pytest.mark.gpu
def test_fp32_wave_generation_matches_oracle_from_theta():
    eng, policies, noiseless, obstats, inp = run_generation(dev, None, weights_dtype="fp32",
                                                            tag_wave=True)
    assert eng.numerics == {"weights": "fp32", "eps_encoding": "none", "path": "tag_wave",
                            "rollout_mode": "episode"}
    y64, e32, info = shared_oracle(inp)
    exact, r = tie(eng, y64, e32, "fp32 wave")
    assert exact
    assert r <= ERR_FACTOR, (r, e32["rew_total"])


@pytest.mark.gpu
def test_bf16_wave_generation_matches_oracle_on_its_rows():
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng, policies = make_engine(dev, general={"ma_tag_wave": True})
    assert eng.numerics == {"weights": "bf16", "eps_encoding": "none", "path": "tag_wave",
                            "rollout_mode": "episode"}
    eng.step([CenteredRanker(), CenteredRanker()])
    state, nets, noise = consumed_inputs(eng, dev)
    y64, e32 = fp32_error_scale(tag_rollout, state, nets, MAX_STEPS, noise=noise)
    exact, r = tie(eng, y64, e32, "bf16 wave")
    assert exact
    assert r <= ERR_FACTOR, (r, e32["rew_total"])
