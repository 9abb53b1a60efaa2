"""MultiAgentGpuEngine in rollout_mode="episode" (one es_tag_episode launch per
generation) against the float64 oracle, on what the engine itself consumed.

After one ``step()`` the test reads back both policies' member blobs, their
obmean/obstd, the seed the engine drew and the env's reset state for the
engine's reset seed, replays the rollout with ``tag_rollout`` and requires
``rew_total`` within ``16 * E32`` and ``member_steps`` exactly. The engine's
seeds were chosen so that no game of that generation comes within 1e-3 of the
catch threshold in the oracle (asserted, cap zero).

Measured on MI355X: rew_total max |err| / E32 = 1.09 (E32 4.21e-05, bound 16);
oracle catches at steps 29, 21, 32 and 18 (games 4, 7, 12 and the noiseless
game 16), thirteen games run all 40 steps, smallest margin 0.0088.
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import ERR_FACTOR, bf16_bits_to_f64, fp32_error_scale, max_ratio
from tests.oracle64_tag import tag_rollout, tag_state

pytestmark = pytest.mark.gpu

MARGIN_MIN = 1e-3
MAX_STEPS = 40
PPG = 16
SEEDS = (1, 2)              # torch.manual_seed (policy init), engine RandomState


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def make_engine(dev, rollout_mode=None, general=None, env=None, seeds=SEEDS):
    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.ma_engine import MultiAgentGpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs.multiagent import BatchedPursuitTag
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import Comm

    torch.manual_seed(seeds[0])
    comm = Comm(dev)
    cfg = AttrDict({"env": {"name": "PursuitTag", "max_steps": MAX_STEPS},
                    "noise": {"tbl_size": 500_000, "std": 0.05},
                    "policy": {"layer_sizes": [16], "ac_std": 0.01, "l2coeff": 0.005,
                               "lr": 0.02, "ob_clip": 5, "save_obs_chance": 1.0},
                    "general": dict({"policies_per_gen": PPG, "batch_size": 100,
                                     "seed": 6}, **(general or {}))})
    tag = BatchedPursuitTag(PPG + 1, dev, max_steps=MAX_STEPS)
    env = tag if env is None else env

    class _View:
        def __init__(self, i):
            self.observation_space = tag.observation_space[i]
            self.action_space = tag.action_space[i]

    policies = []
    for i in range(2):
        nn = FeedForward([16], torch.nn.Tanh(), _View(i), 0.01, 5)
        policies.append(Policy(nn, 0.05, Adam(len(Policy.get_flat(nn)), 0.02)))
    nt = NoiseTable.create_shared(comm, 500_000, len(policies[0]), seed=11, device=dev)
    rs = np.random.RandomState(seeds[1])
    eng = MultiAgentGpuEngine(cfg, comm, policies, nt, env, rs, rollout_mode=rollout_mode)
    return eng, policies


def consumed_inputs(eng, dev):
    """What generation 0's rollout read: (state, nets, noise) for tag_rollout."""
    from es_pytorch_amd.envs.multiagent import BatchedPursuitTag
    B = eng.B
    fresh = BatchedPursuitTag(B, dev, max_steps=MAX_STEPS)
    fresh.reset(0)                       # generation 0, rank 0 -> reset seed 0
    state = tag_state(fresh.p.cpu().numpy())
    nets, ac_std = [], []
    for st in eng.states:
        bits = st.weights.view(torch.int16).cpu().numpy().view(np.uint16)
        nets.append(dict(dims=list(st.dims), weight_rows=bf16_bits_to_f64(bits),
                         obmean=st.obmean.cpu().numpy(), obstd=st.obstd.cpu().numpy(),
                         ob_clip=float(st.policy._module.ob_clip), act_final=1))
        ac_std.append(float(st.acstd_dev.item()))
    noise = dict(seed=int(eng.seed_dev.item()), ac_std=tuple(ac_std), noiseless_from=B - 1)
    return state, nets, noise


def test_episode_generation_matches_oracle(dev):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng, policies = make_engine(dev, "episode")
    assert eng.rollout_mode == "episode"
    flats0 = [p.flat_params.copy() for p in policies]
    noiseless, obstats = eng.step([CenteredRanker(), CenteredRanker()])
    state, nets, noise = consumed_inputs(eng, dev)
    assert noise["ac_std"] == (np.float32(0.01),) * 2 and noise["seed"] > 0
    y64, e32 = fp32_error_scale(tag_rollout, state, nets, MAX_STEPS, noise=noise)
    _, info = tag_rollout(state, nets, MAX_STEPS, noise=noise)
    print("FUSED-ENGINE margins", np.sort(info["margin"])[:4], "catch steps",
          info["catch_step"].tolist())
    assert int((info["margin"] < MARGIN_MIN).sum()) == 0, info["margin"]

    rew = eng.rew_total.cpu().numpy()
    steps = eng.member_steps.cpu().numpy()
    r = max_ratio(rew, y64["rew_total"], e32["rew_total"])
    print(f"ORACLE-RATIO tag engine rew_total ratio={r:.2f} E32={e32['rew_total']:.3g}")
    assert np.array_equal(steps, y64["steps"])
    assert np.isfinite(rew).all() and r <= ERR_FACTOR, (r, e32["rew_total"])
    assert np.array_equal(eng.alive.cpu().numpy(), y64["alive"])

    # strictly competitive: per-game rewards sum to ~0
    assert np.abs(rew.sum(axis=1)).max() < 1e-2
    # ObStat increments: the count is the sum of steps
    total = float(y64["steps"].sum())
    for i, ob in enumerate(obstats):
        assert ob.count == total
        # each game's sums are within 16 E32 of the oracle's; B games add up
        for got, key in ((ob.sum, "ob_sum"), (ob.sumsq, "ob_sumsq")):
            want = y64[key][:, i].sum(0)
            assert np.abs(got - want).max() <= eng.B * ERR_FACTOR * e32[key], key
    assert noiseless == [float(rew[-1, 0]), float(rew[-1, 1])]
    assert eng.timings["env_steps"] == float(steps[:PPG].sum()) * 2 > 0
    assert set(eng.timings) == {"rollout_s", "gen_s", "env_steps"}

    # a second generation: params moved and stayed finite
    eng.update_obstats(obstats)
    eng.step([CenteredRanker(), CenteredRanker()])
    for p, f0 in zip(policies, flats0):
        assert not np.array_equal(p.flat_params, f0)
        assert np.isfinite(p.flat_params).all()
    assert eng.timings["env_steps"] > 0


def test_episode_mode_from_config_and_default(dev):
    eng, _ = make_engine(dev)
    assert eng.rollout_mode == "step"
    eng, _ = make_engine(dev, general={"ma_rollout_mode": "episode"})
    assert eng.rollout_mode == "episode"
    eng, _ = make_engine(dev, "step", general={"ma_rollout_mode": "episode"})
    assert eng.rollout_mode == "step"
    with pytest.raises(ValueError, match="ma_rollout_mode"):
        make_engine(dev, "fused")


def test_episode_mode_rejects_other_envs_and_cpu(dev):
    from es_pytorch_amd.envs.multiagent import BatchedPursuitTag

    class OtherGame:
        N_AGENTS = 2
        batch = PPG + 1
        ob_dims = [8, 8]
        ac_dims = [2, 2]
        device = dev

    with pytest.raises(ValueError, match="BatchedPursuitTag"):
        make_engine(dev, "episode", env=OtherGame())
    with pytest.raises(ValueError, match="GPU"):
        make_engine(dev, "episode", env=BatchedPursuitTag(PPG + 1, "cpu", MAX_STEPS))
    # the same env is fine in step mode
    eng, _ = make_engine(dev, "step", env=OtherGame())
    assert eng.rollout_mode == "step"
