"""The fp8 pair rollout keeps fp8 on under every launch shape, and the launch
shape does not change a bit of the generation: steps_per_launch 1 (per-step
launches of es_loco_pair_step_fp8), 3 and 7 (es_loco_pair_episode_fp8 chunks,
the last one short) and rollout_mode="episode" (one launch) give byte-equal
fitnesses, rollout buffers and updated theta. Mirrors tests/test_pair_episode.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ["fits", "rew_total", "behv", "member_steps", "theta"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _run(dev, rollout_mode, chunk, use_graph=False, pop=16, steps=10):
    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.engine import GpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs import make_batched
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import Comm
    from es_pytorch_amd.utils.rankers import CenteredRanker

    torch.manual_seed(11)
    comm = Comm(dev)
    general = {"policies_per_gen": pop, "batch_size": 500, "seed": 3}
    if chunk is not None:
        general["steps_per_launch"] = chunk
    cfg = AttrDict({"env": {"name": "Humanoid-v2", "max_steps": steps},
                    "noise": {"tbl_size": 2_000_000, "std": 0.02},
                    "policy": {"layer_sizes": [64, 64], "ac_std": 0.01,
                               "l2coeff": 0.005, "lr": 0.01, "ob_clip": 5,
                               "save_obs_chance": 1.0},
                    "general": general})
    env = make_batched("Humanoid-v2", pop + 1, dev, max_steps=steps,
                       terminate_on_fall=True)
    nn = FeedForward([64, 64], torch.nn.Tanh(), env, 0.01, 5)
    policy = Policy(nn, 0.02, Adam(len(Policy.get_flat(nn)), 0.01))
    nt = NoiseTable.create_shared(comm, 2_000_000, len(policy), seed=7, device=dev)
    rs = np.random.RandomState(5)
    eng = GpuEngine(cfg, comm, policy, nt, env, rs, use_graph=use_graph,
                    rollout_mode=rollout_mode, pair_rollout=True, eps_fp8=True)
    assert eng.pair_rollout
    assert eng.eps_fp8, (rollout_mode, chunk)
    if chunk is not None:
        assert eng.steps_per_launch == chunk
    ranker = CenteredRanker()
    eng.step(ranker)
    torch.cuda.synchronize(dev)
    return (np.concatenate([ranker.fits_pos, ranker.fits_neg]).ravel(),
            eng.rew_total.cpu().numpy().copy(),
            eng.behv.cpu().numpy().copy(),
            eng.member_steps.cpu().numpy().copy(),
            eng.theta.cpu().numpy().copy())


@pytest.fixture(scope="module")
def per_step(dev):
    ref = _run(dev, "step", 1)
    print("member_steps of the per-step run:", ref[3])
    return ref


@pytest.mark.parametrize("mode,chunk,graph", [("step", 3, False), ("step", 7, False),
                                              ("episode", 1, False), ("step", 3, True),
                                              ("step", None, True)])
def test_fp8_launch_shapes_agree_bitwise(dev, per_step, mode, chunk, graph):
    out = _run(dev, mode, chunk, use_graph=graph)
    for a, b, name in zip(per_step, out, NAMES):
        np.testing.assert_array_equal(a, b, err_msg=f"{mode}/chunk{chunk}/graph{graph}:{name}")
