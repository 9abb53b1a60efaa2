"""GpuEngine(device_tail=True): a novelty-search generation whose novelty
scores and ranks come from tail.hip, checked against the host novelty and the
host ranker on what the engine mirrored."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def make_engine(**kw):
    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.engine import GpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs import make_batched
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import Comm

    dev = torch.device("cuda", 0)
    torch.manual_seed(4)
    comm = Comm(dev)
    cfg = AttrDict({"env": {"name": "Humanoid-v2", "max_steps": 20},
                    "noise": {"tbl_size": 1_000_000, "std": 0.02},
                    "policy": {"layer_sizes": [32], "ac_std": 0.0, "l2coeff": 0.005,
                               "lr": 0.01, "ob_clip": 5, "save_obs_chance": 1.0},
                    "general": {"policies_per_gen": 16, "batch_size": 500, "seed": 2}})
    env = make_batched("Humanoid-v2", 17, dev, max_steps=20, terminate_on_fall=False)
    nn = FeedForward([32], torch.nn.Tanh(), env, 0.0, 5)
    policy = Policy(nn, 0.02, Adam(len(Policy.get_flat(nn)), 0.01))
    nt = NoiseTable.create_shared(comm, 1_000_000, len(policy), seed=6, device=dev)
    eng = GpuEngine(cfg, comm, policy, nt, env, np.random.RandomState(1),
                    objective="nsr", novelty_k=3, use_graph=False, **kw)
    eng.archive = torch.randn(8, 2, dtype=torch.float64, device=dev) * 3.0
    return eng


def test_generation_with_device_tail():
    from es_pytorch_amd.utils.novelty import novelty
    from es_pytorch_amd.utils.rankers import (CenteredRanker, EliteRanker,
                                              MultiObjectiveRanker)
    eng = make_engine(device_tail=True)
    assert eng.numerics["tail"] == "device"
    archive = eng.archive.cpu().numpy().copy()
    flat0 = eng.policy.flat_params.copy()
    ranker = MultiObjectiveRanker(CenteredRanker(), 0.3)
    eng.step(ranker)
    assert not np.array_equal(eng.policy.flat_params, flat0)

    # the host ranker on the mirror gives the ranks the update used
    host = MultiObjectiveRanker(CenteredRanker(), 0.3)
    host.rank(ranker.fits_pos, ranker.fits_neg, ranker.noise_inds)
    assert ranker.n_fits_ranked == host.n_fits_ranked == 16
    assert ranker.ranked_fits.tobytes() == host.ranked_fits.astype(np.float64).tobytes()

    # the mirror's novelty column: float32 of the host novelty of each member
    behv = eng._member_behv().cpu().numpy().astype(np.float64)
    want = np.float32([novelty(b[:2], archive, 3) for b in behv[:16]])
    got = np.concatenate([ranker.fits_pos[:, 1], ranker.fits_neg[:, 1]])
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=0)   # fp64 bound + 2^-24

    nov = eng.grow_archive()
    assert eng.archive.shape == (9, 2)
    np.testing.assert_allclose(nov, novelty(behv[-1, :2], archive, 3), rtol=1e-12, atol=0)

    with pytest.raises(ValueError, match="CenteredRanker"):
        eng.step(EliteRanker(CenteredRanker(), 0.5))


def test_default_engine_reports_default_tail():
    eng = make_engine()
    assert not eng.device_tail and eng.numerics["tail"] == "default"
    with pytest.raises(ValueError, match="device_tail"):
        make_engine(device_tail=1)
