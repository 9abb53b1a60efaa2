"""GpuEngine(classic_fused=True): one es_classic_episode launch per generation,
against the float64 oracle on what the engine itself consumed.

After one ``step()`` the test reads back the member blob, obmean/obstd, the
seed the engine drew and the env's reset state for the engine's reset seed,
replays the rollout with tests/oracle64_classic.py and requires ``rew_total``
within ``16 * E32``, ``member_steps`` and ``alive`` exactly, the ObStat count
equal to the save_mask-weighted step sum and its sums within ``B * 16 * E32``.
The engine seeds were chosen so that no CartPole slot of that generation comes
within 1e-3 of a decision (force sign, x and theta thresholds) in the oracle
(asserted, cap zero).

Measured on MI355X, rew_total max |err| / E32 (bound 16): CartPole bf16 0.00
(E32 6.56e-07; the reward is the step count), CartPole fp32 0.00 (E32
2.38e-06), Pendulum 1.00 (E32 7.55e-05). Oracle end steps: CartPole bf16 8..11
for all nine slots, smallest margins |a| 0.0036, theta 0.0023; CartPole fp32
22..35 with slot 6 running all 40 steps, smallest margins |a| 0.0018, theta
0.0018. Fused against generic on Pendulum: the fitnesses came out identical.
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import ERR_FACTOR, bf16_bits_to_f64, fp32_error_scale, max_ratio
from tests.oracle64_classic import (cartpole_rollout, cartpole_state, pendulum_rollout,
                                    pendulum_state)

pytestmark = pytest.mark.gpu

MARGIN_MIN = 1e-3
MAX_STEPS = 40
PPG = 8
# (torch.manual_seed for the policy init, engine RandomState) per variant
SEEDS = {("CartPole-v1", "bf16"): (114, 115), ("CartPole-v1", "fp32"): (82, 83),
         ("Pendulum-v1", "bf16"): (1, 2)}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def make_engine(dev, env_name="CartPole-v1", seeds=(1, 2), ac_std=0.01, general=None,
                env=None, module=None, nt_dev=None, **kw):
    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.engine import GpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs import make_batched
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import Comm

    torch.manual_seed(seeds[0])
    comm = Comm(dev)
    cfg = AttrDict({"env": {"name": env_name, "max_steps": MAX_STEPS},
                    "noise": {"tbl_size": 300_000, "std": 0.05},
                    "policy": {"layer_sizes": [16], "ac_std": ac_std, "l2coeff": 0.005,
                               "lr": 0.02, "ob_clip": 5, "save_obs_chance": 1.0},
                    "general": dict({"policies_per_gen": PPG, "batch_size": 100,
                                     "seed": 2}, **(general or {}))})
    env = make_batched(env_name, PPG + 1, dev) if env is None else env
    nn = FeedForward([16], torch.nn.Tanh(), env, ac_std, 5) if module is None \
        else module(env)
    policy = Policy(nn, 0.05, Adam(len(Policy.get_flat(nn)), 0.02))
    nt = NoiseTable.create_shared(comm, 300_000, len(policy), seed=9,
                                  device=dev if nt_dev is None else nt_dev)
    rs = np.random.RandomState(seeds[1])
    return GpuEngine(cfg, comm, policy, nt, env, rs, **kw), policy


def consumed_inputs(eng, dev, env_name):
    """What generation 0's rollout read: (rollout fn, state, net, noise)."""
    from es_pytorch_amd.envs import make_batched
    fresh = make_batched(env_name, eng.B, dev)
    fresh.reset(0)                       # generation 0, rank 0 -> reset seed 0
    if env_name.startswith("CartPole"):
        fn, state = cartpole_rollout, cartpole_state(fresh.state.cpu().numpy())
    else:
        fn, state = pendulum_rollout, pendulum_state(fresh.th.cpu().numpy(),
                                                     fresh.thdot.cpu().numpy())
    w = eng.weights[:, :eng.n].contiguous()     # the row padding is never written
    if eng.fp32:
        rows = w.cpu().numpy().astype(np.float64)
    else:
        rows = bf16_bits_to_f64(w.view(torch.int16).cpu().numpy().view(np.uint16))
    net = dict(dims=list(eng.dims), weight_rows=rows, obmean=eng.obmean.cpu().numpy(),
               obstd=eng.obstd.cpu().numpy(), ob_clip=float(eng.policy._module.ob_clip),
               eps=1, act_final=1)
    noise = dict(seed=int(eng.seed_dev.item()), ac_std=float(eng.acstd_dev.item()),
                 noiseless_from=eng.B - 1)
    return fn, state, net, noise


@pytest.mark.parametrize("env_name,wdt", list(SEEDS), ids=lambda v: str(v))
def test_classic_generation_matches_oracle(dev, env_name, wdt):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng, policy = make_engine(dev, env_name, SEEDS[(env_name, wdt)], classic_fused=True,
                              weights_dtype=wdt)
    assert eng.classic_fused and not eng.fused and eng._graph is None
    assert eng.numerics == {"weights": wdt, "eps_encoding": "none", "path": "classic",
                            "rollout_mode": "step"}
    flat0 = policy.flat_params.copy()
    noiseless, obstat = eng.step(CenteredRanker())
    assert eng._graph is None           # one launch: no hipGraph on this path
    fn, state, net, noise = consumed_inputs(eng, dev, env_name)
    assert noise["ac_std"] == np.float32(0.01) and noise["seed"] > 0
    y64, e32 = fp32_error_scale(fn, state, net, MAX_STEPS, noise=noise)
    _, info = fn(state, net, MAX_STEPS, noise=noise)
    _, info32 = fn(state, net, MAX_STEPS, dtype=np.float32, noise=noise)
    label = f"{env_name} {wdt}"
    print("FUSED-ENGINE", label, "margins",
          {k: float(m.min()) for k, m in info["margins"].items()}, "end steps",
          info["end_step"].tolist())
    for k, m in info["margins"].items():
        assert int((m < MARGIN_MIN).sum()) == 0, (k, m)
    assert np.array_equal(info["end_step"], info32["end_step"])

    rew = eng.rew_total.cpu().numpy()
    steps = eng.member_steps.cpu().numpy()
    r = max_ratio(rew, y64["rew_total"], e32["rew_total"])
    print(f"ORACLE-RATIO classic engine {label} rew_total ratio={r:.2f} "
          f"E32={e32['rew_total']:.3g}")
    assert np.array_equal(steps, y64["member_steps"])
    assert np.array_equal(eng.alive.cpu().numpy(), y64["alive"])
    assert np.isfinite(rew).all() and r <= ERR_FACTOR, (r, e32["rew_total"])
    if env_name.startswith("CartPole"):
        assert (steps < MAX_STEPS).any()            # early exit really happened
        assert np.array_equal(rew, steps)

    # ObStat: save_obs_chance 1 -> every slot but the noiseless one counts
    mask = eng.save_mask.cpu().numpy()
    assert mask.tolist() == [1.0] * PPG + [0.0]
    assert obstat.count == float((y64["member_steps"] * mask).sum()) > 0
    for got, key in ((obstat.sum, "ob_sum"), (obstat.sumsq, "ob_sumsq")):
        want = (y64[key] * mask[:, None]).sum(0)
        assert np.abs(got - want).max() <= eng.B * ERR_FACTOR * e32[key], key
    assert noiseless.reward == float(rew[-1])
    assert eng.timings["env_steps"] == float(steps[:PPG].sum()) > 0
    # behaviour is the env's position at each slot's last live step
    assert torch.equal(eng.behv, eng.env.positions)

    # a second generation: params moved and stayed finite
    eng.update_obstat(obstat)
    eng.step(CenteredRanker())
    assert not np.array_equal(policy.flat_params, flat0)
    assert np.isfinite(policy.flat_params).all()
    assert eng.timings["env_steps"] > 0


def test_classic_fused_opt_in_plumbing(dev):
    eng, _ = make_engine(dev)
    assert not eng.classic_fused and eng.numerics["path"] == "generic"
    eng, _ = make_engine(dev, general={"classic_fused": True})
    assert eng.classic_fused and eng.numerics["path"] == "classic" and not eng.fused
    eng, _ = make_engine(dev, general={"classic_fused": True}, classic_fused=False)
    assert not eng.classic_fused and eng.numerics["path"] == "generic"
    eng, _ = make_engine(dev, general={"classic_fused": False}, classic_fused=True)
    assert eng.classic_fused and eng.numerics["path"] == "classic"


def test_classic_fused_rejections(dev):
    from es_pytorch_amd.envs import make_batched
    from es_pytorch_amd.nn.nn import FFBinned, FFIntegGausAction

    with pytest.raises(ValueError, match="BatchedCartPole"):
        make_engine(dev, "Hopper-v2", env=make_batched("Hopper-v2", PPG + 1, dev),
                    classic_fused=True, fused=False)
    with pytest.raises(ValueError, match="GPU"):
        make_engine(dev, env=make_batched("CartPole-v1", PPG + 1, "cpu"),
                    classic_fused=True)
    with pytest.raises(ValueError, match="GPU"):
        make_engine(torch.device("cpu"), env=make_batched("CartPole-v1", PPG + 1, "cpu"),
                    classic_fused=True)
    with pytest.raises(ValueError, match="plain action head"):
        make_engine(dev, classic_fused=True,
                    module=lambda env: FFBinned([16], torch.nn.Tanh(), env, 5))
    with pytest.raises(ValueError, match="plain action head"):
        make_engine(dev, classic_fused=True,
                    module=lambda env: FFIntegGausAction([16], torch.nn.Tanh(), env, 0.0))
    # the same policies are fine on the generic path
    eng, _ = make_engine(dev, module=lambda env: FFBinned([16], torch.nn.Tanh(), env, 5))
    assert eng.numerics["path"] == "generic"


def test_classic_fused_agrees_with_generic_path(dev):
    """Same seeds, ac_std 0, Pendulum (no thresholds): the fused and the
    generic engine agree on member_steps exactly and on the fitnesses to the
    tolerance test_engine_generic_env_graph holds graph and eager to."""
    from es_pytorch_amd.utils.rankers import CenteredRanker
    fits, steps, nl = {}, {}, {}
    for fused in (False, True):
        eng, _ = make_engine(dev, "Pendulum-v1", (12, 31), ac_std=0.0,
                             classic_fused=fused, use_graph=False)
        assert eng.numerics["path"] == ("classic" if fused else "generic")
        ranker = CenteredRanker()
        noiseless, _ = eng.step(ranker)
        fits[fused] = np.concatenate([ranker.fits_pos, ranker.fits_neg]).ravel()
        steps[fused] = eng.member_steps.cpu().numpy()
        nl[fused] = noiseless.reward
    assert np.array_equal(steps[False], steps[True])
    assert (steps[True] == MAX_STEPS).all()
    print("FUSED-VS-GENERIC max |diff|", np.abs(fits[False] - fits[True]).max(),
          "max |fit|", np.abs(fits[True]).max())
    np.testing.assert_allclose(fits[True], fits[False], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(nl[True], nl[False], rtol=1e-5, atol=1e-5)
    assert np.abs(fits[True]).sum() > 0


def test_classic_fused_noiseless_eval(dev):
    """noiseless_eval() runs the kernel too: it reproduces the noiseless slot
    of a generation evaluated at the same parameters and reset seed."""
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng, _ = make_engine(dev, classic_fused=True)
    rew, behv, n = eng.noiseless_eval()
    assert n == int(rew) > 0 and np.isfinite(behv).all()
    noiseless, _ = eng.step(CenteredRanker())     # gen 0 again: same reset seed
    assert noiseless.reward == rew
