"""MultiAgentGpuEngine with weights_dtype="fp32": the interface (CPU), and a
whole generation tied to the float64 oracle from ``theta`` and the noise table.

The GPU tie never reads the engine's member blobs. It copies each policy's
``theta`` before ``step()``, reads afterwards the offsets, signs, table, seed
and obmean/obstd the generation used, builds the member rows ITSELF with
``fp32_member_rows`` and replays the rollout with ``tag_rollout`` from the
env's reset state. ``rew_total`` must be within ``16 * E32``, ``member_steps``
and ``alive`` exact, in both rollout modes, which consume the same inputs (one
oracle run serves both). So a fault in es_pheno_f32, or in the engine's
offset/sign layout, fails here. The same tie on a bf16 engine must fail: bf16
rows sit thousands of E32 away.

The seeds are such that no game of the generation comes within 1e-3 of the
catch threshold in the oracle and float32 plays the same game (asserted, cap
zero).

The oracle's ``alive`` is "not caught", as the fused kernel's is. The step
loop folds the env's ``done`` into its ``alive``, and ``BatchedPursuitTag``
also sets ``done`` at its step limit, so in rollout mode "step" the exact
comparison is against the oracle's ``alive`` AND ``steps < max_steps`` (see
``tie``).

Measured on MI355X, rew_total max |err| / E32 (E32 2.72e-05, bound 16): fp32
episode 0.82, fp32 step 0.82, steps and alive exact in both; ObStat sums at
most 0.08 x B x E32 (bound 16 x B x E32). The bf16 engine on the same tie:
18 409. The oracle catches at steps 29, 21, 32 and 18 (games 4, 7, 12 and the
noiseless game 16), thirteen games run all 40 steps, smallest margin 0.0107;
float32 plays the same game.
"""
import os

import numpy as np
import pytest
import torch

from tests.oracle64 import ERR_FACTOR, fp32_error_scale, max_ratio
from tests.oracle64_f32 import fp32_member_rows
from tests.oracle64_tag import tag_rollout, tag_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_MIN = 1e-3
MAX_STEPS = 40
PPG = 16
SEEDS = (1, 2)              # torch.manual_seed (policy init), engine RandomState
TBL, TBL_SEED = 500_000, 11


def make_engine(dev, rollout_mode=None, general=None, tbl=TBL, **kw):
    """tests/test_ma_engine_fused.py::make_engine, plus constructor keywords."""
    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.ma_engine import MultiAgentGpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs.multiagent import BatchedPursuitTag
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import Comm

    dev = torch.device(dev)
    torch.manual_seed(SEEDS[0])
    comm = Comm(dev)
    cfg = AttrDict({"env": {"name": "PursuitTag", "max_steps": MAX_STEPS},
                    "noise": {"tbl_size": tbl, "std": 0.05},
                    "policy": {"layer_sizes": [16], "ac_std": 0.01, "l2coeff": 0.005,
                               "lr": 0.02, "ob_clip": 5, "save_obs_chance": 1.0},
                    "general": dict({"policies_per_gen": PPG, "batch_size": 100,
                                     "seed": 6}, **(general or {}))})
    env = BatchedPursuitTag(PPG + 1, dev, max_steps=MAX_STEPS)

    class _View:
        def __init__(self, i):
            self.observation_space = env.observation_space[i]
            self.action_space = env.action_space[i]

    policies = []
    for i in range(2):
        nn = FeedForward([16], torch.nn.Tanh(), _View(i), 0.01, 5)
        policies.append(Policy(nn, 0.05, Adam(len(Policy.get_flat(nn)), 0.02)))
    nt = NoiseTable.create_shared(comm, tbl, len(policies[0]), seed=TBL_SEED, device=dev)
    rs = np.random.RandomState(SEEDS[1])
    eng = MultiAgentGpuEngine(cfg, comm, policies, nt, env, rs, rollout_mode=rollout_mode,
                              **kw)
    return eng, policies


# ---- the interface, on a CPU noise table in rollout mode "step" -------------

def cpu_engine(**kw):
    return make_engine("cpu", tbl=20_000, **kw)[0]


def test_constructor_keyword():
    eng = cpu_engine(weights_dtype="fp32")
    assert eng.weights_dtype == "fp32" and eng.rollout_mode == "step"


def test_config_key_alone():
    eng = cpu_engine(general={"weights_dtype": "fp32"})
    assert eng.weights_dtype == "fp32"


def test_keyword_beats_config():
    eng = cpu_engine(general={"weights_dtype": "fp32"}, weights_dtype="bf16")
    assert eng.weights_dtype == "bf16"
    eng = cpu_engine(general={"weights_dtype": "bf16"}, weights_dtype="fp32")
    assert eng.weights_dtype == "fp32"


def test_default_is_bf16():
    eng = cpu_engine()
    assert eng.weights_dtype == "bf16"
    eng = cpu_engine(weights_dtype=None)
    assert eng.weights_dtype == "bf16"


def test_unknown_value_raises():
    with pytest.raises(ValueError, match="weights_dtype must be 'bf16' or 'fp32', got 'fp16'"):
        cpu_engine(weights_dtype="fp16")
    with pytest.raises(ValueError, match="weights_dtype must be"):
        cpu_engine(general={"weights_dtype": "float32"})


def test_numerics_keys():
    assert cpu_engine().numerics == {"weights": "bf16", "eps_encoding": "none",
                                     "path": "tag", "rollout_mode": "step"}
    assert cpu_engine(weights_dtype="fp32").numerics == {
        "weights": "fp32", "eps_encoding": "none", "path": "tag", "rollout_mode": "step"}


def test_blob_dtype_per_mode():
    for wd, want in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        eng = cpu_engine(weights_dtype=wd)
        for st in eng.states:
            assert st.weights.dtype == want
            assert st.row_stride == (st.n + 7) // 8 * 8
            assert st.weights.shape == (eng.B, st.row_stride)


def test_fp32_config_loads():
    from es_pytorch_amd.config import load_config
    cfg = load_config(os.path.join(ROOT, "configs", "multi_agent_fp32.json"))
    fused = load_config(os.path.join(ROOT, "configs", "multi_agent_fused.json"))
    assert cfg.general.weights_dtype == "fp32" and cfg.general.ma_rollout_mode == "episode"
    want = fused.to_dict()
    want["general"]["weights_dtype"] = "fp32"
    assert cfg.to_dict() == want


# ---- the tie from theta and the table (GPU) ---------------------------------

@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def run_generation(dev, rollout_mode, **kw):
    """One generation; (engine, policies, obstats, inputs) with inputs = what the
    rollout consumed, none of it the member blobs."""
    from es_pytorch_amd.envs.multiagent import BatchedPursuitTag
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng, policies = make_engine(dev, rollout_mode, **kw)
    theta0 = [st.theta.cpu().numpy().copy() for st in eng.states]
    noiseless, obstats = eng.step([CenteredRanker(), CenteredRanker()])
    table = eng.nt.noise.cpu().numpy()
    fresh = BatchedPursuitTag(eng.B, dev, max_steps=MAX_STEPS)
    fresh.reset(0)                       # generation 0, rank 0 -> reset seed 0
    inp = dict(p0=fresh.p.cpu().numpy(), seed=int(eng.seed_dev.item()), table=table,
               pol=[])
    for st, th in zip(eng.states, theta0):
        inp["pol"].append(dict(
            theta=th, offsets=st.offsets.cpu().numpy(), signs=st.signs.cpu().numpy(),
            std=np.float32(st.policy.std), dims=list(st.dims), n=st.n,
            obmean=st.obmean.cpu().numpy(), obstd=st.obstd.cpu().numpy(),
            ob_clip=float(st.policy._module.ob_clip), ac_std=float(st.acstd_dev.item())))
    return eng, policies, noiseless, obstats, inp


def oracle_of(inp):
    """(y64, E32, info) of the generation from theta and the table."""
    B = PPG + 1
    nets, ac_std = [], []
    for q in inp["pol"]:
        offs, signs, n = q["offsets"], q["signs"], q["n"]
        assert q["theta"].dtype == np.float32 and inp["table"].dtype == np.float32
        assert (signs[:PPG // 2] == 1).all() and (signs[PPG // 2:PPG] == -1).all() \
            and signs[-1] == 0 and np.array_equal(offs[:PPG // 2], offs[PPG // 2:PPG])
        noise_rows = np.stack([inp["table"][o:o + n] for o in offs])
        rows = fp32_member_rows(q["theta"], noise_rows, signs, q["std"])
        assert rows.shape == (B, n) and np.array_equal(rows[-1], q["theta"])
        nets.append(dict(dims=q["dims"], weight_rows=rows.astype(np.float64),
                         obmean=q["obmean"], obstd=q["obstd"], ob_clip=q["ob_clip"],
                         act_final=1))
        ac_std.append(q["ac_std"])
    assert tuple(ac_std) == (np.float32(0.01),) * 2 and inp["seed"] > 0
    noise = dict(seed=inp["seed"], ac_std=tuple(ac_std), noiseless_from=B - 1)
    state = tag_state(inp["p0"])
    y64, e32 = fp32_error_scale(tag_rollout, state, nets, MAX_STEPS, noise=noise)
    _, info = tag_rollout(state, nets, MAX_STEPS, noise=noise)
    _, info32 = tag_rollout(state, nets, MAX_STEPS, dtype=np.float32, noise=noise)
    print("FP32-ENGINE margins", np.sort(info["margin"])[:4], "catch steps",
          info["catch_step"].tolist(), "E32 rew_total", e32["rew_total"])
    # the oracle alone: no game on the threshold, float32 plays the same game
    assert int((info["margin"] < MARGIN_MIN).sum()) == 0, info["margin"]
    assert np.array_equal(info["catch_step"], info32["catch_step"])
    return y64, e32, info


_ORACLE = {}


def shared_oracle(inp):
    """Both rollout modes, and the bf16 engine, draw the same inputs from the
    same seeds: one oracle run, and every later caller must bring the same."""
    if not _ORACLE:
        _ORACLE["inp"], _ORACLE["out"] = inp, oracle_of(inp)
    ref = _ORACLE["inp"]
    assert inp["seed"] == ref["seed"] and np.array_equal(inp["p0"], ref["p0"])
    assert np.array_equal(inp["table"], ref["table"])
    for a, b in zip(inp["pol"], ref["pol"]):
        for k in ("theta", "offsets", "signs", "obmean", "obstd"):
            assert np.array_equal(a[k], b[k]), k
    return _ORACLE["out"]


def tie(eng, y64, e32, tag):
    """(steps and alive exact, rew_total ratio) of the engine against the oracle.

    The oracle's and the fused kernel's ``alive`` is "not caught". The step
    loop folds the env's own ``done`` into it, which is also set at the env's
    step limit (``BatchedPursuitTag.step``: ``caught | steps >= max_steps``),
    so in rollout mode "step" a game that was never caught still ends the
    generation with alive == 0. That is the oracle's alive AND steps < limit,
    compared exactly."""
    rew = eng.rew_total.cpu().numpy()
    steps = eng.member_steps.cpu().numpy()
    alive = eng.alive.cpu().numpy()
    want_alive = y64["alive"]
    if eng.rollout_mode == "step":
        want_alive = want_alive * (y64["steps"] < MAX_STEPS)
    print(f"ORACLE-RATIO tag engine {tag} steps exact="
          f"{np.array_equal(steps, y64['steps'])} alive exact="
          f"{np.array_equal(alive, want_alive)}")
    exact = np.array_equal(steps, y64["steps"]) and np.array_equal(alive, want_alive)
    r = max_ratio(rew, y64["rew_total"], e32["rew_total"]) if np.isfinite(rew).all() \
        else float("inf")
    print(f"ORACLE-RATIO tag engine {tag} rew_total ratio={r:.2f} "
          f"E32={e32['rew_total']:.3g} steps/alive exact={exact}")
    return exact, r


@pytest.mark.gpu
@pytest.mark.parametrize("rollout_mode", ["episode", "step"])
def test_fp32_generation_matches_oracle_from_theta(dev, rollout_mode):
    eng, policies, noiseless, obstats, inp = run_generation(dev, rollout_mode,
                                                            weights_dtype="fp32")
    assert eng.numerics == {"weights": "fp32", "eps_encoding": "none", "path": "tag",
                            "rollout_mode": rollout_mode}
    assert all(st.weights.dtype == torch.float32 for st in eng.states)
    y64, e32, info = shared_oracle(inp)
    exact, r = tie(eng, y64, e32, f"fp32 {rollout_mode}")
    total = float(y64["steps"].sum())
    for i, ob in enumerate(obstats):
        for got, key in ((ob.sum, "ob_sum"), (ob.sumsq, "ob_sumsq")):
            want = y64[key][:, i].sum(0)
            print(f"ORACLE-RATIO tag engine fp32 {rollout_mode} {key}[{i}] "
                  f"ratio-of-B*E32={np.abs(got - want).max() / (eng.B * e32[key]):.2f}")
    assert exact
    assert r <= ERR_FACTOR, (r, e32["rew_total"])
    # ObStat increments: the count is the sum of steps; each game's sums are
    # within 16 E32 of the oracle's and B games add up
    for i, ob in enumerate(obstats):
        assert ob.count == total
        for got, key in ((ob.sum, "ob_sum"), (ob.sumsq, "ob_sumsq")):
            want = y64[key][:, i].sum(0)
            assert np.abs(got - want).max() <= eng.B * ERR_FACTOR * e32[key], key
    rew = eng.rew_total.cpu().numpy()
    assert noiseless == [float(rew[-1, 0]), float(rew[-1, 1])]


@pytest.mark.gpu
def test_bf16_generation_misses_the_fp32_tie(dev):
    """Teeth: a default (bf16) engine consumes the same theta, table, offsets
    and seed, and must NOT pass the tie to the fp32 rows."""
    eng, _, _, _, inp = run_generation(dev, "episode")
    assert eng.weights_dtype == "bf16"
    assert all(st.weights.dtype == torch.bfloat16 for st in eng.states)
    y64, e32, info = shared_oracle(inp)
    exact, r = tie(eng, y64, e32, "bf16 episode (teeth)")
    assert (not exact) or r > ERR_FACTOR, (exact, r)


@pytest.mark.gpu
def test_fp32_episode_two_generations(dev):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng, policies = make_engine(dev, "episode", weights_dtype="fp32")
    flats0 = [p.flat_params.copy() for p in policies]
    for _ in range(2):
        _, obstats = eng.step([CenteredRanker(), CenteredRanker()])
        eng.update_obstats(obstats)
        assert set(eng.timings) == {"rollout_s", "gen_s", "env_steps"}
        assert eng.timings["env_steps"] > 0
    for p, f0 in zip(policies, flats0):
        assert not np.array_equal(p.flat_params, f0)
        assert np.isfinite(p.flat_params).all()
    assert eng.numerics["weights"] == "fp32" and eng.gen == 2
