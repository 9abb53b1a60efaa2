"""MultiAgentGpuEngine with pair_rollout=True: the interface (CPU), and a whole
generation tied to the float64 oracle from ``theta`` and the noise table.

The GPU tie follows tests/test_ma_engine_fp32.py, whose engine it builds (16
policies per generation, ``[16]`` hidden, 40 steps) and never reads the
engine's blobs. It copies each policy's ``theta`` before ``step()``, reads
afterwards the offsets, table, seed and obmean/obstd the generation used and
builds the rows ITSELF as ``bf16(theta) +- bf16(sigma * noise[off:off + n])``
(the noiseless game on ``bf16(theta)``), with the round-to-nearest-even of
``bf16_rne`` below, which is checked bit for bit against an es_pheno_bf16 call
on test-owned buffers. ``tag_rollout`` replays the generation from the env's
reset state: ``rew_total`` within ``16 * E32``, ``member_steps`` and ``alive``
exact, ObStat sums within ``16 * B * E32``.

The tie discriminates: the same generation replayed on materialized rows
``bf16(theta +- sigma * noise)``, what the engine evaluates without
pair_rollout, sits outside ``16 * E32`` of the pair replay (both sides are
oracle runs).

The seeds are such that no game of the generation comes within 1e-3 of the
catch threshold in the oracle and float32 plays the same game (asserted, cap
zero).

Measured on MI355X (E32 of rew_total 2.33e-05, bound 16): rew_total max |err|
/ E32 1.26, steps and alive exact, ObStat sums at most 0.08 x B x E32 (bound
16 x B x E32). The materialized-rows replay sits 31 868 x E32 from the pair
replay. The oracle catches at steps 29, 21, 32 and 18 (games 4, 7, 12 and the
noiseless game 16), thirteen games run all 40 steps, smallest margin 0.0088;
float32 plays the same game.
"""
import os

import numpy as np
import pytest
import torch

from tests.oracle64 import ERR_FACTOR, bf16_bits_to_f64, fp32_error_scale, max_ratio
from tests.oracle64_tag import tag_rollout, tag_state
from tests.test_ma_engine_fp32 import MARGIN_MIN, MAX_STEPS, PPG, make_engine, tie

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS, B = PPG // 2, PPG + 1


# ---- the interface, on a CPU noise table ------------------------------------

def cpu_engine(**kw):
    return make_engine("cpu", tbl=20_000, **kw)[0]


def test_pair_needs_episode_mode():
    with pytest.raises(ValueError, match="ma_pair_rollout.*needs ma_rollout_mode='episode'"):
        cpu_engine(pair_rollout=True)
    with pytest.raises(ValueError, match="set ma_rollout_mode='episode' or leave"):
        cpu_engine(rollout_mode="step", pair_rollout=True)


def test_pair_with_fp32_raises():
    with pytest.raises(ValueError, match="ma_pair_rollout.*has no fp32 form - use "
                                         "weights_dtype='bf16' or leave"):
        cpu_engine(pair_rollout=True, weights_dtype="fp32")
    with pytest.raises(ValueError, match="has no fp32 form"):
        cpu_engine(general={"ma_pair_rollout": True, "weights_dtype": "fp32"})


def test_non_bool_raises():
    for bad in (1, 0, "true", "episode", 1.0):
        with pytest.raises(ValueError, match="ma_pair_rollout must be true or false"):
            cpu_engine(pair_rollout=bad)
    with pytest.raises(ValueError, match="ma_pair_rollout must be true or false, got 'yes'"):
        cpu_engine(general={"ma_pair_rollout": "yes"})
    with pytest.raises(ValueError, match="ma_pair_rollout must be true or false"):
        cpu_engine(general={"ma_pair_rollout": None})


def test_config_key_is_read_when_keyword_is_none():
    # True from the config reaches the episode-mode check ...
    with pytest.raises(ValueError, match="needs ma_rollout_mode='episode'"):
        cpu_engine(general={"ma_pair_rollout": True})
    with pytest.raises(ValueError, match="needs ma_rollout_mode='episode'"):
        cpu_engine(general={"ma_pair_rollout": True}, pair_rollout=None)
    # ... the keyword beats it, and the single-policy engine's key is not read
    assert cpu_engine(general={"ma_pair_rollout": True}, pair_rollout=False) \
        .pair_rollout is False
    assert cpu_engine(general={"pair_rollout": True}).pair_rollout is False
    assert cpu_engine(general={"ma_pair_rollout": False}).pair_rollout is False


def test_default_is_unchanged():
    eng = cpu_engine()
    assert eng.pair_rollout is False
    assert eng.numerics == {"weights": "bf16", "eps_encoding": "none", "path": "tag",
                            "rollout_mode": "step"}
    for st in eng.states:
        assert st.weights.shape == (eng.B, st.row_stride)
        assert st.weights.dtype == torch.bfloat16
        for name in ("theta_row", "eps_rows", "_theta_blob", "_eps_blob"):
            assert not hasattr(st, name), name


def test_pair_config_loads():
    from es_pytorch_amd.config import load_config
    cfg = load_config(os.path.join(ROOT, "configs", "multi_agent_pair.json"))
    fused = load_config(os.path.join(ROOT, "configs", "multi_agent_fused.json"))
    assert cfg.general.ma_pair_rollout is True
    assert cfg.general.ma_rollout_mode == "episode"
    assert cfg.general.get("weights_dtype", "bf16") == "bf16"
    want = fused.to_dict()
    want["general"]["ma_pair_rollout"] = True
    assert cfg.to_dict() == want


# ---- the tie from theta and the table (GPU) ---------------------------------

@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def bf16_rne(x):
    """float32 -> bf16 bit patterns, round to nearest, ties to even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    assert np.isfinite(x).all()
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def pair_rows_of(q, table):
    """(B, n) float64 rows [theta + eps_p | theta - eps_p | theta] with
    theta = bf16(theta), eps_p = bf16(float32(std * noise[off_p:off_p + n]))."""
    n, offs = q["n"], q["offsets"]
    assert np.array_equal(offs[:PAIRS], offs[PAIRS:PPG])
    t = bf16_bits_to_f64(bf16_rne(q["theta"]))[None, :]
    noise_rows = np.stack([table[o:o + n] for o in offs[:PAIRS]])
    e = bf16_bits_to_f64(bf16_rne(q["std"] * noise_rows))
    return np.concatenate([t + e, t - e, t], axis=0)


def materialized_rows_of(q, table):
    """(B, n) float64 rows bf16(theta +- std * noise), bf16(theta): the member
    rows of the engine without pair_rollout."""
    n, offs = q["n"], q["offsets"]
    noise_rows = np.stack([table[o:o + n] for o in offs[:PAIRS]])
    s = (q["std"] * noise_rows).astype(np.float32)
    th = q["theta"][None, :]
    return bf16_bits_to_f64(bf16_rne(np.concatenate([th + s, th - s, th], axis=0)))


def generation_inputs(eng, theta0, dev):
    """What the rollout of generation 0 consumed, none of it the engine's rows."""
    from es_pytorch_amd.envs.multiagent import BatchedPursuitTag
    fresh = BatchedPursuitTag(eng.B, dev, max_steps=MAX_STEPS)
    fresh.reset(0)                       # generation 0, rank 0 -> reset seed 0
    inp = dict(p0=fresh.p.cpu().numpy(), seed=int(eng.seed_dev.item()),
               table=eng.nt.noise.cpu().numpy(), pol=[])
    for st, th in zip(eng.states, theta0):
        inp["pol"].append(dict(
            theta=th, offsets=st.offsets.cpu().numpy(), std=np.float32(st.policy.std),
            dims=list(st.dims), n=st.n, obmean=st.obmean.cpu().numpy(),
            obstd=st.obstd.cpu().numpy(), ob_clip=float(st.policy._module.ob_clip),
            ac_std=float(st.acstd_dev.item())))
    return inp


def replay(inp, rows_of):
    """(y64, E32, info) of the generation on the rows rows_of builds."""
    nets, ac_std = [], []
    for q in inp["pol"]:
        assert q["theta"].dtype == np.float32 and inp["table"].dtype == np.float32
        rows = rows_of(q, inp["table"])
        assert rows.shape == (B, q["n"]) and rows.dtype == np.float64
        nets.append(dict(dims=q["dims"], weight_rows=rows, obmean=q["obmean"],
                         obstd=q["obstd"], ob_clip=q["ob_clip"], act_final=1))
        ac_std.append(q["ac_std"])
    assert tuple(ac_std) == (np.float32(0.01),) * 2 and inp["seed"] > 0
    noise = dict(seed=inp["seed"], ac_std=tuple(ac_std), noiseless_from=B - 1)
    state = tag_state(inp["p0"])
    y64, e32 = fp32_error_scale(tag_rollout, state, nets, MAX_STEPS, noise=noise)
    _, info = tag_rollout(state, nets, MAX_STEPS, noise=noise)
    _, info32 = tag_rollout(state, nets, MAX_STEPS, dtype=np.float32, noise=noise)
    return y64, e32, info, info32


def run_generation(dev):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng, policies = make_engine(dev, "episode", pair_rollout=True)
    theta0 = [st.theta.cpu().numpy().copy() for st in eng.states]
    noiseless, obstats = eng.step([CenteredRanker(), CenteredRanker()])
    return eng, noiseless, obstats, generation_inputs(eng, theta0, dev)


@pytest.mark.gpu
def test_bf16_rne_is_es_pheno_bf16(dev):
    """bf16_rne against the kernel that builds the engine's rows: one sigma*eps
    row (zero theta, sign +1) and one theta row (sign 0), bit for bit."""
    from es_pytorch_amd import ops
    rng = np.random.RandomState(3)
    n, stride, std = 179, 184, np.float32(0.05)
    table = rng.randn(4096).astype(np.float32)
    theta = (rng.randn(n) * 0.3).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tbl_d, off_d = t(table), t(np.array([1237], np.int64))
    stream = torch.cuda.current_stream(dev).cuda_stream
    for th, sign, want in ((np.zeros(n, np.float32), 1.0, bf16_rne(std * table[1237:1237 + n])),
                           (theta, 0.0, bf16_rne(theta))):
        out = torch.zeros(stride, dtype=torch.bfloat16, device=dev)
        th_d, sg_d = t(th), t(np.array([sign], np.float32))
        ops.check(ops.hip().es_pheno_bf16(
            out.data_ptr(), th_d.data_ptr(), tbl_d.data_ptr(), off_d.data_ptr(),
            sg_d.data_ptr(), 1, n, stride, float(std), stream), "es_pheno_bf16")
        torch.cuda.synchronize(dev)
        got = out.view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(got[:n], want) and not got[n:].any()


@pytest.mark.gpu
def test_pair_generation_matches_oracle_from_theta(dev):
    eng, noiseless, obstats, inp = run_generation(dev)
    assert eng.numerics == {"weights": "bf16", "eps_encoding": "bf16", "path": "tag_pair",
                            "rollout_mode": "episode"}
    for st in eng.states:
        assert not hasattr(st, "weights")
        assert st._theta_blob.shape == (2, st.row_stride)
        assert st._eps_blob.shape == (PAIRS + 2, st.row_stride)
        assert not st._eps_blob[PAIRS:].view(torch.int16).any()   # the zero row, the guard
    y64, e32, info, info32 = replay(inp, pair_rows_of)
    print("PAIR-ENGINE margins", np.sort(info["margin"])[:4], "catch steps",
          info["catch_step"].tolist(), "E32 rew_total", e32["rew_total"])
    # the oracle alone: no game on the threshold, float32 plays the same game
    assert int((info["margin"] < MARGIN_MIN).sum()) == 0, info["margin"]
    assert np.array_equal(info["catch_step"], info32["catch_step"])
    exact, r = tie(eng, y64, e32, "pair episode")
    assert exact
    assert r <= ERR_FACTOR, (r, e32["rew_total"])
    total = float(y64["steps"].sum())
    for i, ob in enumerate(obstats):
        assert ob.count == total
        for got, key in ((ob.sum, "ob_sum"), (ob.sumsq, "ob_sumsq")):
            want = y64[key][:, i].sum(0)
            print(f"ORACLE-RATIO tag engine pair {key}[{i}] ratio-of-B*E32="
                  f"{np.abs(got - want).max() / (eng.B * e32[key]):.2f}")
            assert np.abs(got - want).max() <= eng.B * ERR_FACTOR * e32[key], key
    rew = eng.rew_total.cpu().numpy()
    assert noiseless == [float(rew[-1, 0]), float(rew[-1, 1])]

    # the tie discriminates: materialized bf16(theta +- sigma*noise) rows play
    # a generation that is outside the bound of the pair replay
    ym, _, _, _ = replay(inp, materialized_rows_of)
    rm = max_ratio(ym["rew_total"], y64["rew_total"], e32["rew_total"])
    print(f"ORACLE-RATIO tag engine materialized-vs-pair rew_total ratio={rm:.1f}")
    assert rm > ERR_FACTOR, rm
    assert np.array_equal(ym["rew_total"][-1], y64["rew_total"][-1])   # both on bf16(theta)


@pytest.mark.gpu
def test_pair_three_generations(dev):
    from es_pytorch_amd.utils.rankers import CenteredRanker
    eng, policies = make_engine(dev, "episode", general={"ma_pair_rollout": True})
    assert eng.pair_rollout is True
    flats = [p.flat_params.copy() for p in policies]
    for gen in range(3):
        noiseless, obstats = eng.step([CenteredRanker(), CenteredRanker()])
        eng.update_obstats(obstats)
        rew = eng.rew_total.cpu().numpy()
        assert noiseless == [float(rew[-1, 0]), float(rew[-1, 1])]
        assert set(eng.timings) == {"rollout_s", "gen_s", "env_steps"}
        assert eng.timings["env_steps"] > 0
        for p, f0 in zip(policies, flats):
            assert not np.array_equal(p.flat_params, f0)
            assert np.isfinite(p.flat_params).all()
        flats = [p.flat_params.copy() for p in policies]
    assert eng.gen == 3 and eng.numerics["path"] == "tag_pair"
