"""GpuEngine(weights_dtype="fp32"): construction (cpu), the tie from
``theta`` and the noise table to the float64 oracle (gpu), its teeth, and
whole generations.

The tie: the engine's own launch wrappers run n steps from a prescribed state
and every rollout buffer must be within ``16 * E32`` of the float64 oracle
whose weight rows the TEST computes from ``engine.theta``, the noise-table
slices at ``engine.offsets``, the signs and sigma — evaluated in float64 and
rounded once to float32 (tests/oracle64_f32.py). Nothing is read back from
``engine.weights``. The same comparison on a bf16-weights engine must exceed
the bound (bf16 rounding is ~2^15 x fp32), or the tie would prove nothing.

Measured on MI355X, worst buffer's max |err| / E32 (bound: 16; the teeth
cases must EXCEED it):

  case                                ratio  worst buffer
  tie_swimmer_step                     1.79  mo_sumsq
  tie_swimmer_noiseless                0.94  rew_total
  tie_humanoid_step                    2.13  behv
  tie_humanoid_noiseless               0.84  s
  teeth_swimmer_bf16                19081.4  s
  teeth_humanoid_bf16               21982.8  behv

The env's fixed matrices are pinned (``matrix_seed``): their default seed goes
through ``hash(name)``, which is salted per process, and the figures above
would otherwise change from process to process.
"""
import json
import os
import zlib

import numpy as np
import pytest
import torch

from es_pytorch_amd.config import AttrDict, load_config
from es_pytorch_amd.core.engine import GpuEngine
from es_pytorch_amd.core.noisetable import NoiseTable
from es_pytorch_amd.core.policy import Policy
from es_pytorch_amd.envs import make_batched
from es_pytorch_amd.nn.nn import FeedForward
from es_pytorch_amd.nn.optimizers import Adam
from es_pytorch_amd.parallel.comm import Comm
from es_pytorch_amd.utils.rankers import CenteredRanker
from tests.oracle64 import ERR_FACTOR, STATE_KEYS, bf16_bits_to_f64, err_scale, loco_rollout
from tests.oracle64_f32 import fp32_member_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- construction
def _setup(general=None):
    """CPU engine arguments, as in tests/test_validation.py."""
    comm = Comm(torch.device("cpu"))
    cfg = AttrDict({
        "env": {"name": "Hopper-v2", "max_steps": 8},
        "noise": {"tbl_size": 10000, "std": 0.02},
        "policy": {"layer_sizes": [16], "ac_std": 0.0, "l2coeff": 0.005,
                   "lr": 0.01, "ob_clip": 5},
        "general": dict({"name": "t", "policies_per_gen": 4, "batch_size": 100},
                        **(general or {})),
    })
    env = make_batched("Hopper-v2", 5, torch.device("cpu"), max_steps=8)
    nn = FeedForward([16], torch.nn.Tanh(), env, 0.0, 5)
    policy = Policy(nn, 0.02, Adam(len(Policy.get_flat(nn)), 0.01))
    nt = NoiseTable.create_shared(comm, 10000, len(policy), seed=1)
    rs = np.random.RandomState(0)
    return cfg, comm, policy, nt, env, rs


def _assert_fp32(eng):
    assert eng.weights.dtype == torch.float32
    assert eng.weights.shape == (eng.M, eng.row_stride) and eng.row_stride % 4 == 0
    assert not eng.pair_rollout and not eng.eps_fp8 and not eng.split_dyn
    assert eng._grad_qstd() == 0.0
    assert eng.numerics == {"weights": "fp32", "eps_encoding": "none", "path": "generic",
                            "rollout_mode": "step"}


def test_fp32_constructor_argument():
    _assert_fp32(GpuEngine(*_setup(), use_graph=False, weights_dtype="fp32"))


def test_fp32_config_key_alone_selects_the_mode():
    _assert_fp32(GpuEngine(*_setup({"weights_dtype": "fp32"}), use_graph=False))


def test_default_stays_bf16():
    eng = GpuEngine(*_setup(), use_graph=False)
    assert eng.weights.dtype == torch.bfloat16
    assert eng.numerics == {"weights": "bf16", "eps_encoding": "none", "path": "generic",
                            "rollout_mode": "step"}
    eng = GpuEngine(*_setup({"weights_dtype": "fp32"}), use_graph=False,
                    weights_dtype="bf16")           # the argument wins
    assert eng.weights.dtype == torch.bfloat16


@pytest.mark.parametrize("flag", ["pair_rollout", "eps_fp8", "split_dyn"])
def test_fp32_rejects_explicit_variant_flags(flag):
    with pytest.raises(ValueError, match=flag):
        GpuEngine(*_setup(), use_graph=False, weights_dtype="fp32", **{flag: True})
    # explicit False is fine
    _assert_fp32(GpuEngine(*_setup(), use_graph=False, weights_dtype="fp32",
                           **{flag: False}))


def test_fp32_ignores_config_variant_flags_with_one_note(capsys):
    general = {"pair_rollout": True, "eps_fp8": True, "split_dyn": True,
               "weights_dtype": "fp32"}
    eng = GpuEngine(*_setup(general), use_graph=False)
    _assert_fp32(eng)
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "weights_dtype=fp32" in err
    for k in ("pair_rollout", "eps_fp8", "split_dyn"):
        assert k in err
    # nothing is printed when there is nothing to ignore
    GpuEngine(*_setup({"weights_dtype": "fp32"}), use_graph=False)
    assert capsys.readouterr().err == ""


@pytest.mark.parametrize("bad", ["fp16", "float32", "", 32])
def test_unknown_weights_dtype_rejected(bad):
    with pytest.raises(ValueError, match="weights_dtype"):
        GpuEngine(*_setup(), use_graph=False, weights_dtype=bad)
    with pytest.raises(ValueError, match="weights_dtype"):
        GpuEngine(*_setup({"weights_dtype": bad}), use_graph=False)


def test_noiseless_weights_row_is_theta_on_cpu():
    """noiseless_eval's CPU branch fills the noiseless row: exact in fp32."""
    eng = GpuEngine(*_setup(), use_graph=False, weights_dtype="fp32")
    eng.weights.zero_()
    eng._step_body = lambda t: None     # the forward is a HIP kernel: not under test
    eng.noiseless_eval()
    assert eng.weights.dtype == torch.float32
    assert torch.equal(eng.weights[:, :eng.n], eng.theta.expand(eng.M, eng.n))


def test_humanoid_fp32_config_loads():
    cfg = load_config(os.path.join(ROOT, "configs", "humanoid_fp32.json"))
    base = load_config(os.path.join(ROOT, "configs", "humanoid.json"))
    assert cfg.general.weights_dtype == "fp32"
    assert cfg.general.pair_rollout is False and cfg.general.eps_fp8 is False
    for sec in ("env", "noise", "policy", "experimental"):
        assert cfg[sec] == base[sec], sec
    with open(os.path.join(ROOT, "configs", "humanoid_fp32.json")) as f:
        assert json.load(f)["general"]["policies_per_gen"] == base.general.policies_per_gen


# ------------------------------------------------------------------- gpu: tie
@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _engine(dev, env_name, hidden, pop, eps, max_steps, weights_dtype, tbl=400_000,
            general=None, **kw):
    torch.manual_seed(31)
    std = 0.05
    comm = Comm(dev)
    cfg = AttrDict({"env": {"name": env_name, "max_steps": max_steps},
                    "noise": {"tbl_size": tbl, "std": std},
                    "policy": {"layer_sizes": hidden, "ac_std": 0.0, "l2coeff": 0.005,
                               "lr": 0.01, "ob_clip": 5, "save_obs_chance": 1.0},
                    "general": dict({"policies_per_gen": pop, "batch_size": 500,
                                     "seed": 3, "eps_per_policy": eps},
                                    **(general or {}))})
    # same env matrices in every process (the default seed is salted per process)
    env = make_batched(env_name, (pop + 1) * eps, dev, max_steps=max_steps,
                       terminate_on_fall=True,
                       matrix_seed=0xE5 + zlib.crc32(env_name.encode()) % 100000)
    nn = FeedForward(hidden, torch.nn.Tanh(), env, 0.0, 5)
    policy = Policy(nn, std, Adam(len(Policy.get_flat(nn)), 0.01))
    nt = NoiseTable.create_shared(comm, tbl, len(policy), seed=7, device=dev)
    kw.setdefault("use_graph", False)
    return GpuEngine(cfg, comm, policy, nt, env, np.random.RandomState(5),
                     weights_dtype=weights_dtype, **kw)


def _bits(tensor):
    return tensor.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _pick_threshold(state, envd, policy, n_steps, members):
    """Fall threshold in the widest gap of the oracle's h (h does not depend
    on the threshold: dead members keep integrating). Candidates are the gap
    centres over every step's h of the initially-live stepped slots; the one
    with the largest margin wins among those that leave both outcomes (with a
    single live slot: h + 0.25, it falls)."""
    envd = dict(envd, fall_thr=-1e9)
    _, infos = loco_rollout(state, envd, policy, n_steps, members, np.float64)
    live = state["alive"][members] > 0
    hs = np.sort(np.concatenate([i["h"][live] for i in infos]))
    if live.sum() == 1:
        return float(np.float32(infos[0]["h"][live][0] + 0.25))
    cands = 0.5 * (hs[1:] + hs[:-1])
    for j in np.argsort(-np.diff(hs)):
        thr = float(np.float32(cands[j]))
        fell = np.zeros(live.sum(), bool)
        for i in infos:
            fell |= i["h"][live] < thr
        if fell.any() and not fell.all():
            return thr
    raise AssertionError("no threshold leaves both outcomes")


def _tie(dev, env_name, hidden, pop, n_steps, mode, weights_dtype):
    """Run n_steps through the engine's wrappers from a prescribed state;
    return (got, y64, e32, state0, members) against the theta+table oracle."""
    eps = 2
    kw = dict(pair_rollout=False) if weights_dtype == "bf16" else {}
    eng = _engine(dev, env_name, hidden, pop, eps, n_steps, weights_dtype, **kw)
    assert eng.fused and not eng.pair_rollout and not eng.split_dyn
    assert eng.numerics["weights"] == weights_dtype and eng.numerics["path"] == "fused"
    env = eng.env
    env.dt, env.ctrl_cost, env.leak, env.alive_bonus = 0.07, 0.05, 0.35, 1.0
    rng = np.random.RandomState(17)
    B, S, D, n = eng.B, env.sdim, env.ob_dim, eng.n
    mm = (eng.M - 1) * eng.eps
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    eng._upload_offsets()
    eng.acstd_dev.fill_(0.0)
    eng._pheno()
    alive = (np.arange(B) % 3 != 1).astype(np.float32)
    alive[mm:] = [1.0, 0.0]                  # noiseless slots: one live, one dead
    state = dict(s=f32(rng.randn(B, S) * 0.6), pos=f32(rng.randn(B, 3)), goal=None,
                 alive=alive, rew_total=f32(rng.randn(B) * 3.0),
                 member_steps=f32(rng.randint(0, 40, size=B)), behv=f32(rng.randn(B, 3)),
                 mo_sum=f32(rng.randn(B, D) * 2.0), mo_sumsq=f32(rng.rand(B, D) * 3.0))
    obmean, obstd = f32(rng.randn(D) * 0.2), f32(rng.rand(D) * 0.5 + 0.3)
    tensors = dict(s=env.s, pos=env.pos, alive=eng.alive, rew_total=eng.rew_total,
                   member_steps=eng.member_steps, behv=eng.behv, mo_sum=eng.mo_sum,
                   mo_sumsq=eng.mo_sumsq)
    for k, tt in tensors.items():
        tt.copy_(torch.from_numpy(state[k]).to(dev))
    eng.obmean.copy_(torch.from_numpy(obmean).to(dev))
    eng.obstd.copy_(torch.from_numpy(obstd).to(dev))

    # the oracle's weight rows: theta, the table slices at the offsets, signs
    # and sigma — float64, rounded once. engine.weights is NOT read.
    theta = eng.theta.cpu().numpy()
    offs = eng.offsets.cpu().numpy()
    table = eng.nt.noise.cpu().numpy()
    signs = eng.signs.cpu().numpy()
    assert theta.dtype == np.float32 and table.dtype == np.float32
    assert (signs[:eng.pairs] == 1).all() and (signs[eng.pairs:-1] == -1).all() \
        and signs[-1] == 0 and len(set(offs[:eng.pairs])) == eng.pairs
    noise_rows = np.stack([table[o:o + n] for o in offs])
    rows = fp32_member_rows(theta, noise_rows, signs, np.float32(eng.policy.std))
    assert np.array_equal(rows[-1], theta)

    members = np.arange(mm, B) if mode == "noiseless" else np.arange(mm)
    policy = dict(dims=list(eng.dims), weight_rows=rows.astype(np.float64), obmean=obmean,
                  obstd=obstd, ob_clip=5.0, eps=eng.eps, wrow0=0, act_mode=0, bins=0)
    envd = dict(A=bf16_bits_to_f64(_bits(env.A_bf16)), B=env.B.cpu().numpy(),
                b0=env.b0.cpu().numpy(), wv=env.wv.cpu().numpy(), wa=env.wa.cpu().numpy(),
                wy=env.wy.cpu().numpy(), wh=env.wh.cpu().numpy(), leak=env.leak,
                ctrl=env.ctrl_cost, alive_bonus=env.alive_bonus, dt=env.dt, terminate=1,
                goal=0, fall_thr=0.0)
    thr = _pick_threshold(state, envd, policy, n_steps, members)
    env.fall_threshold = envd["fall_thr"] = thr
    y64, infos = loco_rollout(state, envd, policy, n_steps, members, np.float64)
    y32, _ = loco_rollout(state, envd, policy, n_steps, members, np.float32)
    for info in infos:
        assert (np.abs(info["h"] - thr) > 1e-3).all(), "h on the fall threshold"
    e32 = {k: err_scale(y32[k][members], y64[k][members]) for k in STATE_KEYS}

    if mode == "step":
        for t in range(n_steps):
            eng._loco_step(t)
    else:
        assert eng.max_steps == n_steps
        eng._loco_noiseless_episode()
    torch.cuda.synchronize(dev)
    got = {k: tt.cpu().numpy() for k, tt in tensors.items()}
    return got, y64, e32, state, members


TIE_SHAPES = {"swimmer": ("Swimmer-v3", [16], 6, 3),
              "humanoid": ("Humanoid-v2", [256, 256], 4, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "noiseless"])
@pytest.mark.parametrize("shape", list(TIE_SHAPES))
def test_fp32_engine_tied_to_theta_and_table(dev, shape, mode):
    from tests.test_kernel_oracle_f32 import compare
    env_name, hidden, pop, n_steps = TIE_SHAPES[shape]
    got, y64, e32, state, members = _tie(dev, env_name, hidden, pop, n_steps, mode, "fp32")
    compare(f"tie_{shape}_{mode}", got, y64, e32, state, members)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(TIE_SHAPES))
def test_bf16_engine_fails_the_same_tie(dev, shape):
    """Teeth: a bf16-weights engine on the same comparison exceeds the bound
    on at least one buffer."""
    env_name, hidden, pop, n_steps = TIE_SHAPES[shape]
    got, y64, e32, state, m = _tie(dev, env_name, hidden, pop, n_steps, "step", "bf16")
    ratios = {k: float(np.max(np.abs(got[k][m].astype(np.float64) - y64[k][m]))) / e32[k]
              for k in STATE_KEYS if e32[k] > 0}
    worst = max(ratios, key=ratios.get)
    print(f"ORACLE-RATIO loco_f32 teeth_{shape}_bf16 WORST ratio={ratios[worst]:.1f} "
          f"({worst})")
    assert ratios[worst] > ERR_FACTOR, ratios


# --------------------------------------------------------- gpu: whole generations
def _two_generations(dev, env_name="Swimmer-v3", hidden=(16,), pop=8, eps=2,
                     max_steps=12, general=None, **kw):
    eng = _engine(dev, env_name, list(hidden), pop, eps, max_steps, "fp32",
                  tbl=300_000, general=general, **kw)
    flat0 = eng.policy.flat_params.copy()
    ranker = CenteredRanker()
    _, obstat = eng.step(ranker)
    eng.update_obstat(obstat)
    eng.step(ranker)
    torch.cuda.synchronize(dev)
    fits = np.concatenate([ranker.fits_pos, ranker.fits_neg]).ravel().copy()
    return eng, flat0, eng.policy.flat_params.copy(), fits


@pytest.mark.gpu
def test_fp32_generations_graph(dev):
    eng, flat0, flat, fits = _two_generations(dev, use_graph=True)
    assert eng.use_graph and eng.fused and eng.weights.dtype == torch.float32
    assert eng.numerics == {"weights": "fp32", "eps_encoding": "none", "path": "fused",
                            "rollout_mode": "step"}
    assert np.isfinite(flat).all() and np.isfinite(fits).all()
    assert not np.array_equal(flat, flat0), "parameters did not move"
    assert (flat != flat0).mean() > 0.9
    assert eng.timings["env_steps"] > 0
    # identically seeded engine: bitwise
    _, _, flat_b, fits_b = _two_generations(dev, use_graph=True)
    assert np.array_equal(flat, flat_b) and np.array_equal(fits, fits_b)
    # no graph: bitwise
    _, _, flat_c, fits_c = _two_generations(dev, use_graph=False)
    assert np.array_equal(flat, flat_c) and np.array_equal(fits, fits_c)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["episode", "steps_per_launch2"])
def test_fp32_launch_shapes_agree_bitwise(dev, variant):
    _, _, flat, fits = _two_generations(dev, use_graph=False)
    if variant == "episode":
        eng, _, flat_v, fits_v = _two_generations(dev, use_graph=False,
                                                  rollout_mode="episode")
        assert eng.numerics["rollout_mode"] == "episode"
    else:
        eng, _, flat_v, fits_v = _two_generations(dev, use_graph=False,
                                                  general={"steps_per_launch": 2})
        assert eng.steps_per_launch == 2
    assert np.array_equal(fits, fits_v) and np.array_equal(flat, flat_v)


@pytest.mark.gpu
def test_fp32_generic_forward_path(dev):
    """CartPole takes the generic torch-env path (es_mlp_fwd_f32 per step)."""
    out = []
    for _ in range(2):
        torch.manual_seed(12)
        comm = Comm(dev)
        cfg = AttrDict({"env": {"name": "CartPole-v1", "max_steps": 40},
                        "noise": {"tbl_size": 300_000, "std": 0.05},
                        "policy": {"layer_sizes": [16], "ac_std": 0.01, "l2coeff": 0.005,
                                   "lr": 0.02, "ob_clip": 5, "save_obs_chance": 1.0},
                        "general": {"policies_per_gen": 8, "batch_size": 100, "seed": 2,
                                    "weights_dtype": "fp32"}})
        env = make_batched("CartPole-v1", 9, dev)
        nn = FeedForward([16], torch.nn.Tanh(), env, 0.01, 5)
        policy = Policy(nn, 0.05, Adam(len(Policy.get_flat(nn)), 0.02))
        nt = NoiseTable.create_shared(comm, 300_000, len(policy), seed=9, device=dev)
        eng = GpuEngine(cfg, comm, policy, nt, env, np.random.RandomState(31),
                        use_graph=False)
        assert not eng.fused and eng.weights.dtype == torch.float32
        assert eng.numerics["path"] == "generic" and eng.numerics["weights"] == "fp32"
        ranker = CenteredRanker()
        flat0 = policy.flat_params.copy()
        eng.step(ranker)
        torch.cuda.synchronize(dev)
        fits = np.concatenate([ranker.fits_pos, ranker.fits_neg]).ravel()
        assert np.isfinite(fits).all() and np.abs(fits).sum() > 0
        assert np.isfinite(policy.flat_params).all()
        assert not np.array_equal(policy.flat_params, flat0)
        out.append((fits.copy(), policy.flat_params.copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
