"""Fused locomotion rollout kernels, ONE step (or three) from a prescribed
state, against the float64 oracle (tests/oracle64.py::loco_step).

Every launch shape runs on test-owned buffers (dynamics matrices included, so
the state dim S is free) and every output buffer is compared:
continuous ones by ``|kernel - oracle64| <= 16 * E32`` (E32: the same step in
numpy float32), ``member_steps``/``alive`` and everything a dead member owns
exactly. Accumulators start non-zero and ``alive`` is mixed, ``ac_std`` is 0
(tests/test_kernel_oracle_noise.py runs the same helpers with noise on).

State dims (dynamics A-matvec, 256 threads: OCT = S/8, PART = 256 // OCT):
  S=8 OCT=1 | S=64 tail loop only | S=144 8-deep prologue + guarded drain, no
  steady loop | S=152 smallest S with the steady loop | S=376 Humanoid |
  S=11, S=17 scalar fallback | S=27 + goal (D=29, fp8 plain row 0) |
  S=63 -> O=64 (fp8 row pairs I2=31 < PART=32).

Measured on MI355X, worst buffer's max |err| / E32 per case (bound: 16):

  case                                ratio  worst buffer
  step_S8                              0.92  s
  step_S64                             1.06  s
  step_S144                            0.67  s
  step_S152                            0.66  s
  step_S376                            0.71  behv
  step_S11_scalar                      0.87  s
  step_S17_scalar                      1.47  rew_total
  step_S27_goal                        0.85  rew_total
  step_S63                             1.00  rew_total
  step_S64_binned                      0.88  rew_total
  step_S11_mode2                       0.82  s
  step_S152_mode3_noterm               1.02  s
  split_G2_S8                          0.96  rew_total
  split_G4_S64                         0.76  pos
  split_G5_S152                        0.80  mo_sumsq
  split_G8_S376                        0.79  mo_sum
  split_G5_S144_goal                   0.67  rew_total
  pair_S8                              1.31  mo_sumsq
  pair_S144_eps2                       0.84  s
  pair_S152                            0.85  mo_sumsq
  pair_S376                            0.70  mo_sum
  pair_S11_scalar                      1.03  s
  pair_S27_goal_binned                 1.06  s
  pair_S64_mode2                       0.85  mo_sumsq
  fp8_S64                              1.00  mo_sumsq
  fp8_S152_eps2                        0.97  mo_sumsq
  fp8_S376                             0.69  mo_sum
  fp8_S27_goal_plain_row0              1.12  mo_sumsq
  fp8_S63_I2_lt_PART                   1.31  s
  fp8_S17_scalar_dyn                   0.95  mo_sum
  pair_episode_S152_1step              0.69  mo_sum
  pair_episode_S152_3steps             1.21  s
  pair_episode_S11_3steps              1.37  mo_sum
  episode256_S64_1step                 1.00  s
  episode256_S152_3steps               1.50  mo_sumsq
  episode512_152x64                    1.00  mo_sumsq
  episode512_376x256                   0.89  behv
  episode512_64x24                     1.23  mo_sumsq
  episode512_S11_goalless_binned       1.00  s
  episode512_S27_goal                  1.13  s
  wiring_step                          0.91  rew_total
  wiring_split                         0.91  rew_total
  wiring_pair                          0.94  rew_total
  wiring_fp8                           1.00  rew_total
  wiring_episode                       0.91  rew_total
  wiring_pair_episode                  0.94  rew_total
  wiring_noiseless                     0.70  s
  wiring_noiseless_pair                0.70  s
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import (ERR_FACTOR, STATE_KEYS, bf16_bits_to_f64, e4m3_byte_to_f64,
                            err_scale, f32_to_bf16_bits,
                            f32_to_e4m3_byte, fp8_byte_position, loco_rollout, n_params,
                            pair_member_rows, top2_logit_gap)

pytestmark = pytest.mark.gpu

OB_CLIP = 5.0
ENV_SCALARS = dict(leak=0.35, ctrl=0.05, alive_bonus=1.0, fall_thr=0.0, dt=0.07)


def C(kernel, S, hidden, seed=0, adim=3, goal=0, terminate=1, bins=0, act_mode=0,
      members=6, eps=1, sigma=0.02, n_steps=1, G=0, block=256, member_base=0, wrow0=0,
      ac_std=0.0, seed_dev=None, salt=1, salt_base=0, noiseless_from=0):
    """Noise (tests/test_kernel_oracle_noise.py): ac_std, seed_dev (None: a
    null pointer), noiseless_from, and `salt` for the per-step entry points or
    `salt_base` for the episode ones. The defaults are noise off."""
    return dict(kernel=kernel, S=S, hidden=hidden, seed=seed, adim=adim, goal=goal,
                terminate=terminate, bins=bins, act_mode=act_mode, members=members,
                eps=eps, sigma=sigma, n_steps=n_steps, G=G, block=block,
                member_base=member_base, wrow0=wrow0, ac_std=ac_std, seed_dev=seed_dev,
                salt=salt, salt_base=salt_base, noiseless_from=noiseless_from)


# `members` counts evaluation slots (step/split/episode) or pairs (pair kernels)
CASES = {
    # ---- es_loco_step: every state dim
    "step_S8": C("step", 8, 16, adim=2, seed=1),
    "step_S64": C("step", 64, 16, eps=2),
    "step_S144": C("step", 144, 16),
    "step_S152": C("step", 152, 64),
    "step_S376": C("step", 376, 64, adim=17),
    "step_S11_scalar": C("step", 11, 16),
    "step_S17_scalar": C("step", 17, 64, adim=6),
    "step_S27_goal": C("step", 27, 16, adim=8, goal=1),
    "step_S63": C("step", 63, 64),
    "step_S64_binned": C("step", 64, 16, bins=5, seed=1),
    "step_S11_mode2": C("step", 11, 16, act_mode=2),
    "step_S152_mode3_noterm": C("step", 152, 16, act_mode=3, terminate=0, seed=1),
    # ---- es_loco_step_split: G x S, 11 slots leave a tail block for every G
    "split_G2_S8": C("split", 8, 16, adim=2, G=2, members=11),
    "split_G4_S64": C("split", 64, 16, G=4, members=11),
    "split_G5_S152": C("split", 152, 64, G=5, members=11),
    "split_G8_S376": C("split", 376, 64, adim=17, G=8, members=11),
    "split_G5_S144_goal": C("split", 144, 16, G=5, members=11, goal=1),
    # ---- es_loco_pair_step (bf16 sigma*eps rows)
    "pair_S8": C("pair", 8, 16, adim=2, members=3),
    "pair_S144_eps2": C("pair", 144, 16, members=3, eps=2, sigma=0.05),
    "pair_S152": C("pair", 152, 64, members=4),
    "pair_S376": C("pair", 376, 64, adim=17, members=3, sigma=0.05),
    "pair_S11_scalar": C("pair", 11, 16, members=4),
    "pair_S27_goal_binned": C("pair", 27, 16, adim=4, goal=1, bins=3, members=4),
    "pair_S64_mode2": C("pair", 64, 64, act_mode=2, members=3),
    # ---- es_loco_pair_step_fp8 (interleaved e4m3 sigma*eps rows)
    "fp8_S64": C("fp8", 64, 16, members=3, adim=8, seed=2),
    "fp8_S152_eps2": C("fp8", 152, 64, members=3, eps=2, sigma=0.05, adim=8),
    "fp8_S376": C("fp8", 376, 64, adim=17, members=3),
    "fp8_S27_goal_plain_row0": C("fp8", 27, 16, adim=8, goal=1, members=4),
    "fp8_S63_I2_lt_PART": C("fp8", 63, 64, members=3, sigma=0.05),
    "fp8_S17_scalar_dyn": C("fp8", 17, 64, adim=6, members=3),
    # ---- es_loco_pair_episode
    "pair_episode_S152_1step": C("pair_episode", 152, 16, members=3),
    "pair_episode_S152_3steps": C("pair_episode", 152, 16, members=3, n_steps=3, eps=2),
    "pair_episode_S11_3steps": C("pair_episode", 11, 16, members=4, n_steps=3,
                                 sigma=0.05, seed=1),
    # ---- es_loco_episode, 256 threads, sub-range of slots on a sub-blob
    "episode256_S64_1step": C("episode", 64, 16, members=8, eps=2, member_base=4,
                              wrow0=2),
    "episode256_S152_3steps": C("episode", 152, 64, members=8, n_steps=3, member_base=3,
                                wrow0=3),
    # ---- es_loco_episode, 512 threads: first layers (152,64) (376,256) (64,24)
    # and a scalar head of 17
    "episode512_152x64": C("episode", 152, 64, adim=17, members=6, block=512,
                           member_base=2, wrow0=2),
    "episode512_376x256": C("episode", 376, 256, adim=17, members=5, block=512,
                            n_steps=3, member_base=1, wrow0=1),
    "episode512_64x24": C("episode", 64, 24, adim=17, members=6, block=512, n_steps=3,
                          eps=2, member_base=2, wrow0=1),
    "episode512_S11_goalless_binned": C("episode", 11, 16, bins=5, members=6, block=512,
                                        member_base=3, wrow0=3),
    "episode512_S27_goal": C("episode", 27, 16, adim=8, goal=1, members=6, block=512,
                             n_steps=3, member_base=2, wrow0=2),
}

def case_dims(c):
    out = c["adim"] * c["bins"] if c["bins"] > 1 else \
        c["adim"] + 1 if c["act_mode"] == 2 else \
        2 * c["adim"] if c["act_mode"] == 3 else c["adim"]
    return [c["S"] + 2 * c["goal"], c["hidden"], out]


# layouts handed to the fp8 pair kernel (tests/test_oracle64_cpu.py checks
# that GpuEngine._fp8_layout_ok accepts each)
FP8_LOCO_DIMS = {k: case_dims(c) for k, c in CASES.items() if c["kernel"] == "fp8"}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ------------------------------------------------------------ case construction
def _bf16_blob(rng, dims, rows, scale=None):
    n = n_params(dims)
    stride = (n + 15) // 16 * 16
    w = np.zeros((rows + 1, stride), dtype=np.float32)      # +1 guard row
    off = 0
    for I, O in zip(dims[:-1], dims[1:]):
        sc = (0.7 / np.sqrt(I)) if scale is None else scale
        w[:rows, off:off + I * O] = rng.randn(rows, I * O) * sc
        off += I * O
        w[:rows, off:off + O] = rng.randn(rows, O) * (0.1 if scale is None else scale)
        off += O
    bits = f32_to_bf16_bits(w)
    return bits, bf16_bits_to_f64(bits)[:, :n], stride


def build(name, cases=CASES):
    """Numpy inputs of a case: env matrices, initial state, weight blobs and
    the oracle's policy/env dicts. No GPU work."""
    c = cases[name]
    rng = np.random.RandomState(1000 + sum(ord(ch) for ch in name) + 7919 * c["seed"])
    S, A, g = c["S"], c["adim"], c["goal"]
    dims = case_dims(c)
    D = dims[0]
    n = n_params(dims)
    paired = c["kernel"] in ("pair", "fp8", "pair_episode")
    nslots = 2 * c["members"] * c["eps"] if paired else c["members"]

    A_bits = f32_to_bf16_bits((rng.randn(S, S) * (1.1 / np.sqrt(S))).astype(np.float32))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    env = dict(A_bits=A_bits, A=bf16_bits_to_f64(A_bits),
               B=f32(rng.randn(A, S) / np.sqrt(A)), b0=f32(rng.randn(S) * 0.1),
               wv=f32(rng.randn(S) / np.sqrt(S)), wa=f32(rng.randn(A) / np.sqrt(A)),
               wy=f32(rng.randn(S) / np.sqrt(S)), wh=f32(rng.randn(S) / np.sqrt(S)),
               terminate=c["terminate"], goal=g, **ENV_SCALARS)
    alive = (np.arange(nslots) % 3 != 1).astype(np.float32)   # mixed 0/1
    rng.shuffle(alive)
    state = dict(
        s=f32(rng.randn(nslots, S) * 0.6), pos=f32(rng.randn(nslots, 3)),
        goal=f32(rng.randn(nslots, 2) * 8.0) if g else None, alive=alive,
        rew_total=f32(rng.randn(nslots) * 3.0),
        member_steps=f32(rng.randint(0, 40, size=nslots)),
        behv=f32(rng.randn(nslots, 3)), mo_sum=f32(rng.randn(nslots, D) * 2.0),
        mo_sumsq=f32(rng.rand(nslots, D) * 3.0))
    obmean = f32(rng.randn(D) * 0.2)
    obstd = f32(rng.rand(D) * 0.5 + 0.3)
    obstd[::5] = 0.05          # some dims clip at +-OB_CLIP

    blobs = {}
    if paired:
        tbits, tvals, stride = _bf16_blob(rng, dims, 1)
        pairs = c["members"]
        e = (rng.randn(pairs, n) * c["sigma"]).astype(np.float32)
        if c["kernel"] == "fp8":
            ebytes = f32_to_e4m3_byte(e)
            evals = e4m3_byte_to_f64(ebytes)
            blob = np.zeros((pairs + 1, stride), dtype=np.uint8)
            blob[:pairs, fp8_byte_position(dims)] = ebytes
            blobs["eps"] = blob
        else:
            ebits = np.zeros((pairs + 1, stride), dtype=np.uint16)
            ebits[:pairs, :n] = f32_to_bf16_bits(e)
            evals = bf16_bits_to_f64(ebits[:pairs, :n])
            blobs["eps"] = ebits
        blobs["theta"] = tbits
        rows = pair_member_rows(tvals[0], evals)
        wrow0, members = 0, np.arange(nslots)
    else:
        if c["kernel"] == "episode":
            members = np.arange(c["member_base"], nslots)
        else:
            members = np.arange(nslots)
        nrows = int(members.max()) // c["eps"] - c["wrow0"] + 1
        wbits, rows, stride = _bf16_blob(rng, dims, nrows)
        rows = rows[:nrows]
        blobs["weights"] = wbits
        wrow0 = c["wrow0"]
        assert (members // c["eps"] - wrow0).min() == 0
    policy = dict(dims=dims, weight_rows=rows, obmean=obmean, obstd=obstd,
                  ob_clip=OB_CLIP, eps=c["eps"], wrow0=wrow0, act_mode=c["act_mode"],
                  bins=c["bins"])
    return dict(c=c, name=name, dims=dims, stride=stride, env=env, state=state,
                obmean=obmean, obstd=obstd, blobs=blobs, policy=policy, members=members,
                nslots=nslots)


EPISODE_KERNELS = ("episode", "pair_episode")


def case_noise(c):
    """(noise dict, salt_base) the oracle gets for a case: step t of an
    episode kernel draws with salt_base + t, a per-step launch with `salt`."""
    noise = dict(seed=c["seed_dev"], ac_std=c["ac_std"],
                 noiseless_from=c["noiseless_from"])
    return noise, c["salt_base"] if c["kernel"] in EPISODE_KERNELS else c["salt"] - 1


def oracle(case, with_infos=False):
    """(y64 state, E32 per buffer over the stepped slots); asserts that no
    discrete outcome sits on a rounding edge."""
    c, m = case["c"], case["members"]
    env = {k: v for k, v in case["env"].items() if k != "A_bits"}
    noise, salt_base = case_noise(c)
    y64, infos = loco_rollout(case["state"], env, case["policy"], c["n_steps"], m,
                              np.float64, noise, salt_base)
    y32, _ = loco_rollout(case["state"], env, case["policy"], c["n_steps"], m, np.float32,
                          noise, salt_base)
    e32 = {k: err_scale(y32[k][m], y64[k][m]) for k in STATE_KEYS}
    for info in infos:
        assert (np.abs(info["h"] - np.float32(env["fall_thr"])) > 1e-3).all(), \
            "h on the fall threshold"
        if c["bins"] > 1:
            assert top2_logit_gap(info["net_out"], c["bins"]) > 1e-3, "logit tie"
    if c["terminate"]:
        was = case["state"]["alive"][m] > 0
        now = y64["alive"][m] > 0
        assert (was & ~now).any() and (was & now).any(), \
            "need both terminated and surviving members"
    if with_infos:
        return y64, e32, infos
    return y64, e32


# -------------------------------------------------------------------- launching
def bf16_tensor(bits, dev):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()) \
        .view(torch.bfloat16).to(dev)


def launch(dev, case):
    """Upload, run the case's kernel once, return the state as numpy."""
    from es_pytorch_amd import ops
    lib = ops.hip()
    c, env = case["c"], case["env"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = {k: t(v) for k, v in case["state"].items() if v is not None}
    ev = {k: t(env[k]) for k in ("B", "b0", "wv", "wa", "wy", "wh")}
    A_d = bf16_tensor(env["A_bits"], dev)
    mean_d, std_d = t(case["obmean"]), t(case["obstd"])
    acstd = torch.full((1,), c["ac_std"], dtype=torch.float32, device=dev)
    seed_d = None if c["seed_dev"] is None else t(np.array([c["seed_dev"]], np.int64))
    dims_arr = np.array(case["dims"], dtype=np.int32)
    goal_ptr = st["goal"].data_ptr() if c["goal"] else None
    bufs = (st["s"].data_ptr(), st["pos"].data_ptr(), goal_ptr, A_d.data_ptr(),
            ev["B"].data_ptr(), ev["b0"].data_ptr(), ev["wv"].data_ptr(),
            ev["wa"].data_ptr(), ev["wy"].data_ptr(), ev["wh"].data_ptr(),
            st["alive"].data_ptr(), st["rew_total"].data_ptr(),
            st["member_steps"].data_ptr(), st["behv"].data_ptr(),
            st["mo_sum"].data_ptr(), st["mo_sumsq"].data_ptr())
    flags = (c["S"], c["adim"], c["goal"], c["terminate"], c["noiseless_from"], c["bins"],
             c["eps"], c["act_mode"])
    scal = tuple(float(env[k]) for k in ("leak", "ctrl", "alive_bonus", "fall_thr", "dt"))
    head = (mean_d.data_ptr(), std_d.data_ptr(), dims_arr.ctypes.data, len(dims_arr),
            None if seed_d is None else seed_d.data_ptr())
    tail = (OB_CLIP, acstd.data_ptr(), case["stride"])
    k = c["kernel"]
    keep = []
    if k in ("step", "split"):
        w = bf16_tensor(case["blobs"]["weights"], dev)
        args = (w.data_ptr(),) + head + (c["salt"],) + tail + bufs + (case["nslots"],) + \
            flags + scal
        if k == "step":
            rc = lib.es_loco_step(*args, _stream(dev))
        else:
            scratch = torch.zeros(case["nslots"] * 64, dtype=torch.float32, device=dev)
            keep.append(scratch)
            rc = lib.es_loco_step_split(*args, scratch.data_ptr(), c["G"], _stream(dev))
    elif k in ("pair", "fp8", "pair_episode"):
        th = bf16_tensor(case["blobs"]["theta"], dev)
        ep = t(case["blobs"]["eps"]) if k == "fp8" else \
            bf16_tensor(case["blobs"]["eps"], dev)
        pre = (th.data_ptr(), ep.data_ptr()) + head
        post = bufs + (c["members"],) + flags + scal
        if k == "pair_episode":
            rc = lib.es_loco_pair_episode(*pre, *tail, *post, c["n_steps"], c["salt_base"],
                                          _stream(dev))
        else:
            fn = lib.es_loco_pair_step_fp8 if k == "fp8" else lib.es_loco_pair_step
            assert c["n_steps"] == 1
            rc = fn(*pre, c["salt"], *tail, *post, _stream(dev))
    else:
        w = bf16_tensor(case["blobs"]["weights"], dev)
        mb = c["member_base"]
        rc = lib.es_loco_episode(w.data_ptr(), *head, c["n_steps"], *tail, *bufs, mb,
                                 case["nslots"] - mb, c["salt_base"], c["wrow0"], *flags,
                                 *scal, c["block"], _stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    out = {kk: st[kk].cpu().numpy() for kk in STATE_KEYS}
    del keep
    return out


def compare(label, got, y64, e32, state0, members):
    """Continuous buffers within 16 E32; counters, alive, everything a dead
    member owns and every slot outside `members` exact."""
    m = members

    def ratio(k):
        d = float(np.max(np.abs(got[k][m].astype(np.float64) - y64[k][m])))
        return 0.0 if d == 0.0 else d / e32[k] if e32[k] > 0 else np.inf

    for k in STATE_KEYS:
        assert np.isfinite(got[k][m]).all(), (label, k)
        print(f"ORACLE-RATIO loco {label} {k} ratio={ratio(k):.2f} E32={e32[k]:.3g}")
    print(f"ORACLE-RATIO loco {label} WORST ratio={max(ratio(k) for k in STATE_KEYS):.2f}")
    assert np.array_equal(got["member_steps"][m], y64["member_steps"][m]), label
    assert np.array_equal(got["alive"][m], y64["alive"][m]), label
    dead = m[state0["alive"][m] == 0]
    assert dead.size, "case needs dead members"
    for k in ("behv", "rew_total", "mo_sum", "mo_sumsq", "member_steps", "alive"):
        assert np.array_equal(got[k][dead], state0[k][dead]), (label, k, "dead moved")
    rest = np.setdiff1d(np.arange(state0["s"].shape[0]), m)
    for k in STATE_KEYS:
        assert np.array_equal(got[k][rest], state0[k][rest]), (label, k, "untouched slot")
    for k in STATE_KEYS:
        assert ratio(k) <= ERR_FACTOR, (label, k, ratio(k), e32[k])


@pytest.mark.parametrize("name", list(CASES))
def test_loco_kernel_matches_oracle(dev, name):
    case = build(name)
    y64, e32 = oracle(case)
    got = launch(dev, case)
    compare(name, got, y64, e32, case["state"], case["members"])


# ---------------------------------------------------------------- engine wiring
def _engine(dev, mode):
    from es_pytorch_amd.config import AttrDict
    from es_pytorch_amd.core.engine import GpuEngine
    from es_pytorch_amd.core.noisetable import NoiseTable
    from es_pytorch_amd.core.policy import Policy
    from es_pytorch_amd.envs import make_batched
    from es_pytorch_amd.nn.nn import FeedForward
    from es_pytorch_amd.nn.optimizers import Adam
    from es_pytorch_amd.parallel.comm import Comm

    torch.manual_seed(31)
    pop, eps, std, name = 6, 2, 0.05, "Swimmer-v3"
    comm = Comm(dev)
    cfg = AttrDict({"env": {"name": name, "max_steps": 1},
                    "noise": {"tbl_size": 200_000, "std": std},
                    "policy": {"layer_sizes": [16], "ac_std": 0.0, "l2coeff": 0.005,
                               "lr": 0.01, "ob_clip": 5, "save_obs_chance": 1.0},
                    "general": {"policies_per_gen": pop, "batch_size": 500, "seed": 3,
                                "eps_per_policy": eps, "dyn_group": 4}})
    env = make_batched(name, (pop + 1) * eps, dev, max_steps=1, terminate_on_fall=True)
    nn = FeedForward([16], torch.nn.Tanh(), env, 0.0, 5)
    policy = Policy(nn, std, Adam(len(Policy.get_flat(nn)), 0.01))
    nt = NoiseTable.create_shared(comm, 200_000, len(policy), seed=7, device=dev)
    eng = GpuEngine(cfg, comm, policy, nt, env, np.random.RandomState(5), use_graph=False,
                    split_dyn=(mode == "split"),
                    pair_rollout=mode in ("pair", "fp8", "pair_episode", "noiseless_pair"),
                    eps_fp8=(mode == "fp8"))
    assert eng.fused and eng.split_dyn == (mode == "split")
    assert eng.eps_fp8 == (mode == "fp8")
    return eng


def _bits(tensor):
    return tensor.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def wiring_setup(dev, mode, ac_std=0.0, seed_dev=None):
    """An engine of `mode` on a registry env with a prescribed state in its
    own buffers; the oracle's inputs are read back from those buffers.
    Returns (eng, state, tensors, members, policy, envd)."""
    eng = _engine(dev, mode)
    env = eng.env
    env.dt, env.ctrl_cost, env.leak, env.alive_bonus = 0.07, 0.05, 0.35, 1.0
    rng = np.random.RandomState(17)
    B, S, D, n = eng.B, env.sdim, env.ob_dim, eng.n
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    eng._upload_offsets()
    eng.acstd_dev.fill_(ac_std)
    if seed_dev is not None:
        eng.seed_dev.copy_(torch.tensor([seed_dev], dtype=torch.int64))
    eng._pheno()
    alive = (np.arange(B) % 3 != 1).astype(np.float32)
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

    # oracle inputs are read back from the engine's own buffers
    mm = (eng.M - 1) * eng.eps
    if eng.pair_rollout:
        tvals = bf16_bits_to_f64(_bits(eng.theta_row))[0, :n]
        if eng.eps_fp8:
            evals = e4m3_byte_to_f64(
                eng.eps_rows.cpu().numpy()[:, fp8_byte_position(eng.dims)])
        else:
            evals = bf16_bits_to_f64(_bits(eng.eps_rows))[:, :n]
        rows = np.concatenate([pair_member_rows(tvals, evals), tvals[None, :]])
    else:
        rows = bf16_bits_to_f64(_bits(eng.weights))[:, :n]
    members = np.arange(mm, B) if mode.startswith("noiseless") else np.arange(mm)
    policy = dict(dims=list(eng.dims), weight_rows=rows, obmean=obmean, obstd=obstd,
                  ob_clip=5.0, eps=eng.eps, wrow0=0, act_mode=0, bins=0)
    envd = dict(A=bf16_bits_to_f64(_bits(env.A_bf16)), B=env.B.cpu().numpy(),
                b0=env.b0.cpu().numpy(), wv=env.wv.cpu().numpy(), wa=env.wa.cpu().numpy(),
                wy=env.wy.cpu().numpy(), wh=env.wh.cpu().numpy(), leak=env.leak,
                ctrl=env.ctrl_cost, alive_bonus=env.alive_bonus, dt=env.dt, terminate=1,
                goal=0, fall_thr=0.0)
    return eng, state, tensors, members, policy, envd


def wiring_reference(eng, state, policy, envd, members, n_steps=1, noise=None,
                     salt_base=0):
    """Sets the fall threshold (engine env and envd) and returns (y64, E32).

    Threshold: centre of the widest gap in the oracle's first-step h over the
    live stepped slots, so both outcomes occur, that keeps every h of every
    step more than 1e-3 away (h does not depend on the threshold)."""
    roll = lambda dt: loco_rollout(state, envd, policy, n_steps, members, dt, noise,
                                   salt_base)
    _, infos = roll(np.float64)
    hs = np.sort(infos[0]["h"][state["alive"][members] > 0])
    all_h = np.concatenate([info["h"] for info in infos])
    if hs.size > 1:
        mids = 0.5 * (hs[:-1] + hs[1:])
        order = np.argsort(-np.diff(hs), kind="stable")
        thr = next(float(np.float32(mids[j])) for j in order
                   if (np.abs(all_h - np.float32(mids[j])) > 1e-3).all())
    else:
        thr = float(np.float32(hs[0] + 0.25))   # one live slot (noiseless member): it falls
    eng.env.fall_threshold = envd["fall_thr"] = thr
    y64, infos = roll(np.float64)
    y32, _ = roll(np.float32)
    for info in infos:
        assert (np.abs(info["h"] - envd["fall_thr"]) > 1e-3).all()
    e32 = {k: err_scale(y32[k][members], y64[k][members]) for k in STATE_KEYS}
    return y64, e32


def wiring_state(tensors):
    return {k: tt.cpu().numpy() for k, tt in tensors.items()}


@pytest.mark.parametrize("mode", ["step", "split", "pair", "fp8", "episode",
                                  "pair_episode", "noiseless", "noiseless_pair"])
def test_engine_wiring_one_step(dev, mode):
    """The engine's own launch wrappers, one step on a registry env: pins the
    40-argument call order that the direct calls above bypass. Every env
    scalar is distinct so a swapped pair of arguments shows."""
    eng, state, tensors, members, policy, envd = wiring_setup(dev, mode)
    mm = (eng.M - 1) * eng.eps
    y64, e32 = wiring_reference(eng, state, policy, envd, members)

    if mode in ("step", "split", "pair", "fp8"):
        eng._loco_step(0)
    elif mode == "episode":
        eng._loco_episode(0, mm, mm)
    elif mode == "pair_episode":
        eng._loco_pair_episode()
    else:
        eng._loco_noiseless_episode()
    torch.cuda.synchronize(dev)
    compare(f"wiring_{mode}", wiring_state(tensors), y64, e32, state, members)
