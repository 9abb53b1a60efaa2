"""The kernels' random numbers against the float64 oracle's own Philox
(tests/oracle64.py: philox4x32_10, normal4, noise_table, action_noise).

The oracle restates the generator from the paper and shares no code with
csrc/philox.h, so a wrong round, key schedule, counter layout, component
order or sin/cos swap cannot sit in both arms. Three groups:

* es_noise_fill against noise_table, every (n, seed, stream) of the grid
  below plus n = 2^23 + 1029, the smallest size that enters the grid-stride
  loop (8192 blocks x 256 threads x 4 elements) and still ends in a ragged
  group. NaN padding behind n stays bit-identical.
* es_mlp_fwd and es_mlp_fwd_f32 with action noise on: every member is
  compared, noisy ones included. Both kernels run the same bf16-exact weight
  values, so one oracle evaluation serves both.
* Every rollout entry point with noise on from a prescribed state, and the
  engine's launch wrappers with seed_dev and acstd_dev set.

Bound as everywhere: ``|kernel - oracle64| <= 16 * E32``; alive,
member_steps, dead members, untouched slots, padding and the binned decode
are exact. tests/test_oracle64_noise_cpu.py checks on the CPU that the cases
meet their input conditions and that each plausible wrong draw would move
the result by more than 100 * 16 * E32.

The nets of the forward cases are [11,16,3] (raw decode) and [11,16,4]
(modes 2 and 3); the binned case needs an output width that 5 divides
([11,16,15]) and the many-outputs case one beyond the block ([11,16,300]).

The counter's high word (group >> 32) would need a table of 2^34 elements and
stays unexercised on the GPU; the oracle's known-answer vectors cover it.

Measured on MI355X, max |err| / E32 (bound: 16):

  table fill (worst over the keys)    ratio
  n = 1, 2, 3, 4, 5 (16 keys each)     2.81
  n = 1027                             1.19
  n = 2^20 + 5                         1.13
  n = 2^23 + 1029 (grid-stride loop)   1.00

  forward case                 es_mlp_fwd  es_mlp_fwd_f32
  mode0_eps1                         0.74            0.74
  mode0_eps2                         0.54            0.54
  mode0_noiseless_from_0             1.83            1.83
  mode0_noiseless_from_B             1.14            1.14
  mode0_null_seed_salt7              0.66            0.66
  mode0_seed_carry                   1.26            1.26
  mode0_A300                         1.03            0.86
  mode2_eps1                         0.99            0.99
  mode2_eps2_acstd_ignored           0.59            0.59
  mode3_eps1                         1.43            1.43
  mode3_eps2                         1.00            1.00
  binned5_no_noise                   0.41            0.41

  rollout case                        ratio  worst buffer
  step_S8                              0.77  pos
  step_S8_null_seed                    1.00  s
  step_S376                            0.75  mo_sumsq
  step_S11_mode2                       1.04  s
  step_S64_mode3                       1.00  mo_sumsq
  step_S64_binned_no_noise             0.90  rew_total
  split_G4_S64                         0.85  mo_sumsq
  pair_S8                              1.17  s
  pair_S64_eps2                        1.06  pos
  fp8_S64                              1.00  mo_sumsq
  pair_episode_S152                    0.97  s
  episode256_S64                       1.02  s
  episode512_S11                       1.00  pos
  f32_step_S8                          0.97  s
  f32_episode_S64                      1.14  s
  wiring_step                          1.91  mo_sumsq
  wiring_split                         1.91  mo_sumsq
  wiring_pair                          1.96  mo_sumsq
  wiring_fp8                           1.54  mo_sumsq
  wiring_episode                       1.01  pos
  wiring_pair_episode                  1.22  s
  wiring_noiseless                     1.57  rew_total
  wiring_noiseless_pair                1.57  rew_total

The wiring rows are the worst of three runs: the registry env's matrices are
salted per process, so their ratios move from run to run; all other rows
repeat to the digit.
"""
import functools

import numpy as np
import pytest
import torch

from tests import oracle64 as o64
from tests import test_kernel_oracle_f32 as tf
from tests import test_kernel_oracle_loco as tl
from tests import test_kernel_oracle_mlp as tm
from tests.oracle64 import (ERR_FACTOR, fp32_error_scale, max_ratio, n_params,
                            noise_table, policy_actions, top2_logit_gap)

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ noise table
TABLE_NS = [1, 2, 3, 4, 5, 1027, 2 ** 20 + 5]
TABLE_SEEDS = [0, 99, 0x123456789ABCDEF0, 2 ** 64 - 1]
TABLE_STREAMS = [0, 1, 0xAC, 0xFFFFFFFF]
TABLE_BIG_N = 8_388_608 + 1029
TABLE_PAD = 8
PAD_BITS = 0x7FC12345          # a NaN with a payload: any write shows


def table_buffer(n):
    """int32 view of n + TABLE_PAD floats, all PAD_BITS."""
    return np.full(n + TABLE_PAD, PAD_BITS, dtype=np.int32)


def check_table(label, got_bits, n, seed, stream):
    """`got_bits`: the int32 buffer after a fill of its first n elements."""
    y64, e32 = fp32_error_scale(noise_table, n, seed, stream)
    got = got_bits.view(np.float32)
    assert (got_bits[n:] == PAD_BITS).all(), (label, "padding overwritten")
    assert np.isfinite(got[:n]).all(), label
    r = max_ratio(got[:n], y64, e32)
    print(f"ORACLE-RATIO noise {label} n={n} seed={seed:#x} stream={stream:#x} "
          f"ratio={r:.2f} E32={e32:.3g}")
    assert r <= ERR_FACTOR, (label, n, seed, stream, r, e32)
    return r


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _gpu_fill(dev, n, seed, stream):
    from es_pytorch_amd import ops
    buf = torch.from_numpy(table_buffer(n)).to(dev)
    rc = ops.hip().es_noise_fill(buf.data_ptr(), n, seed, stream,
                                 torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    return buf.cpu().numpy()


@pytest.mark.parametrize("seed", TABLE_SEEDS)
@pytest.mark.parametrize("n", TABLE_NS)
def test_noise_fill_matches_oracle(dev, n, seed):
    for stream in TABLE_STREAMS:
        check_table("fill", _gpu_fill(dev, n, seed, stream), n, seed, stream)


@pytest.mark.parametrize("seed,stream", list(zip(TABLE_SEEDS, TABLE_STREAMS)))
def test_noise_fill_grid_stride_matches_oracle(dev, seed, stream):
    n = TABLE_BIG_N
    assert (n + 3) // 4 > 8192 * 256 and n % 4 != 0
    check_table("fill_grid_stride", _gpu_fill(dev, n, seed, stream), n, seed, stream)


# ---------------------------------------------------------------- forward cases
FWD_B = 6
SEED_WIDE = 0x123456789ABCDEF0


def F(dims, eps=1, act_mode=0, bins=0, ac_std=None, seed=SEED_WIDE, salt=3,
      noiseless_from=4, net_seed=0):
    return dict(dims=dims, eps=eps, act_mode=act_mode, bins=bins, ac_std=ac_std, seed=seed,
                salt=salt, noiseless_from=noiseless_from, net_seed=net_seed)


# noiseless_from = 4 of 6 slots: slots 0..2 ("plus") and slot 3 (a "minus"
# slot, see minus_to_plus) draw, slots 4 and 5 do not
FWD_CASES = {
    "mode0_eps1": F([11, 16, 3], ac_std=0.3),
    "mode0_eps2": F([11, 16, 3], eps=2, ac_std=0.3, seed=123, salt=4),
    "mode0_noiseless_from_0": F([11, 16, 3], ac_std=0.3, noiseless_from=0),
    "mode0_noiseless_from_B": F([11, 16, 3], ac_std=0.3, noiseless_from=FWD_B),
    "mode0_null_seed_salt7": F([11, 16, 3], ac_std=0.3, seed=None, salt=7),
    "mode0_seed_carry": F([11, 16, 3], ac_std=0.3, seed=0xFFFFFFFF, salt=1),
    "mode0_A300": F([11, 16, 300], ac_std=0.3),
    "mode2_eps1": F([11, 16, 4], act_mode=2),
    "mode2_eps2_acstd_ignored": F([11, 16, 4], eps=2, act_mode=2, ac_std=0.3),
    "mode3_eps1": F([11, 16, 4], act_mode=3),
    "mode3_eps2": F([11, 16, 4], eps=2, act_mode=3, seed=123, salt=4),
    "binned5_no_noise": F([11, 16, 15], bins=5, ac_std=0.3, noiseless_from=FWD_B),
}


def fwd_draws(c):
    """Does the case draw at all?"""
    return c["bins"] <= 1 and c["noiseless_from"] > 0 and \
        (c["act_mode"] in (2, 3) or bool(c["ac_std"]))


def fwd_noise(c):
    return dict(seed=c["seed"], salt=c["salt"], ac_std=c["ac_std"] or 0.0,
                noiseless_from=c["noiseless_from"])


@functools.lru_cache(maxsize=None)
def build_fwd(name):
    """Inputs of a forward case, shared by both kernels: bf16 weight bits and
    the same values as a float32 blob with NaN padding."""
    c = FWD_CASES[name]
    dims, eps = c["dims"], c["eps"]
    rng = np.random.RandomState(sum(ord(ch) for ch in name) + 7919 * c["net_seed"])
    rows = (FWD_B + eps - 1) // eps
    wbits, wvals, stride = tm.make_net(rng, dims, rows)
    n = n_params(dims)
    w32 = wvals[:rows].astype(np.float32)
    w32[:, n:] = np.nan
    assert stride % 4 == 0 and np.array_equal(w32[:, :n].astype(np.float64),
                                              wvals[:rows, :n])
    obs, obmean, obstd = tm.make_obs(rng, FWD_B, dims[0])
    A = dims[-1]
    adim = A - 1 if c["act_mode"] == 2 else A // 2 if c["act_mode"] == 3 else \
        A // c["bins"] if c["bins"] > 1 else A
    alow = arange = None
    if c["bins"] > 1:
        alow = (rng.randn(adim) - 2.0).astype(np.float32)
        arange = (rng.rand(adim) * 3.0 + 0.5).astype(np.float32)
    kw = dict(dims=dims, weight_rows=wvals, obs=obs, obmean=obmean, obstd=obstd,
              ob_clip=tm.OB_CLIP, eps=eps, act_mode=c["act_mode"], bins=c["bins"],
              alow=alow, arange=arange)
    return dict(c=c, name=name, wbits=wbits, w32=w32, stride=stride, obs=obs,
                obmean=obmean, obstd=obstd, adim=adim, alow=alow, arange=arange, kw=kw)


@functools.lru_cache(maxsize=None)
def fwd_reference(name):
    """(y64 actions, E32, net outputs) of a forward case; asserts the case's
    input conditions. No GPU work. Callers must not modify the arrays."""
    case = build_fwd(name)
    c = case["c"]
    y64, e32 = fp32_error_scale(policy_actions, noise=fwd_noise(c), **case["kw"])
    clean, net = policy_actions(**case["kw"])
    nf = c["noiseless_from"]
    # noise-free slots are the noise-free decode, noisy ones are far from it
    assert np.array_equal(y64[nf:], clean[nf:]), name
    if fwd_draws(c):
        assert (np.abs(y64[:nf] - clean[:nf]).max(axis=1) > 1e-3).all(), name
    else:
        assert np.array_equal(y64, clean), name
    if c["bins"] > 1:
        assert top2_logit_gap(net, c["bins"]) > 1e-3, "binned logits on a rounding edge"
    if c["act_mode"] == 3:
        sd = net[:nf, case["adim"]:]
        assert (sd > 0).any() and (sd < 0).any(), "mode 3 needs both signs of the std"
    if c["act_mode"] == 2:
        assert (net[:nf, 0] != 0).all()
    return y64, e32, net


def launch_fwd(dev, case, kind, ac_std="case", noiseless_from=None):
    c = case["c"]
    kw = dict(eps=c["eps"], act_mode=c["act_mode"], bins=c["bins"], alow=case["alow"],
              arange=case["arange"],
              noiseless_from=c["noiseless_from"] if noiseless_from is None else
              noiseless_from,
              ac_std=c["ac_std"] if ac_std == "case" else ac_std, seed=c["seed"],
              salt=c["salt"])
    args = (case["stride"], case["obs"], case["obmean"], case["obstd"], case["adim"])
    if kind == "bf16":
        return tm.launch(dev, c["dims"], case["wbits"], *args, **kw)
    return tf.launch_fwd(dev, c["dims"], case["w32"], *args, **kw)


@pytest.mark.parametrize("kind", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(FWD_CASES))
def test_mlp_fwd_with_noise_matches_oracle(dev, name, kind):
    case = build_fwd(name)
    c = case["c"]
    y64, e32, _ = fwd_reference(name)
    got = launch_fwd(dev, case, kind)
    r = max_ratio(got, y64, e32)
    print(f"ORACLE-RATIO noise fwd_{kind} {name} ratio={r:.2f} E32={e32:.3g}")
    assert np.isfinite(got).all(), name
    assert r <= ERR_FACTOR, (name, kind, r, e32)
    if not fwd_draws(c):
        # nothing may draw: bit for bit the launch with no ac_std and no noisy slot
        quiet = launch_fwd(dev, case, kind, ac_std=None, noiseless_from=0)
        assert np.array_equal(got.view(np.uint32), quiet.view(np.uint32)), name


# ---------------------------------------------------------------- rollout cases
C = tl.C
SEED_DEV = 0x123456789ABCDEF0

# bf16 kernels (tests.test_kernel_oracle_loco.build / launch). `members` counts
# slots, or pairs for the pair kernels; noiseless_from lies strictly inside the
# launched slots and beyond their first half, so a "minus" slot draws too.
LOCO_CASES = {
    "step_S8": C("step", 8, 16, adim=2, ac_std=0.3, seed_dev=SEED_DEV, salt=3,
                 noiseless_from=4, seed=3),
    "step_S8_null_seed": C("step", 8, 16, adim=2, ac_std=0.3, seed_dev=None, salt=7,
                           noiseless_from=4, seed=5),
    "step_S376": C("step", 376, 64, adim=17, ac_std=0.3, seed_dev=0xFFFFFFFF, salt=1,
                   noiseless_from=4, seed=0),
    "step_S11_mode2": C("step", 11, 16, act_mode=2, seed_dev=SEED_DEV, salt=3,
                        noiseless_from=4, seed=1),
    "step_S64_mode3": C("step", 64, 16, act_mode=3, seed_dev=SEED_DEV, salt=3,
                        noiseless_from=4, seed=0),
    "step_S64_binned_no_noise": C("step", 64, 16, bins=5, ac_std=0.3, seed_dev=SEED_DEV,
                                  salt=3, noiseless_from=4, seed=0),
    "split_G4_S64": C("split", 64, 16, G=4, members=11, ac_std=0.3, seed_dev=SEED_DEV,
                      salt=3, noiseless_from=8, seed=0),
    "pair_S8": C("pair", 8, 16, adim=2, members=3, ac_std=0.3, seed_dev=SEED_DEV, salt=3,
                 noiseless_from=5, seed=4),
    "pair_S64_eps2": C("pair", 64, 16, members=3, eps=2, ac_std=0.3, seed_dev=SEED_DEV,
                       salt=3, noiseless_from=9, seed=1),
    "fp8_S64": C("fp8", 64, 16, adim=8, members=3, ac_std=0.3, seed_dev=SEED_DEV, salt=3,
                 noiseless_from=5, seed=1),
    "pair_episode_S152": C("pair_episode", 152, 16, members=3, n_steps=3, ac_std=0.3,
                           seed_dev=SEED_DEV, salt_base=5, noiseless_from=5, seed=7),
    # slots 3..9 of 10: pair (3, 8) draws on both sides, slot 9 does not
    "episode256_S64": C("episode", 64, 16, members=10, n_steps=3, member_base=3, wrow0=3,
                        ac_std=0.3, seed_dev=SEED_DEV, salt_base=5, noiseless_from=9,
                        seed=1),
    "episode512_S11": C("episode", 11, 16, members=6, n_steps=3, block=512, ac_std=0.3,
                        seed_dev=SEED_DEV, salt_base=2, noiseless_from=4, seed=1),
}

# fp32-weights kernels (tests.test_kernel_oracle_f32.build_loco / launch_loco)
F32_LOCO_CASES = {
    "f32_step_S8": tf.C("step", 8, 16, adim=2, ac_std=0.3, seed_dev=SEED_DEV, salt=3,
                        noiseless_from=4, seed=1),
    "f32_episode_S64": tf.C("episode", 64, 16, n_steps=3, ac_std=0.3, seed_dev=SEED_DEV,
                            salt_base=5, noiseless_from=4, seed=1),
}

ALL_LOCO = list(LOCO_CASES) + list(F32_LOCO_CASES)

# the fp8 layouts of this file, for tests/test_oracle64_cpu.py's layout check
FP8_NOISE_DIMS = {k: tl.case_dims(c) for k, c in LOCO_CASES.items() if c["kernel"] == "fp8"}


def loco_draws(c):
    return c["bins"] <= 1 and (c["act_mode"] in (2, 3) or c["ac_std"] != 0)


def build_loco(name):
    if name in F32_LOCO_CASES:
        return tf.build_loco(name, F32_LOCO_CASES)
    return tl.build(name, LOCO_CASES)


def minus_to_plus(slots, nslots):
    """The evaluation slots are laid out [plus half | minus half]: slot
    b + nslots // 2 is the antithetic partner of slot b (for the pair kernels
    bm = bp + pairs * eps). Maps every minus slot to its plus slot."""
    slots = np.asarray(slots)
    half = nslots // 2
    return np.where((slots >= half) & (slots < 2 * half), slots - half, slots)


def loco_rollout_kwargs(case):
    """Arguments of o64.loco_rollout for a case (both builders)."""
    c = case["c"]
    env = {k: v for k, v in case["env"].items() if k != "A_bits"}
    noise, salt_base = tl.case_noise(c)
    return dict(state=case["state"], env=env, policy=case["policy"], n_steps=c["n_steps"],
                members=case["members"], noise=noise, salt_base=salt_base)


@functools.lru_cache(maxsize=None)
def loco_reference(name):
    """(case, y64, E32) of a rollout case. Asserts the conditions of the
    noise-free modules (inside their oracle()) and the noise ones: among the
    noisy live slots some action is clamped and some is not, a plus and a
    minus slot of one pair both draw and their draws differ, and live slots
    lie on both sides of noiseless_from. No GPU work; callers must not modify
    the arrays."""
    case = build_loco(name)
    c, m = case["c"], case["members"]
    orc = tf.loco_oracle if name in F32_LOCO_CASES else tl.oracle
    y64, e32, infos = orc(case, with_infos=True)
    nf = c["noiseless_from"]
    assert m.min() < nf <= m.max(), "noiseless_from inside the launched slots"
    live = case["state"]["alive"][m] > 0
    assert (live & (m < nf)).any() and (live & (m >= nf)).any(), \
        "live slots on both sides of noiseless_from"
    assert (~live).any(), "case needs dead members"
    if not loco_draws(c):
        return case, y64, e32
    raw = np.abs(infos[0]["act_raw"][live & (m < nf)])
    assert (raw > 1.0).any() and (raw < 1.0).any(), "clamped and unclamped noisy actions"
    kw = loco_rollout_kwargs(case)
    seed = o64.noise_seed(dict(kw["noise"], salt=kw["salt_base"] + 1))
    odim = case["dims"][-1]
    minus = m[(m < nf) & (minus_to_plus(m, case["nslots"]) != m)]
    plus = minus_to_plus(minus, case["nslots"])
    ok = np.isin(plus, m)
    assert ok.any(), "a pair with both slots noisy"
    zp = o64.action_draws(seed, plus[ok], odim, c["adim"])
    zm = o64.action_draws(seed, minus[ok], odim, c["adim"])
    assert (np.abs(zp - zm).max(axis=1) > 1e-3).any(), "pair draws differ"
    return case, y64, e32


def compare_loco(name, got, case, y64, e32):
    cmp_ = tf.compare if name in F32_LOCO_CASES else tl.compare
    cmp_(f"noise_{name}", got, y64, e32, case["state"], case["members"])


@pytest.mark.parametrize("name", ALL_LOCO)
def test_loco_kernel_with_noise_matches_oracle(dev, name):
    case, y64, e32 = loco_reference(name)
    if name in F32_LOCO_CASES:
        got = tf.launch_loco(dev, case)
    else:
        got = tl.launch(dev, case)
    compare_loco(name, got, case, y64, e32)


# ---------------------------------------------------------------- engine wiring
WIRING_SEED = 0x12345678FFFFFFFF       # seed + salt carries into the key's high word
WIRING_AC_STD = 0.2


@pytest.mark.parametrize("mode", ["step", "split", "pair", "fp8", "episode",
                                  "pair_episode", "noiseless", "noiseless_pair"])
def test_engine_wiring_with_noise(dev, mode):
    """The engine's launch wrappers with seed_dev and acstd_dev set: two
    per-step launches (salts t + 1 = 1, 2), two-step episode launches with
    salt_base = 2 (salts 3, 4) as under steps_per_launch, and the noiseless
    episode, whose slots must match the noise-free oracle with ac_std on."""
    eng, state, tensors, members, policy, envd = tl.wiring_setup(
        dev, mode, ac_std=WIRING_AC_STD, seed_dev=WIRING_SEED)
    mm = (eng.M - 1) * eng.eps
    noise = dict(seed=WIRING_SEED, ac_std=WIRING_AC_STD, noiseless_from=mm)
    if mode.startswith("noiseless"):
        ref = dict(n_steps=1, noise=None)
    elif mode in ("episode", "pair_episode"):
        ref = dict(n_steps=2, noise=noise, salt_base=2)
    else:
        ref = dict(n_steps=2, noise=noise, salt_base=0)
    y64, e32 = tl.wiring_reference(eng, state, policy, envd, members, **ref)
    if ref["noise"] is not None:
        # the noise matters: the noise-free rollout is far outside the bound
        clean, _ = o64.loco_rollout(state, envd, policy, 2, members)
        assert np.abs(clean["s"][members] - y64["s"][members]).max() > \
            100 * ERR_FACTOR * e32["s"]

    if mode in ("step", "split", "pair", "fp8"):
        eng._loco_step(0)
        eng._loco_step(1)
    elif mode == "episode":
        eng._loco_episode(0, mm, mm, n_steps=2, salt_base=2)
    elif mode == "pair_episode":
        eng._loco_pair_episode(n_steps=2, salt_base=2)
    else:
        eng._loco_noiseless_episode()
    torch.cuda.synchronize(dev)
    tl.compare(f"noise_wiring_{mode}", tl.wiring_state(tensors), y64, e32, state, members)
