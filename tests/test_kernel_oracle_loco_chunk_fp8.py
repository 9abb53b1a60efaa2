"""es_loco_pair_episode_fp8 — the fp8 pair rollout running several env steps
per launch (rollout_loco.hip, loco_pair_chunk_fp8_kernel) — against the
float64 oracle and, bitwise, against per-step launches.

Helpers and criterion are those of test_kernel_oracle_loco.py: continuous
buffers within ``16 * E32`` of the oracle, ``member_steps``, ``alive`` and
everything a dead member owns exact. Three steps, 2-3 pairs, 256 threads.

The kernel has four instantiations (es_loco_pair_episode_fp8_config): sized
for 3 or 4 blocks per CU, and with or without the state carried in LDS between
the steps of a launch. With the carry on, steps 2.. read the raw state and the
normalized observation that the previous step's epilogue left in LDS instead
of reloading them; S % 8 != 0 falls back to the reload.

  case            what it exercises
  S152            dynamics A ring with a drain residue
  S256            two ring turns, one output per thread
  S11_scalar      scalar dynamics fallback: the carry must fall back
  S32_goal        goal dims of the carried observation (D = 34)
  S152_eps2       two episodes per pair
  S64_binned      adim 16 x 16 bins head (256 outputs; the head's output and
                  the carried observation share an LDS buffer)
  S152_noise      ac_std = 0.3, salt_base = 5: step i draws with salt 5 + i

Data seeds are chosen on the CPU (test_chunk_case_conditions): in every case
a member terminates before the last step and one survives all three.

Measured on MI355X, worst buffer's max |err| / E32 per case (bound: 16), the
same for the 3- and the 4-block variant with the carry on (the four variants
are bitwise equal):

  S152 1.05 | S256 1.13 | S11_scalar 1.45 | S32_goal 1.00 | S152_eps2 1.00 |
  S64_binned 1.19 | S152_noise 1.34
"""
import functools

import numpy as np
import pytest
import torch

from tests import test_kernel_oracle_loco as tl
from tests.oracle64 import STATE_KEYS
from tests.test_kernel_oracle_loco import C, compare, oracle

N_STEPS = 3
SEED_DEV = 0x123456789ABCDEF0
VARIANTS = [(3, 1), (3, 0), (4, 1), (4, 0)]   # (blocks per CU, carry)


def K(S, hidden, salt_base=0, **kw):
    # an "fp8" case (tl.build lays out the e4m3 rows) stepped N_STEPS times;
    # tl.case_noise hands the oracle salt - 1 as the salt base
    return C("fp8", S, hidden, n_steps=N_STEPS, salt=salt_base + 1, **kw)


CASES = {
    "S152": K(152, 16, adim=8, members=3, seed=0),
    "S256": K(256, 16, adim=8, members=3, seed=0),
    "S11_scalar": K(11, 16, members=3, seed=0),
    "S32_goal": K(32, 16, adim=8, goal=1, members=3, seed=0),
    "S152_eps2": K(152, 64, adim=8, eps=2, members=2, sigma=0.05, seed=0),
    "S64_binned": K(64, 16, adim=16, bins=16, members=3, seed=0),
    "S152_noise": K(152, 16, adim=8, members=3, ac_std=0.3, seed_dev=SEED_DEV,
                    salt_base=5, noiseless_from=5, seed=0),
}
# data seeds at which the oracle's own checks and those of
# test_chunk_case_conditions hold
for _name, _seed in (("S256", 2),):
    CASES[_name]["seed"] = _seed

FP8_DIMS = {k: tl.case_dims(c) for k, c in CASES.items()}


def build(name):
    """tests.test_kernel_oracle_loco.build for a case of this file (that
    build() looks its case up in its own table)."""
    key = "chunk_fp8_" + name
    assert key not in tl.CASES
    tl.CASES[key] = CASES[name]
    try:
        return tl.build(key)
    finally:
        del tl.CASES[key]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, y64, E32, infos); no GPU work. Callers must not modify it."""
    case = build(name)
    y64, e32, infos = oracle(case, with_infos=True)
    return case, y64, e32, infos


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def variant_config():
    """Selects a kernel variant; the library's default comes back afterwards."""
    from es_pytorch_amd import ops
    lib = ops.hip()

    def select(blocks, carry):
        assert lib.es_loco_pair_episode_fp8_config(blocks, carry) == 0
    yield select
    assert lib.es_loco_pair_episode_fp8_config(0, 0) == 0


# ------------------------------------------------------------------- CPU checks
def test_fp8_layouts_accepted():
    from es_pytorch_amd.core.engine import GpuEngine
    for key, dims in FP8_DIMS.items():
        assert GpuEngine._fp8_layout_ok(dims), key


@pytest.mark.parametrize("name", list(CASES))
def test_chunk_case_conditions(name):
    """Inputs of a case: a live member terminates before the last step, one
    survives every step, some start dead (oracle() itself asserts that no h
    sits on the fall threshold and no binned logit ties)."""
    case, y64, _, infos = reference(name)
    c, m = case["c"], case["members"]
    assert c["n_steps"] == N_STEPS and len(infos) == N_STEPS
    assert c["terminate"]
    early = np.zeros(len(m), dtype=bool)
    for info in infos[:-1]:
        early |= info["alive_before"] & info["done"]
    assert early.any(), "a member terminates before the last step"
    assert (y64["alive"][m] > 0).any(), "a member survives"
    assert (case["state"]["alive"][m] == 0).any(), "dead members"
    if name == "S11_scalar":
        assert c["S"] % 8 != 0
    else:
        assert c["S"] % 8 == 0
    if c["ac_std"]:
        nf = c["noiseless_from"]
        assert m.min() < nf <= m.max()


# -------------------------------------------------------------------- launching
def _upload(dev, case):
    c, env = case["c"], case["env"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(st={k: t(v) for k, v in case["state"].items() if v is not None},
             ev={k: t(env[k]) for k in ("B", "b0", "wv", "wa", "wy", "wh")},
             A=tl.bf16_tensor(env["A_bits"], dev), mean=t(case["obmean"]),
             std=t(case["obstd"]),
             acstd=torch.full((1,), c["ac_std"], dtype=torch.float32, device=dev),
             seed=None if c["seed_dev"] is None else
             t(np.array([c["seed_dev"]], np.int64)),
             theta=tl.bf16_tensor(case["blobs"]["theta"], dev),
             eps=t(case["blobs"]["eps"]),
             dims=np.array(case["dims"], dtype=np.int32))
    return d


def _args(case, d):
    """(pre, tail, post) of the pair entry points' argument lists."""
    c, env, st, ev = case["c"], case["env"], d["st"], d["ev"]
    goal_ptr = st["goal"].data_ptr() if c["goal"] else None
    bufs = (st["s"].data_ptr(), st["pos"].data_ptr(), goal_ptr, d["A"].data_ptr(),
            ev["B"].data_ptr(), ev["b0"].data_ptr(), ev["wv"].data_ptr(),
            ev["wa"].data_ptr(), ev["wy"].data_ptr(), ev["wh"].data_ptr(),
            st["alive"].data_ptr(), st["rew_total"].data_ptr(),
            st["member_steps"].data_ptr(), st["behv"].data_ptr(),
            st["mo_sum"].data_ptr(), st["mo_sumsq"].data_ptr())
    flags = (c["S"], c["adim"], c["goal"], c["terminate"], c["noiseless_from"], c["bins"],
             c["eps"], c["act_mode"])
    scal = tuple(float(env[k]) for k in ("leak", "ctrl", "alive_bonus", "fall_thr", "dt"))
    pre = (d["theta"].data_ptr(), d["eps"].data_ptr(), d["mean"].data_ptr(),
           d["std"].data_ptr(), d["dims"].ctypes.data, len(d["dims"]),
           None if d["seed"] is None else d["seed"].data_ptr())
    tail = (tl.OB_CLIP, d["acstd"].data_ptr(), case["stride"])
    post = bufs + (c["members"],) + flags + scal
    return pre, tail, post


def _read(dev, d):
    torch.cuda.synchronize(dev)
    return {k: d["st"][k].cpu().numpy() for k in STATE_KEYS}


def launch_chunk(dev, case, n_steps):
    """One es_loco_pair_episode_fp8 launch of n_steps steps."""
    from es_pytorch_amd import ops
    d = _upload(dev, case)
    pre, tail, post = _args(case, d)
    rc = ops.hip().es_loco_pair_episode_fp8(*pre, *tail, *post, n_steps,
                                            case["c"]["salt"] - 1, tl._stream(dev))
    assert rc == 0, rc
    return _read(dev, d)


def launch_steps(dev, case, n_steps):
    """n_steps es_loco_pair_step_fp8 launches, salts salt_base + 1 .. + n_steps."""
    from es_pytorch_amd import ops
    d = _upload(dev, case)
    pre, tail, post = _args(case, d)
    for i in range(n_steps):
        rc = ops.hip().es_loco_pair_step_fp8(*pre, case["c"]["salt"] + i, *tail, *post,
                                             tl._stream(dev))
        assert rc == 0, rc
    return _read(dev, d)


# -------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [3, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_chunk_fp8_matches_oracle(dev, variant_config, name, blocks):
    case, y64, e32, _ = reference(name)
    variant_config(blocks, 1)
    got = launch_chunk(dev, case, N_STEPS)
    compare(f"chunk_fp8_{name}_b{blocks}", got, y64, e32, case["state"], case["members"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("name", list(CASES))
def test_chunk_fp8_bitwise_equals_steps(dev, variant_config, name, k):
    """One launch of k steps = k per-step launches, every output buffer, for
    each of the four variants."""
    case = reference(name)[0]
    ref = launch_steps(dev, case, k)
    for blocks, carry in VARIANTS:
        variant_config(blocks, carry)
        got = launch_chunk(dev, case, k)
        for key in STATE_KEYS:
            np.testing.assert_array_equal(
                got[key], ref[key], err_msg=f"{name} k={k} b{blocks} carry{carry}: {key}")
