"""The STAGE levels of the fp8 multi-step pair kernel (rollout_loco.hip,
loco_pair_chunk_fp8_kernel<MINB, false, STAGE>): operands that cannot change
during a launch are copied to LDS once and read there.

  level 1  obmean, obstd, b0, wv, wy, wh, wa and the layer biases
  level 2  also the last layer's weights when that layer is on the scalar path

Staging moves loads, not arithmetic: for every level and both register
budgets (es_loco_pair_episode_fp8_config 3 / 4; level 2 has one build, used
under both settings) one launch of k steps must equal k per-step
es_loco_pair_step_fp8 launches bit for bit in every state buffer. Cases: the
seven of test_kernel_oracle_loco_chunk_fp8.py (vectorized heads: level 2 has
nothing to add there and runs as level 1) and three with a scalar head:

  S152_head17   [152, 16, 16, 17], adim 17: PART = 256 // 17 = 15, the
                flagship's arm
  S152_head5    adim 5: PART = 51
  S64_head143   13 dims x 11 bins = 143 outputs: PART == 1

The staged levels also meet the float64 oracle at the project's 16 * E32 on
the three new cases. Measured on MI355X, worst buffer's max |err| / E32
(levels 1 and 2, both settings, are bitwise equal, so one figure each):

  S152_head17 1.58 | S152_head5 1.01 | S64_head143 1.30

Level selection (es_loco_pair_episode_fp8_stage): -1 = the highest level, up
to es_loco_pair_episode_fp8_stage_max, at which the whole grid is resident,
since blocks retire only when the launch ends; a forced level that cannot
hold the grid is an error (-110). The library's own cap is 0 (the staged
levels did not clear the project's speed bar), so the tests of the automatic
choice raise it to 2.
"""
import functools

import numpy as np
import pytest
import torch

from tests import test_kernel_oracle_loco as tl
from tests import test_kernel_oracle_loco_chunk_fp8 as tc
from tests.oracle64 import STATE_KEYS
from tests.test_kernel_oracle_loco import compare, oracle
from tests.test_kernel_oracle_loco_chunk_fp8 import K, launch_chunk, launch_steps

LEVELS = [0, 1, 2]
BLOCKS = [3, 4]
LDS_PER_CU = 160 * 1024
LDS_PER_BLOCK_MAX = 64 * 1024

# data seeds chosen on the CPU (test_stage_case_conditions)
NEW_CASES = {
    "S152_head17": dict(K(152, 16, adim=17, members=3, seed=1), dims=[152, 16, 16, 17]),
    "S152_head5": K(152, 16, adim=5, members=3, seed=0),
    "S64_head143": K(64, 16, adim=13, bins=11, members=3, seed=7),
}
HEAD_PART = {"S152_head17": 15, "S152_head5": 51, "S64_head143": 1}
# level 2 holds two blocks per CU, level 1 three or more (test_stage_lds_sizes)
BIG_HEAD = dict(K(64, 256, adim=9, bins=5, seed=0), members=None)
ALL_CASES = list(tc.CASES) + list(NEW_CASES)


_TL_CASE_DIMS = tl.case_dims


def case_dims(c):
    return list(c["dims"]) if "dims" in c else _TL_CASE_DIMS(c)


def build(name, c=None):
    """The numpy inputs of a case of this file or of the chunk test's table.
    tl.build() looks its case up in its own table and lays the net out with
    its own case_dims(); a case with two hidden layers carries `dims`."""
    if c is None and name in tc.CASES:
        return tc.build(name)
    key = "chunk_fp8_stage_" + name
    assert key not in tl.CASES
    tl.CASES[key] = NEW_CASES[name] if c is None else c
    orig = tl.case_dims
    tl.case_dims = case_dims
    try:
        return tl.build(key)
    finally:
        tl.case_dims = orig
        del tl.CASES[key]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, y64, E32, infos); no GPU work. Callers must not modify it."""
    case = build(name)
    y64, e32, infos = oracle(case, with_infos=True)
    return case, y64, e32, infos


@functools.lru_cache(maxsize=None)
def inputs(name):
    return reference(name)[0] if name in NEW_CASES else tc.reference(name)[0]


def vec_ok(dims):
    """mlp_shape_init's vec_ok per layer."""
    out, off = [], 0
    for I, O in zip(dims[:-1], dims[1:]):
        out.append(O % 8 == 0 and O <= 8 * 256 and off % 8 == 0)
        off += I * O + O
    return out


def lds_bytes(c, dims, level):
    """Dynamic LDS of a launch: mlp_pair_lds_bytes + loco_stage_lds_bytes."""
    S, A, D = c["S"], c["adim"], dims[0]
    maxdim = (max(dims) + 3) & ~3
    carve = 2 * (2 * maxdim * 4 + 256 * 8 * 4 + ((S + 3) & ~3) * 4 + 64 * 4)
    if level < 1:
        return carve
    n = 4 * (2 * D + 4 * S + A + 2 * sum(dims[1:]))
    if level >= 2 and not vec_ok(dims)[-1]:
        n += 3 * dims[-2] * dims[-1]
    return carve + ((n + 15) & ~15)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture
def stage_config():
    """Selects a register budget (carry off) and a stage level; the library's
    defaults, automatic level included, come back afterwards."""
    from es_pytorch_amd import ops
    lib = ops.hip()

    def select(blocks, level, auto_max=2):
        assert lib.es_loco_pair_episode_fp8_config(blocks, 0) == 0
        assert lib.es_loco_pair_episode_fp8_stage(level) == 0
        assert lib.es_loco_pair_episode_fp8_stage_max(auto_max) == 0
    yield select
    assert lib.es_loco_pair_episode_fp8_config(0, 0) == 0


def last_stage():
    from es_pytorch_amd import ops
    return ops.hip().es_loco_pair_episode_fp8_last_stage()


# ------------------------------------------------------------------- CPU checks
@pytest.mark.parametrize("name", list(NEW_CASES))
def test_stage_case_conditions(name):
    """The new cases: an accepted fp8 layout whose head is on the scalar path
    at the PART it is meant to exercise, and test_chunk_case_conditions'
    demands on the data (oracle() itself asserts that no h sits on the fall
    threshold and no binned logit ties)."""
    from es_pytorch_amd.core.engine import GpuEngine
    case, y64, _, infos = reference(name)
    c, m, dims = case["c"], case["members"], case["dims"]
    assert dims == case_dims(NEW_CASES[name])
    assert GpuEngine._fp8_layout_ok(dims), dims
    ok = vec_ok(dims)
    assert not ok[-1] and all(ok[:-1]), ok
    assert 256 // dims[-1] == HEAD_PART[name]
    assert c["S"] % 8 == 0 and c["n_steps"] == tc.N_STEPS and c["terminate"]
    early = np.zeros(len(m), dtype=bool)
    for info in infos[:-1]:
        early |= info["alive_before"] & info["done"]
    assert early.any(), "a member terminates before the last step"
    assert (y64["alive"][m] > 0).any(), "a member survives"
    assert (case["state"]["alive"][m] == 0).any(), "dead members"


def test_stage_lds_sizes():
    """The shapes the selection tests rely on, from the LDS sizes alone."""
    # the flagship: levels 1 and 2 leave three blocks per CU (640 blocks on
    # 256 CUs need 2.5), and level 2 is the issue's 25,920 + 26,380 bytes
    flag = dict(S=376, adim=17)
    fdims = [376, 256, 256, 17]
    assert lds_bytes(flag, fdims, 0) == 25920
    assert lds_bytes(flag, fdims, 2) == 25920 + ((26380 + 15) & ~15)
    assert LDS_PER_CU // lds_bytes(flag, fdims, 2) == 3
    # BIG_HEAD: level 2 fits a block's LDS limit but only twice per CU
    dims = case_dims(BIG_HEAD)
    assert not vec_ok(dims)[-1]
    l1, l2 = lds_bytes(BIG_HEAD, dims, 1), lds_bytes(BIG_HEAD, dims, 2)
    assert l2 <= LDS_PER_BLOCK_MAX and LDS_PER_CU // l2 == 2
    assert LDS_PER_CU // l1 >= 4
    # a head too large for one block's LDS at level 2
    huge = [64, 256, 143]
    assert lds_bytes(dict(S=64, adim=13), huge, 2) > LDS_PER_BLOCK_MAX


# -------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("name", ALL_CASES)
def test_stage_bitwise_equals_steps(dev, stage_config, name, k):
    """One launch of k steps at every level and register budget = k per-step
    launches, every state buffer."""
    case = inputs(name)
    ref = launch_steps(dev, case, k)
    for level in LEVELS:
        for blocks in BLOCKS:
            stage_config(blocks, level)
            got = launch_chunk(dev, case, k)
            assert last_stage() == level
            for key in STATE_KEYS:
                np.testing.assert_array_equal(
                    got[key], ref[key], err_msg=f"{name} k={k} b{blocks} stage{level}: {key}")


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", list(NEW_CASES))
def test_stage_matches_oracle(dev, stage_config, name, level, blocks):
    case, y64, e32, _ = reference(name)
    stage_config(blocks, level)
    got = launch_chunk(dev, case, tc.N_STEPS)
    assert last_stage() == level
    compare(f"chunk_fp8_stage{level}_{name}_b{blocks}", got, y64, e32, case["state"],
            case["members"])


def _launch_rc(dev, case, n_steps):
    """launch_chunk without the assertion: (return code, state or None)."""
    from es_pytorch_amd import ops
    d = tc._upload(dev, case)
    pre, tail, post = tc._args(case, d)
    rc = ops.hip().es_loco_pair_episode_fp8(*pre, *tail, *post, n_steps,
                                            case["c"]["salt"] - 1, tl._stream(dev))
    return rc, (tc._read(dev, d) if rc == 0 else None)


@pytest.mark.gpu
def test_forced_level_too_large_for_a_block(dev, stage_config):
    """[64, 256, 143]: the staged head alone exceeds one block's LDS. Forcing
    level 2 is an error, whatever the grid; automatic runs level 1."""
    case = build("huge_head", K(64, 256, adim=13, bins=11, members=2, seed=0))
    stage_config(4, 2)
    rc, _ = _launch_rc(dev, case, 1)
    assert rc == -110
    stage_config(4, -1)
    rc, got = _launch_rc(dev, case, 1)
    assert rc == 0 and last_stage() == 1
    ref = launch_steps(dev, case, 1)
    for key in STATE_KEYS:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)


@pytest.mark.gpu
def test_automatic_falls_back_past_residency(dev, stage_config):
    """BIG_HEAD at 2 * CUs + 1 blocks: level 2 holds two blocks per CU
    (test_stage_lds_sizes), so the grid is not resident there; forced it is
    an error, automatic takes level 1, and the result is level 0's."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    case = build("big_head", dict(BIG_HEAD, members=2 * cus + 1))
    stage_config(4, 2)
    rc, _ = _launch_rc(dev, case, 2)
    assert rc == -110
    stage_config(4, -1)
    rc, got = _launch_rc(dev, case, 2)
    assert rc == 0 and last_stage() == 1
    stage_config(4, 0)
    rc, ref = _launch_rc(dev, case, 2)
    assert rc == 0 and last_stage() == 0
    for key in STATE_KEYS:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
    # one block fewer per CU than level 2 holds: resident, level 2 runs
    small = build("big_head_fits", dict(BIG_HEAD, members=3))
    stage_config(4, -1)
    rc, _ = _launch_rc(dev, small, 2)
    assert rc == 0 and last_stage() == 2


@pytest.mark.gpu
def test_automatic_default_is_level_0(dev, stage_config):
    """Out of the box the automatic choice is capped at level 0."""
    from es_pytorch_amd import ops
    stage_config(4, -1)
    assert ops.hip().es_loco_pair_episode_fp8_config(0, 0) == 0   # the defaults
    launch_chunk(dev, inputs("S152_head17"), 1)
    assert last_stage() == 0
