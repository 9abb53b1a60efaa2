"""Batched-load paths of the locomotion rollout kernels against the float64
oracle: the scalar-layer walks (mlp_core.h, ES_HEAD_BT = 8 rows per batch),
the action term of the dynamics (rollout_loco.hip, ES_DYN_BM_BT = 16 rows per
batch) and the fused two-member epilogue / obs pass of the pair kernels.

Helpers, criterion and launch code are those of test_kernel_oracle_loco.py:
continuous buffers within ``16 * E32`` of the oracle, ``member_steps``,
``alive`` and everything a dead member owns exact. One step (three for the
episode kernel), 256 threads, a few members.

Scalar-layer walk (head of width O, PART = 256 // O, input width I): the
block-uniform trip count is T = ceil(I / PART); trips 0..T-2 run in batches
of 8, the remainder (T-1) % 8 plus the one trip only some threads own drain
together. Head cases, all with a 17-wide head (PART = 15) unless stated:

  hidden   T   per-thread trips   path
  16 (O=3, PART=85)  1    1 / 0      drain<0>, most partitions empty
  104      7    7 / 6              drain<6>            (Bt-1)
  120      8    8 (all)            drain<7>            (Bt, equal counts)
  128      9    9 / 8              1 batch + drain<0>  (Bt+1 / Bt)
  136     10   10 / 9              1 batch + drain<1>
  248     17   17 / 16             2 batches + drain<0> (2Bt+1)
  256     18   18 / 17             2 batches + drain<1> (flagship head)
  121 on S=64 (first layer, PART=2)  32   3 batches + drain<7>
  130 on S=24 (first layer, PART=1)  24   thread-per-output walk, 2 batches
                                          + drain<7>

Action term: A = 1, 9 (drain only), 16 (one full batch), 17 (batch + 1),
64 (four batches, the most loco_setup allows).

Pair epilogue: S=256 (one output per thread), S=376 (second sweep on 120
threads), S=8 (part of wave 0 holds outputs, the minus member's bookkeeping
lane holds none), goal=1, eps=2. ``alive`` of the pair cases is prescribed:
pair 0 has the plus member alive and the minus dead, pair 1 the reverse.

Measured on MI355X, worst buffer's max |err| / E32 (bound: 16): 0.58-1.72
over the 45 cases; the largest are pair_episode_S256_3steps 1.72,
step_act_A1 1.67, pair_act_A64 1.67, fp8_head_h16_a3 1.44.
"""
import numpy as np
import pytest
import torch

from tests import test_kernel_oracle_loco as tl
from tests.test_kernel_oracle_loco import C, compare, launch, oracle

pytestmark = pytest.mark.gpu

PAIRED = ("pair", "fp8", "pair_episode")


def _head(kernel, hidden, **kw):
    members = 3 if kernel in PAIRED else 6
    return C(kernel, 64, hidden, adim=17, members=members, **kw)


CASES = {}
for _k in ("step", "pair", "fp8"):
    _m = 3 if _k in PAIRED else 6
    # ---- scalar-layer walk trip counts
    CASES[f"{_k}_head_h16_a3"] = C(_k, 64, 16, adim=3, members=_m)
    CASES[f"{_k}_head_h104"] = _head(_k, 104)
    CASES[f"{_k}_head_h120"] = _head(_k, 120, seed=1)
    CASES[f"{_k}_head_h128"] = _head(_k, 128)
    CASES[f"{_k}_head_h136"] = _head(_k, 136, seed=1)
    CASES[f"{_k}_head_h248"] = _head(_k, 248)
    CASES[f"{_k}_head_h256_flagship"] = _head(_k, 256, seed=1)
    CASES[f"{_k}_first_h121_S64"] = C(_k, 64, 121, adim=3, members=_m)
    CASES[f"{_k}_first_h130_S24_part1"] = C(_k, 24, 130, adim=3, members=_m, seed=1)
for _k in ("step", "pair"):
    _m = 3 if _k in PAIRED else 6
    # ---- action-term batching
    for _a in (1, 9, 16, 17, 64):
        CASES[f"{_k}_act_A{_a}"] = C(_k, 64, 16, adim=_a, members=_m, seed=_a % 3)
# ---- fused pair epilogue
CASES["pair_epi_S256"] = C("pair", 256, 16, members=3)
CASES["fp8_epi_S256"] = C("fp8", 256, 16, members=3, seed=1)
CASES["pair_epi_S376_goal_eps2"] = C("pair", 376, 16, adim=17, goal=1, eps=2, members=2)
CASES["fp8_epi_S376_goal_eps2"] = C("fp8", 376, 16, adim=17, goal=1, eps=2, members=2,
                                    seed=1)
CASES["pair_epi_S8_goal"] = C("pair", 8, 16, adim=2, goal=1, members=4)
CASES["pair_epi_S8_eps2"] = C("pair", 8, 16, adim=2, eps=2, members=3, seed=1)
CASES["step_epi_S256_goal"] = C("step", 256, 16, goal=1, members=6)
CASES["pair_episode_S256_3steps"] = C("pair_episode", 256, 16, members=3, n_steps=3)
# data seeds at which the oracle's own case checks hold (both terminated and
# surviving members, no h within 1e-3 of the fall threshold)
for _name, _seed in (("step_head_h256_flagship", 2), ("pair_head_h16_a3", 1),
                     ("fp8_head_h128", 3), ("step_act_A1", 2)):
    CASES[_name]["seed"] = _seed

# layouts handed to the fp8 pair kernel (all accepted by
# GpuEngine._fp8_layout_ok; test_fp8_layouts_accepted checks it without a GPU
# call)
FP8_DIMS = {k: tl.case_dims(c) for k, c in CASES.items() if c["kernel"] == "fp8"}


def build(name):
    """tests.test_kernel_oracle_loco.build for a case of this file. That
    build() looks its case up in its own table, so the case is entered there
    for the duration of the call. Pair cases get a prescribed ``alive``."""
    assert name not in tl.CASES
    tl.CASES[name] = CASES[name]
    try:
        case = tl.build(name)
    finally:
        del tl.CASES[name]
    c = case["c"]
    if c["kernel"] in PAIRED:
        pairs, eps = c["members"], c["eps"]
        alive = np.ones(case["nslots"], dtype=np.float32)
        for e in range(eps):
            alive[(pairs + 0) * eps + e] = 0.0      # pair 0: plus alive, minus dead
            alive[1 * eps + e] = 0.0                # pair 1: plus dead, minus alive
        case["state"]["alive"] = alive
    return case


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def test_fp8_layouts_accepted():
    from es_pytorch_amd.core.engine import GpuEngine
    assert FP8_DIMS
    for key, dims in FP8_DIMS.items():
        assert GpuEngine._fp8_layout_ok(dims), key


@pytest.mark.parametrize("name", list(CASES))
def test_batched_loco_kernel_matches_oracle(dev, name):
    case = build(name)
    y64, e32 = oracle(case)
    got = launch(dev, case)
    compare(name, got, y64, e32, case["state"], case["members"])
