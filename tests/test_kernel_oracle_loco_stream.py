"""Stream loops of the pair rollout kernels (the set rings) against the
float64 oracle: the set ring of the pair A stream (loco_dyn_partials_pair,
rollout_loco.hip) and of the fp8 pair forward's vec layers
(mlp_layers_pair_fp8, mlp_core.h).

Helpers, criterion and launch code are those of test_kernel_oracle_loco.py:
continuous buffers within ``16 * E32`` of the oracle, ``member_steps``,
``alive`` and everything a dead member owns exact. One step, 256 threads,
2-3 pairs (6 members for the one-member ``step`` kernel, whose A stream is
the old loop and is run at the same shapes).

A stream (kernels ``pair`` and ``fp8``). OCT = S / 8, PART = 256 // OCT; a
thread owns n = S // PART rows (nmin) or one more. nmin < 8: the ring is
skipped and the serial tail walks every row. Otherwise 8 rows load up
front, T = (nmin - 8) // 12 whole turns of three 4-row sub-trips run, and
the rem = n - 12 T - 8 rows left (0..12) load ahead of the drain:

  S     PART  n        T   rem     path
  8     256   0 / 1    -   -       tail only, most partitions empty
  64    32    2        -   -       tail only
  120   17    7 / 8    -   -       tail only (ring skipped at nmin = 7)
  128   16    8        0   0       prologue + drain, nothing behind it
  136   15    9 / 10   0   1 / 2
  144   14    10 / 11  0   2 / 3
  152   13    11 / 12  0   3 / 4
  160   12    13 / 14  0   5 / 6
  184   11    16 / 17  0   8 / 9
  192   10    19 / 20  0   11 / 12  longest drain, no turn
  200   10    20       1   0        one turn
  224   9     24 / 25  1   4 / 5
  248   8     31       1   11
  256   8     32       2   0        two turns
  288   7     41 / 42  2   9 / 10
  344   5     68 / 69  5   0 / 1
  376   5     75 / 76  5   7 / 8    flagship

Every drain residue 0..12 occurs, with threads of one block one row apart
wherever n is given as a / b.

fp8 vec forward (kernel ``fp8``; the ``pair`` kernel's bf16 forward is not
changed and runs the first-layer cases as a control). OCT = O / 8,
PART = 256 // OCT; the walk is by row PAIRS of the I - (I & 1) rows behind
the odd row 0; a thread owns n = I2 // PART pairs or one more. nmin < 2: ring
skipped. Otherwise 2 pairs load up front, T = (nmin - 2) // 4 whole turns of
two 2-pair sub-trips run, and rem = n - 4 T - 2 pairs (0..4) drain:

  layer            I     PART  n        T   rem
  first, O = 256   16    8     1        -   -      tail only
                   27    8     1 / 2    -   -      odd I: row-0 path, tail only
                   32    8     2        0   0
                   34 g  8     2 / 3    0   0 / 1  (S = 32, goal-conditioned)
                   35    8     2 / 3    0   0 / 1  odd I
                   48    8     3        0   1
                   64    8     4        0   2
                   66 g  8     4 / 5    0   2 / 3
                   80    8     5        0   3
                   82 g  8     5 / 6    0   3 / 4
                   83    8     5 / 6    0   3 / 4  odd I
                   96    8     6        1   0      one turn
                   130 g 8     8 / 9    1   2 / 3
                   160   8     10       2   0      two turns
                   226 g 8     14 / 15  3   0 / 1  three turns
                   376   8     23 / 24  5   1 / 2  flagship first layer
  hidden, O = I = 64    32    1        -   -      tail only
  hidden, O = I = 128   16    4        0   2
  hidden, O = I = 256   8     16       3   2      flagship hidden layer
                                                   (16 actions x 16 bins)

All 63 cases pass on MI355X with the rings; that they also pass on the
copy-rotated loops the rings replaced was established at commit b3e3cdb,
which still carried those loops behind a preprocessor switch (since
removed). ``build()`` + ``oracle()`` of every case run on the CPU.
"""
import numpy as np
import pytest
import torch

from tests import test_kernel_oracle_loco as tl
from tests.test_kernel_oracle_loco import C, compare, launch, oracle

pytestmark = pytest.mark.gpu

PAIRED = ("pair", "fp8")

CASES = {}
# ---- A stream: every path of the ring, both pair kernels
for _S in (8, 64, 120, 128, 136, 144, 152, 160, 184, 192, 200, 224, 248, 256, 288,
           344, 376):
    for _k in ("pair", "fp8"):
        CASES[f"{_k}_A_S{_S}"] = C(_k, _S, 16, adim=2 if _S == 8 else 3, members=2)
# the one-member kernel at the ring's corner shapes (its loop is unchanged)
for _S in (120, 128, 192, 200, 376):
    CASES[f"step_A_S{_S}"] = C("step", _S, 16, members=6)
# ---- fp8 vec forward, first layer O = 256
for _S, _g in ((16, 0), (27, 0), (32, 0), (32, 1), (35, 0), (48, 0), (64, 0), (64, 1),
               (80, 0), (80, 1), (83, 0), (96, 0), (128, 1), (160, 0), (224, 1),
               (376, 0)):
    CASES[f"fp8_F_I{_S + 2 * _g}"] = C("fp8", _S, 256, goal=_g, members=2)
for _S, _g in ((32, 0), (80, 1), (96, 0), (376, 0)):
    CASES[f"pair_F_I{_S + 2 * _g}"] = C("pair", _S, 256, goal=_g, members=2)
# ---- fp8 vec forward, hidden layer (binned head: O = adim * bins)
CASES["fp8_H_64x64"] = C("fp8", 64, 64, adim=8, bins=8, members=3)
CASES["fp8_H_128x128"] = C("fp8", 64, 128, adim=16, bins=8, members=3)
CASES["fp8_H_256x256"] = C("fp8", 64, 256, adim=16, bins=16, members=2)
CASES["pair_H_128x128"] = C("pair", 64, 128, adim=16, bins=8, members=3)

# data seeds at which the oracle's own case checks hold (both terminated and
# surviving members, no h within 1e-3 of the fall threshold, no logit tie);
# found by running build() + oracle() on the CPU
SEEDS = {"fp8_A_S8": 4, "fp8_A_S64": 1, "fp8_A_S120": 1, "pair_A_S128": 1,
         "fp8_A_S128": 2, "pair_A_S136": 4, "fp8_A_S136": 2, "pair_A_S144": 3,
         "fp8_A_S144": 1, "pair_A_S152": 3, "fp8_A_S160": 1, "pair_A_S184": 2,
         "fp8_A_S192": 1, "fp8_A_S200": 1, "fp8_A_S224": 1, "pair_A_S248": 2,
         "fp8_A_S248": 1, "pair_A_S256": 1, "fp8_A_S288": 2, "pair_A_S376": 4,
         "fp8_A_S376": 2, "fp8_F_I16": 2, "fp8_F_I27": 2, "fp8_F_I35": 3,
         "fp8_F_I48": 2, "fp8_F_I66": 2, "fp8_F_I80": 1, "fp8_F_I82": 2,
         "fp8_F_I83": 3, "fp8_F_I160": 1, "fp8_F_I226": 3, "fp8_F_I376": 2,
         "pair_F_I32": 2, "pair_F_I376": 2, "fp8_H_256x256": 2, "pair_H_128x128": 3}
for _name, _seed in SEEDS.items():
    CASES[_name]["seed"] = _seed

FP8_DIMS = {k: tl.case_dims(c) for k, c in CASES.items() if c["kernel"] == "fp8"}


def build(name):
    """tests.test_kernel_oracle_loco.build for a case of this file (entered in
    that module's table for the duration of the call). Pair cases get a
    prescribed ``alive``: pair 0 plus alive / minus dead, pair 1 the reverse."""
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
            alive[(pairs + 0) * eps + e] = 0.0
            alive[1 * eps + e] = 0.0
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
def test_stream_loco_kernel_matches_oracle(dev, name):
    case = build(name)
    y64, e32 = oracle(case)
    got = launch(dev, case)
    compare(name, got, y64, e32, case["state"], case["members"])
