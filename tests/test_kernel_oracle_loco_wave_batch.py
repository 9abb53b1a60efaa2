"""es_loco_wave_batch_episode / _f32 (a wavefront per member, its E = eps
episodes as the columns of fp32 MFMA products, activations and state in
registers) against the float64 oracle, with the builder, ``reference`` and the
launcher of tests/test_kernel_oracle_loco_batch.py and the comparison and bound
of tests/test_kernel_oracle_loco.py: ``|kernel - oracle64| <= 16 * E32`` per
float buffer; ``alive``, ``member_steps``, what a dead slot owns and slots
outside the range exact.

Cases: that file's cases that fit 64 wide, and s64_full (every dimension four
tiles, fp32 rows run fewer than four members a block) and two_blocks (six
members at eps 2: a partly filled last block, waves that end at different
steps). In every case the first member enters with all columns dead and the
second with its first column dead.

Measured on MI355X, worst max |err| / E32 (bound 16), bf16 / fp32: e1 1.00 /
1.06, e3 2.14 / 1.93, e16 1.98 / 1.51, odd_binned 1.00 / 1.04, goal 0.89 / 1.28,
mode2 2.06 / 0.92, mode3_noterm 1.52 / 1.43, subrange 1.21 / 1.02, s64_full 1.41
/ 1.51, two_blocks 1.00 / 1.63; noise on: e3 0.92, mode2 1.54.
"""
from unittest import mock

import numpy as np
import pytest

import tests.test_kernel_oracle_loco as L
import tests.test_kernel_oracle_loco_batch as B
import tests.test_kernel_oracle_loco_wave as V
from tests.oracle64 import ERR_FACTOR, STATE_KEYS

CASES = {k: B.CASES[k] for k in ("e1", "e3", "e16", "odd_binned", "goal", "mode2",
                                 "mode3_noterm", "subrange")}
CASES["s64_full"] = B.B(64, [64, 64], 3, adim=8, seed=6)
CASES["two_blocks"] = B.B(11, [24], 2, n_mem=6, seed=33)
ALL = [(n, f32) for f32 in (False, True) for n in CASES]
ids, dev = V.ids, V.dev


def build(name, f32, noise_on=False):
    with mock.patch.object(B, "CASES", CASES):
        return B.build(name, f32, noise_on)


@pytest.mark.parametrize("case", ALL + [c + (True,) for c in B.NOISE_CASES], ids=ids)
def test_loco_wave_batch_cases_meet_their_input_conditions(case):
    case = build(*case)
    y64, _ = B.reference(case)
    if case["name"] == "two_blocks":     # in both blocks waves end at different steps
        m = case["members"]
        ends = (y64["member_steps"][m] - case["state"]["member_steps"][m]).reshape(-1, 2).max(1)
        assert len(ends) == 6 and len(set(ends[:4])) > 1 and len(set(ends[4:])) > 1, ends


class Slots(V.Slots):
    """V.Slots launching the wave batch entry points on the case's member range."""

    def launch(self, n_steps=V.N_STEPS, n_members=None, **kw):
        from es_pytorch_amd import ops
        lib = ops.hip()
        alias = type("Lib", (), dict(es_loco_wave_episode=lib.es_loco_wave_batch_episode,
                                     es_loco_wave_episode_f32=lib.es_loco_wave_batch_episode_f32))
        n = len(self.case["members"]) if n_members is None else n_members
        with mock.patch.object(ops, "hip", lambda: alias):
            return super().launch(n_steps, n_members=n, **kw)


def run(dev, case):
    g = Slots(dev, case)
    assert g.launch() == 0
    return g.read()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL, ids=ids)
def test_loco_wave_batch_matches_oracle(dev, case):
    case = build(*case)
    y64, e32 = B.reference(case)
    L.compare("wave batch " + case["name"], run(dev, case), y64, e32, case["state"],
              case["members"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", B.NOISE_CASES, ids=ids)
def test_loco_wave_batch_noise_on(dev, case):
    """The noisy members match the oracle drawing the same Philox noise and left
    the noise-off oracle; the last member, noiseless, matches that one."""
    noisy = build(*case, noise_on=True)
    E, m = noisy["c"]["eps"], noisy["members"]
    y64, e32 = B.reference(noisy)
    got = run(dev, noisy)
    L.compare("wave batch noise " + noisy["name"], got, y64, e32, noisy["state"], m)
    y_off, e_off = B.reference(build(*case))
    last, rest = m[-E:], m[2 * E:-E]
    for k in STATE_KEYS:
        assert np.abs(got[k][last] - y_off[k][last]).max() <= ERR_FACTOR * e_off[k], k
    assert np.abs(got["rew_total"][rest] - y_off["rew_total"][rest]).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("e3", False), ("subrange", True)], ids=ids)
def test_loco_wave_batch_split_and_repeat_bitwise(dev, case):
    """With noise on, so that the salt matters: 5 + 7 steps (salt_base 0, then
    5) equal one 12-step launch bit for bit, and so does a repeat launch."""
    case = build(*case, noise_on=True)
    one, g = run(dev, case), Slots(dev, case)
    assert V.same_bits(one, run(dev, case))
    assert g.launch(5, salt_base=0) == 0
    mid = g.read()
    assert g.launch(7, salt_base=5) == 0
    assert not np.array_equal(mid["member_steps"], g.read()["member_steps"])
    assert V.same_bits(one, g.read())


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_loco_wave_batch_codes_and_noops(dev, f32):
    """-118 from the launch and es_loco_wave_batch_check alike, -104 and -105 as
    before, nothing written; no steps or no members is a no-op returning 0."""
    from es_pytorch_amd import ops
    case = build("e3", f32)
    g = Slots(dev, case)
    before = g.read()
    unchanged = lambda: V.same_bits(before, g.read())

    def check(dims, eps=3, S=11, stride=1 << 20):
        d = np.array(dims, dtype=np.int32)
        return ops.hip().es_loco_wave_batch_check(d.ctypes.data, len(d), stride, S, 3, 0,
                                                  int(f32), eps)

    assert check(case["dims"], stride=case["stride"]) == 0
    assert g.launch(0) == 0 and g.launch(-2) == 0 and unchanged()
    assert g.launch(n_members=0) == 0 and unchanged()
    for eps in (0, 17):
        with mock.patch.dict(case["c"], eps=eps):
            assert g.launch() == -118 and unchanged(), eps
        assert check(case["dims"], eps) == -118
    assert g.launch(n_members=4) == -118 and unchanged()      # no multiple of eps
    with mock.patch.dict(case["c"], member_base=1):
        assert g.launch(n_members=3) == -118 and unchanged()
    # a 65-wide layer, S 65, a row over the LDS budget
    for dims, S, want in (([11, 65, 3], 11, -118), ([65, 16, 3], 65, -118),
                          ([64] + [64] * 7 + [3], 64, -118), ([11, 16, 3], 12, -104)):
        assert g.launch(dims=dims, S=S, stride=1 << 20) == want and unchanged(), dims
        assert check(dims, S=S) == want, dims
    assert g.launch(dims=[11, 16, 4], stride=1 << 20) == -105 and unchanged()
