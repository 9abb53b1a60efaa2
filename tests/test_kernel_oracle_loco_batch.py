"""es_loco_batch_episode / _f32 (a block per member, its E = eps episodes as the
columns of fp32 MFMA products) against the float64 oracle, with the builder,
``expected`` and the launcher of tests/test_kernel_oracle_loco_wave.py and the
comparison and bound of tests/test_kernel_oracle_loco.py:
``|kernel - oracle64| <= 16 * E32`` per float buffer; ``alive``,
``member_steps``, what a dead slot owns and slots outside the range exact. The
kernel keeps the wave kernel's semantic for a slot that died.

Cases (3-4 members of E slots, 12 steps, bf16 and fp32 rows): e1 / e3 / e16 the
column padding at both ends on [11, 24, 3] (K tail I % 4, output tile tail
O < 16, four K slices); h96_256 two 64-output groups (two K slices each) and
four (the output split); odd_binned row stride n + 3 behind an odd O (element loads) with bins 5;
goal S 27, D 29, adim 8; mode2; mode3_noterm; subrange member_base / wrow0 with
guard slots on both sides; wide264 a K slice of more than one load fragment;
humanoid_e16 HumanoidFlagrun's env at E 16, 119 KB of LDS (the raised limit).
In every case the first member enters with all columns dead and the second with
its first column dead.

Measured on MI355X, worst max |err| / E32 (bound 16), bf16 / fp32: e1 1.00 /
1.00, e3 3.05 / 1.93, e16 1.41 / 1.15, h96_256 2.59 / 1.00, odd_binned 1.17 /
1.05, goal 1.09 / 1.29, mode2 2.06 / 1.64, mode3_noterm 1.41 / 1.44, subrange
1.75 / 1.00, wide264 1.23 / 2.20, humanoid_e16 1.00 / 0.91; noise on: e3 1.00,
mode2 1.23.
"""
from unittest import mock

import numpy as np
import pytest

import tests.test_kernel_oracle_loco as L
import tests.test_kernel_oracle_loco_wave as V
from tests.oracle64 import ERR_FACTOR, STATE_KEYS, err_scale, top2_logit_gap

N_STEPS, FALL_THR = V.N_STEPS, V.FALL_THR


def B(S, hidden, eps, n_mem=4, **kw):
    mb = kw.pop("member_base", 0)
    return dict(V.E(S, hidden, eps=eps, member_base=mb, **kw), members=mb + (n_mem + 1) * eps,
                n_mem=n_mem)


CASES = {
    "e1": B(11, [24], 1, seed=6),
    "e3": B(11, [24], 3, seed=16),
    "e16": B(11, [24], 16, n_mem=3, seed=3),
    "h96_256": B(16, [96, 256], 3, seed=0),
    "odd_binned": B(17, [24, 13], 3, bins=5, seed=0),
    "goal": B(27, [64], 3, adim=8, goal=1, seed=49),
    "mode2": B(11, [16], 3, act_mode=2, seed=5),
    "mode3_noterm": B(8, [16], 3, adim=2, act_mode=3, terminate=0, seed=0),
    "subrange": B(11, [16], 3, member_base=3, wrow0=1, seed=49),
    "wide264": B(64, [264], 3, n_mem=3, adim=17, seed=19),
    "humanoid_e16": B(376, [256], 16, n_mem=3, adim=17, goal=1, seed=2),
}
STRIDE_PAD = {"odd_binned": 3}
# cases in which a member's columns die at different steps beside a survivor;
# the others have a survivor and a slot that dies inside
STAGGERED = ("e3", "e16", "goal", "mode2", "subrange", "wide264")
NOISE_CASES = [("e3", False), ("mode2", True)]
ALL = [(n, f32) for f32 in (False, True) for n in CASES]
ids = V.ids


def build(name, f32, noise_on=False):
    """V.build's case on this file's CASES; the launch covers n_mem members from
    member_base (the eps slots behind them are guards), the first of which
    enters dead and the second with its first column dead."""
    with mock.patch.multiple(V, CASES=CASES, STRIDE_PAD=STRIDE_PAD):
        case = V.build(name, f32, noise_on)
    c = case["c"]
    E, mb, n = c["eps"], c["member_base"], CASES[name]["n_mem"] * c["eps"]
    case["members"] = np.arange(mb, mb + n)
    if noise_on:                      # the last launched member is the noiseless one
        c["noiseless_from"] = mb + n - E
    alive = np.ones_like(case["state"]["alive"])
    alive[mb:mb + E + 1] = 0.0
    case["state"]["alive"] = alive
    return case


def reference(case):
    """(y64, E32 per buffer); asserts the case's input conditions."""
    c, m = case["c"], case["members"]
    (y64, i64), (y32, i32) = V.expected(case, np.float64), V.expected(case, np.float32)
    for a, b in zip(i64, i32):
        assert (np.abs(a["h"] - FALL_THR) > 1e-3).all(), "h on thr"
        assert np.array_equal(a["done"], b["done"]), "float32 plays another game"
        live = a["alive_before"]
        if c["bins"] > 1 and live.any():
            assert top2_logit_gap(a["net_out"][live], c["bins"]) > 1e-3, "logit tie"
            assert np.array_equal(a["actions"][live], b["actions"][live]), "another bin"
    assert np.array_equal(y64["member_steps"], y32["member_steps"])
    if c["terminate"]:
        took = y64["member_steps"][m] - case["state"]["member_steps"][m]
        stag = case["name"] in STAGGERED
        took = took.reshape(-1, c["eps"]) if stag else took.reshape(1, -1)
        assert any((t == N_STEPS).any() and
                   len(set(t[(t > 0) & (t < N_STEPS)])) >= 1 + stag
                   for t in took), "no member whose columns die at different steps"
    return y64, {k: err_scale(y32[k][m], y64[k][m]) for k in STATE_KEYS}


@pytest.mark.parametrize("case", ALL + [c + (True,) for c in NOISE_CASES], ids=ids)
def test_loco_batch_cases_meet_their_input_conditions(case):
    reference(build(*case))


# -------------------------------------------------------------------- GPU side
dev = V.dev


class Slots(V.Slots):
    """V.Slots launching the batch entry points on the case's member range."""

    def launch(self, n_steps=N_STEPS, n_members=None, **kw):
        from es_pytorch_amd import ops
        lib = ops.hip()
        alias = type("Lib", (), dict(es_loco_wave_episode=lib.es_loco_batch_episode,
                                     es_loco_wave_episode_f32=lib.es_loco_batch_episode_f32))
        n = len(self.case["members"]) if n_members is None else n_members
        with mock.patch.object(ops, "hip", lambda: alias):
            return super().launch(n_steps, n_members=n, **kw)


def run(dev, case):
    g = Slots(dev, case)
    assert g.launch() == 0
    return g.read()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL, ids=ids)
def test_loco_batch_matches_oracle(dev, case):
    case = build(*case)
    y64, e32 = reference(case)
    L.compare("batch " + case["name"], run(dev, case), y64, e32, case["state"],
              case["members"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", NOISE_CASES, ids=ids)
def test_loco_batch_noise_on(dev, case):
    """The noisy members match the oracle drawing the same Philox noise and left
    the noise-off oracle; the last member, noiseless, matches that one."""
    noisy = build(*case, noise_on=True)
    E, m = noisy["c"]["eps"], noisy["members"]
    y64, e32 = reference(noisy)
    got = run(dev, noisy)
    L.compare("batch noise " + noisy["name"], got, y64, e32, noisy["state"], m)
    y_off, e_off = reference(build(*case))
    last, rest = m[-E:], m[2 * E:-E]
    for k in STATE_KEYS:
        assert np.abs(got[k][last] - y_off[k][last]).max() <= ERR_FACTOR * e_off[k], k
    assert np.abs(got["rew_total"][rest] - y_off["rew_total"][rest]).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("e3", False), ("subrange", True)], ids=ids)
def test_loco_batch_split_and_repeat_bitwise(dev, case):
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
def test_loco_batch_codes_and_noops(dev, f32):
    """-117 from the launch and es_loco_batch_check alike, -104 and -105 as
    before, nothing written; no steps or no members is a no-op returning 0."""
    from es_pytorch_amd import ops
    case = build("e3", f32)
    g = Slots(dev, case)
    before = g.read()
    unchanged = lambda: V.same_bits(before, g.read())

    def check(dims, eps, S=11, stride=1 << 20):
        d = np.array(dims, dtype=np.int32)
        return ops.hip().es_loco_batch_check(d.ctypes.data, len(d), stride, S, 3, 0,
                                             int(f32), eps)

    assert check(case["dims"], 3, stride=case["stride"]) == 0
    assert g.launch(0) == 0 and g.launch(-2) == 0 and unchanged()
    assert g.launch(n_members=0) == 0 and unchanged()
    for eps in (0, 17):
        with mock.patch.dict(case["c"], eps=eps):
            assert g.launch() == -117 and unchanged(), eps
        assert check(case["dims"], eps) == -117
    assert g.launch(n_members=4) == -117 and unchanged()
    assert check([2048, 2048, 3], 16, S=2048, stride=1 << 24) == -117   # beyond any LDS
    assert g.launch(dims=[11, 16, 3], S=12, stride=1 << 20) == -104 and unchanged()
    assert check([11, 16, 3], 3, S=12) == -104
    assert g.launch(dims=[11, 16, 4], stride=1 << 20) == -105 and unchanged()
