"""es_classic_wave_episode / es_classic_wave_episode_f32 (a wavefront per slot,
weights in LDS, nets at most 64 wide) against the float64 oracle, with the
cases, the bound (``|kernel - oracle64| <= 16 * E32`` per float buffer, step
counters and ``alive`` exact, NaN guard rows intact) and the helpers of
tests/test_kernel_oracle_classic.py.

Cases of its own, at the smallest shapes where the lane mapping can go wrong:

  cartpole_w64  [4,64,64,1]  one input partition (P = 1), the full wave owns
                             outputs, the largest covered row (fp32: 2 slots
                             per block)
  cartpole_odd  [4,24,12,1]  output widths that are no power of two (P = 2 and
                             P = 4, lanes without an output), row stride
                             n + 3 so that most rows start off 16 B and take
                             the element-wise copy into LDS
  pendulum_odd  [3,20,1]     the same on Pendulum, 3 inputs

Their seeds meet the condition of the existing CartPole cases on the oracle
alone (no slot within 1e-3 of a decision, float32 plays the same game), which
oracle() asserts.

Measured on MI355X, worst max |err| / E32 per case (bound 16), bf16 / fp32
rows: the four existing cases 1.00 / 1.00, 1.00 / 1.00, 1.03 / 1.00, 1.03 /
1.00 (the block kernel's figures), cartpole_w64 1.00 / 1.00, cartpole_odd
1.00 / 1.00, pendulum_odd 1.80 (th, E32 1.97e-07) / 1.00; noise on 1.00 / 1.00,
Pendulum 1.02.
"""
import numpy as np
import pytest
import torch

from tests.oracle64_classic import CARTPOLE_KEYS
from tests.test_kernel_oracle_classic import (CASES, OB_CLIP, DeviceSlots, build_case,
                                              case_id, case_noise, check, oracle,
                                              state_keys)

pytestmark = pytest.mark.gpu

CASES.update({
    "cartpole_w64": ("cartpole", [4, 64, 64, 1], 5, 6, 1, 0, (1, 1)),
    "cartpole_odd": ("cartpole", [4, 24, 12, 1], 9, 12, 1, 3, (4, 1)),
    "pendulum_odd": ("pendulum", [3, 20, 1], 7, 8, 1, 0, (1, 1)),
})
WAVE_CASES = ["cartpole_base", "cartpole_eps2", "pendulum_base", "pendulum_time_limit",
              "cartpole_w64", "cartpole_odd", "pendulum_odd"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class WaveSlots(DeviceSlots):
    """DeviceSlots whose launch goes to the wave kernel."""

    def launch(self, n_steps, salt_base=0, n_slots=None, env_kind=None, ob_dim=None):
        from es_pytorch_amd import ops
        s = self.state
        ptr = lambda x: x.data_ptr() if x is not None else None
        fn = ops.hip().es_classic_wave_episode_f32 if self.c["f32"] else \
            ops.hip().es_classic_wave_episode
        st, st2 = (s["state"], None) if self.kind == 0 else (s["th"], s["thdot"])
        rc = fn(ptr(st), ptr(st2), ptr(s["env_steps"]), ptr(s["alive"]),
                ptr(s["member_steps"]), ptr(s["rew_total"]), ptr(s["ob_sum"]),
                ptr(s["ob_sumsq"]), ptr(self.w), ptr(self.mean), ptr(self.std),
                self.dims.ctypes.data, len(self.dims), self.stride, OB_CLIP,
                ptr(self.acstd), ptr(self.seed), salt_base,
                self.kind if env_kind is None else env_kind,
                self.ob_dim if ob_dim is None else ob_dim, self.max_env,
                self.B if n_slots is None else n_slots, n_steps, self.c["eps"], 1,
                self.noiseless_from, torch.cuda.current_stream(self.dev).cuda_stream)
        torch.cuda.synchronize(self.dev)
        return rc


def run_wave(dev, name, f32=False, noise_on=False):
    c = build_case(name, f32)
    g = WaveSlots(dev, c, case_noise(c) if noise_on else None)
    assert g.launch(c["n_steps"]) == 0
    return g.read()


@pytest.mark.parametrize("case", [(n, f32) for f32 in (False, True) for n in WAVE_CASES],
                         ids=case_id)
def test_classic_wave_matches_oracle(dev, case):
    name, f32 = case
    y64, e32, info = oracle(name, f32)
    check("wave " + case_id(case), CASES[name][0], run_wave(dev, name, f32), y64, e32)


@pytest.mark.parametrize("case", [("cartpole_base", False), ("cartpole_base", True),
                                  ("pendulum_base", False)], ids=case_id)
def test_classic_wave_noise_on(dev, case):
    """ac_std 0.3, every slot but the last noisy: the rollout matches the
    oracle drawing the same Philox noise, the last slot the noise-off oracle,
    and the noisy slots measurably left it."""
    name, f32 = case
    kind = CASES[name][0]
    y64, e32, info = oracle(name, f32, noise_on=True)
    got = run_wave(dev, name, f32, noise_on=True)
    check("wave " + case_id(case) + "_noise_on", kind, got, y64, e32)
    y_off, e_off, _ = oracle(name, f32)
    check("wave " + case_id(case) + "_last_slot_vs_noise_off", kind, got, y_off, e_off,
          slots=slice(CASES[name][2] - 1, None))
    key = "state" if kind == "cartpole" else "th"
    assert np.abs(got[key][:-1] - y_off[key][:-1]).max() > 1e-3


@pytest.mark.parametrize("case", [("cartpole_odd", False), ("pendulum_time_limit", False),
                                  ("cartpole_eps2", True)], ids=case_id)
def test_classic_wave_split_and_repeat_bitwise(dev, case):
    """With noise on, so that the salt matters: 5 + 7 steps (salt_base 0, then
    5) equal one 12-step launch bit for bit, and so does a repeat launch."""
    name, f32 = case
    c = build_case(name, f32)
    one = run_wave(dev, name, f32, noise_on=True)
    again = run_wave(dev, name, f32, noise_on=True)
    g = WaveSlots(dev, c, case_noise(c))
    assert g.launch(5, salt_base=0) == 0
    mid = g.read()
    assert g.launch(7, salt_base=5) == 0
    two = g.read()
    assert not np.array_equal(mid["member_steps"], two["member_steps"])
    for k in state_keys(c["kind"]):
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), k
        assert np.array_equal(one[k].view(np.uint8), again[k].view(np.uint8)), k


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_classic_wave_codes_and_noops(dev, f32):
    """A net the kernel does not cover is -116 from the launch and from
    es_classic_wave_check alike; the existing codes keep their meaning; nothing
    is written in either case; no steps or no slots is a no-op returning 0."""
    from es_pytorch_amd import ops
    g = WaveSlots(dev, build_case("cartpole_base", f32))
    before = g.read()

    def unchanged():
        now = g.read()
        return all(np.array_equal(before[k].view(np.uint8), now[k].view(np.uint8))
                   for k in CARTPOLE_KEYS)

    def shape_check(dims, stride=1 << 20):
        d = np.array(dims, dtype=np.int32)
        return ops.hip().es_classic_wave_check(d.ctypes.data, len(d), stride, int(f32))

    assert g.launch(0) == 0 and unchanged()
    assert g.launch(-3) == 0 and unchanged()
    assert g.launch(4, n_slots=0) == 0 and unchanged()
    assert g.launch(4, env_kind=2) == -113 and unchanged()
    assert g.launch(4, ob_dim=5) == -114 and unchanged()
    good, stride = g.dims, g.stride
    assert shape_check(good, stride) == 0
    g.stride = 1 << 20      # wide enough for every net below: -102 is not the answer
    for dims, want in (([4, 256, 256, 1], -116), ([4, 65, 1], -116), ([4, 16, 0], -115)):
        g.dims = np.array(dims, dtype=np.int32)
        assert g.launch(4) == want and unchanged(), dims
        assert shape_check(dims) == want, dims
    g.dims, g.stride = good, 8                      # row_stride < n
    assert g.launch(4) == -102 and unchanged()
    assert shape_check(good, 8) == -102
