"""es_loco_wave_episode / _f32 (a wavefront per slot, state and nets at most 64
wide) against the float64 oracle, with the builder, the comparison and the
bound of tests/test_kernel_oracle_loco.py: ``|kernel - oracle64| <= 16 * E32``
per float buffer; ``alive``, ``member_steps``, what a dead slot owns and slots
outside the range exact. The kernel stops stepping a slot that died, so
expected() keeps ``s`` and ``pos`` from the last step a slot entered alive.

Cases (CASES; about 9 slots, 12 steps, bf16 and fp32 rows): hopper has OP 16,
P 4 in the dynamics; ant_goal P 1 and the goal dims in lanes 27, 28; s64_full
the full wave and the largest env block (bf16 rows run 4 slots a block, fp32
rows 2); odd_binned widths that are no power of two and row stride n + 3, so
rows take the element-wise copy into LDS.

Measured on MI355X, worst max |err| / E32 (bound 16), bf16 / fp32: hopper 1.61
/ 1.76, ant_goal 1.90 / 0.97, s64_full 1.04 / 1.73, odd_binned 1.10 / 1.00,
mode2 0.97 / 1.58, mode3_noterm 1.75 / 1.24, eps2_subrange 1.18 / 1.60; noise
on: hopper 1.18 / 1.77, mode2 1.43 / 1.00.
"""
from unittest import mock

import numpy as np
import pytest
import torch

import tests.test_kernel_oracle_loco as L
from tests.oracle64 import (ERR_FACTOR, STATE_KEYS, err_scale, loco_step, n_params,
                            top2_logit_gap)
from tests.test_kernel_oracle_f32 import make_net_f32

N_STEPS = 12
E = lambda S, hidden, **kw: L.C("episode", S, hidden, n_steps=N_STEPS, members=9, **kw)
CASES = {
    "hopper": E(11, [32, 32], seed=0),
    "ant_goal": E(27, [64, 64], adim=8, goal=1, seed=2),
    "s64_full": E(64, [64], adim=8, seed=0),
    "odd_binned": E(17, [24, 12], adim=6, bins=5, seed=44),
    "mode2": E(11, [16], act_mode=2, seed=1),
    "mode3_noterm": E(8, [16], adim=2, act_mode=3, terminate=0, seed=0),
    "eps2_subrange": dict(E(11, [16], eps=2, member_base=3, wrow0=1, seed=3), members=12),
}
FALL_THR = -0.5                         # 0.0 kills most slots within 12 steps
STRIDE_PAD = {"odd_binned": 3}          # row stride n + 3
NOISE = dict(ac_std=0.3, seed_dev=0x5EED1234ABCD)
NOISE_CASES = [(n, f32) for n in ("hopper", "mode2") for f32 in (False, True)]
ALL = [(n, f32) for f32 in (False, True) for n in CASES]
ids = lambda v: f"{v[0]}-{'f32' if v[1] else 'bf16'}" + ("-noise" if len(v) > 2 else "")
_case_dims = L.case_dims
wave_dims = lambda c: [c["S"] + 2 * c["goal"], *c["hidden"], _case_dims(c)[-1]]


def build(name, f32, noise_on=False):
    """L.build's case with several hidden layers, this file's fall threshold
    and row stride, and float32 rows where asked for."""
    c = dict(CASES[name])
    if noise_on:
        c.update(NOISE, noiseless_from=c["members"] - 1)
    # L.build reads its widths through the module global L.case_dims (one
    # hidden layer), replaced for the call; the assert fails should that change
    with mock.patch.object(L, "case_dims", wave_dims):
        case = L.build(name, {name: c})
    assert case["dims"] == wave_dims(c)
    case["env"]["fall_thr"] = FALL_THR
    n, pad = n_params(case["dims"]), STRIDE_PAD.get(name)
    rows = case["blobs"]["weights"].shape[0] - 1
    if f32:
        fpad = 0 if pad is None else n + pad - (n + 3) // 4 * 4
        case["w"], case["stride"] = make_net_f32(np.random.RandomState(77 + c["seed"]),
                                                 case["dims"], rows, fpad)
        case["policy"]["weight_rows"] = case["w"][:, :n].astype(np.float64)
    else:
        case["w"] = case["blobs"]["weights"]
        if pad is not None:
            case["stride"] = n + pad
            case["w"] = np.zeros((rows + 1, n + pad), dtype=np.uint16)
            case["w"][:, :n] = case["blobs"]["weights"][:, :n]
    case["f32"] = f32
    return case


def expected(case, dtype):
    """(state, infos): loco_step N_STEPS times; s and pos from the last step a
    slot entered alive."""
    c, m = case["c"], case["members"]
    env = {k: v for k, v in case["env"].items() if k != "A_bits"}
    noise = L.case_noise(c)[0] if c["ac_std"] else None
    state = case["state"]
    kept = {k: state[k].astype(dtype) for k in ("s", "pos")}
    infos = []
    for t in range(N_STEPS):
        live = m[state["alive"][m] > 0]
        state, info = loco_step(state, env, case["policy"], m, dtype, noise, t)
        for k in kept:
            kept[k][live] = state[k][live]
        infos.append(info)
    return dict(state, **kept), infos


def reference(case):
    """(y64, E32 per buffer); asserts the case's input conditions: no h within
    1e-3 of the threshold, no logit tie, float32 plays the same discrete game,
    and a slot dead on entry, one that dies inside and one that survives."""
    c, m = case["c"], case["members"]
    (y64, i64), (y32, i32) = expected(case, np.float64), expected(case, np.float32)
    for a, b in zip(i64, i32):
        assert (np.abs(a["h"] - FALL_THR) > 1e-3).all(), "h on thr"
        assert np.array_equal(a["done"], b["done"]), "float32 plays another game"
        live = a["alive_before"]     # a dead slot's logits decide nothing
        if c["bins"] > 1 and live.any():
            assert top2_logit_gap(a["net_out"][live], c["bins"]) > 1e-3, "logit tie"
            assert np.array_equal(a["actions"][live], b["actions"][live]), "another bin"
    assert np.array_equal(y64["member_steps"], y32["member_steps"])
    if c["terminate"]:
        took = y64["member_steps"][m] - case["state"]["member_steps"][m]
        was = case["state"]["alive"][m] > 0
        assert (~was).any() and (took == N_STEPS).any()
        assert (was & (took < N_STEPS) & (y64["alive"][m] == 0)).any(), "nobody dies inside"
    return y64, {k: err_scale(y32[k][m], y64[k][m]) for k in STATE_KEYS}


@pytest.mark.parametrize("case", ALL + [c + (True,) for c in NOISE_CASES], ids=ids)
def test_loco_wave_cases_meet_their_input_conditions(case):
    reference(build(*case))


# -------------------------------------------------------------------- GPU side
@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class Slots:
    """A case's buffers on the device and launches on them."""

    def __init__(self, dev, case):
        self.dev, self.case, c, env = dev, case, case["c"], case["env"]
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.st = {k: t(v) for k, v in case["state"].items()}
        self.w = t(case["w"]) if case["f32"] else L.bf16_tensor(case["w"], dev)
        seed = None if c["seed_dev"] is None else np.array([c["seed_dev"]], np.int64)
        self.keep = [t(case["obmean"]), t(case["obstd"]), t(seed),
                     torch.full((1,), c["ac_std"], dtype=torch.float32, device=dev),
                     L.bf16_tensor(env["A_bits"], dev)] + \
            [t(env[k]) for k in ("B", "b0", "wv", "wa", "wy", "wh")]

    def launch(self, n_steps=N_STEPS, salt_base=0, dims=None, stride=None, S=None,
               n_members=None):
        from es_pytorch_amd import ops
        c, env, st = self.case["c"], self.case["env"], self.st
        ptr = lambda x: None if x is None else x.data_ptr()
        mean, std, seed, acstd, *mats = map(ptr, self.keep)
        dims = np.array(self.case["dims"] if dims is None else dims, dtype=np.int32)
        fn = ops.hip().es_loco_wave_episode_f32 if self.case["f32"] else \
            ops.hip().es_loco_wave_episode
        mb = c["member_base"]
        rc = fn(ptr(self.w), mean, std, dims.ctypes.data, len(dims), seed, n_steps, L.OB_CLIP,
                acstd, self.case["stride"] if stride is None else stride,
                ptr(st["s"]), ptr(st["pos"]), ptr(st["goal"]), *mats,
                *(ptr(st[k]) for k in ("alive", "rew_total", "member_steps", "behv",
                                       "mo_sum", "mo_sumsq")),
                mb, self.case["nslots"] - mb if n_members is None else n_members, salt_base,
                c["wrow0"], c["S"] if S is None else S, c["adim"], c["goal"], c["terminate"],
                c["noiseless_from"], c["bins"], c["eps"], c["act_mode"],
                *(float(env[k]) for k in ("leak", "ctrl", "alive_bonus", "fall_thr", "dt")),
                torch.cuda.current_stream(self.dev).cuda_stream)
        torch.cuda.synchronize(self.dev)
        return rc

    def read(self):
        return {k: self.st[k].cpu().numpy() for k in STATE_KEYS}


def run(dev, case):
    g = Slots(dev, case)
    assert g.launch() == 0
    return g.read()


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in STATE_KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL, ids=ids)
def test_loco_wave_matches_oracle(dev, case):
    case = build(*case)
    y64, e32 = reference(case)
    L.compare("wave " + case["name"], run(dev, case), y64, e32, case["state"],
              case["members"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", NOISE_CASES, ids=ids)
def test_loco_wave_noise_on(dev, case):
    """The noisy slots match the oracle drawing the same Philox noise and left
    the noise-off oracle; the last slot, noiseless, matches that one."""
    noisy = build(*case, noise_on=True)
    y64, e32 = reference(noisy)
    got = run(dev, noisy)
    L.compare("wave noise " + noisy["name"], got, y64, e32, noisy["state"], noisy["members"])
    y_off, e_off = reference(build(*case))
    for k in STATE_KEYS:
        assert np.abs(got[k][-1] - y_off[k][-1]).max() <= ERR_FACTOR * e_off[k], k
    assert np.abs(got["rew_total"][:-1] - y_off["rew_total"][:-1]).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("hopper", False), ("eps2_subrange", True)], ids=ids)
def test_loco_wave_split_and_repeat_bitwise(dev, case):
    """With noise on, so that the salt matters: 5 + 7 steps (salt_base 0, then
    5) equal one 12-step launch bit for bit, and so does a repeat launch."""
    case = build(*case, noise_on=True)
    one, g = run(dev, case), Slots(dev, case)
    assert same_bits(one, run(dev, case))
    assert g.launch(5, salt_base=0) == 0
    mid = g.read()
    assert g.launch(7, salt_base=5) == 0
    assert not np.array_equal(mid["member_steps"], g.read()["member_steps"])
    assert same_bits(one, g.read())


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_loco_wave_codes_and_noops(dev, f32):
    """-116 from the launch and es_loco_wave_check alike, -104 and -105 as
    before, nothing written; no steps or no members is a no-op returning 0."""
    from es_pytorch_amd import ops
    case = build("hopper", f32)
    g = Slots(dev, case)
    before = g.read()
    unchanged = lambda: same_bits(before, g.read())

    def check(dims, S=11, stride=1 << 20):
        d = np.array(dims, dtype=np.int32)
        return ops.hip().es_loco_wave_check(d.ctypes.data, len(d), stride, S, 3, 0, int(f32))

    assert check(case["dims"], stride=case["stride"]) == 0
    assert g.launch(0) == 0 and g.launch(-2) == 0 and unchanged()
    assert g.launch(n_members=0) == 0 and unchanged()
    for dims, S, want in (([11, 65, 3], 11, -116), ([11, 256, 256, 3], 11, -116),
                          ([72, 16, 3], 72, -116), ([11, 16, 3], 12, -104)):
        assert g.launch(dims=dims, S=S, stride=1 << 20) == want and unchanged(), dims
        assert check(dims, S) == want, dims
    assert g.launch(dims=[11, 16, 4], stride=1 << 20) == -105 and unchanged()
