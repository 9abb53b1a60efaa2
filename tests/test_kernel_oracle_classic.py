"""es_classic_episode / es_classic_episode_f32 against the float64 oracle
(tests/oracle64_classic.py).

Every case calls the kernel directly on test-owned buffers and asserts
``|kernel - oracle64| <= 16 * E32`` per float buffer, E32 being the error of
the same rollout evaluated in numpy float32; ``member_steps``, ``env_steps``
and ``alive`` must match exactly. The state buffers are read at launch and
written back, so they cannot start as NaN; instead every buffer carries one
more slot row than the launch covers, filled with NaN, which must still be NaN
afterwards.

CartPole has three discrete decisions per step: the force is the SIGN of the
action, and the episode ends when |x| passes 2.4 or |theta| passes 12 degrees.
A slot whose float64 value comes within 1e-3 of one of them could legitimately
take the other branch in fp32. The seeds and the hand-placed starts below were
chosen so that NO slot does (asserted on the oracle alone, cap zero, also
without a GPU in tests/test_oracle64_classic_cpu.py), and so that the float32
oracle plays the same game as the float64 one: same force signs at every live
step, same end steps. The forwards run on identical weight values, so the
action error is of order 1e-6 and 1e-3 is ample. Pendulum has no threshold on
a float.

CartPole starts (make_cartpole): slot 0 sits 5 mm inside the x threshold
moving out (ends at step 1), slot 1 runs at it (ends by x mid-rollout), slot 2
leans at 0.15 rad and falling (ends by theta mid-rollout), slot 3 has its env
step counter 3 below MAX_STEPS (the time limit ends it at step 3); the rest
start within +-0.05 and never end. Pendulum time limit: slot 2 starts 3 steps
from its limit.

Measured on MI355X, max |err| / E32 over the float buffers of each case
(bound: 16), on bf16 rows and on fp32 rows:

  case                                    bf16  worst buffer  its E32    fp32  worst buffer  its E32
  cartpole_base                           1.00  state         2.02e-07   1.00  state         1.92e-07
  cartpole_wide                           1.00  state         1.92e-07   1.00  state         1.92e-07
  cartpole_eps2                           1.00  state         2.52e-07   1.00  state         2.96e-07
  pendulum_base                           1.03  rew_total     1.13e-05   1.00  thdot         9.41e-07
  pendulum_time_limit                     1.03  rew_total     1.13e-05   1.00  thdot         9.41e-07
  cartpole_base noise_on                  1.00  ob_sumsq      1.15e-06   1.00  state         1.50e-07
  cartpole_base last slot vs noise off    0.62  ob_sum        7.17e-07   0.20  ob_sum        9.99e-07
  pendulum_base noise_on                  1.00  th            3.43e-07
  pendulum_base last slot vs noise off    0.45  rew_total     1.13e-05

A ratio of 1.00 is the kernel landing on the float32 oracle's own value at the
worst element: both evaluate the same operations in the same order.
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import ERR_FACTOR, fp32_error_scale, max_ratio, n_params
from tests.oracle64_classic import (CARTPOLE_KEYS, CP_MAX_STEPS, PD_MAX_STEPS,
                                    PENDULUM_KEYS, cartpole_rollout, cartpole_state,
                                    pendulum_rollout, pendulum_state)
from tests.test_kernel_oracle_f32 import make_net_f32
from tests.test_kernel_oracle_mlp import bf16_tensor, make_net

pytestmark = pytest.mark.gpu

MARGIN_MIN = 1e-3
OB_CLIP = 5.0
EXACT_KEYS = ("member_steps", "env_steps", "alive")

# name -> (kind, dims, slots, steps, eps, stride_pad,
#          rng seeds (bf16 rows, fp32 rows))
CASES = {
    "cartpole_base": ("cartpole", [4, 16, 1], 9, 12, 1, 0, (218, 1014)),
    "cartpole_wide": ("cartpole", [4, 256, 256, 1], 5, 6, 1, 0, (2, 2)),
    "cartpole_eps2": ("cartpole", [4, 16, 1], 8, 12, 2, 8, (4, 4)),
    "pendulum_base": ("pendulum", [3, 16, 1], 9, 12, 1, 0, (1, 1)),
    "pendulum_time_limit": ("pendulum", [3, 16, 1], 9, 12, 1, 0, (1, 1)),
}
ALL_CASES = [(n, f32) for f32 in (False, True) for n in CASES]
# ac_std is large next to the tag test's 0.05: CartPole only feels the noise
# through the sign of the action
NOISE = dict(seed=20250311, ac_std=0.3)


def case_id(p):
    return p[0] + ("_f32" if p[1] else "")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def float_keys(kind):
    return (("state",) if kind == "cartpole" else ("th", "thdot")) + \
        ("rew_total", "ob_sum", "ob_sumsq")


def state_keys(kind):
    return CARTPOLE_KEYS if kind == "cartpole" else PENDULUM_KEYS


def rollout_fn(kind):
    return cartpole_rollout if kind == "cartpole" else pendulum_rollout


def make_cartpole(rng, B):
    s = rng.uniform(-0.05, 0.05, size=(B, 4)).astype(np.float32)
    s[0] = [2.395, 1.0, 0.01, 0.0]       # out by x at step 1
    s[1] = [2.30, 2.0, -0.01, 0.0]       # out by x mid-rollout
    s[2] = [0.0, 0.0, 0.15, 0.6]         # out by theta mid-rollout
    steps = np.zeros(B, np.float32)
    steps[3] = CP_MAX_STEPS - 3          # the time limit ends it at step 3
    return cartpole_state(s, steps)


def make_pendulum(rng, B, time_limit):
    th = rng.uniform(-np.pi, np.pi, size=B).astype(np.float32)
    thdot = rng.uniform(-1.0, 1.0, size=B).astype(np.float32)
    steps = np.zeros(B, np.float32)
    if time_limit:
        steps[2] = PD_MAX_STEPS - 3
    return pendulum_state(th, thdot, steps)


def build_case(name, f32=False):
    kind, dims, B, n_steps, eps, pad, seeds = CASES[name]
    rng = np.random.RandomState(seeds[int(f32)])
    rows = (B + eps - 1) // eps
    n = n_params(dims)
    if f32:
        w, stride = make_net_f32(rng, dims, rows, pad)
        wvals = w[:, :n].astype(np.float64)
    else:
        w, wvals, stride = make_net(rng, dims, rows, pad)
    D = dims[0]
    obmean = (rng.randn(D) * 0.1).astype(np.float32)
    obstd = (rng.rand(D) + 0.5).astype(np.float32)
    net = dict(dims=dims, weight_rows=wvals, obmean=obmean, obstd=obstd, ob_clip=OB_CLIP,
               eps=eps, act_final=1)
    state = make_cartpole(rng, B) if kind == "cartpole" else \
        make_pendulum(rng, B, name == "pendulum_time_limit")
    return dict(name=name, kind=kind, f32=f32, B=B, n_steps=n_steps, eps=eps, dims=dims,
                net=net, w=w, stride=stride, obmean=obmean, obstd=obstd, state=state)


def case_noise(c):
    return dict(NOISE, noiseless_from=c["B"] - 1)


_ORACLE = {}


def oracle(name, f32=False, noise_on=False):
    """(y64, E32, info64) of the case's whole rollout; computed once. Asserts
    what the oracle alone must meet: no slot on a decision's rounding edge,
    and single precision plays the same game."""
    key = (name, f32, noise_on)
    if key not in _ORACLE:
        c = build_case(name, f32)
        fn = rollout_fn(c["kind"])
        noise = case_noise(c) if noise_on else None
        y64, e32 = fp32_error_scale(fn, c["state"], c["net"], c["n_steps"], noise=noise)
        _, info = fn(c["state"], c["net"], c["n_steps"], noise=noise)
        _, info32 = fn(c["state"], c["net"], c["n_steps"], dtype=np.float32, noise=noise)
        for k, m in info["margins"].items():
            assert int((m < MARGIN_MIN).sum()) == 0, (key, k, m)
        assert np.array_equal(info["end_step"], info32["end_step"]), key
        if c["kind"] == "cartpole":     # the force is the action's sign
            assert np.array_equal(info["actions"] > 0, info32["actions"] > 0), key
        _ORACLE[key] = (y64, e32, info)
    return _ORACLE[key]


class DeviceSlots:
    """Device copies of a case: state with one NaN guard row, the net."""

    def __init__(self, dev, c, noise=None):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.dev, self.B, self.c = dev, c["B"], c
        self.keys = state_keys(c["kind"])
        self.state = {}
        for k in self.keys:
            a = np.asarray(c["state"][k])
            g = np.full((1,) + a.shape[1:], np.nan, dtype=a.dtype)
            self.state[k] = t(np.concatenate([a, g], axis=0))
        self.w = t(c["w"]) if c["f32"] else bf16_tensor(c["w"], dev)
        self.mean, self.std = t(c["obmean"]), t(c["obstd"])
        self.dims = np.array(c["dims"], dtype=np.int32)
        self.stride = c["stride"]
        self.kind = 0 if c["kind"] == "cartpole" else 1
        self.ob_dim = 4 if c["kind"] == "cartpole" else 3
        self.max_env = CP_MAX_STEPS if c["kind"] == "cartpole" else PD_MAX_STEPS
        self.seed = self.acstd = None
        self.noiseless_from = 0
        if noise is not None:
            self.seed = t(np.array([noise["seed"]], np.int64))
            self.acstd = t(np.array([noise["ac_std"]], np.float32))
            self.noiseless_from = noise["noiseless_from"]

    def launch(self, n_steps, salt_base=0, n_slots=None, env_kind=None, ob_dim=None):
        from es_pytorch_amd import ops
        s = self.state
        ptr = lambda x: x.data_ptr() if x is not None else None
        fn = ops.hip().es_classic_episode_f32 if self.c["f32"] else \
            ops.hip().es_classic_episode
        if self.kind == 0:
            st, st2 = s["state"].data_ptr(), None
        else:
            st, st2 = s["th"].data_ptr(), s["thdot"].data_ptr()
        rc = fn(st, st2, s["env_steps"].data_ptr(), s["alive"].data_ptr(),
                s["member_steps"].data_ptr(), s["rew_total"].data_ptr(),
                s["ob_sum"].data_ptr(), s["ob_sumsq"].data_ptr(), self.w.data_ptr(),
                self.mean.data_ptr(), self.std.data_ptr(), self.dims.ctypes.data,
                len(self.dims), self.stride, OB_CLIP, ptr(self.acstd), ptr(self.seed),
                salt_base, self.kind if env_kind is None else env_kind,
                self.ob_dim if ob_dim is None else ob_dim, self.max_env,
                self.B if n_slots is None else n_slots, n_steps, self.c["eps"], 1,
                self.noiseless_from, torch.cuda.current_stream(self.dev).cuda_stream)
        torch.cuda.synchronize(self.dev)
        return rc

    def read(self):
        """Host copy of the B slots; the guard row must still be NaN."""
        out = {}
        for k, v in self.state.items():
            a = v.cpu().numpy()
            assert np.isnan(a[self.B:]).all(), f"{k}: guard row written"
            out[k] = a[:self.B]
        return out


def run_case(dev, name, f32=False, noise_on=False):
    c = build_case(name, f32)
    g = DeviceSlots(dev, c, case_noise(c) if noise_on else None)
    assert g.launch(c["n_steps"]) == 0
    return g.read()


def check(label, kind, got, y64, e32, slots=slice(None)):
    for k in EXACT_KEYS:
        assert np.array_equal(got[k][slots], y64[k][slots]), (label, k)
    worst = (0.0, "")
    ratios = {}
    for k in float_keys(kind):
        assert np.isfinite(got[k]).all(), (label, k)
        ratios[k] = max_ratio(got[k][slots], y64[k][slots], e32[k])
        print(f"ORACLE-RATIO classic {label} {k} ratio={ratios[k]:.2f} E32={e32[k]:.3g}")
        worst = max(worst, (ratios[k], k))
    print(f"ORACLE-RATIO classic {label} worst ratio={worst[0]:.2f} ({worst[1]}) "
          f"E32={e32[worst[1]]:.3g}")
    for k, r in ratios.items():
        assert r <= ERR_FACTOR, (label, k, r, e32[k])


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_classic_episode_matches_oracle(dev, case):
    name, f32 = case
    y64, e32, info = oracle(name, f32)
    got = run_case(dev, name, f32)
    check(case_id(case), CASES[name][0], got, y64, e32)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_classic_episode_cartpole_endings(dev, f32):
    """The base case ends slots at step 1, mid-rollout by x and by theta, by
    the time limit, and not at all; a slot that ended at step k matches the
    oracle's own k-step rollout: nothing touched it afterwards."""
    c = build_case("cartpole_base", f32)
    y64, e32, info = oracle("cartpole_base", f32)
    es, n = info["end_step"], c["n_steps"]
    assert es[0] == 1 and 1 < es[1] < n and 1 < es[2] < n and es[3] == 3, es
    assert (es[4:] == 0).all(), es
    assert abs(y64["state"][1, 0]) > 2.4 and abs(y64["state"][2, 2]) > 0.2094
    assert abs(y64["state"][3, 0]) < 2.4 and abs(y64["state"][3, 2]) < 0.2094
    got = run_case(dev, "cartpole_base", f32)
    for b in np.nonzero(es > 0)[0]:
        k = int(es[b])
        yk, ek = fp32_error_scale(cartpole_rollout, c["state"], c["net"], k)
        assert got["member_steps"][b] == k and got["alive"][b] == 0.0
        assert got["rew_total"][b] == k
        for key in float_keys("cartpole"):
            r = max_ratio(got[key][b], yk[key][b], ek[key])
            assert r <= ERR_FACTOR, (b, key, r)
    for b in np.nonzero(es == 0)[0]:
        assert got["member_steps"][b] == n and got["alive"][b] == 1.0
    assert got["env_steps"][3] == CP_MAX_STEPS


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_classic_episode_pendulum_time_limit(dev, f32):
    y64, e32, info = oracle("pendulum_time_limit", f32)
    assert info["end_step"].tolist() == [0, 0, 3] + [0] * 6
    got = run_case(dev, "pendulum_time_limit", f32)
    assert got["env_steps"][2] == PD_MAX_STEPS and got["member_steps"][2] == 3
    assert got["alive"].tolist() == [1, 1, 0] + [1] * 6


@pytest.mark.parametrize("case", [("cartpole_base", False), ("pendulum_base", False),
                                  ("cartpole_base", True)], ids=case_id)
def test_classic_episode_noise_on(dev, case):
    """ac_std 0.3, every slot but the last noisy: the whole rollout matches
    the oracle drawing the same Philox noise; the last slot (>=
    noiseless_from) matches the noise-off oracle of its slot, and the noisy
    slots measurably left it."""
    name, f32 = case
    kind = CASES[name][0]
    y64, e32, info = oracle(name, f32, noise_on=True)
    got = run_case(dev, name, f32, noise_on=True)
    check(case_id(case) + "_noise_on", kind, got, y64, e32)
    y_off, e_off, _ = oracle(name, f32)
    last = slice(CASES[name][2] - 1, None)
    check(case_id(case) + "_noise_on_last_slot_vs_noise_off", kind, got, y_off, e_off,
          slots=last)
    key = "state" if kind == "cartpole" else "th"
    assert np.abs(got[key][:-1] - y_off[key][:-1]).max() > 1e-3


@pytest.mark.parametrize("case", [("cartpole_base", False), ("pendulum_time_limit", False),
                                  ("cartpole_eps2", True)], ids=case_id)
def test_classic_episode_split_and_repeat_bitwise(dev, case):
    """5 + 7 steps (salt_base 0, then 5) == one 12-step launch, bit for bit,
    with noise on so that the salt matters; and a repeat launch is bitwise
    equal."""
    name, f32 = case
    c = build_case(name, f32)
    one = run_case(dev, name, f32, noise_on=True)
    again = run_case(dev, name, f32, noise_on=True)
    g = DeviceSlots(dev, c, case_noise(c))
    assert g.launch(5, salt_base=0) == 0
    mid = g.read()
    assert g.launch(7, salt_base=5) == 0
    two = g.read()
    assert not np.array_equal(mid["member_steps"], two["member_steps"])
    for k in state_keys(c["kind"]):
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), k
        assert np.array_equal(one[k].view(np.uint8), again[k].view(np.uint8)), k


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_classic_episode_argument_errors_and_noops(dev, f32):
    """Shape errors pass mlp_shape_init's codes through, the kernel's own
    limits have codes of their own, and nothing launches in either case;
    n_slots or n_steps <= 0 is a no-op returning 0."""
    c = build_case("cartpole_base", f32)
    g = DeviceSlots(dev, c)
    before = g.read()

    def unchanged():
        now = g.read()
        return all(np.array_equal(before[k].view(np.uint8), now[k].view(np.uint8))
                   for k in CARTPOLE_KEYS)

    assert g.launch(0) == 0 and unchanged()
    assert g.launch(-3) == 0 and unchanged()
    assert g.launch(4, n_slots=0) == 0 and unchanged()
    assert g.launch(4, env_kind=2) == -113 and unchanged()
    assert g.launch(4, env_kind=-1) == -113 and unchanged()
    assert g.launch(4, ob_dim=5) == -114 and unchanged()
    assert g.launch(4, env_kind=1) == -114 and unchanged()   # Pendulum wants 3
    good = g.dims
    for dims, want in (([5, 8, 1], -114),           # observation width
                       ([4, 16, 0], -115),          # no output
                       ([4, 2049, 1], -101),        # dim > ES_MAXDIM
                       ([4] * 10, -100)):           # 9 layers > ES_MAXL
        g.dims = np.array(dims, dtype=np.int32)
        assert g.launch(4) == want and unchanged(), dims
    g.dims = good
    g.stride = 8                                    # row_stride < n
    assert g.launch(4) == -102 and unchanged()
