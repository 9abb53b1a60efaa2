"""es_tag_episode_f32 against the float64 oracle (tests/oracle64_tag.py).

The fp32-rows twin of tests/test_kernel_oracle_tag.py, whose helpers it uses:
direct calls on test-owned buffers, ``|kernel - oracle64| <= 16 * E32`` per
state buffer (E32: the same rollout in numpy float32), ``steps`` and ``alive``
exact, one NaN guard row behind every state buffer. The weight blobs are drawn
as ``make_net`` draws them, but the float32 values are kept unrounded.

Every case asserts on the oracle alone, cap zero, that no game comes within
1e-3 of the catch threshold and that float32 ends the same games at the same
steps.

``scalar_walks`` covers the two ways a 16-byte fp32 load could go misaligned:
policy 0 has row stride 185 floats (% 4 == 1), so every layer must take the
scalar walk; policy 1 has a 6-wide layer, so the next weight block starts at
element 54 (% 4 == 2).

Measured on MI355X, max |err| / E32 over the buffers of each case (bound: 16):

  case                            ratio  worst buffer  its E32
  base                             1.00  ob_sumsq      8.51e-06
  asymmetric                       1.00  rew_total     3.89e-06
  flagship_width                   0.97  p             1.14e-07
  scalar_walks                     1.31  p             3.89e-07
  noise_on                         1.00  rew_total     4.14e-06
  noise_on_last_game_vs_noise_off  0.98  rew_total     2.63e-06

Teeth: the base case's values rounded to bf16 and run through es_tag_episode
sit 8 895 (rew_total) to 25 180 (ob_sum) x E32 from the fp32-rows oracle.

Oracle catch steps (noise off; the same with noise on) and smallest margins
(noise off / on): base 1, 3, never x7, 0.0194 / 0.0227; asymmetric 1, 3, 5,
never x6, 0.0173 / 0.0164; flagship_width 1, 2, 6, never x2, 0.0132 / 0.0108;
scalar_walks 1, never, 4, never x6, 0.0541 / 0.0543.
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import ERR_FACTOR, f32_to_bf16_bits, fp32_error_scale, max_ratio, n_params
from tests.oracle64_tag import TAG_KEYS, tag_rollout, tag_state
from tests.test_kernel_oracle_tag import (FLOAT_KEYS, MARGIN_MIN, NOISE, DeviceGame, check,
                                          make_starts)

pytestmark = pytest.mark.gpu

# name -> (dims0, dims1, games, steps, (stride_pad0, stride_pad1),
#          (ob_clip0, ob_clip1), rng seed)
CASES = {
    "base": ([8, 16, 2], [8, 16, 2], 9, 12, (0, 0), (5.0, 5.0), 4),
    "asymmetric": ([8, 16, 2], [8, 32, 32, 2], 9, 12, (0, 8), (5.0, 1.5), 6),
    "flagship_width": ([8, 256, 256, 2], [8, 256, 256, 2], 5, 6, (0, 0), (5.0, 5.0), 3),
    "scalar_walks": ([8, 16, 2], [8, 6, 16, 2], 9, 12, (1, 0), (5.0, 5.0), 7),
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def make_net_f32(rng, dims, rows, stride_pad=0):
    """make_net's blob (rows + 1 rows, the same draws and scales) with the
    float32 values kept as they are; returns (float32 array, stride)."""
    n = n_params(dims)
    stride = (n + 7) // 8 * 8 + stride_pad
    w = np.zeros((rows + 1, stride), dtype=np.float32)
    off = 0
    for I, O in zip(dims[:-1], dims[1:]):
        w[:, off:off + I * O] = rng.randn(rows + 1, I * O) * (0.7 / np.sqrt(I))
        off += I * O
        w[:, off:off + O] = rng.randn(rows + 1, O) * 0.1
        off += O
    return w, stride


def build_case(name):
    dims0, dims1, B, n_steps, pads, clips, seed = CASES[name]
    rng = np.random.RandomState(seed)
    nets, dev_nets = [], []
    for dims, pad, clip in zip((dims0, dims1), pads, clips):
        w, stride = make_net_f32(rng, dims, B, pad)
        obmean = (rng.randn(8) * 0.3).astype(np.float32)
        obstd = (rng.rand(8) + 0.5).astype(np.float32)
        nets.append(dict(dims=dims, weight_rows=w.astype(np.float64), obmean=obmean,
                         obstd=obstd, ob_clip=clip, act_final=1))
        # wbits: the same values rounded to bf16, for the dtype's teeth
        dev_nets.append(dict(dims=dims, w32=w, wbits=f32_to_bf16_bits(w), stride=stride,
                             obmean=obmean, obstd=obstd, ob_clip=clip))
    state = tag_state(make_starts(rng, B))
    return dict(B=B, n_steps=n_steps, nets=nets, dev_nets=dev_nets, state=state)


_ORACLE = {}


def oracle(name, noise=None):
    """(y64, E32, info64) of the case's whole rollout; computed once."""
    key = (name, noise is not None)
    if key not in _ORACLE:
        c = build_case(name)
        y64, e32 = fp32_error_scale(tag_rollout, c["state"], c["nets"], c["n_steps"],
                                    noise=noise)
        _, info = tag_rollout(c["state"], c["nets"], c["n_steps"], noise=noise)
        _, info32 = tag_rollout(c["state"], c["nets"], c["n_steps"], dtype=np.float32,
                                noise=noise)
        assert int((info["margin"] < MARGIN_MIN).sum()) == 0, (name, info["margin"])
        assert np.array_equal(info["catch_step"], info32["catch_step"]), name
        _ORACLE[key] = (y64, e32, info)
    return _ORACLE[key]


class DeviceGameF32(DeviceGame):
    """DeviceGame with float32 weight blobs, launched through
    es_tag_episode_f32."""

    def __init__(self, dev, c, noise=None):
        super().__init__(dev, c, noise)
        for net, n in zip(self.nets, c["dev_nets"]):
            net["w"] = torch.from_numpy(np.ascontiguousarray(n["w32"])).to(dev)
            assert net["w"].dtype == torch.float32

    def launch(self, n_steps, salt_base=0, n_games=None, n_agents=2, ob_dim=8):
        from es_pytorch_amd import ops
        s, (n0, n1) = self.state, self.nets
        ptr = lambda x: x.data_ptr() if x is not None else None
        rc = ops.hip().es_tag_episode_f32(
            s["p"].data_ptr(), s["v"].data_ptr(), s["alive"].data_ptr(),
            s["steps"].data_ptr(), s["rew_total"].data_ptr(), s["ob_sum"].data_ptr(),
            s["ob_sumsq"].data_ptr(), n0["w"].data_ptr(), n1["w"].data_ptr(),
            n0["mean"].data_ptr(), n1["mean"].data_ptr(), n0["std"].data_ptr(),
            n1["std"].data_ptr(), n0["dims"].ctypes.data, len(n0["dims"]),
            n1["dims"].ctypes.data, len(n1["dims"]), n0["stride"], n1["stride"],
            n0["clip"], n1["clip"], ptr(self.acstd[0] if self.acstd else None),
            ptr(self.acstd[1] if self.acstd else None), ptr(self.seed), salt_base,
            n_agents, ob_dim, self.B if n_games is None else n_games, n_steps, 1,
            self.noiseless_from, torch.cuda.current_stream(self.dev).cuda_stream)
        torch.cuda.synchronize(self.dev)
        return rc


def run_case(dev, name, noise=None):
    c = build_case(name)
    g = DeviceGameF32(dev, c, noise)
    assert g.launch(c["n_steps"]) == 0
    return g.read()


def test_cases_take_the_paths_they_name():
    """The alignment facts the scalar_walks case rests on."""
    d0, d1, _, _, pads, _, _ = CASES["scalar_walks"]
    assert ((n_params(d0) + 7) // 8 * 8 + pads[0]) == 185 and 185 % 4 == 1
    assert d1[1] == 6 and (d1[0] * d1[1] + d1[1]) == 54 and 54 % 4 == 2


@pytest.mark.parametrize("name", list(CASES))
def test_tag_episode_f32_matches_oracle(dev, name):
    y64, e32, info = oracle(name)
    got = run_case(dev, name)
    check("f32 " + name, got, y64, e32)


def test_tag_episode_f32_base_game_endings(dev):
    """A game that ended at step k has steps == k, rewards that stop there and
    p/v holding the terminal state, with d < 0.3."""
    c = build_case("base")
    y64, e32, info = oracle("base")
    cs = info["catch_step"]
    n = c["n_steps"]
    assert (cs == 1).any() and ((cs > 1) & (cs < n)).any() and (cs == 0).any(), cs
    got = run_case(dev, "base")
    for b in np.nonzero(cs > 0)[0]:
        k = int(cs[b])
        yk, ek = fp32_error_scale(tag_rollout, c["state"], c["nets"], k)
        assert got["steps"][b] == k and got["alive"][b] == 0.0
        for key in FLOAT_KEYS:
            r = max_ratio(got[key][b], yk[key][b], ek[key])
            assert r <= ERR_FACTOR, (b, key, r)
        d = np.linalg.norm(got["p"][b, 0] - got["p"][b, 1])
        assert d < 0.3, (b, d)
    for b in np.nonzero(cs == 0)[0]:
        assert got["steps"][b] == n and got["alive"][b] == 1.0


def test_tag_episode_f32_noise_on(dev):
    """ac_std 0.05 on both agents, games 0..7 noisy: the rollout matches the
    oracle drawing the same Philox noise; the last game (>= noiseless_from)
    matches the noise-off oracle of its slot."""
    y64, e32, info = oracle("base", NOISE)
    got = run_case(dev, "base", NOISE)
    check("f32 noise_on", got, y64, e32)
    y_off, e_off, _ = oracle("base")
    last = slice(NOISE["noiseless_from"], None)
    check("f32 noise_on_last_game_vs_noise_off", got, y_off, e_off, games=last)
    assert np.abs(got["p"][:8] - y_off["p"][:8]).max() > 1e-3


def test_tag_episode_f32_split_launches_bitwise(dev):
    """5 + 7 steps (salt_base 0, then 5) == one 12-step launch, bit for bit,
    with noise on so that the salt matters."""
    c = build_case("base")
    one = run_case(dev, "base", NOISE)
    g = DeviceGameF32(dev, c, NOISE)
    assert g.launch(5, salt_base=0) == 0
    mid = g.read()
    assert g.launch(7, salt_base=5) == 0
    two = g.read()
    assert not np.array_equal(mid["steps"], two["steps"])
    for k in TAG_KEYS:
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), k


def test_tag_episode_f32_repeat_bitwise(dev):
    a = run_case(dev, "base", NOISE)
    b = run_case(dev, "base", NOISE)
    for k in TAG_KEYS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_tag_episode_f32_argument_errors_and_noops(dev):
    """The codes of es_tag_episode, and nothing launches in any of them."""
    c = build_case("base")
    g = DeviceGameF32(dev, c)
    before = g.read()

    def unchanged():
        now = g.read()
        return all(np.array_equal(before[k].view(np.uint8), now[k].view(np.uint8))
                   for k in TAG_KEYS)

    assert g.launch(0) == 0 and unchanged()
    assert g.launch(-3) == 0 and unchanged()
    assert g.launch(4, n_games=0) == 0 and unchanged()
    assert g.launch(4, n_agents=3) == -112 and unchanged()
    assert g.launch(4, ob_dim=9) == -110 and unchanged()
    good = g.nets[1]["dims"]
    for dims, want in (([9, 8, 2], -110),           # observation width
                       ([8, 16, 1], -111),          # fewer than two outputs
                       ([8, 2049, 2], -101),        # dim > ES_MAXDIM
                       ([8] * 10, -100)):           # 9 layers > ES_MAXL
        g.nets[1]["dims"] = np.array(dims, dtype=np.int32)
        assert g.launch(4) == want and unchanged(), dims
    g.nets[1]["dims"] = good
    g.nets[1]["stride"] = 8                        # row_stride < n
    assert g.launch(4) == -102 and unchanged()


def test_bf16_rows_miss_the_fp32_oracle(dev):
    """Teeth for the dtype: the base case's values rounded to bf16 and run
    through es_tag_episode miss the fp32-rows oracle on at least one buffer,
    so a kernel that silently read bf16 would not pass the cases above."""
    c = build_case("base")
    y64, e32, _ = oracle("base")
    g = DeviceGame(dev, c)                 # bf16 blobs from the same values
    assert g.nets[0]["w"].dtype == torch.bfloat16
    assert g.launch(c["n_steps"]) == 0
    got = g.read()
    ratios = {k: max_ratio(got[k], y64[k], e32[k]) for k in FLOAT_KEYS}
    print("ORACLE-RATIO tag f32 teeth (bf16 rows vs fp32 oracle)",
          {k: round(float(r), 1) for k, r in ratios.items()})
    assert max(ratios.values()) > ERR_FACTOR, ratios
