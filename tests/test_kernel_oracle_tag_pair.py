"""es_tag_pair_episode against the float64 oracle (tests/oracle64_tag.py).

The pair form of tests/test_kernel_oracle_tag.py, whose helpers it uses: direct
calls on test-owned buffers, ``|kernel - oracle64| <= 16 * E32`` per float
state buffer (E32: the same rollout in numpy float32), ``steps`` and ``alive``
exact, one NaN guard row behind every state buffer, which must still be NaN
after every launch (the noiseless block's missing "-" member included). The
theta blob (one row) and the sigma*eps blob carry a guard row of bf16 NaNs.

The oracle's weight rows are ``f64(bf16 theta) +- f64(bf16 eps_p)``, built from
the bit patterns the kernel is given, in the slot order [+pairs | -pairs |
single]; the single game runs on ``bf16 theta``. The oracle's float32 run
rounds that sum to fp32, as the kernel's ``t + e`` does.

Every case asserts on the oracle alone, cap zero, that no game comes within
1e-3 of the catch threshold and that float32 ends the same games at the same
steps. The start positions put the runner 0.2 from the chaser in game 0 (the
"+" game of pair 0) and in game pairs + 1 (the "-" game of pair 1), and 0.2 /
0.5 apart in the two games of pair 2 where there is one, so that one game of a
block ends while its partner plays on, either way round.

Measured on MI355X, max |err| / E32 over the buffers of each case (bound: 16):

  case                                     ratio  worst buffer  its E32
  base                                      1.76  rew_total     2.29e-06
  asymmetric                                1.00  rew_total     7.94e-06
  misaligned                                1.00  p             1.28e-07
  wide_scalar                               2.45  p             1.45e-07
  flagship_width                            2.38  rew_total     1.01e-06
  no_single                                 1.00  p             1.90e-07
  base noise_on                             1.95  rew_total     2.29e-06
  base noise_on_single_vs_noise_off         1.35  rew_total     2.29e-06
  asymmetric noise_on                       1.19  v             9.64e-08
  asymmetric noise_on_single_vs_noise_off   0.56  ob_sum        1.77e-06

With every eps row zero the pair launch equalled es_tag_episode bit for bit in
all six cases, noise on: no layer kind of mlp_layers_pair differs from
mlp_layers in tiling or accumulation order.

Oracle catch steps, noise off (0: never): base 1, 0, 1, 0 | 0, 1, 6, 0 | 0
(noise on: the 6 is a 5), smallest margin 0.0185 (0.0238); asymmetric 1, 0, 1,
0 | 0, 1, 0, 0 | 0, margin 0.0846 (0.0870); misaligned, wide_scalar and
flagship_width 1, 0 | 0, 1 | 0, margins 0.0777, 0.1188, 0.0887; no_single 1, 0,
1 | 0, 1, 0, margin 0.1014.
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import (ERR_FACTOR, bf16_bits_to_f64, f32_to_bf16_bits, fp32_error_scale,
                            max_ratio, n_params)
from tests.oracle64_tag import TAG_KEYS, tag_rollout, tag_state
from tests.test_kernel_oracle_mlp import bf16_tensor
from tests.test_kernel_oracle_tag import FLOAT_KEYS, MARGIN_MIN, DeviceGame, check

pytestmark = pytest.mark.gpu

BF16_NAN = 0x7FC0
EPS_SCALE = 0.05                 # sigma*eps against weights of 0.7 / sqrt(I)
NOISE_SEED, AC_STD = 20240607, (0.05, 0.05)

# name -> (dims0, dims1, pairs, single, steps, (stride_pad0, stride_pad1),
#          (ob_clip0, ob_clip1), rng seed)
CASES = {
    "base": ([8, 16, 2], [8, 16, 2], 4, 1, 12, (0, 0), (5.0, 5.0), 4),
    "asymmetric": ([8, 16, 2], [8, 32, 32, 2], 4, 1, 12, (0, 8), (5.0, 1.5), 1),
    "misaligned": ([8, 12, 16, 2], [8, 16, 2], 2, 1, 8, (0, 0), (5.0, 5.0), 1),
    "wide_scalar": ([8, 132, 2], [8, 16, 2], 2, 1, 6, (0, 0), (5.0, 5.0), 1),
    "flagship_width": ([8, 256, 256, 2], [8, 256, 256, 2], 2, 1, 6, (0, 0), (5.0, 5.0), 1),
    "no_single": ([8, 16, 2], [8, 16, 2], 3, 0, 8, (0, 0), (5.0, 5.0), 1),
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def close_games(pairs):
    """game -> runner's start distance from the chaser, for the close games."""
    close = {0: 0.2, pairs + 1: 0.2}
    if pairs >= 3:
        close[2], close[pairs + 2] = 0.2, 0.5
    return close


def make_pair_starts(rng, pairs, single):
    """p (B, 2, 2): the close_games as they say, the others at least 1.5 apart,
    all within +-2.5."""
    B = 2 * pairs + single
    close = close_games(pairs)
    p = np.zeros((B, 2, 2), dtype=np.float32)
    for b in range(B):
        while True:
            c = rng.uniform(-2.0, 2.0, size=2)
            if b in close:
                th = rng.uniform(0, 2 * np.pi)
                r = c + close[b] * np.array([np.cos(th), np.sin(th)])
            else:
                r = rng.uniform(-2.5, 2.5, size=2)
            if np.abs(r).max() <= 2.5 and (b in close or np.linalg.norm(r - c) >= 1.5):
                break
        p[b, 0], p[b, 1] = c, r
    return p


def make_pair_net(rng, dims, pairs, single, stride_pad):
    """(theta bits (2, stride), eps bits (pairs + single + 1, stride), stride):
    theta drawn as make_net draws a row, eps at EPS_SCALE, the single block's
    eps row zero, the last row of each blob NaN."""
    n = n_params(dims)
    stride = (n + 7) // 8 * 8 + stride_pad
    th = np.zeros((2, stride), dtype=np.float32)
    off = 0
    for I, O in zip(dims[:-1], dims[1:]):
        th[0, off:off + I * O] = rng.randn(I * O) * (0.7 / np.sqrt(I))
        off += I * O
        th[0, off:off + O] = rng.randn(O) * 0.1
        off += O
    ep = np.zeros((pairs + single + 1, stride), dtype=np.float32)
    ep[:pairs, :n] = rng.randn(pairs, n) * EPS_SCALE
    tbits, ebits = f32_to_bf16_bits(th), f32_to_bf16_bits(ep)
    tbits[-1] = BF16_NAN
    ebits[-1] = BF16_NAN
    return tbits, ebits, stride


def pair_rows(tbits, ebits, pairs, single):
    """The effective rows in slot order, float64, from the bit patterns."""
    t = bf16_bits_to_f64(tbits[0])[None, :]
    e = bf16_bits_to_f64(ebits[:pairs])
    rows = [t + e, t - e]
    if single:
        assert not ebits[pairs].any()
        rows.append(t)
    return np.concatenate(rows, axis=0)


def build_case(name, zero_eps=False):
    dims0, dims1, pairs, single, n_steps, pads, clips, seed = CASES[name]
    rng = np.random.RandomState(seed)
    B = 2 * pairs + single
    nets, dev_nets = [], []
    for dims, pad, clip in zip((dims0, dims1), pads, clips):
        tbits, ebits, stride = make_pair_net(rng, dims, pairs, single, pad)
        if zero_eps:
            ebits[:-1] = 0
        obmean = (rng.randn(8) * 0.3).astype(np.float32)
        obstd = (rng.rand(8) + 0.5).astype(np.float32)
        nets.append(dict(dims=dims, weight_rows=pair_rows(tbits, ebits, pairs, single),
                         obmean=obmean, obstd=obstd, ob_clip=clip, act_final=1))
        # wbits: B copies of the theta row (and a NaN guard row), what
        # es_tag_episode is given in the zero-eps comparison
        wbits = np.concatenate([np.repeat(tbits[:1], B, axis=0), tbits[1:]], axis=0)
        dev_nets.append(dict(dims=dims, wbits=wbits, tbits=tbits, ebits=ebits, stride=stride,
                             obmean=obmean, obstd=obstd, ob_clip=clip))
    state = tag_state(make_pair_starts(rng, pairs, single))
    return dict(B=B, pairs=pairs, single=single, n_steps=n_steps, nets=nets,
                dev_nets=dev_nets, state=state)


def noise_of(name):
    pairs = CASES[name][2]
    return dict(seed=NOISE_SEED, ac_std=AC_STD, noiseless_from=2 * pairs)


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


class PairGame(DeviceGame):
    """DeviceGame plus the theta and sigma*eps blobs; launch() is the pair
    kernel, DeviceGame.launch (es_tag_episode on the B theta copies) stays
    reachable as launch_per_game()."""

    def __init__(self, dev, c, noise=None):
        super().__init__(dev, c, noise)
        self.pairs, self.single = c["pairs"], c["single"]
        for net, n in zip(self.nets, c["dev_nets"]):
            net["theta"] = bf16_tensor(n["tbits"], dev)
            net["eps"] = bf16_tensor(n["ebits"], dev)

    launch_per_game = DeviceGame.launch

    def launch(self, n_steps, salt_base=0, n_pairs=None, n_single=None, n_agents=2,
               ob_dim=8):
        from es_pytorch_amd import ops
        s, (n0, n1) = self.state, self.nets
        ptr = lambda x: x.data_ptr() if x is not None else None
        rc = ops.hip().es_tag_pair_episode(
            s["p"].data_ptr(), s["v"].data_ptr(), s["alive"].data_ptr(),
            s["steps"].data_ptr(), s["rew_total"].data_ptr(), s["ob_sum"].data_ptr(),
            s["ob_sumsq"].data_ptr(), n0["theta"].data_ptr(), n1["theta"].data_ptr(),
            n0["eps"].data_ptr(), n1["eps"].data_ptr(),
            n0["mean"].data_ptr(), n1["mean"].data_ptr(), n0["std"].data_ptr(),
            n1["std"].data_ptr(), n0["dims"].ctypes.data, len(n0["dims"]),
            n1["dims"].ctypes.data, len(n1["dims"]), n0["stride"], n1["stride"],
            n0["clip"], n1["clip"], ptr(self.acstd[0] if self.acstd else None),
            ptr(self.acstd[1] if self.acstd else None), ptr(self.seed), salt_base,
            n_agents, ob_dim, self.pairs if n_pairs is None else n_pairs,
            self.single if n_single is None else n_single, n_steps, 1,
            self.noiseless_from, torch.cuda.current_stream(self.dev).cuda_stream)
        torch.cuda.synchronize(self.dev)
        return rc


def run_case(dev, name, noise=None):
    c = build_case(name)
    g = PairGame(dev, c, noise)
    assert g.launch(c["n_steps"]) == 0
    return g.read()


def bitwise_equal(a, b):
    return [k for k in TAG_KEYS if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]


def test_cases_take_the_paths_they_name():
    """The layout facts the misaligned and wide_scalar cases rest on."""
    d = CASES["misaligned"][0]
    assert d[0] * d[1] + d[1] == 108 and 108 % 8 == 4 and d[2] == 16 and 256 // 16 > 1
    assert d[1] % 8 != 0 and 256 // d[1] > 1
    assert 256 // CASES["wide_scalar"][0][1] == 1
    d = CASES["flagship_width"][0]
    assert d[2] % 8 == 0 and (d[0] * d[1] + d[1]) % 8 == 0
    assert 3 * (256 // (d[2] // 8)) < d[1]          # the depth-4 ring is entered
    assert CASES["no_single"][3] == 0 and all(CASES[k][3] == 1 for k in CASES
                                              if k != "no_single")


@pytest.mark.parametrize("name", list(CASES))
def test_pair_episode_matches_oracle(dev, name):
    y64, e32, info = oracle(name)
    got = run_case(dev, name)
    check("pair " + name, got, y64, e32)


@pytest.mark.parametrize("name", ["base", "asymmetric"])
def test_pair_episode_noise_on(dev, name):
    """ac_std 0.05 on both agents, every pair game noisy, the single game
    (>= noiseless_from) not: it matches the noise-off oracle of its slot."""
    noise = noise_of(name)
    y64, e32, info = oracle(name, noise)
    got = run_case(dev, name, noise)
    check(f"pair {name} noise_on", got, y64, e32)
    y_off, e_off, _ = oracle(name)
    last = slice(noise["noiseless_from"], None)
    check(f"pair {name} noise_on_single_vs_noise_off", got, y_off, e_off, games=last)
    assert np.abs(got["p"][:last.start] - y_off["p"][:last.start]).max() > 1e-3


def test_pair_episode_one_sided_catch(dev):
    """Pair 0: "+" caught early, "-" plays all steps. Pair 1: the reverse.
    Pair 2: both caught, at different steps. The game that ended holds the
    oracle's state of its catch step; nothing its partner did touched it."""
    c = build_case("base")
    y64, e32, info = oracle("base")
    cs, n, P = info["catch_step"], c["n_steps"], c["pairs"]
    assert 0 < cs[0] < n and cs[P] == 0, cs
    assert cs[1] == 0 and 0 < cs[P + 1] < n, cs
    assert cs[2] > 0 and cs[P + 2] > 0 and cs[2] != cs[P + 2], cs
    got = run_case(dev, "base")
    for b in np.nonzero(cs > 0)[0]:
        k = int(cs[b])
        yk, ek = fp32_error_scale(tag_rollout, c["state"], c["nets"], k)
        assert got["steps"][b] == k and got["alive"][b] == 0.0
        for key in FLOAT_KEYS:
            r = max_ratio(got[key][b], yk[key][b], ek[key])
            assert r <= ERR_FACTOR, (b, key, r)
        assert np.linalg.norm(got["p"][b, 0] - got["p"][b, 1]) < 0.3, b
    for b in np.nonzero(cs == 0)[0]:
        assert got["steps"][b] == n and got["alive"][b] == 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_pair_episode_zero_eps_is_per_game_kernel_bitwise(dev, name):
    """Every eps row zero: the pair launch equals es_tag_episode on n_games
    copies of the theta row, bit for bit, noise on (same tiling and
    accumulation order, t + 0 == t, and the noise keyed by the game index)."""
    c = build_case(name, zero_eps=True)
    noise = noise_of(name)
    a = PairGame(dev, c, noise)
    assert a.launch(c["n_steps"]) == 0
    b = PairGame(dev, c, noise)
    assert b.launch_per_game(c["n_steps"]) == 0
    got, ref = a.read(), b.read()
    assert ref["steps"].max() > 1 and np.isfinite(ref["rew_total"]).all()
    assert bitwise_equal(got, ref) == [], name


def test_pair_episode_split_launches_bitwise(dev):
    """5 + 7 steps (salt_base 0, then 5) == one 12-step launch, bit for bit,
    with noise on so that the salt matters; games 0, 2, 5 and 6 end in the
    first part while their partners play through both."""
    c = build_case("base")
    noise = noise_of("base")
    one = run_case(dev, "base", noise)
    g = PairGame(dev, c, noise)
    assert g.launch(5, salt_base=0) == 0
    mid = g.read()
    assert g.launch(7, salt_base=5) == 0
    two = g.read()
    assert not np.array_equal(mid["steps"], two["steps"])
    assert bitwise_equal(one, two) == []


def test_pair_episode_all_caught_changes_nothing(dev):
    """A launch on games that all arrive with alive == 0 leaves every buffer
    as it was."""
    c = build_case("base")
    g = PairGame(dev, c, noise_of("base"))
    assert g.launch(3) == 0
    g.state["alive"][:g.B].zero_()
    before = g.read()
    assert g.launch(c["n_steps"], salt_base=3) == 0
    assert bitwise_equal(before, g.read()) == []


def test_pair_episode_repeat_bitwise(dev):
    noise = noise_of("asymmetric")
    a = run_case(dev, "asymmetric", noise)
    b = run_case(dev, "asymmetric", noise)
    assert bitwise_equal(a, b) == []


def test_pair_episode_argument_errors_and_noops(dev):
    """The codes of es_tag_episode, -113 for an n_single that is neither 0 nor
    1 (or a negative n_pairs), and nothing launches in any of them; no games
    or no steps is a no-op returning 0."""
    c = build_case("base")
    g = PairGame(dev, c)
    before = g.read()
    unchanged = lambda: bitwise_equal(before, g.read()) == []

    assert g.launch(0) == 0 and unchanged()
    assert g.launch(-3) == 0 and unchanged()
    assert g.launch(4, n_pairs=0, n_single=0) == 0 and unchanged()
    assert g.launch(4, n_single=2) == -113 and unchanged()
    assert g.launch(4, n_single=-1) == -113 and unchanged()
    assert g.launch(4, n_pairs=-1) == -113 and unchanged()
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
