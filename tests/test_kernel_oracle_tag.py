"""es_tag_episode against the float64 oracle (tests/oracle64_tag.py).

Every case calls the kernel directly on test-owned buffers and asserts
``|kernel - oracle64| <= 16 * E32`` per state buffer, E32 being the error of
the same rollout evaluated in numpy float32; ``steps`` and ``alive`` must match
exactly. The state buffers are read at launch and written back, so they
cannot start as NaN; instead every buffer carries one more game row than the
launch covers, filled with NaN, which must still be NaN afterwards.

A catch is a threshold (d < 0.3): a game whose float64 distance comes within
1e-3 of it could legitimately end a step apart in fp32. The seeds below were
chosen so that NO game does (asserted on the oracle alone, cap zero).

Measured on MI355X, max |err| / E32 over the buffers of each case (bound: 16):

  case                            ratio  worst buffer  its E32
  base                             1.24  rew_total     2.63e-06
  asymmetric                       1.87  ob_sumsq      5.37e-06
  flagship_width                   0.84  ob_sumsq      7.94e-07
  noise_on                         1.24  rew_total     2.62e-06
  noise_on_last_game_vs_noise_off  1.24  rew_total     2.63e-06

Oracle catch steps of the base case: games 0 and 1 end at steps 1 and 3, the
other seven never; smallest margin 0.0195 (noise on: 0.0228).
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import ERR_FACTOR, fp32_error_scale, max_ratio
from tests.oracle64_tag import TAG_KEYS, tag_rollout, tag_state
from tests.test_kernel_oracle_mlp import bf16_tensor, make_net

pytestmark = pytest.mark.gpu

MARGIN_MIN = 1e-3
N_CLOSE = 4                               # games 0..3 start close
CLOSE_DIST = (0.2, 0.4, 0.6, 0.8)         # runner's distance from the chaser
FLOAT_KEYS = ("p", "v", "rew_total", "ob_sum", "ob_sumsq")

# name -> (dims0, dims1, games, steps, (stride_pad0, stride_pad1),
#          (ob_clip0, ob_clip1), rng seed)
CASES = {
    "base": ([8, 16, 2], [8, 16, 2], 9, 12, (0, 0), (5.0, 5.0), 4),
    "asymmetric": ([8, 16, 2], [8, 32, 32, 2], 9, 12, (0, 8), (5.0, 1.5), 6),
    "flagship_width": ([8, 256, 256, 2], [8, 256, 256, 2], 5, 6, (0, 0), (5.0, 5.0), 3),
}
NOISE = dict(seed=20240607, ac_std=(0.05, 0.05), noiseless_from=8)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def make_starts(rng, B):
    """p (B, 2, 2): games 0..3 with the runner CLOSE_DIST from the chaser in a
    random direction, the others at least 1.5 apart, all within +-2.5."""
    p = np.zeros((B, 2, 2), dtype=np.float32)
    for b in range(B):
        while True:
            c = rng.uniform(-2.0, 2.0, size=2)
            if b < N_CLOSE:
                th = rng.uniform(0, 2 * np.pi)
                r = c + CLOSE_DIST[b] * np.array([np.cos(th), np.sin(th)])
            else:
                r = rng.uniform(-2.5, 2.5, size=2)
            if np.abs(r).max() <= 2.5 and (b < N_CLOSE or np.linalg.norm(r - c) >= 1.5):
                break
        p[b, 0], p[b, 1] = c, r
    return p


def build_case(name):
    dims0, dims1, B, n_steps, pads, clips, seed = CASES[name]
    rng = np.random.RandomState(seed)
    nets, dev_nets = [], []
    for dims, pad, clip in zip((dims0, dims1), pads, clips):
        wbits, wvals, stride = make_net(rng, dims, B, pad)
        obmean = (rng.randn(8) * 0.3).astype(np.float32)
        obstd = (rng.rand(8) + 0.5).astype(np.float32)
        nets.append(dict(dims=dims, weight_rows=wvals, obmean=obmean, obstd=obstd,
                         ob_clip=clip, act_final=1))
        dev_nets.append(dict(dims=dims, wbits=wbits, stride=stride, obmean=obmean,
                             obstd=obstd, ob_clip=clip))
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
        # the oracle alone: no game on the catch threshold, and single
        # precision plays the same game
        assert int((info["margin"] < MARGIN_MIN).sum()) == 0, (name, info["margin"])
        assert np.array_equal(info["catch_step"], info32["catch_step"]), name
        _ORACLE[key] = (y64, e32, info)
    return _ORACLE[key]


class DeviceGame:
    """Device copies of a case: state with one NaN guard row, both nets."""

    def __init__(self, dev, c, noise=None):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.dev, self.B = dev, c["B"]
        self.state = {}
        for k in TAG_KEYS:
            a = np.asarray(c["state"][k])
            g = np.full((1,) + a.shape[1:], np.nan, dtype=a.dtype)
            self.state[k] = t(np.concatenate([a, g], axis=0))
        self.nets = []
        for n in c["dev_nets"]:
            self.nets.append(dict(w=bf16_tensor(n["wbits"], dev), mean=t(n["obmean"]),
                                  std=t(n["obstd"]), stride=n["stride"],
                                  dims=np.array(n["dims"], dtype=np.int32),
                                  clip=n["ob_clip"]))
        self.seed = self.acstd = None
        self.noiseless_from = 0
        if noise is not None:
            self.seed = t(np.array([noise["seed"]], np.int64))
            self.acstd = [t(np.array([s], np.float32)) for s in noise["ac_std"]]
            self.noiseless_from = noise["noiseless_from"]

    def launch(self, n_steps, salt_base=0, n_games=None, n_agents=2, ob_dim=8):
        from es_pytorch_amd import ops
        s, (n0, n1) = self.state, self.nets
        ptr = lambda x: x.data_ptr() if x is not None else None
        rc = ops.hip().es_tag_episode(
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

    def read(self):
        """Host copy of the B games; the guard row must still be NaN."""
        out = {}
        for k, v in self.state.items():
            a = v.cpu().numpy()
            assert np.isnan(a[self.B:]).all(), f"{k}: guard row written"
            out[k] = a[:self.B]
        return out


def run_case(dev, name, noise=None):
    c = build_case(name)
    g = DeviceGame(dev, c, noise)
    assert g.launch(c["n_steps"]) == 0
    return g.read()


def check(name, got, y64, e32, games=slice(None)):
    assert np.array_equal(got["steps"][games], y64["steps"][games]), name
    assert np.array_equal(got["alive"][games], y64["alive"][games]), name
    worst = (0.0, "")
    for k in FLOAT_KEYS:
        assert np.isfinite(got[k]).all(), (name, k)
        r = max_ratio(got[k][games], y64[k][games], e32[k])
        print(f"ORACLE-RATIO tag {name} {k} ratio={r:.2f} E32={e32[k]:.3g}")
        worst = max(worst, (r, k))
    print(f"ORACLE-RATIO tag {name} worst ratio={worst[0]:.2f} ({worst[1]})")
    for k in FLOAT_KEYS:
        r = max_ratio(got[k][games], y64[k][games], e32[k])
        assert r <= ERR_FACTOR, (name, k, r, e32[k])


@pytest.mark.parametrize("name", list(CASES))
def test_tag_episode_matches_oracle(dev, name):
    y64, e32, info = oracle(name)
    got = run_case(dev, name)
    check(name, got, y64, e32)


def test_tag_episode_base_game_endings(dev):
    """The base case ends games at step 1, mid-episode and not at all; a game
    that ended at step k has steps == k, rewards that stop there and p/v
    holding the terminal state."""
    c = build_case("base")
    y64, e32, info = oracle("base")
    cs = info["catch_step"]
    n = c["n_steps"]
    assert (cs == 1).any() and ((cs > 1) & (cs < n)).any() and (cs == 0).any(), cs
    got = run_case(dev, "base")
    for b in np.nonzero(cs > 0)[0]:
        k = int(cs[b])
        # the oracle's own k-step rollout of this game: nothing after step k
        # may have touched the state
        yk, ek = fp32_error_scale(tag_rollout, c["state"], c["nets"], k)
        assert got["steps"][b] == k and got["alive"][b] == 0.0
        for key in FLOAT_KEYS:
            r = max_ratio(got[key][b], yk[key][b], ek[key])
            assert r <= ERR_FACTOR, (b, key, r)
        d = np.linalg.norm(got["p"][b, 0] - got["p"][b, 1])
        assert d < 0.3, (b, d)
    for b in np.nonzero(cs == 0)[0]:
        assert got["steps"][b] == n and got["alive"][b] == 1.0


def test_tag_episode_noise_on(dev):
    """ac_std 0.05 on both agents, games 0..7 noisy: the whole rollout matches
    the oracle drawing the same Philox noise; the last game (>=
    noiseless_from) matches the noise-off oracle of its slot."""
    y64, e32, info = oracle("base", NOISE)
    got = run_case(dev, "base", NOISE)
    check("noise_on", got, y64, e32)
    y_off, e_off, _ = oracle("base")
    last = slice(NOISE["noiseless_from"], None)
    check("noise_on_last_game_vs_noise_off", got, y_off, e_off, games=last)
    # and the noise is really on: the noisy games left the noise-off path
    assert np.abs(got["p"][:8] - y_off["p"][:8]).max() > 1e-3


def test_tag_episode_split_launches_bitwise(dev):
    """5 + 7 steps (salt_base 0, then 5) == one 12-step launch, bit for bit,
    with noise on so that the salt matters."""
    c = build_case("base")
    one = run_case(dev, "base", NOISE)
    g = DeviceGame(dev, c, NOISE)
    assert g.launch(5, salt_base=0) == 0
    mid = g.read()
    assert g.launch(7, salt_base=5) == 0
    two = g.read()
    assert not np.array_equal(mid["steps"], two["steps"])
    for k in TAG_KEYS:
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), k


def test_tag_episode_repeat_bitwise(dev):
    a = run_case(dev, "base", NOISE)
    b = run_case(dev, "base", NOISE)
    for k in TAG_KEYS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_tag_episode_argument_errors_and_noops(dev):
    """Shape errors pass mlp_shape_init's codes through, the game's limits
    have codes of their own, and nothing launches in either case; n_games or
    n_steps <= 0 is a no-op returning 0."""
    c = build_case("base")
    g = DeviceGame(dev, c)
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
