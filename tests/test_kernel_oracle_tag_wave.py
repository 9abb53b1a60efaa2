"""es_tag_wave_episode / es_tag_wave_episode_f32 (a wavefront per game, both
member rows in LDS, policies at most 64 wide) against the float64 oracle, with
the bound (``|kernel - oracle64| <= 16 * E32`` per float buffer, ``steps`` and
``alive`` exact, NaN guard row intact) and the helpers of
tests/tag_harness.py. The blobs are drawn as
``make_net_f32`` draws them; the bf16 rows are those values rounded. Every case
has 9 games and 12 steps, so the last block is partly empty at 4, 2 and 1 games
per block (wide64: 2 on bf16, 1 on fp32). Every oracle asserts, cap zero, that
no game comes within 1e-3 of the catch threshold and that float32 ends the
same games at the same steps.

Measured on MI355X, worst max |err| / E32 per case (bound 16), bf16 / fp32
rows: base 1.24 / 1.00, asymmetric 1.87 / 1.00, wide64 1.16 / 0.87, odd 1.47 /
1.48, mixed 1.00 / 1.29; noise on base 1.24 / 1.04, mixed 1.35 / 1.34. Oracle
catch steps (both dtypes, noise off and on): base 1, 3; asymmetric 1, 3, 5;
wide64 1, never, 8; odd 1, never, 7; mixed 1, 4; every other game never.
"""
import functools

import numpy as np
import pytest
import torch

from es_pytorch_amd import ops
from tests.oracle64 import bf16_bits_to_f64, f32_to_bf16_bits, fp32_error_scale
from tests.oracle64_tag import TAG_KEYS, tag_rollout, tag_state
from tests.tag_harness import (MARGIN_MIN, NOISE, DeviceGame, check, make_net_f32,
                               make_starts)

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)

# name -> (dims0, dims1, (stride_pad0, stride_pad1), (ob_clip0, ob_clip1), rng seed)
CASES = {
    "base": ([8, 16, 2], [8, 16, 2], (0, 0), (5.0, 5.0), 4),
    # unequal rows: the second row's offset in LDS matters
    "asymmetric": ([8, 16, 2], [8, 32, 32, 2], (0, 8), (5.0, 1.5), 6),
    # one input partition, every lane an output
    "wide64": ([8, 64, 64, 2], [8, 64, 64, 2], (0, 0), (5.0, 5.0), 5),
    # no power of two, 2, 4 and 8 partitions; misaligned rows: element-wise copy
    "odd": ([8, 24, 12, 2], [8, 6, 16, 2], (3, 1), (5.0, 1.5), 1),
    # three outputs: A_i = 3 in the noise counter
    "mixed": ([8, 64, 2], [8, 5, 3], (0, 0), (5.0, 5.0), 7),
}
B, N_STEPS = 9, 12
DTYPES = [False, True]
dtype_id = lambda f32: "f32" if f32 else "bf16"


def build_case(name, f32):
    dims0, dims1, pads, clips, seed = CASES[name]
    rng = np.random.RandomState(seed)
    nets, dev_nets = [], []
    for dims, pad, clip in zip((dims0, dims1), pads, clips):
        w, stride = make_net_f32(rng, dims, B, pad)
        wbits = f32_to_bf16_bits(w)
        obmean = (rng.randn(8) * 0.3).astype(np.float32)
        obstd = (rng.rand(8) + 0.5).astype(np.float32)
        rows = w.astype(np.float64) if f32 else bf16_bits_to_f64(wbits)
        nets.append(dict(dims=dims, weight_rows=rows, obmean=obmean, obstd=obstd,
                         ob_clip=clip, act_final=1))
        dev_nets.append(dict(dims=dims, w32=w, wbits=wbits, stride=stride, obmean=obmean,
                             obstd=obstd, ob_clip=clip))
    state = tag_state(make_starts(rng, B))
    return dict(B=B, n_steps=N_STEPS, f32=f32, nets=nets, dev_nets=dev_nets, state=state)


@functools.lru_cache(maxsize=None)
def oracle(name, f32, noisy=False):
    """(y64, E32, info64) of the case's whole rollout; computed once."""
    c, noise = build_case(name, f32), NOISE if noisy else None
    y64, e32 = fp32_error_scale(tag_rollout, c["state"], c["nets"], N_STEPS, noise=noise)
    _, info = tag_rollout(c["state"], c["nets"], N_STEPS, noise=noise)
    _, info32 = tag_rollout(c["state"], c["nets"], N_STEPS, dtype=np.float32, noise=noise)
    assert int((info["margin"] < MARGIN_MIN).sum()) == 0, (name, info["margin"])
    assert np.array_equal(info["catch_step"], info32["catch_step"]), name
    return y64, e32, info


class WaveGame(DeviceGame):
    """DeviceGame whose launch goes to the wave kernel of the case's dtype."""

    def __init__(self, dev, c, noise=None):
        super().__init__(dev, c, noise)
        self.f32 = c["f32"]
        if self.f32:
            self.use_f32_blobs(c)

    def entry(self):
        return ops.hip().es_tag_wave_episode_f32 if self.f32 else ops.hip().es_tag_wave_episode

    def shape_check(self):
        n0, n1 = self.nets
        return ops.hip().es_tag_wave_check(
            n0["dims"].ctypes.data, len(n0["dims"]), n1["dims"].ctypes.data,
            len(n1["dims"]), n0["stride"], n1["stride"], int(self.f32))


def run_case(dev, name, f32, noise=None):
    g = WaveGame(dev, build_case(name, f32), noise)
    assert g.shape_check() == 0
    assert g.launch(N_STEPS) == 0
    return g.read()


@pytest.mark.parametrize("f32", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("name", list(CASES))
def test_tag_wave_matches_oracle(name, f32):
    y64, e32, info = oracle(name, f32)
    check(f"wave {dtype_id(f32)} {name}", run_case(dev, name, f32), y64, e32)


@pytest.mark.parametrize("f32", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("name", ["base", "mixed"])
def test_tag_wave_noise_on(name, f32):
    """Games 0..7 noisy: the oracle with the same Philox noise; the last game the
    noise-off oracle; and the noisy games measurably left it."""
    y64, e32, info = oracle(name, f32, noisy=True)
    got = run_case(dev, name, f32, NOISE)
    tag = f"wave {dtype_id(f32)} {name}"
    check(tag + " noise_on", got, y64, e32)
    y_off, e_off, _ = oracle(name, f32)
    check(tag + " noise_on_last_game_vs_noise_off", got, y_off, e_off,
          games=slice(NOISE["noiseless_from"], None))
    assert np.abs(got["p"][:8] - y_off["p"][:8]).max() > 1e-3


def test_tag_wave_split_and_repeat_bitwise():
    """With noise on, so that the salt matters: 5 + 7 steps (salt_base 0, then
    5) equal one 12-step launch bit for bit, and so does a repeat launch."""
    one = run_case(dev, "asymmetric", False, NOISE)
    again = run_case(dev, "asymmetric", False, NOISE)
    g = WaveGame(dev, build_case("asymmetric", False), NOISE)
    assert g.launch(5, salt_base=0) == 0
    mid = g.read()
    assert g.launch(7, salt_base=5) == 0
    two = g.read()
    assert not np.array_equal(mid["steps"], two["steps"])
    for k in TAG_KEYS:
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), k
        assert np.array_equal(one[k].view(np.uint8), again[k].view(np.uint8)), k


@pytest.mark.parametrize("f32", DTYPES, ids=dtype_id)
def test_tag_wave_codes_and_noops(f32):
    """-116 for a pair the kernel does not cover, behind es_tag_episode's codes, from
    the launch and es_tag_wave_check alike; nothing written; no-ops return 0."""
    g = WaveGame(dev, build_case("base", f32))
    before = g.read()

    def unchanged():
        now = g.read()
        return all(np.array_equal(before[k].view(np.uint8), now[k].view(np.uint8))
                   for k in TAG_KEYS)

    assert g.launch(0) == 0 and unchanged()
    assert g.launch(4, n_games=0) == 0 and unchanged()
    assert g.launch(4, n_agents=3) == -112 and unchanged()
    assert g.launch(4, ob_dim=9) == -110 and unchanged()
    good = [n["dims"] for n in g.nets], [n["stride"] for n in g.nets]
    deep = [8, 64, 64, 64, 64, 2]     # 13 186 elements: two fp32 rows exceed 64 KB
    for d0, d1, want in (([8, 16, 2], [8, 65, 2], -116),
                         (deep, deep, -116 if f32 else 0),
                         ([8, 16, 2], [9, 8, 2], -110),
                         ([8, 65, 1], [8, 16, 2], -111)):    # -111 before -116
        for net, d in zip(g.nets, (d0, d1)):
            net["dims"], net["stride"] = np.array(d, dtype=np.int32), 1 << 20
        assert g.shape_check() == want, (d0, d1)
        if want != 0:           # (the covered deep pair would read rows the blobs lack)
            assert g.launch(4) == want and unchanged(), (d0, d1)
    for net, d, s in zip(g.nets, *good):
        net["dims"], net["stride"] = d, s
    g.nets[1]["stride"] = 8                        # row_stride < n
    assert g.launch(4) == -102 and g.shape_check() == -102 and unchanged()
