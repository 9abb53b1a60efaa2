"""CPU checks of the oracle's random numbers (tests/oracle64.py) and of the
cases of tests/test_kernel_oracle_noise.py. No GPU.

* The oracle's Philox reproduces the published Random123 known-answer
  vectors of philox4x32-10, so it is tied to the paper and not to
  csrc/philox.h.
* es_noise_fill_cpu, the CPU twin of the table fill, is held to the oracle
  under the project's bound, ``|twin - oracle64| <= 16 * E32``. Measured
  ratios: 1.00 - 1.01 over the whole grid.
* Every GPU noise case meets its input conditions.
* Teeth: for every case that draws, each plausible wrong draw moves the
  oracle's result by more than 100 * 16 * E32 of that case, so a kernel with
  that fault would miss the GPU bound by two orders of magnitude.
"""
import numpy as np
import pytest

from tests import oracle64 as o64
from tests import test_kernel_oracle_noise as tn
from tests.oracle64 import ERR_FACTOR, noise_table, philox4x32_10, policy_actions

TEETH = 100 * ERR_FACTOR


# ---------------------------------------------------------------- known answers
KNOWN_ANSWERS = [   # counter x4, key x2 -> output x4 (Random123 kat_vectors)
    ((0x00000000,) * 4, (0x00000000,) * 2,
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2,
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        assert tuple(int(w) for w in philox4x32_10(ctr, key)) == want
    # vectorised: the three vectors at once, one counter/key word per array
    ctr = [np.array([k[0][i] for k in KNOWN_ANSWERS]) for i in range(4)]
    key = [np.array([k[1][i] for k in KNOWN_ANSWERS]) for i in range(2)]
    got = np.stack(philox4x32_10(ctr, key), axis=1)
    assert np.array_equal(got, np.array([k[2] for k in KNOWN_ANSWERS], dtype=np.uint64))


def test_normal4_word_order_and_uniform_edges():
    """Group, seed and stream land in the documented counter/key words, and
    the uniforms round as float32: the top 128 words give u = 1.0."""
    g, seed, stream = 0x0000000500000007, 0x1111111122222222, 0xAC
    w = philox4x32_10((7, 5, stream, o64.NOISE_TAG), (0x22222222, 0x11111111))
    u = [np.float32(int(x)) for x in w]
    s = np.float32(2.0 ** -32)
    u1, u2, u3, u4 = (u[0] + np.float32(1)) * s, u[1] * s, (u[2] + np.float32(1)) * s, u[3] * s
    tp = np.float64(np.float32(6.2831853071795864769))
    r1, r2 = np.sqrt(-2 * np.log(np.float64(u1))), np.sqrt(-2 * np.log(np.float64(u3)))
    want = [r1 * np.cos(tp * u2), r1 * np.sin(tp * u2), r2 * np.cos(tp * u4),
            r2 * np.sin(tp * u4)]
    assert np.array_equal(o64.normal4(g, seed, stream), np.array(want))
    assert np.float32(0xFFFFFFFF) * s == np.float32(1.0)
    assert np.float32(0xFFFFFF80) * s == np.float32(1.0)
    assert np.float32(0xFFFFFF7F) * s < np.float32(1.0)
    t32 = noise_table(9, seed, stream, np.float32)
    assert t32.dtype == np.float32
    t64 = noise_table(9, seed, stream)
    assert np.array_equal(t64[4:8], o64.normal4(1, seed, stream))
    assert o64.action_noise(seed, 1) == o64.normal4(1, seed, o64.ACTION_STREAM)[0]


# --------------------------------------------------------------------- CPU fill
def _cpu_fill(n, seed, stream):
    from es_pytorch_amd import ops
    buf = tn.table_buffer(n)
    ops.cpu().es_noise_fill_cpu(buf.ctypes.data, n, seed, stream)
    return buf


@pytest.mark.parametrize("seed", tn.TABLE_SEEDS)
@pytest.mark.parametrize("n", tn.TABLE_NS)
def test_cpu_noise_fill_matches_oracle(n, seed):
    """n = 2^20 + 5 runs on two threads with a group-aligned chunk boundary;
    the padding behind n keeps its NaN payload."""
    for stream in tn.TABLE_STREAMS:
        tn.check_table("cpu_fill", _cpu_fill(n, seed, stream), n, seed, stream)


def test_noise_table_depends_on_every_key_and_stream_bit_field():
    n = 1027
    base = _cpu_fill(n, 99, 1)[:n]
    for seed, stream in ((99 + (1 << 32), 1), (99 + (1 << 63), 1), (99, 1 + (1 << 31)),
                         (99, 0)):
        other = _cpu_fill(n, seed, stream)[:n]
        assert not np.array_equal(base, other), (seed, stream)
        # and the oracle follows the twin there
        tn.check_table("cpu_fill_field", _cpu_fill(n, seed, stream), n, seed, stream)
    assert not np.array_equal(noise_table(n, 99, 1), noise_table(n, 99 + (1 << 32), 1))
    assert not np.array_equal(noise_table(n, 99, 1), noise_table(n, 99, 0xAC))


# ------------------------------------------------------------- input conditions
def test_noise_off_is_bit_identical():
    """noise=None, a noise dict that gates every slot off, and ac_std = 0 all
    give the bits of the noise-free evaluation."""
    case = tn.build_loco("step_S8")
    kw = tn.loco_rollout_kwargs(case)
    ref, _ = o64.loco_rollout(kw["state"], kw["env"], kw["policy"], 1, kw["members"])
    for noise in (dict(kw["noise"], noiseless_from=0), dict(kw["noise"], ac_std=0.0)):
        got, _ = o64.loco_rollout(**dict(kw, noise=noise))
        for k in o64.STATE_KEYS:
            assert np.array_equal(got[k], ref[k]), k
    got, _ = o64.loco_rollout(**kw)
    assert not np.array_equal(got["s"], ref["s"])


@pytest.mark.parametrize("name", list(tn.FWD_CASES))
def test_gpu_noise_fwd_cases_meet_their_input_conditions(name):
    y64, e32, _ = tn.fwd_reference(name)
    assert np.isfinite(y64).all() and np.isfinite(e32) and e32 > 0


@pytest.mark.parametrize("name", tn.ALL_LOCO)
def test_gpu_noise_loco_cases_meet_their_input_conditions(name):
    """The conditions of the noise-free modules (h off the fall threshold,
    both outcomes, dead members, no logit tie) and the noise ones (asserted
    inside loco_reference)."""
    case, y64, e32 = tn.loco_reference(name)
    assert all(np.isfinite(v) and v > 0 for v in e32.values()), name


def test_noise_cases_cover_the_issue_list():
    kernels = {c["kernel"] for c in tn.LOCO_CASES.values()}
    assert kernels == {"step", "split", "pair", "fp8", "pair_episode", "episode"}
    assert {c["block"] for c in tn.LOCO_CASES.values() if c["kernel"] == "episode"} == \
        {256, 512}
    assert any(c["seed_dev"] is None for c in tn.LOCO_CASES.values())
    assert {c["kernel"] for c in tn.F32_LOCO_CASES.values()} == {"step", "episode"}
    for c in list(tn.LOCO_CASES.values()) + list(tn.F32_LOCO_CASES.values()):
        if c["kernel"] in ("episode", "pair_episode"):
            assert c["salt_base"] > 0 and c["n_steps"] == 3


# ------------------------------------------------------------------------ teeth
def _wrong_draws(kind, nslots):
    real = o64.action_draws

    def b_plus_1(seed, members, width, cols, dtype=np.float64):
        return real(seed, np.asarray(members) + 1, width, cols, dtype)

    def component_1(seed, members, width, cols, dtype=np.float64):
        ctr = np.asarray(members, dtype=np.uint64)[:, None] * np.uint64(width) + \
            np.arange(cols, dtype=np.uint64)[None, :]
        return o64.normal4(ctr, seed, o64.ACTION_STREAM, dtype)[..., 1]

    def minus_gets_plus(seed, members, width, cols, dtype=np.float64):
        return real(seed, tn.minus_to_plus(members, nslots), width, cols, dtype)

    return dict(b_plus_1=b_plus_1, component_1=component_1,
                minus_gets_plus=minus_gets_plus)[kind]


WRONG = ["noise_off", "salt_off_by_one", "b_plus_1", "component_1", "minus_gets_plus"]


@pytest.mark.parametrize("wrong", WRONG)
@pytest.mark.parametrize("name", [k for k, c in tn.FWD_CASES.items() if tn.fwd_draws(c)])
def test_fwd_noise_cases_have_teeth(monkeypatch, name, wrong):
    case = tn.build_fwd(name)
    y64, e32, _ = tn.fwd_reference(name)
    noise = tn.fwd_noise(case["c"])
    if wrong == "noise_off":
        noise = None
    elif wrong == "salt_off_by_one":
        noise = dict(noise, salt=noise["salt"] + 1)
    else:
        monkeypatch.setattr(o64, "action_draws", _wrong_draws(wrong, tn.FWD_B))
    bad, _ = policy_actions(noise=noise, **case["kw"])
    moved = float(np.abs(bad - y64).max())
    assert moved > TEETH * e32, (name, wrong, moved, e32)


@pytest.mark.parametrize("wrong", WRONG)
@pytest.mark.parametrize("name", [k for k in tn.ALL_LOCO if tn.loco_draws(
    {**tn.LOCO_CASES, **tn.F32_LOCO_CASES}[k])])
def test_loco_noise_cases_have_teeth(monkeypatch, name, wrong):
    case, y64, e32 = tn.loco_reference(name)
    kw = tn.loco_rollout_kwargs(case)
    if wrong == "noise_off":
        kw["noise"] = None
    elif wrong == "salt_off_by_one":
        kw["salt_base"] += 1
    else:
        monkeypatch.setattr(o64, "action_draws", _wrong_draws(wrong, case["nslots"]))
    bad, _ = o64.loco_rollout(**kw)
    m = case["members"]
    moved = float(np.abs(bad["s"][m] - y64["s"][m]).max())
    assert moved > TEETH * e32["s"], (name, wrong, moved, e32["s"])
