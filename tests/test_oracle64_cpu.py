"""CPU checks of the float64 oracle itself (tests/oracle64.py).

The GPU tests trust the oracle, so it is tied here to independent ground:
torch's own bf16 / e4m3fn casts, a float64 torch.nn stack built through the
engine's forward_perm, the CPU SyntheticLocomotion env, and a literal
transcription of GpuEngine._step_body's bookkeeping lines.
"""
import numpy as np
import pytest
import torch

from tests import oracle64 as o64
from tests.oracle64 import (ERR_FACTOR, bf16_bits_to_f64, e4m3_byte_to_f64, err_scale,
                            f32_to_bf16_bits, f32_to_e4m3_byte, fp8_byte_position,
                            layer_is_octet_tiled, layer_offsets, loco_step, mlp_forward,
                            n_params, policy_actions)


# --------------------------------------------------------------------- codecs
def _torch_bf16_bits(x):
    return torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)


def _torch_e4m3_bytes(x):
    return torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def _finite_e4m3_values():
    b = np.arange(256, dtype=np.uint8)
    v = e4m3_byte_to_f64(b)
    return b[~np.isnan(v)], v[~np.isnan(v)]


def test_bf16_codec_matches_torch():
    rng = np.random.RandomState(0)
    x = np.concatenate([
        rng.randn(200_000).astype(np.float32),
        (rng.randn(50_000) * 1e-30).astype(np.float32),
        (rng.randn(50_000) * 1e30).astype(np.float32),
        np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -126, 2.0 ** -140], np.float32)])
    # every tie: a bf16 value plus exactly half a bf16 ulp
    hi = rng.randint(0, 0x7F00, size=50_000).astype(np.uint32)
    ties = ((hi << 16) | 0x8000).view(np.float32)
    x = np.concatenate([x, ties, -ties])
    bits = f32_to_bf16_bits(x)
    assert np.array_equal(bits, _torch_bf16_bits(x))
    # decode is exact and encode(decode) is the identity on finite patterns
    all_bits = np.arange(0x7F80, dtype=np.uint16)
    vals = bf16_bits_to_f64(all_bits)
    want = torch.from_numpy(all_bits.view(np.int16)).view(torch.bfloat16).double().numpy()
    assert np.array_equal(vals, want)
    assert np.array_equal(f32_to_bf16_bits(vals.astype(np.float32)), all_bits)


def test_e4m3_decode_matches_torch():
    b = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(b).view(torch.float8_e4m3fn).double().numpy()
    got = e4m3_byte_to_f64(b)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    assert np.nanmax(got) == 448.0 and got[1] == 2.0 ** -9


def test_e4m3_encode_matches_torch_everywhere():
    bytes_, vals = _finite_e4m3_values()
    # every representable value encodes to itself (value compare: +-0)
    enc = f32_to_e4m3_byte(vals.astype(np.float32))
    assert np.array_equal(e4m3_byte_to_f64(enc), vals)
    assert np.array_equal(enc, _torch_e4m3_bytes(vals.astype(np.float32)))
    # every midpoint between neighbours, and one float32 ulp either side
    pos = np.sort(vals[vals >= 0])
    mid = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (pos[:-1] + pos[1:]) / 2)
    pts = np.concatenate([mid, np.nextafter(mid, np.float32(0)),
                          np.nextafter(mid, np.float32(1e9))])
    pts = np.concatenate([pts, -pts])
    assert np.array_equal(f32_to_e4m3_byte(pts), _torch_e4m3_bytes(pts))
    # RNE spot values
    rt = lambda v: float(e4m3_byte_to_f64(f32_to_e4m3_byte(np.float32(v))))
    assert rt(2.0 ** -10) == 0.0 and rt(3 * 2.0 ** -10) == 2.0 ** -8
    # random floats over the whole finite range and the sigma*eps range
    rng = np.random.RandomState(1)
    x = np.concatenate([rng.randn(300_000) * 0.02, rng.randn(300_000),
                        rng.uniform(-448, 448, 100_000),
                        rng.randn(100_000) * 1e-3]).astype(np.float32)
    assert np.array_equal(f32_to_e4m3_byte(x), _torch_e4m3_bytes(x))


# --------------------------------------------------------------------- layout
def _all_fp8_dims():
    from tests.test_kernel_oracle_loco import FP8_LOCO_DIMS
    from tests.test_kernel_oracle_noise import FP8_NOISE_DIMS
    from tests.test_kernel_oracle_ops import FP8_PHENO_DIMS
    return {**{"loco_" + k: v for k, v in FP8_LOCO_DIMS.items()},
            **{"noise_" + k: v for k, v in FP8_NOISE_DIMS.items()},
            **{"pheno_" + k: v for k, v in FP8_PHENO_DIMS.items()}}


def test_fp8_byte_position_is_a_permutation_and_layouts_are_accepted():
    from es_pytorch_amd.core.engine import GpuEngine
    cases = _all_fp8_dims()
    assert len(cases) >= 8
    for key, dims in cases.items():
        n = n_params(dims)
        pos = fp8_byte_position(dims)
        assert np.array_equal(np.sort(pos), np.arange(n)), key
        assert GpuEngine._fp8_layout_ok(dims), key
        # pheno.hip's documented address for an even-input octet-tiled layer
        for woff, boff, I, O in layer_offsets(dims)[0]:
            if not layer_is_octet_tiled(woff, O):
                assert np.array_equal(pos[woff:boff], np.arange(woff, boff)), key
                continue
            ro = I % 2
            for i in range(ro, I):
                for o_ in range(O):
                    r = i - ro
                    want = woff + ro * O + (r & ~1) * O + (o_ >> 3) * 16 + (r & 1) * 8 + \
                        (o_ & 7)
                    assert pos[woff + i * O + o_] == want, (key, i, o_)
            assert np.array_equal(pos[boff:boff + O], np.arange(boff, boff + O))
    # the misaligned (7,16) layer really is in plain order
    woff, boff, _, _ = layer_offsets(cases["pheno_misaligned_layer_plain"])[0][1]
    pos = fp8_byte_position(cases["pheno_misaligned_layer_plain"])
    assert woff == 28 and np.array_equal(pos[woff:boff], np.arange(woff, boff))


# -------------------------------------------------------------------- forward
@pytest.mark.parametrize("dims,act_final", [([11, 64, 64, 3], 1), ([7, 16, 5], 0),
                                            ([29, 8], 1), ([9, 40, 24, 17], 1)])
def test_mlp_forward_matches_float64_torch_stack(dims, act_final):
    from es_pytorch_amd.core.engine import forward_perm
    torch.manual_seed(sum(dims))
    layers = []
    for li, (I, O) in enumerate(zip(dims[:-1], dims[1:])):
        layers.append(torch.nn.Linear(I, O))
        if li < len(dims) - 2 or act_final:
            layers.append(torch.nn.Tanh())
    net = torch.nn.Sequential(*layers).double()
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])  # W(O,I), b
    fwd = flat[forward_perm(dims)].numpy()          # the engine's forward layout
    x = torch.randn(5, dims[0], dtype=torch.float64)
    want = net(x).detach().numpy()
    got = mlp_forward(dims, fwd, x.numpy(), act_final)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
    # float32 evaluation stays within float32 distance of it
    got32 = mlp_forward(dims, fwd, x.numpy(), act_final, dtype=np.float32)
    assert got32.dtype == np.float32
    assert np.abs(got32 - want).max() < 1e-5


def test_policy_actions_normalisation_rows_and_decodes():
    rng = np.random.RandomState(3)
    dims = [6, 8, 6]
    n = n_params(dims)
    rows = rng.randn(5, n) * 0.4
    obs = rng.randn(4, 6) * 3
    mean, std = rng.randn(6), rng.rand(6) + 0.1
    kw = dict(dims=dims, weight_rows=rows, obs=obs, obmean=mean, obstd=std, ob_clip=2.0)
    xn = np.clip((obs - mean) / std, -2.0, 2.0)
    assert (np.abs((obs - mean) / std) > 2.0).any()
    # slots 6..9 with eps=2 and wrow0=1 read rows 2,2,3,3
    act, net = policy_actions(members=np.arange(6, 10), eps=2, wrow0=1, **kw)
    for k, r in enumerate([2, 2, 3, 3]):
        np.testing.assert_allclose(net[k], mlp_forward(dims, rows[r], xn[k]), atol=1e-15)
    assert np.array_equal(act, net)
    a2, net2 = policy_actions(act_mode=2, **kw)
    assert np.array_equal(a2, net2[:, 1:])
    a3, net3 = policy_actions(act_mode=3, **kw)
    assert np.array_equal(a3, net3[:, :3])
    alow, arange = np.array([-2.0, 1.0]), np.array([4.0, 0.5])
    ab, netb = policy_actions(bins=3, alow=alow, arange=arange, **kw)
    best = netb.reshape(4, 2, 3).argmax(2)
    np.testing.assert_allclose(ab, alow + arange * best / 2.0, atol=1e-15)
    al, _ = policy_actions(bins=3, loco=True, **kw)
    assert np.array_equal(al, -1.0 + best)


# ------------------------------------------------------------------- env step
def _env_dict(env, fall_thr):
    return dict(A=env.A.double().numpy(), B=env.B.numpy(), b0=env.b0.numpy(),
                wv=env.wv.numpy(), wa=env.wa.numpy(), wy=env.wy.numpy(),
                wh=env.wh.numpy(), leak=env.leak, ctrl=env.ctrl_cost,
                alive_bonus=env.alive_bonus, fall_thr=fall_thr, dt=env.dt,
                terminate=int(env.terminate_on_fall), goal=int(env.goal_conditioned))


@pytest.mark.parametrize("terminate", [True, False])
@pytest.mark.parametrize("name", ["Hopper", "Walker2d", "AntFlagrun", "Humanoid"])
def test_loco_step_matches_cpu_env_and_step_body(name, terminate):
    """Oracle step == SyntheticLocomotion(device='cpu').step for the state,
    positions, reward and termination, and == the bookkeeping lines of
    GpuEngine._step_body (transcribed below) for the accumulators."""
    from es_pytorch_amd.envs.locomotion import SyntheticLocomotion
    Bn = 12
    goal = name.endswith("Flagrun")
    env = SyntheticLocomotion(name, Bn, device="cpu", max_steps=1000,
                              terminate_on_fall=terminate, goal_conditioned=goal,
                              matrix_seed=4321)
    rng = np.random.RandomState(200 + len(name) + int(terminate))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    S, D, A = env.sdim, env.ob_dim, env.ac_dim
    env.reset(seed=5)
    env.s.copy_(torch.from_numpy(f32(rng.randn(Bn, S) * 0.6)))
    env.pos.copy_(torch.from_numpy(f32(rng.randn(Bn, 3))))
    alive = f32(np.arange(Bn) % 3 != 1)
    state = dict(s=env.s.numpy().copy(), pos=env.pos.numpy().copy(),
                 goal=env.goal.numpy().copy() if goal else None, alive=alive,
                 rew_total=f32(rng.randn(Bn) * 3), member_steps=f32(rng.randint(0, 9, Bn)),
                 behv=f32(rng.randn(Bn, 3)), mo_sum=f32(rng.randn(Bn, D)),
                 mo_sumsq=f32(rng.rand(Bn, D)))
    # zero weights + bf16 biases, no final tanh: the actions ARE the biases
    # (exact in float32, some beyond the +-1 action clamp), so the env and
    # the oracle are fed identical actions
    dims = [D, A]
    rows = np.zeros((Bn, n_params(dims)))
    rows[:, D * A:] = bf16_bits_to_f64(f32_to_bf16_bits(f32(rng.randn(Bn, A) * 0.8)))
    policy = dict(dims=dims, weight_rows=rows, obmean=f32(rng.randn(D) * 0.1),
                  obstd=f32(rng.rand(D) + 0.5), ob_clip=5.0, act_final=0)
    envd = _env_dict(env, env.fall_threshold)
    _, info = loco_step(state, envd, policy)
    if terminate:
        # put the threshold inside the widest gap of h so both outcomes occur
        hs = np.sort(info["h"])
        j = int(np.argmax(np.diff(hs)))
        env.fall_threshold = float(np.float32(0.5 * (hs[j] + hs[j + 1])))
        envd = _env_dict(env, env.fall_threshold)
    y64, info = loco_step(state, envd, policy)
    y32, _ = loco_step(state, envd, policy, dtype=np.float32)
    assert (np.abs(info["h"] - envd["fall_thr"]) > 1e-3).all()
    assert (np.abs(info["net_out"]) > 1.0).any()
    acts = torch.from_numpy(info["net_out"].astype(np.float32))   # unclamped
    assert np.array_equal(acts.numpy().astype(np.float64), info["net_out"])

    # ---- the env itself
    ob, rew, done = env.step(acts)
    if terminate:
        assert done.any() and (~done).any()
    else:
        assert not done.any()
    tol = lambda k: ERR_FACTOR * err_scale(y32[k], y64[k])
    assert np.abs(env.s.numpy() - y64["s"]).max() <= tol("s")
    assert np.abs(env.pos.numpy() - y64["pos"]).max() <= tol("pos")
    assert np.array_equal(done.numpy(), info["done"])

    # ---- GpuEngine._step_body bookkeeping, transcribed (float64 torch)
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64).copy())
    alive_t, rew_total, member_steps, behv = (t64(state[k]) for k in
                                              ("alive", "rew_total", "member_steps",
                                               "behv"))
    rew_d, ob_d, positions = rew.double(), ob.double(), env.positions.double()
    rew_total.add_(rew_d * alive_t)
    member_steps.add_(alive_t)
    am = alive_t.bool().unsqueeze(1)
    behv.copy_(torch.where(am, positions, behv))
    w = alive_t
    ob_sum = (ob_d * w.unsqueeze(1)).sum(0)
    ob_sumsq = (ob_d * ob_d * w.unsqueeze(1)).sum(0)
    alive_t.mul_(1.0 - done.double())
    assert np.abs(rew_total.numpy() - y64["rew_total"]).max() <= tol("rew_total")
    assert np.array_equal(member_steps.numpy(), y64["member_steps"])
    assert np.abs(behv.numpy() - y64["behv"]).max() <= tol("behv")
    assert np.array_equal(alive_t.numpy(), y64["alive"])
    d_sum = (y64["mo_sum"] - state["mo_sum"].astype(np.float64)).sum(0)
    d_sq = (y64["mo_sumsq"] - state["mo_sumsq"].astype(np.float64)).sum(0)
    assert np.abs(ob_sum.numpy() - d_sum).max() <= Bn * tol("mo_sum")
    assert np.abs(ob_sumsq.numpy() - d_sq).max() <= Bn * tol("mo_sumsq")
    # dead members: nothing they own moves
    dead = alive == 0
    for k in ("rew_total", "member_steps", "behv", "mo_sum", "mo_sumsq", "alive"):
        assert np.array_equal(y64[k][dead], state[k][dead].astype(np.float64)), k


def test_loco_step_members_subset_leaves_other_slots_alone():
    from tests.test_kernel_oracle_loco import build
    case = build("episode256_S64_1step")
    env = {k: v for k, v in case["env"].items() if k != "A_bits"}
    y, _ = loco_step(case["state"], env, case["policy"], case["members"])
    rest = np.setdiff1d(np.arange(case["nslots"]), case["members"])
    assert rest.size
    for k in o64.STATE_KEYS:
        assert np.array_equal(y[k][rest], case["state"][k][rest].astype(np.float64)), k
        assert not np.array_equal(y["s"][case["members"]],
                                  case["state"]["s"][case["members"]])


def test_gpu_loco_cases_meet_their_input_conditions():
    """Every GPU case: no h within 1e-3 of the fall threshold, no binned
    logit tie, both outcomes present, dead members present (the oracle side
    of tests/test_kernel_oracle_loco.py, which needs no GPU)."""
    from tests.test_kernel_oracle_loco import CASES, build, oracle
    for name in CASES:
        case = build(name)
        y64, e32 = oracle(case)
        m = case["members"]
        assert (case["state"]["alive"][m] == 0).any(), name
        assert all(np.isfinite(v) and v > 0 for v in e32.values()), name


def test_error_scale_floor():
    y = np.array([4.0, -8.0])
    assert err_scale(y.astype(np.float32), y) == 8.0 * 2.0 ** -24
    assert err_scale(y + np.array([0.0, 1e-3]), y) == pytest.approx(1e-3)
