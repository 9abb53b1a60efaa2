"""The fp32-weights kernels (weights_dtype = "fp32") on test-owned buffers,
against the float64 oracle (tests/oracle64.py).

es_pheno_f32 is compared bit for bit: the kernel's contract is ONE rounding,
``float32(theta + float32(sign*std) * noise)``. es_mlp_fwd_f32,
es_loco_step_f32 and es_loco_episode_f32 assert the project's bound
``|kernel - oracle64| <= 16 * E32`` with the fp32 weight VALUES taken exactly
(E32: the same computation in numpy float32).

Forward tiling (mlp_layers_f32): G = 4 outputs per thread (quads), pipeline
depth d = 4, 256 threads, so for a quad-tiled layer (I, O): TILES = O/4,
PART = 256 // TILES; prologue needs I > 3*PART, the steady loop I > 7*PART.

  case                          layer      TILES PART  boundary
  vec_11x4_tiles1               (11,4)         1  256  TILES = 1, I < PART
  vec_40x64_tail_only           (40,64)       16   16  I <= 3*PART: tail loop only
  vec_100x64_prologue_drain     (100,64)      16   16  3*PART < I <= 7*PART
  vec_260x64_steady_ragged      (260,64)      16   16  steady loop, 260 = 16*16+4
  vec_400x24_tiles6             (400,24)       6   42  6*42 = 252: 4 idle threads
  vec_376x256_flagship          (376,256)     64    4  + (256,256), scalar head 17
  vec_9x1024_part1              (9,1024)     256    1  PART = 1
  vec_9x2048_wide               (9,2048)     512    1  TILES > 256: two tile sweeps
  scalar_10x130                 (10,130)       -    1  O % 4 != 0, thread per output
  scalar_5x300_two_sweeps       (5,300)        -    0  O > 256
  scalar_3x16_misaligned_woff   (3,16)         -   16  woff = 18: scalar walk
  scalar_row_stride_odd         (11,8)         -   32  row_stride % 4 != 0
  eight_layers                  8 layers
  (64,3) scalar heads ride on the vec nets; eps = 2, row_stride > n and
  act_final = 0 are spread over the cases (see CASES).

Measured on MI355X, max |err| / E32 per case (bound: 16):

  case                                ratio  E32
  vec_11x4_tiles1                      0.80  2.83e-07
  vec_40x64_tail_only                  0.66  2.35e-07
  vec_100x64_prologue_drain            0.66  2.88e-07
  vec_260x64_steady_ragged             0.93  1.79e-07
  vec_400x24_tiles6                    0.60  2.51e-07
  vec_376x256_flagship                 0.71  3.19e-07
  vec_9x1024_part1                     0.53  2.63e-07
  vec_9x2048_wide                      0.44  3.83e-07
  scalar_10x130                        0.50  2.64e-07
  scalar_5x300_two_sweeps              0.69  6.01e-07
  scalar_3x16_misaligned_woff          0.96  1.75e-07
  scalar_row_stride_odd                0.65  2.39e-07
  eight_layers                         2.29  2.44e-08
  binned_decode                        0.55  1.08e-07
  mode2_integ_gauss                    1.00  1.04e-07
  mode3_integ_gauss_multi              0.75  1.43e-07
  noiseless_from_tail                  0.56  1.41e-07
  noiseless_from_tail_mode2            0.54  9.54e-08

  case                                ratio  worst buffer
  step_S8                              1.43  mo_sumsq
  step_S64_eps2                        1.09  pos
  step_S152                            0.76  mo_sum
  step_S376                            0.64  mo_sum
  step_S11_scalar                      0.80  rew_total
  step_S27_goal                        1.00  mo_sumsq
  step_S64_binned                      0.80  s
  step_S11_mode2                       0.90  s
  step_S152_mode3_noterm               0.94  mo_sumsq
  episode256_S152_3steps               1.43  mo_sumsq
  episode512_376x256                   0.79  mo_sum
  episode512_S11_binned                1.31  behv

es_pheno_f32: bit-exact on every case.
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import (ERR_FACTOR, STATE_KEYS, bf16_bits_to_f64, err_scale,
                            f32_to_bf16_bits, fp32_error_scale, loco_rollout, max_ratio,
                            n_params, policy_actions, top2_logit_gap)

gpu = pytest.mark.gpu

OB_CLIP = 5.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ----------------------------------------------------------------------- pheno
PHENO_SHAPES = [(1000, 0), (1001, 7), (1007, 9), (1000, 8), (2_097_152 + 13, 11)]
PHENO_STD = np.float32(0.02)


def pheno_inputs(n, pad):
    """Seeded inputs of a pheno case (numpy only, shared by the GPU test and
    the CPU double-rounding check)."""
    big = n > 2_000_000
    rng = np.random.RandomState(n % 1000 + pad + 5)
    if big:
        tab = rng.randn(n + 16).astype(np.float32)
        offs = np.array([3, 6], dtype=np.int64)
        signs = np.array([1.0, -1.0], dtype=np.float32)
    else:
        tab = rng.randn(1_000_000).astype(np.float32)
        offs = np.array([0, 1, 2, 3, 4001, 70_002, 900_007], dtype=np.int64)
        signs = np.array([1, -1, 1, -1, 0, 1, -1], dtype=np.float32)
    assert set(offs % 4) == ({3, 2} if big else {0, 1, 2, 3})
    theta = rng.randn(n).astype(np.float32)
    return tab, offs, signs, theta


def pheno_oracle(theta, tab, off, sign, std, n, wide=np.float64):
    s32 = np.float32(sign) * np.float32(std)          # the kernel's own scalar
    return (theta.astype(wide) + wide(s32) * tab[off:off + n].astype(wide)).astype(
        np.float32)


@pytest.mark.parametrize("n,pad", PHENO_SHAPES)
def test_pheno_f32_oracle_has_no_double_rounding_edge(n, pad):
    """float64 and longdouble evaluation round to the same float32 at every
    element of these inputs, so the float64 oracle IS the singly-rounded
    fmaf result the kernel must produce."""
    if np.finfo(np.longdouble).nmant <= np.finfo(np.float64).nmant:
        pytest.skip("no extended-precision longdouble on this platform")
    tab, offs, signs, theta = pheno_inputs(n, pad)
    for o, sg in zip(offs, signs):
        a = pheno_oracle(theta, tab, o, sg, PHENO_STD, n, np.float64)
        b = pheno_oracle(theta, tab, o, sg, PHENO_STD, n, np.longdouble)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@gpu
@pytest.mark.parametrize("n,pad", PHENO_SHAPES)
def test_pheno_f32_bit_exact(dev, n, pad):
    """n % 8 in {0, 1, 7}, row_stride = n + pad with the padding untouched,
    offsets of every residue mod 4, n > 1024*1024 (two rows) where the
    grid-stride loop iterates, signs +1 / -1 / 0."""
    from es_pytorch_amd import ops
    tab, offs, signs, theta = pheno_inputs(n, pad)
    stride = n + pad
    assert stride % 4 == 0 and stride >= n
    P = len(offs)
    fill = np.float32(-7.25)
    out = torch.full((P, stride), float(fill), dtype=torch.float32, device=dev)
    tab_d, th_d, offs_d, signs_d = (_t(a, dev) for a in (tab, theta, offs, signs))
    rc = ops.hip().es_pheno_f32(out.data_ptr(), th_d.data_ptr(), tab_d.data_ptr(),
                                offs_d.data_ptr(), signs_d.data_ptr(), P, n, stride,
                                float(PHENO_STD), _stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    for p, (o, sg) in enumerate(zip(offs, signs)):
        want = pheno_oracle(theta, tab, o, sg, PHENO_STD, n)
        bad = np.flatnonzero(got[p, :n].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (p, bad[:5], got[p, bad[:5]], want[bad[:5]])
        assert (got[p, n:] == fill).all(), f"row {p}: padding overwritten"
        if sg == 0:
            assert np.array_equal(got[p, :n].view(np.uint32), theta.view(np.uint32))
        else:
            assert not np.array_equal(got[p, :n], theta)


@gpu
def test_pheno_f32_rejects_unaligned_stride(dev):
    """Rows must stay 16-B aligned for the vector stores: nothing launches."""
    from es_pytorch_amd import ops
    out = torch.full((2, 16), 3.0, dtype=torch.float32, device=dev)
    z = torch.zeros(64, dtype=torch.float32, device=dev)
    o = torch.zeros(2, dtype=torch.int64, device=dev)
    for n, stride in ((9, 10), (9, 8)):
        rc = ops.hip().es_pheno_f32(out.data_ptr(), z.data_ptr(), z.data_ptr(),
                                    o.data_ptr(), z.data_ptr(), 1, n, stride, 0.02,
                                    _stream(dev))
        torch.cuda.synchronize(dev)
        assert rc == -102
    assert (out == 3.0).all()


# --------------------------------------------------------------------- forward
# name -> (dims, B, eps, act_final, act_mode, bins, stride_pad)
FWD_CASES = {
    "vec_11x4_tiles1": ([11, 4], 3, 1, 0, 0, 0, 0),
    "vec_40x64_tail_only": ([40, 64, 3], 4, 2, 1, 0, 0, 0),
    "vec_100x64_prologue_drain": ([100, 64, 3], 3, 1, 0, 0, 0, 8),
    "vec_260x64_steady_ragged": ([260, 64, 3], 3, 1, 1, 0, 0, 0),
    "vec_400x24_tiles6": ([400, 24, 5], 3, 1, 1, 0, 0, 4),
    "vec_376x256_flagship": ([376, 256, 256, 17], 6, 2, 1, 0, 0, 0),
    "vec_9x1024_part1": ([9, 1024, 5], 2, 1, 1, 0, 0, 0),
    "vec_9x2048_wide": ([9, 2048, 5], 2, 1, 1, 0, 0, 0),
    "scalar_10x130": ([10, 130, 4], 3, 1, 1, 0, 0, 0),
    "scalar_5x300_two_sweeps": ([5, 300, 2], 3, 1, 0, 0, 0, 0),
    "scalar_3x16_misaligned_woff": ([5, 3, 16, 4], 3, 1, 1, 0, 0, 0),
    "scalar_row_stride_odd": ([11, 8], 3, 1, 1, 0, 0, 1),
    "eight_layers": ([6, 16, 12, 16, 8, 24, 16, 8, 4], 3, 1, 1, 0, 0, 0),
    "binned_decode": ([11, 64, 15], 5, 1, 1, 0, 5, 0),
    "mode2_integ_gauss": ([11, 16, 4], 4, 2, 1, 2, 0, 0),
    "mode3_integ_gauss_multi": ([11, 16, 6], 4, 1, 1, 3, 0, 0),
}


def make_net_f32(rng, dims, rows, stride_pad=0):
    """float32 weight blob (rows, stride), NO guard row; per-layer scale
    0.7/sqrt(I) so pre-activations stay O(1). Padding is NaN: it is never a
    weight, and a read of it that reaches an output shows."""
    n = n_params(dims)
    stride = (n + 3) // 4 * 4 + stride_pad
    w = np.full((rows, stride), np.nan, dtype=np.float32)
    off = 0
    for I, O in zip(dims[:-1], dims[1:]):
        w[:, off:off + I * O] = rng.randn(rows, I * O) * (0.7 / np.sqrt(I))
        off += I * O
        w[:, off:off + O] = rng.randn(rows, O) * 0.1
        off += O
    return w, stride


def make_obs(rng, B, D):
    """obs = mean + std * z with some |z| beyond the clip and small stds."""
    obmean = (rng.randn(D) * 0.3).astype(np.float32)
    obstd = (rng.rand(D) + 0.5).astype(np.float32)
    obstd[::3] = 0.01
    z = rng.randn(B, D) * 1.5
    z[:, ::4] = 8.0 * np.sign(z[:, ::4])
    obs = (obmean + obstd * z).astype(np.float32)
    return obs, obmean, obstd


def launch_fwd(dev, dims, w, stride, obs, obmean, obstd, adim_out, eps=1, act_final=1,
               act_mode=0, bins=0, alow=None, arange=None, noiseless_from=0, ac_std=None,
               seed=None, salt=0):
    from es_pytorch_amd import ops
    B = obs.shape[0]
    w_d, obs_d, mean_d, std_d = (_t(a, dev) for a in (w, obs, obmean, obstd))
    out = torch.full((B, adim_out), float("nan"), dtype=torch.float32, device=dev)
    alow_d = _t(alow, dev) if alow is not None else None
    ar_d = _t(arange, dev) if arange is not None else None
    acs_d = _t(np.array([ac_std], np.float32), dev) if ac_std is not None else None
    seed_d = _t(np.array([seed], np.int64), dev) if seed is not None else None
    dims_arr = np.array(dims, dtype=np.int32)
    rc = ops.hip().es_mlp_fwd_f32(
        out.data_ptr(), obs_d.data_ptr(), w_d.data_ptr(), mean_d.data_ptr(),
        std_d.data_ptr(), dims_arr.ctypes.data, len(dims),
        seed_d.data_ptr() if seed_d is not None else None, salt, B, OB_CLIP,
        acs_d.data_ptr() if acs_d is not None else None, stride, act_final,
        noiseless_from, bins, eps, act_mode,
        alow_d.data_ptr() if alow_d is not None else None,
        ar_d.data_ptr() if ar_d is not None else None, _stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def check(kind, name, got, y64, e32):
    r = max_ratio(got, y64, e32)
    print(f"ORACLE-RATIO {kind} {name} ratio={r:.2f} E32={e32:.3g}")
    assert np.isfinite(got).all(), name
    assert r <= ERR_FACTOR, (name, r, e32)


def build_fwd_case(name):
    dims, B, eps, act_final, act_mode, bins, pad = FWD_CASES[name]
    rng = np.random.RandomState(sum(ord(ch) for ch in name))  # stable per case
    rows = (B + eps - 1) // eps
    w, stride = make_net_f32(rng, dims, rows, pad)
    obs, obmean, obstd = make_obs(rng, B, dims[0])
    A = dims[-1]
    adim = A - 1 if act_mode == 2 else A // 2 if act_mode == 3 else \
        A // bins if bins > 1 else A
    alow = arange = None
    if bins > 1:
        alow = (rng.randn(adim) - 2.0).astype(np.float32)
        arange = (rng.rand(adim) * 3.0 + 0.5).astype(np.float32)
    n = n_params(dims)
    kw = dict(dims=dims, weight_rows=w[:, :n].astype(np.float64), obs=obs, obmean=obmean,
              obstd=obstd, ob_clip=OB_CLIP, eps=eps, act_final=act_final,
              act_mode=act_mode, bins=bins, alow=alow, arange=arange)
    return dict(dims=dims, B=B, eps=eps, act_final=act_final, act_mode=act_mode,
                bins=bins, w=w, stride=stride, obs=obs, obmean=obmean, obstd=obstd,
                adim=adim, alow=alow, arange=arange, kw=kw)


@gpu
@pytest.mark.parametrize("name", list(FWD_CASES))
def test_mlp_fwd_f32_matches_oracle(dev, name):
    c = build_fwd_case(name)
    y64, e32 = fp32_error_scale(policy_actions, **c["kw"])
    if c["bins"] > 1:
        _, net = policy_actions(**c["kw"])
        assert top2_logit_gap(net, c["bins"]) > 1e-3, "binned logits on a rounding edge"
    xn = (c["obs"].astype(np.float64) - c["obmean"]) / c["obstd"]
    assert (np.abs(xn) > OB_CLIP).any() and (np.abs(xn) < OB_CLIP).any()
    got = launch_fwd(dev, c["dims"], c["w"], c["stride"], c["obs"], c["obmean"],
                     c["obstd"], c["adim"], eps=c["eps"], act_final=c["act_final"],
                     act_mode=c["act_mode"], bins=c["bins"], alow=c["alow"],
                     arange=c["arange"], noiseless_from=0)
    check("mlp_f32", name, got, y64, e32)


@gpu
def test_mlp_fwd_f32_rows_shared_by_eps(dev):
    """eps=2: slots 2r and 2r+1 read the SAME weight row (b // eps)."""
    c = build_fwd_case("vec_40x64_tail_only")
    obs = c["obs"].copy()
    obs[1] = obs[0]          # same row, same obs -> same action
    obs[2] = obs[0]          # next row, same obs -> different action
    got = launch_fwd(dev, c["dims"], c["w"], c["stride"], obs, c["obmean"], c["obstd"],
                     c["adim"], eps=2)
    assert np.array_equal(got[0], got[1])
    assert not np.array_equal(got[0], got[2])


@gpu
def test_mlp_fwd_f32_noiseless_from(dev):
    """Members >= noiseless_from match the (noise-free) oracle; members below
    it carry action noise and must differ from it. The noise itself is the
    bf16-weights kernel's: same counters and salts."""
    dims, B, k = [11, 16, 3], 4, 2
    rng = np.random.RandomState(77)
    w, stride = make_net_f32(rng, dims, B, 4)   # 248: rows 16-B aligned as bf16 too
    assert stride % 8 == 0
    n = n_params(dims)
    obs, obmean, obstd = make_obs(rng, B, dims[0])
    kw = dict(dims=dims, weight_rows=w[:, :n].astype(np.float64), obs=obs, obmean=obmean,
              obstd=obstd, ob_clip=OB_CLIP)
    y64, e32 = fp32_error_scale(policy_actions, **kw)
    got = launch_fwd(dev, dims, w, stride, obs, obmean, obstd, dims[-1],
                     noiseless_from=k, ac_std=0.3, seed=123, salt=4)
    check("mlp_f32", "noiseless_from_tail", got[k:], y64[k:], e32)
    for b in range(k):
        assert np.abs(got[b] - y64[b]).max() > 1e-3, b
    # same seed/salt/counters as es_mlp_fwd: on bf16-representable weights the
    # two kernels add the same noise to (nearly) the same net output
    from es_pytorch_amd import ops
    wb = np.nan_to_num(w, nan=0.0)
    bits = f32_to_bf16_bits(wb)
    wq = bf16_bits_to_f64(bits).astype(np.float32)
    got_q = launch_fwd(dev, dims, wq, stride, obs, obmean, obstd, dims[-1],
                       noiseless_from=k, ac_std=0.3, seed=123, salt=4)
    out = torch.full((B, dims[-1]), float("nan"), dtype=torch.float32, device=dev)
    w_d = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).to(dev)
    obs_d, mean_d, std_d = (_t(a, dev) for a in (obs, obmean, obstd))
    acs_d, seed_d = _t(np.array([0.3], np.float32), dev), _t(np.array([123], np.int64), dev)
    dims_arr = np.array(dims, dtype=np.int32)
    rc = ops.hip().es_mlp_fwd(out.data_ptr(), obs_d.data_ptr(), w_d.data_ptr(),
                              mean_d.data_ptr(), std_d.data_ptr(), dims_arr.ctypes.data,
                              len(dims), seed_d.data_ptr(), 4, B, OB_CLIP,
                              acs_d.data_ptr(), stride, 1, k, 0, 1, 0, None, None,
                              _stream(dev))
    assert rc == 0
    torch.cuda.synchronize(dev)
    assert np.abs(out.cpu().numpy() - got_q).max() < 1e-5
    # mode 2 draws its std from the net: same split
    dims2 = [11, 16, 4]
    w, stride = make_net_f32(rng, dims2, B)
    kw = dict(dims=dims2, weight_rows=w[:, :n_params(dims2)].astype(np.float64), obs=obs,
              obmean=obmean, obstd=obstd, ob_clip=OB_CLIP, act_mode=2)
    y64, e32 = fp32_error_scale(policy_actions, **kw)
    got = launch_fwd(dev, dims2, w, stride, obs, obmean, obstd, 3, act_mode=2,
                     noiseless_from=k, seed=123, salt=4)
    check("mlp_f32", "noiseless_from_tail_mode2", got[k:], y64[k:], e32)
    for b in range(k):
        assert np.abs(got[b] - y64[b]).max() > 1e-3, b


@gpu
@pytest.mark.parametrize("dims,stride_delta,want", [
    ([4] * 10, 0, -100),            # 9 layers > ES_MAXL
    ([4, 2049, 2], 0, -101),        # dim > ES_MAXDIM
    ([4, 8, 2], -1, -102),          # row_stride < n
])
def test_mlp_fwd_f32_argument_errors(dev, dims, stride_delta, want):
    from es_pytorch_amd import ops
    n = n_params(dims)
    stride = n + stride_delta
    buf = torch.zeros(max(n, 64) + 64, dtype=torch.float32, device=dev)
    f = torch.ones(4096, dtype=torch.float32, device=dev)
    out = torch.full((64,), 7.0, dtype=torch.float32, device=dev)
    dims_arr = np.array(dims, dtype=np.int32)
    rc = ops.hip().es_mlp_fwd_f32(out.data_ptr(), f.data_ptr(), buf.data_ptr(),
                                  f.data_ptr(), f.data_ptr(), dims_arr.ctypes.data,
                                  len(dims), None, 0, 1, OB_CLIP, None, stride, 1, 0, 0, 1,
                                  0, None, None, _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == want
    assert (out == 7.0).all(), "nothing may launch on an argument error"


# --------------------------------------------------------------------- rollout
ENV_SCALARS = dict(leak=0.35, ctrl=0.05, alive_bonus=1.0, fall_thr=0.0, dt=0.07)


def C(kernel, S, hidden, seed=0, adim=3, goal=0, terminate=1, bins=0, act_mode=0,
      members=6, eps=1, n_steps=1, block=256, member_base=0, wrow0=0, ac_std=0.0,
      seed_dev=None, salt=1, salt_base=0, noiseless_from=0):
    """ac_std, seed_dev, salt / salt_base and noiseless_from: the noise of
    tests/test_kernel_oracle_noise.py; the defaults are noise off."""
    return dict(kernel=kernel, S=S, hidden=hidden, seed=seed, adim=adim, goal=goal,
                terminate=terminate, bins=bins, act_mode=act_mode, members=members,
                eps=eps, n_steps=n_steps, block=block, member_base=member_base,
                wrow0=wrow0, ac_std=ac_std, seed_dev=seed_dev, salt=salt,
                salt_base=salt_base, noiseless_from=noiseless_from)


LOCO_CASES = {
    # ---- es_loco_step_f32: every state dim of the dynamics A-matvec
    "step_S8": C("step", 8, 16, adim=2, seed=1),
    "step_S64_eps2": C("step", 64, 16, eps=2),
    "step_S152": C("step", 152, 64),
    "step_S376": C("step", 376, 64, adim=17),
    "step_S11_scalar": C("step", 11, 16, seed=2),
    "step_S27_goal": C("step", 27, 16, adim=8, goal=1),
    "step_S64_binned": C("step", 64, 16, bins=5, seed=1),
    "step_S11_mode2": C("step", 11, 16, act_mode=2),
    "step_S152_mode3_noterm": C("step", 152, 16, act_mode=3, terminate=0, seed=1),
    # ---- es_loco_episode_f32, 256 threads, sub-range of slots on a sub-blob
    "episode256_S152_3steps": C("episode", 152, 64, members=8, n_steps=3, member_base=3,
                                wrow0=3),
    # ---- es_loco_episode_f32, 512 threads
    "episode512_376x256": C("episode", 376, 256, adim=17, members=5, block=512,
                            n_steps=3, member_base=1, wrow0=1, seed=5),
    "episode512_S11_binned": C("episode", 11, 16, bins=5, members=6, block=512,
                               n_steps=3, member_base=3, wrow0=3, seed=17),
}


def case_dims(c):
    out = c["adim"] * c["bins"] if c["bins"] > 1 else \
        c["adim"] + 1 if c["act_mode"] == 2 else \
        2 * c["adim"] if c["act_mode"] == 3 else c["adim"]
    return [c["S"] + 2 * c["goal"], c["hidden"], out]


def build_loco(name, cases=None):
    """Numpy inputs of a case: env matrices, a prescribed initial state with
    non-zero accumulators and mixed alive, the fp32 weight blob and the
    oracle's policy/env dicts. No GPU work."""
    c = (LOCO_CASES if cases is None else cases)[name]
    rng = np.random.RandomState(2000 + sum(ord(ch) for ch in name) + 7919 * c["seed"])
    S, A, g = c["S"], c["adim"], c["goal"]
    dims = case_dims(c)
    D = dims[0]
    n = n_params(dims)
    nslots = c["members"]
    A_bits = f32_to_bf16_bits((rng.randn(S, S) * (1.1 / np.sqrt(S))).astype(np.float32))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    env = dict(A_bits=A_bits, A=bf16_bits_to_f64(A_bits),
               B=f32(rng.randn(A, S) / np.sqrt(A)), b0=f32(rng.randn(S) * 0.1),
               wv=f32(rng.randn(S) / np.sqrt(S)), wa=f32(rng.randn(A) / np.sqrt(A)),
               wy=f32(rng.randn(S) / np.sqrt(S)), wh=f32(rng.randn(S) / np.sqrt(S)),
               terminate=c["terminate"], goal=g, **ENV_SCALARS)
    alive = (np.arange(nslots) % 3 != 1).astype(np.float32)   # mixed 0/1
    rng.shuffle(alive)
    state = dict(
        s=f32(rng.randn(nslots, S) * 0.6), pos=f32(rng.randn(nslots, 3)),
        goal=f32(rng.randn(nslots, 2) * 8.0) if g else None, alive=alive,
        rew_total=f32(rng.randn(nslots) * 3.0),
        member_steps=f32(rng.randint(0, 40, size=nslots)),
        behv=f32(rng.randn(nslots, 3)), mo_sum=f32(rng.randn(nslots, D) * 2.0),
        mo_sumsq=f32(rng.rand(nslots, D) * 3.0))
    obmean = f32(rng.randn(D) * 0.2)
    obstd = f32(rng.rand(D) * 0.5 + 0.3)
    obstd[::5] = 0.05          # some dims clip at +-OB_CLIP
    members = np.arange(c["member_base"], nslots)
    nrows = int(members.max()) // c["eps"] - c["wrow0"] + 1
    assert (members // c["eps"] - c["wrow0"]).min() == 0
    w, stride = make_net_f32(rng, dims, nrows)
    policy = dict(dims=dims, weight_rows=w[:, :n].astype(np.float64), obmean=obmean,
                  obstd=obstd, ob_clip=OB_CLIP, eps=c["eps"], wrow0=c["wrow0"],
                  act_mode=c["act_mode"], bins=c["bins"])
    return dict(c=c, name=name, dims=dims, stride=stride, env=env, state=state,
                obmean=obmean, obstd=obstd, w=w, policy=policy, members=members,
                nslots=nslots)


def loco_oracle(case, with_infos=False):
    """(y64 state, E32 per buffer over the stepped slots); asserts that no
    discrete outcome sits on a rounding edge and both outcomes occur."""
    c, m = case["c"], case["members"]
    env = {k: v for k, v in case["env"].items() if k != "A_bits"}
    noise = dict(seed=c["seed_dev"], ac_std=c["ac_std"],
                 noiseless_from=c["noiseless_from"])
    salt_base = c["salt_base"] if c["kernel"] == "episode" else c["salt"] - 1
    y64, infos = loco_rollout(case["state"], env, case["policy"], c["n_steps"], m,
                              np.float64, noise, salt_base)
    y32, _ = loco_rollout(case["state"], env, case["policy"], c["n_steps"], m, np.float32,
                          noise, salt_base)
    e32 = {k: err_scale(y32[k][m], y64[k][m]) for k in STATE_KEYS}
    for info in infos:
        assert (np.abs(info["h"] - np.float32(env["fall_thr"])) > 1e-3).all(), \
            "h on the fall threshold"
        if c["bins"] > 1:
            assert top2_logit_gap(info["net_out"], c["bins"]) > 1e-3, "logit tie"
    assert (case["state"]["alive"][m] == 0).any(), "case needs dead members"
    if c["terminate"]:
        was = case["state"]["alive"][m] > 0
        now = y64["alive"][m] > 0
        assert (was & ~now).any() and (was & now).any(), \
            "need both terminated and surviving members"
    if with_infos:
        return y64, e32, infos
    return y64, e32


def launch_loco(dev, case):
    from es_pytorch_amd import ops
    lib = ops.hip()
    c, env = case["c"], case["env"]
    st = {k: _t(v, dev) for k, v in case["state"].items() if v is not None}
    ev = {k: _t(env[k], dev) for k in ("B", "b0", "wv", "wa", "wy", "wh")}
    A_d = torch.from_numpy(np.ascontiguousarray(env["A_bits"]).view(np.int16).copy()) \
        .view(torch.bfloat16).to(dev)
    mean_d, std_d, w = _t(case["obmean"], dev), _t(case["obstd"], dev), _t(case["w"], dev)
    acstd = torch.full((1,), c["ac_std"], dtype=torch.float32, device=dev)
    seed_d = None if c["seed_dev"] is None else _t(np.array([c["seed_dev"]], np.int64), dev)
    dims_arr = np.array(case["dims"], dtype=np.int32)
    goal_ptr = st["goal"].data_ptr() if c["goal"] else None
    bufs = (st["s"].data_ptr(), st["pos"].data_ptr(), goal_ptr, A_d.data_ptr(),
            ev["B"].data_ptr(), ev["b0"].data_ptr(), ev["wv"].data_ptr(),
            ev["wa"].data_ptr(), ev["wy"].data_ptr(), ev["wh"].data_ptr(),
            st["alive"].data_ptr(), st["rew_total"].data_ptr(),
            st["member_steps"].data_ptr(), st["behv"].data_ptr(),
            st["mo_sum"].data_ptr(), st["mo_sumsq"].data_ptr())
    flags = (c["S"], c["adim"], c["goal"], c["terminate"], c["noiseless_from"], c["bins"],
             c["eps"], c["act_mode"])
    scal = tuple(float(env[k]) for k in ("leak", "ctrl", "alive_bonus", "fall_thr", "dt"))
    head = (mean_d.data_ptr(), std_d.data_ptr(), dims_arr.ctypes.data, len(dims_arr),
            None if seed_d is None else seed_d.data_ptr())
    tail = (OB_CLIP, acstd.data_ptr(), case["stride"])
    if c["kernel"] == "step":
        assert c["n_steps"] == 1
        rc = lib.es_loco_step_f32(w.data_ptr(), *head, c["salt"], *tail, *bufs, case["nslots"],
                                  *flags, *scal, _stream(dev))
    else:
        mb = c["member_base"]
        rc = lib.es_loco_episode_f32(w.data_ptr(), *head, c["n_steps"], *tail, *bufs, mb,
                                     case["nslots"] - mb, c["salt_base"], c["wrow0"], *flags,
                                     *scal,
                                     c["block"], _stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    return {kk: st[kk].cpu().numpy() for kk in STATE_KEYS}


def compare(label, got, y64, e32, state0, members):
    """Continuous buffers within 16 E32; counters, alive, everything a dead
    member owns and every slot outside `members` exact."""
    m = members

    def ratio(k):
        d = float(np.max(np.abs(got[k][m].astype(np.float64) - y64[k][m])))
        return 0.0 if d == 0.0 else d / e32[k] if e32[k] > 0 else np.inf

    for k in STATE_KEYS:
        assert np.isfinite(got[k][m]).all(), (label, k)
        print(f"ORACLE-RATIO loco_f32 {label} {k} ratio={ratio(k):.2f} E32={e32[k]:.3g}")
    worst = max(STATE_KEYS, key=ratio)
    print(f"ORACLE-RATIO loco_f32 {label} WORST ratio={ratio(worst):.2f} ({worst})")
    assert np.array_equal(got["member_steps"][m], y64["member_steps"][m]), label
    assert np.array_equal(got["alive"][m], y64["alive"][m]), label
    dead = m[state0["alive"][m] == 0]
    assert dead.size, "case needs dead members"
    for k in ("behv", "rew_total", "mo_sum", "mo_sumsq", "member_steps", "alive"):
        assert np.array_equal(got[k][dead], state0[k][dead]), (label, k, "dead moved")
    rest = np.setdiff1d(np.arange(state0["s"].shape[0]), m)
    for k in STATE_KEYS:
        assert np.array_equal(got[k][rest], state0[k][rest]), (label, k, "untouched slot")
    for k in STATE_KEYS:
        assert ratio(k) <= ERR_FACTOR, (label, k, ratio(k), e32[k])


@pytest.mark.parametrize("name", list(LOCO_CASES))
def test_loco_f32_cases_meet_their_input_conditions(name):
    """No GPU: the seeds give dead members, both termination outcomes and no
    discrete outcome on a rounding edge (asserted inside loco_oracle)."""
    loco_oracle(build_loco(name))


@gpu
@pytest.mark.parametrize("name", list(LOCO_CASES))
def test_loco_f32_kernel_matches_oracle(dev, name):
    case = build_loco(name)
    y64, e32 = loco_oracle(case)
    got = launch_loco(dev, case)
    compare(name, got, y64, e32, case["state"], case["members"])
