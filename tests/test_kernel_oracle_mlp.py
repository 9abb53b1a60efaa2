"""es_mlp_fwd against the float64 oracle, one case per mlp_layers branch.

Every case calls the kernel directly on test-owned buffers and asserts
``|kernel - oracle64| <= 16 * E32`` where E32 is the error of the same
forward evaluated in numpy float32 (tests/oracle64.py). Block size is 256, so
for a layer (I, O): vec path OCT = O/8, PART = 256 // OCT; scalar path
PART = 256 // O.

Measured on MI355X, max |err| / E32 per case (bound: 16):

  case                                ratio  E32
  vec_11x8_one_layer                   1.00  3.29e-07
  vec_100x64_tail_only                 1.97  1.34e-07
  vec_130x64_prologue_drain            0.84  1.61e-07
  vec_260x64_steady_loop               0.22  3.11e-07
  vec_400x24_oct3                      0.74  3.68e-07
  vec_376x256_flagship                 0.33  4.04e-07
  vec_9x2048_part1                     0.51  2.99e-07
  scalar_10x130_thread_per_output      0.26  2.32e-07
  scalar_5x300_two_sweeps              0.21  3.37e-07
  scalar_7x16_misaligned_woff          1.35  3.12e-08
  eight_layers                         2.36  1.55e-08
  binned_decode                        0.36  1.66e-07
  mode2_integ_gauss                    0.81  7.29e-08
  mode3_integ_gauss_multi              1.62  7.78e-08
  noiseless_from_tail                  0.80  5.21e-08
  noiseless_from_tail_mode2            0.70  8.42e-08
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import (ERR_FACTOR, bf16_bits_to_f64, f32_to_bf16_bits,
                            fp32_error_scale, max_ratio, n_params, policy_actions,
                            top2_logit_gap)

pytestmark = pytest.mark.gpu

OB_CLIP = 5.0

# name -> (dims, B, eps, act_final, act_mode, bins, stride_pad)
CASES = {
    # vec path
    "vec_11x8_one_layer": ([11, 8], 3, 1, 0, 0, 0, 0),
    "vec_100x64_tail_only": ([100, 64, 3], 4, 2, 1, 0, 0, 0),
    "vec_130x64_prologue_drain": ([130, 64, 3], 3, 1, 0, 0, 0, 8),
    "vec_260x64_steady_loop": ([260, 64, 3], 3, 1, 1, 0, 0, 0),
    "vec_400x24_oct3": ([400, 24, 5], 3, 1, 1, 0, 0, 0),
    "vec_376x256_flagship": ([376, 256, 256, 17], 6, 2, 1, 0, 0, 0),
    "vec_9x2048_part1": ([9, 2048, 5], 2, 1, 1, 0, 0, 0),
    # scalar path ((256,17) and (64,3) also ride on the nets above)
    "scalar_10x130_thread_per_output": ([10, 130, 4], 3, 1, 1, 0, 0, 0),
    "scalar_5x300_two_sweeps": ([5, 300, 2], 3, 1, 0, 0, 0, 0),
    "scalar_7x16_misaligned_woff": ([3, 7, 16, 4], 3, 1, 1, 0, 0, 0),
    # depth
    "eight_layers": ([6, 16, 12, 16, 8, 24, 16, 8, 4], 3, 1, 1, 0, 0, 0),
    # decode modes
    "binned_decode": ([11, 64, 15], 5, 1, 1, 0, 5, 0),
    "mode2_integ_gauss": ([11, 16, 4], 4, 2, 1, 2, 0, 0),
    "mode3_integ_gauss_multi": ([11, 16, 6], 4, 1, 1, 3, 0, 0),
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def make_net(rng, dims, rows, stride_pad=0):
    """bf16 weight blob (rows+1 guard row, stride) with per-layer scale
    0.7/sqrt(I) so pre-activations stay O(1); returns (bits, values, stride)."""
    n = n_params(dims)
    stride = (n + 7) // 8 * 8 + stride_pad
    w = np.zeros((rows + 1, stride), dtype=np.float32)
    off = 0
    for I, O in zip(dims[:-1], dims[1:]):
        w[:, off:off + I * O] = rng.randn(rows + 1, I * O) * (0.7 / np.sqrt(I))
        off += I * O
        w[:, off:off + O] = rng.randn(rows + 1, O) * 0.1
        off += O
    bits = f32_to_bf16_bits(w)
    return bits, bf16_bits_to_f64(bits), stride


def make_obs(rng, B, D):
    """obs = mean + std * z with some |z| beyond the clip and small stds."""
    obmean = (rng.randn(D) * 0.3).astype(np.float32)
    obstd = (rng.rand(D) + 0.5).astype(np.float32)
    obstd[::3] = 0.01
    z = rng.randn(B, D) * 1.5
    z[:, ::4] = 8.0 * np.sign(z[:, ::4])
    obs = (obmean + obstd * z).astype(np.float32)
    return obs, obmean, obstd


def bf16_tensor(bits, dev):
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).to(dev)


def launch(dev, dims, wbits, stride, obs, obmean, obstd, adim_out, eps=1, act_final=1,
           act_mode=0, bins=0, alow=None, arange=None, noiseless_from=0, ac_std=None,
           seed=None, salt=0):
    from es_pytorch_amd import ops
    B = obs.shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    w_d, obs_d, mean_d, std_d = bf16_tensor(wbits, dev), t(obs), t(obmean), t(obstd)
    out = torch.full((B, adim_out), float("nan"), dtype=torch.float32, device=dev)
    alow_d = t(alow) if alow is not None else None
    ar_d = t(arange) if arange is not None else None
    acs_d = t(np.array([ac_std], np.float32)) if ac_std is not None else None
    seed_d = t(np.array([seed], np.int64)) if seed is not None else None
    dims_arr = np.array(dims, dtype=np.int32)
    rc = ops.hip().es_mlp_fwd(
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


def check(name, got, y64, e32):
    r = max_ratio(got, y64, e32)
    print(f"ORACLE-RATIO mlp {name} ratio={r:.2f} E32={e32:.3g}")
    assert np.isfinite(got).all(), name
    assert r <= ERR_FACTOR, (name, r, e32)


def build_case(name):
    dims, B, eps, act_final, act_mode, bins, pad = CASES[name]
    rng = np.random.RandomState(sum(ord(ch) for ch in name))  # stable per case
    rows = (B + eps - 1) // eps
    wbits, wvals, stride = make_net(rng, dims, rows, pad)
    obs, obmean, obstd = make_obs(rng, B, dims[0])
    A = dims[-1]
    adim = A - 1 if act_mode == 2 else A // 2 if act_mode == 3 else \
        A // bins if bins > 1 else A
    alow = arange = None
    if bins > 1:
        alow = (rng.randn(adim) - 2.0).astype(np.float32)
        arange = (rng.rand(adim) * 3.0 + 0.5).astype(np.float32)
    kw = dict(dims=dims, weight_rows=wvals, obs=obs, obmean=obmean, obstd=obstd,
              ob_clip=OB_CLIP, eps=eps, act_final=act_final, act_mode=act_mode,
              bins=bins, alow=alow, arange=arange)
    return dict(dims=dims, B=B, eps=eps, act_final=act_final, act_mode=act_mode,
                bins=bins, wbits=wbits, stride=stride, obs=obs, obmean=obmean,
                obstd=obstd, adim=adim, alow=alow, arange=arange, kw=kw)


@pytest.mark.parametrize("name", list(CASES))
def test_mlp_fwd_matches_oracle(dev, name):
    c = build_case(name)
    y64, e32 = fp32_error_scale(policy_actions, **c["kw"])
    if c["bins"] > 1:
        _, net = policy_actions(**c["kw"])
        assert top2_logit_gap(net, c["bins"]) > 1e-3, "binned logits on a rounding edge"
    # the inputs must exercise what the case claims
    xn = (c["obs"].astype(np.float64) - c["obmean"]) / c["obstd"]
    assert (np.abs(xn) > OB_CLIP).any() and (np.abs(xn) < OB_CLIP).any()
    got = launch(dev, c["dims"], c["wbits"], c["stride"], c["obs"], c["obmean"],
                 c["obstd"], c["adim"], eps=c["eps"], act_final=c["act_final"],
                 act_mode=c["act_mode"], bins=c["bins"], alow=c["alow"],
                 arange=c["arange"], noiseless_from=0)
    check(name, got, y64, e32)


def test_mlp_fwd_rows_shared_by_eps(dev):
    """eps=2: slots 2r and 2r+1 read the SAME weight row (b // eps)."""
    c = build_case("vec_100x64_tail_only")
    obs = c["obs"].copy()
    obs[1] = obs[0]          # same row, same obs -> same action
    obs[2] = obs[0]          # next row, same obs -> different action
    got = launch(dev, c["dims"], c["wbits"], c["stride"], obs, c["obmean"], c["obstd"],
                 c["adim"], eps=2)
    assert np.array_equal(got[0], got[1])
    assert not np.array_equal(got[0], got[2])


def test_mlp_fwd_noiseless_from(dev):
    """Members >= noiseless_from match the (noise-free) oracle; members below
    it carry action noise and must differ from it."""
    dims, B, k = [11, 16, 3], 4, 2
    rng = np.random.RandomState(77)
    wbits, wvals, stride = make_net(rng, dims, B)
    obs, obmean, obstd = make_obs(rng, B, dims[0])
    kw = dict(dims=dims, weight_rows=wvals, obs=obs, obmean=obmean, obstd=obstd,
              ob_clip=OB_CLIP)
    y64, e32 = fp32_error_scale(policy_actions, **kw)
    got = launch(dev, dims, wbits, stride, obs, obmean, obstd, dims[-1],
                 noiseless_from=k, ac_std=0.3, seed=123, salt=4)
    check("noiseless_from_tail", got[k:], y64[k:], e32)
    for b in range(k):
        assert np.abs(got[b] - y64[b]).max() > 1e-3, b
    # mode 2 draws its std from the net: same split
    dims2 = [11, 16, 4]
    wbits, wvals, stride = make_net(rng, dims2, B)
    kw = dict(dims=dims2, weight_rows=wvals, obs=obs, obmean=obmean, obstd=obstd,
              ob_clip=OB_CLIP, act_mode=2)
    y64, e32 = fp32_error_scale(policy_actions, **kw)
    got = launch(dev, dims2, wbits, stride, obs, obmean, obstd, 3, act_mode=2,
                 noiseless_from=k, seed=123, salt=4)
    check("noiseless_from_tail_mode2", got[k:], y64[k:], e32)
    for b in range(k):
        assert np.abs(got[b] - y64[b]).max() > 1e-3, b


@pytest.mark.parametrize("dims,stride_delta,want", [
    ([4] * 10, 0, -100),            # 9 layers > ES_MAXL
    ([4, 2049, 2], 0, -101),        # dim > ES_MAXDIM
    ([4, 8, 2], -1, -102),          # row_stride < n
])
def test_mlp_fwd_argument_errors(dev, dims, stride_delta, want):
    from es_pytorch_amd import ops
    n = n_params(dims)
    stride = n + stride_delta
    buf = torch.zeros(max(n, 64) + 64, dtype=torch.bfloat16, device=dev)
    f = torch.ones(4096, dtype=torch.float32, device=dev)
    out = torch.full((64,), 7.0, dtype=torch.float32, device=dev)
    dims_arr = np.array(dims, dtype=np.int32)
    rc = ops.hip().es_mlp_fwd(out.data_ptr(), f.data_ptr(), buf.data_ptr(), f.data_ptr(),
                              f.data_ptr(), dims_arr.ctypes.data, len(dims), None, 0, 1,
                              OB_CLIP, None, stride, 1, 0, 0, 1, 0, None, None,
                              _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == want
    assert (out == 7.0).all(), "nothing may launch on an argument error"
