"""The reference's own fp32 perturbed forwards (recorded once by
tools/make_ref_fp32_fixture.py into tests/golden/fp32_forward/*.npz) against
the float64 oracle, and the fp32 HIP kernels against both.

The oracle runs on the singly-rounded fp32 member rows
``float32(flat + float32(+-std) * noise)`` permuted to the forward layout; the
reference rounds the product and the sum separately and runs torch's fp32
forward. Bound: ``16 * E32`` (E32: the oracle's forward in numpy float32).

cpu: recorded reference outputs within 16 E32 of the oracle. Measured
max |ref - oracle64| / E32:

  fixture               ratio  E32
  d11_16_24_3_s020       0.87  7.12e-07
  d11_16_24_3_s050       0.92  2.42e-07
  d29_64_8_s020          0.85  4.94e-07

gpu: es_pheno_f32 + es_mlp_fwd_f32 on the same inputs within 16 E32 of the
oracle, hence within 32 E32 of the recorded reference outputs (asserted).
Measured on MI355X, max |kernel - oracle64| / E32 and max |kernel - ref| / E32:

  fixture               oracle  reference
  d11_16_24_3_s020        0.86       0.92
  d11_16_24_3_s050        1.02       1.48
  d29_64_8_s020           0.90       1.39
"""
import glob
import os

import numpy as np
import pytest
import torch

from tests.oracle64 import ERR_FACTOR, fp32_error_scale, max_ratio, policy_actions
from tests.oracle64_f32 import flat_to_forward, fp32_member_rows

FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                         "golden", "fp32_forward", "*.npz")))
NAMES = [os.path.splitext(os.path.basename(p))[0] for p in FIXTURES]


def load(path):
    """Fixture -> oracle inputs. Members are [+noise rows | -noise rows];
    slot b = member * n_obs + k evaluates observation k."""
    f = np.load(path)
    dims = [int(v) for v in f["dims"]]
    P, K = f["noise"].shape[0], f["obs"].shape[0]
    theta = flat_to_forward(dims, f["flat"])
    noise = flat_to_forward(dims, f["noise"])
    noise2 = np.concatenate([noise, noise])
    signs = np.concatenate([np.ones(P), -np.ones(P)]).astype(np.float32)
    rows = fp32_member_rows(theta, noise2, signs, f["std"])
    obs = np.tile(f["obs"], (2 * P, 1))
    kw = dict(dims=dims, weight_rows=rows.astype(np.float64), obs=obs,
              obmean=f["obmean"], obstd=f["obstd"], ob_clip=float(f["ob_clip"]), eps=K,
              act_final=1)
    ref = np.concatenate([f["out_pos"], f["out_neg"]]).reshape(2 * P * K, dims[-1])
    return dict(f=f, dims=dims, theta=theta, noise=noise, signs=signs, rows=rows,
                obs=obs, kw=kw, ref=ref, P=P, K=K)


def test_fixtures_present():
    assert len(FIXTURES) == 3, FIXTURES


@pytest.mark.parametrize("name,path", list(zip(NAMES, FIXTURES)), ids=NAMES)
def test_reference_outputs_match_oracle(name, path):
    c = load(path)
    xn = (c["obs"].astype(np.float64) - c["f"]["obmean"]) / c["f"]["obstd"]
    clip = float(c["f"]["ob_clip"])
    assert (np.abs(xn) > clip).any() and (np.abs(xn) < clip).any()
    # the perturbation is visible at this precision: +noise and -noise differ
    assert np.abs(c["f"]["out_pos"] - c["f"]["out_neg"]).max() > 1e-3
    y64, e32 = fp32_error_scale(policy_actions, **c["kw"])
    r = max_ratio(c["ref"], y64, e32)
    print(f"ORACLE-RATIO ref_fp32 {name} ratio={r:.2f} E32={e32:.3g}")
    assert r <= ERR_FACTOR, (name, r, e32)


@pytest.mark.gpu
@pytest.mark.parametrize("name,path", list(zip(NAMES, FIXTURES)), ids=NAMES)
def test_fp32_kernels_match_oracle_and_reference(name, path):
    from es_pytorch_amd import ops
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    c = load(path)
    dims, P, K = c["dims"], c["P"], c["K"]
    n = c["theta"].size
    M, B = 2 * P, 2 * P * K
    stride = (n + 7) // 8 * 8
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    # noise table: row p starts at residue p mod 4, so every 4-B alignment occurs
    gap = (n + 7) // 4 * 4
    table = np.zeros(P * gap + 8, dtype=np.float32)
    offs = np.array([p * gap + p % 4 for p in range(P)] * 2, dtype=np.int64)
    for p in range(P):
        table[offs[p]:offs[p] + n] = c["noise"][p]
    assert set(offs % 4) == {0, 1, 2, 3}
    th_d, tab_d, offs_d, signs_d = t(c["theta"]), t(table), t(offs), t(c["signs"])
    w = torch.full((M, stride), float("nan"), dtype=torch.float32, device=dev)
    rc = ops.hip().es_pheno_f32(w.data_ptr(), th_d.data_ptr(), tab_d.data_ptr(),
                                offs_d.data_ptr(), signs_d.data_ptr(), M, n, stride,
                                float(c["f"]["std"]), stream)
    assert rc == 0, rc
    obs_d, mean_d, std_d = t(c["obs"]), t(c["f"]["obmean"]), t(c["f"]["obstd"])
    out = torch.full((B, dims[-1]), float("nan"), dtype=torch.float32, device=dev)
    dims_arr = np.array(dims, dtype=np.int32)
    rc = ops.hip().es_mlp_fwd_f32(out.data_ptr(), obs_d.data_ptr(), w.data_ptr(),
                                  mean_d.data_ptr(), std_d.data_ptr(),
                                  dims_arr.ctypes.data, len(dims), None, 0, B,
                                  float(c["f"]["ob_clip"]), None, stride, 1, 0, 0, K, 0,
                                  None, None, stream)
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    got_rows = w.cpu().numpy()[:, :n]
    assert np.array_equal(got_rows.view(np.uint32), c["rows"].view(np.uint32)), \
        "pheno rows differ from the singly-rounded oracle rows"
    got = out.cpu().numpy()
    y64, e32 = fp32_error_scale(policy_actions, **c["kw"])
    r = max_ratio(got, y64, e32)
    rr = max_ratio(got, c["ref"], e32)
    print(f"ORACLE-RATIO ref_fp32_gpu {name} ratio={r:.2f} vs_reference={rr:.2f} "
          f"E32={e32:.3g}")
    assert np.isfinite(got).all()
    assert r <= ERR_FACTOR, (name, r, e32)
    assert rr <= 2 * ERR_FACTOR, (name, rr, e32)
