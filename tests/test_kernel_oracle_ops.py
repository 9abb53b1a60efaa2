"""es_grad_gather, es_pheno_bf16, es_pheno_fp8, es_adam_step and es_sgd_step
against the float64 oracle (tests/oracle64.py), at the sizes where each
kernel switches branch.

Encodings (bf16, e4m3) and one-hot quantized gathers are compared exactly.
Continuous outputs are bounded by ``16 * E32`` with E32 the error of the same
computation in numpy float32.

The pheno_bf16 cases use a power-of-two sigma: ``sign * sigma * noise`` is
then exact in float32, so ``theta + sign*sigma*noise`` has ONE float32
rounding whether or not the compiler fuses it into an FMA, and the bf16 bits
are uniquely defined. The small sizes repeat at sigma = 0.02, where each
element must equal the bf16 rounding of the fused or of the unfused sum.

Measured on MI355X, max |err| / E32 per case (bound: 16):

  es_grad_gather (n_params: elems1=4097, elems2=524365, elems4=1049089)
  ELEMS     n_pop    qstd=0 qstd=.02
  elems1        1      0.53     0.50
  elems1        2      0.66     0.92
  elems1      256      1.16     0.95
  elems1      257      0.89     1.13
  elems1      333      1.00     1.00
  elems2        1      0.70     0.62
  elems2        2      0.55     1.00
  elems2      256      1.02     1.00
  elems2      257      1.00     1.14
  elems2      333      1.00     1.00
  elems4        1      0.75     0.62
  elems4        2      0.90     0.91
  elems4      256      1.00     1.00
  elems4      257      1.00     0.94
  elems4      333      1.00     1.00

  buffer        ratio  E32
  adam_theta     1.00  5.3e-07
  adam_m         1.00  1.38e-07
  adam_v         1.00  2.16e-08
  sgd_theta      1.00  4.74e-07
  sgd_v          1.00  1.37e-07
"""
import numpy as np
import pytest
import torch

from tests.oracle64 import (ERR_FACTOR, adam_steps, e4m3_byte_to_f64, e4m3_roundtrip_f32,
                            f32_to_bf16_bits, fp32_error_scale, fp8_byte_position,
                            grad_gather, max_ratio, n_params, quantized_table, sgd_steps)

pytestmark = pytest.mark.gpu

TABLE_N = 1_300_000
GATHER_N = {"elems1": 4097, "elems2": 524_288 + 77, "elems4": 1_048_576 + 513}
QSTD = 0.02

# fp8 blob layouts: even / odd first-layer input, scalar head, misaligned
# later layer in plain order (also listed in tests/test_oracle64_cpu.py)
FP8_PHENO_DIMS = {
    "even_input_scalar_head": [12, 16, 3],
    "odd_input_vec_head": [29, 64, 8],
    "misaligned_layer_plain": [3, 7, 16, 4],
    "hidden64_head17": [64, 24, 17],
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@pytest.fixture(scope="module")
def table():
    """Shared read-only noise table: float32 values, their e4m3 round trip at
    QSTD, and the device copy (made on first use)."""
    rng = np.random.RandomState(1234)
    t = rng.randn(TABLE_N).astype(np.float32)
    return {"f32": t, "q": quantized_table(t, QSTD), "dev": None}


def _table_dev(table, dev):
    if table["dev"] is None:
        table["dev"] = torch.from_numpy(table["f32"]).to(dev)
    return table["dev"]


def _gather(dev, table, offs, fits, n, qstd):
    from es_pytorch_amd import ops
    offs_d = torch.from_numpy(offs).to(dev)
    fits_d = torch.from_numpy(fits).to(dev)
    g = torch.full((n + 8,), 7.0, dtype=torch.float32, device=dev)
    rc = ops.hip().es_grad_gather(g.data_ptr(), _table_dev(table, dev).data_ptr(),
                                  fits_d.data_ptr(), offs_d.data_ptr(), len(offs), n,
                                  float(qstd), _stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    out = g.cpu().numpy()
    assert (out[n:] == 7.0).all(), "wrote past n_params"
    return out[:n]


@pytest.mark.parametrize("qstd", [0.0, QSTD])
@pytest.mark.parametrize("n_pop", [1, 2, 256, 257, 333])
@pytest.mark.parametrize("nkey", list(GATHER_N))
def test_grad_gather_matches_oracle(dev, table, nkey, n_pop, qstd):
    n = GATHER_N[nkey]
    rng = np.random.RandomState(n_pop * 7 + len(nkey) + int(qstd > 0))
    offs = rng.randint(0, TABLE_N - n, size=n_pop).astype(np.int64)
    fits = rng.randn(n_pop).astype(np.float32)
    vals = table["q"] if qstd > 0 else table["f32"]
    y64, e32 = fp32_error_scale(grad_gather, vals, offs, fits, n)
    got = _gather(dev, table, offs, fits, n, qstd)
    r = max_ratio(got, y64, e32)
    print(f"ORACLE-RATIO ops gather_{nkey}_pop{n_pop}_q{int(qstd > 0)} ratio={r:.2f} "
          f"E32={e32:.3g}")
    assert r <= ERR_FACTOR, (r, e32)


@pytest.mark.parametrize("n_pop,hot", [(1, 0), (2, 1), (257, 100), (257, 256), (333, 300)])
@pytest.mark.parametrize("nkey", list(GATHER_N))
def test_grad_gather_quantized_one_hot_exact(dev, table, nkey, n_pop, hot):
    """One-hot fits: the gather returns exactly the e4m3 round trip of the hot
    row — in the middle of a pipelined tile, at a tile's single-row tail, and
    in the n_pop=1 fallback."""
    n = GATHER_N[nkey]
    rng = np.random.RandomState(n_pop + hot)
    offs = rng.randint(0, TABLE_N - n, size=n_pop).astype(np.int64)
    fits = np.zeros(n_pop, dtype=np.float32)
    fits[hot] = 1.0
    got = _gather(dev, table, offs, fits, n, QSTD)
    want = table["q"][offs[hot]:offs[hot] + n]
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # the transform is not the identity on this table, so a dropped
    # quantization step cannot pass
    assert not np.array_equal(want, table["f32"][offs[hot]:offs[hot] + n])


# ------------------------------------------------------------------ pheno bf16
def _pheno_bf16(dev, theta, tab_d, offs, signs, n, stride, std):
    from es_pytorch_amd import ops
    P = len(offs)
    out = torch.full((P, stride), -21555, dtype=torch.int16, device=dev)  # 0xABCD
    # every device buffer stays referenced until the kernel has finished
    th_d = torch.from_numpy(theta).to(dev)
    offs_d = torch.from_numpy(offs).to(dev)
    signs_d = torch.from_numpy(signs).to(dev)
    rc = ops.hip().es_pheno_bf16(out.data_ptr(), th_d.data_ptr(), tab_d.data_ptr(),
                                 offs_d.data_ptr(), signs_d.data_ptr(), P, n, stride,
                                 float(std), _stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    return out.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("n,pad", [(1000, 0), (1001, 7), (1007, 9), (1000, 8),
                                   (2_097_152 + 13, 11)])
def test_pheno_bf16_bit_exact(dev, table, n, pad):
    """n % 8 in {0, 1, 7}, row_stride = n + pad, and n > 1024*2048 (two rows)
    where the grid-stride loop iterates; offsets of every residue mod 4."""
    big = n > 2_000_000
    rng = np.random.RandomState(n % 1000 + pad)
    if big:
        tab = rng.randn(n + 16).astype(np.float32)
        tab_d = torch.from_numpy(tab).to(dev)
        offs = np.array([3, 6], dtype=np.int64)
        signs = np.array([1.0, -1.0], dtype=np.float32)
    else:
        tab, tab_d = table["f32"], _table_dev(table, dev)
        offs = np.array([0, 1, 2, 3, 4001, 70_002, 900_007], dtype=np.int64)
        signs = np.array([1, -1, 1, -1, 0, 1, -1], dtype=np.float32)
    assert set(offs % 4) == ({3, 2} if big else {0, 1, 2, 3})
    stride = n + pad
    assert stride % 8 == 0 and stride >= n      # rows stay 16-B aligned
    theta = rng.randn(n).astype(np.float32)
    std = np.float32(2.0 ** -5)
    got = _pheno_bf16(dev, theta, tab_d, offs, signs, n, stride, std)
    for p, (o, sg) in enumerate(zip(offs, signs)):
        want = f32_to_bf16_bits(theta + (np.float32(sg) * std) * tab[o:o + n])
        bad = np.flatnonzero(got[p, :n] != want)
        assert bad.size == 0, (p, bad[:5], got[p, bad[:5]], want[bad[:5]])
        assert (got[p, n:] == 0xABCD).all(), f"row {p}: padding overwritten"
    if big:
        return
    # realistic sigma: the product now rounds, so the kernel may legitimately
    # produce either the fused (one rounding) or the unfused (two roundings)
    # float32 sum; each element must be the bf16 RNE of one of the two
    std = np.float32(0.02)
    got = _pheno_bf16(dev, theta, tab_d, offs, signs, n, stride, std)
    for p, (o, sg) in enumerate(zip(offs, signs)):
        s32 = np.float32(sg) * std
        unfused = f32_to_bf16_bits(theta + s32 * tab[o:o + n])
        fused = f32_to_bf16_bits((theta.astype(np.float64) + np.float64(s32) *
                                  tab[o:o + n].astype(np.float64)).astype(np.float32))
        ok = (got[p, :n] == unfused) | (got[p, :n] == fused)
        assert ok.all(), (p, np.flatnonzero(~ok)[:5])


# ------------------------------------------------------------------- pheno fp8
@pytest.mark.parametrize("std", [0.02, 0.7])
@pytest.mark.parametrize("key", list(FP8_PHENO_DIMS))
def test_pheno_fp8_exact(dev, table, key, std):
    from es_pytorch_amd import ops
    dims = FP8_PHENO_DIMS[key]
    n = n_params(dims)
    stride = (n + 15) // 16 * 16 + 16
    offs = np.array([0, 1, 2, 3, 555_555], dtype=np.int64)
    P = len(offs)
    out = torch.full((P + 1, stride), 0x55, dtype=torch.uint8, device=dev)
    dims_arr = np.array(dims, dtype=np.int32)
    offs_d = torch.from_numpy(offs).to(dev)     # referenced until the sync below
    rc = ops.hip().es_pheno_fp8(out.data_ptr(), _table_dev(table, dev).data_ptr(),
                                offs_d.data_ptr(), dims_arr.ctypes.data, len(dims), P, n, stride, float(std),
                                _stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    blob = out.cpu().numpy()
    pos = fp8_byte_position(dims)
    assert sorted(pos) == list(range(n))
    for p, o in enumerate(offs):
        want = e4m3_roundtrip_f32(np.float32(std) * table["f32"][o:o + n])
        got = e4m3_byte_to_f64(blob[p][pos])
        assert not np.isnan(got).any()
        bad = np.flatnonzero(got != want)        # value compare: -0 == 0
        assert bad.size == 0, (p, bad[:5], got[bad[:5]], want[bad[:5]])
        assert (blob[p, n:] == 0).all(), "row padding must be zero"
    assert (blob[P] == 0x55).all(), "wrote past the last row"
    # the case must be able to tell rounding modes apart: some value sits in
    # the upper half of its e4m3 interval (truncation would differ)
    exact = np.float32(std) * table["f32"][:n]
    assert (np.abs(e4m3_roundtrip_f32(exact)) > np.abs(exact)).any()


# ------------------------------------------------------------------ optimizers
OPT_N = 524_288 + 1234      # > 2048 blocks * 256 threads: the loops iterate


def test_adam_step_grid_stride_matches_oracle(dev):
    from es_pytorch_amd import ops
    rng = np.random.RandomState(5)
    theta0 = rng.randn(OPT_N).astype(np.float32)
    m0 = (rng.randn(OPT_N) * 0.1).astype(np.float32)
    v0 = (rng.rand(OPT_N) * 0.1).astype(np.float32)
    g = (rng.randn(OPT_N) * 64).astype(np.float32)
    lr, b1, b2, eps, l2, gscale = 0.01, 0.9, 0.999, 1e-8, 0.005, 1.0 / 64
    a_list = [lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) for t in (1, 2, 3)]
    y64, e32 = fp32_error_scale(adam_steps, theta0, m0, v0, g, a_list, b1, b2, eps, l2,
                                gscale)
    th, m, v, gd = (torch.from_numpy(x.copy()).to(dev) for x in (theta0, m0, v0, g))
    for a in a_list:
        rc = ops.hip().es_adam_step(th.data_ptr(), m.data_ptr(), v.data_ptr(),
                                    gd.data_ptr(), OPT_N, float(a), b1, b2, eps, l2,
                                    gscale, _stream(dev))
        assert rc == 0, rc
    torch.cuda.synchronize(dev)
    for k, t in (("theta", th), ("m", m), ("v", v)):
        r = max_ratio(t.cpu().numpy(), y64[k], e32[k])
        print(f"ORACLE-RATIO ops adam_{k} ratio={r:.2f} E32={e32[k]:.3g}")
        assert r <= ERR_FACTOR, (k, r, e32[k])
    assert np.array_equal(gd.cpu().numpy(), g)


def test_sgd_step_grid_stride_matches_oracle(dev):
    from es_pytorch_amd import ops
    rng = np.random.RandomState(6)
    theta0 = rng.randn(OPT_N).astype(np.float32)
    v0 = (rng.randn(OPT_N) * 0.1).astype(np.float32)
    g = (rng.randn(OPT_N) * 64).astype(np.float32)
    lr, mom, l2, gscale = 0.01, 0.9, 0.005, 1.0 / 64
    y64, e32 = fp32_error_scale(sgd_steps, theta0, v0, g, 3, lr, mom, l2, gscale)
    th, v, gd = (torch.from_numpy(x.copy()).to(dev) for x in (theta0, v0, g))
    for _ in range(3):
        rc = ops.hip().es_sgd_step(th.data_ptr(), v.data_ptr(), gd.data_ptr(), OPT_N, lr,
                                   mom, l2, gscale, _stream(dev))
        assert rc == 0, rc
    torch.cuda.synchronize(dev)
    for k, t in (("theta", th), ("v", v)):
        r = max_ratio(t.cpu().numpy(), y64[k], e32[k])
        print(f"ORACLE-RATIO ops sgd_{k} ratio={r:.2f} E32={e32[k]:.3g}")
        assert r <= ERR_FACTOR, (k, r, e32[k])
