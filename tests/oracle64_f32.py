"""Oracle helpers for the fp32-weights mode (weights_dtype = "fp32").

Plain numpy like tests/oracle64.py, and no code shared with ``es_pytorch_amd``.
The fp32 member row is defined by ONE rounding,

    row[b][t] = float32( theta[t] + float32(sign[b] * std) * noise[b][t] )

evaluated here in float64 and rounded once (tests/test_kernel_oracle_f32.py
checks on its seeded inputs that float64 is wide enough for that to be the
correctly rounded result).
"""
import numpy as np


def fp32_member_rows(theta, noise_rows, signs, std):
    """theta (n,), noise_rows (M, n), signs (M,), std scalar -> (M, n) float32
    VALUES of the fp32 member rows, singly rounded."""
    th = np.asarray(theta, dtype=np.float32).astype(np.float64)[None, :]
    nz = np.asarray(noise_rows, dtype=np.float32).astype(np.float64)
    s32 = (np.asarray(signs, dtype=np.float32) * np.float32(std)).astype(np.float32)
    return (th + s32.astype(np.float64)[:, None] * nz).astype(np.float32)


def flat_to_forward(dims, flat):
    """Reorder the last axis from the flat state_dict layout (per layer W as
    (O, I) row-major, then b) to the forward layout (per layer W^T as (I, O)
    row-major, then b)."""
    flat = np.asarray(flat)
    out = np.empty_like(flat)
    off = 0
    for I, O in zip(dims[:-1], dims[1:]):
        w = flat[..., off:off + I * O].reshape(flat.shape[:-1] + (O, I))
        out[..., off:off + I * O] = np.swapaxes(w, -1, -2).reshape(
            flat.shape[:-1] + (I * O,))
        off += I * O
        out[..., off:off + O] = flat[..., off:off + O]
        off += O
    assert off == flat.shape[-1]
    return out
