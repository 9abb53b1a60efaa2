#!/usr/bin/env python3
"""Record the REFERENCE's own fp32 perturbed forwards as a data fixture.

Run by hand (needs a checkout of the reference implementation; nothing in the
test suite does). Imports the reference with the stand-in modules of
``tools/make_ref_fixture.py``, builds a reference ``Policy`` around a reference
``FeedForward`` and, for a few small shapes, records what
``policy.pheno(+-noise)(ob, rs=None)`` returns — the reference's
``flat_params + std * noise`` and its fp32 torch forward — together with every
input needed to recompute it:

  flat     (n,)      float32  flat_params (state_dict order)
  obmean   (D,)      float32
  obstd    (D,)      float32  some entries 0.05 so that clipping occurs
  noise    (4, n)    float32  perturbation rows (flat order)
  obs      (7, D)    float32
  std      ()        float32  sigma
  ob_clip  ()        float32
  dims     (L+1,)    int32    layer widths
  out_pos  (4, 7, A) float32  reference outputs for +noise
  out_neg  (4, 7, A) float32  reference outputs for -noise

Data only, a few KB per file; tests/test_fp32_reference_fixture.py reads it.

Usage: python tools/make_ref_fp32_fixture.py <reference_root> [out_dir]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_ref_fixture import _EnvShim, install_stub_modules  # noqa: E402

# (ob_dim, hidden, ac_dim, sigma)
SHAPES = [(11, [16, 24], 3, 0.02), (11, [16, 24], 3, 0.05), (29, [64], 8, 0.02)]
N_NOISE, N_OBS, OB_CLIP = 4, 7, 5.0


def record(ref_policy_cls, ref_ff_cls, ref_adam_cls, D, hidden, A, sigma, seed):
    torch.manual_seed(seed)
    rng = np.random.RandomState(seed)
    nn = ref_ff_cls(list(hidden), torch.nn.Tanh(), _EnvShim(D, A), ac_std=0.01,
                    ob_clip=OB_CLIP)
    policy = ref_policy_cls(nn, sigma, ref_adam_cls(len(ref_policy_cls.get_flat(nn)), 0.01))
    # biases start at zero in the reference's init; make them count
    policy.flat_params += (0.05 * rng.randn(len(policy))).astype(np.float32)
    flat = policy.flat_params.astype(np.float32).copy()
    obmean = (rng.randn(D) * 0.3).astype(np.float32)
    obstd = (rng.rand(D) * 0.5 + 0.3).astype(np.float32)
    obstd[::4] = 0.05
    nn.set_ob_mean_std(obmean, obstd)
    noise = rng.randn(N_NOISE, len(policy)).astype(np.float32)
    z = rng.randn(N_OBS, D) * 1.5
    z[:, ::3] *= 4.0                      # some |z| beyond the clip
    obs = (obmean + obstd * z).astype(np.float32)
    outs = {1: [], -1: []}
    with torch.no_grad():
        for sign in (1, -1):
            for p in range(N_NOISE):
                module = policy.pheno(np.float32(sign) * noise[p])
                rows = [module(torch.from_numpy(obs[k]), rs=None).numpy().copy()
                        for k in range(N_OBS)]
                outs[sign].append(np.stack(rows))
    assert np.array_equal(policy.flat_params, flat), "pheno must not move flat_params"
    xn = (obs - obmean) / obstd
    assert (np.abs(xn) > OB_CLIP).any() and (np.abs(xn) < OB_CLIP).any()
    return dict(flat=flat, obmean=obmean, obstd=obstd, noise=noise, obs=obs,
                std=np.float32(sigma), ob_clip=np.float32(OB_CLIP),
                dims=np.array([D] + list(hidden) + [A], dtype=np.int32),
                out_pos=np.stack(outs[1]).astype(np.float32),
                out_neg=np.stack(outs[-1]).astype(np.float32))


def main(ref_root, out_dir="tests/golden/fp32_forward"):
    install_stub_modules()
    sys.path.insert(0, ref_root)
    from src.core.policy import Policy as RefPolicy
    from src.nn.nn import FeedForward as RefFeedForward
    from src.nn.optimizers import Adam as RefAdam

    os.makedirs(out_dir, exist_ok=True)
    for k, (D, hidden, A, sigma) in enumerate(SHAPES):
        rec = record(RefPolicy, RefFeedForward, RefAdam, D, hidden, A, sigma, 4321 + k)
        name = "d" + "_".join(str(v) for v in rec["dims"]) + f"_s{int(sigma * 1000):03d}.npz"
        np.savez(os.path.join(out_dir, name), **rec)
        print(f"wrote {out_dir}/{name}: n={rec['flat'].size} out={rec['out_pos'].shape}")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(*sys.argv[1:])
