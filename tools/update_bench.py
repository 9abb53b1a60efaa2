#!/usr/bin/env python3
"""The update at the end of a generation alone: ranked fits and noise offsets
to the new theta, timed with device events on one GPU.

  default  es_grad_gather then es_adam_step: GpuEngine.step() without
           split_update
  split    es_grad_update (grad_update.hip), one launch whose grid also splits
           the population: split_update=True

For every point (net, pairs) both arms see the same table, offsets and fits and
ALTERNATE (default, split, default, ...) after a warm-up. A library without
es_grad_update (an earlier revision through ES_HIP_SO) runs the default arm
only.

The project's bar for a speed claim: the SLOWEST split run must lead the
FASTEST default run by more than three times the run-to-run spread (max - min
within an arm, the larger of the two).

  python tools/update_bench.py
  python tools/update_bench.py --pairs 2048 --table 50000000 --json out.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from es_pytorch_amd import ops  # noqa: E402

NETS = ([4, 32, 32, 1], [11, 32, 32, 3], [29, 64, 64, 8], [376, 256, 256, 17])
ADAM = (0.01, 0.9, 0.999, 1e-8)      # a, b1, b2, eps
L2 = 0.005


def n_params(dims):
    return sum((i + 1) * o for i, o in zip(dims[:-1], dims[1:]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pairs", type=int, nargs="+", default=[128, 512, 2048, 5120])
    p.add_argument("--table", type=int, default=250_000_000, help="floats in the table")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--runs", type=int, default=5, help="timed runs per arm")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--json", type=str, default=None, help="also write the rows here")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("update_bench needs a GPU: a CPU timing says nothing about this path")
    dev = torch.device("cuda", 0)
    lib = ops.hip()
    arms = ("default", "split") if hasattr(lib, "es_grad_update") else ("default",)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    table = torch.randn(args.table, device=dev, generator=gen)
    stream = torch.cuda.current_stream(dev).cuda_stream

    out = []
    print(f"{'net':>18} {'n_params':>8} {'pairs':>6} {'Y':>4} {'arm':>8} {'update_us med':>13} "
          f"{'min':>9} {'max':>9}")
    for dims in NETS:
        n = n_params(dims)
        for pairs in args.pairs:
            offs = torch.randint(0, args.table - n, (pairs,), device=dev, generator=gen)
            fits = torch.randn(pairs, device=dev, generator=gen)
            theta0 = torch.randn(n, device=dev, generator=gen)
            st = {a: [torch.empty(n, device=dev) for _ in range(4)] for a in arms}
            Y = 0
            if "split" in arms:
                y, floats = ctypes.c_int32(0), ctypes.c_int64(0)
                ops.check(lib.es_grad_update_plan(pairs, n, ctypes.byref(y),
                                                  ctypes.byref(floats)), "es_grad_update_plan")
                Y = y.value
                partials = torch.empty(floats.value, device=dev)
                ticket = torch.zeros((n + 255) // 256, dtype=torch.int32, device=dev)

            def default(theta, m, v, g):
                ops.check(lib.es_grad_gather(g.data_ptr(), table.data_ptr(), fits.data_ptr(),
                                             offs.data_ptr(), pairs, n, 0.0, stream),
                          "es_grad_gather")
                ops.check(lib.es_adam_step(theta.data_ptr(), m.data_ptr(), v.data_ptr(),
                                           g.data_ptr(), n, *ADAM, L2, 0.5 / pairs, stream),
                          "es_adam_step")

            def split(theta, m, v, g):
                ops.check(lib.es_grad_update(
                    theta.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(),
                    partials.data_ptr(), ticket.data_ptr(), table.data_ptr(), fits.data_ptr(),
                    offs.data_ptr(), pairs, n, 0.0, 0, *ADAM, L2, 0.5 / pairs, stream),
                    "es_grad_update")

            fns = {"default": default, "split": split}
            runs = {a: [] for a in arms}
            for it in range(args.warmup + args.runs):
                for a in arms:                  # alternate the arms
                    theta, m, v, g = st[a]
                    theta.copy_(theta0)
                    m.zero_()
                    v.zero_()
                    torch.cuda.synchronize(dev)
                    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    e0.record()
                    fns[a](theta, m, v, g)
                    e1.record()
                    torch.cuda.synchronize(dev)
                    if it >= args.warmup:
                        runs[a].append(1e3 * e0.elapsed_time(e1))
            for a in arms:
                t = np.array(runs[a])
                out.append({"dims": dims, "n_params": n, "pairs": pairs, "Y": Y, "arm": a,
                            "update_us": t.tolist(), "update_us_med": float(np.median(t))})
                print(f"{str(dims):>18} {n:>8} {pairs:>6} {Y:>4} {a:>8} {np.median(t):>13.1f} "
                      f"{t.min():>9.1f} {t.max():>9.1f}", flush=True)
            if "split" not in arms:
                continue
            # faster and different is not faster: the same update to fp32 rounding
            scale = float(st["default"][3].abs().max())
            gdiff = float((st["default"][3] - st["split"][3]).abs().max()) / scale
            assert gdiff < 1e-4, gdiff
            d, s = (np.array(runs[a]) for a in arms)
            spread = max(d.max() - d.min(), s.max() - s.min())
            lead = d.min() - s.max()
            verdict = {"dims": dims, "pairs": pairs, "lead_us": float(lead),
                       "spread_us": float(spread), "clears_bar": bool(lead > 3 * spread),
                       "speedup_med": float(np.median(d) / np.median(s)),
                       "g_max_rel_diff": gdiff}
            out.append(verdict)
            print(f"      fastest default - slowest split = {lead:.1f} us, spread "
                  f"{spread:.1f} us, bar (3x spread) "
                  f"{'cleared' if verdict['clears_bar'] else 'NOT cleared'}, median "
                  f"speed-up {verdict['speedup_med']:.2f}x", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
