#!/usr/bin/env python3
"""The tail of a novelty-search generation alone: novelty of every member
against the archive, then fitness rows to the ranked fits `rf` that
es_grad_gather consumes, timed with device events on one GPU.

  default  torch cdist + topk in fp64 (novelty_batch), rows to the host, the
           numpy MultiObjectiveRanker, rf and ri uploaded: GpuEngine.step()
           without device_tail
  device   es_novelty_knn + es_rank_tail (tail.hip): device_tail=True

For every point both arms see the same behaviours, archive and rewards and
ALTERNATE (default, device, default, ...) after a warm-up. The end event is
recorded after rf is on the device, so the default arm's host ranking is
inside its window. Peak torch.cuda.max_memory_allocated is taken per arm.

The project's bar for a speed claim: the SLOWEST device run must lead the
FASTEST default run by more than three times the run-to-run spread (max - min
within an arm, the larger of the two).

  python tools/tail_bench.py
  python tools/tail_bench.py --members 2561 --archive 1024 --json out.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from es_pytorch_amd import ops  # noqa: E402
from es_pytorch_amd.utils.novelty import novelty_batch, novelty_knn  # noqa: E402
from es_pytorch_amd.utils.rankers import CenteredRanker, MultiObjectiveRanker  # noqa: E402

ARMS = ("default", "device")     # old -> new
W = 0.3


def rows_of(rew, nov, offs, pairs):
    """The (pairs, 5) fp64 rows of GpuEngine.step() for two objectives."""
    fits = torch.stack([rew, nov], dim=1)
    rows = torch.empty((pairs, 5), dtype=torch.float64, device=rew.device)
    rows[:, :2] = fits[:pairs].double()
    rows[:, 2:4] = fits[pairs:2 * pairs].double()
    rows[:, -1] = offs.double()
    return rows


def tail_default(behv, archive, rew, offs, pairs, k, ws):
    nov = novelty_batch(behv[:, :2], archive, k)
    all_rows = rows_of(rew, nov, offs, pairs).cpu().numpy()
    ranker = MultiObjectiveRanker(CenteredRanker(), W)
    ranker.rank(all_rows[:, :2], all_rows[:, 2:4], all_rows[:, -1])
    rf = torch.from_numpy(np.ascontiguousarray(ranker.ranked_fits,
                                               dtype=np.float32)).to(behv.device)
    ri = torch.from_numpy(np.ascontiguousarray(ranker.noise_inds,
                                               dtype=np.int64)).to(behv.device)
    return rf, ri


def tail_device(behv, archive, rew, offs, pairs, k, ws):
    nov = novelty_knn(behv, archive, k).float()
    rows = rows_of(rew, nov, offs, pairs)
    rf, ri, counts = ws
    ops.check(ops.hip().es_rank_tail(
        rf.data_ptr(), ri.data_ptr(), counts.data_ptr(), rows.data_ptr(), pairs, 2,
        float(np.float32(W)), float(np.float32(1.0 - W)), 0, 0,
        torch.cuda.current_stream().cuda_stream), "es_rank_tail")
    return rf, ri


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--members", type=int, nargs="+", default=[2561, 20481],
                   help="members on the rank (2 * pairs + 1)")
    p.add_argument("--archive", type=int, nargs="+", default=[16, 1024, 16384])
    p.add_argument("-k", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--runs", type=int, default=5, help="timed runs per arm")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--json", type=str, default=None, help="also write the rows here")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tail_bench needs a GPU: a CPU timing says nothing about this path")
    dev = torch.device("cuda", 0)
    fns = {"default": tail_default, "device": tail_device}

    out = []
    print(f"{'members':>8} {'archive':>8} {'arm':>8} {'tail_ms med':>11} {'min':>9} {'max':>9} "
          f"{'peak MB':>9}")
    for M in args.members:
        for N in args.archive:
            g = torch.Generator(device=dev).manual_seed(args.seed)
            pairs = (M - 1) // 2
            behv = torch.randn(M, 3, device=dev, generator=g) * 3.0
            archive = torch.randn(N, 2, device=dev, generator=g, dtype=torch.float64) * 3.0
            rew = torch.randn(M, device=dev, generator=g)
            offs = torch.randint(0, 1 << 30, (pairs,), device=dev, generator=g)
            ws = (torch.empty(pairs, dtype=torch.float32, device=dev),
                  torch.empty(pairs, dtype=torch.int64, device=dev),
                  torch.empty(4 * pairs, dtype=torch.int32, device=dev))
            runs = {a: [] for a in ARMS}
            peak = {a: 0 for a in ARMS}
            res = {}
            for it in range(args.warmup + args.runs):
                for a in ARMS:                  # alternate the arms
                    torch.cuda.synchronize(dev)
                    torch.cuda.reset_peak_memory_stats(dev)
                    base = torch.cuda.memory_allocated(dev)   # incl. library workspaces
                    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    e0.record()
                    rf, ri = fns[a](behv, archive, rew, offs, pairs, args.k, ws)
                    e1.record()
                    torch.cuda.synchronize(dev)
                    res[a] = (rf.cpu().numpy().copy(), ri.cpu().numpy().copy())
                    peak[a] = max(peak[a], torch.cuda.max_memory_allocated(dev) - base)
                    if it >= args.warmup:
                        runs[a].append(e0.elapsed_time(e1))
                    del rf, ri
            # faster and different is not faster: the novelty columns agree to
            # fp32 rounding, so ranks can differ only where two scores round apart
            same = float(np.mean(res["default"][0] == res["device"][0]))
            assert np.array_equal(res["default"][1], res["device"][1])
            for a in ARMS:
                t = np.array(runs[a])
                out.append({"members": M, "archive": N, "k": args.k, "arm": a,
                            "tail_ms": t.tolist(), "tail_ms_med": float(np.median(t)),
                            "peak_bytes": int(peak[a])})
                print(f"{M:>8} {N:>8} {a:>8} {np.median(t):>11.3f} {t.min():>9.3f} "
                      f"{t.max():>9.3f} {peak[a] / 2**20:>9.1f}", flush=True)
            d, n = (np.array(runs[a]) for a in ARMS)
            spread = max(d.max() - d.min(), n.max() - n.min())
            lead = d.min() - n.max()
            verdict = {"members": M, "archive": N, "lead_ms": float(lead),
                       "spread_ms": float(spread), "clears_bar": bool(lead > 3 * spread),
                       "speedup_med": float(np.median(d) / np.median(n)),
                       "rf_equal_fraction": same}
            out.append(verdict)
            print(f"      fastest default - slowest device = {lead:.3f} ms, spread "
                  f"{spread:.3f} ms, bar (3x spread) "
                  f"{'cleared' if verdict['clears_bar'] else 'NOT cleared'}, median "
                  f"speed-up {verdict['speedup_med']:.1f}x, rf equal on {same:.4f} of the "
                  f"pairs", flush=True)
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
