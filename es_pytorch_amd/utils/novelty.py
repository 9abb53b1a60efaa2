"""Novelty-search support: behaviour archive + k-nearest-neighbour novelty.

Same math as the reference (``src/utils/novelty.py:9-18``): the archive is a
growing (N, d) array of behaviours; novelty = mean Euclidean distance to the
k nearest archive entries; new entries are produced on rank 0 and broadcast
(reference ``comm.scatter([b]*size)`` -> RCCL broadcast).

``novelty_batch`` is the population-engine version: novelty of B behaviours
against the archive in one torch cdist + topk (on device when the archive
tensor lives there) — SURVEY.md K8. ``novelty_knn`` is its device counterpart
in hand-written HIP (``ops/csrc/hip/tail.hip``): the same scores in fp64
without the (B, N) distance matrix.


PROVENANCE: novelty/update_archive reproduce the reference math
(src/utils/novelty.py); the batched on-device variants are original.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from es_pytorch_amd.parallel.comm import Comm


def update_archive(comm: Optional[Comm], behaviour: Sequence[float],
                   archive: Optional[np.ndarray]) -> np.ndarray:
    """Broadcast rank-0's new behaviour and append it (reference ``novelty.py:9-13``)."""
    if comm is not None:
        behaviour = comm.broadcast_obj(behaviour, src=0)
    behaviour = np.asarray(behaviour, dtype=np.float64)
    if archive is None:
        return np.array([behaviour])
    return np.concatenate((archive, [behaviour]))


def novelty(behaviour: np.ndarray, archive: np.ndarray, n: int) -> float:
    """Mean distance to the n nearest archive entries (reference ``novelty.py:16-18``)."""
    d = np.linalg.norm(np.asarray(archive, dtype=np.float64) -
                       np.asarray(behaviour, dtype=np.float64)[None, :], axis=1)
    k = min(n, len(d))
    return float(np.mean(np.partition(d, k - 1)[:k]))


def novelty_batch(behaviours: torch.Tensor, archive: torch.Tensor, n: int) -> torch.Tensor:
    """Novelty of (B, d) behaviours vs an (N, d) archive; stays on device.

    :returns: (B,) float32 novelty scores
    """
    d = torch.cdist(behaviours.to(archive.dtype), archive)  # (B, N)
    k = min(n, archive.shape[0])
    smallest, _ = torch.topk(d, k, dim=1, largest=False)
    return smallest.mean(dim=1).float()


def novelty_knn(behaviours: torch.Tensor, archive: torch.Tensor, n: int) -> torch.Tensor:
    """Novelty of B behaviours vs an (N, 2) archive by the fused kNN kernel
    (``es_novelty_knn``): each behaviour's n best squared distances stay in
    registers while the archive streams through LDS, so nothing of size B x N
    is ever written.

    :param behaviours: (B, >=2) float32 CUDA tensor; columns 0 and 1 are read.
        Rows may be strided (a view such as ``buf.view(M, eps, 3)[:, -1]``),
        the two columns of a row are adjacent.
    :param archive: (N, 2) contiguous float64 CUDA tensor, N >= 1
    :param n: neighbours, 1..32; min(n, N) are averaged
    :returns: (B,) float64 novelty scores
    """
    from es_pytorch_amd import ops
    if not (behaviours.is_cuda and archive.is_cuda):
        raise ValueError("novelty_knn runs on CUDA tensors only (novelty_batch "
                         "is the torch version)")
    if behaviours.dtype != torch.float32 or behaviours.dim() != 2 or \
            behaviours.shape[1] < 2 or behaviours.stride(1) != 1:
        raise ValueError("behaviours must be (B, >=2) float32 with adjacent columns")
    if archive.dtype != torch.float64 or archive.dim() != 2 or archive.shape[1] != 2 \
            or not archive.is_contiguous():
        raise ValueError("archive must be (N, 2) contiguous float64")
    B = behaviours.shape[0]
    out = torch.empty(B, dtype=torch.float64, device=archive.device)
    stride = behaviours.stride(0) if B > 1 else 0
    ops.check(ops.hip().es_novelty_knn(
        out.data_ptr(), behaviours.data_ptr(), stride, B, archive.data_ptr(),
        archive.shape[0], int(n), torch.cuda.current_stream(archive.device).cuda_stream),
        "es_novelty_knn")
    return out
