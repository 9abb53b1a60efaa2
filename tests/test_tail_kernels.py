"""tail.hip against the host: es_novelty_knn against utils.novelty.novelty
(float64 numpy), es_rank_tail against the host rankers, bit for bit."""
import numpy as np
import pytest
import torch

from es_pytorch_amd import ops
from es_pytorch_amd.utils.novelty import novelty, novelty_knn
from es_pytorch_amd.utils.rankers import (CenteredRanker, DoublePositiveCenteredRanker,
                                          MultiObjectiveRanker)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, N, k): B on lane and block edges, N below / at k and on the wave-slice
# (256) and tile (1024) edges, k on each list length (4, 8, 16, 32) and across
KNN_CASES = [(1, 1, 1), (63, 255, 1), (65, 2, 3), (257, 3, 3), (63, 257, 3),
             (1, 9, 10), (257, 10, 10), (65, 1023, 10), (257, 2049, 10),
             (63, 15, 16), (65, 16, 16), (257, 1025, 16),
             (65, 16, 17), (63, 17, 17), (1, 2049, 17),
             (1, 31, 32), (257, 32, 32), (65, 1025, 32), (63, 2049, 32)]


def knn_inputs(B, N, k, cols):
    """A 5 x 5 integer-grid archive (duplicate rows, equal distances) and
    behaviours around it; behaviour 0 sits on archive row 0."""
    rng = np.random.default_rng(1000 * B + 10 * N + k)
    archive = rng.integers(0, 5, (N, 2)).astype(np.float64)
    behv = rng.uniform(-1, 5, (B, cols)).astype(np.float32)
    behv[0, :2] = archive[0]
    behv[B // 2, :2] = np.round(behv[B // 2, :2])      # on the grid: tied distances
    return archive, behv


@pytest.mark.parametrize("B,N,k", KNN_CASES)
def test_novelty_knn_matches_host(B, N, k):
    archive, behv = knn_inputs(B, N, k, 2)
    got = novelty_knn(torch.from_numpy(behv).to(DEV), torch.from_numpy(archive).to(DEV), k)
    want = [novelty(b.astype(np.float64), archive, k) for b in behv]
    assert got.dtype == torch.float64 and novelty(behv[0], archive, 1) == 0.0
    # <= 64 fp64 roundings (1.4e-14), with room for sqrt
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-12, atol=0)


def test_novelty_knn_strided_rows():
    """The (M, eps, 3) behaviour buffer's last-episode rows, stride 6, in place."""
    archive, behv = knn_inputs(65, 257, 10, 6)
    view = torch.from_numpy(behv).to(DEV).view(65, 2, 3)[:, -1]
    assert view.stride(0) == 6
    got = novelty_knn(view, torch.from_numpy(archive).to(DEV), 10)
    want = [novelty(b[3:5].astype(np.float64), archive, 10) for b in behv]
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("N,k", [(8, 0), (8, 33), (0, 3)])
def test_novelty_knn_rejects(N, k):
    buf = torch.zeros(16, 2, dtype=torch.float64, device=DEV)
    behv = torch.zeros(4, 2, dtype=torch.float32, device=DEV)
    assert ops.hip().es_novelty_knn(buf.data_ptr(), behv.data_ptr(), 2, 4,
                                    buf.data_ptr(), N, k, None) == -119


def rank_tail(rows, O, w, mode, j_split, launches=1):
    R = rows.shape[0]
    d_rows = torch.from_numpy(rows).to(DEV)
    rf = torch.empty(R, dtype=torch.float32, device=DEV)
    ri = torch.empty(R, dtype=torch.int64, device=DEV)
    counts = torch.full((2 * R * O,), 7, dtype=torch.int32, device=DEV)
    out = []
    for _ in range(launches):
        ops.check(ops.hip().es_rank_tail(
            rf.data_ptr(), ri.data_ptr(), counts.data_ptr(), d_rows.data_ptr(), R, O,
            float(np.float32(w)), float(np.float32(1.0 - w)), mode, j_split,
            torch.cuda.current_stream().cuda_stream), "es_rank_tail")
        out.append((rf.cpu().numpy(), ri.cpu().numpy()))
    return out


def host_rank(rows, O, w, mode):
    ranker = (CenteredRanker, DoublePositiveCenteredRanker)[mode]()
    if O == 2:
        ranker = MultiObjectiveRanker(ranker, w)
    ranker.rank(rows[:, :O], rows[:, O:2 * O], rows[:, -1])
    return ranker.ranked_fits.astype(np.float32), ranker.noise_inds.astype(np.int64)


@pytest.mark.parametrize("j_split", [0, 1, 3])
@pytest.mark.parametrize("O,mode,w", [(1, 0, 1.0), (1, 1, 1.0), (2, 0, 0.3), (2, 1, 0.3),
                                      (2, 1, 0.0), (2, 0, 1.0)])
@pytest.mark.parametrize("R", [1, 2, 127, 128, 129, 513, 2049])
def test_rank_tail_matches_host_ranker(R, O, mode, w, j_split):
    rng = np.random.default_rng(R + 10 * O + mode)
    rows = np.empty((R, 2 * O + 1))
    rows[:, :2 * O] = rng.choice([-2.0, -1.0, -0.0, 0.0, 1.0], (R, 2 * O))
    rows[:, -1] = rng.integers(0, 1 << 40, R)
    (rf, ri), (rf2, ri2) = rank_tail(rows, O, w, mode, j_split, launches=2)
    want_rf, want_ri = host_rank(rows, O, w, mode)
    assert rf.tobytes() == want_rf.tobytes()
    assert np.array_equal(ri, want_ri)
    assert rf2.tobytes() == rf.tobytes() and np.array_equal(ri2, ri)


def test_rank_tail_ranks_in_float64():
    """Fitnesses one 2^-40 apart: equal as float32, where index order would rank
    them, but not as float64."""
    rng = np.random.default_rng(40)
    rows = np.empty((129, 5))
    rows[:, :4] = 1.0 + rng.integers(0, 2, (129, 4)) * 2.0 ** -40
    rows[:, 0], rows[:, 2] = 1.0 + 2.0 ** -40, 1.0     # every + above every -
    rows[:, -1] = np.arange(129)
    assert (rows[:, 0].astype(np.float32) == rows[:, 2].astype(np.float32)).all()
    (rf, ri), = rank_tail(rows, 2, 0.3, 0, 0)
    want_rf, want_ri = host_rank(rows, 2, 0.3, 0)
    assert rf.tobytes() == want_rf.tobytes() and np.array_equal(ri, want_ri)
