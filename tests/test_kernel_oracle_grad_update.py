"""es_grad_update (grad_update.hip: the gather split over the population and
the Adam/SGD step in one launch) against the float64 oracle, bound 16 x E32.

n_pop cases per n_params: Y is the plan's split for that n_params at the
largest population here (1031); 4Y-1, 32Y and 32Y+1 are then fewer rows than
waves (at Y = 1; at a larger Y the plan for so few rows picks a smaller split,
which is the rule under test), one turn of the 8-row ring per wave, and one
turn plus a row. n_pop 1 and 2 leave waves without rows at every n_params.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.oracle64 import (ERR_FACTOR, adam_steps, fp32_error_scale, grad_gather,
                            max_ratio, quantized_table, sgd_steps)

pytestmark = pytest.mark.gpu

TABLE_N = 1_300_000
QSTD = 0.02
DEPTH = 8                                   # GU_DEPTH
ADAM = (0, 0.01, 0.9, 0.999, 1e-8)          # opt, a, b1, b2, eps
SGD = (1, 0.02, 0.9, 0.0, 0.0)              # opt, lr, momentum, -, -
L2, GSCALE = 0.005, 1.0 / 64.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def table(dev):
    t = np.random.RandomState(1234).randn(TABLE_N).astype(np.float32)
    return {"f32": t, "q": quantized_table(t, QSTD), "dev": torch.from_numpy(t).to(dev)}


def plan(n_pop, n):
    from es_pytorch_amd import ops
    y, floats = ctypes.c_int32(0), ctypes.c_int64(0)
    rc = ops.hip().es_grad_update_plan(n_pop, n, ctypes.byref(y), ctypes.byref(floats))
    assert rc == 0, rc
    return y.value, floats.value


def workspace(dev, n_pop, n):
    return (torch.empty(plan(n_pop, n)[1], dtype=torch.float32, device=dev),
            torch.zeros((n + 255) // 256, dtype=torch.int32, device=dev))


def launch(dev, table, offs, fits, n, qstd, hyper=ADAM, state=None, ws=None):
    """One launch on buffers 8 floats longer than n; returns g, theta, m, v."""
    from es_pytorch_amd import ops
    state = state or {k: np.zeros(n, np.float32) for k in ("theta", "m", "v")}
    buf = {k: torch.full((n + 8,), 7.0, dtype=torch.float32, device=dev)
           for k in ("g", "theta", "m", "v")}
    for k, x in state.items():
        buf[k][:n] = torch.from_numpy(x).to(dev)
    partials, ticket = ws or workspace(dev, len(offs), n)
    offs_d, fits_d = torch.from_numpy(offs).to(dev), torch.from_numpy(fits).to(dev)
    rc = ops.hip().es_grad_update(
        buf["theta"].data_ptr(), buf["m"].data_ptr(), buf["v"].data_ptr(),
        buf["g"].data_ptr(), partials.data_ptr(), ticket.data_ptr(), table["dev"].data_ptr(),
        fits_d.data_ptr(), offs_d.data_ptr(), len(offs), n, float(qstd), *hyper, L2, GSCALE,
        torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    assert int(ticket.abs().sum()) == 0, "a ticket was not put back"
    out = {k: b.cpu().numpy() for k, b in buf.items()}
    for k, x in out.items():
        assert (x[n:] == 7.0).all(), f"wrote past n_params in {k}"
    return {k: x[:n] for k, x in out.items()}


def problem(n, n_pop, seed, align=None):
    rng = np.random.RandomState(seed)
    offs = rng.randint(0, TABLE_N - n - 4, size=n_pop).astype(np.int64)
    if align is not None:                   # all 16-byte aligned rows, or all odd
        offs = offs // 4 * 4 + align
    return offs, rng.randn(n_pop).astype(np.float32)


def check_g(dev, table, n, n_pop, qstd, align=None):
    offs, fits = problem(n, n_pop, n + 7 * n_pop + int(qstd > 0), align)
    y64, e32 = fp32_error_scale(grad_gather, table["q"] if qstd > 0 else table["f32"],
                                offs, fits, n)
    r = max_ratio(launch(dev, table, offs, fits, n, qstd)["g"], y64, e32)
    print(f"ORACLE-RATIO grad_update g_n{n}_pop{n_pop}_q{int(qstd > 0)}_a{align} "
          f"Y={plan(n_pop, n)[0]} ratio={r:.2f} E32={e32:.3g}")
    assert r <= ERR_FACTOR, (r, e32)


@pytest.mark.parametrize("qstd", [0.0, QSTD])
@pytest.mark.parametrize("pop", ["1", "2", "4Y-1", "4YD", "4YD+1", "1031"])
@pytest.mark.parametrize("n", [1, 255, 257, 1539, 4097, 70001, 131073])
def test_g_matches_oracle(dev, table, n, pop, qstd):
    Y = plan(1031, n)[0]
    assert (Y == 1) == (n == 131073)   # 513 columns: no split, two staging tiles
    check_g(dev, table, n, {"1": 1, "2": 2, "4Y-1": 4 * Y - 1, "4YD": 4 * Y * DEPTH,
                            "4YD+1": 4 * Y * DEPTH + 1, "1031": 1031}[pop], qstd)


@pytest.mark.parametrize("align", [0, 1])
def test_g_aligned_and_odd_offsets(dev, table, align):
    check_g(dev, table, 1539, 1031, 0.0, align)


@pytest.mark.parametrize("hot", [0, 1030, 1031 // 32, 1031 // 32 + (1031 * 2 // 32 - 32) // 4])
def test_quantized_one_hot_exact(dev, table, hot):
    """The hot row first, last, first of block 1's slice and first of its wave
    1 (1031 rows at n = 1539 split 32 ways): g is that quantised row exactly."""
    n = 1539
    assert plan(1031, n)[0] == 32
    offs, _ = problem(n, 1031, hot)
    fits = np.zeros(1031, np.float32)
    fits[hot] = 1.0
    got = launch(dev, table, offs, fits, n, QSTD)["g"]
    want = table["q"][offs[hot]:offs[hot] + n]
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert not np.array_equal(want, table["f32"][offs[hot]:offs[hot] + n])


def oracle_step(hyper, state, g):
    """(y64, E32) of one optimizer step from `state` on the float32 g."""
    if hyper[0] == 0:
        return fp32_error_scale(adam_steps, state["theta"], state["m"], state["v"], g,
                                [hyper[1]], hyper[2], hyper[3], hyper[4], L2, GSCALE)
    return fp32_error_scale(sgd_steps, state["theta"], state["v"], g, 1, hyper[1], hyper[2],
                            L2, GSCALE)


def random_state(n, seed):
    rng = np.random.RandomState(seed)
    return {"theta": rng.randn(n).astype(np.float32),
            "m": (0.1 * rng.randn(n)).astype(np.float32),
            "v": (0.01 * rng.rand(n)).astype(np.float32)}


@pytest.mark.parametrize("hyper", [ADAM, SGD], ids=["adam", "sgd"])
@pytest.mark.parametrize("n", [1539, 4097])
def test_optimizer_and_ticket_reset(dev, table, n, hyper):
    """Two launches on one workspace, nothing cleared between them: after each,
    the state is the oracle's step from the previous state on that launch's own
    float32 g (which isolates the optimizer from the summation order)."""
    state, ws = random_state(n, n), workspace(dev, 300, n)
    for step in range(2):
        offs, fits = problem(n, 300, n + step)
        out = launch(dev, table, offs, fits, n, 0.0, hyper, state, ws)
        y64, e32 = oracle_step(hyper, state, out["g"])
        for k in y64:
            r = max_ratio(out[k], y64[k], e32[k])
            print(f"ORACLE-RATIO grad_update {'sgd' if hyper[0] else 'adam'}_{k}_n{n}"
                  f"_step{step} ratio={r:.2f} E32={e32[k]:.3g}")
            assert r <= ERR_FACTOR, (k, r)
        if hyper[0]:
            assert np.array_equal(out["m"], state["m"]), "SGD touched m"
        state = {k: out[k] for k in state}


def test_deterministic(dev, table):
    offs, fits = problem(1539, 1031, 5)
    a, b = (launch(dev, table, offs, fits, 1539, QSTD, ADAM, random_state(1539, 9))
            for _ in range(2))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("n_pop,n,opt", [(0, 16, 0), (16, 0, 0), (16, 16, 2)])
def test_error_code(dev, n_pop, n, opt):
    from es_pytorch_amd import ops
    z = torch.zeros(512, dtype=torch.float32, device=dev)
    zi = torch.zeros(512, dtype=torch.int64, device=dev)
    rc = ops.hip().es_grad_update(
        z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), zi.data_ptr(),
        z.data_ptr(), z.data_ptr(), zi.data_ptr(), n_pop, n, 0.0, opt, 0.01, 0.9, 0.999, 1e-8,
        0.0, 1.0, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == -120
