"""GpuEngine(split_update=True): a Hopper generation whose gather and optimizer
step are the one es_grad_update launch, beside the same engine with the mode
off; both gradients against the float64 gather, the split engine's step against
the float64 optimizer on its own gradient. The engine builder is
tests/test_fp32_engine.py's."""
import numpy as np
import pytest
import torch

from tests.oracle64 import (ERR_FACTOR, adam_steps, fp32_error_scale, grad_gather, max_ratio,
                            sgd_steps)
from tests.test_fp32_engine import _engine

PPG = 32


def make_engine(dev, **kw):
    return _engine(dev, "Hopper-v3", [32, 32], PPG, 1, 10, "bf16", **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("optim", ["adam", "sgd"])
def test_generation_with_split_update(optim):
    from es_pytorch_amd.nn.optimizers import SGD
    from es_pytorch_amd.utils.rankers import CenteredRanker
    dev = torch.device("cuda", 0)
    engines = {False: make_engine(dev), True: make_engine(dev, split_update=True)}
    four = dict(engines[True].numerics)
    assert four.pop("update") == "split" and len(four) == 4
    assert engines[False].numerics["update"] == "default"
    assert engines[False].numerics == four          # the key is not stored
    rankers, before = {}, {}
    for on, eng in engines.items():
        if optim == "sgd":
            eng.policy.optim = SGD(eng.n, 0.02)
        before[on] = {k: getattr(eng, k).cpu().numpy().copy() for k in ("theta", "m", "v")}
        rankers[on] = CenteredRanker()
        eng.step(rankers[on])
    # the same rollout kernels on the same inputs
    assert np.array_equal(rankers[True].ranked_fits, rankers[False].ranked_fits)
    assert np.array_equal(rankers[True].noise_inds, rankers[False].noise_inds)

    eng, n = engines[True], engines[True].n
    fits = np.asarray(rankers[True].ranked_fits, np.float32)
    inds = np.asarray(rankers[True].noise_inds, np.int64)
    y64, e32 = fp32_error_scale(grad_gather, eng.nt.noise.cpu().numpy(), inds, fits, n)
    for on, e in engines.items():
        r = max_ratio(e.grad.cpu().numpy(), y64, e32)
        print(f"ORACLE-RATIO split_update {optim} grad split={on} ratio={r:.2f} E32={e32:.3g}")
        assert r <= ERR_FACTOR, (on, r)

    opt, g, b = eng.policy.optim, eng.grad.cpu().numpy(), before[True]
    assert opt.t == 1
    if optim == "adam":
        a = opt.lr * np.sqrt(1 - opt.beta2) / (1 - opt.beta1)
        o64, oe = fp32_error_scale(adam_steps, b["theta"], b["m"], b["v"], g, [a], opt.beta1,
                                   opt.beta2, opt.epsilon, 0.005, 1.0 / PPG)
    else:
        o64, oe = fp32_error_scale(sgd_steps, b["theta"], b["v"], g, 1, opt.lr, opt.momentum,
                                   0.005, 1.0 / PPG)
    for k in o64:
        r = max_ratio(getattr(eng, k).cpu().numpy(), o64[k], oe[k])
        print(f"ORACLE-RATIO split_update {optim} {k} ratio={r:.2f} E32={oe[k]:.3g}")
        assert r <= ERR_FACTOR, (k, r)
    assert not np.array_equal(eng.theta.cpu().numpy(), b["theta"])


def test_split_update_rejections_cpu():
    cpu = torch.device("cpu")
    assert not make_engine(cpu).split_update                   # default off
    for kw in (dict(split_update=1), dict(general={"split_update": "yes"})):
        with pytest.raises(ValueError, match="split_update must be true or false"):
            make_engine(cpu, **kw)
    with pytest.raises(ValueError, match="needs a GPU engine"):
        make_engine(cpu, split_update=True)


@pytest.mark.gpu
def test_split_update_needs_the_symbol(monkeypatch):
    from es_pytorch_amd import ops
    from es_pytorch_amd.nn.optimizers import SimpleES
    from es_pytorch_amd.utils.rankers import CenteredRanker
    dev = torch.device("cuda", 0)
    assert make_engine(dev, general={"split_update": True}).split_update
    eng = make_engine(dev, split_update=True)
    with pytest.warns(UserWarning):
        eng.policy.optim = SimpleES(eng.n, 0.01)
    with pytest.raises(TypeError, match="supports Adam/SGD"):
        eng.step(CenteredRanker())
    # a library of an earlier revision: no fallback to the two launches
    real = ops.hip()
    old = type("OldLib", (), {"__getattr__": lambda self, k: getattr(real, k)
                              if "grad_update" not in k else object.__getattribute__(self, k)})()
    monkeypatch.setattr(ops, "hip", lambda: old)
    with pytest.raises(RuntimeError, match="es_grad_update"):
        make_engine(dev, split_update=True)
