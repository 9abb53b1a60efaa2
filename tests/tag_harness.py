"""What the PursuitTag kernel tests share (tests/test_kernel_oracle_tag*.py;
the engine tests take MARGIN_MIN): the start positions and the fp32 blob of a
case, device copies of a case with a NaN guard row behind every state buffer,
the argument list of the per-game entry points, and the comparison against the
float64 oracle (tests/oracle64_tag.py): ``|kernel - oracle64| <= 16 * E32`` per
float state buffer, ``steps`` and ``alive`` exact.
"""
import numpy as np
import torch

from tests.oracle64 import ERR_FACTOR, max_ratio, n_params
from tests.oracle64_tag import TAG_KEYS
from tests.test_kernel_oracle_mlp import bf16_tensor

MARGIN_MIN = 1e-3                         # no oracle game this close to d == 0.3
N_CLOSE = 4                               # games 0..3 start close
CLOSE_DIST = (0.2, 0.4, 0.6, 0.8)         # runner's distance from the chaser
FLOAT_KEYS = ("p", "v", "rew_total", "ob_sum", "ob_sumsq")
NOISE = dict(seed=20240607, ac_std=(0.05, 0.05), noiseless_from=8)


def make_starts(rng, B):
    """p (B, 2, 2): games 0..3 with the runner CLOSE_DIST from the chaser in a
    random direction, the others at least 1.5 apart, all within +-2.5."""
    p = np.zeros((B, 2, 2), dtype=np.float32)
    for b in range(B):
        while True:
            c = rng.uniform(-2.0, 2.0, size=2)
            if b < N_CLOSE:
                th = rng.uniform(0, 2 * np.pi)
                r = c + CLOSE_DIST[b] * np.array([np.cos(th), np.sin(th)])
            else:
                r = rng.uniform(-2.5, 2.5, size=2)
            if np.abs(r).max() <= 2.5 and (b < N_CLOSE or np.linalg.norm(r - c) >= 1.5):
                break
        p[b, 0], p[b, 1] = c, r
    return p


def make_net_f32(rng, dims, rows, stride_pad=0):
    """make_net's blob (rows + 1 rows, the same draws and scales) with the
    float32 values kept as they are; returns (float32 array, stride)."""
    n = n_params(dims)
    stride = (n + 7) // 8 * 8 + stride_pad
    w = np.zeros((rows + 1, stride), dtype=np.float32)
    off = 0
    for I, O in zip(dims[:-1], dims[1:]):
        w[:, off:off + I * O] = rng.randn(rows + 1, I * O) * (0.7 / np.sqrt(I))
        off += I * O
        w[:, off:off + O] = rng.randn(rows + 1, O) * 0.1
        off += O
    return w, stride


class DeviceGame:
    """Device copies of a case: state with one NaN guard row, both nets (bf16
    blobs from ``wbits``). launch() goes to es_tag_episode; a subclass for
    another per-game entry point overrides entry()."""

    def __init__(self, dev, c, noise=None):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.dev, self.B = dev, c["B"]
        self.state = {}
        for k in TAG_KEYS:
            a = np.asarray(c["state"][k])
            g = np.full((1,) + a.shape[1:], np.nan, dtype=a.dtype)
            self.state[k] = t(np.concatenate([a, g], axis=0))
        self.nets = []
        for n in c["dev_nets"]:
            self.nets.append(dict(w=bf16_tensor(n["wbits"], dev), mean=t(n["obmean"]),
                                  std=t(n["obstd"]), stride=n["stride"],
                                  dims=np.array(n["dims"], dtype=np.int32),
                                  clip=n["ob_clip"]))
        self.seed = self.acstd = None
        self.noiseless_from = 0
        if noise is not None:
            self.seed = t(np.array([noise["seed"]], np.int64))
            self.acstd = [t(np.array([s], np.float32)) for s in noise["ac_std"]]
            self.noiseless_from = noise["noiseless_from"]

    def use_f32_blobs(self, c):
        """Replace the bf16 blobs by the case's float32 ones (``w32``)."""
        for net, n in zip(self.nets, c["dev_nets"]):
            net["w"] = torch.from_numpy(np.ascontiguousarray(n["w32"])).to(self.dev)
            assert net["w"].dtype == torch.float32

    def args(self, n_steps, salt_base=0, n_games=None, n_agents=2, ob_dim=8):
        """The argument list of the per-game entry points."""
        s, (n0, n1) = self.state, self.nets
        ptr = lambda x: x.data_ptr() if x is not None else None
        return (
            s["p"].data_ptr(), s["v"].data_ptr(), s["alive"].data_ptr(),
            s["steps"].data_ptr(), s["rew_total"].data_ptr(), s["ob_sum"].data_ptr(),
            s["ob_sumsq"].data_ptr(), n0["w"].data_ptr(), n1["w"].data_ptr(),
            n0["mean"].data_ptr(), n1["mean"].data_ptr(), n0["std"].data_ptr(),
            n1["std"].data_ptr(), n0["dims"].ctypes.data, len(n0["dims"]),
            n1["dims"].ctypes.data, len(n1["dims"]), n0["stride"], n1["stride"],
            n0["clip"], n1["clip"], ptr(self.acstd[0] if self.acstd else None),
            ptr(self.acstd[1] if self.acstd else None), ptr(self.seed), salt_base,
            n_agents, ob_dim, self.B if n_games is None else n_games, n_steps, 1,
            self.noiseless_from, torch.cuda.current_stream(self.dev).cuda_stream)

    def entry(self):
        from es_pytorch_amd import ops
        return ops.hip().es_tag_episode

    def launch(self, *a, **kw):
        rc = self.entry()(*self.args(*a, **kw))
        torch.cuda.synchronize(self.dev)
        return rc

    def read(self):
        """Host copy of the B games; the guard row must still be NaN."""
        out = {}
        for k, v in self.state.items():
            a = v.cpu().numpy()
            assert np.isnan(a[self.B:]).all(), f"{k}: guard row written"
            out[k] = a[:self.B]
        return out


def check(name, got, y64, e32, games=slice(None)):
    assert np.array_equal(got["steps"][games], y64["steps"][games]), name
    assert np.array_equal(got["alive"][games], y64["alive"][games]), name
    worst = (0.0, "")
    for k in FLOAT_KEYS:
        assert np.isfinite(got[k]).all(), (name, k)
        r = max_ratio(got[k][games], y64[k][games], e32[k])
        print(f"ORACLE-RATIO tag {name} {k} ratio={r:.2f} E32={e32[k]:.3g}")
        worst = max(worst, (r, k))
    print(f"ORACLE-RATIO tag {name} worst ratio={worst[0]:.2f} ({worst[1]})")
    for k in FLOAT_KEYS:
        r = max_ratio(got[k][games], y64[k][games], e32[k])
        assert r <= ERR_FACTOR, (name, k, r, e32[k])
