"""Float64 numpy oracle for the HIP kernels.

Plain numpy, float64 maths, no torch ops and no code shared with
``es_pytorch_amd``: every formula below is written out from the documented
semantics (``envs/locomotion.py``, ``GpuEngine._step_body``, the layout notes
at the top of ``pheno.hip``), so a bug in the kernels' shared device code
cannot hide in both arms of a comparison. The random numbers are restated
too: Philox4x32-10 is written out from the paper and checked against its
published known-answer vectors (tests/test_oracle64_noise_cpu.py).

Every maths function takes a ``dtype``. ``float64`` is the oracle;
``float32`` re-runs the SAME natural-order evaluation in single precision and
``fp32_error_scale`` turns the difference into the per-buffer error scale
``E32`` that the GPU tests assert against (``|kernel - oracle64| <= 16 E32``).
Inputs (weights, observations, scalars) are float32/bf16/e4m3 VALUES and are
taken exactly; scalar parameters are rounded to float32 first because that is
what the kernels receive.
"""
import numpy as np

ERR_FACTOR = 16.0          # |kernel - oracle64| <= ERR_FACTOR * E32
_F32_EPS_FLOOR = 2.0 ** -24


# --------------------------------------------------------------------- codecs
def bf16_bits_to_f64(bits):
    """uint16 bf16 bit patterns -> float64 (exact)."""
    b = np.asarray(bits).astype(np.uint32) << np.uint32(16)
    return b.view(np.float32).astype(np.float64)


def f32_to_bf16_bits(x):
    """float32 -> bf16 bit patterns, round-to-nearest-even (finite inputs)."""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
    u = u.astype(np.uint64)
    keep = u >> np.uint64(16)
    rest = u & np.uint64(0xFFFF)
    up = (rest > 0x8000) | ((rest == 0x8000) & ((keep & np.uint64(1)) == 1))
    return (keep + up.astype(np.uint64)).astype(np.uint16)


def e4m3_byte_to_f64(b):
    """OCP e4m3fn byte -> float64 (0x7F / 0xFF are NaN)."""
    b = np.asarray(b).astype(np.int64)
    sign = 1.0 - 2.0 * ((b >> 7) & 1)
    ex = (b >> 3) & 15
    man = (b & 7).astype(np.float64)
    sub = man * 2.0 ** -9                                # exponent field 0
    nrm = (8.0 + man) * np.exp2((ex - 10).astype(np.float64))
    v = np.where(ex == 0, sub, nrm)
    v = np.where((ex == 15) & ((b & 7) == 7), np.nan, v)
    return sign * v


def f32_to_e4m3_byte(x):
    """float32 -> OCP e4m3fn byte, RNE with subnormals. Magnitudes that round
    above 448 (the largest finite value) give the NaN byte, like the torch
    cast; NaN in gives NaN out."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    a = np.abs(x)
    sign = (np.signbit(x).astype(np.int64)) << 7
    with np.errstate(divide="ignore", invalid="ignore"):
        _, e = np.frexp(a)                    # a = m * 2^e, m in [0.5, 1)
    e = e.astype(np.int64) - 1                # a in [2^e, 2^(e+1))
    e = np.maximum(e, -6)                     # subnormals share 2^-6's quantum
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(a * np.exp2((3 - e).astype(np.float64)))  # units of 2^(e-3)
    # normal: q in [8, 16]; subnormal: q in [0, 8]
    carry = q >= 16
    e = np.where(carry, e + 1, e)
    q = np.where(carry, 8.0, q)
    with np.errstate(invalid="ignore"):
        qi = np.where(np.isfinite(q), q, 0).astype(np.int64)
    is_sub = qi < 8
    byte = np.where(is_sub, qi, ((e + 7) << 3) | (qi - 8))
    over = ~np.isfinite(a) | (e > 8) | ((e == 8) & (qi - 8 >= 7))
    byte = np.where(over, 0x7F, byte)
    return (byte | sign).astype(np.uint8)


def e4m3_roundtrip_f32(x):
    """decode(encode(float32 x)) as float32."""
    return e4m3_byte_to_f64(f32_to_e4m3_byte(x)).astype(np.float32)


# --------------------------------------------------------------------- layout
def layer_offsets(dims):
    """Forward-layout blob: per layer W^T (I x O, row-major) then b (O).
    Returns ([(woff, boff, I, O)], n)."""
    out, off = [], 0
    for I, O in zip(dims[:-1], dims[1:]):
        out.append((off, off + I * O, I, O))
        off += I * O + O
    return out, off


def n_params(dims):
    return layer_offsets(dims)[1]


def layer_is_octet_tiled(woff, O):
    """Layers the kernels walk in 8-wide output octets."""
    return O % 8 == 0 and O <= 2048 and woff % 8 == 0


def fp8_byte_position(dims):
    """pos[t] = byte at which forward-layout element t lives in an fp8 row.

    pheno.hip: in an octet-tiled layer the weight rows are stored two at a
    time — for each row pair, for each output octet, the 8 bytes of the even
    row then the 8 bytes of the odd row. With an odd number of input rows the
    first row stays in plain order and pairing starts at row 1. Every other
    element (other layers, all biases) keeps its own index.
    """
    layers, n = layer_offsets(dims)
    src_of_byte = np.arange(n, dtype=np.int64)
    for woff, boff, I, O in layers:
        if not layer_is_octet_tiled(woff, O):
            continue
        first = I % 2
        pairs = (I - first) // 2
        start = woff + first * O
        elems = np.arange(start, start + 2 * pairs * O, dtype=np.int64)
        # element order is (pair, row-in-pair, octet, lane); byte order swaps
        # the two middle axes
        grid = elems.reshape(pairs, 2, O // 8, 8)
        src_of_byte[start:start + 2 * pairs * O] = grid.transpose(0, 2, 1, 3).reshape(-1)
    pos = np.empty(n, dtype=np.int64)
    pos[src_of_byte] = np.arange(n, dtype=np.int64)
    return pos


# ---------------------------------------------------------------------- noise
_U32 = np.uint64(0xFFFFFFFF)
_SH32 = np.uint64(32)
PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))     # round multipliers
PHILOX_W = (np.uint64(0x9E3779B9), np.uint64(0xBB67AE85))     # key bumps
NOISE_TAG = 0x6573616D                                        # counter word 3
ACTION_STREAM = 0xAC


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11; Random123), written
    out from the paper: counter = 4 words, key = 2 words, each a scalar or an
    array of 32-bit values (they broadcast). Returns the 4 output words as
    uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(w, dtype=np.uint64) & _U32 for w in counter)
    k0, k1 = (np.asarray(w, dtype=np.uint64) & _U32 for w in key)
    for _ in range(10):
        p0 = PHILOX_M[0] * c0            # 32 x 32 -> 64 bits, no overflow
        p1 = PHILOX_M[1] * c2
        c0, c1, c2, c3 = ((p1 >> _SH32) ^ c1 ^ k0, p1 & _U32,
                          (p0 >> _SH32) ^ c3 ^ k1, p0 & _U32)
        k0 = (k0 + PHILOX_W[0]) & _U32
        k1 = (k1 + PHILOX_W[1]) & _U32
    return c0, c1, c2, c3


def normal4(g, seed, stream, dtype=np.float64):
    """The four standard normals of group(s) `g` under (seed, stream).

    Counter (g lo, g hi, stream, NOISE_TAG), key (seed lo, seed hi). The
    uniforms are float32 values and their roundings are part of the contract:
    u1, u3 = (float32(word) + 1) * 2^-32 in (0, 1] from words 0 and 2,
    u2, u4 = float32(word) * 2^-32 in [0, 1] from words 1 and 3 (the top 128
    words round up to 2^32, so 1.0 is reached). Box-Muller in `dtype` with the
    float32 value of 2*pi: (r1 cos, r1 sin, r2 cos, r2 sin), r = sqrt(-2 log u).
    Returns an array of shape g.shape + (4,)."""
    g = np.asarray(g, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    w = philox4x32_10((g & _U32, g >> _SH32, int(stream) & 0xFFFFFFFF, NOISE_TAG),
                      (seed & 0xFFFFFFFF, seed >> 32))
    w = [np.broadcast_to(x, g.shape).astype(np.float32) for x in w]   # one rounding
    scale = np.float32(2.0 ** -32)
    one = np.float32(1.0)
    u1, u3 = (w[0] + one) * scale, (w[2] + one) * scale
    u2, u4 = w[1] * scale, w[3] * scale
    two_pi = dtype(np.float32(6.2831853071795864769))
    r1 = np.sqrt(dtype(-2.0) * np.log(u1.astype(dtype)))
    r2 = np.sqrt(dtype(-2.0) * np.log(u3.astype(dtype)))
    t1 = two_pi * u2.astype(dtype)
    t2 = two_pi * u4.astype(dtype)
    return np.stack([r1 * np.cos(t1), r1 * np.sin(t1), r2 * np.cos(t2), r2 * np.sin(t2)],
                    axis=-1)


def noise_table(n, seed, stream, dtype=np.float64):
    """Noise table of n elements: element i is component i & 3 of group i >> 2."""
    groups = np.arange((int(n) + 3) // 4, dtype=np.uint64)
    return normal4(groups, seed, stream, dtype).reshape(-1)[:int(n)]


def action_noise(seed, ctr, dtype=np.float64):
    """Action-noise draw(s) at counter(s) `ctr`: component 0 of the group
    `ctr` of stream ACTION_STREAM."""
    return normal4(ctr, seed, ACTION_STREAM, dtype)[..., 0]


def action_draws(seed, members, width, cols, dtype=np.float64):
    """z[k, d] = action_noise(seed, members[k] * width + d) for d < cols: the
    draws of absolute slots `members` of a net whose output is `width` wide."""
    ctr = np.asarray(members, dtype=np.uint64)[:, None] * np.uint64(width) + \
        np.arange(cols, dtype=np.uint64)[None, :]
    return action_noise(seed, ctr, dtype)


def noise_seed(noise):
    """Key of a launch: seed_dev + salt in 64-bit arithmetic, or the salt
    alone when there is no seed_dev (seed None)."""
    base = 0 if noise["seed"] is None else int(noise["seed"])
    return (base + int(noise["salt"])) & (2 ** 64 - 1)


# -------------------------------------------------------------------- forward
def _act(v, dtype):
    return np.tanh(v.astype(dtype, copy=False))


def mlp_forward(dims, weight_row, x, act_final=1, dtype=np.float64):
    """MLP forward on forward-layout weights.

    weight_row: (n,) or (B, n) weight VALUES (bias included); x: (D,) or
    (B, D). Accumulates over the input index in ascending order in `dtype`.
    Returns (B, dims[-1]) (or 1-D if both inputs were 1-D).
    """
    w = np.asarray(weight_row)
    x = np.asarray(x)
    one = w.ndim == 1 and x.ndim == 1
    w = np.atleast_2d(w).astype(dtype)
    h = np.atleast_2d(x).astype(dtype)
    if w.shape[0] == 1 and h.shape[0] > 1:
        w = np.broadcast_to(w, (h.shape[0], w.shape[1]))
    layers, n = layer_offsets(dims)
    assert w.shape[1] >= n and h.shape[1] == dims[0]
    for li, (woff, boff, I, O) in enumerate(layers):
        Wt = w[:, woff:boff].reshape(-1, I, O)
        acc = np.zeros((h.shape[0], O), dtype=dtype)
        for i in range(I):
            acc = acc + h[:, i:i + 1] * Wt[:, i, :]
        acc = acc + w[:, boff:boff + O]
        h = _act(acc, dtype) if (li < len(layers) - 1 or act_final) else acc
    return h[0] if one else h


def policy_actions(dims, weight_rows, obs, obmean, obstd, ob_clip, members=None,
                   eps=1, wrow0=0, act_final=1, act_mode=0, bins=0, alow=None,
                   arange=None, loco=False, dtype=np.float64, noise=None):
    """Actions of evaluation slots `members` (default: every row of obs).

    obs[k] is the observation of slot members[k]; slot b uses weight row
    b // eps - wrow0. Decode: act_mode 2 -> outputs 1.. (output 0 is the std),
    act_mode 3 -> first half, bins > 1 -> per-dim argmax over `bins` logits
    mapped to alow + arange * j/(bins-1) (or to [-1, 1] when loco=True), else
    the raw outputs.

    noise: None (noise off) or a dict of seed (None: no seed_dev), salt,
    ac_std and noiseless_from. Slots b < noiseless_from get
    z = action_noise(seed + salt, b * odim + d), odim the net's output width:
    the raw decode adds ac_std * z iff ac_std != 0, mode 2 adds out[0] * z and
    mode 3 |out[adim + d]| * z iff that std != 0, whatever ac_std is; the
    binned decode never draws. The actions are returned unclamped.
    Returns (actions, net_outputs).
    """
    obs = np.asarray(obs)
    nb = obs.shape[0]
    members = np.arange(nb) if members is None else np.asarray(members)
    rows = members // eps - wrow0
    w = np.asarray(weight_rows)[rows]
    clip = dtype(np.float32(ob_clip))
    xn = (obs.astype(dtype) - np.asarray(obmean).astype(dtype)) / \
        np.asarray(obstd).astype(dtype)
    xn = np.minimum(np.maximum(xn, -clip), clip)
    out = mlp_forward(dims, w, xn, act_final, dtype)
    odim = out.shape[1]
    noisy = None
    if noise is not None:
        noisy = (members < int(noise["noiseless_from"]))[:, None]
    if act_mode in (2, 3):
        if act_mode == 2:
            a, std = out[:, 1:].copy(), out[:, :1]
        else:
            a, std = out[:, :odim // 2].copy(), np.abs(out[:, odim // 2:2 * (odim // 2)])
        if noisy is not None and noisy.any():
            z = action_draws(noise_seed(noise), members, odim, a.shape[1], dtype)
            a = np.where(noisy & (std != 0), a + std * z, a)
        return a, out
    if bins and bins > 1:
        adim = out.shape[1] // bins
        best = out.reshape(nb, adim, bins).argmax(axis=2).astype(dtype)
        frac = best / dtype(bins - 1)
        if loco:
            return dtype(-1.0) + dtype(2.0) * frac, out
        return np.asarray(alow).astype(dtype) + np.asarray(arange).astype(dtype) * frac, out
    a = out.copy()
    if noisy is not None and noisy.any():
        ac_std = dtype(np.float32(noise["ac_std"]))
        if ac_std != 0:
            z = action_draws(noise_seed(noise), members, odim, odim, dtype)
            a = np.where(noisy, a + ac_std * z, a)
    return a, out


def top2_logit_gap(net_out, bins):
    """Smallest gap between the best and second-best logit of any binned dim."""
    o = np.asarray(net_out, dtype=np.float64)
    o = np.sort(o.reshape(o.shape[0], -1, bins), axis=2)
    return float((o[..., -1] - o[..., -2]).min())


# ------------------------------------------------------------------- env step
STATE_KEYS = ("s", "pos", "alive", "rew_total", "member_steps", "behv", "mo_sum",
              "mo_sumsq")


def copy_state(state):
    return {k: (None if v is None else np.array(v, copy=True)) for k, v in state.items()}


def loco_obs(state, goal_flag, dtype=np.float64):
    s = state["s"].astype(dtype)
    if not goal_flag:
        return s
    rel = (state["goal"].astype(dtype) - state["pos"][:, :2].astype(dtype)) * \
        dtype(np.float32(0.1))
    return np.concatenate([s, rel], axis=1)


def loco_step(state, env, policy, members=None, dtype=np.float64, noise=None,
              salt_base=0):
    """One env step for evaluation slots `members` (default all).

    state: dict of (B, ...) arrays — s (B,S), pos (B,3), goal (B,2) or None,
    alive, rew_total, member_steps (B,), behv (B,3), mo_sum, mo_sumsq (B,D).
    env: dict — A (S,S) VALUES of the bf16 matrix, B (Adim,S), b0, wv, wy, wh
    (S,), wa (Adim,), leak, ctrl, alive_bonus, fall_thr, dt, terminate, goal.
    policy: kwargs of policy_actions except obs/members/loco/dtype.
    noise: None or a dict of seed, ac_std and noiseless_from (see
    policy_actions); the step draws with salt salt_base + 1, so salt_base =
    s - 1 reproduces a per-step launch with salt s.
    Returns (new_state, info); rows outside `members` are returned unchanged.
    info holds h, the clamped actions, the actions before the clamp and the
    net outputs of the stepped slots.
    """
    f = lambda v: dtype(np.float32(v))
    B = state["s"].shape[0]
    members = np.arange(B) if members is None else np.asarray(members)
    g = int(env["goal"])
    st = {k: (None if state[k] is None else state[k].astype(dtype)) for k in state}
    sub = {k: (None if st[k] is None else st[k][members]) for k in st}
    S = sub["s"].shape[1]

    obs = loco_obs(sub, g, dtype)
    if noise is not None:
        noise = dict(noise, salt=int(salt_base) + 1)
    act, net = policy_actions(obs=obs, members=members, loco=True, dtype=dtype,
                              noise=noise, **policy)
    a = np.minimum(np.maximum(act, dtype(-1.0)), dtype(1.0))

    A = np.asarray(env["A"]).astype(dtype)
    Bm = np.asarray(env["B"]).astype(dtype)
    s = sub["s"]
    pre = np.zeros_like(s)
    for i in range(S):
        pre = pre + s[:, i:i + 1] * A[i:i + 1, :]
    pre = pre + np.asarray(env["b0"]).astype(dtype)
    for k in range(a.shape[1]):
        pre = pre + a[:, k:k + 1] * Bm[k:k + 1, :]
    leak = f(env["leak"])
    sn = (dtype(1.0) - leak) * s + leak * np.tanh(pre)

    def dot(m, v):
        v = np.asarray(v).astype(dtype)
        acc = np.zeros(m.shape[0], dtype=dtype)
        for i in range(m.shape[1]):
            acc = acc + m[:, i] * v[i]
        return acc

    vfwd = dot(sn, env["wv"]) + dot(dtype(0.5) * a, env["wa"])
    vy = dot(sn, env["wy"])
    h = dot(sn, env["wh"])
    asq = dot(a * a, np.ones(a.shape[1]))
    pos = sub["pos"]
    if g:
        rx = sub["goal"][:, 0] - pos[:, 0]
        ry = sub["goal"][:, 1] - pos[:, 1]
        inv = dtype(1.0) / (np.sqrt(rx * rx + ry * ry) + f(1e-6))
        rew = vfwd * rx * inv + vy * ry * inv - f(env["ctrl"]) * asq + f(env["alive_bonus"])
    else:
        rew = vfwd - f(env["ctrl"]) * asq + f(env["alive_bonus"])
    npos = np.stack([pos[:, 0] + f(env["dt"]) * vfwd, pos[:, 1] + f(env["dt"]) * vy, h],
                    axis=1)
    done = (h < f(env["fall_thr"])) if env["terminate"] else np.zeros(len(h), bool)
    alive = sub["alive"]
    live = alive > 0

    new = dict(sub)
    new["s"] = sn
    new["pos"] = npos
    new["rew_total"] = sub["rew_total"] + rew * alive
    new["member_steps"] = sub["member_steps"] + alive
    new["behv"] = np.where(live[:, None], npos, sub["behv"])
    ob_new = sn
    if g:
        rel = (sub["goal"] - npos[:, :2]) * f(0.1)
        ob_new = np.concatenate([sn, rel], axis=1)
    new["mo_sum"] = np.where(live[:, None], sub["mo_sum"] + ob_new, sub["mo_sum"])
    new["mo_sumsq"] = np.where(live[:, None], sub["mo_sumsq"] + ob_new * ob_new,
                               sub["mo_sumsq"])
    new["alive"] = alive * (dtype(1.0) - done.astype(dtype))

    out = st
    for k in new:
        if new[k] is not None:
            out[k] = out[k].copy()
            out[k][members] = new[k]
    info = {"h": h.astype(np.float64), "actions": a, "act_raw": act, "net_out": net,
            "done": done, "alive_before": live}
    return out, info


def loco_rollout(state, env, policy, n_steps, members=None, dtype=np.float64,
                 noise=None, salt_base=0):
    """n_steps consecutive loco_step calls, step t = 1.. drawing with salt
    salt_base + t; returns (state, [info per step])."""
    infos = []
    for t in range(n_steps):
        state, info = loco_step(state, env, policy, members, dtype, noise, salt_base + t)
        infos.append(info)
    return state, infos


def pair_member_rows(theta_vals, eps_vals, dtype=np.float64):
    """Effective weight rows of the antithetic pair kernels: theta_vals (n,)
    are the bf16(theta) values, eps_vals (pairs, n) the decoded sigma*eps rows
    in ELEMENT order. Returns (2*pairs, n): rows [theta+eps_p | theta-eps_p],
    so slot bp = p*eps+e reads row p and bm = (pairs+p)*eps+e row pairs+p."""
    t = np.asarray(theta_vals, dtype=np.float64)[None, :]
    e = np.asarray(eps_vals, dtype=np.float64)
    return np.concatenate([t + e, t - e], axis=0).astype(dtype)


# ------------------------------------------------------------------ optimizers
def adam_steps(theta, m, v, g, a_list, b1, b2, eps, l2, gscale, dtype=np.float64):
    f = lambda x: dtype(np.float32(x))
    theta, m, v, g = (np.asarray(z).astype(dtype) for z in (theta, m, v, g))
    for a in a_list:
        gg = f(l2) * theta - g * f(gscale)
        m = f(b1) * m + (dtype(1.0) - f(b1)) * gg
        v = f(b2) * v + (dtype(1.0) - f(b2)) * gg * gg
        theta = theta - f(a) * m / (np.sqrt(v) + f(eps))
    return {"theta": theta, "m": m, "v": v}


def sgd_steps(theta, v, g, n_steps, lr, momentum, l2, gscale, dtype=np.float64):
    f = lambda x: dtype(np.float32(x))
    theta, v, g = (np.asarray(z).astype(dtype) for z in (theta, v, g))
    for _ in range(n_steps):
        gg = f(l2) * theta - g * f(gscale)
        v = f(momentum) * v + (dtype(1.0) - f(momentum)) * gg
        theta = theta - f(lr) * v
    return {"theta": theta, "v": v}


def grad_gather(table_vals, offsets, fits, n, dtype=np.float64):
    """g[t] = sum_p fits[p] * table_vals[offsets[p] + t], p ascending."""
    tv = np.asarray(table_vals)
    acc = np.zeros(n, dtype=dtype)
    for o, fv in zip(np.asarray(offsets), np.asarray(fits)):
        acc = acc + dtype(fv) * tv[int(o):int(o) + n].astype(dtype)
    return acc


def quantized_table(table_f32, qstd):
    """decode(encode(float32(qstd*x))) * float32(1/qstd), float32 steps."""
    q = np.float32(qstd)
    qinv = np.float32(1.0) / q
    return (e4m3_roundtrip_f32(np.asarray(table_f32, np.float32) * q) * qinv).astype(
        np.float32)


# ------------------------------------------------------------------ tolerances
def err_scale(y32, y64):
    """E32 = max |y32 - y64|, floored at 2^-24 * max |y64|."""
    y64 = np.asarray(y64, dtype=np.float64)
    d = float(np.max(np.abs(np.asarray(y32, dtype=np.float64) - y64))) if y64.size else 0.0
    return max(d, _F32_EPS_FLOOR * float(np.max(np.abs(y64))) if y64.size else 0.0)


def fp32_error_scale(fn, *args, **kw):
    """Evaluate fn(..., dtype=float64) and fn(..., dtype=float32).

    fn returns an array, a dict of arrays, or a tuple whose first item is one
    of those. Returns (y64, E32) with E32 a float or a dict of floats keyed
    like y64 (None entries are skipped).
    """
    y64 = fn(*args, dtype=np.float64, **kw)
    y32 = fn(*args, dtype=np.float32, **kw)
    if isinstance(y64, tuple):
        y64, y32 = y64[0], y32[0]
    if isinstance(y64, dict):
        return y64, {k: err_scale(y32[k], y64[k]) for k in y64 if y64[k] is not None}
    return y64, err_scale(y32, y64)


def max_ratio(got, y64, e32):
    """max |got - y64| / E32 — the figure the tests bound by ERR_FACTOR."""
    return float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(y64, np.float64)))) / e32
