"""Float64 statement of the fused attention kernels (csrc/attention.hip: k_attn_fwd, k_attn_bwd_dq, k_attn_bwd_dkv) and the
score patterns that drive them into their edge cases.  Host only: the -m gpu tests compare the kernels with it, and
test_attn_ref_host.py checks it (and the patterns) against torch autograd without a GPU.

Conventions are the kernels': head dim 64, scale = 1/8, lse in base 2 of the scaled scores (log2 sum_j 2^(c s_ij) with
c = scale * log2 e), positions in tiles of 64 keys (forward) and waves of 32 queries."""
import numpy as np

from paa_amd.model import bf16_bits, bf16_to_f32, split_bf16

HD = 64
SCALE = HD ** -0.5
LOG2E = 1.4426950408889634
C2 = SCALE * LOG2E                       # scaled score in log2 units per unit of raw score q.k
NAN16 = 0x7FE5                           # bf16 NaN: the pad rows of every input plane and the untouched outputs
NAN32 = 0x7FE5A5A5                       # float32 NaN of the same kind for lse / delta
PATTERNS = ("random", "rising", "falling", "peaked", "flat", "negshift", "dominant_last")
FWD_TILE, WAVE, LAZY_STEP = 64, 32, 8.0  # k_attn_fwd: keys per iteration, queries per wave, lazy max threshold (log2)


def bf16_round(x):
    """float64 -> nearest bf16 value (through float32, round-to-nearest-even as v_cvt_pk_bf16_f32), as float64."""
    return bf16_to_f32(bf16_bits(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ------------------------------------------------------------------------------------------ patterns
def _jumps(T):
    """Key positions where `rising` steps up: a third and two thirds of the way through the 64-key tiles, and halfway
    into the last (partial) tile.  `falling` steps down there and at the end of the first tile."""
    nt = -(-T // FWD_TILE)
    if nt < 2:
        return []
    last = FWD_TILE * (nt - 1)
    return sorted({FWD_TILE * t for t in (nt // 3, 2 * nt // 3) if t >= 1} | {last + (T - last) // 2})


def head_pattern(name, T, rng):
    """float32 (q, k, v), each (T, 64), of one head whose score rows follow pattern `name` (one of PATTERNS)."""
    n = lambda: rng.standard_normal((T, HD))
    q, k, v = n(), n(), n()
    if name == "random":                          # the distribution the older attention tests use
        q, k, v = q * 1.5, k * 1.5, v * 1.5
    elif name in ("rising", "falling"):           # dimension 0 carries a level 16 (log2) per jump; noise sigma ~1.4 elsewhere
        steps = np.zeros(T)
        for j in (_jumps(T) if name == "rising" else sorted(set(_jumps(T)) | {FWD_TILE} if T > FWD_TILE else ())):
            steps[j:] += 16.0
        lvl = steps if name == "rising" else steps[-1] - steps
        q[:, 0] = 8.0
        k[:, 0] = lvl / (C2 * 8.0)
    elif name == "peaked":                        # q_i = 2 k_j(i) with |k| fixed: key j(i) leads by G (1 - cos) in log2 units
        G = np.log2(max(T, 2)) + 10.0
        k *= np.sqrt(G / (2.0 * C2)) / np.linalg.norm(k, axis=1, keepdims=True)
        k = bf16_round(k)
        q = 2.0 * k[rng.integers(0, T, T)]
    elif name == "flat":                          # every score 0: uniform rows
        q[:] = 0.0
    elif name == "negshift":                      # scaled scores ~ -151.5 +- 1.4: lse < -128, exp2(-lse) overflows f32
        q[:, 0] = 30.0
        k[:, 0] = -28.0
    elif name == "dominant_last":                 # key T-1 (in the masked last tile) leads every row by ~16 (log2)
        q[:, 0] = 8.0
        k[:, 0] = 0.0
        k[T - 1, 0] = 16.0 / (C2 * 8.0)
    else:
        raise ValueError(name)
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32)


def build_inputs(B, nh, T, P, Tp, split, seed, patterns=None):
    """Planes of one attention call: qkv (B*P, 3H) and dO (B*P, H) as uint16 bf16 bits (hi, and lo in split mode);
    rows [T, P) of every clip in every plane hold the NaN sentinel.  Head (b, h) follows patterns[b * nh + h]
    (default: PATTERNS in turn).  Returns a dict with the planes, the float64 values they represent (qkv (B, T, 3H),
    do (B, T, H)), those values as (hi, lo) plane pairs (qkv_pl, do_pl; lo = 0 in bf16 mode) and the per-head
    pattern names."""
    assert 1 <= T < P and Tp >= T
    H = nh * HD
    rng = np.random.default_rng(seed)
    pats = list(patterns) if patterns is not None else [PATTERNS[i % len(PATTERNS)] for i in range(B * nh)]
    qkv = np.zeros((B, P, 3 * H), np.float32)
    do = np.zeros((B, P, H), np.float32)
    for b in range(B):
        for h in range(nh):
            for i, x in enumerate(head_pattern(pats[b * nh + h], T, rng)):
                qkv[b, :T, i * H + h * HD:i * H + (h + 1) * HD] = x
        do[b, :T] = rng.standard_normal((T, H))
    out = {"patterns": pats}
    for name, x in (("qkv", qkv), ("do", do)):
        hi, lo = split_bf16(x) if split else (bf16_bits(x), None)
        vh = bf16_to_f32(hi).astype(np.float64)
        vl = bf16_to_f32(lo).astype(np.float64) if split else np.zeros_like(vh)
        for pl in (hi, lo):
            if pl is not None:
                pl[:, T:] = NAN16
        out[name + "_hi"] = hi.reshape(B * P, -1)
        out[name + "_lo"] = None if lo is None else lo.reshape(B * P, -1)
        out[name] = (vh + vl)[:, :T]
        out[name + "_pl"] = (vh[:, :T], vl[:, :T])
    return out


def head_slices(val, nh, h):
    """(q, k, v) of head h from a (T, 3H) float64 qkv block."""
    H = nh * HD
    return tuple(val[:, i * H + h * HD:i * H + (h + 1) * HD] for i in range(3))


def head_planes(inp, b, nh, h):
    """(q, k, v, do) of head (b, h) as (hi, lo) pairs of float64 plane values: the operands of attn_emulated."""
    (qh, ql), (dh, dl) = inp["qkv_pl"], inp["do_pl"]
    cols = slice(h * HD, (h + 1) * HD)
    return (*zip(head_slices(qh[b], nh, h), head_slices(ql[b], nh, h)), (dh[b][:, cols], dl[b][:, cols]))


# ------------------------------------------------------------------------------------------ reference
def scores2(q, k):
    """Scaled scores in log2 units, c * q.k (float64)."""
    return (q @ k.T) * C2


def lazy_max_trace(s2):
    """Replays k_attn_fwd's running maximum on scaled scores s2 (T, T): waves of 32 queries, tiles of 64 keys, a lane's
    maximum raised only when the tile's maximum exceeds it by more than 8, and only when some lane of the wave does so.
    Returns (m, raised): m[i, t] is query i's maximum when key tile t is exponentiated, raised[w, t] whether wave w
    raised at tile t."""
    T = s2.shape[0]
    nt = -(-T // FWD_TILE)
    m = np.empty((T, nt))
    raised = np.zeros((-(-T // WAVE), nt), bool)
    for w in range(raised.shape[0]):
        rows = s2[w * WAVE:(w + 1) * WAVE]
        cur = np.full(rows.shape[0], -np.inf)
        for t in range(nt):
            mx = rows[:, t * FWD_TILE:(t + 1) * FWD_TILE].max(1)
            up = mx > cur + LAZY_STEP
            if up.any():
                raised[w, t] = True
                cur = np.where(up, mx, cur)
            m[w * WAVE:(w + 1) * WAVE, t] = cur
    return m, raised


def lazy_max_raises(s2):
    """(raises after the first tile, raises in the last tile) of the forward's lazy running maximum, counted per wave."""
    _, raised = lazy_max_trace(s2)
    return int(raised[:, 1:].sum()), int(raised[:, -1].sum()) if raised.shape[1] > 1 else 0


def attn_ref(q, k, v, do):
    """One head in float64.  q, k, v, do: (T, 64) float64, the exact values the kernel's planes hold.
    Returns o, lse (base 2, the kernel's convention), dq, dk, dv, nat and kappa.  nat: for dq and dk, the natural scale
    scale * (P * (|dP| + |delta|)) |K| (|Q| for dk), the sum of the magnitudes of the terms each entry is summed from;
    kappa = max nat / max |dq| (|dk|).  A large kappa marks a saturated head, whose gradient is small next to those
    terms, so that any rounding of them is magnified."""
    s2 = scores2(q, k)
    mx = s2.max(1, keepdims=True)
    e = np.exp2(s2 - mx)
    l = e.sum(1, keepdims=True)
    p = e / l
    o = p @ v
    dp = do @ v.T
    delta = (do * o).sum(1, keepdims=True)
    ds = p * (dp - delta)
    dq, dk = ds @ k * SCALE, ds.T @ q * SCALE
    w = p * (np.abs(dp) + np.abs(delta)) * SCALE
    nat = {"dq": w @ np.abs(k), "dk": w.T @ np.abs(q)}
    kappa = {t: nat[t].max() / max(np.abs(g).max(), 1e-300) for t, g in (("dq", dq), ("dk", dk))}
    return {"o": o, "lse": mx[:, 0] + np.log2(l[:, 0]), "dq": dq, "dk": dk, "dv": p.T @ do, "nat": nat, "kappa": kappa}


def _planes(x, split):
    """The (hi, lo) bf16 planes a kernel stores for float32 x (lo = bf16(x - hi) in split mode, 0 in bf16 mode)."""
    x32 = np.asarray(x, dtype=np.float32)
    hi = bf16_round(x32)
    return hi, (bf16_round(x32 - hi) if split else np.zeros_like(hi))


def _mm(a, b):
    """a @ b of two (hi, lo) pairs as the 3-pass MFMA forms it: hi*hi + hi*lo + lo*hi, the lo*lo term dropped."""
    return a[0] @ b[0] + a[0] @ b[1] + a[1] @ b[0]


def _t(a):
    return a[0].T, a[1].T


def attn_emulated(q, k, v, do, mode, o_stored=None):
    """One head with the kernels' own arithmetic in float64.  q, k, v, do: (hi, lo) pairs of plane values (lo = 0 in
    bf16 mode).  Products go through _mm, and every value a kernel rounds to bf16 planes is rounded here too: the
    forward's unnormalised P at the lazily raised maximum, O, and the backward's P and dS (hi + lo pairs in split
    mode).  o_stored: the O the kernel stored, which is what enters delta (default: this function's own O, rounded).
    Returns o, lse, dq, dk, dv."""
    split = mode == "split"
    s2 = _mm(q, _t(k)) * C2
    mx = s2.max(1, keepdims=True)
    lse = mx[:, 0] + np.log2(np.exp2(s2 - mx).sum(1))
    m, _ = lazy_max_trace(s2)
    mj = np.repeat(m, FWD_TILE, axis=1)[:, :s2.shape[1]]
    f = np.exp2(mj - lse[:, None])
    pu = _planes(np.exp2(s2 - mj), split)
    o = _mm((pu[0] * f, pu[1] * f), v)
    od = sum(_planes(o, split)) if o_stored is None else o_stored
    p = np.exp2(s2 - lse[:, None])
    ds = _planes(p * (_mm(do, _t(v)) - ((do[0] + do[1]) * od).sum(1, keepdims=True)), split)
    return {"o": o, "lse": lse, "dq": _mm(ds, k) * SCALE, "dk": _mm(_t(ds), q) * SCALE, "dv": _mm(_t(_planes(p, split)), do)}
