"""Integer-valued data for bit-exact tests of the accumulating kernels (host only; the GPU tests and tests/test_exact_data_host.py share it).

The technique ("Exact-data tests"): when every input is a small integer (or a small integer times a power of two), every product and every
partial sum of a kernel is exactly representable in its fp32 accumulator IN ANY ORDER, so the order of summation, which is a kernel's
only legitimate freedom on random data, has no effect.  What is left are the documented rounding points (one RNE each), which an fp64
evaluation reproduces: an exactly representable value converts double -> float -> half / bf16 with a single rounding.  The result must
then match bit for bit, and a dropped, duplicated or mis-masked element changes bits.

Every *_expect function returns, next to the expected tensors, the PRECONDITIONS the argument rests on, as {name: (value, limit)} with
value < limit required; check_pre() asserts them, and every test calls it: a case cannot pass because its data was not exact."""
import functools

import torch

LIMIT = float(2 ** 24)   # integers below 2^24 in magnitude are exact in fp32
F16_MAX = 65504.0
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def check_pre(pre):
    for name, (value, limit) in pre.items():
        assert value < limit, f"exactness precondition {name}: {value} is not below {limit}"


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g)


def _to_f16(v64):
    """fp64 -> fp16 through fp32: a single rounding when v64 is exact in fp32 (asserted)"""
    v32 = v64.float()
    fin = torch.isfinite(v64)
    assert torch.equal(v32.double()[fin], v64[fin]), "value not exact in fp32: the conversion would round twice"
    return v32.half()


def seed_of(*key):
    """one deterministic seed per case"""
    s = 0
    for k in key:
        s = (s * 1000003 + (int(k) if not isinstance(k, str) else sum(map(ord, k)))) % (2 ** 31 - 1)
    return s


# ---- K10  y = fp16( fp16(x B^T) A^T + bias ) --------------------------------------------------------------------------------------

K10_TOKENS = [1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 64, 65, 128, 255, 256]
K10_MID = (2048, 600, 1536)   # K, r, N of the token sweep
# (T, K, r, N, with_bias)
K10_SHAPES = (
    [(T,) + K10_MID + (bool(i % 2),) for i, T in enumerate(K10_TOKENS)]
    # the shapes of tests/test_gpu_lowrank_forward.py
    + [(1, 4096, 1843, 4096, False), (16, 4096, 1024, 4096, True), (2, 4096, 1024, 4096, True), (3, 11008, 1500, 4096, True),
       (4, 4096, 2686, 11008, False), (33, 4096, 2686, 11008, False), (7, 11008, 1500, 4096, True), (256, 768, 345, 3072, True),
       (5, 64, 3, 70, True)]
    # Llama-13B down_proj: K beyond the GEMV kernel's register budget, decode-sized T -> the MFMA kernel with one token tile
    + [(4, 13824, 2048, 5120, True), (1, 13824, 2048, 5120, False), (2, 13824, 2048, 5120, True)]
    + [(4, 11264, 512, 1024, True), (1, 11264, 512, 1024, False)]   # the largest K the GEMV pair takes
    + [(256, 11008, 1500, 4096, False)]
    + [(T, 256, r, 130, bool(r % 2)) for T in (2, 7) for r in (1, 63, 64, 65)]
    + [(T, 256, 65, N, bool(N % 2)) for T in (3, 7) for N in (1, 15, 17, 33, 70)]
    + [(5, 256, 4096, 1024, True), (40, 128, 4096, 300, False)]    # sl1 = 32 with sl2 = 16 on a 256-CU device
)
K10_BIG = [(256, 11008, 1500, 4096), (33, 4096, 2686, 11008), (4, 13824, 2048, 5120)]   # must show rounded entries and ties above 2048
# (T, K, r, N, with_bias) with x in [-60, 60]: |z| passes 2048, so the rounding of z itself (ties included) and fp16 saturation of y are exercised
K10_WIDE_X = [(33, 4096, 1024, 4096, True), (4, 4096, 1024, 4096, False), (130, 2048, 600, 1536, True)]
K10_REUSE_SHAPE = (2048, 600, 1536)
K10_REUSE_TOKENS = [256, 1, 33, 4, 2, 17, 3]


def k10_data(g, T, K, r, N, with_bias, positive=False, xmax=3):
    """x in [-xmax, xmax], B and A in {-1, 0, 1}, integer bias in [-64, 64]; positive: B and A in {1, 2} (a +Inf in x then gives +Inf, not
    NaN, in fp64, and the finite rows grow large enough to saturate fp16)"""
    x = _ints(g, -xmax, xmax, (T, K)).half()
    lo, hi = (1, 2) if positive else (-1, 1)
    B = _ints(g, lo, hi, (r, K)).half()
    A = _ints(g, lo, hi, (N, r)).half()
    bias = _ints(g, -64, 64, (N,)).half() if with_bias else None
    return x, B, A, bias


def k10_expect(x, B, A, bias):
    """(z_ref fp16 [T, r], y_ref fp16 [T, N], pre): z_ref = fp16(x B^T), y_ref = fp16(z_ref A^T + bias), the kernel's two rounding points"""
    xd, Bd, Ad = x.double(), B.double(), A.double()
    z_ref = _to_f16(xd @ Bd.T)
    zd = z_ref.double()
    y64 = zd @ Ad.T
    y_abs = zd.abs() @ Ad.abs().T
    if bias is not None:
        y64 = y64 + bias.double()
        y_abs = y_abs + bias.double().abs()
    pre = {"max sum_k |x||B|": ((xd.abs() @ Bd.abs().T).max().item(), LIMIT),
           "max sum_j |z||A| + |bias|": (y_abs.max().item(), LIMIT),
           "max |z| (fp16 range)": (zd.abs().max().item(), F16_MAX)}
    return z_ref, _to_f16(y64), pre


def k10_y64(x, B, A, bias):
    """the unrounded second stage (fp64), for counting the entries that need rounding"""
    z_ref = _to_f16(x.double() @ B.double().T)
    y64 = z_ref.double() @ A.double().T
    return y64 + bias.double() if bias is not None else y64


def round_stats(v64):
    """(entries that fp16 must round, exact ties among them, entries that overflow to Inf) of finite fp64 values"""
    h = v64.float().half()
    fin = torch.isfinite(h)
    rounded = fin & (h.double() != v64)
    # a tie: v is the midpoint of h and the fp16 number next to it, other = 2 v - h (adjacent numbers of one sign differ by one in their bits)
    other = 2 * v64 - h.double()
    o16 = other.float().half()
    adjacent = (o16.view(torch.int16).int() - h.view(torch.int16).int()).abs() == 1
    tie = rounded & (o16.double() == other) & adjacent
    return int(rounded.sum()), int(tie.sum()), int((~fin).sum())


# ---- K12  y = fp16( x w^T + bias ),  w = fp16(scale (q - zero)) ---------------------------------------------------------------------

K12_TOKENS = [1, 4, 31, 32, 33, 256]
K12_KS = [1, 8, 15, 16, 17, 24, 127, 128, 129, 144, 152, 352, 1000, 1001] + [128 * j for j in range(2, 10)]
# (T, N): on a 256-CU device the feature tile is 32, 16 and 8 wide
K12_TN = [(256, 1001), (256, 600), (33, 70)]
K12_PLAIN = [(256, 11008, 4096), (33, 4096, 11008), (4, 4096, 4096), (1, 11008, 4096), (31, 4096, 11008)]   # (T, K, N): the three 7B shapes
K12_BIG = [(256, 11008, 4096), (33, 4096, 11008)]   # must show rounded entries and fp16 overflow
K12_OFFSETS = [16, 5]   # column offsets of the code views: rows stay 16-byte aligned / lose the alignment


def k12_cases():
    """(T, K, N, with_bias, max_code)"""
    cases = [(T, K, N, bool((K + N) % 2), 255) for K in K12_KS for T, N in K12_TN]
    cases += [(T, 352, 300, bool(T % 2), 255) for T in K12_TOKENS] + [(T, 1001, 37, bool(T % 2), 63) for T in K12_TOKENS]
    cases += [(T, K, N, bool(T % 2), mc) for T, K, N in K12_PLAIN for mc in (255, 63)]
    return cases


def k12_data(g, T, K, N, with_bias, max_code=255, positive=False):
    """x in {-1, 0, 1}; codes over 0..max_code with both ends in every row (K >= 2); zero an integer in 0..max_code, with rows at 0, at
    max_code and at a half-integer; scale a power of two in 2^-4..2^-1, a few rows 4.  positive: zero = 0 and codes >= 1, every weight > 0."""
    x = _ints(g, -1, 1, (T, K)).half()
    q = _ints(g, 1 if positive else 0, max_code, (N, K))
    n = torch.arange(N)
    if K >= 2 and not positive:
        q[n, n % K] = 0
        q[n, (n + 1) % K] = max_code
    elif not positive:
        q[:, 0] = torch.where(n % 2 == 0, 0, max_code)
    zero = _ints(g, 0, max_code, (N,)).float()
    zero[n % 16 == 3] = 0.0
    zero[n % 16 == 7] = float(max_code)
    half = n % 16 == 11
    zero[half] = zero[half].clamp(max=max_code - 1) + 0.5
    if positive:
        zero[:] = 0.0
    scale = torch.pow(2.0, -_ints(g, 1, 4, (N,)).float())
    scale[n % 32 == 13] = 4.0
    bias = _ints(g, -64, 64, (N,)).half() if with_bias else None
    return x, q.to(torch.uint8), scale, zero, bias


def k12_weight(q, scale, zero):
    """fp64 w = scale (q - zero); asserted exact in fp16, so it IS the kernel's fp16 weight"""
    w = scale.double()[:, None] * (q.double() - zero.double()[:, None])
    assert torch.equal(w.half().double(), w), "scale * (q - zero) is not exact in fp16"
    return w


def k12_expect(x, q, scale, zero, bias):
    """(y_ref fp16 [T, N], y64, pre).  Per output feature n all terms are integer multiples of a unit u_n (scale_n, halved for a half-integer
    zero; 1 at most when an integer bias is added): the fp32 sums are exact while sum |terms| / u_n < 2^24."""
    w = k12_weight(q, scale, zero)
    xd = x.double()
    y64 = xd @ w.T
    mag = xd.abs() @ w.abs().T
    unit = torch.where(zero.double() == zero.double().floor(), scale.double(), scale.double() / 2)
    if bias is not None:
        y64 = y64 + bias.double()
        mag = mag + bias.double().abs()
        unit = unit.clamp(max=1.0)
    pre = {"max_n sum_k |x||w| / unit_n": ((mag / unit[None, :]).max().item(), LIMIT)}
    return _to_f16(y64), y64, pre


def k12_class(T, K, N, cus, ldq_aligned=True):
    """coverage class of a case under the host dispatch of asvd_w8_linear_f16 (restated for COUNTING only, never for an expected value):
    (feature tile, 16-byte loads?, what K leaves beyond a multiple of 128, whole iterations mod 8)"""
    nT = (T + 31) // 32
    ft = 32
    while ft > 8 and nT * ((N + ft - 1) // ft) < cus:
        ft //= 2
    vec = ldq_aligned and K % 8 == 0
    nkfull = K // 128 if vec else 0
    rem = K % 128
    tail = "none" if rem == 0 else ("lt16" if rem < 16 else ("ge16_whole" if K % 16 == 0 else "ge16_partial"))
    return ft, vec, tail, (nkfull % 8 if nkfull else None)


def k10_class(T, K, r, N, cus):
    """coverage class of a case under the host dispatch of asvd_lowrank_forward_f16 (for COUNTING only)"""
    rp = (r + 63) // 64 * 64
    nT = (T + 31) // 32
    sl1 = 32 if nT * (rp // 32) >= cus // 2 else 16
    sl2 = 32 if nT * ((N + 31) // 32) >= cus // 2 else 16
    TT = 1 if T <= 1 else (2 if T <= 2 else 4)
    if T <= 4 and K <= 11264 and rp <= 11264 and TT * max(K, rp) * 2 <= 96 * 1024:
        return ("gemv", TT)
    return ("mfma", sl1, sl2, "decode_bigK" if T <= 4 else "tiles")


def k10_missing(classes):
    """the K10 dispatch classes that no case reaches: the GEMV pair at 1, 2 and 4 token rows, the MFMA kernel at every pair of tile widths,
    and the MFMA kernel at decode size (K beyond the GEMV pair)"""
    want = {("gemv", 1), ("gemv", 2), ("gemv", 4)} | {("mfma", a, b) for a in (16, 32) for b in (16, 32)} | {("mfma", "decode_bigK")}
    have = {c[:3] if c[0] == "mfma" else c for c in classes} | {("mfma", c[3]) for c in classes if c[0] == "mfma"}
    return sorted(want - have, key=str)


def k12_views(K):
    """(column offset, row stride a multiple of 16) of the three code tensors every K12 case runs: contiguous, and views at the offsets of
    K12_OFFSETS into a buffer whose row stride is a multiple of 16"""
    return [(0, K % 16 == 0)] + [(off, True) for off in K12_OFFSETS]


def k12_missing(classes):
    want = {(ft, vec, tail) for ft in (8, 16, 32) for vec in (True, False) for tail in ("none", "lt16", "ge16_partial")}
    have = {c[:3] for c in classes}
    residues = {c[3] for c in classes if c[1] and c[3] is not None}
    return sorted(want - have, key=str) + [f"nkfull mod 8 == {j}" for j in range(8) if j not in residues]


# ---- K9  (|W - A B|^2, |W|^2) -----------------------------------------------------------------------------------------------------

K9_SHAPES = [(520, 264, 77), (1000, 777, 345), (129, 136, 1), (4096, 4096, 1843), (70016, 160, 40)]


def k9_cases():
    """(m, n, r, w_dtype, ab_dtype, path, strided).  path: 'fused' (one launch; needs n % 8 == 0), 'padded' (three launches: n % 8 != 0, or a
    B that is not 16-byte aligned), 'f32' (fp32 factors)"""
    out = []
    for m, n, r in K9_SHAPES:
        for wdt in ("f32", "f16", "bf16"):
            for strided in (False, True):
                for abdt in ("f16", "bf16"):
                    for path in (("fused", "padded") if n % 8 == 0 else ("padded",)):
                        out.append((m, n, r, wdt, abdt, path, strided))
                out.append((m, n, r, wdt, "f32", "f32", strided))
    return out


@functools.lru_cache(maxsize=4)
def k9_data(m, n, r, lim):
    """integer factors in [-lim, lim], a sparse d in {-1, 0, 1}, and W = A B + d in fp64 (cached: the dtype variants of a shape share it)"""
    g = torch.Generator().manual_seed(seed_of(m, n, r, lim))
    A = _ints(g, -lim, lim, (m, r)).double()
    B = _ints(g, -lim, lim, (r, n)).double()
    d = (_ints(g, -1, 1, (m, n)) * (torch.rand((m, n), generator=g) < 0.05)).double()
    W = A @ B
    W += d
    return A, B, d, W


def k9_expect(m, n, r, w_dtype):
    """(A, B fp64, W in w_dtype, e2, w2, pre): factors in [-2, 2] (in {-1, 0, 1} for a bf16 W, whose integers end at 256)"""
    lim = 1 if w_dtype == torch.bfloat16 else 2
    A, B, d, W = k9_data(m, n, r, lim)
    Wt = W.to(w_dtype)
    assert torch.equal(Wt.double(), W), f"W is not exact in {w_dtype}"
    e2, w2 = (d * d).sum().item(), (W * W).sum().item()
    pre = {"r max|A| max|B| (fp32 product sums)": (float(r * lim * lim), LIMIT), "sum W^2 (fp64 sums)": (w2, float(2 ** 53))}
    return A, B, Wt, e2, w2, pre


# ---- K8  |W|^2 --------------------------------------------------------------------------------------------------------------------

K8_SHAPES = [(1, 1), (37, 100), (2047, 4096)]


def k8_data(g, m, n):
    """entries in {-2..2}, thinned so that the sum of squares stays below 2^23"""
    W = _ints(g, -2, 2, (m, n))
    keep = min(1.0, 2 ** 23 / (2.0 * m * n))
    if keep < 1.0:
        W = W * (torch.rand((m, n), generator=g) < keep)
    if m * n == 1:
        W[:] = 2
    return W


def k8_expect(W):
    ss = (W.double() ** 2).sum().item()
    return ss, {"sum W^2": (ss, LIMIT)}


# ---- K1/K2  |x| column statistics ---------------------------------------------------------------------------------------------------

ABSSTAT_ROWS = [1, 37, 2047, 2048]
ABSSTAT_COLS = [64, 100, 4096, 11008]
ABSSTAT_MODES = ["abs_mean", "abs_max", "sq_mean"]


def absstat_data(g, rows, cols, dtype):
    return _ints(g, -6, 6, (rows, cols)).to(dtype)


def absstat_expect(acc, x, method):
    """the accumulator after one hook call, by the kernel's stated contract: the exact column sum (of |x|, or of x^2 rounded to the dtype —
    exact here), ONE fp32 divide by rows, one rounding to the accumulator's dtype, `+=` with one rounding; abs_max: where(max > acc, max, acc)"""
    xd = x.double()
    if method == "abs_max":
        mx = xd.abs().amax(0).to(acc.dtype)
        return torch.where(mx > acc, mx, acc), {"max |x| (exact in the dtype)": (xd.abs().max().item(), 256.0)}
    a = xd.abs() if method == "abs_mean" else xd * xd
    assert torch.equal(a.to(x.dtype).double(), a)
    S = a.sum(0)
    mean = (S.float() / float(x.shape[0])).to(acc.dtype)
    return (acc.float() + mean.float()).to(acc.dtype), {"max column sum": (S.max().item(), LIMIT)}


def absstat_oracle(acc, x, method):
    """the same update through the CPU oracle (the reference hook's own torch ops)"""
    from oracle import asvd_oracle as O
    if method == "sq_mean":
        return O.fisher_update(acc, x)
    return O.hook_update(acc, x.unsqueeze(0), method)


# ---- w8_dequant -------------------------------------------------------------------------------------------------------------------

def dequant_data(g, rows=37, reps=2):
    """codes [rows, 256 * reps], every row a shuffle of all 256 codes (reps times); random fp32 scale and zero, nothing special about them"""
    q = torch.stack([torch.cat([torch.randperm(256, generator=g) for _ in range(reps)]) for _ in range(rows)]).to(torch.uint8)
    scale = torch.rand(rows, generator=g) * 0.02 + 1e-4
    zero = torch.rand(rows, generator=g) * 255.0
    return q, scale, zero


def dequant_expect(q, scale, zero, dtype):
    """torch-CPU fp32 restatement: the subtraction, one fp32 product, one rounding to dtype"""
    return (scale[:, None] * (q.float() - zero[:, None])).to(dtype)


# ---- non-finite inputs: one bad token row, every other row untouched ------------------------------------------------------------------

# (name, (T, K, r, N), positive weights, bad row, bad k, value).  Positive weights: the fp64 reference of a row with +Inf is +Inf, not NaN.
# "last8": the bad value sits among the last 8 elements of a K = 11008 row, the 16-byte piece next to the GEMV kernel's masked lanes.
K10_NONFINITE = [
    ("nan_mfma", (33, 4096, 1024, 4096), False, 17, 100, float("nan")),
    ("nan_gemv", (2, 4096, 1024, 4096), False, 0, 4095, float("nan")),
    ("inf_mfma", (33, 11008, 70, 600), True, 32, 5000, float("inf")),
    ("inf_last8_mfma", (40, 11008, 70, 600), True, 3, 11008 - 3, float("inf")),
    ("inf_last8_gemv", (4, 11008, 300, 600), True, 1, 11008 - 3, float("inf")),
]
# (name, (T, K, N), positive weights, bad row, bad k, value)
K12_NONFINITE = [
    ("nan", (33, 4096, 4096), False, 32, 77, float("nan")),
    ("inf", (33, 4096, 4096), True, 5, 4000, float("inf")),
    ("neg_inf", (4, 1024, 600), True, 2, 0, float("-inf")),
    ("inf_last8", (33, 11008, 4096), True, 31, 11008 - 3, float("inf")),
    ("inf_ragged_tail", (5, 1001, 70), True, 4, 1000, float("inf")),
]


def with_bad_value(x, row, k, value):
    xb = x.clone()
    xb[row, k] = value
    return xb


def value_class(t):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf, element for element"""
    return torch.isnan(t) * 1 + (t == float("inf")) * 2 + (t == float("-inf")) * 3


def k10_row_ref(xrow, B, A, bias):
    """fp64 evaluation of ONE token row that may hold a non-finite value (the same two rounding points; no exactness is claimed for it)"""
    z = (xrow.double()[None, :] @ B.double().T).float().half()
    y = z.double() @ A.double().T
    if bias is not None:
        y = y + bias.double()
    return y.float().half()[0]


def k12_row_ref(xrow, q, scale, zero, bias):
    y = xrow.double()[None, :] @ k12_weight(q, scale, zero).T
    if bias is not None:
        y = y + bias.double()
    return y.float().half()[0]
