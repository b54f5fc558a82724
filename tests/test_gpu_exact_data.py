"""The accumulating kernels on integer-valued data (tests/exact_data.py, DESIGN.md 4, "Exact-data tests"): every partial sum is exactly representable in any
order, so the kernel's only freedom is the one RNE rounding at each documented rounding point and the result must equal the fp64
evaluation of those rounding points BIT FOR BIT.  No tolerance anywhere in this file: every comparison is torch.equal, NaN positions
included.  tests/test_exact_data_host.py shows on the CPU that every case stays within the exactness preconditions; they are asserted
again here, so a case cannot pass because its data was not exact."""
import pytest
import torch

from tests import exact_data as E

pytestmark = pytest.mark.gpu


def same(got, want):
    """bit comparison of a device result with a host expectation: NaN exactly where the expectation has NaN, every other element (Inf
    included) equal"""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and torch.equal(got[~gn], want[~wn])


def where_differs(got, want, limit=8):
    """rows / columns of the mismatches, for the assertion message: the pattern names the bug (a k-chunk, a tile edge, a wave)"""
    got = got.detach().cpu()
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    idx = bad.nonzero()
    rows, cols = sorted(set(idx[:, 0].tolist())), sorted(set(idx[:, -1].tolist()))
    first = [(tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in idx[:limit]]
    return f"{int(bad.sum())} of {bad.numel()} differ; rows {rows[:limit]}... ({len(rows)}), cols {cols[:limit]}... ({len(cols)}); (index, got, want): {first}"


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- K10 --------------------------------------------------------------------------------------------------------------------------

def _z_of(work, T, rp):
    """the intermediate z as the launch left it: [32 ceil(T / 32), rp] fp16 at byte offset 256 of the workspace"""
    Tp = (T + 31) // 32 * 32
    return work[256:256 + 2 * Tp * rp].view(torch.float16).view(Tp, rp)


def _check_k10(gpu, x, B, A, bias, z_ref, y_ref, packed=None):
    from asvd4llm_amd import ops
    T, r = x.shape[0], B.shape[0]
    Ap, Bp, work = packed or ops.lowrank_pack(A.to(gpu), B.to(gpu))   # a fresh workspace is zero-filled
    y = ops.lowrank_forward(x.to(gpu), Ap, Bp, None if bias is None else bias.to(gpu), work)
    torch.cuda.synchronize()
    assert same(y, y_ref), where_differs(y, y_ref)
    if packed is None:
        z = _z_of(work, T, Ap.shape[1]).cpu()
        assert same(z[:T, :r], z_ref), where_differs(z[:T, :r], z_ref)
        assert not bool(z[T:].any()) and not bool(z[:, r:].any())     # padding rows and padded ranks: exactly zero
    return y


@pytest.mark.parametrize("T,K,r,N,with_bias", E.K10_SHAPES)
def test_k10_fused_forward_is_exact(gpu, T, K, r, N, with_bias):
    g = torch.Generator().manual_seed(E.seed_of(10, T, K, r, N))
    x, B, A, bias = E.k10_data(g, T, K, r, N, with_bias)
    z_ref, y_ref, pre = E.k10_expect(x, B, A, bias)
    E.check_pre(pre)
    _check_k10(gpu, x, B, A, bias, z_ref, y_ref)


@pytest.mark.parametrize("T,K,r,N,with_bias", E.K10_WIDE_X)
def test_k10_z_rounding_and_output_saturation(gpu, T, K, r, N, with_bias):
    """x in [-60, 60]: |z| passes 2048, so z itself needs rounding (exact ties included: the first rounding point), and a part of y overflows
    fp16: +-Inf exactly where the reference rounds to +-Inf"""
    g = torch.Generator().manual_seed(E.seed_of(13, T, K, r, N))
    x, B, A, bias = E.k10_data(g, T, K, r, N, with_bias, xmax=60)
    z_ref, y_ref, pre = E.k10_expect(x, B, A, bias)
    E.check_pre(pre)
    assert bool((z_ref.abs() > 2048).any()) and bool(torch.isinf(y_ref).any())
    _check_k10(gpu, x, B, A, bias, z_ref, y_ref)


def test_k10_one_workspace_over_changing_token_counts(gpu):
    """one packed module, one workspace, token counts that move between the MFMA kernel and the three GEMV variants: what an earlier call
    left in z (rows beyond this call's tokens) and in the barrier words must not reach a later result"""
    from asvd4llm_amd import ops
    K, r, N = E.K10_REUSE_SHAPE
    g = torch.Generator().manual_seed(E.seed_of(11, K, r, N))
    _, B, A, bias = E.k10_data(g, 1, K, r, N, True)
    packed = ops.lowrank_pack(A.to(gpu), B.to(gpu))
    for T in E.K10_REUSE_TOKENS:
        x = E.k10_data(g, T, K, r, N, False)[0]   # fresh activations every call
        z_ref, y_ref, pre = E.k10_expect(x, B, A, bias)
        E.check_pre(pre)
        _check_k10(gpu, x, B, A, bias, z_ref, y_ref, packed)
    ops.lowrank_check(packed[2])


@pytest.mark.parametrize("name,shape,positive,row,k,value", E.K10_NONFINITE, ids=[c[0] for c in E.K10_NONFINITE])
def test_k10_bad_token_row_stays_in_its_row(gpu, name, shape, positive, row, k, value):
    """a NaN / Inf in one token row: every other row is bit-identical to the run without it, and the row itself is non-finite wherever the
    fp64 reference is (the kernel may turn Inf into NaN there: zero-padded ranks and masked GEMV lanes multiply it by zero, DESIGN.md 4, "Exact-data tests").
    The positive-weight cases also saturate fp16 in rows with finite inputs: +Inf exactly where the reference rounds to +Inf."""
    T, K, r, N = shape
    g = torch.Generator().manual_seed(E.seed_of(100, *shape))
    x, B, A, bias = E.k10_data(g, T, K, r, N, True, positive)
    z_ref, y_ref, pre = E.k10_expect(x, B, A, bias)
    E.check_pre(pre)
    y0 = _check_k10(gpu, x, B, A, bias, z_ref, y_ref)
    xb = E.with_bad_value(x, row, k, value)
    from asvd4llm_amd import ops
    Ap, Bp, work = ops.lowrank_pack(A.to(gpu), B.to(gpu))
    y1 = ops.lowrank_forward(xb.to(gpu), Ap, Bp, bias.to(gpu), work).cpu()
    keep = torch.arange(T) != row
    assert same(y1[keep], y_ref[keep]) and same(y1[keep], y0.cpu()[keep]), where_differs(y1[keep], y_ref[keep])
    lost = ~torch.isfinite(E.k10_row_ref(xb[row], B, A, bias))
    assert bool(lost.all()) and not bool(torch.isfinite(y1[row][lost]).any())


def test_k10_cases_reach_every_dispatch_class(gpu):
    """the host dispatch of asvd_lowrank_forward_f16 restated (for counting only) with this device's CU count: the GEMV pair at 1, 2 and 4
    token rows, the MFMA kernel at all four (phase-1, phase-2) tile widths, and the MFMA kernel at decode size with K > 11264"""
    classes = {}
    for T, K, r, N, _ in E.K10_SHAPES:
        classes.setdefault(E.k10_class(T, K, r, N, _cus()), []).append((T, K, r, N))
    print({c: len(v) for c, v in classes.items()})
    missing = E.k10_missing(set(classes))
    assert not missing, missing


# ---- K12 --------------------------------------------------------------------------------------------------------------------------

def _check_k12(gpu, x, q, scale, zero, bias, y_ref):
    from asvd4llm_amd import ops
    xd, sd, zd, bd = x.to(gpu), scale.to(gpu), zero.to(gpu), None if bias is None else bias.to(gpu)
    N, K = q.shape
    y0 = None
    for off in [0] + E.K12_OFFSETS:   # one buffer per view: the views at different offsets would overlap in one
        if off == 0:
            qv = q.to(gpu)
        else:
            big = torch.full((N, (K + 15) // 16 * 16 + 48), 255, dtype=torch.uint8, device=gpu)
            big[:, off:off + K] = q.to(gpu)
            qv = big[:, off:off + K]
        y = ops.w8_linear(xd, qv, sd, zd, bd)
        assert same(y, y_ref), (off, where_differs(y, y_ref))
        if y0 is None:
            y0 = y
        else:   # the same arithmetic whatever the load path (NaN-free here or not: compare the bits)
            assert torch.equal(y.view(torch.int16), y0.view(torch.int16)), off
    return y0


@pytest.mark.parametrize("T,K,N,with_bias,max_code", E.k12_cases())
def test_k12_w8_forward_is_exact(gpu, T, K, N, with_bias, max_code):
    g = torch.Generator().manual_seed(E.seed_of(12, T, K, N, max_code))
    x, q, scale, zero, bias = E.k12_data(g, T, K, N, with_bias, max_code)
    y_ref, _, pre = E.k12_expect(x, q, scale, zero, bias)
    E.check_pre(pre)
    _check_k12(gpu, x, q, scale, zero, bias, y_ref)


@pytest.mark.parametrize("name,shape,positive,row,k,value", E.K12_NONFINITE, ids=[c[0] for c in E.K12_NONFINITE])
def test_k12_bad_token_row_stays_in_its_row(gpu, name, shape, positive, row, k, value):
    """a NaN / +Inf / -Inf in one token row: the other rows do not move, and the row itself has the reference's class (NaN, +Inf, -Inf)
    element for element — nothing in the kernel multiplies a padding zero by an activation"""
    T, K, N = shape
    g = torch.Generator().manual_seed(E.seed_of(120, *shape))
    x, q, scale, zero, bias = E.k12_data(g, T, K, N, True, 255, positive)
    y_ref, _, pre = E.k12_expect(x, q, scale, zero, bias)
    E.check_pre(pre)
    _check_k12(gpu, x, q, scale, zero, bias, y_ref)
    xb = E.with_bad_value(x, row, k, value)
    want = y_ref.clone()
    want[row] = E.k12_row_ref(xb[row], q, scale, zero, bias)
    assert not bool(torch.isfinite(want[row]).any())
    y1 = _check_k12(gpu, xb, q, scale, zero, bias, want)   # `same`: NaN where NaN, +-Inf where +-Inf, every finite element equal
    assert torch.equal(E.value_class(y1.cpu()), E.value_class(want))


def test_k12_cases_reach_every_dispatch_class(gpu):
    """the host dispatch of asvd_w8_linear_f16 restated (for counting only) with this device's CU count: feature tiles of 8, 16 and 32, each
    with 16-byte and with element loads, each with K % 128 == 0, < 16 and >= 16 with a partial chunk; and every `nkfull mod 8`, i.e. every
    split of the whole iterations into groups of W8_U and leftover single iterations per wave"""
    classes = {}
    for T, K, N, _, _ in E.k12_cases():
        for off, ld_ok in E.k12_views(K):
            c = E.k12_class(T, K, N, _cus(), ld_ok and off % 16 == 0)
            classes[c] = classes.get(c, 0) + 1
    print(classes)
    missing = E.k12_missing(set(classes))
    assert not missing, missing


# ---- w8_dequant -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_w8_dequant_vs_fp32_restatement(gpu, dt):
    """every code in every row, random scale and zero, against torch-CPU fp32 `(scale * (q - zero)).to(dtype)`, through the 16-byte kernel
    (aligned codes) and the element kernel (a view at column offset 5)"""
    from asvd4llm_amd import ops
    q, scale, zero = E.dequant_data(torch.Generator().manual_seed(5))
    want = E.dequant_expect(q, scale, zero, E.DTYPES[dt])
    assert bool(torch.isfinite(want).all())
    got = ops.w8_dequant(q.to(gpu), scale.to(gpu), zero.to(gpu), E.DTYPES[dt])
    assert same(got, want), where_differs(got, want)
    big = torch.zeros((q.shape[0], q.shape[1] + 32), dtype=torch.uint8, device=gpu)
    big[:, 5:5 + q.shape[1]] = q.to(gpu)
    got = ops.w8_dequant(big[:, 5:5 + q.shape[1]], scale.to(gpu), zero.to(gpu), E.DTYPES[dt])
    assert same(got, want), where_differs(got, want)


# ---- K9 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,r,wdt,abdt,path,strided", E.k9_cases())
def test_k9_reconstruct_err_is_exact(gpu, m, n, r, wdt, abdt, path, strided):
    """W = A B + d with integer factors and a sparse d in {-1, 0, 1}: out = (sum d^2, sum W^2), both exact integers, compared with ==.
    path: the one-launch kernel, the three-launch kernel (n % 8 != 0, or a B that is not 16-byte aligned) and the fp32-factor kernel"""
    from asvd4llm_amd import ops
    A, B, Wt, e2, w2, pre = E.k9_expect(m, n, r, E.DTYPES[wdt])
    E.check_pre(pre)
    Ad = A.to(E.DTYPES[abdt]).to(gpu)
    if path == "padded" and n % 8 == 0:   # contiguous, but starting one element off a 16-byte boundary: the entry takes the three-launch path
        buf = torch.empty(r * n + 8, dtype=E.DTYPES[abdt], device=gpu)
        Bd = buf[1:1 + r * n].view(r, n)
        Bd.copy_(B.to(E.DTYPES[abdt]))
        assert Bd.is_contiguous() and Bd.data_ptr() % 16 != 0
    else:
        Bd = B.to(E.DTYPES[abdt]).to(gpu)
        assert Bd.data_ptr() % 16 == 0
    if strided:                           # a column slice of a wider matrix: ldw > n
        big = torch.full((m, n + 24), 3.0, dtype=E.DTYPES[wdt], device=gpu)
        big[:, 8:8 + n] = Wt.to(gpu)
        Wd = big[:, 8:8 + n]
        assert Wd.stride(0) > n
    else:
        Wd = Wt.to(gpu)
    out = ops.reconstruct_err(Wd, Ad, Bd).cpu()
    want = torch.tensor([e2, w2], dtype=torch.float64)
    assert torch.equal(out, want), (out.tolist(), want.tolist(), (out - want).tolist())


# ---- K8 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("m,n", E.K8_SHAPES)
def test_k8_fro_norm_sq_is_exact(gpu, m, n, dt):
    from asvd4llm_amd import ops
    W = E.k8_data(torch.Generator().manual_seed(E.seed_of(8, m, n)), m, n)
    ss, pre = E.k8_expect(W)
    E.check_pre(pre)
    Wd = W.to(E.DTYPES[dt]).to(gpu)
    assert ops.fro_norm_sq(Wd).item() == ss
    if n > 8:   # a strided view: columns 3 .. n - 4 of the same matrix
        ssv, pre = E.k8_expect(W[:, 3:n - 4])
        assert ops.fro_norm_sq(Wd[:, 3:n - 4]).item() == ssv


# ---- K1/K2 ------------------------------------------------------------------------------------------------------------------------

def _absstat_views(x, gpu):
    """(name, device view) of one host matrix: contiguous; a strided view whose rows keep their 16-byte alignment; a view whose base is one
    element off (the kernel's element-load branch)"""
    rows, cols = x.shape
    out = [("contiguous", x.to(gpu))]
    for name, off in (("strided", 0), ("misaligned", 1)):
        big = torch.full((rows, cols + 16), 9.0, dtype=x.dtype, device=gpu)
        big[:, off:off + cols] = x.to(gpu)
        out.append((name, big[:, off:off + cols]))
    return out


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("cols", E.ABSSTAT_COLS)
@pytest.mark.parametrize("rows", E.ABSSTAT_ROWS)
def test_absstat_is_exact(gpu, rows, cols, dt):
    """three accumulating hook calls in each mode: the accumulator equals, bit for bit, both the kernel's stated contract
    (exact_data.absstat_expect) and the CPU oracle.  The views (strided, misaligned base) must give the same bits as the contiguous tensor."""
    from asvd4llm_amd import ops
    dtype = E.DTYPES[dt]
    g = torch.Generator().manual_seed(E.seed_of(1, rows, cols, dt))
    xs = [E.absstat_data(g, rows, cols, dtype) for _ in range(3)]
    with_views = (rows, cols) in ((37, 100), (2047, 4096), (2048, 64), (1, 11008))
    for method in E.ABSSTAT_MODES:
        want, oracle = torch.zeros(cols, dtype=dtype), None
        accs = {name: torch.zeros(cols, dtype=dtype, device=gpu) for name in (("contiguous", "strided", "misaligned") if with_views else ("contiguous",))}
        for x in xs:
            want, pre = E.absstat_expect(want, x, method)
            E.check_pre(pre)
            oracle = E.absstat_oracle(oracle, x, method)
            assert torch.equal(want, oracle)
            for name, xv in _absstat_views(x, gpu) if with_views else [("contiguous", x.to(gpu))]:
                ops.absstat_accum(xv, accs[name], method)
                assert same(accs[name], want), (method, name, where_differs(accs[name], want))


@pytest.mark.parametrize("method", E.ABSSTAT_MODES)
@pytest.mark.parametrize("rows,cols", [(37, 100), (2047, 4096), (2048, 11008)])
def test_absstat_partial_then_finalize_into_two_accumulators(gpu, rows, cols, method):
    """what the calibration hook calls: ONE absstat_partial, then absstat_finalize into the accumulators of the Linears that share the input —
    here two of different dtype and different prior contents.  Each must equal absstat_accum on its own, and the contract."""
    from asvd4llm_amd import ops
    g = torch.Generator().manual_seed(E.seed_of(2, rows, cols, method))
    x = E.absstat_data(g, rows, cols, torch.float16)
    priors = [torch.randint(0, 8, (cols,), generator=g).to(torch.float16), (torch.randint(0, 64, (cols,), generator=g) / 8).to(torch.float32)]
    xd = x.to(gpu)
    work = ops.absstat_partial(xd, method)
    for prior in priors:
        want, pre = E.absstat_expect(prior, x, method)
        E.check_pre(pre)
        acc = ops.absstat_finalize(work, rows, cols, prior.clone().to(gpu), method)
        alone = ops.absstat_accum(xd, prior.clone().to(gpu), method)
        assert torch.equal(acc, alone)
        assert same(acc, want), (method, prior.dtype, where_differs(acc, want))
