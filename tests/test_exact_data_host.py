"""The exact-data references of tests/exact_data.py, on the CPU alone: for every case of tests/test_gpu_exact_data.py the order-independence
preconditions hold, and the expected output contains what the case claims to exercise (entries that need rounding, exact ties, fp16
overflow, non-finite rows).  Nothing here touches the library: it shows that the references stay within the exactness conditions."""
import pytest
import torch

from tests import exact_data as E


@pytest.mark.parametrize("T,K,r,N,with_bias", E.K10_SHAPES)
def test_k10_preconditions(T, K, r, N, with_bias):
    g = torch.Generator().manual_seed(E.seed_of(10, T, K, r, N))
    x, B, A, bias = E.k10_data(g, T, K, r, N, with_bias)
    z_ref, y_ref, pre = E.k10_expect(x, B, A, bias)
    E.check_pre(pre)
    assert z_ref.shape == (T, r) and y_ref.shape == (T, N) and bool(torch.isfinite(y_ref).all())
    assert (bias is not None) == with_bias
    if (T, K, r, N) in E.K10_BIG:
        rounded, ties, inf = E.round_stats(E.k10_y64(x, B, A, bias))
        print(f"K10 {(T, K, r, N)}: {rounded} of {y_ref.numel()} entries rounded, {ties} exact ties, |z| <= {z_ref.abs().max().item()}")
        assert rounded >= y_ref.numel() // 4 and ties >= 100 and inf == 0   # the rounding mode is exercised
        assert bool((z_ref.abs() <= 2048).all())                             # z itself is exact in fp16


@pytest.mark.parametrize("T,K,r,N,with_bias", E.K10_WIDE_X)
def test_k10_wide_x_rounds_z_and_saturates_y(T, K, r, N, with_bias):
    g = torch.Generator().manual_seed(E.seed_of(13, T, K, r, N))
    x, B, A, bias = E.k10_data(g, T, K, r, N, with_bias, xmax=60)
    z_ref, y_ref, pre = E.k10_expect(x, B, A, bias)
    E.check_pre(pre)
    zr, zt, zi = E.round_stats(x.double() @ B.double().T)
    yr, yt, yi = E.round_stats(E.k10_y64(x, B, A, bias))
    print(f"K10 wide x {(T, K, r, N)}: z {zr} of {z_ref.numel()} rounded, {zt} ties; y {yr} of {y_ref.numel()} rounded, {yt} ties, {yi} overflow to Inf")
    assert zr >= z_ref.numel() // 20 and zt >= 100 and zi == 0      # the FIRST rounding point is exercised, ties included
    assert yr >= y_ref.numel() // 4 and yi >= 100 and yi < y_ref.numel() // 2 and int(torch.isinf(y_ref).sum()) == yi


def test_k10_case_list_covers_what_it_names():
    shapes = {(T, K, r, N) for T, K, r, N, _ in E.K10_SHAPES}
    assert all(s in shapes for s in E.K10_BIG)
    assert {T for T, K, r, N in shapes if (K, r, N) == E.K10_MID} == set(E.K10_TOKENS)
    assert any(T <= 4 and K == 13824 for T, K, r, N in shapes) and (4, 11264, 512, 1024) in shapes
    assert {r for T, K, r, N in shapes} >= {1, 63, 64, 65} and {N for T, K, r, N in shapes} >= {1, 15, 17, 33, 70}
    assert {b for *_, b in E.K10_SHAPES} == {True, False}
    # on the 256 CUs of an MI355X every dispatch class is populated (the GPU test repeats this with the device's own count)
    missing = E.k10_missing({E.k10_class(T, K, r, N, 256) for T, K, r, N in shapes})
    assert not missing, missing


@pytest.mark.parametrize("T,K,N,with_bias,max_code", E.k12_cases())
def test_k12_preconditions(T, K, N, with_bias, max_code):
    g = torch.Generator().manual_seed(E.seed_of(12, T, K, N, max_code))
    x, q, scale, zero, bias = E.k12_data(g, T, K, N, with_bias, max_code)
    y_ref, y64, pre = E.k12_expect(x, q, scale, zero, bias)   # asserts that scale (q - zero) is exact in fp16
    E.check_pre(pre)
    assert int(q.max()) <= max_code
    if K >= 2:
        assert bool((q == 0).any(1).all()) and bool((q == max_code).any(1).all())   # both ends of the code range in every row
    if N >= 32:
        assert bool((zero == 0).any()) and bool((zero == max_code).any()) and bool((zero != zero.floor()).any()) and bool((scale == 4).any())
    if (T, K, N) in E.K12_BIG:
        rounded, ties, inf = E.round_stats(y64)
        print(f"K12 {(T, K, N)} codes <= {max_code}: {rounded} of {y_ref.numel()} entries rounded, {ties} exact ties, {inf} overflow to Inf")
        assert rounded >= y_ref.numel() // 16 and ties >= 100
        if max_code == 255:
            assert inf >= 1 and int(torch.isinf(y_ref).sum()) == inf   # the scale-4 rows saturate fp16: pinned


def test_k12_case_list_covers_what_it_names():
    cases = E.k12_cases()
    assert {T for T, *_ in cases} >= set(E.K12_TOKENS)
    assert {K for _, K, *_ in cases} >= {1, 8, 15, 16, 17, 127, 128, 129, 144, 352, 1001} | {128 * j for j in range(1, 10)}
    assert {(N, K) for _, K, N, *_ in cases} >= {(4096, 4096), (11008, 4096), (4096, 11008)}
    assert {mc for *_, mc in cases} == {255, 63}
    classes = set()
    for T, K, N, _, _ in cases:
        for off, ld_ok in E.k12_views(K):
            classes.add(E.k12_class(T, K, N, 256, ld_ok and off % 16 == 0))
    missing = E.k12_missing(classes)
    assert not missing, missing


@pytest.mark.parametrize("m,n,r", E.K9_SHAPES)
@pytest.mark.parametrize("wdt", ["f32", "f16", "bf16"])
def test_k9_preconditions(m, n, r, wdt):
    A, B, Wt, e2, w2, pre = E.k9_expect(m, n, r, E.DTYPES[wdt])   # asserts that W is exact in its dtype
    E.check_pre(pre)
    assert e2 >= 1 and w2 > e2 and e2 == int(e2) and w2 == int(w2)
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(A.to(dt).double(), A) and torch.equal(B.to(dt).double(), B)


def test_k9_case_list_crosses_paths_dtypes_and_layouts():
    cases = E.k9_cases()
    for path, abs_ in (("fused", ("f16", "bf16")), ("padded", ("f16", "bf16")), ("f32", ("f32",))):
        have = {(w, a, s) for m, n, r, w, a, p, s in cases if p == path}
        assert have == {(w, a, s) for w in ("f32", "f16", "bf16") for a in abs_ for s in (False, True)}, path
    assert {(m, n, r) for m, n, r, *_ in cases} == set(E.K9_SHAPES)
    assert all(n % 8 == 0 for m, n, r, w, a, p, s in cases if p == "fused")


@pytest.mark.parametrize("m,n", E.K8_SHAPES)
def test_k8_preconditions(m, n):
    W = E.k8_data(torch.Generator().manual_seed(E.seed_of(8, m, n)), m, n)
    ss, pre = E.k8_expect(W)
    E.check_pre(pre)
    assert ss >= 1 and int(W.abs().max()) <= 2
    for dt in E.DTYPES.values():
        assert torch.equal(W.to(dt).double(), W.double())


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("rows,cols", [(r, c) for r in E.ABSSTAT_ROWS for c in (64, 100)] + [(2047, 4096), (2048, 11008)])
def test_absstat_restatement_equals_the_oracle(rows, cols, dt):
    """the contract restated in exact_data.absstat_expect against oracle.hook_update / fisher_update (the reference hook's torch-CPU ops), bit
    for bit over three accumulating calls; the GPU test must equal both"""
    dtype = E.DTYPES[dt]
    g = torch.Generator().manual_seed(E.seed_of(1, rows, cols, dt))
    xs = [E.absstat_data(g, rows, cols, dtype) for _ in range(3)]
    for method in E.ABSSTAT_MODES:
        acc, want = torch.zeros(cols, dtype=dtype), None
        for x in xs:
            acc, pre = E.absstat_expect(acc, x, method)
            E.check_pre(pre)
            want = E.absstat_oracle(want, x, method)
            assert torch.equal(acc, want), (method, rows, cols, dt)
        assert bool((acc > 0).any())
    if rows > 1:
        mean, _ = E.absstat_expect(torch.zeros(cols, dtype=dtype), xs[0], "abs_mean")
        exact = xs[0].double().abs().mean(0)
        assert rows in (2048,) or bool((mean.double() != exact).any())   # the divide rounds (rows no power of two): the rounding points matter


@pytest.mark.parametrize("name,shape,positive,row,k,value", E.K10_NONFINITE, ids=[c[0] for c in E.K10_NONFINITE])
def test_k10_nonfinite_cases(name, shape, positive, row, k, value):
    T, K, r, N = shape
    g = torch.Generator().manual_seed(E.seed_of(100, *shape))
    x, B, A, bias = E.k10_data(g, T, K, r, N, True, positive)
    z_ref, y_ref, pre = E.k10_expect(x, B, A, bias)
    E.check_pre(pre)
    bad = E.k10_row_ref(E.with_bad_value(x, row, k, value)[row], B, A, bias)
    assert not bool(torch.isfinite(bad).any())                       # the whole row is lost in the reference
    if value == float("inf"):
        assert bool((bad == float("inf")).all())                     # positive weights: +Inf, not NaN
        assert K - k <= 8 or "last8" not in name
        sat = int(torch.isinf(y_ref).sum())
        print(f"K10 {name}: {sat} of {y_ref.numel()} finite-input entries saturate fp16")
        assert 0 < sat < y_ref.numel()                       # fp16 output saturation of rows with finite inputs


@pytest.mark.parametrize("name,shape,positive,row,k,value", E.K12_NONFINITE, ids=[c[0] for c in E.K12_NONFINITE])
def test_k12_nonfinite_cases(name, shape, positive, row, k, value):
    T, K, N = shape
    g = torch.Generator().manual_seed(E.seed_of(120, *shape))
    x, q, scale, zero, bias = E.k12_data(g, T, K, N, True, 255, positive)
    y_ref, y64, pre = E.k12_expect(x, q, scale, zero, bias)
    E.check_pre(pre)
    bad = E.k12_row_ref(E.with_bad_value(x, row, k, value)[row], q, scale, zero, bias)
    want = 1 if value != value else (2 if value > 0 else 3)
    assert bool((E.value_class(bad) == want).all())                  # NaN / +Inf / -Inf over the whole row, nothing mixed


def test_dequant_data_has_every_code_in_every_row():
    q, scale, zero = E.dequant_data(torch.Generator().manual_seed(5))
    assert all(len(set(row.tolist())) == 256 for row in q) and q.shape[1] % 16 == 0
    assert bool((scale > 0).all()) and bool(torch.isfinite(E.dequant_expect(q, scale, zero, torch.float16)).all())
