"""torch-tensor front end of the C ABI (include/asvd_hip.h).  torch is used for device memory and streams only —
every arithmetic step below runs in libasvd_hip.so.  Tensors must live on a gfx950 device; nothing falls back to CPU."""
import ctypes
import os

import torch

from . import _lib as L

_DT = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}")


def _dev(t, name):
    if not t.is_cuda:
        raise L.AsvdHipError(f"{name} must be a device tensor (got {t.device}); the ASVD hot path has no CPU fallback")
    return t


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class _NoCtx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NOCTX = _NoCtx()


def _on(device):
    """context that makes `device` current — nothing at all when it already is (torch.cuda.device costs several microseconds per call,
    which is most of a decode-sized launch)"""
    return _NOCTX if torch.cuda.current_device() == device.index else torch.cuda.device(device)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _work(nbytes, device):
    w = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    fill = os.environ.get("ASVD_DEBUG_WORKFILL")  # debug: poison (255 -> NaN patterns) or zero the workspace to expose reads of unwritten memory
    if fill is not None:
        w.fill_(int(fill))
    return w


def absstat_accum(x2d, acc, method):
    """acc (in place) <- hook update with |x| column statistic over rows of x2d [rows, cols] (act_aware_utils.py:64-74)"""
    lib = L.load(True)
    _dev(x2d, "x"), _dev(acc, "acc")
    assert x2d.dim() == 2 and x2d.stride(1) == 1 and acc.is_contiguous() and acc.numel() == x2d.shape[1]
    rows, cols = x2d.shape
    mode = L.STAT_SQ_MEAN if method == "sq_mean" else (L.STAT_ABS_MEAN if "abs_mean" in method else L.STAT_ABS_MAX)
    nb = ctypes.c_size_t()
    L.check(lib.asvd_absstat_worksize(rows, cols, ctypes.byref(nb)), "asvd_absstat_worksize")
    work = _work(nb.value, x2d.device)
    with _on(x2d.device):
        L.check(lib.asvd_absstat_accum(_ptr(x2d), _dt(x2d), rows, cols, x2d.stride(0), _ptr(acc), _dt(acc), mode, _ptr(work),
                                       work.numel(), _stream(x2d)), "asvd_absstat_accum")
    return acc


def _stat_mode(method):
    return L.STAT_SQ_MEAN if method == "sq_mean" else (L.STAT_ABS_MEAN if "abs_mean" in method else L.STAT_ABS_MAX)


def absstat_partial(x2d, method):
    """first half of absstat_accum: ONE pass over x2d, fp32 partial statistics in a workspace tensor (returned) that
    absstat_finalize applies to any number of accumulators (Linears that share this input)"""
    lib = L.load(True)
    _dev(x2d, "x")
    assert x2d.dim() == 2 and x2d.stride(1) == 1
    rows, cols = x2d.shape
    nb = ctypes.c_size_t()
    L.check(lib.asvd_absstat_worksize(rows, cols, ctypes.byref(nb)), "asvd_absstat_worksize")
    work = _work(nb.value, x2d.device)
    with _on(x2d.device):
        L.check(lib.asvd_absstat_partial(_ptr(x2d), _dt(x2d), rows, cols, x2d.stride(0), _stat_mode(method), _ptr(work), work.numel(), _stream(x2d)),
                "asvd_absstat_partial")
    return work


def absstat_finalize(work, rows, cols, acc, method):
    lib = L.load(True)
    _dev(acc, "acc")
    assert acc.is_contiguous() and acc.numel() == cols
    with _on(acc.device):
        L.check(lib.asvd_absstat_finalize(_ptr(work), work.numel(), rows, cols, _ptr(acc), _dt(acc), _stat_mode(method), _stream(acc)),
                "asvd_absstat_finalize")
    return acc


def make_scale(scaling, fisher=None, alpha=1.0, eps=1e-6):
    """s = scaling**alpha [* fisher**alpha] + eps in the dtype of `scaling` (svd_linear.py:48-59)"""
    lib = L.load(True)
    _dev(scaling, "scaling")
    scaling = scaling.contiguous()
    if fisher is not None:
        fisher = fisher.to(scaling.dtype).contiguous()
    out = torch.empty_like(scaling)
    with torch.cuda.device(scaling.device):
        L.check(lib.asvd_make_scale(_ptr(scaling), _ptr(fisher), _dt(scaling), scaling.numel(), float(alpha), float(eps), _ptr(out),
                                    _stream(scaling)), "asvd_make_scale")
    return out


def make_scale_batched(scalings, fishers=None, alpha=1.0, eps=1e-6):
    """batched make_scale (asvd_make_scale_batched): one ABI call for a list of same-length, same-dtype statistics vectors"""
    lib = L.load(True)
    B = len(scalings)
    scalings = [_dev(s, "scaling").contiguous() for s in scalings]
    n, dt = scalings[0].numel(), scalings[0].dtype
    assert all(s.numel() == n and s.dtype == dt for s in scalings)
    if fishers is not None:
        fishers = [None if f is None else f.to(dt).contiguous() for f in fishers]
    outs = [torch.empty_like(s) for s in scalings]
    arr = ctypes.c_void_p * B
    f_p = arr(*[(f.data_ptr() if f is not None else None) for f in fishers]) if fishers is not None else None
    with torch.cuda.device(scalings[0].device):
        L.check(lib.asvd_make_scale_batched(B, arr(*[s.data_ptr() for s in scalings]), f_p, _dt(scalings[0]), n, float(alpha), float(eps),
                                            arr(*[o.data_ptr() for o in outs]), _stream(scalings[0])), "asvd_make_scale_batched")
    return outs


def scale_cols(w, s=None):
    """fp32 w * s[None, :] (svd_linear.py:47,60)"""
    lib = L.load(True)
    _dev(w, "w")
    assert w.dim() == 2 and w.stride(1) == 1
    m, n = w.shape
    out = torch.empty((m, n), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        L.check(lib.asvd_scale_cols(_ptr(w), _dt(w), m, n, w.stride(0), _ptr(s), _dt(s) if s is not None else 0, _ptr(out), n,
                                    _stream(w)), "asvd_scale_cols")
    return out


class SvdInfo:
    """per-problem {status, sweeps, pairs rotated in the last sweep} + the path bits of the CALL the problem was part of
    (asvd_svd_get_last_path: reduced / reduce_fallback / plain_retry / split / split_refused / gram_retry)"""

    def __init__(self, status, sweeps, last_rot, path=0):
        self.status, self.sweeps, self.last_rotated_pairs, self.path = status, sweeps, last_rot, path
        self.reorth = None  # ReorthInfo of the long side's vectors when the call ran with ortho=True
        self.reduced = bool(path & L.PATH_REDUCED)
        self.reduce_fallback = bool(path & L.PATH_REDUCE_FALLBACK)
        self.plain_retry = bool(path & L.PATH_PLAIN_RETRY)
        self.split = bool(path & L.PATH_SPLIT)
        self.split_refused = bool(path & L.PATH_SPLIT_REFUSED)
        self.gram_retry = bool(path & L.PATH_GRAM_RETRY)

    def __repr__(self):
        return (f"SvdInfo(status={self.status}, sweeps={self.sweeps}, last_rotated_pairs={self.last_rotated_pairs}, reduced={self.reduced}, "
                f"reduce_fallback={self.reduce_fallback}, plain_retry={self.plain_retry}, split={self.split}, gram_retry={self.gram_retry})")


class ReorthInfo:
    """per-problem result of asvd_reorth_batched: status (0, N_NOCONV, N_NAN), passes made, max |Q^T Q - I| at entry and measured at exit"""

    def __init__(self, status, passes, e_before, e_after):
        self.status, self.passes, self.e_before, self.e_after = status, passes, e_before, e_after

    def __repr__(self):
        return f"ReorthInfo(status={self.status}, passes={self.passes}, e_before={self.e_before:.3g}, e_after={self.e_after:.3g})"


def _bits_to_float(i):
    return ctypes.c_float.from_buffer(ctypes.c_int(i)).value


def reorth_batched(Qs, max_passes=0, tol=0.0):
    """Make the columns of every Q [m, k] (same shape and row stride, fp32, m >= k) orthonormal IN PLACE and in their given order
    (asvd_reorth_batched: Q <- Q - Q (striu(E) + diag(E) / 2), E = Q^T Q - I, until max |E| <= tol).  Returns [ReorthInfo]; a problem that
    is refused (entry max |E| > 0.25 or non-finite) is left untouched with a positive status."""
    lib = L.load(True)
    B = len(Qs)
    assert B >= 1
    m, k = Qs[0].shape
    dev = Qs[0].device
    for q in Qs:
        _dev(q, "Q")
        assert q.shape == (m, k) and q.dtype == torch.float32 and q.stride(1) == 1 and q.stride(0) == Qs[0].stride(0)
    ldq = Qs[0].stride(0) if m > 1 else max(Qs[0].stride(0), k)
    nb = ctypes.c_size_t()
    L.check(lib.asvd_reorth_worksize(B, m, k, ctypes.byref(nb)), "asvd_reorth_worksize")
    work = _work(nb.value, dev)
    arr = ctypes.c_void_p * B
    info = (ctypes.c_int * (4 * B))()
    with torch.cuda.device(dev):
        rc = lib.asvd_reorth_batched(B, arr(*[q.data_ptr() for q in Qs]), m, k, ldq, int(max_passes), float(tol), _ptr(work), work.numel(), info,
                                     _stream(Qs[0]))
    L.check(rc, "asvd_reorth_batched")
    return [ReorthInfo(info[4 * b], info[4 * b + 1], _bits_to_float(info[4 * b + 2]), _bits_to_float(info[4 * b + 3])) for b in range(B)]


def reorth(Q, max_passes=0, tol=0.0):
    return reorth_batched([Q], max_passes, tol)[0]


def svd_batched(mats, col_scales=None, k=None, want_vectors=True, max_sweeps=0, tol=0.0, ortho=False):
    """Economy SVD of a list of same-shape device matrices: mats[b] * diag(col_scales[b]) = U S V^T.
    Returns (U list [m,k], S list [k], V list [n,k], infos).  U/V lists are None when want_vectors is False.
    ortho (with vectors): the long side's vectors (U when m >= n, else V) go through reorth_batched after the factorisation — S and the short
    side are not touched, infos[b].reorth holds the ReorthInfo (a refused or unconverged pass is reported there, not raised)."""
    lib = L.load(True)
    B = len(mats)
    assert B >= 1
    m, n = mats[0].shape
    dev = mats[0].device
    for a in mats:
        _dev(a, "matrix")
        assert a.shape == (m, n) and a.dtype == mats[0].dtype and a.stride(1) == 1 and a.stride(0) == mats[0].stride(0)
    kmax = min(m, n)
    k = kmax if k is None else int(k)
    assert 1 <= k <= kmax
    nb = ctypes.c_size_t()
    L.check(lib.asvd_svd_worksize(B, m, n, 1 if want_vectors else 0, ctypes.byref(nb)), "asvd_svd_worksize")
    work = _work(nb.value, dev)
    S = [torch.empty(k, dtype=torch.float32, device=dev) for _ in range(B)]
    U = [torch.empty((m, k), dtype=torch.float32, device=dev) for _ in range(B)] if want_vectors else None
    V = [torch.empty((n, k), dtype=torch.float32, device=dev) for _ in range(B)] if want_vectors else None
    arr = ctypes.c_void_p * B
    a_p = arr(*[a.data_ptr() for a in mats])
    s_p = arr(*[s.data_ptr() for s in S])
    u_p = arr(*[u.data_ptr() for u in U]) if want_vectors else None
    v_p = arr(*[v.data_ptr() for v in V]) if want_vectors else None
    if col_scales is not None:
        for s in col_scales:
            _dev(s, "col_scale")
            assert s.numel() == n and s.is_contiguous() and s.dtype == col_scales[0].dtype
        c_p = arr(*[s.data_ptr() for s in col_scales])
        cdt = _dt(col_scales[0])
    else:
        c_p, cdt = None, 0
    info = (ctypes.c_int * (4 * B))()
    with torch.cuda.device(dev):
        rc = lib.asvd_svd_batched(B, a_p, _dt(mats[0]), m, n, mats[0].stride(0), c_p, cdt, u_p, s_p, v_p, k, int(max_sweeps),
                                  float(tol), _ptr(work), work.numel(), info, _stream(mats[0]))
        path = int(lib.asvd_svd_get_last_path())
    L.check(rc, "asvd_svd_batched")
    infos = [SvdInfo(info[4 * b], info[4 * b + 1], info[4 * b + 2], path) for b in range(B)]
    if ortho and want_vectors:
        del work  # the SVD's workspace (23.9 GiB for 32 x 4096^2) goes back to the allocator before the pass takes its own
        for i, r in zip(infos, reorth_batched(U if m >= n else V)):
            i.reorth = r
    return U, S, V, infos


def svd(a, col_scale=None, k=None, want_vectors=True, max_sweeps=0, tol=0.0, ortho=False):
    U, S, V, infos = svd_batched([a], None if col_scale is None else [col_scale], k, want_vectors, max_sweeps, tol, ortho)
    if want_vectors:
        return U[0], S[0], V[0], infos[0]
    return None, S[0], None, infos[0]


SIGMA_MAX_COLS = 16384  # asvd_sigma_max_batched keeps the Lanczos vector in LDS


def sigma_max_batched(mats, max_steps=0, tol=0.0):
    """Largest singular value of each matrix of a same-shape list (Lanczos, asvd_sigma_max_batched).
    Returns (list of 0-dim fp32 device tensors, list of (status, steps)).  Matrices with more than SIGMA_MAX_COLS columns,
    and any problem the Lanczos iteration reports as not converged, go through the values-only k=1 mode of the Jacobi SVD."""
    lib = L.load(True)
    B = len(mats)
    assert B >= 1
    m, n = mats[0].shape
    dev = mats[0].device
    for a in mats:
        _dev(a, "matrix")
        assert a.shape == (m, n) and a.dtype == mats[0].dtype and a.stride(1) == 1 and a.stride(0) == mats[0].stride(0)
    if n > SIGMA_MAX_COLS:
        _, S, _, infos = svd_batched(mats, None, k=1, want_vectors=False)
        return [s[0] for s in S], [(i.status, -i.sweeps) for i in infos]
    nb = ctypes.c_size_t()
    L.check(lib.asvd_sigma_max_worksize(B, m, n, int(max_steps), ctypes.byref(nb)), "asvd_sigma_max_worksize")
    work = _work(nb.value, dev)
    out = torch.empty(B, dtype=torch.float32, device=dev)
    arr = ctypes.c_void_p * B
    a_p = arr(*[a.data_ptr() for a in mats])
    o_p = arr(*[out.data_ptr() + 4 * b for b in range(B)])
    info = (ctypes.c_int * (2 * B))()
    with torch.cuda.device(dev):
        rc = lib.asvd_sigma_max_batched(B, a_p, _dt(mats[0]), m, n, mats[0].stride(0), o_p, int(max_steps), float(tol), _ptr(work),
                                        work.numel(), info, _stream(mats[0]))
    L.check(rc, "asvd_sigma_max_batched")
    sig = [out[b] for b in range(B)]
    infos = [(info[2 * b], info[2 * b + 1]) for b in range(B)]
    redo = [b for b in range(B) if infos[b][0] == 1]  # ASVD_N_NOCONV: still moving after max_steps
    if redo:
        _, S, _, jinfos = svd_batched([mats[b] for b in redo], None, k=1, want_vectors=False)
        for b, s, ji in zip(redo, S, jinfos):
            sig[b] = s[0]
            infos[b] = (ji.status, -ji.sweeps)
    return sig, infos


def truncate_split(U, S, V, s, r, sigma_fuse, out_dtype):
    """(A [m,r], B [r,n], nan_flags[3]) per SVDLinear.__init__ + un-scaling (svd_linear.py:69-70,16-24,102)"""
    lib = L.load(True)
    _dev(U, "U")
    m, n = U.shape[0], V.shape[0]
    assert U.stride(1) == 1 and V.stride(1) == 1 and U.shape[1] >= r and V.shape[1] >= r and S.numel() >= r
    A = torch.empty((m, r), dtype=out_dtype, device=U.device)
    Bm = torch.empty((r, n), dtype=out_dtype, device=U.device)
    flags = torch.zeros(3, dtype=torch.int32, device=U.device)
    with torch.cuda.device(U.device):
        L.check(lib.asvd_truncate_split(_ptr(U), U.stride(0), _ptr(S), _ptr(V), V.stride(0), _ptr(s), _dt(s) if s is not None else 0,
                                        m, n, r, L.FUSE[sigma_fuse], _ptr(A), _ptr(Bm), _DT[out_dtype], _ptr(flags), _stream(U)),
                "asvd_truncate_split")
    return A, Bm, flags


def truncate_split_batched(Us, Ss, Vs, ss, r, sigma_fuse, out_dtype):
    """batched truncate_split (asvd_truncate_split_batched) over same-shape problems: returns ([A], [B], flags [batch, 3])"""
    lib = L.load(True)
    B = len(Us)
    m, n = Us[0].shape[0], Vs[0].shape[0]
    dev = Us[0].device
    for U, S, V in zip(Us, Ss, Vs):
        _dev(U, "U")
        assert U.shape[0] == m and V.shape[0] == n and U.stride(1) == 1 and V.stride(1) == 1 and U.stride(0) == Us[0].stride(0) and V.stride(0) == Vs[0].stride(0)
        assert U.shape[1] >= r and V.shape[1] >= r and S.numel() >= r
    As = [torch.empty((m, r), dtype=out_dtype, device=dev) for _ in range(B)]
    Bs = [torch.empty((r, n), dtype=out_dtype, device=dev) for _ in range(B)]
    flags = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    arr = ctypes.c_void_p * B
    s_p = arr(*[(x.data_ptr() if x is not None else None) for x in ss]) if ss is not None else None
    sdt = _dt(ss[0]) if ss is not None and ss[0] is not None else 0
    with torch.cuda.device(dev):
        L.check(lib.asvd_truncate_split_batched(B, arr(*[u.data_ptr() for u in Us]), Us[0].stride(0), arr(*[x.data_ptr() for x in Ss]),
                                                arr(*[v.data_ptr() for v in Vs]), Vs[0].stride(0), s_p, sdt, m, n, r, L.FUSE[sigma_fuse],
                                                arr(*[a.data_ptr() for a in As]), arr(*[b.data_ptr() for b in Bs]), _DT[out_dtype], _ptr(flags),
                                                _stream(Us[0])), "asvd_truncate_split_batched")
    return As, Bs, flags


LOWRANK_MAX_TOKENS = 256  # ASVD_LOWRANK_MAX_TOKENS


def lowrank_pack(A, B):
    """Pad ALinear.weight [N, r] / BLinear.weight [r, K] (fp16, CUDA) to the layout asvd_lowrank_forward_f16 streams:
    (Ap [N, rp], Bp [rp, K], work) with rp = asvd_lowrank_padded_rank(r); work carries the zeroed barrier words."""
    lib = L.load(True)
    _dev(A, "A")
    N, r = A.shape
    K = B.shape[1]
    assert A.dtype == torch.float16 and B.dtype == torch.float16 and B.shape[0] == r
    if K % 64:
        raise ValueError(f"fused low-rank forward needs in_features % 64 == 0 (got {K})")
    rp = int(lib.asvd_lowrank_padded_rank(r))
    Ap = torch.zeros((N, rp), dtype=torch.float16, device=A.device)
    Ap[:, :r] = A
    Bp = torch.zeros((rp, K), dtype=torch.float16, device=A.device)
    Bp[:r] = B
    work = torch.zeros(int(lib.asvd_lowrank_work_bytes(LOWRANK_MAX_TOKENS, rp)), dtype=torch.uint8, device=A.device)
    return Ap, Bp, work


_LOWRANK_CALLS = {}   # launches since the last give-up check, PER WORKSPACE (every SVDLinear owns one): data_ptr -> count


def lowrank_check(work):
    """read (one host sync) and clear the give-up word of a fused-forward workspace; raises when a launch since the last check left its grid barrier"""
    _LOWRANK_CALLS[work.data_ptr()] = 0
    flags = work[:16].view(torch.int32)
    if int(flags[2].item()) != 0:
        flags[2] = 0
        raise L.AsvdHipError("asvd_lowrank_forward_f16 / asvd_lowrank_packed_f16: a workgroup gave up at the in-kernel grid barrier (the launch was not "
                             "fully resident); its output was poisoned with NaN.  Use the two launches (fused_forward / fused_packed = False) next to "
                             "persistent kernels of other streams.")


def lowrank_forward(x2d, Ap, Bp, bias, work):
    """y = fp16(fp16(x Bp^T) Ap^T + bias) in one launch (K10, svd_linear.py:105-109) for x2d [T <= 256, K] fp16"""
    lib = L.load(True)
    _dev(x2d, "x")
    T, K = x2d.shape
    N, rp = Ap.shape
    assert x2d.dtype == torch.float16 and x2d.is_contiguous() and Bp.shape == (rp, K) and 1 <= T <= LOWRANK_MAX_TOKENS
    y = torch.empty((T, N), dtype=torch.float16, device=x2d.device)
    with _on(x2d.device):
        L.check(lib.asvd_lowrank_forward_f16(_ptr(x2d), T, _ptr(Bp), _ptr(Ap), _ptr(bias), N, K, rp, _ptr(y), _ptr(work), work.numel(),
                                             _stream(x2d)), "asvd_lowrank_forward_f16")
    # word 2 of the barrier state: some workgroup left the in-kernel grid barrier without its peers (the workgroups of the launch were not all
    # resident); the kernel has poisoned what it wrote of y with NaN in that case.  The word is STICKY (only the host clears it), so it does not
    # have to be read after every launch: reading it is a host sync of ~18 us on a 21 us call (round 4 measured the fused forward "slower than
    # two GEMMs" under ASVD_STRICT for exactly that reason).  ASVD_STRICT checks every 64th launch OF EACH WORKSPACE (the counter is keyed by
    # the workspace: with one global counter only the modules that happened to make a 64th call were ever checked — ADVICE r5), ASVD_DEBUG
    # every launch; lowrank_check(work) reads it on demand (SVDLinear.check_fused_forward: call it at the end of a generate / eval loop).
    _lowrank_count(work)
    return y


def _lowrank_count(work):
    """one more launch on `work`; reads its give-up word under ASVD_DEBUG (every launch) and ASVD_STRICT (every 64th launch of the workspace)"""
    key = work.data_ptr()
    n = _LOWRANK_CALLS.get(key, 0) + 1
    _LOWRANK_CALLS[key] = n
    if os.environ.get("ASVD_DEBUG") or (os.environ.get("ASVD_STRICT") == "1" and n >= 64):
        lowrank_check(work)


def fro_norm_sq(w):
    lib = L.load(True)
    _dev(w, "w")
    assert w.dim() == 2 and w.stride(1) == 1
    m, n = w.shape
    nb = ctypes.c_size_t()
    L.check(lib.asvd_fro_worksize(m, n, ctypes.byref(nb)), "asvd_fro_worksize")
    work = _work(nb.value, w.device)
    out = torch.empty(1, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        L.check(lib.asvd_fro_norm_sq(_ptr(w), _dt(w), m, n, w.stride(0), _ptr(out), _ptr(work), work.numel(), _stream(w)),
                "asvd_fro_norm_sq")
    return out


def reconstruct_err(W, A, B):
    """(|W - A B|_F^2, |W|_F^2) as a device double[2] tensor"""
    lib = L.load(True)
    _dev(W, "W")
    m, n = W.shape
    r = A.shape[1]
    assert A.shape == (m, r) and B.shape == (r, n) and A.is_contiguous() and B.is_contiguous() and A.dtype == B.dtype
    nb = ctypes.c_size_t()
    L.check(lib.asvd_reconstruct_worksize(m, n, r, ctypes.byref(nb)), "asvd_reconstruct_worksize")
    work = _work(nb.value, W.device)
    out = torch.empty(2, dtype=torch.float64, device=W.device)
    with torch.cuda.device(W.device):
        L.check(lib.asvd_reconstruct_err(_ptr(W), _dt(W), W.stride(0), _ptr(A), _ptr(B), _dt(A), m, n, r, _ptr(out), _ptr(work),
                                         work.numel(), _stream(W)), "asvd_reconstruct_err")
    return out


GROUP_SIZES = (64, 128)   # K14: columns per scale / zero pair; 0 stands for one pair per row


def _group(group_size):
    g = int(group_size)
    if g != 0 and g not in GROUP_SIZES:
        raise ValueError(f"group_size must be 0 (per row), 64 or 128 (got {group_size})")
    return g


def n_groups(cols, group_size):
    """groups per row of `cols` columns: ceil(cols / group_size); the last one is shorter when cols is no multiple of it"""
    return (int(cols) + group_size - 1) // group_size


def _check_params(what, scale, zero, rows, cols, group, dev):
    """scale / zero fp32 contiguous on `dev`: [rows] per row (any shape of that many elements, as before), [rows, ng] per group"""
    ok = scale.dtype == torch.float32 and zero.dtype == torch.float32 and scale.is_contiguous() and zero.is_contiguous() \
        and scale.device == dev and zero.device == dev
    if group:
        shape = (rows, n_groups(cols, group))
        if not ok or tuple(scale.shape) != shape or tuple(zero.shape) != shape:
            raise ValueError(f"{what} with group_size={group} needs scale / zero {list(shape)} fp32 contiguous on the device of the codes "
                             f"(got {tuple(scale.shape)}, {tuple(zero.shape)})")
    elif not ok or scale.numel() != rows or zero.numel() != rows:
        raise ValueError(f"{what} needs scale / zero [{rows}] fp32 contiguous on the device of the codes")


MSE_MAX_CANDIDATES = 256   # RTN_MAX_CAND of csrc/rtn_quant.hip


def _mse_params(norm, grid, maxshrink):
    """the clip search's parameters as asvd_rtn_quant_mse_batched accepts them: (norm, grid, maxshrink) as float, int, float"""
    norm, maxshrink = float(norm), float(maxshrink)
    if int(grid) != grid:
        raise ValueError(f"mse_grid must be an integer (got {grid})")
    grid = int(grid)
    if not (0.0 < norm < float("inf")):
        raise ValueError(f"mse_norm must be positive and finite (got {norm})")
    if grid < 1:
        raise ValueError(f"mse_grid must be at least 1 (got {grid})")
    if not (0.0 < maxshrink <= 1.0):
        raise ValueError(f"mse_maxshrink must be in (0, 1] (got {maxshrink})")
    if not 1 <= int(maxshrink * grid) <= MSE_MAX_CANDIDATES:
        raise ValueError(f"int(mse_maxshrink * mse_grid) must be in 1..{MSE_MAX_CANDIDATES} candidates (got {int(maxshrink * grid)})")
    return norm, grid, maxshrink


def rtn_quant_batched(ws, bits, want_params=False, group_size=0, mse=False, mse_norm=2.4, mse_grid=100, mse_maxshrink=0.8):
    """Round-to-nearest fake quantization (quantization.py:17-21,31-145 with perchannel=True, sym=False, mse=False) of a list of 2-D
    device tensors of any shapes, strides (unit column stride) and dtypes, ONE launch per 16 of them (asvd_rtn_quant_batched), then one
    host sync for the per-tensor flags.  Returns one entry per tensor: the quantized tensor (new, contiguous, same dtype) — or the input
    tensor itself when one of its rows has scale 0, which the reference leaves unchanged (Quantizer.ready()).  want_params: the entry is
    (out, q, scale, zero, flagged) with q the uint8 codes [rows, cols] (0 where q is NaN) and scale / zero fp32 [rows].
    group_size 64 / 128 (K14, asvd_rtn_quant_grouped_batched): every group of that many columns of a row is quantized as a row of its own;
    scale / zero are [rows, ceil(cols / group_size)], and a tensor is flagged when one of its GROUPS has scale 0.
    mse (K15, asvd_rtn_quant_mse_batched): the reference Quantizer's mse=True.  Every row (or group) tries int(mse_maxshrink * mse_grid) ranges
    shrunk by p = 1 - i / mse_grid and keeps the scale / zero with the smallest sum |q(x) - x|^mse_norm (the lowest index among ties; a unit
    with a NaN, an Inf or scale 0 keeps its min / max pair); everything else — shapes, flags, the arithmetic of out and q — is unchanged."""
    lib = L.load(True)
    group = _group(group_size)
    if mse:
        mse_args = _mse_params(mse_norm, mse_grid, mse_maxshrink)
    if not 1 <= int(bits) <= 8:
        raise ValueError(f"bits must be in 1..8 (got {bits})")
    ws = list(ws)
    if not ws:
        return []
    dev = _dev(ws[0], "w").device
    for w in ws:
        _dev(w, "w")
        if w.dim() != 2 or w.stride(1) != 1 or w.device != dev:
            raise ValueError(f"rtn_quant needs 2-D tensors with unit column stride on one device (got {tuple(w.shape)}, stride {w.stride()}, {w.device})")
        _dt(w)
    B = len(ws)
    outs = [torch.empty(w.shape, dtype=w.dtype, device=dev) for w in ws]
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    if want_params:
        qs = [torch.empty(w.shape, dtype=torch.uint8, device=dev) for w in ws]
        pshape = (lambda w: (w.shape[0], n_groups(w.shape[1], group))) if group else (lambda w: (w.shape[0],))
        scales = [torch.empty(pshape(w), dtype=torch.float32, device=dev) for w in ws]
        zeros = [torch.empty(pshape(w), dtype=torch.float32, device=dev) for w in ws]
    vp, i64 = ctypes.c_void_p * B, ctypes.c_int64 * B
    ptrs = lambda ts: vp(*[t.data_ptr() for t in ts])  # noqa: E731
    args = (B, ptrs(ws), (ctypes.c_int * B)(*[_dt(w) for w in ws]), i64(*[w.shape[0] for w in ws]), i64(*[w.shape[1] for w in ws]),
            i64(*[w.stride(0) for w in ws]), int(bits), ptrs(outs), i64(*[w.shape[1] for w in ws]), ptrs(scales) if want_params else None,
            ptrs(zeros) if want_params else None, ptrs(qs) if want_params else None, _ptr(flags), _stream(ws[0]))
    with _on(dev):
        if mse:
            L.check(lib.asvd_rtn_quant_mse_batched(*args, group, *mse_args), "asvd_rtn_quant_mse_batched")
        elif group:
            L.check(lib.asvd_rtn_quant_grouped_batched(*args, group), "asvd_rtn_quant_grouped_batched")
        else:
            L.check(lib.asvd_rtn_quant_batched(*args), "asvd_rtn_quant_batched")
    flagged = [bool(f) for f in flags.tolist()]
    res = [w if f else o for w, o, f in zip(ws, outs, flagged)]
    if want_params:
        return [(o, q, s, z, f) for o, q, s, z, f in zip(res, qs, scales, zeros, flagged)]
    return res


def rtn_quant(w, bits, want_params=False, group_size=0, mse=False, mse_norm=2.4, mse_grid=100, mse_maxshrink=0.8):
    """rtn_quant_batched for one tensor"""
    return rtn_quant_batched([w], bits, want_params, group_size, mse, mse_norm, mse_grid, mse_maxshrink)[0]


W8_MAX_TOKENS = 256  # ASVD_W8_MAX_TOKENS (asvd_w8_linear_max_tokens)

ACT_DTYPES = (torch.float16, torch.bfloat16)   # activation types of the packed-weight forward kernels (K12 - K14, K16, K17; bf16: K19)


def _act_dtype(what, x2d, bias, weight_dtype):
    """the act_dtype argument of the asvd_*_a16 entries.  `weight_dtype` names the weight the codes stand for (a module passes
    self.weight_dtype), and the kernels form that weight in registers: x, bias and y are of that dtype, fp16 or bf16.  Raises ValueError before
    the library or the device is asked for."""
    if weight_dtype not in ACT_DTYPES:
        raise ValueError(f"{what}: weight_dtype must be torch.float16 or torch.bfloat16 (got {weight_dtype}); there is no fp32 forward kernel")
    if x2d.dtype != weight_dtype or (bias is not None and bias.dtype != weight_dtype):
        raise ValueError(f"{what} with weight_dtype={weight_dtype} needs x and bias of that dtype (got x {x2d.dtype}"
                         + (f", bias {bias.dtype})" if bias is not None else ")"))
    return _DT[weight_dtype]


def w8_linear(x2d, q, scale, zero, bias=None, group_size=0, weight_dtype=torch.float16):
    """y = fp16(x2d . w^T + bias) with w = fp16(scale * (q - zero)) dequantized in registers (K12, asvd_w8_linear_a16): x2d [T <= 256, K] fp16
    contiguous, q [N, K] uint8 (unit column stride), scale / zero [N] fp32, bias [N] fp16 or None.  One launch, deterministic.
    group_size 64 / 128 (K14): scale / zero [N, ceil(K / group_size)]; K % 16 == 0 and 16-byte-aligned x and rows only.
    weight_dtype=torch.bfloat16 (K19): the same with bf16 for fp16 throughout (x, bias, y and the weight the codes stand for)."""
    act = _act_dtype("w8_linear", x2d, bias, weight_dtype)
    lib = L.load(True)
    group = _group(group_size)
    _dev(x2d, "x")
    if x2d.dim() != 2 or q.dim() != 2 or x2d.dtype != weight_dtype or q.dtype != torch.uint8 or not x2d.is_contiguous() or q.stride(1) != 1:
        raise ValueError(f"w8_linear needs x [T, K] fp16 contiguous and q [N, K] uint8 (got {tuple(x2d.shape)} {x2d.dtype}, {tuple(q.shape)} {q.dtype})")
    T, K = x2d.shape
    N = q.shape[0]
    if q.shape[1] != K or not 1 <= T <= W8_MAX_TOKENS:
        raise ValueError(f"w8_linear: x {tuple(x2d.shape)} against q {tuple(q.shape)}; 1 <= tokens <= {W8_MAX_TOKENS}")
    if scale.dtype != torch.float32 or zero.dtype != torch.float32 or (not group and (scale.numel() != N or zero.numel() != N)) \
            or not scale.is_contiguous() \
            or not zero.is_contiguous() or (bias is not None and (bias.dtype != weight_dtype or bias.numel() != N or not bias.is_contiguous())):
        raise ValueError("w8_linear needs scale / zero [N] fp32 and bias [N] fp16 (or None), contiguous")
    if q.device != x2d.device or scale.device != x2d.device or zero.device != x2d.device or (bias is not None and bias.device != x2d.device):
        raise ValueError("w8_linear: all tensors must live on the device of x")
    if group:
        _check_params("w8_linear", scale, zero, N, K, group, x2d.device)
        if K % 16 or x2d.data_ptr() % 16 or q.data_ptr() % 16 or q.stride(0) % 16:
            raise ValueError("w8_linear with group_size needs K % 16 == 0 and x and the rows of q 16-byte aligned")
    y = torch.empty((T, N), dtype=weight_dtype, device=x2d.device)
    with _on(x2d.device):
        L.check(lib.asvd_w8_linear_a16(x2d.data_ptr(), act, T, q.data_ptr(), q.stride(0), scale.data_ptr(), zero.data_ptr(), group,
                                       bias.data_ptr() if bias is not None else None, N, K, y.data_ptr(), _stream(x2d)), "asvd_w8_linear_a16")
    return y


def w8_dequant(q, scale, zero, dtype, out=None, group_size=0):
    """the dense weight scale * (q - zero) in `dtype` (fp16 / bf16 / fp32), value for value the `out` of rtn_quant for these codes
    (asvd_w8_dequant).  q [rows, cols] uint8 with unit column stride; out: optional destination [rows, cols] with unit column stride.
    group_size 64 / 128 (asvd_w8_dequant_grouped): scale / zero [rows, ceil(cols / group_size)]."""
    lib = L.load(True)
    group = _group(group_size)
    _dev(q, "q")
    if q.dim() != 2 or q.dtype != torch.uint8 or q.stride(1) != 1 or dtype not in _DT:
        raise ValueError(f"w8_dequant needs q [rows, cols] uint8 with unit column stride and a float dtype (got {tuple(q.shape)} {q.dtype}, {dtype})")
    rows, cols = q.shape
    if group:
        _check_params("w8_dequant", scale, zero, rows, cols, group, q.device)
    elif scale.dtype != torch.float32 or zero.dtype != torch.float32 or scale.numel() != rows or zero.numel() != rows or not scale.is_contiguous() \
            or not zero.is_contiguous() or scale.device != q.device or zero.device != q.device:
        raise ValueError("w8_dequant needs scale / zero [rows] fp32 contiguous on the device of q")
    if out is None:
        out = torch.empty((rows, cols), dtype=dtype, device=q.device)
    elif out.shape != q.shape or out.dtype != dtype or out.stride(1) != 1 or out.device != q.device:
        raise ValueError(f"w8_dequant: out must be [{rows}, {cols}] {dtype} with unit column stride on the device of q")
    if rows == 0 or cols == 0:
        return out
    with _on(q.device):
        if group:
            L.check(lib.asvd_w8_dequant_grouped(q.data_ptr(), q.stride(0), scale.data_ptr(), zero.data_ptr(), group, rows, cols, out.data_ptr(),
                                                _DT[dtype], out.stride(0), _stream(q)), "asvd_w8_dequant_grouped")
            return out
        L.check(lib.asvd_w8_dequant(q.data_ptr(), q.stride(0), scale.data_ptr(), zero.data_ptr(), rows, cols, out.data_ptr(), _DT[dtype],
                                    out.stride(0), _stream(q)), "asvd_w8_dequant")
    return out


def wb_row_bytes(cols, bits):
    """bytes of a bitstream row of `cols` codes of `bits` (4 or 6) bits: ceil(cols / 64) * 8 * bits (asvd_wb_row_bytes; a host-side query)"""
    n = L.load().asvd_wb_row_bytes(int(cols), int(bits))
    if n < 0:
        raise ValueError(f"bit-packed rows hold 1 or more codes of 4 or 6 bits (got {cols} codes of {bits} bits)")
    return int(n)


def wb_pack(q, bits, out=None):
    """uint8 codes q [rows, cols] (unit column stride) -> bitstream rows uint8 [rows, wb_row_bytes(cols, bits)] (K13, asvd_wb_pack): code k of
    a row in bits [bits k, bits (k + 1)) of the row read as one little-endian integer, zero-padded to whole blocks of 64 codes."""
    lib = L.load(True)
    _dev(q, "q")
    if q.dim() != 2 or q.dtype != torch.uint8 or q.stride(1) != 1 or q.shape[0] < 1 or q.shape[1] < 1:
        raise ValueError(f"wb_pack needs q [rows, cols] uint8 with unit column stride (got {tuple(q.shape)} {q.dtype})")
    rows, cols = q.shape
    nb = wb_row_bytes(cols, bits)
    if out is None:
        out = torch.empty((rows, nb), dtype=torch.uint8, device=q.device)
    elif out.shape != (rows, nb) or out.dtype != torch.uint8 or out.stride(1) != 1 or out.device != q.device:
        raise ValueError(f"wb_pack: out must be [{rows}, {nb}] uint8 with unit column stride on the device of q")
    with _on(q.device):
        L.check(lib.asvd_wb_pack(q.data_ptr(), q.stride(0), rows, cols, int(bits), out.data_ptr(), out.stride(0), _stream(q)), "asvd_wb_pack")
    return out


def wb_dequant(qbits, bits, cols, scale, zero, dtype, out=None, group_size=0):
    """the dense weight scale * (code - zero) [rows, cols] in `dtype` (fp16 / bf16 / fp32) from bitstream rows qbits [rows, wb_row_bytes(cols,
    bits)] (asvd_wb_dequant): value for value w8_dequant on the unpacked codes.  out: optional destination with unit column stride.
    group_size 64 / 128 (asvd_wb_dequant_grouped): scale / zero [rows, ceil(cols / group_size)]."""
    lib = L.load(True)
    group = _group(group_size)
    _dev(qbits, "qbits")
    if qbits.dim() != 2 or qbits.dtype != torch.uint8 or qbits.stride(1) != 1 or dtype not in _DT:
        raise ValueError(f"wb_dequant needs qbits [rows, row bytes] uint8 with unit column stride and a float dtype (got {tuple(qbits.shape)} "
                         f"{qbits.dtype}, {dtype})")
    rows, cols = qbits.shape[0], int(cols)
    if qbits.shape[1] != wb_row_bytes(cols, bits):
        raise ValueError(f"wb_dequant: {tuple(qbits.shape)} is not the bitstream of [{rows}, {cols}] codes of {bits} bits")
    if group:
        _check_params("wb_dequant", scale, zero, rows, cols, group, qbits.device)
    elif scale.dtype != torch.float32 or zero.dtype != torch.float32 or scale.numel() != rows or zero.numel() != rows or not scale.is_contiguous() \
            or not zero.is_contiguous() or scale.device != qbits.device or zero.device != qbits.device:
        raise ValueError("wb_dequant needs scale / zero [rows] fp32 contiguous on the device of qbits")
    if out is None:
        out = torch.empty((rows, cols), dtype=dtype, device=qbits.device)
    elif out.shape != (rows, cols) or out.dtype != dtype or out.stride(1) != 1 or out.device != qbits.device:
        raise ValueError(f"wb_dequant: out must be [{rows}, {cols}] {dtype} with unit column stride on the device of qbits")
    if rows == 0:
        return out
    with _on(qbits.device):
        if group:
            L.check(lib.asvd_wb_dequant_grouped(qbits.data_ptr(), qbits.stride(0), int(bits), scale.data_ptr(), zero.data_ptr(), group, rows, cols,
                                                out.data_ptr(), _DT[dtype], out.stride(0), _stream(qbits)), "asvd_wb_dequant_grouped")
            return out
        L.check(lib.asvd_wb_dequant(qbits.data_ptr(), qbits.stride(0), int(bits), scale.data_ptr(), zero.data_ptr(), rows, cols, out.data_ptr(),
                                    _DT[dtype], out.stride(0), _stream(qbits)), "asvd_wb_dequant")
    return out


def wb_linear(x2d, qbits, bits, scale, zero, bias=None, group_size=0, weight_dtype=torch.float16):
    """w8_linear on bitstream rows (K13, asvd_wb_linear_a16): x2d [T <= 256, K] fp16 contiguous, K % 16 == 0, qbits [N, wb_row_bytes(K, bits)]
    uint8, scale / zero [N] fp32, bias [N] fp16 or None; x2d and the rows 16-byte aligned.  The bits of w8_linear on the same codes.
    group_size 64 / 128 (K14): scale / zero [N, ceil(K / group_size)].  weight_dtype=torch.bfloat16 (K19): bf16 for fp16 throughout."""
    act = _act_dtype("wb_linear", x2d, bias, weight_dtype)
    lib = L.load(True)
    group = _group(group_size)
    _dev(x2d, "x")
    if x2d.dim() != 2 or qbits.dim() != 2 or x2d.dtype != weight_dtype or qbits.dtype != torch.uint8 or not x2d.is_contiguous() or qbits.stride(1) != 1:
        raise ValueError(f"wb_linear needs x [T, K] fp16 contiguous and qbits [N, row bytes] uint8 (got {tuple(x2d.shape)} {x2d.dtype}, "
                         f"{tuple(qbits.shape)} {qbits.dtype})")
    T, K = x2d.shape
    N = qbits.shape[0]
    if K < 1 or K % 16 or qbits.shape[1] != wb_row_bytes(K, bits) or not 1 <= T <= W8_MAX_TOKENS:
        raise ValueError(f"wb_linear: x {tuple(x2d.shape)} against qbits {tuple(qbits.shape)} of {bits}-bit codes; K % 16 == 0, 1 <= tokens <= {W8_MAX_TOKENS}")
    if scale.dtype != torch.float32 or zero.dtype != torch.float32 or (not group and (scale.numel() != N or zero.numel() != N)) \
            or not scale.is_contiguous() \
            or not zero.is_contiguous() or (bias is not None and (bias.dtype != weight_dtype or bias.numel() != N or not bias.is_contiguous())):
        raise ValueError("wb_linear needs scale / zero [N] fp32 and bias [N] fp16 (or None), contiguous")
    if group:
        _check_params("wb_linear", scale, zero, N, K, group, scale.device)
    if qbits.device != x2d.device or scale.device != x2d.device or zero.device != x2d.device or (bias is not None and bias.device != x2d.device):
        raise ValueError("wb_linear: all tensors must live on the device of x")
    if x2d.data_ptr() % 16 or qbits.data_ptr() % 16 or qbits.stride(0) % 16:
        raise ValueError("wb_linear needs x and the rows of qbits 16-byte aligned")
    y = torch.empty((T, N), dtype=weight_dtype, device=x2d.device)
    with _on(x2d.device):
        L.check(lib.asvd_wb_linear_a16(x2d.data_ptr(), act, T, qbits.data_ptr(), qbits.stride(0), int(bits), scale.data_ptr(), zero.data_ptr(), group,
                                       bias.data_ptr() if bias is not None else None, N, K, y.data_ptr(), _stream(x2d)), "asvd_wb_linear_a16")
    return y


def lowrank_packed_work(T, r, device):
    """a zeroed workspace of asvd_lowrank_packed_f16 for up to T tokens at rank r: the barrier words (which must start at zero) and the intermediate"""
    return torch.zeros(int(L.load().asvd_lowrank_packed_work_bytes(int(T), int(r))), dtype=torch.uint8, device=device)


def lowrank_packed_forward(x2d, B_codes, B_scale, B_zero, A_codes, A_scale, A_zero, bits, bias, work, group_size=0, weight_dtype=torch.float16):
    """y = fp16(fp16(x wB^T) wA^T + bias) for a pair of packed factors in one launch (K16, asvd_lowrank_packed_a16): the bits of w8_linear /
    wb_linear applied twice.  x2d [T <= 256, K] fp16 contiguous; bits is the STORAGE width of both factors: 8 (B_codes [r, K], A_codes [N, r]
    uint8, one code per byte) or 6 / 4 (bitstream rows [r, wb_row_bytes(K, bits)], [N, wb_row_bytes(r, bits)]); scale / zero fp32 [r] and [N],
    or with group_size 64 / 128 [r, ceil(K / G)] and [N, ceil(r / G)]; bias [N] fp16 or None; K % 16 == 0 and r % 16 == 0, x and the code rows
    16-byte aligned; work from lowrank_packed_work(>= T, r), one per stream in flight.  weight_dtype=torch.bfloat16 (K19): bf16 for fp16
    throughout, the intermediate included (the same workspace: 2 bytes per element)."""
    act = _act_dtype("lowrank_packed_forward", x2d, bias, weight_dtype)
    lib = L.load(True)
    group, bits = _group(group_size), int(bits)
    _dev(x2d, "x")
    if bits not in (8, 6, 4):
        raise ValueError(f"lowrank_packed_forward: storage width 8, 6 or 4 bits (got {bits})")
    if x2d.dim() != 2 or x2d.dtype != weight_dtype or not x2d.is_contiguous() or any(
            c.dim() != 2 or c.dtype != torch.uint8 or c.stride(1) != 1 for c in (B_codes, A_codes)):
        raise ValueError("lowrank_packed_forward needs x [T, K] fp16 contiguous and uint8 code matrices with unit column stride")
    T, K = x2d.shape
    r, N = B_codes.shape[0], A_codes.shape[0]
    wB, wA = (K, r) if bits == 8 else (wb_row_bytes(K, bits) if K > 0 else -1, wb_row_bytes(r, bits))
    if K % 16 or r % 16 or B_codes.shape[1] != wB or A_codes.shape[1] != wA or not 1 <= T <= W8_MAX_TOKENS:
        raise ValueError(f"lowrank_packed_forward: x {tuple(x2d.shape)} against B {tuple(B_codes.shape)} and A {tuple(A_codes.shape)} at {bits} bits; "
                         f"K % 16 == 0, r % 16 == 0, 1 <= tokens <= {W8_MAX_TOKENS}")
    dev = x2d.device
    _check_params("lowrank_packed_forward (B)", B_scale, B_zero, r, K, group, dev)
    _check_params("lowrank_packed_forward (A)", A_scale, A_zero, N, r, group, dev)
    if bias is not None and (bias.dtype != weight_dtype or bias.numel() != N or not bias.is_contiguous() or bias.device != dev):
        raise ValueError("lowrank_packed_forward needs bias [N] fp16 contiguous on the device of x (or None)")
    if B_codes.device != dev or A_codes.device != dev or work.device != dev:
        raise ValueError("lowrank_packed_forward: all tensors must live on the device of x")
    if x2d.data_ptr() % 16 or B_codes.data_ptr() % 16 or A_codes.data_ptr() % 16 or B_codes.stride(0) % 16 or A_codes.stride(0) % 16:
        raise ValueError("lowrank_packed_forward needs x and the code rows 16-byte aligned")
    y = torch.empty((T, N), dtype=weight_dtype, device=dev)
    with _on(dev):
        L.check(lib.asvd_lowrank_packed_a16(x2d.data_ptr(), act, T, B_codes.data_ptr(), B_codes.stride(0), B_scale.data_ptr(), B_zero.data_ptr(),
                                            A_codes.data_ptr(), A_codes.stride(0), A_scale.data_ptr(), A_zero.data_ptr(), bits, group,
                                            bias.data_ptr() if bias is not None else None, N, K, r, y.data_ptr(), work.data_ptr(), work.numel(),
                                            _stream(x2d)), "asvd_lowrank_packed_a16")
    _lowrank_count(work)   # the give-up word of the workspace: as lowrank_forward
    return y


PACKED_GEMM_MAX_TOKENS = 1 << 20  # ASVD_PACKED_GEMM_MAX_TOKENS (asvd_packed_gemm_max_tokens)


def packed_gemm(x2d, codes, bits, scale, zero, bias=None, group_size=0, weight_dtype=torch.float16):
    """y = fp16(x2d . w^T + bias) with w = fp16(scale * (code - zero)) for inputs beyond decode (K17, asvd_packed_gemm_a16): the token-tiled
    GEMM that stages x through LDS once per workgroup and streams the codes once per tile of up to 128 tokens.  x2d [T, K] fp16 contiguous,
    K % 16 == 0, 1 <= T <= PACKED_GEMM_MAX_TOKENS.  bits is the STORAGE width of `codes`: 8 (W8Linear.qweight: [N, K] uint8, unit column
    stride) or 6 / 4 (WBLinear.qbits: bitstream rows [N, wb_row_bytes(K, bits)]).  scale / zero [N] fp32, or with group_size 64 / 128
    [N, ceil(K / group_size)]; bias [N] fp16 or None; x2d and the code rows 16-byte aligned.  One launch, deterministic; the weight is the
    one w8_dequant / wb_dequant write, bit for bit.  weight_dtype=torch.bfloat16 (K19): bf16 for fp16 throughout.  Every argument check comes
    before the device is asked for."""
    act = _act_dtype("packed_gemm", x2d, bias, weight_dtype)
    group, bits = _group(group_size), int(bits)
    if bits not in (8, 6, 4):
        raise ValueError(f"packed_gemm: storage width 8, 6 or 4 bits (got {bits})")
    if x2d.dim() != 2 or codes.dim() != 2 or x2d.dtype != weight_dtype or codes.dtype != torch.uint8 or not x2d.is_contiguous() or codes.stride(1) != 1:
        raise ValueError(f"packed_gemm needs x [T, K] fp16 contiguous and codes [N, row bytes] uint8 with unit column stride (got {tuple(x2d.shape)} "
                         f"{x2d.dtype}, {tuple(codes.shape)} {codes.dtype})")
    T, K = x2d.shape
    N = codes.shape[0]
    if K < 1 or K % 16 or N < 1 or codes.shape[1] != (K if bits == 8 else wb_row_bytes(K, bits)) or not 1 <= T <= PACKED_GEMM_MAX_TOKENS:
        raise ValueError(f"packed_gemm: x {tuple(x2d.shape)} against codes {tuple(codes.shape)} at {bits} bits; K % 16 == 0, "
                         f"1 <= tokens <= {PACKED_GEMM_MAX_TOKENS}")
    dev = x2d.device
    _check_params("packed_gemm", scale, zero, N, K, group, dev)
    if bias is not None and (bias.dtype != weight_dtype or bias.numel() != N or not bias.is_contiguous() or bias.device != dev):
        raise ValueError("packed_gemm needs bias [N] fp16 contiguous on the device of x (or None)")
    if codes.device != dev:
        raise ValueError("packed_gemm: all tensors must live on the device of x")
    if x2d.data_ptr() % 16 or codes.data_ptr() % 16 or codes.stride(0) % 16:
        raise ValueError("packed_gemm needs x and the code rows 16-byte aligned")
    _dev(x2d, "x")
    lib = L.load(True)
    y = torch.empty((T, N), dtype=weight_dtype, device=dev)
    with _on(dev):
        L.check(lib.asvd_packed_gemm_a16(x2d.data_ptr(), act, T, codes.data_ptr(), codes.stride(0), bits, scale.data_ptr(), zero.data_ptr(), group,
                                         bias.data_ptr() if bias is not None else None, N, K, y.data_ptr(), _stream(x2d)), "asvd_packed_gemm_a16")
    return y


# ---- K20: decode attention on a low-rank KV cache (csrc/lowrank_kv.hip) ----------------------------------------------------------------

KV_ROPE = {"none": L.KV_ROPE_NONE, "half": L.KV_ROPE_HALF}


def rope_table(Tmax, D, theta=10000.0, device=None):
    """(cos, sin) fp32 [Tmax, D/2] of the rotary embedding: angle(t, i) = t * theta^(-2i / D), the HF Llama inverse frequencies.  Row t rotates
    position t; lowrank_kv_scores / lowrank_kv_decode apply it to the pairs (i, i + D/2) (rotate_half)."""
    if D < 2 or D % 2 or Tmax < 1:
        raise ValueError(f"rope_table: Tmax >= 1 and an even D (got {Tmax}, {D})")
    inv = 1.0 / (float(theta) ** (torch.arange(0, D, 2, dtype=torch.int64, device=device).float() / D))
    ang = torch.arange(Tmax, dtype=torch.int64, device=device).float()[:, None] * inv[None, :]
    return ang.cos().contiguous(), ang.sin().contiguous()


def lowrank_kv_plan(B, H, Tmax):
    """(token tile of the score kernels, split length, number of splits) K20 uses for (B, H, Tmax): host only"""
    tile, split, n = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    L.check(L.load(False).asvd_lowrank_kv_plan(B, H, Tmax, ctypes.byref(tile), ctypes.byref(split), ctypes.byref(n)), "asvd_lowrank_kv_plan")
    return tile.value, split.value, n.value


def lowrank_kv_work(B, H, Tmax, r_k, r_v, device):
    """the workspace of one K20 call at these sizes (uint8, reusable across steps; one per stream)"""
    nb = ctypes.c_size_t()
    L.check(L.load(False).asvd_lowrank_kv_worksize(B, H, Tmax, r_k, r_v, ctypes.byref(nb)), "asvd_lowrank_kv_worksize")
    return _work(nb.value, device)


KV_DTYPES = (torch.float16, torch.bfloat16)   # element types of K20 / K21: q, Ak, Av, the biases, out and an unquantised cache share ONE (bf16: K22)


def _kv_name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp16"


def _kv_cache_arg(name, c, B, dev, dt=torch.float16):
    if c.dim() != 3 or c.dtype != dt or c.shape[0] != B or c.stride(2) != 1 or c.device != dev:
        raise ValueError(f"{name}: cache [B, Tmax, r] {_kv_name(dt)} (the dtype of q) with unit rank stride on the device of q "
                         f"(got {tuple(c.shape)} {c.dtype})")
    r = c.shape[2]
    if r < 16 or r % 16:
        raise ValueError(f"{name}: rank {r} is not a multiple of 16")
    if c.data_ptr() % 16 or c.stride(1) % 8 or c.stride(0) % 8 or c.stride(1) < r:
        raise ValueError(f"{name}: rows must be 16-byte aligned (row stride {c.stride(1)}, batch stride {c.stride(0)} elements)")
    return r


def _kv_args(name, q, ck, lens, Ak, bk, rope, H_kv, r_k=None):
    """r_k: given when the caller has checked the cache by rules of its own (an int8 cache, K21).  q is fp16 or bf16 and every other
    16-bit argument has q's dtype (the caller checks Av, bv and out against it)"""
    if q.dim() != 3 or q.dtype not in KV_DTYPES or not q.is_contiguous():
        raise ValueError(f"{name} needs q [B, H, D] fp16 or bf16 contiguous (got {tuple(q.shape)} {q.dtype})")
    B, H, D = q.shape
    dt, dn = q.dtype, _kv_name(q.dtype)
    dev = q.device
    if D not in (64, 128) or H < 1 or H_kv < 1 or H % H_kv:
        raise ValueError(f"{name}: head size 64 or 128 and H_kv dividing H (got D {D}, H {H}, H_kv {H_kv})")
    if r_k is None:
        r_k = _kv_cache_arg(name, ck, B, dev, dt)
    Tmax = ck.shape[1]
    if lens.dtype != torch.int32 or lens.shape != (B,) or not lens.is_contiguous() or lens.device != dev:
        raise ValueError(f"{name} needs lens int32 [B] on the device of q")
    if Ak.dtype != dt or tuple(Ak.shape) != (H_kv * D, r_k) or not Ak.is_contiguous() or Ak.device != dev or Ak.data_ptr() % 16:
        raise ValueError(f"{name} needs Ak [H_kv * D, r_k] {dn} (the dtype of q) contiguous (got {tuple(Ak.shape)} {Ak.dtype})")
    if bk is not None and (bk.dtype != dt or bk.numel() != H_kv * D or not bk.is_contiguous() or bk.device != dev):
        raise ValueError(f"{name} needs bk [H_kv * D] {dn} (the dtype of q) contiguous or None")
    mode, cos, sin = "none", None, None
    if rope is not None:
        mode, (cos, sin) = "half", rope
        if bk is not None:
            raise ValueError(f"{name}: a key bias cannot be combined with a rotation")
        for t in (cos, sin):
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < Tmax or t.shape[1] != D // 2 or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{name} needs cos / sin fp32 [>= Tmax, D/2] contiguous on the device of q")
    return B, H, D, r_k, Tmax, mode, cos, sin


def _kv_value_args(name, q, Av, bv, out, H_kv, r_v):
    """Av, bv and a given out against q: one dtype"""
    B, H, D = q.shape
    dt, dn, dev = q.dtype, _kv_name(q.dtype), q.device
    if Av.dtype != dt or tuple(Av.shape) != (H_kv * D, r_v) or not Av.is_contiguous() or Av.device != dev or Av.data_ptr() % 16:
        raise ValueError(f"{name} needs Av [H_kv * D, r_v] {dn} (the dtype of q) contiguous (got {tuple(Av.shape)} {Av.dtype})")
    if bv is not None and (bv.dtype != dt or bv.numel() != H_kv * D or not bv.is_contiguous() or bv.device != dev):
        raise ValueError(f"{name} needs bv [H_kv * D] {dn} (the dtype of q) contiguous or None")
    if out is not None and (out.dtype != dt or tuple(out.shape) != (B, H, D) or not out.is_contiguous() or out.device != dev):
        raise ValueError(f"{name}: out must be [B, H, D] {dn} (the dtype of q) contiguous on the device of q")


def _kv_entry(lib, name, q):
    """(the C entry, its dtype code): fp16 calls keep the K20 / K21 entries, bf16 goes to their _a16 forms (K22)"""
    if q.dtype == torch.bfloat16:
        return getattr(lib, name + "_a16"), L.BF16, name + "_a16"
    return getattr(lib, name), L.F16, name


def lowrank_kv_scores(q, ck, lens, Ak, H_kv, scale, bk=None, rope=None, work=None):
    """S [B, H, Tmax] fp32 = scale * q_h . K_h[t] with K_h = C_k A_k[kv(h)]^T (rotated by rope = (cos, sin) tables when given), zeros at
    t >= lens[b] (K20 stages a and b, asvd_lowrank_kv_scores).  q [B, H, D] fp16 (already rotated), ck [B, Tmax, r_k] fp16 (strided views with
    16-byte aligned rows are fine), lens int32 [B], Ak [H_kv * D, r_k] fp16.  Every argument check comes before the device is asked for.
    All of q, ck, Ak, bk may be bf16 instead (K22, asvd_lowrank_kv_scores_a16: q~ is rounded to bf16, the product runs on the bf16 MFMA); mixed
    dtypes and fp32 are a ValueError."""
    B, H, D, r_k, Tmax, mode, cos, sin = _kv_args("lowrank_kv_scores", q, ck, lens, Ak, bk, rope, H_kv)
    _dev(q, "q")
    lib = L.load(True)
    dev = q.device
    if work is None:
        work = lowrank_kv_work(B, H, Tmax, r_k, 16, dev)
    out = torch.empty((B, H, Tmax), dtype=torch.float32, device=dev)
    with _on(dev):
        fn, dtc, fname = _kv_entry(lib, "asvd_lowrank_kv_scores", q)
        L.check(fn(q.data_ptr(), ck.data_ptr(), lens.data_ptr(), Ak.data_ptr(), _ptr(bk), _ptr(cos), _ptr(sin), dtc, KV_ROPE[mode], float(scale), B, H,
                   H_kv, D, r_k, Tmax, ck.stride(1), ck.stride(0), out.data_ptr(), work.data_ptr(), work.numel(), _stream(q)), fname)
    return out


def lowrank_kv_decode(q, ck, cv, lens, Ak, Av, H_kv, scale, bk=None, bv=None, rope=None, work=None, out=None):
    """out [B, H, D] fp16 = softmax over t < lens[b] of the scores above, times V_h = C_v A_v[kv(h)]^T + b_v, for ONE new query token per
    sequence (K20, asvd_lowrank_kv_decode).  cv [B, Tmax, r_v] fp16 like ck, Av [H_kv * D, r_v] fp16.  A sequence with lens[b] == 0 gets
    zeros.  Asynchronous on the current stream, no host sync, graph-capturable when `work` and `out` are given.
    All of q, ck, cv, Ak, Av, bk, bv and out may be bf16 instead (K22, asvd_lowrank_kv_decode_a16): q~, p and out are rounded to bf16 (RNE) where
    the fp16 form rounds to fp16, on the bf16 MFMA, with the same sums in the same order.  Mixed dtypes and fp32 are a ValueError."""
    B, H, D, r_k, Tmax, mode, cos, sin = _kv_args("lowrank_kv_decode", q, ck, lens, Ak, bk, rope, H_kv)
    dev = q.device
    r_v = _kv_cache_arg("lowrank_kv_decode", cv, B, dev, q.dtype)
    if cv.shape[1] != Tmax:
        raise ValueError("lowrank_kv_decode: ck and cv hold different token counts")
    _kv_value_args("lowrank_kv_decode", q, Av, bv, out, H_kv, r_v)
    _dev(q, "q")
    lib = L.load(True)
    if work is None:
        work = lowrank_kv_work(B, H, Tmax, r_k, r_v, dev)
    if out is None:
        out = torch.empty((B, H, D), dtype=q.dtype, device=dev)
    with _on(dev):
        fn, dtc, fname = _kv_entry(lib, "asvd_lowrank_kv_decode", q)
        L.check(fn(q.data_ptr(), ck.data_ptr(), cv.data_ptr(), lens.data_ptr(), Ak.data_ptr(), Av.data_ptr(), _ptr(bk), _ptr(bv), _ptr(cos), _ptr(sin),
                   dtc, KV_ROPE[mode], float(scale), B, H, H_kv, D, r_k, r_v, Tmax, ck.stride(1), ck.stride(0), cv.stride(1), cv.stride(0),
                   out.data_ptr(), work.data_ptr(), work.numel(), _stream(q)), fname)
    return out


# ---- K21: the low-rank KV cache as int8 codes (csrc/lowrank_kv_q8.hip, csrc/lowrank_kv_q8.h) -------------------------------------------

KV_Q8_GROUP = 32   # latent columns per fp32 scale


def lowrank_kv_groups(r):
    """scales per cache row of r columns: groups of 32, a 16-wide last one when r % 32 == 16"""
    return (int(r) + KV_Q8_GROUP - 1) // KV_Q8_GROUP


def _kv_per_column(scales, r):
    return scales.repeat_interleave(KV_Q8_GROUP, -1)[..., :r]


def lowrank_kv_quant_torch(x):
    """(codes int8 [..., r], scales fp32 [..., ceil(r / 32)]) of x [..., r], r a multiple of 16: the K21 format in torch ops, on any device,
    bit for bit what lowrank_kv_quant writes.  x goes through fp16 first.  Per group of 32 columns: s = amax / 127 (fp32 division),
    code = clamp(rint(x / s), -127, 127); a group of zeros has s = 0, a group with a NaN or an Inf s = NaN, both with codes 0."""
    r = x.shape[-1]
    if r < 16 or r % 16:
        raise ValueError(f"lowrank_kv_quant_torch: rank {r} is not a multiple of 16")
    ng = lowrank_kv_groups(r)
    xf = x.half().float()
    g = torch.nn.functional.pad(xf, (0, ng * KV_Q8_GROUP - r)).reshape(*x.shape[:-1], ng, KV_Q8_GROUP)
    bad = ~torch.isfinite(g).all(-1)
    amax = torch.where(torch.isfinite(g), g.abs(), torch.zeros_like(g)).amax(-1)
    s = amax / torch.full_like(amax, 127.0)   # a tensor divisor: a Python scalar may be turned into a multiplication by 1 / 127
    zero = bad | (amax == 0)
    sd = torch.where(zero, torch.ones_like(s), s)
    codes = torch.round(g / sd[..., None]).clamp(-127.0, 127.0)
    codes = torch.where(zero[..., None], torch.zeros_like(codes), codes).to(torch.int8)
    s = torch.where(bad, torch.full_like(s, float("nan")), s)
    return codes.reshape(*x.shape[:-1], ng * KV_Q8_GROUP)[..., :r].contiguous(), s


def lowrank_kv_dequant(codes, scales):
    """fp16 [..., r] = fp16(float(code) * s): the value every K21 kernel uses for a code, any int8 code, any device"""
    r = codes.shape[-1]
    if codes.dtype != torch.int8 or scales.dtype != torch.float32 or scales.shape[:-1] != codes.shape[:-1] or scales.shape[-1] < lowrank_kv_groups(r):
        raise ValueError(f"lowrank_kv_dequant: codes int8 [..., r] and scales fp32 [..., >= ceil(r / 32)] (got {tuple(codes.shape)} {codes.dtype}, "
                         f"{tuple(scales.shape)} {scales.dtype})")
    return (codes.float() * _kv_per_column(scales[..., :lowrank_kv_groups(r)], r)).half()


def _kv_q8_arg(name, codes, scales, B, dev):
    """the rules of an int8 cache [B, Tmax, r] and its scales [B, Tmax, >= ng]; returns r"""
    if codes.dim() != 3 or codes.dtype != torch.int8 or codes.shape[0] != B or codes.stride(2) != 1 or codes.device != dev:
        raise ValueError(f"{name}: codes [B, Tmax, r] int8 with unit rank stride on the device of q (got {tuple(codes.shape)} {codes.dtype})")
    r = codes.shape[2]
    if r < 16 or r % 16:
        raise ValueError(f"{name}: rank {r} is not a multiple of 16")
    if codes.data_ptr() % 16 or codes.stride(1) % 16 or codes.stride(0) % 16 or codes.stride(1) < r:
        raise ValueError(f"{name}: code rows must be 16-byte aligned (row stride {codes.stride(1)}, batch stride {codes.stride(0)} bytes)")
    if scales.dim() != 3 or scales.dtype != torch.float32 or tuple(scales.shape[:2]) != tuple(codes.shape[:2]) or scales.shape[2] < lowrank_kv_groups(r) \
            or scales.stride(2) != 1 or scales.stride(1) < lowrank_kv_groups(r) or scales.device != dev:
        raise ValueError(f"{name}: scales [B, Tmax, >= {lowrank_kv_groups(r)}] fp32 with unit last stride on the device of q "
                         f"(got {tuple(scales.shape)} {scales.dtype})")
    return r


def lowrank_kv_quant(x, codes_out, scales_out):
    """codes_out int8 [B, n, r] and scales_out fp32 [B, n, >= ceil(r / 32)] (strided views: the slice [:, t0 : t0 + n] of a cache) <- the K21
    quantisation of x [B, n, r] fp16 (asvd_lowrank_kv_quant: one launch on the current stream, no host sync; nothing outside the
    B * n destination rows is written).  Every argument check comes before the device is asked for."""
    if x.dim() != 3 or x.dtype != torch.float16 or x.stride(2) != 1:
        raise ValueError(f"lowrank_kv_quant needs x [B, n, r] fp16 with unit rank stride (got {tuple(x.shape)} {x.dtype})")
    B, n, r = x.shape
    if B < 1 or n < 1:
        raise ValueError("lowrank_kv_quant: no rows")
    if tuple(codes_out.shape) != (B, n, r) or scales_out.dim() != 3:
        raise ValueError(f"lowrank_kv_quant: codes_out {tuple(codes_out.shape)} does not match x {tuple(x.shape)}")
    _kv_q8_arg("lowrank_kv_quant", codes_out, scales_out, B, x.device)
    if x.data_ptr() % 16 or x.stride(1) % 8 or x.stride(0) % 8 or x.stride(1) < r:
        raise ValueError(f"lowrank_kv_quant: rows of x must be 16-byte aligned (row stride {x.stride(1)}, batch stride {x.stride(0)} elements)")
    _dev(x, "x")
    lib = L.load(True)
    with _on(x.device):
        L.check(lib.asvd_lowrank_kv_quant(x.data_ptr(), x.stride(1), x.stride(0), codes_out.data_ptr(), codes_out.stride(1), codes_out.stride(0),
                                          scales_out.data_ptr(), scales_out.stride(1), scales_out.stride(0), L.F16, B, n, r, _stream(x)),
                "asvd_lowrank_kv_quant")
    return codes_out, scales_out


def _kv_args_q8(name, q, ck, sk, lens, Ak, bk, rope, H_kv):
    """_kv_args for an int8 key cache: the same rules, with _kv_q8_arg's in place of the fp16 cache's"""
    if q.dim() != 3:
        raise ValueError(f"{name} needs q [B, H, D] fp16 or bf16 contiguous (got {tuple(q.shape)} {q.dtype})")
    return _kv_args(name, q, ck, lens, Ak, bk, rope, H_kv, r_k=_kv_q8_arg(name, ck, sk, q.shape[0], q.device))


def lowrank_kv_scores_q8(q, ck, sk, lens, Ak, H_kv, scale, bk=None, rope=None, work=None):
    """lowrank_kv_scores on an int8 cache: ck int8 codes [B, Tmax, r_k] and sk fp32 scales [B, Tmax, >= ceil(r_k / 32)] (K21,
    asvd_lowrank_kv_scores_q8).  The bits of lowrank_kv_scores(q, lowrank_kv_dequant(ck, sk), ...).  With bf16 q, Ak, bk (K22,
    asvd_lowrank_kv_scores_q8_a16): the bits of the bf16 call on lowrank_kv_dequant(ck, sk).bfloat16(), the same codes rounded twice."""
    B, H, D, r_k, Tmax, mode, cos, sin = _kv_args_q8("lowrank_kv_scores_q8", q, ck, sk, lens, Ak, bk, rope, H_kv)
    _dev(q, "q")
    lib = L.load(True)
    dev = q.device
    if work is None:
        work = lowrank_kv_work(B, H, Tmax, r_k, 16, dev)
    out = torch.empty((B, H, Tmax), dtype=torch.float32, device=dev)
    with _on(dev):
        fn, dtc, fname = _kv_entry(lib, "asvd_lowrank_kv_scores_q8", q)
        L.check(fn(q.data_ptr(), ck.data_ptr(), sk.data_ptr(), lens.data_ptr(), Ak.data_ptr(), _ptr(bk), _ptr(cos), _ptr(sin), dtc, KV_ROPE[mode],
                   float(scale), B, H, H_kv, D, r_k, Tmax, ck.stride(1), ck.stride(0), sk.stride(1), sk.stride(0), out.data_ptr(), work.data_ptr(),
                   work.numel(), _stream(q)), fname)
    return out


def lowrank_kv_decode_q8(q, ck, cv, sk, sv, lens, Ak, Av, H_kv, scale, bk=None, bv=None, rope=None, work=None, out=None):
    """lowrank_kv_decode on an int8 cache: ck / cv int8 codes, sk / sv their fp32 group scales (K21, asvd_lowrank_kv_decode_q8).  The bits of
    lowrank_kv_decode on the dequantised cache; same workspace (lowrank_kv_work), asynchronous, graph-capturable when `work` and `out` are given.
    With bf16 q, Ak, Av, bk, bv, out (K22, asvd_lowrank_kv_decode_q8_a16): the bits of the bf16 lowrank_kv_decode on
    lowrank_kv_dequant(codes, scales).bfloat16(); the cache format does not change."""
    name = "lowrank_kv_decode_q8"
    B, H, D, r_k, Tmax, mode, cos, sin = _kv_args_q8(name, q, ck, sk, lens, Ak, bk, rope, H_kv)
    dev = q.device
    r_v = _kv_q8_arg(name, cv, sv, B, dev)
    if cv.shape[1] != Tmax:
        raise ValueError(f"{name}: ck and cv hold different token counts")
    _kv_value_args(name, q, Av, bv, out, H_kv, r_v)
    _dev(q, "q")
    lib = L.load(True)
    if work is None:
        work = lowrank_kv_work(B, H, Tmax, r_k, r_v, dev)
    if out is None:
        out = torch.empty((B, H, D), dtype=q.dtype, device=dev)
    with _on(dev):
        fn, dtc, fname = _kv_entry(lib, "asvd_lowrank_kv_decode_q8", q)
        L.check(fn(q.data_ptr(), ck.data_ptr(), cv.data_ptr(), sk.data_ptr(), sv.data_ptr(), lens.data_ptr(), Ak.data_ptr(), Av.data_ptr(), _ptr(bk),
                   _ptr(bv), _ptr(cos), _ptr(sin), dtc, KV_ROPE[mode], float(scale), B, H, H_kv, D, r_k, r_v, Tmax, ck.stride(1), ck.stride(0),
                   cv.stride(1), cv.stride(0), sk.stride(1), sk.stride(0), sv.stride(1), sv.stride(0), out.data_ptr(), work.data_ptr(), work.numel(),
                   _stream(q)), fname)
    return out


PROFILE_CLASSES = ["pack", "sgram", "evd", "supdate", "finalize", "snapshot", "gram1", "update1", "supgram"]


def svd_profile(enable=None, keep_split=False):
    """enable/disable HIP-event timing of the SVD kernel classes, or read the last call's totals.  keep_split: the profiled call keeps the
    two-halves split (asvd_svd_set_profiling mode 2; read the halves with svd_split_profile) instead of running every kernel alone on the chip"""
    lib = L.load(False)
    if enable is not None:
        lib.asvd_svd_set_profiling((2 if keep_split else 1) if enable else 0)
        return None
    names = PROFILE_CLASSES
    ms = (ctypes.c_float * len(names))()
    n = (ctypes.c_int * len(names))()
    lib.asvd_svd_get_profile(ms, n)
    out = {names[i]: {"ms": ms[i], "launches": n[i]} for i in range(len(names))}
    cnt = (ctypes.c_longlong * 3)()
    lib.asvd_svd_get_pair_counts(cnt)
    out["pairs"] = {"visited": int(cnt[0]), "rotated": int(cnt[1]), "super_updates": int(cnt[2])}
    sms = (ctypes.c_float * 64)()
    srot = (ctypes.c_longlong * 64)()
    ns = min(64, lib.asvd_svd_get_sweep_times(sms, srot, 64))
    out["sweep_ms"] = [float(sms[i]) for i in range(ns)]
    out["sweep_rotated"] = [int(srot[i]) for i in range(ns)]
    return out


def svd_split_profile():
    """per-half class times of the last call profiled with keep_split (asvd_svd_get_split_profile), or None when that call did not split:
    {"halves": [{class: {"ms", "launches"}} x 2], "supgram_ms": {"half0", "half1", "union", "both"}}"""
    lib = L.load(False)
    n = len(PROFILE_CLASSES)
    ms = (ctypes.c_float * (2 * n))()
    ln = (ctypes.c_int * (2 * n))()
    ov = (ctypes.c_float * 4)()
    if lib.asvd_svd_get_split_profile(ms, ln, ov) != 1:
        return None
    halves = [{PROFILE_CLASSES[i]: {"ms": ms[h * n + i], "launches": ln[h * n + i]} for i in range(n)} for h in range(2)]
    return {"halves": halves, "supgram_ms": {"half0": ov[0], "half1": ov[1], "union": ov[2], "both": ov[3]}}


def svd_set_split(mode):
    """asvd_svd_set_split: 0 never split a batch over the two chip halves, 1 split when allowed, -1 default (as 1 unless ASVD_SPLIT=0)"""
    L.load(False).asvd_svd_set_split(int(mode))
