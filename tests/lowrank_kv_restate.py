"""fp64 restatement of decode attention on a low-rank KV cache (K20): the oracle of tests/test_gpu_lowrank_kv.py, checked on the host
against torch SDPA and the installed transformers' rotary embedding by tests/test_lowrank_kv_host.py.  Plain form only: it rebuilds
K = C_k A_k^T (+ b_k) and V = C_v A_v^T + b_v in full and never uses the absorbed products the kernel uses."""
import torch


def rotate_half_table(x, cos, sin):
    """x [..., T, D]; cos / sin [T, D/2]: row t rotates position t, pairs (i, i + D/2)"""
    half = x.shape[-1] // 2
    lo, hi = x[..., :half], x[..., half:]
    c, s = cos.to(x.dtype), sin.to(x.dtype)
    return torch.cat([lo * c - hi * s, hi * c + lo * s], -1)


def rebuild(c, A, bias, H_kv, H):
    """[B, T, r] x [H_kv * D, r] -> [B, H, T, D] fp64, KV head h // (H / H_kv) for head h"""
    B, T, _ = c.shape
    D = A.shape[0] // H_kv
    x = c.double() @ A.double().T
    if bias is not None:
        x = x + bias.double()
    return x.view(B, T, H_kv, D).permute(0, 2, 1, 3).repeat_interleave(H // H_kv, 1)


def kv_scores(q, ck, lens, Ak, H_kv, scale, bk=None, rope=None):
    """S [B, H, Tmax] fp64 = scale * q_h . K_h[t]; zeros at t >= lens[b]"""
    B, H, D = q.shape
    K = rebuild(ck, Ak, bk, H_kv, H)
    if rope is not None:
        K = rotate_half_table(K, rope[0].double()[: K.shape[2]], rope[1].double()[: K.shape[2]])
    S = scale * torch.einsum("bhd,bhtd->bht", q.double(), K)
    live = torch.arange(ck.shape[1])[None, :] < torch.as_tensor(lens).long().cpu()[:, None]
    return torch.where(live[:, None, :].to(S.device), S, torch.zeros_like(S)), live


def kv_decode(q, ck, cv, lens, Ak, Av, H_kv, scale, bk=None, bv=None, rope=None):
    """out [B, H, D] fp64: softmax over t < lens[b]; a sequence with lens[b] == 0 gives zeros"""
    B, H, D = q.shape
    S, live = kv_scores(q, ck, lens, Ak, H_kv, scale, bk, rope)
    live = live.to(S.device)
    V = rebuild(cv, Av, bv, H_kv, H)
    S = S.masked_fill(~live[:, None, :], float("-inf"))
    out = torch.zeros(B, H, D, dtype=torch.float64, device=S.device)
    for b in range(B):
        if live[b].any():
            p = torch.softmax(S[b], -1)
            p = torch.where(live[b][None, :], p, torch.zeros_like(p))
            out[b] = torch.einsum("ht,htd->hd", p[:, live[b]], V[b][:, live[b]])
    return out
