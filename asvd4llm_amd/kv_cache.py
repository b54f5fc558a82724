"""Inference on a LOW-RANK KV cache: what --compress_kv_cache buys at run time.

After the search, k_proj / v_proj are SVDLinear(BLinear: hidden -> r, ALinear: r -> H_kv * D).  The cache below keeps the r-wide BLinear
outputs (r_k + r_v values per token and layer) instead of K and V (2 * H_kv * D values); ALinear moves to the other side of the attention
product (csrc/lowrank_kv.hip, K20; DESIGN.md 4 "K20").

  LowRankKVCache      preallocated C_k / C_v buffers per layer and the lengths, host and device side; quant="int8" keeps a layer as 8-bit
                      codes and one fp32 scale per token and 32 columns (K21, csrc/lowrank_kv_q8.hip; DESIGN.md 4 "K21")
  LowRankKVAttention  prefill / decode of one attention layer on that cache; decode runs K20, or torch on the same cache on a refusal;
                      a bf16 layer takes the kernel only when asked (kv_bf16 / ASVD_KV_BF16=1: K22, DESIGN.md 4 "K22")
  greedy_decode       a runner for Llama-family HF models that owns its loop (no transformers attention or cache class is patched)
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


def kv_bf16_enabled():
    """decode attention of a bf16 layer on the K20 kernels is opt-in (ASVD_KV_BF16=1, or kv_bf16=True on LowRankKVAttention / greedy_decode):
    the bf16 form of csrc/lowrank_kv.hip (K22) rounds q~, p and the output to bf16 where torch's bf16 route rounds K, V and its own
    intermediates, so the output bits of a bf16 model change with the switch.  Off, a bf16 layer answers "not fp16" and decodes in torch."""
    return os.environ.get("ASVD_KV_BF16", "0") == "1"


class FactorPair(nn.Module):
    """y = ALinear(BLinear(x)): the shape of SVDLinear from two given nn.Linear (no factorisation, works on the CPU)"""

    def __init__(self, BLinear, ALinear):
        super().__init__()
        self.BLinear, self.ALinear = BLinear, ALinear

    def forward(self, x):
        return self.ALinear(self.BLinear(x))


class _TokenCache:
    """[B, Tmax, width] buffers per layer, filled from the front; lengths per layer and sequence on the host (bookkeeping, no sync) and on
    the device (int32, what the kernel reads).  quant: None, "int8", or one of the two per layer.  An int8 layer holds ck / cv as int8 codes and
    sk / sv as their fp32 group scales [B, Tmax, ceil(width / 32)] (sk / sv are None for the other layers); dtype then is the type read() answers in."""

    def __init__(self, n_layers, batch, max_tokens, widths, device, dtype=torch.float16, quant=None):
        if n_layers < 1 or batch < 1 or max_tokens < 1:
            raise ValueError("cache needs n_layers, batch, max_tokens >= 1")
        if isinstance(widths[0], int):
            widths = [tuple(widths)] * n_layers
        if len(widths) != n_layers or any(len(w) != 2 or min(w) < 1 for w in widths):
            raise ValueError("one (key width, value width) pair for the cache, or one per layer")
        self.n_layers, self.batch, self.max_tokens, self.widths = n_layers, batch, max_tokens, [tuple(int(x) for x in w) for w in widths]
        self.device, self.dtype = torch.device(device), dtype
        quant = [quant] * n_layers if quant is None or isinstance(quant, str) else list(quant)
        if len(quant) != n_layers or any(q not in (None, "int8") for q in quant):
            raise ValueError('quant is None, "int8", or a list with one of the two per layer')
        if any(q and (w[0] % 16 or w[1] % 16) for q, w in zip(quant, self.widths)):
            raise ValueError("an int8 layer needs widths that are multiples of 16")
        self.quant = quant
        kinds = [torch.int8 if q else dtype for q in quant]
        self.ck = [torch.empty(batch, max_tokens, w[0], dtype=k, device=self.device) for w, k in zip(self.widths, kinds)]
        self.cv = [torch.empty(batch, max_tokens, w[1], dtype=k, device=self.device) for w, k in zip(self.widths, kinds)]
        scales = lambda i: [torch.empty(batch, max_tokens, ops.lowrank_kv_groups(w[i]), dtype=torch.float32, device=self.device) if q else None
                            for w, q in zip(self.widths, quant)]
        self.sk, self.sv = scales(0), scales(1)
        self.lens = torch.zeros(n_layers, batch, dtype=torch.int32, device=self.device)
        self.host_lens = [[0] * batch for _ in range(n_layers)]

    def reset(self):
        self.lens.zero_()
        self.host_lens = [[0] * self.batch for _ in range(self.n_layers)]

    def _store(self, layer, seqs, t0, c, ck_rows, cv_rows):
        """rows [len(seqs), c, width] into positions t0 .. t0 + c of the sequences `seqs` (a slice).  An int8 layer quantises them: with the
        kernel when they are fp16 or bf16 on the device (bf16 rows through .half(): the format is defined on fp16 values), with the same
        definition in torch otherwise (through .half() as well).  Codes and scales are the same bits either way.  A bf16 latent beyond
        65504 is an Inf in fp16 and turns its group into a NaN group, as it does in the torch definition."""
        if c == 0:
            return
        if not self.quant[layer]:
            self.ck[layer][seqs, t0:t0 + c] = ck_rows
            self.cv[layer][seqs, t0:t0 + c] = cv_rows
            return
        for codes, scales, rows in ((self.ck[layer], self.sk[layer], ck_rows), (self.cv[layer], self.sv[layer], cv_rows)):
            if rows.is_cuda and rows.dtype in (torch.float16, torch.bfloat16):
                if rows.dtype == torch.bfloat16:
                    rows = rows.half()
                if rows.stride(2) != 1 or rows.stride(1) % 8 or rows.stride(0) % 8 or rows.data_ptr() % 16:
                    rows = rows.contiguous()
                ops.lowrank_kv_quant(rows, codes[seqs, t0:t0 + c], scales[seqs, t0:t0 + c])
            else:
                q, sc = ops.lowrank_kv_quant_torch(rows)
                codes[seqs, t0:t0 + c] = q
                scales[seqs, t0:t0 + c] = sc

    def read(self, layer, T, dtype=None):
        """(C_k, C_v) of the first T tokens of `layer` in `dtype` (default: the cache's): the values decode attends to, dequantised for an
        int8 layer (fp16 values, K21's d = fp16(code * s)), a plain slice otherwise"""
        dtype = dtype or self.dtype
        if not self.quant[layer]:
            return self.ck[layer][:, :T].to(dtype), self.cv[layer][:, :T].to(dtype)
        return (ops.lowrank_kv_dequant(self.ck[layer][:, :T], self.sk[layer][:, :T]).to(dtype),
                ops.lowrank_kv_dequant(self.cv[layer][:, :T], self.sv[layer][:, :T]).to(dtype))

    def append(self, layer, ck_new, cv_new, counts=None):
        """append ck_new / cv_new [B, n, width] to `layer`: a prefill chunk (n > 1) or one token.  counts: valid new tokens per sequence
        (right-padded chunks), default n for all.  Returns the lengths before the append (host list).  Raises when a sequence would overflow."""
        wk, wv = self.widths[layer]
        B = self.batch
        if ck_new.dim() != 3 or cv_new.dim() != 3 or ck_new.shape[0] != B or cv_new.shape[0] != B or ck_new.shape[1] != cv_new.shape[1] \
                or ck_new.shape[2] != wk or cv_new.shape[2] != wv:
            raise ValueError(f"append: [B, n, {wk}] and [B, n, {wv}] expected (got {tuple(ck_new.shape)}, {tuple(cv_new.shape)})")
        n = ck_new.shape[1]
        counts = [n] * B if counts is None else [int(c) for c in counts]
        if len(counts) != B or any(c < 0 or c > n for c in counts):
            raise ValueError("append: one count in [0, n] per sequence")
        before = list(self.host_lens[layer])
        if any(before[b] + counts[b] > self.max_tokens for b in range(B)):
            raise IndexError(f"append: layer {layer} would pass max_tokens = {self.max_tokens} (lengths {before}, new {counts})")
        if len(set(before)) == 1 and len(set(counts)) == 1:
            t0, c = before[0], counts[0]
            self._store(layer, slice(None), t0, c, ck_new[:, :c], cv_new[:, :c])
            self.lens[layer] += c
        else:
            for b in range(B):
                self._store(layer, slice(b, b + 1), before[b], counts[b], ck_new[b:b + 1, :counts[b]], cv_new[b:b + 1, :counts[b]])
            self.lens[layer] += torch.tensor(counts, dtype=torch.int32).to(self.device)
        self.host_lens[layer] = [before[b] + counts[b] for b in range(B)]
        return before

    def bytes_per_token(self, layer=None):
        """bytes one token occupies in this cache: in `layer`, or in all layers together"""
        size = torch.empty(0, dtype=self.dtype).element_size()
        layers = range(self.n_layers) if layer is None else [layer]
        q8 = lambda w: w + 4 * ops.lowrank_kv_groups(w)   # a byte per code, an fp32 scale per 32 columns
        return sum(sum(q8(w) for w in self.widths[i]) if self.quant[i] else sum(self.widths[i]) * size for i in layers)

    def dense_bytes_per_token(self, H_kv, D, layer=None):
        """bytes of the full K and V of one token: the cache this one replaces"""
        size = torch.empty(0, dtype=self.dtype).element_size()
        return 2 * H_kv * D * size * (self.n_layers if layer is None else 1)


class LowRankKVCache(_TokenCache):
    """LowRankKVCache(n_layers, batch, max_tokens, ranks, device, quant=None): ranks = (r_k, r_v), or one pair per layer.  ck[layer] / cv[layer]
    are the BLinear outputs of k_proj / v_proj, [B, max_tokens, r] fp16; lens[layer] the int32 device lengths K20 reads.  quant="int8" (or a list
    with None / "int8" per layer): ck / cv are int8 codes and sk / sv their fp32 scales (K21); append still takes fp16 rows, read() dequantises."""


class DenseKVCache(_TokenCache):
    """the ordinary cache in the same interface: ck / cv hold the (rotated) K and V, [B, max_tokens, H_kv * D]"""

    def __init__(self, n_layers, batch, max_tokens, H_kv, D, device, dtype=torch.float16):
        super().__init__(n_layers, batch, max_tokens, (H_kv * D, H_kv * D), device, dtype)


def rotate_half(x, cos, sin):
    """x [..., D] with the pairs (i, i + D/2) rotated by cos / sin [..., D/2] (broadcast against x's leading dimensions)"""
    half = x.shape[-1] // 2
    lo, hi = x[..., :half], x[..., half:]
    return torch.cat([lo * cos - hi * sin, hi * cos + lo * sin], -1)


def _plain_linear(m):
    return type(m) is nn.Linear and not (m._forward_hooks or m._forward_pre_hooks or m._backward_hooks)


class LowRankKVAttention(nn.Module):
    """One attention layer on a low-rank cache.  q_proj / o_proj: any module; k_proj / v_proj: modules with BLinear and ALinear
    (SVDLinear).  n_heads / n_kv_heads; scale (default D^-1/2); rope = None (no positional rotation: OPT) or (cos, sin) fp32 tables
    [>= max_tokens, D/2] from ops.rope_table (Llama).  kernel=False keeps everything in torch (also on the CPU).  kv_bf16: whether a bf16
    layer (hidden, ALinear weights and biases all bf16) decodes on the kernel's bf16 form (K22); None reads ASVD_KV_BF16=1 (kv_bf16_enabled)."""

    def __init__(self, q_proj, k_proj, v_proj, o_proj, n_heads, n_kv_heads=None, scale=None, rope=None, kernel=True, kv_bf16=None):
        super().__init__()
        for name, m in (("k_proj", k_proj), ("v_proj", v_proj)):
            if not (hasattr(m, "BLinear") and hasattr(m, "ALinear")):
                raise TypeError(f"{name} is not a factor pair (BLinear, ALinear): nothing low-rank to cache")
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = q_proj, k_proj, v_proj, o_proj
        self.n_heads, self.n_kv_heads = int(n_heads), int(n_kv_heads or n_heads)
        self.head_dim = k_proj.ALinear.out_features // self.n_kv_heads
        self.scale = float(scale) if scale is not None else self.head_dim ** -0.5
        self.rope = rope
        self.kernel = bool(kernel)
        self.kv_bf16 = kv_bf16_enabled() if kv_bf16 is None else bool(kv_bf16)
        self._work = {}

    @property
    def ranks(self):
        return self.k_proj.BLinear.out_features, self.v_proj.BLinear.out_features

    # ---- the pieces both paths share -------------------------------------------------------------------------------------------------
    def _rope_rows(self, pos, dtype):
        cos, sin = self.rope
        return cos[pos].to(dtype), sin[pos].to(dtype)

    def _project(self, hidden, cache, layer):
        """q [B, n, H, D] (rotated), and the new tokens' BLinear outputs appended to the cache; returns q and the positions [B, n]"""
        B, n, _ = hidden.shape
        ck_new, cv_new = self.k_proj.BLinear(hidden), self.v_proj.BLinear(hidden)
        before = cache.append(layer, ck_new.to(cache.dtype), cv_new.to(cache.dtype))
        pos = torch.tensor(before, device=hidden.device)[:, None] + torch.arange(n, device=hidden.device)[None, :]
        q = self.q_proj(hidden).view(B, n, self.n_heads, self.head_dim)
        if self.rope is not None:
            cos, sin = self._rope_rows(pos, torch.float32)
            q = rotate_half(q.float(), cos[:, :, None, :], sin[:, :, None, :]).to(hidden.dtype)
        return q, pos

    def _attend_torch(self, q, pos, cache, layer):
        """reconstruct K and V of the cached tokens through ALinear and attend with torch SDPA; query i of sequence b sees t <= pos[b, i]"""
        B, n = pos.shape
        T = max(cache.host_lens[layer])
        dt = q.dtype
        ck, cv = cache.read(layer, T, dt)
        K = self.k_proj.ALinear(ck).view(B, T, self.n_kv_heads, self.head_dim)
        V = self.v_proj.ALinear(cv).view(B, T, self.n_kv_heads, self.head_dim)
        if self.rope is not None:
            cos, sin = self._rope_rows(torch.arange(T, device=q.device), torch.float32)
            K = rotate_half(K.float(), cos[None, :, None, :], sin[None, :, None, :]).to(dt)
        rep = self.n_heads // self.n_kv_heads
        K, V = K.transpose(1, 2), V.transpose(1, 2)
        if rep > 1:
            K, V = K.repeat_interleave(rep, 1), V.repeat_interleave(rep, 1)
        mask = torch.arange(T, device=q.device)[None, None, None, :] <= pos[:, None, :, None]
        o = F.scaled_dot_product_attention(q.transpose(1, 2), K, V, attn_mask=mask, scale=self.scale)
        return o.transpose(1, 2).reshape(B, n, self.n_heads * self.head_dim)

    # ---- public ------------------------------------------------------------------------------------------------------------------------
    def refusal(self, hidden):
        """why decode(hidden, ...) would not take the K20 kernel: a short reason, or None when it does"""
        kA, kB, vA, vB = self.k_proj.ALinear, self.k_proj.BLinear, self.v_proj.ALinear, self.v_proj.BLinear
        if not self.kernel:
            return "switched off"
        if not all(type(m) is nn.Linear for m in (kA, kB, vA, vB)):
            return "packed factors"
        if not all(_plain_linear(m) for m in (kA, kB, vA, vB)) or self.k_proj._forward_hooks or self.v_proj._forward_hooks:
            return "hooks"
        if hidden.dim() != 3 or hidden.shape[1] != 1:
            return "token count"
        if hidden.dtype == torch.bfloat16 and self.kv_bf16:   # K22: one dtype for the query, the factors and their biases
            if any(t is not None and t.dtype != torch.bfloat16 for t in (kA.weight, vA.weight, kA.bias, vA.bias)):
                return "mixed dtypes"
        elif not (hidden.dtype == torch.float16 and kA.weight.dtype == torch.float16 and vA.weight.dtype == torch.float16):
            return "not fp16"
        if self.head_dim not in (64, 128) or self.n_heads % self.n_kv_heads:
            return "head size"
        if any(r < 16 or r % 16 for r in self.ranks):
            return "ranks"
        if self.rope is not None and kA.bias is not None:
            return "key bias under rotation"
        if torch.is_grad_enabled() and hidden.requires_grad:
            return "autograd"
        if not (hidden.is_cuda and kA.weight.device == hidden.device and vA.weight.device == hidden.device):
            return "not on the device"
        return None

    def prefill(self, hidden, cache, layer):
        """hidden [B, n, hidden] (a whole prompt or a chunk of it): BLinear once, append, causal attention the ordinary way"""
        q, pos = self._project(hidden, cache, layer)
        return self.o_proj(self._attend_torch(q, pos, cache, layer))

    def decode(self, hidden, cache, layer):
        """hidden [B, 1, hidden]: one new token per sequence"""
        why = self.refusal(hidden)
        q, pos = self._project(hidden, cache, layer)
        if why is not None:
            return self.o_proj(self._attend_torch(q, pos, cache, layer))
        B = hidden.shape[0]
        r_k, r_v = self.ranks
        key = (hidden.device.index, torch.cuda.current_stream(hidden.device).cuda_stream, B, cache.max_tokens)
        work = self._work.get(key)
        if work is None:
            work = self._work[key] = ops.lowrank_kv_work(B, self.n_heads, cache.max_tokens, r_k, r_v, hidden.device)
        kA, vA = self.k_proj.ALinear, self.v_proj.ALinear
        q3 = q.reshape(B, self.n_heads, self.head_dim).contiguous()
        kw = dict(bk=kA.bias.detach() if kA.bias is not None else None, bv=vA.bias.detach() if vA.bias is not None else None, rope=self.rope, work=work)
        if cache.quant[layer]:   # K21: the same stages on codes and scales
            o = ops.lowrank_kv_decode_q8(q3, cache.ck[layer], cache.cv[layer], cache.sk[layer], cache.sv[layer], cache.lens[layer],
                                         kA.weight.detach(), vA.weight.detach(), self.n_kv_heads, self.scale, **kw)
        else:
            o = ops.lowrank_kv_decode(q3, cache.ck[layer], cache.cv[layer], cache.lens[layer], kA.weight.detach(), vA.weight.detach(),
                                      self.n_kv_heads, self.scale, **kw)
        return self.o_proj(o.view(B, 1, self.n_heads * self.head_dim))


class _DenseAttention(nn.Module):
    """the same layer on the ordinary cache (rotated K and V in full): the baseline of greedy_decode(cache="dense")"""

    def __init__(self, q_proj, k_proj, v_proj, o_proj, n_heads, n_kv_heads, scale, rope):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = q_proj, k_proj, v_proj, o_proj
        self.n_heads, self.n_kv_heads, self.scale, self.rope = n_heads, n_kv_heads, scale, rope
        self.head_dim = q_proj.out_features // n_heads

    def prefill(self, hidden, cache, layer):
        B, n, _ = hidden.shape
        pos = torch.tensor(cache.host_lens[layer], device=hidden.device)[:, None] + torch.arange(n, device=hidden.device)[None, :]
        q = self.q_proj(hidden).view(B, n, self.n_heads, self.head_dim)
        k = self.k_proj(hidden).view(B, n, self.n_kv_heads, self.head_dim)
        if self.rope is not None:
            cos, sin = self.rope[0][pos][:, :, None, :], self.rope[1][pos][:, :, None, :]
            q, k = rotate_half(q.float(), cos, sin).to(hidden.dtype), rotate_half(k.float(), cos, sin).to(hidden.dtype)
        cache.append(layer, k.reshape(B, n, -1).to(cache.dtype), self.v_proj(hidden).to(cache.dtype))
        T = max(cache.host_lens[layer])
        K, V = cache.read(layer, T, hidden.dtype)
        K = K.view(B, T, self.n_kv_heads, self.head_dim).transpose(1, 2)
        V = V.view(B, T, self.n_kv_heads, self.head_dim).transpose(1, 2)
        rep = self.n_heads // self.n_kv_heads
        if rep > 1:
            K, V = K.repeat_interleave(rep, 1), V.repeat_interleave(rep, 1)
        mask = torch.arange(T, device=hidden.device)[None, None, None, :] <= pos[:, None, :, None]
        o = F.scaled_dot_product_attention(q.transpose(1, 2), K, V, attn_mask=mask, scale=self.scale)
        return self.o_proj(o.transpose(1, 2).reshape(B, n, self.n_heads * self.head_dim))

    decode = prefill


def is_llama_family(model):
    """the attribute names greedy_decode walks"""
    try:
        layer = model.model.layers[0]
        return all(hasattr(layer.self_attn, n) for n in ("q_proj", "k_proj", "v_proj", "o_proj")) and hasattr(layer, "input_layernorm") \
            and hasattr(layer, "post_attention_layernorm") and hasattr(layer, "mlp") and hasattr(model.model, "norm") and hasattr(model, "lm_head") \
            and hasattr(model.model, "embed_tokens")
    except (AttributeError, IndexError, TypeError):
        return False


def rope_theta_of(config):
    """the rotary base as the installed transformers exposes it: config.rope_parameters["rope_theta"] (5.x) or config.rope_theta"""
    params = getattr(config, "rope_parameters", None)
    if isinstance(params, dict) and "rope_theta" in params:
        kind = params.get("rope_type", "default")
        if kind != "default":
            raise NotImplementedError(f"greedy_decode serves the default rotary embedding only (config has rope_type {kind})")
        return float(params["rope_theta"])
    return float(getattr(config, "rope_theta", 10000.0))


def _is_pair(m):
    return hasattr(m, "BLinear") and hasattr(m, "ALinear")


def kv_ranks(model):
    """(key width, value width) the cache of greedy_decode(cache="lowrank") keeps per token in every layer of a Llama-family model:
    (r_k, r_v) where k_proj and v_proj are both factor pairs; a layer the search left uncompressed keeps the full (H_kv * D, H_kv * D)"""
    out = []
    for l in model.model.layers:
        k, v = l.self_attn.k_proj, l.self_attn.v_proj
        if _is_pair(k) and _is_pair(v):
            out.append((k.BLinear.out_features, v.BLinear.out_features))
        else:
            out.append(((k.ALinear if _is_pair(k) else k).out_features, (v.ALinear if _is_pair(v) else v).out_features))
    return out


def decode_routes(model, kernel=True, kv_bf16=None):
    """what greedy_decode(model, ..., cache="lowrank", kernel=kernel, kv_bf16=kv_bf16) does with a decode step, per layer: "kernel" (K20),
    the refusal reason of LowRankKVAttention (torch on the low-rank cache), or "uncompressed" (the layer keeps its K and V).  Host only."""
    cfg = model.config
    H, H_kv = cfg.num_attention_heads, getattr(cfg, "num_key_value_heads", None) or cfg.num_attention_heads
    out = []
    for l in model.model.layers:
        a = l.self_attn
        if not (_is_pair(a.k_proj) and _is_pair(a.v_proj)):
            out.append("uncompressed")
            continue
        w = a.k_proj.ALinear.weight if hasattr(a.k_proj.ALinear, "weight") else None
        probe = torch.empty(1, 1, 1, dtype=w.dtype if w is not None else torch.float16, device=w.device if w is not None else "cpu")
        why = LowRankKVAttention(a.q_proj, a.k_proj, a.v_proj, a.o_proj, H, H_kv, 1.0, (None, None), kernel, kv_bf16).refusal(probe)   # rope: the runner always rotates
        out.append("kernel" if why is None else why)
    return out


@torch.no_grad()
def greedy_decode(model, input_ids, n_new, cache="lowrank", kernel=True, forced=None, kv_quant=None, kv_bf16=None):
    """Greedy decoding of a Llama-family HF model with this module's caches: prefill input_ids [B, n], then one token per step.
    cache="lowrank": where k_proj / v_proj are factor pairs the cache holds their BLinear outputs and decode steps run K20 (kernel=True) or
    torch on the same cache (kernel=False, also on the CPU); a layer the search left uncompressed keeps its K and V.  cache="dense": the ordinary K / V cache, any k_proj / v_proj.
    kv_quant="int8" (cache="lowrank" only): the layers whose k_proj and v_proj are both factor pairs keep their latents as int8 codes (K21) and
    decode on them; an uncompressed layer keeps its fp16 K and V.
    kv_bf16: passed to LowRankKVAttention (a bf16 model's decode steps on the kernel, K22; None reads ASVD_KV_BF16=1).
    forced [B, n_new] (optional): the tokens fed back instead of the runner's own choices, to compare runs on one token stream.
    Returns (tokens [B, n_new], logits [n_new, B, vocab]): logits[s] chose tokens[:, s]."""
    if not is_llama_family(model):
        raise TypeError("greedy_decode walks model.model.layers[i].{input_layernorm, self_attn.{q,k,v,o}_proj, post_attention_layernorm, mlp}, "
                        "model.model.norm and lm_head: this model does not have them")
    if cache not in ("lowrank", "dense"):
        raise ValueError('cache is "lowrank" or "dense"')
    if n_new < 1:
        raise ValueError("n_new >= 1")
    if kv_quant not in (None, "int8") or (kv_quant and cache != "lowrank"):
        raise ValueError('kv_quant is None or "int8", and only the low-rank cache is quantised')
    cfg = model.config
    H, H_kv = cfg.num_attention_heads, getattr(cfg, "num_key_value_heads", None) or cfg.num_attention_heads
    D = getattr(cfg, "head_dim", None) or cfg.hidden_size // H
    layers = model.model.layers
    dev = input_ids.device
    B, n = input_ids.shape
    Tmax = n + n_new
    dtype = layers[0].self_attn.q_proj.weight.dtype if hasattr(layers[0].self_attn.q_proj, "weight") else torch.float16
    rope = ops.rope_table(Tmax, D, rope_theta_of(cfg), dev)
    scale = D ** -0.5
    if cache == "lowrank":
        pairs = [_is_pair(l.self_attn.k_proj) and _is_pair(l.self_attn.v_proj) for l in layers]
        # an uncompressed layer keeps K and V (never quantised) in its slot of the same cache
        kv = LowRankKVCache(len(layers), B, Tmax, kv_ranks(model), dev, dtype, quant=[kv_quant if p else None for p in pairs])
        attn = [(LowRankKVAttention(a.q_proj, a.k_proj, a.v_proj, a.o_proj, H, H_kv, scale, rope, kernel, kv_bf16) if _is_pair(a.k_proj) and _is_pair(a.v_proj)
                 else _DenseAttention(a.q_proj, a.k_proj, a.v_proj, a.o_proj, H, H_kv, scale, rope)) for a in (l.self_attn for l in layers)]
    else:
        kv = DenseKVCache(len(layers), B, Tmax, H_kv, D, dev, dtype)
        attn = [_DenseAttention(l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.o_proj, H, H_kv, scale, rope) for l in layers]

    def step(ids, first):
        x = model.model.embed_tokens(ids)
        for i, l in enumerate(layers):
            h = l.input_layernorm(x)
            x = x + (attn[i].prefill(h, kv, i) if first else attn[i].decode(h, kv, i))
            x = x + l.mlp(l.post_attention_layernorm(x))
        return model.lm_head(model.model.norm(x[:, -1:]))[:, 0]

    tokens, logits = [], []
    ids = input_ids
    for s in range(n_new):
        lg = step(ids, s == 0)
        logits.append(lg)
        tokens.append(lg.argmax(-1, keepdim=True))
        ids = tokens[-1] if forced is None else forced[:, s:s + 1].to(dev)
    return torch.cat(tokens, 1), torch.stack(logits, 0)
