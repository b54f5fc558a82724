"""What the packed Linear modules (w8_linear.W8Linear: one code per byte; wb_linear.WBLinear: codes at their own width) have in common: the
protection of the buffers that define the weight against dtype casts of the model, the conditions under which forward() takes a kernel, and
the dequantize + F.linear path every other input takes."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

# Token count up to which an input beyond decode size takes the token-tiled GEMM on the codes (K17, csrc/w8_linear.hip: ops.packed_gemm) once it
# is switched on (packed_gemm_enabled): the largest measured token count at which that kernel is no slower than dequantize + F.linear, the path
# these inputs take otherwise (tools/bench_w8_forward.py --gemm on MI355X, graph replay, profiles/w8_gemm.json, DESIGN.md section 4 "K17").  On the
# Llama-2-7B plain set the kernel takes 0.56 / 0.57 / 0.74 / 0.86 of the dense path's time at 32 / 64 / 128 / 256 tokens with byte codes (0.49 /
# 0.52 / 0.72 / 0.86 with 4-bit rows) and 1.30 / 1.34 at 512 / 2048 (1.42 / 1.36); on the ASVD-0.9 rank_align 128 factor set 0.58 / 0.60 / 0.64 /
# 0.84, then 1.04 / 1.30.  6-bit rows and group-wise scales (measured on 8 of the 32 blocks) cross between 256 and 512 as well; byte codes with
# groups of 64 on the plain set are level at 256 (1.007, inside the dense path's spread).  Above the constant the dense path is faster and costs an
# out x in fp16 temporary per call (90 MB for an 11008 x 4096 layer).
# bf16 inputs (packed_bf16_enabled) take the same constant.  Measured once for bf16 (tools/bench_w8_forward.py --gemm --dtype bf16, one run on one
# MI355X, profiles/w8_forward_bf16.json): against dequantize + F.linear in bf16 the kernel takes 0.55 / 0.56 / 0.73 / 0.85 of the time at 32 / 64 /
# 128 / 256 tokens with byte codes on the plain set and 1.31 / 1.34 at 512 / 2048 (ASVD-0.9 set 0.58 / 0.59 / 0.63 / 0.83, then 1.04 / 1.30; 4-bit
# rows with G = 128 on 8 blocks 0.54 / 0.56 / 0.77 / 0.88, then 1.47 / 1.52): the fp16 crossover, between 256 and 512.
PACKED_GEMM_MAX_TOKENS = 256


def packed_gemm_enabled():
    """The token-tiled GEMM on the codes is opt-in (ASVD_PACKED_GEMM=1, or `module.packed_gemm = True` on one packed Linear): it avoids the
    out x in fp16 temporary of dequantize + F.linear; off, every input beyond decode size keeps that path."""
    return os.environ.get("ASVD_PACKED_GEMM", "0") == "1"


def packed_bf16_enabled():
    """bf16 inputs on the packed-weight kernels are opt-in (ASVD_PACKED_BF16=1, or `module.packed_bf16 = True` on one packed Linear or
    SVDLinear): the kernels of csrc/w8_linear.hip in their bf16 form (K19), for a module whose weight_dtype and bias are bf16 as well, under the
    token thresholds of the fp16 form.  Measured in one run only (profiles/w8_forward_bf16.json, DESIGN.md section 4 "K19"), hence still a
    switch; off, a bf16 input keeps dequantize + F.linear."""
    return os.environ.get("ASVD_PACKED_BF16", "0") == "1"


class PackedLinear(nn.Module):
    """base of the packed Linears.  A subclass registers `scales`, `zeros` (fp32 [out]) and `bias` (weight_dtype [out] or None) next to its
    codes, sets `out_features` and `weight_dtype`, and provides dequantize() and kernel_rows_ok()."""

    def _apply(self, fn, *args, **kwargs):
        # The buffers DEFINE the weight: a dtype cast of the model (.half(), .double(), .to(dtype)) must not touch the fp32 scales and zeros,
        # and the bias stays in weight_dtype with the weight it belongs to.  Device moves go through.  forward() casts to the input's dtype.
        keep = {n: getattr(self, n) for n in ("scales", "zeros", "bias") if getattr(self, n) is not None}
        super()._apply(fn, *args, **kwargs)
        for n, old in keep.items():
            new = getattr(self, n)
            if new.dtype != old.dtype:
                setattr(self, n, old.to(new.device))
        return self

    def _kernel_dtype_ok(self, x, bf16=None):
        """input, weight and bias are ALL fp16, or ALL bf16 with the bf16 form switched on (`bf16`: the caller's own switch; None: this
        module's, packed_bf16_enabled).  Mixed dtypes never take a kernel."""
        dt = self.weight_dtype
        if x.dtype != dt or (self.bias is not None and self.bias.dtype != dt):
            return False
        if dt == torch.bfloat16:
            return bool(getattr(self, "packed_bf16", False) or packed_bf16_enabled()) if bf16 is None else bool(bf16)
        return dt == torch.float16

    def _kernel_input(self, x, max_tokens, bf16=None):
        """x as the contiguous 16-byte-aligned [tokens, in] fp16 (or, switched on, bf16: _kernel_dtype_ok) matrix the forward kernels take, or
        None when this input goes through dequantize + F.linear: not on the device, not of the kernels' dtype (input, weight or bias), more than
        max_tokens tokens, under autograd, or code rows that do not allow 16-byte loads"""
        tokens = x.numel() // x.shape[-1] if x.shape[-1] else 0
        if not (x.is_cuda and self._kernel_dtype_ok(x, bf16) and 0 < tokens <= max_tokens
                and not (torch.is_grad_enabled() and x.requires_grad) and self.kernel_rows_ok()):
            return None
        x2d = x.reshape(-1, x.shape[-1])
        x2d = x2d if x2d.is_contiguous() else x2d.contiguous()
        return x2d if x2d.data_ptr() % 16 == 0 else None

    def _gemm_input(self, x, decode_max_tokens):
        """x as _kernel_input gives it when it goes to the token-tiled GEMM (K17): switched on, more tokens than the decode kernel takes
        (`decode_max_tokens`), at most PACKED_GEMM_MAX_TOKENS, and the conditions of _kernel_input; None otherwise"""
        if not (getattr(self, "packed_gemm", False) or packed_gemm_enabled()):
            return None
        x2d = self._kernel_input(x, PACKED_GEMM_MAX_TOKENS)
        return x2d if x2d is not None and x2d.shape[0] > decode_max_tokens else None

    def _dense_forward(self, x):
        w, b = self.dequantize(), self.bias
        if x.dtype != w.dtype:   # a model cast to another dtype: the same weight, converted for the GEMM (exact into a wider type)
            w, b = w.to(x.dtype), None if b is None else b.to(x.dtype)
        return F.linear(x, w, b)
