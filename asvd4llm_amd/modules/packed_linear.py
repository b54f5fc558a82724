"""What the packed Linear modules (w8_linear.W8Linear: one code per byte; wb_linear.WBLinear: codes at their own width) have in common: the
protection of the buffers that define the weight against dtype casts of the model, the conditions under which forward() takes a kernel, and
the dequantize + F.linear path every other input takes."""
import torch
import torch.nn as nn
import torch.nn.functional as F


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

    def _kernel_input(self, x, max_tokens):
        """x as the contiguous 16-byte-aligned [tokens, in] fp16 matrix the forward kernels take, or None when this input goes through
        dequantize + F.linear: not on the device, not fp16 (input, weight or bias), more than max_tokens tokens, under autograd, or code rows
        that do not allow 16-byte loads"""
        tokens = x.numel() // x.shape[-1] if x.shape[-1] else 0
        if not (x.is_cuda and x.dtype == torch.float16 and self.weight_dtype == torch.float16 and 0 < tokens <= max_tokens
                and (self.bias is None or self.bias.dtype == torch.float16) and not (torch.is_grad_enabled() and x.requires_grad)
                and self.kernel_rows_ok()):
            return None
        x2d = x.reshape(-1, x.shape[-1])
        x2d = x2d if x2d.is_contiguous() else x2d.contiguous()
        return x2d if x2d.data_ptr() % 16 == 0 else None

    def _dense_forward(self, x):
        w, b = self.dequantize(), self.bias
        if x.dtype != w.dtype:   # a model cast to another dtype: the same weight, converted for the GEMM (exact into a wider type)
            w, b = w.to(x.dtype), None if b is None else b.to(x.dtype)
        return F.linear(x, w, b)
