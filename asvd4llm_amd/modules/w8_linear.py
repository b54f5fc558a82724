"""W8Linear — a Linear whose RTN-quantized weight stays packed: uint8 codes plus one fp32 scale and zero per output row.

The weight it stands for is  w[n, k] = (scales[n] * (qweight[n, k] - zeros[n])).to(weight_dtype),  the value the fake quantizer
(quantization.rtn_quant_sequential) writes into an nn.Linear, bit for bit.  Decode-sized fp16 inputs run on the W8A16 kernel of
csrc/w8_linear.hip, which dequantizes to exactly that value in registers (bf16 inputs of a bf16 module too once ASVD_PACKED_BF16=1 or
`packed_bf16 = True` switches them on, modules/packed_linear.py); every other input dequantizes the layer's weight into a temporary
(csrc/w8_linear.hip as well) and calls F.linear on it, so the model's resident size stays packed.  Opt-in (ASVD_PACKED_GEMM=1 or `packed_gemm = True`,
modules/packed_linear.py): fp16 inputs of 17 .. PACKED_GEMM_MAX_TOKENS tokens run on the token-tiled GEMM on the codes instead (K17), without the temporary.

Not an nn.Linear subclass on purpose: collect_linear_info, the calibration hooks and quantization._find_linears select nn.Linear modules and
must keep ignoring packed ones.

Group-wise scales (`group_size` 64 or 128, K14): `scales` / `zeros` are [out, ceil(in / group_size)], one pair per group of that many input
columns, w[n, k] = (scales[n, k // G] * (qweight[n, k] - zeros[n, k // G])).to(weight_dtype); `group_size` 0 is the per-row form above."""
import torch
import torch.nn as nn

from .. import ops
from .packed_linear import PackedLinear

# Token count up to which forward() takes the kernel: the measured crossover (tools/bench_w8_forward.py --force_kernel --tokens 1,4,16,32,64 on
# MI355X, profiles/w8_forward.json).  Against the fake-quantized fp16 weights through nn.Linear on the Llama-2-7B ASVD-0.9
# shape set with rank_align 128 the packed pass takes 0.72 / 0.73 / 0.86 of the time at 1 / 4 / 16 tokens in device time (graph replay; 0.69 / 0.70 /
# 0.76 eager) and 1.07 / 1.28 at 32 / 64 (the kernel re-reads x once per workgroup, which costs more than the halved weight stream saves from 32
# tokens on).  These figures hold for rows that allow 16-byte loads only: see W8Linear.kernel_rows_ok.
# Layers with group-wise scales take the same constant: NOT MEASURED for grouped scales (the grouped kernel streams 8 bytes per group more;
# tools/bench_w8_forward.py --group_size measures it next to the per-row pass on the same codes).
# bf16 inputs (opt-in, packed_linear.packed_bf16_enabled) take the same constant.  Measured once for bf16 (--dtype bf16 --force_kernel --tokens
# 1,4,16,32,64 of the same tool, one run, profiles/w8_forward_bf16.json): against bf16 nn.Linear on the fake-quantized weights the packed pass takes
# 0.64 / 0.65 / 0.76 of the time at 1 / 4 / 16 tokens in graph time on the ASVD-0.9 set and 1.07 / 1.29 at 32 / 64 (plain set 0.60 / 0.61 / 0.69,
# then 1.08 / 1.12), and 0.38 / 0.39 / 0.45 of dequantize + F.linear in bf16, the path a bf16 module takes with the switch off: the fp16 crossover.
W8_FORWARD_MAX_TOKENS = 16


def param_shape(out_features, in_features, group_size):
    """shape of `scales` / `zeros`: [out] per row, [out, ceil(in / group_size)] per group"""
    g = ops._group(group_size)
    return (int(out_features), ops.n_groups(in_features, g)) if g else (int(out_features),)


def expand_groups(p, in_features, group_size):
    """scales / zeros as a column ([out, 1]) or, grouped, spread over their columns ([out, in]), for the torch form of dequantize()"""
    if not group_size:
        return p[:, None]
    return p.repeat_interleave(group_size, dim=1)[:, :in_features]


class W8Linear(PackedLinear):
    """y = x w^T + bias with w held as `qweight` uint8 [out, in], `scales` fp32 [out], `zeros` fp32 [out] (persistent buffers: they are what
    state_dict() and save_pretrained() write) and an optional `bias` buffer in the original dtype."""

    def __init__(self, in_features, out_features, bias=True, bits=8, weight_dtype=torch.float16, device=None, group_size=0):
        super().__init__()
        if not 1 <= int(bits) <= 8:
            raise ValueError(f"bits must be in 1..8 (got {bits}): one code per byte")
        self.in_features, self.out_features, self.bits, self.weight_dtype = int(in_features), int(out_features), int(bits), weight_dtype
        self.group_size = ops._group(group_size)
        pshape = param_shape(self.out_features, self.in_features, self.group_size)
        self.register_buffer("qweight", torch.zeros((self.out_features, self.in_features), dtype=torch.uint8, device=device))
        self.register_buffer("scales", torch.zeros(pshape, dtype=torch.float32, device=device))
        self.register_buffer("zeros", torch.zeros(pshape, dtype=torch.float32, device=device))
        self.register_buffer("bias", torch.zeros(self.out_features, dtype=weight_dtype, device=device) if bias else None)

    @classmethod
    def from_codes(cls, qweight, scales, zeros, bias, bits, weight_dtype, group_size=0):
        """wrap the outputs of ops.rtn_quant_batched(..., want_params=True) without copying them"""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.out_features, self.in_features = (int(d) for d in qweight.shape)
        self.bits, self.weight_dtype, self.group_size = int(bits), weight_dtype, ops._group(group_size)
        pshape = param_shape(self.out_features, self.in_features, self.group_size)
        if self.group_size and (tuple(scales.shape) != pshape or tuple(zeros.shape) != pshape):
            raise ValueError(f"group_size={self.group_size}: scales / zeros must be {list(pshape)} (got {tuple(scales.shape)}, {tuple(zeros.shape)})")
        self.register_buffer("qweight", qweight)
        self.register_buffer("scales", scales)
        self.register_buffer("zeros", zeros)
        self.register_buffer("bias", bias)
        return self

    def dequantize(self):
        """the weight in weight_dtype.  CUDA: csrc/w8_linear.hip; CPU: the same arithmetic in torch (fp32 subtraction, one fp32 product, one
        rounding)"""
        if self.qweight.is_cuda:
            return ops.w8_dequant(self.qweight, self.scales, self.zeros, self.weight_dtype, group_size=self.group_size)
        sc, zr = (expand_groups(p, self.in_features, self.group_size) for p in (self.scales, self.zeros))
        return (sc * (self.qweight.float() - zr)).to(self.weight_dtype)

    def kernel_rows_ok(self):
        """the code rows allow the kernel's 16-byte loads: in_features % 16 == 0 and 16-byte-aligned contiguous storage.  Other rows (odd ranks:
        K = 1843) would run the kernel on element loads, measured 2-4x SLOWER than fp16 nn.Linear (profiles/w8_forward_align1.json): forward()
        keeps them off the kernel"""
        q = self.qweight
        return self.in_features % 16 == 0 and q.is_contiguous() and q.data_ptr() % 16 == 0

    def forward(self, x):
        x2d = self._kernel_input(x, W8_FORWARD_MAX_TOKENS)
        if x2d is not None:
            y = ops.w8_linear(x2d, self.qweight, self.scales, self.zeros, self.bias, group_size=self.group_size, weight_dtype=self.weight_dtype)
            return y.view(*x.shape[:-1], self.out_features)
        x2d = self._gemm_input(x, W8_FORWARD_MAX_TOKENS)   # opt-in (packed_linear.packed_gemm_enabled): the GEMM on the codes, one per byte
        if x2d is not None:
            y = ops.packed_gemm(x2d, self.qweight, 8, self.scales, self.zeros, self.bias, group_size=self.group_size,
                                weight_dtype=self.weight_dtype)
            return y.view(*x.shape[:-1], self.out_features)
        return self._dense_forward(x)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, bits={self.bits}, weight_dtype={self.weight_dtype}" + (
            f", group_size={self.group_size}" if self.group_size else "")
