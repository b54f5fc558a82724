"""WBLinear — a Linear whose RTN-quantized weight stays packed at the width of its codes: 6 or 4 bits per weight plus one fp32 scale and zero
per output row.  The sibling of W8Linear (one code per byte) for the widths that leave room.

The weight it stands for is  w[n, k] = (scales[n] * (code[n, k] - zeros[n])).to(weight_dtype),  the value the fake quantizer
(quantization.rtn_quant_sequential) writes into an nn.Linear, bit for bit.  `qbits` holds the codes of a row as a little-endian bitstream: code k
in bits [bits k, bits (k + 1)) of the row read as one little-endian integer, zero-padded to whole blocks of 64 codes, so a row is
ceil(in / 64) * 8 * bits bytes (csrc/w8_linear.hip, K13; the on-disk format "bitstream64" of export.py).  Decode-sized fp16 inputs run on the
kernel that unpacks in registers and gives the bits of the W8A16 kernel on the same codes; every other input dequantizes the layer's weight into
a temporary and calls F.linear on it.  Opt-in (ASVD_PACKED_GEMM=1 or `packed_gemm = True`, modules/packed_linear.py): fp16 inputs of 17 ..
PACKED_GEMM_MAX_TOKENS tokens run on the token-tiled GEMM on the bitstream rows instead (K17), without the temporary.

Neither an nn.Linear nor a W8Linear on purpose: the nn.Linear selections must keep ignoring packed layers and export.packed_layers_of must keep
telling the two storage forms apart.

Group-wise scales (`group_size` 64 or 128, K14): `scales` / `zeros` are [out, ceil(in / group_size)], one pair per group of that many input
columns, as in W8Linear; `group_size` 0 is the per-row form above.  4 bits with groups of 128 is 4.5 bits per weight."""
import torch
import torch.nn as nn

from .. import ops
from .packed_linear import PackedLinear
from .w8_linear import expand_groups, param_shape

# Token count up to which forward() takes the kernel.  NOT MEASURED for this kernel: the value is W8_FORWARD_MAX_TOKENS (modules/w8_linear.py),
# whose tile loop this kernel shares; tools/bench_w8_forward.py --code_bits 6 / 4 (with and without --force_kernel) measures WBLinear's own two
# paths.  The figures hold for rows that allow 16-byte loads only: see WBLinear.kernel_rows_ok.  Layers with group-wise scales take the same
# constant, NOT MEASURED for grouped scales either (--group_size of the same tool).  bf16 inputs (opt-in, packed_linear.packed_bf16_enabled) take
# it too; measured once for bf16 at 4 bits with G = 128 (--dtype bf16 --code_bits 4 --group_size 128 --tokens 1,4,16, one run,
# profiles/w8_forward_bf16.json): 0.46 / 0.47 / 0.54 of dequantize + F.linear in bf16 at 1 / 4 / 16 tokens in graph time on the ASVD-0.9 set (plain
# set 0.40 / 0.43 / 0.51); larger token counts NOT MEASURED for this kernel in bf16 either.
WB_FORWARD_MAX_TOKENS = 16

WB_BITS = (4, 6)


row_bytes = ops.wb_row_bytes   # ceil(cols / 64) * 8 * bits; ValueError for other widths


def pack_codes_torch(q, bits):
    """uint8 codes [rows, cols] -> bitstream rows [rows, row_bytes(cols, bits)], in torch (any device; the CPU form of ops.wb_pack)"""
    rows, cols = q.shape
    nb = row_bytes(cols, bits)
    c = torch.zeros((rows, (cols + 63) // 64 * 64), dtype=torch.int32, device=q.device)
    c[:, :cols] = q.to(torch.int32) & ((1 << bits) - 1)
    if bits == 4:       # two codes per byte
        out = c[:, 0::2] | (c[:, 1::2] << 4)
    else:               # four codes per three bytes
        c0, c1, c2, c3 = c[:, 0::4], c[:, 1::4], c[:, 2::4], c[:, 3::4]
        out = torch.stack((c0 | ((c1 & 3) << 6), (c1 >> 2) | ((c2 & 15) << 4), (c2 >> 4) | (c3 << 2)), dim=-1)
    return out.reshape(rows, nb).to(torch.uint8)


def unpack_codes_torch(qbits, bits, cols):
    """bitstream rows -> uint8 codes [rows, cols], in torch (any device)"""
    rows = qbits.shape[0]
    if qbits.shape[1] != row_bytes(cols, bits):
        raise ValueError(f"{tuple(qbits.shape)} is not the bitstream of [{rows}, {cols}] codes of {bits} bits")
    b = qbits.to(torch.int32)
    if bits == 4:
        c = torch.stack((b & 15, b >> 4), dim=-1)
    else:
        b0, b1, b2 = b[:, 0::3], b[:, 1::3], b[:, 2::3]
        c = torch.stack((b0 & 63, ((b0 >> 6) | (b1 << 2)) & 63, ((b1 >> 4) | (b2 << 4)) & 63, b2 >> 2), dim=-1)
    return c.reshape(rows, -1)[:, :cols].to(torch.uint8)


class WBLinear(PackedLinear):
    """y = x w^T + bias with w held as `qbits` uint8 [out, row_bytes(in, bits)], `scales` fp32 [out], `zeros` fp32 [out] (persistent buffers:
    they are what state_dict() and save_pretrained() write) and an optional `bias` buffer in the original dtype.  `in_features` is an attribute:
    the padded buffer does not tell it."""

    def __init__(self, in_features, out_features, bias=True, bits=6, weight_dtype=torch.float16, device=None, group_size=0):
        super().__init__()
        self.in_features, self.out_features, self.bits, self.weight_dtype = int(in_features), int(out_features), int(bits), weight_dtype
        self.group_size = ops._group(group_size)
        nb = row_bytes(self.in_features, self.bits)
        pshape = param_shape(self.out_features, self.in_features, self.group_size)
        self.register_buffer("qbits", torch.zeros((self.out_features, nb), dtype=torch.uint8, device=device))
        self.register_buffer("scales", torch.zeros(pshape, dtype=torch.float32, device=device))
        self.register_buffer("zeros", torch.zeros(pshape, dtype=torch.float32, device=device))
        self.register_buffer("bias", torch.zeros(self.out_features, dtype=weight_dtype, device=device) if bias else None)

    @classmethod
    def from_bits(cls, qbits, in_features, scales, zeros, bias, bits, weight_dtype, group_size=0):
        """wrap bitstream rows (ops.wb_pack) and the scale / zero of ops.rtn_quant_batched(..., want_params=True) without copying them"""
        if qbits.dim() != 2 or qbits.dtype != torch.uint8 or qbits.shape[1] != row_bytes(in_features, bits):
            raise ValueError(f"qbits {tuple(qbits.shape)} {qbits.dtype} is not the bitstream of {in_features} codes of {bits} bits per row")
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.out_features, self.in_features = int(qbits.shape[0]), int(in_features)
        self.bits, self.weight_dtype, self.group_size = int(bits), weight_dtype, ops._group(group_size)
        pshape = param_shape(self.out_features, self.in_features, self.group_size)
        if self.group_size and (tuple(scales.shape) != pshape or tuple(zeros.shape) != pshape):
            raise ValueError(f"group_size={self.group_size}: scales / zeros must be {list(pshape)} (got {tuple(scales.shape)}, {tuple(zeros.shape)})")
        self.register_buffer("qbits", qbits)
        self.register_buffer("scales", scales)
        self.register_buffer("zeros", zeros)
        self.register_buffer("bias", bias)
        return self

    @classmethod
    def from_codes(cls, qweight, scales, zeros, bias, bits, weight_dtype, group_size=0):
        """from one-byte codes [out, in] (what W8Linear.from_codes wraps): packed on the device by csrc/w8_linear.hip, on the CPU in torch"""
        row_bytes(qweight.shape[1], bits)
        qbits = ops.wb_pack(qweight, bits) if qweight.is_cuda else pack_codes_torch(qweight, bits)
        return cls.from_bits(qbits, qweight.shape[1], scales, zeros, bias, bits, weight_dtype, group_size)

    def codes(self):
        """the codes one per byte, uint8 [out, in]"""
        return unpack_codes_torch(self.qbits, self.bits, self.in_features)

    def dequantize(self):
        """the weight in weight_dtype.  CUDA: csrc/w8_linear.hip; CPU: a torch unpack, then W8Linear's arithmetic (fp32 subtraction, one fp32
        product, one rounding)"""
        if self.qbits.is_cuda:
            return ops.wb_dequant(self.qbits, self.bits, self.in_features, self.scales, self.zeros, self.weight_dtype, group_size=self.group_size)
        sc, zr = (expand_groups(p, self.in_features, self.group_size) for p in (self.scales, self.zeros))
        return (sc * (self.codes().float() - zr)).to(self.weight_dtype)

    def kernel_rows_ok(self):
        """the kernel takes whole 16-code chunks through 16-byte loads only: in_features % 16 == 0 and 16-byte-aligned contiguous storage (a row
        is a multiple of 16 bytes).  Other rows dequantize, as W8Linear keeps them off its kernel."""
        q = self.qbits
        return self.in_features % 16 == 0 and q.is_contiguous() and q.data_ptr() % 16 == 0

    def forward(self, x):
        x2d = self._kernel_input(x, WB_FORWARD_MAX_TOKENS)
        if x2d is not None:
            y = ops.wb_linear(x2d, self.qbits, self.bits, self.scales, self.zeros, self.bias, group_size=self.group_size,
                              weight_dtype=self.weight_dtype)
            return y.view(*x.shape[:-1], self.out_features)
        x2d = self._gemm_input(x, WB_FORWARD_MAX_TOKENS)   # opt-in (packed_linear.packed_gemm_enabled): the GEMM on the bitstream rows
        if x2d is not None:
            y = ops.packed_gemm(x2d, self.qbits, self.bits, self.scales, self.zeros, self.bias, group_size=self.group_size,
                                weight_dtype=self.weight_dtype)
            return y.view(*x.shape[:-1], self.out_features)
        return self._dense_forward(x)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, bits={self.bits}, weight_dtype={self.weight_dtype}" + (
            f", group_size={self.group_size}" if self.group_size else "")
