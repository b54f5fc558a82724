"""RTN weight quantization of the compressed model (quantization.py:147-175 of the reference) on the HIP kernel of csrc/rtn_quant.hip.

The reference's `rtn_quant_sequential(model, wbits)` walks the decoder blocks and, for every module whose type is exactly nn.Linear
(`find_layers`, which recurses into SVDLinear, so ALinear and BLinear are both quantized), replaces `weight.data` by the per-row
round-to-nearest fake quantization of the weight, in the weight's own dtype.  lm_head and the embeddings sit outside the blocks and
are left alone.  Here the weights of one block go through ONE batched launch (ops.rtn_quant_batched); the arithmetic is the
reference's bit for bit.  `rtn_pack_sequential` is the same step with the weights kept as uint8 codes (modules/w8_linear.py) or, for 6 and 4 bits, as codes of their own
width (modules/wb_linear.py).  `group_size` 64 / 128 gives both steps one scale and zero per group of that many input columns instead of per
row (csrc K14): the reference has that only inside AutoAWQ (`q_group_size: 128`), and the factor pairs of ASVD, whose columns carry the
falling sqrt(sigma), need it at 4 bits.  `mse=True` turns on the clip search of the reference's Quantizer (csrc K15; its defaults: norm 2.4,
grid 100, maxshrink 0.8), which the reference's own RTN step leaves off: every row or group keeps the shrunk range with the smallest error instead
of its min / max.  AWQ (`awq_quant_sequential`) needs the `awq` package and is not provided."""
import torch
import torch.nn as nn

from . import ops
from .modules.svd_linear import SVDLinear
from .modules.w8_linear import W8Linear
from .modules.wb_linear import WB_BITS, WBLinear
from .sweep_eval import find_decoder_blocks


def _find_linears(module, name=""):
    """(name, module) of every module of exact type nn.Linear under `module`, in the reference's find_layers order (:147-153)"""
    if type(module) is nn.Linear:
        return [(name, module)]
    res = []
    for child_name, child in module.named_children():
        res += _find_linears(child, name + "." + child_name if name != "" else child_name)
    return res


def rtn_targets(model):
    """(full name, nn.Linear) pairs rtn_quant_sequential quantizes.  The decoder blocks are found by structure
    (sweep_eval.find_decoder_blocks), not by the model name as the reference does, so families other than llama / opt work too."""
    blocks_name, blocks = find_decoder_blocks(model)
    if blocks is None:
        raise ValueError("no decoder blocks (nn.ModuleList of Linear-holding modules) found in the model")
    out = []
    for i, block in enumerate(blocks):
        out += [(f"{blocks_name}.{i}.{n}", m) for n, m in _find_linears(block)]
    return out


@torch.no_grad()
def rtn_quant_sequential(model, wbits, group_size=0, mse=False):
    """quantization.py:157-175: round-to-nearest `wbits`-bit fake quantization (per output row, asymmetric, no MSE search) of every
    nn.Linear weight in the decoder blocks, one batched launch per block.  A tensor with a row whose scale is 0 is left unchanged, as
    the reference's Quantizer.ready() check does.  The one-launch forward copies of every SVDLinear in a block are dropped
    (refresh_fused), so that they are rebuilt from the quantized factors.  Returns the number of weights replaced.
    group_size 64 / 128: every group of that many columns of a row is quantized as a row of its own (the Quantizer on the weight reshaped
    to groups; the last group of a row is shorter when in_features is no multiple); a tensor with a group of scale 0 is left unchanged.
    mse: the Quantizer's clip search (mse=True) per row or group, with the reference's defaults."""
    group_size = ops._group(group_size)
    blocks_name, blocks = find_decoder_blocks(model)
    if blocks is None:
        raise ValueError("no decoder blocks (nn.ModuleList of Linear-holding modules) found in the model")
    dev = getattr(model, "device", None)
    n_done = 0
    for block in blocks:
        if dev is not None:
            block.to(dev)  # quantization.py:165 `layers[i].to(model.device)`
        subset = _find_linears(block)
        if not subset:
            continue
        outs = ops.rtn_quant_batched([lin.weight.data for _, lin in subset], wbits, group_size=group_size, mse=bool(mse))
        for (_, lin), out in zip(subset, outs):
            if out is not lin.weight.data:
                n_done += 1
            lin.weight.data = out
        for m in block.modules():
            if isinstance(m, SVDLinear):
                m.refresh_fused()
    print(f"rtn int{wbits}{_group_tag(group_size)}{_mse_tag(mse)}: {n_done} weights quantized in {len(blocks)} blocks of {blocks_name}")
    return n_done


def _group_tag(group_size):
    return f" g{group_size}" if group_size else ""


def _mse_tag(mse):
    return " mse" if mse else ""


def _set_submodule(root, name, new):
    parent_name, _, child = name.rpartition(".")
    setattr(root.get_submodule(parent_name) if parent_name else root, child, new)


@torch.no_grad()
def rtn_pack_sequential(model, wbits, storage="bytes", group_size=0, mse=False):
    """rtn_quant_sequential with the result kept PACKED: per decoder block one batched launch that also emits the uint8 codes and the per-row
    fp32 scale / zero, and every target nn.Linear replaced by a W8Linear holding them (one byte per weight for any wbits <= 8; the bias is
    kept as it is).  The packed layer stands for exactly the fake-quantized weight: W8Linear.dequantize() is the `out` of the launch, bit
    for bit.  That is checked on the device for every tensor before it is replaced; a tensor stays an nn.Linear — fake-quantized, or
    unchanged when the kernel flags a row with scale 0, exactly as rtn_quant_sequential leaves it — when its fake-quantized weight holds a
    non-finite value or its codes do not reproduce it (one flag read-back per block).  Returns the number of weights packed.
    storage="bits" (wbits 6 or 4 only): the codes of the launch are packed to their own width (ops.wb_pack), the byte codes released and the
    layer becomes a WBLinear; the check is the same, on what ops.wb_dequant reads back from the bit-packed rows.
    group_size 64 / 128: scale / zero per group of that many columns ([out, ceil(in / group_size)] each, 8 bytes per group in the byte count);
    the modules carry the group size and the check is the same.
    mse: the scale / zero of every row or group come from the Quantizer's clip search; the modules, the check and the byte count see only other
    values."""
    if storage not in ("bytes", "bits"):
        raise ValueError(f"storage must be 'bytes' or 'bits' (got {storage!r})")
    if storage == "bits" and int(wbits) not in WB_BITS:
        raise ValueError(f"bit-packed storage holds codes of 4 or 6 bits (got wbits={wbits}); 8-bit codes are already one per byte")
    group_size = ops._group(group_size)
    blocks_name, blocks = find_decoder_blocks(model)
    if blocks is None:
        raise ValueError("no decoder blocks (nn.ModuleList of Linear-holding modules) found in the model")
    dev = getattr(model, "device", None)
    n_packed, bytes_before, bytes_after = 0, 0, 0
    for block in blocks:
        if dev is not None:
            block.to(dev)
        subset = _find_linears(block)
        if not subset:
            continue
        res = ops.rtn_quant_batched([lin.weight.data for _, lin in subset], wbits, want_params=True, group_size=group_size, mse=bool(mse))
        bad, packed = [], []
        for (_, lin), (out, q, scale, zero, flagged) in zip(subset, res):
            packed.append(ops.wb_pack(q, wbits) if storage == "bits" and not flagged else None)
            if flagged:
                bad.append(torch.ones((), dtype=torch.bool, device=q.device))
            else:
                back = (ops.wb_dequant(packed[-1], wbits, q.shape[1], scale, zero, out.dtype, group_size=group_size) if storage == "bits"
                        else ops.w8_dequant(q, scale, zero, out.dtype, group_size=group_size))
                bits_t = torch.int32 if out.dtype == torch.float32 else torch.int16
                bad.append(~torch.isfinite(out).all() | (back.view(bits_t) != out.view(bits_t)).any())
        bad = torch.stack(bad).tolist()   # the one read-back of the block
        for (name, lin), (out, q, scale, zero, flagged), qbits, keep in zip(subset, res, packed, bad):
            nbytes = lin.weight.numel() * lin.weight.element_size()
            if keep:
                lin.weight.data = out   # the input itself when flagged (ops.rtn_quant_batched)
                continue
            bias = lin.bias.data if lin.bias is not None else None
            if storage == "bits":
                new = WBLinear.from_bits(qbits, q.shape[1], scale, zero, bias, wbits, out.dtype, group_size)
            else:
                new = W8Linear.from_codes(q, scale, zero, bias, wbits, out.dtype, group_size)
            _set_submodule(block, name, new)
            n_packed += 1
            bytes_before += nbytes
            bytes_after += (qbits if storage == "bits" else q).numel() + 4 * (scale.numel() + zero.numel())
        del res, packed   # storage="bits": the byte codes go with them
        for m in block.modules():
            if isinstance(m, SVDLinear):
                m.refresh_fused()
    print(f"rtn int{wbits}{_group_tag(group_size)}{_mse_tag(mse)} {'bit-packed' if storage == 'bits' else 'packed'}: {n_packed} weights in {len(blocks)} blocks, {bytes_before} -> {bytes_after} bytes")
    return n_packed
