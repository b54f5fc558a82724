"""numpy restatement of the "bitstream64" storage of RTN codes at 6 and 4 bits, written from the format's definition (include/asvd_hip.h, K13)
and not from the module: a row of K codes is a little-endian bitstream, code k in bits [bits k, bits (k + 1)) of the row read as one
little-endian integer, zero-padded to whole blocks of 64 codes.  Test code only: the product path is csrc/w8_linear.hip."""
import numpy as np


def row_bytes(K, bits):
    return -(-K // 64) * 8 * bits


def pack(q, bits):
    """uint8 codes [rows, K] -> uint8 [rows, row_bytes(K, bits)]"""
    q = np.asarray(q, dtype=np.uint8)
    rows, K = q.shape
    pad = np.zeros((rows, -(-K // 64) * 64), dtype=np.uint8)
    pad[:, :K] = q
    bit = np.unpackbits(pad[..., None], axis=-1, bitorder="little")[..., :bits]          # [rows, codes, bits], least significant first
    return np.packbits(bit.reshape(rows, -1), axis=-1, bitorder="little")


def unpack(packed, bits, K):
    """uint8 [rows, row_bytes(K, bits)] -> uint8 codes [rows, K]; the padding codes are returned apart, for the check that they are zero"""
    packed = np.asarray(packed, dtype=np.uint8)
    rows = packed.shape[0]
    assert packed.shape[1] == row_bytes(K, bits), (packed.shape, K, bits)
    bit = np.unpackbits(packed, axis=-1, bitorder="little").reshape(rows, -1, bits)
    codes = (bit.astype(np.uint16) << np.arange(bits, dtype=np.uint16)).sum(axis=-1).astype(np.uint8)
    return codes[:, :K], codes[:, K:]


def word_reading(packed, bits, k):
    """code k of every row read the way a kernel does: out of the 32-bit little-endian words of the row, across a word boundary where it
    straddles one"""
    words = np.ascontiguousarray(packed).view("<u4").astype(np.uint64)
    lo, sh = (bits * k) // 32, (bits * k) % 32
    v = words[:, lo] >> np.uint64(sh)
    if sh + bits > 32:
        v = v | (words[:, lo + 1] << np.uint64(32 - sh))
    return (v & np.uint64((1 << bits) - 1)).astype(np.uint8)
