"""numpy side of the operator tests of the 16-bit upsamplers (vits_op_upsample16: tests/test_gpu_upsample_ops.py, tests/test_upsample_op_host.py): the operand
rounding of the two 16-bit types, the float64 reference of ConvTranspose1d with kernel = 2 x stride written from its formula, the exact reference of the 16-bit
copy, and the sequential fp32 chain on the same operands (tests/split_ref.py chain32) that the printed ratio is taken against.

Per utterance of L input positions, s = stride, k = 2 s, with x[-1] = x[L] = 0:
    n in [0, s L + k - s - 2 crop):  q = (n + crop) // s,  ph = (n + crop) % s
    y[co, n] = bias[co] + sum_ci x[ci, q] w[ci, co, ph] + x[ci, q - 1] w[ci, co, ph + s]
Everything here works on ONE utterance [c_in, L]; the un-cropped result has s (L + 1) samples m = s q + ph, and crop removes `crop` of them at each end."""
import numpy as np

import split_ref as R

BF16, F16 = 1, 2  # pkg.ARITH_*


def round16(v, arith):
    """fp32 -> the nearest value of the arithmetic's 16-bit type (ties to even), as fp32"""
    v = np.ascontiguousarray(v, np.float32)
    return v.astype(np.float16).astype(np.float32) if arith == F16 else R.bf16_rne(v)


def bits16(v, arith):
    """the bit patterns of round16(v), uint16"""
    v = np.ascontiguousarray(v, np.float32)
    if arith == F16:
        return v.astype(np.float16).view(np.uint16)
    return (R.bf16_rne(v).view(np.uint32) >> 16).astype(np.uint16)


def operands(x, w, pre_slope, arith):
    """what the matrix cores multiply: round16(leaky_relu(x, pre_slope)) and round16(w)"""
    return round16(R.lrelu32(x, pre_slope), arith), round16(w, arith)


def out_len(L, stride, crop):
    return stride * L + stride - 2 * crop  # k - stride = stride


def crop_cols(full, crop):
    """[rows, s (L + 1)] un-cropped -> [rows, s L + s - 2 crop]"""
    return full[:, crop: full.shape[1] - crop]


def upsample64(xr, wr, bias, stride):
    """float64, un-cropped: xr [c_in, L], wr [c_in, c_out, 2 s] (already rounded operands), bias [c_out] or None -> [c_out, s (L + 1)]"""
    cin, L = xr.shape
    cout, s = wr.shape[1], stride
    xp = np.zeros((cin, L + 2), np.float64)  # column q + 1 = x[q]: x[-1] and x[L] are zero
    xp[:, 1:L + 1] = xr
    w64 = wr.astype(np.float64)
    a = xp[:, 1:L + 2].T @ w64[:, :, :s].reshape(cin, cout * s) + xp[:, 0:L + 1].T @ w64[:, :, s:].reshape(cin, cout * s)  # [q, co * s + ph]
    full = a.reshape(L + 1, cout, s).transpose(1, 0, 2).reshape(cout, (L + 1) * s)
    if bias is not None:
        full = full + np.asarray(bias, np.float64)[:, None]
    return full


def chain_channels(cout, ncols):
    """the fixed subset of output channels the chain is computed on (split_ref.chain_rows)"""
    return R.chain_rows(cout, ncols)


def upsample_chain32(xr, wr, bias, stride, channels):
    """the sequential fp32 chain over the 2 c_in products (c_in-major, tap 0 then tap 1) of the given output channels, then + bias in fp32: fp32 [len(channels), s (L + 1)]"""
    cin, L = xr.shape
    s = stride
    xp = np.zeros((cin, L + 2), np.float32)
    xp[:, 1:L + 1] = xr
    A = np.empty((2 * cin, L + 1), np.float32)
    A[0::2] = xp[:, 1:L + 2]
    A[1::2] = xp[:, 0:L + 1]
    ws = wr[:, channels, :]  # [c_in, m, 2 s]
    W = np.empty((len(channels) * s, 2 * cin), np.float32)  # row = channel * s + phase
    W[:, 0::2] = ws[:, :, :s].transpose(1, 2, 0).reshape(-1, cin)
    W[:, 1::2] = ws[:, :, s:].transpose(1, 2, 0).reshape(-1, cin)
    acc = R.chain32(W, A).reshape(len(channels), s, L + 1).transpose(0, 2, 1).reshape(len(channels), (L + 1) * s)
    if bias is not None:
        acc = (acc + np.asarray(bias, np.float32)[channels][:, None]).astype(np.float32)
    return acc


def y16_bits(v, slope, arith):
    """the 16-bit copy of an fp32 array: the type's RNE of leaky_relu(v, slope), as bit patterns"""
    return bits16(R.lrelu32(v, slope), arith)
