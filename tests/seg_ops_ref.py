"""Plain numpy restatement, in float64, of the operators in csrc/ojf_seg_ops.hip (the AdapNet++ front end around the
convolutions: modules/adapnet.py, modules/pipeline.py:42-60,181-185).  Nothing here imports the package: the host test
(test_stream_ops_host.py) shows that every function equals the torch CPU operator it restates, the GPU test
(test_seg_ops_gpu.py) holds the kernels to them.

Layout: pixel rows.  An image is [npix, C] (or [B, H, W, C] where the geometry matters); a result that the kernel stores
as fp32 is returned in float64 and rounded by the caller (for one division or one product of two fp32 values the double
rounding through float64 is innocuous: 53 >= 2 * 24 + 2)."""
import numpy as np


def pack_input(src, divisor):
    """pipeline.py:44,50: [3, H, W] planes (or one [H, W] plane replicated three times: the depth form) divided by
    ``divisor`` -> [H * W, 8] rows, channels 3..7 zero."""
    src = np.asarray(src, np.float64)
    planes = src.reshape(-1, src.shape[-2] * src.shape[-1])
    if planes.shape[0] == 1:
        planes = np.repeat(planes, 3, axis=0)
    assert planes.shape[0] == 3
    out = np.zeros((planes.shape[1], 8), np.float64)
    out[:, :3] = (planes / np.float64(divisor)).T
    return out


def maxpool3s2p1(x):
    """nn.MaxPool2d(3, stride 2, padding 1) of [B, H, W, C]: -Inf padding, a NaN in the window wins."""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = np.full((B, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf)
    pad[:, 1:H + 1, 1:W + 1] = x
    out = np.full((B, Ho, Wo, C), -np.inf)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, pad[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2])  # np.maximum propagates NaN
    return out


def channel_mean(x):
    """Global average over the pixels of [npix, C] -> [C]."""
    x = np.asarray(x, np.float64)
    return x.sum(axis=0) / np.float64(x.shape[0])


def broadcast(vec, npix, gate=None):
    """out[p, c] = vec[c] (* gate[p, c]) -> [npix, C]."""
    out = np.repeat(np.asarray(vec, np.float64)[None, :], npix, axis=0)
    return out if gate is None else out * np.asarray(gate, np.float64)


def pool_fc(x, weight, bias, act, npix_out, gate=None):
    """The squeeze chain (adapnet.py:204-210, :292-296): mean over the pixels of x [npix_in, c_in] -> weight [c_out, c_in]
    @ mean + bias -> optional ReLU -> broadcast to [npix_out, c_out] (x gate [npix_out, c_out])."""
    assert act in ('relu', 'none')
    v = np.asarray(weight, np.float64) @ channel_mean(x)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)
    if act == 'relu':
        v = np.where(v < 0, 0.0, v)
    return broadcast(v, npix_out, gate)


def softmax_max(logits):
    """torch.softmax(logits, 1).max(1) of [npix, C] -> (scores f64 [npix], ids int64 [npix]).  The id is the FIRST maximum
    of the softmax values.  A row that holds a NaN or a +Inf (inf - inf) is all-NaN after the softmax, and so is a row of
    nothing but -Inf; the maximum of an all-NaN row is its first element: (NaN, 0)."""
    l = np.asarray(logits, np.float64)
    npix, C = l.shape
    scores, ids = np.empty(npix), np.zeros(npix, np.int64)
    for p in range(npix):
        row = l[p]
        m = row.max()  # NaN if any NaN
        if np.isnan(m) or np.isinf(m):  # NaN / +Inf in the row, or only -Inf
            scores[p], ids[p] = np.nan, 0
            continue
        e = np.exp(row - m)
        sm = e / e.sum()
        ids[p] = int(np.argmax(sm))  # first maximum
        scores[p] = sm[ids[p]]
    return scores, ids
