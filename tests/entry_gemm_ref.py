"""float64 numpy restatement of the stand-alone branch-entry GEMM of a VortexPooling (entry1x1_kernel in both forms, ojf_entry_gemm in
include/ojf.h) and of the persistent form's strip walk.  Not a test; tests/test_entry_gemm_host.py and tests/test_entry_gemm_gpu.py use it.

Planes are arrays [group, npix, 4] of float32 (the kernel's [group][npix] float4): channel c of pixel p is planes[c // 4, p, c % 4].
Split planes hold, per float4, the fp16 halves {h0 h1 h2 h3 | l0 l1 l2 l3} of four values; the value they mean is h + l."""
import numpy as np

F32 = np.float32
SHARDS, COL_MAX = 16, 256
COL_SCALE = 1048576.0
STRIP = 64  # pixels of a strip: four waves of 16


def strips_of(npix):
    return (npix + STRIP - 1) // STRIP


def product_grid(strips, cus, blocks_per_cu=3, max_blocks=0):
    """Blocks of the persistent launch: what the device holds at once, at most one per strip (and at most max_blocks, tests only)."""
    grid = min(strips, blocks_per_cu * cus) if cus > 0 else strips
    return min(grid, max_blocks) if max_blocks > 0 else grid


def walk_strip(b, grid, strips, k):
    """Strip k of block b's walk, -1 past its end (csrc/ojf_net.hip entry_walk_strip).  strips and grid both multiples of 8: the block
    stays inside band b & 7 - one eighth of the strips - and walks (b >> 3) + k * grid / 8 within it; otherwise b + k * grid."""
    if (strips | grid) & 7 == 0:
        per, j = strips >> 3, (b >> 3) + k * (grid >> 3)
        return (b & 7) * per + j if j < per else -1
    s = b + k * grid
    return s if s < strips else -1


def walk(b, grid, strips):
    out, k = [], 0
    while walk_strip(b, grid, strips, k) >= 0:
        out.append(walk_strip(b, grid, strips, k))
        k += 1
    return out


def to_planes(x):
    """[channels (a multiple of 4), npix] -> planes [channels / 4, npix, 4]"""
    c, npix = x.shape
    return np.ascontiguousarray(x.reshape(c // 4, 4, npix).transpose(0, 2, 1))


def from_planes(p):
    g, npix, _ = p.shape
    return np.ascontiguousarray(p.transpose(0, 2, 1).reshape(g * 4, npix))


def split_planes(p):
    """fp32 planes -> split planes (as float32 bit patterns): h = fp16(x), l = fp16(x - h)"""
    with np.errstate(over='ignore', invalid='ignore'):
        hi = p.astype(np.float16)
        lo = (p - hi.astype(F32)).astype(np.float16)
    return np.ascontiguousarray(np.concatenate([hi, lo], axis=-1)).view(F32)


def unsplit_planes(s):
    """split planes -> the fp32 values they mean (h + l, exact in fp32)"""
    h = np.ascontiguousarray(s).view(np.float16).reshape(s.shape[:-1] + (8,))
    with np.errstate(invalid='ignore'):
        return h[..., :4].astype(F32) + h[..., 4:].astype(F32)


def gemm(weight, bias, x, act_n):
    """weight [c_out, c_in], bias [c_out], x [c_in, npix] (the values the kernel reads) -> (out [c_out, npix] float64 with ReLU on channels
    < act_n, mag [c_out, npix] = sum_k |w_k x_k|, the scale of the rounding error)"""
    w64, x64 = weight.astype(np.float64), x.astype(np.float64)
    lin = w64 @ x64 + bias.astype(np.float64)[:, None]
    out = lin.copy()
    out[:act_n] = np.maximum(lin[:act_n], 0.0)
    return out, np.abs(w64) @ np.abs(x64)


def column_sums(x):
    """-> (sum over the pixels [c_in] float64, sum of magnitudes)"""
    x64 = x.astype(np.float64)
    return x64.sum(axis=1), np.abs(x64).sum(axis=1)
