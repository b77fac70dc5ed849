"""Plain numpy restatement of the SEGCONV inference dropout (include/ojf.h, ojf_segconv_set_dropout): the always-on
``F.dropout(y, p=0.5, training=True)`` of a multi-scale unit (adapnet.py BottleneckSSMA.forward) as the kernel epilogue
draws it.

Element (pixel p, channel c) of a layer with c_out channels, stream id s, state {seed, frame}:
  counter = {p * ceil(c_out / 4) + c // 4, s, frame & 0xffffffff, frame >> 32}, key = {seed & 0xffffffff, seed >> 32};
  kept iff bit 0 of word c % 4 of Philox-4x32-10(counter, key) is set.  A kept value is v + v, a dropped one +0.0.
p runs batch-major, row-major over the output: (b * Ho + y) * Wo + x."""
import numpy as np

M32 = np.uint64(0xffffffff)
_MUL = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
_BUMP = (np.uint64(0x9E3779B9), np.uint64(0xBB67AE85))


def _u64(v):
    return np.asarray(v, dtype=np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 (Salmon et al. 2011, Random123) on arrays of 32-bit values held in uint64: 10 rounds, the key
    bumped after each.  Returns the four output words (uint64 arrays, broadcast over the inputs)."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(v) for v in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0, p1 = _MUL[0] * c0, _MUL[1] * c2  # < 2^64: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + _BUMP[0]) & M32, (k1 + _BUMP[1]) & M32
    return c0, c1, c2, c3


def counters(n_pix, c_out):
    """Word 0 of the counter of every (pixel, 4-channel group): [n_pix, ceil(c_out / 4)] (mod 2^32)."""
    g = (c_out + 3) // 4
    return (np.arange(n_pix, dtype=np.uint64)[:, None] * np.uint64(g) + np.arange(g, dtype=np.uint64)[None, :]) & M32


def keep_mask(seed, frame, stream_id, n_pix, c_out):
    """bool [n_pix, c_out]: the elements the layer keeps (and doubles).  seed / frame: Python ints, taken mod 2^64 (a
    negative int64 state word is the same 64 bits)."""
    seed, frame = int(seed) & (2 ** 64 - 1), int(frame) & (2 ** 64 - 1)
    words = philox4x32_10(counters(n_pix, c_out), int(stream_id) & 0xffffffff, frame & 0xffffffff, frame >> 32,
                          seed & 0xffffffff, seed >> 32)
    bits = np.stack(words, axis=-1) & np.uint64(1)  # [n_pix, groups, 4]: word c % 4 of group c // 4
    return bits.reshape(n_pix, -1)[:, :c_out].astype(bool)


def keep_mask_nchw(seed, frame, stream_id, batch, c_out, h, w):
    """keep_mask laid out as a [batch, c_out, h, w] array (the module's NCHW output)."""
    return keep_mask(seed, frame, stream_id, batch * h * w, c_out).reshape(batch, h, w, c_out).transpose(0, 3, 1, 2)


def apply(v, keep):
    """The epilogue's dropout on values v (any float array) with a mask of the same shape."""
    return np.where(keep, v + v, np.zeros_like(v))
