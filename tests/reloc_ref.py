"""Numpy restatement of the relocalisation definition in csrc/ojf_reloc.hip (the code image, the ferns, the dissimilarity,
query and insert), written for clarity, frame by frame and fern by fern.  The GPU tests pin the kernels to it bit for bit."""
import numpy as np

NO_KEY = np.uint64(0xffffffffffffffff)


def quantise(depth, mask=None):
    """(valid bool [h,w], q u32 [h,w]): valid = mask != 0, finite, 0 < d < 64; q = rint(d * 1024) (0 where not valid)."""
    d = np.asarray(depth, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        valid = np.isfinite(d) & (d > np.float32(0)) & (d < np.float32(64))
    if mask is not None:
        valid = valid & (np.asarray(mask).view(np.uint8) != 0 if np.asarray(mask).dtype == np.bool_ else np.asarray(mask) != 0)
    q = np.zeros(d.shape, dtype=np.uint32)
    q[valid] = np.rint(d[valid] * np.float32(1024.0)).astype(np.uint32)
    return valid, q


def code_image(depth, mask, image, cell):
    """(values f32 [4,CH,CW], valid bool [CH,CW]) of one frame; image u8 [h,w,4] (R, G, B, padding) or None."""
    h, w = depth.shape
    c = int(cell)
    CH, CW = h // c, w // c
    assert CH >= 1 and CW >= 1
    valid, q = quantise(depth, mask)
    values = np.zeros((4, CH, CW), dtype=np.float32)
    ok = np.zeros((CH, CW), dtype=bool)
    for i in range(CH):
        for j in range(CW):
            win = (slice(i * c, i * c + c), slice(j * c, j * c + c))
            n = int(valid[win].sum())
            S = int(q[win][valid[win]].astype(np.uint64).sum())
            assert S < 2 ** 32
            if 2 * n >= c * c:
                ok[i, j] = True
                values[0, i, j] = (np.float32(S) / np.float32(n)) * np.float32(2.0 ** -10)
            if image is not None:
                for ch in range(3):
                    Sb = int(image[win][..., ch].astype(np.uint64).sum())
                    values[1 + ch, i, j] = np.float32(Sb) / np.float32(c * c)
    return values, ok


def fern_bits(values, ok, table):
    """u8 [M] four-bit codes of the ferns of ``table`` ({'cell', 'channel', 'threshold'} [M,4]) on a code image."""
    cells = ok.size
    v = values.reshape(4, cells)
    okf = ok.reshape(cells)
    M = table['cell'].shape[0]
    out = np.zeros(M, dtype=np.uint8)
    for m in range(M):
        for j in range(4):
            ci, ch, thr = int(table['cell'][m, j]), int(table['channel'][m, j]) & 3, np.float32(table['threshold'][m, j])
            bit = False
            if 0 <= ci < cells:
                bit = bool(v[ch, ci] > thr) and (ch != 0 or bool(okf[ci]))
            out[m] |= int(bit) << j
    return out


def pack(nibbles):
    """u32 [M/8]: fern m in word m / 8 at bits 4 * (m % 8)."""
    nib = np.asarray(nibbles, dtype=np.uint32).reshape(-1, 8)
    return (nib << (4 * np.arange(8, dtype=np.uint32))).sum(axis=1).astype(np.uint32)


def unpack(words):
    w = np.asarray(words, dtype=np.uint32).reshape(-1, 1)
    return ((w >> (4 * np.arange(8, dtype=np.uint32))) & np.uint32(15)).astype(np.uint8).reshape(-1)


def encode(depth, mask, image, cell, table):
    """(codes u32 [M/8], code image f32 [4,CH,CW]) of one frame."""
    values, ok = code_image(depth, mask, image, cell)
    return pack(fern_bits(values, ok, table)), values


def differ(a, b):
    """The number of ferns whose nibbles differ, fern by fern."""
    return int((unpack(a) != unpack(b)).sum())


def differ_packed(a, b):
    """The same by the kernel's word arithmetic: popcount((x | x>>1 | x>>2 | x>>3) & 0x11111111) of x = a ^ b.  ``b`` may
    be [K, M/8]: one count per row."""
    x = np.asarray(a, dtype=np.uint32) ^ np.asarray(b, dtype=np.uint32)
    y = (x | (x >> np.uint32(1)) | (x >> np.uint32(2)) | (x >> np.uint32(3))) & np.uint32(0x11111111)
    bits = np.unpackbits(np.ascontiguousarray(y).view(np.uint8).reshape(y.shape + (4,)), axis=-1)
    return bits.reshape(y.shape[:-1] + (-1,)).sum(axis=-1).astype(np.int64)


def keys(code, db_codes, count):
    """u64 [count]: differ << 32 | index against the first ``count`` keyframes."""
    if count == 0:
        return np.zeros(0, dtype=np.uint64)
    d = differ_packed(code, np.asarray(db_codes)[:count]).astype(np.uint64)
    return (d << np.uint64(32)) | np.arange(count, dtype=np.uint64)


def query(code, db_codes, count, k):
    """u64 [k]: the k smallest keys ascending, all-ones where there are fewer."""
    out = np.full(k, NO_KEY, dtype=np.uint64)
    ks = np.sort(keys(code, db_codes, count))[:k]
    out[:len(ks)] = ks
    return out


class Store:
    """codes u32 [capacity, M/8], poses f64 [capacity, 12], count."""

    def __init__(self, capacity, words):
        self.codes = np.zeros((capacity, words), dtype=np.uint32)
        self.poses = np.zeros((capacity, 12), dtype=np.float64)
        self.count = 0
        self.capacity = capacity

    def insert(self, codes, poses, min_differ, force=False):
        """(best u64 [n], flags i32 [n]) of n frames offered in order."""
        n = len(codes)
        best, flags = np.full(n, NO_KEY, dtype=np.uint64), np.zeros(n, dtype=np.int32)
        for f in range(n):
            ks = keys(codes[f], self.codes, self.count)
            if len(ks):
                best[f] = ks.min()
            wanted = force or self.count == 0 or int(best[f] >> np.uint64(32)) > min_differ
            if not wanted:
                flags[f] = 0
            elif self.count == self.capacity:
                flags[f] = 2
            else:
                flags[f] = 1
                self.codes[self.count] = codes[f]
                self.poses[self.count] = np.asarray(poses[f], dtype=np.float64).reshape(-1)[:12]
                self.count += 1
        return best, flags


def pack_image(image):
    """u8 [h,w,4] of a float [3,h,w] image on the 0..255 scale (color.pack_image: clamp, round half to even, u8, padding 0) or
    of u8 [h,w,3|4]."""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        out = np.zeros(image.shape[:2] + (4,), dtype=np.uint8)
        out[..., :image.shape[2]] = image
        return out
    px = np.rint(np.clip(image.astype(np.float32), 0.0, 255.0)).astype(np.uint8).transpose(1, 2, 0)
    out = np.zeros(px.shape[:2] + (4,), dtype=np.uint8)
    out[..., :3] = px
    return out
