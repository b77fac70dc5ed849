"""float64 numpy restatement of one fused VortexPooling tail launch (vortex_tail_kernel through ojf_vortex_tail, include/ojf.h) and the
shared, never modified cases of its tests.  Not a test; tests/test_vortex_tail_host.py and tests/test_vortex_tail_gpu.py use it.

   t_b = ReLU(W1_b v_b + b1_b), y = bf + sum_b Wf[:, b*C_OUT .. (b+1)*C_OUT) t_b;  kind 1: entry = We y + be (ReLU on channels < act_n) and
   the channel sums of y;  kind 19: ten LeakyReLU(0.01) pointwise layers and est = tanh(last layer) * scale.
Every function also returns the magnitude sum_k |w_k| m_k carried through the layers (m = |input| at the start): the scale fp32
accumulation errors are proportional to."""
import functools

import numpy as np

F32 = np.float32
C, C4, C_OUT, CS = 19, 5, 114, 20
HEAD_DIMS = (114, 95, 95, 76, 76, 57, 57, 38, 38, 19, 19, 9)
FRAMES = [(8, 8), (5, 7), (15, 32), (24, 64)]  # one full block | npix 35: lanes and whole waves past the image | 7.5 blocks | 24 blocks, banded


@functools.lru_cache(maxsize=None)
def layers():
    """The raw fp32 layers, read-only: widths scaled so that activations stay O(1) through the head."""
    rng = np.random.default_rng(11)

    def mat(co, ci, gain=1.0):
        return (rng.standard_normal((co, ci)) * gain / np.sqrt(ci)).astype(F32)

    d = dict(
        w1=np.stack([mat(C_OUT, C) for _ in range(4)]), b1=(rng.standard_normal((4, C_OUT)) * 0.1).astype(F32),
        wf=mat(C_OUT, 4 * C_OUT), bf=(rng.standard_normal(C_OUT) * 0.1).astype(F32),
        we=mat(4 * CS, C_OUT), be=(rng.standard_normal(4 * CS) * 0.1).astype(F32),
        hw=[mat(HEAD_DIMS[l + 1], HEAD_DIMS[l], 1.4) for l in range(11)],
        hb=[(rng.standard_normal(HEAD_DIMS[l + 1]) * 0.05).astype(F32) for l in range(11)])
    for v in d.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def branch_inputs(npix):
    """[4, C, npix] float32 >= 0 (the branches' 3x3 pairs end in ReLU), read-only"""
    v = np.abs(np.random.default_rng(200 + npix).standard_normal((4, C, npix))).astype(F32)
    v.setflags(write=False)
    return v


def to_planes(v):
    """[4, C, npix] -> planes [4, C4, npix, 4] (channels C .. 4*C4-1 zero)"""
    nb, c, npix = v.shape
    full = np.zeros((nb, 4 * C4, npix), F32)
    full[:, :c] = v
    return np.ascontiguousarray(full.reshape(nb, C4, 4, npix).transpose(0, 1, 3, 2))


def tail(v, L):
    """-> (y [C_OUT, npix] float64, magnitude)"""
    v64 = v.astype(np.float64)
    y, my = L['bf'].astype(np.float64)[:, None] + np.zeros((C_OUT, v.shape[2])), np.abs(L['bf']).astype(np.float64)[:, None] + np.zeros((C_OUT, v.shape[2]))
    for b in range(4):
        w1, wf = L['w1'][b].astype(np.float64), L['wf'][:, b * C_OUT:(b + 1) * C_OUT].astype(np.float64)
        t = np.maximum(w1 @ v64[b] + L['b1'][b].astype(np.float64)[:, None], 0.0)
        mt = np.abs(w1) @ np.abs(v64[b]) + np.abs(L['b1'][b]).astype(np.float64)[:, None]
        y, my = y + wf @ t, my + np.abs(wf) @ mt
    return y, my


def entry(y, my, L, act_n):
    we = L['we'].astype(np.float64)
    lin = we @ y + L['be'].astype(np.float64)[:, None]
    out = lin.copy()
    out[:act_n] = np.maximum(lin[:act_n], 0.0)
    return out, np.abs(we) @ my + np.abs(L['be']).astype(np.float64)[:, None]


def head(y, L, scale):
    x = y
    for l in range(11):
        x = L['hw'][l].astype(np.float64) @ x + L['hb'][l].astype(np.float64)[:, None]
        if l < 10:
            x = np.where(x > 0, x, 0.01 * x)
    return np.tanh(x) * scale
