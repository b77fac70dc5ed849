"""CPU: the ABI row of ojf_vortex_tail, the refusals it makes before any HIP call, the plan rows of the two fused tails, and the float64
restatement's own layout helpers (tests/vortex_tail_ref.py)."""
import ctypes
import os
import re

import numpy as np

from online_joint_depthfusion_and_semantic_amd import _lib
import vortex_tail_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_params(name):
    text = open(os.path.join(ROOT, 'include', 'ojf.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, text)
    assert m, name
    return [' '.join(p.split()) for p in m.group(1).split(',')]


def test_abi_row_matches_the_header():
    res, args = _lib.SIGNATURES['ojf_vortex_tail']
    params = header_params('ojf_vortex_tail')
    assert res is _lib._i and len(args) == len(params) == 23
    for ctype, decl in zip(args, params):
        want = _lib._vp if ('*' in decl or decl.startswith('ojf_stream_t')) else (_lib._f if decl.startswith('float ') else _lib._i)
        assert ctype is want, decl
    names = [d.split()[-1].lstrip('*') for d in params]
    assert names == ['kind', 'w1_host', 'b1_host', 'wf_host', 'bf_host', 'c', 'c_out', 'next_w_host', 'next_b_host', 'next_dims_host',
                     'v_dev', 'c4', 'npix', 'out_dev', 'og_store', 'split_groups', 'act_n', 'colsums_dev', 'rows_stride', 'rows_n',
                     'scale', 'form', 'stream']


def test_refusals_before_any_device_call():
    lib = _lib.load()
    host = np.zeros(64, np.float32)  # stands in for addresses nothing reads
    dev = host.ctypes.data
    cs = np.array([20], np.int32)
    head = np.array(ref.HEAD_DIMS, np.int32)

    def call(kind=1, w1=dev, b1=dev, wf=dev, bf=dev, c=19, c_out=114, nw=dev, nb=dev, dims=cs.ctypes.data, v=dev, c4=5, npix=9, out=dev,
             og_store=20, split_groups=5, act_n=20, colsums=dev, rows_stride=9, rows_n=9, form=1):
        return lib.ojf_vortex_tail(kind, w1, b1, wf, bf, c, c_out, nw, nb, dims, v, c4, npix, out, og_store, split_groups, act_n, colsums,
                                   rows_stride, rows_n, 1.0, form, None)

    for bad in (dict(w1=None), dict(b1=None), dict(wf=None), dict(bf=None), dict(nw=None), dict(nb=None), dict(dims=None), dict(v=None),
                dict(out=None), dict(colsums=None)):
        assert call(**bad) != 0 and lib.ojf_last_error().startswith(b'ojf_vortex_tail:') and b'null' in lib.ojf_last_error(), bad
    for bad in (dict(kind=0), dict(kind=20), dict(c=0), dict(c=33), dict(c_out=112), dict(c_out=129), dict(c4=0), dict(c4=9), dict(c4=4),
                dict(npix=0), dict(form=2), dict(form=-1), dict(og_store=21), dict(split_groups=21), dict(split_groups=-1), dict(act_n=-1)):
        assert call(**bad) != 0 and lib.ojf_last_error().startswith(b'ojf_vortex_tail:'), bad
    wrong = head.copy()
    wrong[3] = 81  # six tiles where the chain has five
    short = head.copy()
    short[0] = 113
    for bad in (dict(dims=wrong.ctypes.data), dict(dims=short.ctypes.data), dict(rows_n=0), dict(rows_n=10), dict(rows_stride=8)):
        assert call(kind=19, **dict(dict(dims=head.ctypes.data), **bad)) != 0 and lib.ojf_last_error().startswith(b'ojf_vortex_tail:'), bad


def test_plan_rows_of_the_two_fused_tails():
    """The headline net runs one tail with the next entry GEMM and one with the prediction head - the two forms ojf_vortex_tail launches."""
    buf = ctypes.create_string_buffer(8192)
    n = _lib.load().ojf_net_plan(3, 9, 5, 0, 240, 320, _lib.ARITH_F16X3, buf, 8192)
    assert n > 0
    names = buf.value.split(b'\n')[:-1]  # one name per line
    assert len(names) == n
    assert names.count(b'vortex_tail_kernel (+ next entry GEMM)') == 1 and names.count(b'vortex_tail_kernel (+ prediction head)') == 1
    assert names.index(b'vortex_tail_kernel (+ next entry GEMM)') < names.index(b'vortex_tail_kernel (+ prediction head)')


def test_reference_planes_layout():
    v = ref.branch_inputs(35)
    p = ref.to_planes(v)
    assert p.shape == (4, ref.C4, 35, 4)
    assert p[2, 4, 17, 2] == v[2, 18, 17] and p[3, 4, 0, 3] == 0.0  # channel 18 = group 4, slot 2; channel 19 is padding
    assert [h * w for h, w in ref.FRAMES] == [64, 35, 480, 1536]
