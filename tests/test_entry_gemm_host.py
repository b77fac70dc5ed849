"""CPU: the strip walk of the persistent entry GEMM (entry1x1_persistent_kernel, restated in tests/entry_gemm_ref.py) hands every strip
to exactly one block, in both of its cases; the grid rule; the ABI row of ojf_entry_gemm and the refusals it makes before any HIP call."""
import os
import re

import numpy as np

from online_joint_depthfusion_and_semantic_amd import _lib
import entry_gemm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_strip_is_walked_exactly_once():
    banded = plain = 0
    for strips in range(1, 81):
        for grid in range(1, 41):
            taken = [s for b in range(grid) for s in ref.walk(b, grid, strips)]
            assert sorted(taken) == list(range(strips)), (strips, grid)
            if strips % 8 == 0 and grid % 8 == 0:
                banded += 1
                per = strips // 8
                for b in range(grid):  # a block never leaves its XCD's band, the eighth the one-strip grid gives that XCD
                    assert all(s // per == b % 8 for s in ref.walk(b, grid, strips)), (strips, grid, b)
            else:
                plain += 1
    assert banded == 10 * 5 and plain == 80 * 40 - 50


def test_walk_is_ascending_and_ends_for_good():
    for strips, grid in [(24, 16), (24, 8), (24, 5), (31, 8), (31, 1), (1200, 768), (4800, 768), (7, 8)]:
        for b in range(grid):
            w = ref.walk(b, grid, strips)
            assert w == sorted(w) and len(set(w)) == len(w)
            assert all(ref.walk_strip(b, grid, strips, k) == -1 for k in range(len(w), len(w) + 3))
        if grid <= strips:
            assert all(ref.walk(b, grid, strips) for b in range(grid))  # no idle block under the product rule


def test_one_strip_per_block_is_the_one_strip_kernels_banding():
    """With as many blocks as strips the walk is the one-strip kernel's block -> strip map (banded_block_x)."""
    for strips in (8, 24, 1200, 31, 9):
        for b in range(strips):
            want = (b & 7) * (strips >> 3) + (b >> 3) if strips % 8 == 0 else b
            assert ref.walk(b, strips, strips) == [want]


def test_grid_rule():
    assert ref.product_grid(1200, 256) == 768 and ref.product_grid(4800, 256) == 768  # the headline frame, 640x480
    assert ref.product_grid(75, 256) == 75                                              # small frames: one strip per block
    assert ref.product_grid(24, 256, max_blocks=5) == 5 and ref.product_grid(8, 256, max_blocks=24) == 8
    lens = sorted(len(ref.walk(b, 768, 1200)) for b in range(768))
    assert lens[0] == 1 and lens[-1] == 2 and sum(lens) == 1200


def header_params(name):
    text = open(os.path.join(ROOT, 'include', 'ojf.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, text)
    assert m, name
    return [' '.join(p.split()) for p in m.group(1).split(',')]


def test_abi_row_matches_the_header():
    res, args = _lib.SIGNATURES['ojf_entry_gemm']
    params = header_params('ojf_entry_gemm')
    assert res is _lib._i and len(args) == len(params) == 16
    for ctype, decl in zip(args, params):
        want = _lib._vp if ('*' in decl or decl.startswith('ojf_stream_t')) else _lib._i
        assert decl.startswith('int ') or want is _lib._vp, decl
        assert ctype is want, decl
    names = [d.split()[-1].lstrip('*') for d in params]
    assert names == ['weight_host', 'bias_host', 'c_in_phys', 'cs', 'in_dev', 'in_split', 'c4_in', 'npix', 'out_dev', 'og_store',
                     'split_groups', 'act_n', 'colsums_dev', 'form', 'max_blocks', 'stream']


def test_refusals_before_any_device_call():
    lib = _lib.load()
    w, b = np.zeros((80, 120), np.float32), np.zeros(80, np.float32)
    host = np.zeros(64, np.float32)  # stands in for device addresses nothing reads
    dev = host.ctypes.data

    def call(weight=w.ctypes.data, bias=b.ctypes.data, c_in_phys=120, cs=20, inp=dev, c4_in=30, npix=9, out=dev, og_store=20,
             split_groups=5, act_n=20, colsums=dev, form=1, max_blocks=0):
        return lib.ojf_entry_gemm(weight, bias, c_in_phys, cs, inp, 0, c4_in, npix, out, og_store, split_groups, act_n, colsums, form,
                                  max_blocks, None)

    for bad in (dict(weight=None), dict(bias=None), dict(inp=None), dict(out=None), dict(colsums=None)):
        assert call(**bad) != 0 and lib.ojf_last_error().startswith(b'ojf_entry_gemm:') and b'null' in lib.ojf_last_error(), bad
    for bad in (dict(c_in_phys=132), dict(c_in_phys=118), dict(cs=24), dict(cs=18), dict(c4_in=31), dict(c4_in=0), dict(npix=0),
                dict(og_store=21), dict(split_groups=21), dict(split_groups=-1), dict(act_n=-1), dict(form=2), dict(max_blocks=-1)):
        assert call(**bad) != 0 and lib.ojf_last_error().startswith(b'ojf_entry_gemm:'), bad
