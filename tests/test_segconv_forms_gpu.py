"""Every SEGCONV kernel form without dropout (csrc/ojf_seg.hip), one form at a time, on the tables of segconv_form_cases.py:
each row against a float64 convolution on the CPU at the bar of this kernel family (max|err| <= 3e-5 * max|ref| + 1e-6 per
member and epilogue, test_segconv_gpu.py), on fresh outputs and on caller-owned channel slices whose rows are NOT 16-byte
aligned (the per-element arms of seg_epilogue_px), and a launch trace from a child process that proves which form ran:
prediction (segconv_form_cases.predict_form / predict_multi) == launch, form and grid, for every row.

Input pixels that no tap of the layer reaches (a 1x1 convolution of stride 2 reads every other row and column) hold NaN:
entries of the last K block beyond the kernel window (their taps run to ty >= ksize) must read nothing."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import segconv_form_cases as fc
from segconv_form_cases import FORM_TABLE, DECONV_TABLE, MULTI_TABLE, PLACEMENTS, DECONV_PLACEMENTS, SENTINEL, predict_form, predict_multi
from test_segconv_dropout_gpu import make_case, reference as reference3, padded, to_nhwc_batch, EPILOGUES

pytestmark = pytest.mark.gpu

KW = {'plain': (None, False, False), 'relu': ('relu', False, False), 'res_relu': ('relu', True, False), 'sigmoid_mul': ('sigmoid', False, True),
      'res_sigmoid_mul': ('sigmoid', True, True)}  # epilogue -> (activation, residual, gate)


def reference(lin, res, gate, epilogue):
    """float64: the three epilogues of the dropout test, plus ReLU alone and residual + sigmoid + gate (all three row kinds)."""
    if epilogue == 'relu':
        return F.relu(lin)
    if epilogue == 'res_sigmoid_mul':
        return torch.sigmoid(lin + res.double()) * gate.double()
    return reference3(lin, res, gate, epilogue)


def unread_pixels(k, s, d, p, H, W, Ho, Wo):
    """bool [H, W]: input pixels no tap of any output pixel lands on."""
    hits = F.conv_transpose2d(torch.ones(1, 1, Ho, Wo), torch.ones(1, 1, k, k), stride=s, dilation=d)[0, 0]  # rows -p .. of the padded image
    hits = hits[p:p + H, p:p + W]
    full = torch.zeros(H, W)
    full[:hits.shape[0], :hits.shape[1]] = hits
    return full == 0


def device_inputs(row, xs, dev):
    """The members' inputs as NHWC rows on the device, NaN where the layer reads nothing."""
    k, s, d, p, H, W = row[3:9]
    g = fc.geometry(*row[1:10])
    dead = unread_pixels(k, s, d, p, H, W, g.Ho, g.Wo)
    out = []
    for x in xs:
        x = x.clone()
        x[:, :, dead] = float('nan')
        out.append(to_nhwc_batch(x.to(dev)))
    return out


def place(t, kind, dev, poison=False):
    """The CPU tensor [B, c, H, W] as a channel slice of a wider NHWC buffer of sentinels (segconv_form_cases.SLICE_KINDS):
    returns (buffer, slice); poison: the slice holds NaN instead of t."""
    B, c, H, W = t.shape
    lo, cb = fc.slice_geometry(kind, c)
    buf = torch.full((B, H, W, cb), SENTINEL, dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
    view = buf[:, lo:lo + c]
    if poison:
        view.fill_(float('nan'))
    else:
        view.copy_(t.to(dev))
    assert (buf.data_ptr() % 16 == 0) and ((view.data_ptr() % 16 == 0 and cb % 4 == 0) == fc.rows_aligned(kind, c))
    return buf, view


def untouched_outside(buf, view):
    """Every channel of the buffer outside the slice still holds the sentinel, bit for bit."""
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    c = view.shape[1]
    sent = torch.tensor(SENTINEL, dtype=torch.float32, device=buf.device)
    return bool((buf[:, :lo] == sent).all()) and bool((buf[:, lo + c:] == sent).all())


_worst = {}  # form -> worst err / bar so far (printed per row: the numbers of DESIGN.md 6.1.1)


def check(got, ref, what, form):
    ref = ref.numpy()
    out = got.cpu().numpy()
    assert out.shape == ref.shape, what
    assert np.isfinite(out).all(), (what, 'non-finite output')
    bar = 3e-5 * np.abs(ref).max() + 1e-6
    err = np.abs(out - ref).max()
    _worst[form] = max(_worst.get(form, 0.0), err / bar)
    print('segconv-forms %-14s %-44s err %.3e bar %.3e err/bar %.3f' % (form, '/'.join(map(str, what)), err, bar, err / bar))
    assert err <= bar, (what, err, bar)


def net_check(dev):
    from online_joint_depthfusion_and_semantic_amd import _lib
    return _lib.load().ojf_net_check(_lib.stream_ptr(dev))


def group_kwargs(epilogue, ress, gates):
    act, use_res, use_gate = KW[epilogue]
    return {'act': act, 'residuals': ress if use_res else None, 'muls': gates if use_gate else None}


@pytest.mark.parametrize('row', FORM_TABLE, ids=[r[0] for r in FORM_TABLE])
def test_form_row_matches_float64(row):
    from online_joint_depthfusion_and_semantic_amd import segconv
    from online_joint_depthfusion_and_semantic_amd.segconv import SegConv
    name, cout, n, form = row[0], row[2], row[10], row[11]
    dev = torch.device('cuda:0')
    convs, xs, ress, gates, lins = make_case(row)
    ops = [SegConv(c) for c in convs]
    xg = device_inputs(row, xs, dev)
    # (a) fresh outputs: the launch's own rows, pad channels c_out .. round_up(c_out, 8) exactly 0
    rg = [to_nhwc_batch(r.to(dev)) for r in ress]
    gg = [to_nhwc_batch(g.to(dev)) for g in gates]
    for epilogue in EPILOGUES:
        outs = segconv.group(ops, xg, **group_kwargs(epilogue, rg, gg))
        for m in range(n):
            check(outs[m], reference(lins[m], ress[m], gates[m], epilogue), (name, 'fresh', epilogue, m), form)
            if cout % 8:
                assert float(padded(outs[m])[:, cout:].abs().max()) == 0.0, (name, epilogue, m)
    # (b) caller-owned rows: output, residual and gate each a channel slice of its own wider buffer, misaligned one at a time
    for placement in PLACEMENTS:
        epilogue, ko, kr, kg = placement
        ob = [place(lins[m], ko, dev, poison=True) for m in range(n)]
        rb = [place(r, kr, dev) for r in ress] if kr else None
        gb = [place(g, kg, dev) for g in gates] if kg else None
        keep = [b.clone() for b, _ in (rb or []) + (gb or [])]
        segconv.group(ops, xg, outs=[v for _, v in ob], **group_kwargs(epilogue, rb and [v for _, v in rb], gb and [v for _, v in gb]))
        torch.cuda.synchronize()
        for m in range(n):
            what = (name, '%s-%s-%s' % (ko, kr, kg), epilogue, m)
            check(ob[m][1], reference(lins[m], ress[m], gates[m], epilogue), what, form)
            assert untouched_outside(*ob[m]), (what, 'wrote outside its channel slice')
        assert all(torch.equal(b, k) for (b, _), k in zip((rb or []) + (gb or []), keep)), (name, placement)
    print('segconv-forms-worst %s %s %.3f' % (form, name, _worst[form]))
    assert net_check(dev) == 0


def make_deconv(row, seed=0):
    name, cin, cout, _, _, _, _, h, w, B, _, form, s = row
    g = torch.Generator().manual_seed(seed + cin * 131 + cout * 7 + s)
    dc = nn.ConvTranspose2d(cin, cout, 2 * s, stride=s, padding=s // 2, bias=True)
    with torch.no_grad():
        dc.weight.copy_(torch.randn(dc.weight.shape, generator=g) / np.sqrt(cin * 4))
        dc.bias.copy_(torch.randn(cout, generator=g) * 0.5)
    x = torch.randn((B, cin, h, w), generator=g) * 2
    return dc, x


@pytest.mark.parametrize('row', DECONV_TABLE, ids=[r[0] for r in DECONV_TABLE])
def test_deconv_row_matches_float64(row):
    from online_joint_depthfusion_and_semantic_amd.segconv import SegDeconv
    name, cout, form, s = row[0], row[2], row[11], row[12]
    dev = torch.device('cuda:0')
    dc, x = make_deconv(row)
    lin = F.conv_transpose2d(x.double(), dc.weight.detach().double(), dc.bias.detach().double(), stride=s, padding=s // 2)
    op = SegDeconv(dc)
    xg = to_nhwc_batch(x.to(dev))
    for epilogue in ('plain', 'relu'):
        got = op(xg, act=KW[epilogue][0])
        check(got, reference(lin, None, None, epilogue), (name, 'fresh', epilogue), form)
        assert float(padded(got)[:, cout:].abs().max()) == 0.0, (name, epilogue)
    for epilogue, ko in DECONV_PLACEMENTS:
        buf, view = place(lin, ko, dev, poison=True)
        op(xg, out=view, act=KW[epilogue][0])
        torch.cuda.synchronize()
        check(view, reference(lin, None, None, epilogue), (name, ko, epilogue), form)
        assert untouched_outside(buf, view), (name, ko, 'wrote outside its channel slice')
    print('segconv-forms-worst %s %s %.3f' % (form, name, _worst[form]))
    assert net_check(dev) == 0


def make_multi(members, dev):
    """One member per spec: (SegConv, input rows, keyword arguments of segconv.multi) and its float64 reference."""
    from online_joint_depthfusion_and_semantic_amd.segconv import SegConv
    calls, refs = [], []
    for i, spec in enumerate(members):
        row = ('member',) + spec[:8] + (1, 1)
        convs, xs, ress, gates, lins = make_case(row, seed=1000 * (i + 1))
        act, use_res, use_gate = KW[spec[8]]
        kw = {'act': act}
        if use_res:
            kw['residual'] = to_nhwc_batch(ress[0].to(dev))
        if use_gate:
            kw['mul'] = to_nhwc_batch(gates[0].to(dev))
        calls.append((SegConv(convs[0]), device_inputs(row, xs, dev)[0], kw))
        refs.append(reference(lins[0], ress[0], gates[0], spec[8]))
    return calls, refs


@pytest.mark.parametrize('row', MULTI_TABLE, ids=[r[0] for r in MULTI_TABLE])
def test_multi_list_matches_float64(row):
    """Every member of a heterogeneous launch against ITS float64 reference (not its own single call), pad channels zero."""
    from online_joint_depthfusion_and_semantic_amd import segconv
    name, members, form = row
    dev = torch.device('cuda:0')
    calls, refs = make_multi(members, dev)
    outs = segconv.multi(calls)
    torch.cuda.synchronize()
    for m, (out, ref) in enumerate(zip(outs, refs)):
        check(out, ref, (name, members[m][8], m), form)
        if out.shape[1] % 8:
            assert float(padded(out)[:, out.shape[1]:].abs().max()) == 0.0, (name, m)
    assert net_check(dev) == 0


# ---- the launch trace -------------------------------------------------------------------------------------------------------
def run_traced():
    """Child process body: every row of the tables once (plain epilogue, fresh outputs), the five cases of
    test_segconv_gpu.test_heterogeneous_multi_launch_equals_separate_calls, its many-pixel SHAPES rows and the stem pair, each
    preceded by a marker line on stderr."""
    from online_joint_depthfusion_and_semantic_amd import segconv
    from online_joint_depthfusion_and_semantic_amd.segconv import SegConv, SegDeconv
    import test_segconv_gpu as t
    dev = torch.device('cuda:0')

    def mark(*what):
        torch.cuda.synchronize()
        sys.stderr.write('CASE %s\n' % ' '.join(map(str, what)))
        sys.stderr.flush()

    for row in FORM_TABLE:
        convs, xs, _, _, _ = make_case(row, fp64=False)
        ops = [SegConv(c) for c in convs]
        xg = [to_nhwc_batch(x.to(dev)) for x in xs]
        mark('form', row[0])
        segconv.group(ops, xg)
    for row in DECONV_TABLE:
        dc, x = make_deconv(row)
        op = SegDeconv(dc)
        xg = to_nhwc_batch(x.to(dev))
        mark('form', row[0])
        op(xg)
    for name, members, _ in MULTI_TABLE:
        calls = []
        for i, spec in enumerate(members):
            convs, xs, ress, gates, _ = make_case(('member',) + spec[:8] + (1, 1), seed=1000 * (i + 1), fp64=False)
            act, use_res, use_gate = KW[spec[8]]
            kw = {'act': act}
            if use_res:
                kw['residual'] = to_nhwc_batch(ress[0].to(dev))
            if use_gate:
                kw['mul'] = to_nhwc_batch(gates[0].to(dev))
            calls.append((SegConv(convs[0]), to_nhwc_batch(xs[0].to(dev)), kw))
        mark('multi', name)
        segconv.multi(calls)
    for i, calls in enumerate(t.heterogeneous_cases()):
        ops = [(SegConv(m), x, kw) for m, x, kw in calls]
        mark('hetero', i)
        segconv.multi(ops)
    for shape in t.SHAPES[-5:] + [(3, 64, 7, 2, 1, 3, 240, 320)]:
        members = 2 if shape[0] == 3 else 1  # the stem of both encoders
        convs, xs, _, _, _ = make_case(('shape',) + shape + (1, members), fp64=False)
        ops = [SegConv(c) for c in convs]
        xg = [to_nhwc_batch(x.to(dev)) for x in xs]
        mark('shape', 'x'.join(map(str, shape)))
        segconv.group(ops, xg)
    mark('end')


_TRACE_SCRIPT = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tests'))
import test_segconv_forms_gpu as t
t.run_traced()
print('TRACED')
'''

_LAUNCH = re.compile(r'^segconv (gemm \d+x\d+|<\d,\d,\d,\d>(?: drop)?|\w+<[\d,]+>) +n (\d+)  .* n_kb +(\d+)  grid (\d+)x(\d+)x(\d+) S (\d+)(.*)$')
_MEMBER = re.compile(r'^segconv (multi<[\d,]+>) +member (\d+)/(\d+)  .* n_kb +(\d+)  grid (\d+)x(\d+)x(\d+) S (\d+)(.*)$')


_traced = []  # the child's outcome, a failure included: it runs once per session


def traced():
    """See run_child_traced; a child that failed is not started again - the failure is raised again."""
    if not _traced:
        try:
            _traced.append(run_child_traced())
        except BaseException as e:
            _traced.append(e)
            raise
    if isinstance(_traced[0], BaseException):
        raise AssertionError('the traced child process failed earlier in this session: %r' % (_traced[0],))
    return _traced[0]


def run_child_traced():
    """The child's trace, once per session: {case: [launch, ...]}, launch = ('launch', form, n, n_kb, (X, Y, Z), S, suffix) or
    ('member', form, i, n, n_kb, (X, Y, total), S).  OJF_SEG_TRACE=1, every other OJF_SEG_* variable removed."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith('OJF_SEG_')}
    env['OJF_SEG_TRACE'] = '1'
    out = subprocess.run([sys.executable, '-c', _TRACE_SCRIPT, root], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'TRACED' in out.stdout, out.stderr[-3000:]
    cases, case = {}, None
    for line in out.stderr.splitlines():
        if line.startswith('CASE '):
            case = tuple(line.split()[1:])
            cases[case] = []
            continue
        if not line.startswith('segconv ') or case is None:
            continue
        m = _MEMBER.match(line)
        if m:
            cases[case].append(('member', m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), tuple(map(int, m.group(5, 6, 7))), int(m.group(8))))
            continue
        m = _LAUNCH.match(line)
        assert m, line  # a trace line this test cannot read
        cases[case].append(('launch', m.group(1), int(m.group(2)), int(m.group(3)), tuple(map(int, m.group(4, 5, 6))), int(m.group(7)), m.group(8)))
    assert ('end',) in cases
    return cases


def test_tables_reach_every_form():
    """Per row: exactly one launch, of the form the row names and predict_form predicts, on the predicted grid and map;
    transposed convolutions say so.  Heterogeneous lists: one multi<form> launch with a line per member, the mixed lists
    separate launches of the predicted forms.  Together the rows reach every form without dropout; nothing prints wide<2>."""
    cases = traced()
    reached = set()
    for row in FORM_TABLE + DECONV_TABLE:
        up = row[12] if len(row) > 12 else 0
        pred = predict_form(*row[1:11], deconv_stride=up)
        got = cases.get(('form', row[0]))
        assert got is not None and len(got) == 1 and got[0][0] == 'launch', (row[0], got)
        _, form, n, n_kb, grid, S, suffix = got[0]
        assert form == row[11] == pred.form, (row[0], form, pred.form)
        assert (n, n_kb, grid, S) == (row[10], pred.counts[0], pred.grid, pred.smap[0]), (row[0], got[0], pred)
        assert (' deconv' in suffix) == bool(up), (row[0], suffix)
        reached.add(form)
    assert reached == set(fc.ALL_FORMS), sorted(set(fc.ALL_FORMS) ^ reached)
    multi_reached = set()
    for name, members, form in MULTI_TABLE:
        pred = predict_multi(members)
        got = cases.get(('multi', name))
        assert got, name
        if form == 'separate':
            assert len(got) >= 2 and all(g[0] == 'launch' for g in got), (name, got)
            assert [(g[1], g[2], g[4], g[5]) for g in got] == [(p.form, p.grid[2], p.grid, p.smap[0]) for p in pred.groups], (name, got, pred.groups)
            continue
        assert all(g[0] == 'member' and g[1] == form for g in got), (name, got)
        assert [(g[2], g[3]) for g in got] == [(i, len(members)) for i in range(len(members))], (name, got)  # ONE launch: a line per member
        for g, (smap, xy) in zip(got, pred.maps):
            assert (g[5], g[6]) == (xy + (pred.total,), smap[0]), (name, g, pred)
        multi_reached.add(form)
    assert multi_reached == set(fc.MULTI_FORMS)
    for case, launches in cases.items():
        assert not any('wide' in l[1] for l in launches), case
    # the many-pixel layers of a 640x480 frame and the stem pair: GEMM-shaped forms
    shapes = [c for c in cases if c[0] == 'shape']
    assert len(shapes) == 6
    for c in shapes:
        assert len(cases[c]) == 1 and cases[c][0][1] in fc.GEMM_FORMS, (c, cases[c])


def test_heterogeneous_cases_are_one_launch_each():
    """The trace proof for test_segconv_gpu.test_heterogeneous_multi_launch_equals_separate_calls: its first four cases are one
    multi<form> launch each (a line per member), the last - a mix of a split-K and a plain member - falls back."""
    import test_segconv_gpu as t
    cases = traced()
    n_cases = len(t.HETERO_CASES)
    for i, members in enumerate(t.HETERO_CASES):
        got = cases.get(('hetero', str(i)))
        assert got, i
        if i < n_cases - 1:
            assert all(g[0] == 'member' for g in got) and len({g[1] for g in got}) == 1, (i, got)
            assert [(g[2], g[3]) for g in got] == [(m, len(members)) for m in range(len(members))], (i, got)
        else:
            assert len(got) >= 2 and all(g[0] == 'launch' for g in got), (i, got)
