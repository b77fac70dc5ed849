"""SEGCONV inference dropout (ojf_segconv_set_dropout, the always-on dropout of AdapNet++'s multi-scale units) one layer
at a time: the dropped set against the numpy restatement (dropout_ref.py), the kept values against twice an fp64
convolution, and against the same layer without dropout bit for bit where both run in the same kernel form.  TABLE
reaches every DROP instantiation the default dispatcher launches; test_table_reaches_every_drop_form proves it from the
launch trace of a child process (OJF_SEG_TRACE is read once per process)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dropout_ref import keep_mask_nchw

pytestmark = pytest.mark.gpu

# (name, c_in, c_out, k, stride, dilation, padding, H, W, batch, members, kernel form of the dropout launch,
#  the launch without dropout takes the same kernel: bit-exact comparison)
TABLE = [
    ('gemm64_aligned_layer4', 512, 2048, 1, 1, 1, 0, 15, 20, 1, 2, 'gemm 64x64', True),
    ('gemm64_unaligned', 40, 30, 3, 1, 1, 1, 30, 40, 4, 2, 'gemm 64x64', True),
    ('gemm128_aligned', 128, 2048, 1, 1, 1, 0, 15, 20, 3, 2, 'gemm 128x128', True),
    ('gemm128_unaligned', 40, 2048, 3, 1, 1, 1, 15, 20, 3, 2, 'gemm 128x128', True),
    ('gemm128x160_aligned', 512, 2048, 1, 1, 1, 0, 15, 20, 4, 2, 'gemm 128x160', True),
    ('gemm128x160_unaligned', 40, 128, 3, 1, 1, 1, 60, 80, 4, 2, 'gemm 128x160', True),
    ('gemm128x80_aligned', 256, 128, 3, 1, 1, 1, 30, 40, 8, 2, 'gemm 128x80', True),
    ('gemm128x80_unaligned', 232, 128, 3, 1, 1, 1, 30, 40, 8, 2, 'gemm 128x80', True),
    ('drop_mw4_layer2', 64, 512, 1, 1, 1, 0, 30, 40, 1, 2, '<4,1,1,4> drop', False),
    ('drop_mw2', 64, 512, 1, 1, 1, 0, 8, 12, 1, 2, '<2,1,1,4> drop', False),
    ('drop_mw1', 64, 512, 1, 1, 1, 0, 4, 6, 1, 1, '<1,1,1,4> drop', False),
    ('drop_c30', 64, 30, 3, 1, 1, 1, 7, 9, 1, 1, '<1,1,1,4> drop', True),
    ('drop_c6', 64, 6, 1, 1, 1, 0, 7, 9, 1, 1, '<1,1,1,4> drop', False),
    ('drop_c2', 64, 2, 1, 1, 1, 0, 7, 9, 1, 1, '<1,1,1,4> drop', False),
    ('drop_c5_batch3_pair', 64, 5, 3, 1, 1, 1, 7, 9, 3, 2, '<1,1,1,4> drop', True),
]
DROP_FORMS = ('gemm 64x64', 'gemm 128x128', 'gemm 128x160', 'gemm 128x80', '<4,1,1,4> drop', '<2,1,1,4> drop', '<1,1,1,4> drop')

# {seed, frame} states: both 32-bit halves non-zero; the second seed has bit 63 set (a negative int64)
STATES = [(0x0123456789abcdef, (5 << 32) | 0x9e3779b9), (-0x1234567890abcdef, (0x7ffffffe << 32) | 3)]


def to_nhwc_batch(x, pad_to=8):
    from online_joint_depthfusion_and_semantic_amd.segconv import nhwc
    b, c = x.shape[:2]
    buf = nhwc((c + pad_to - 1) // pad_to * pad_to, x.shape[2], x.shape[3], x.device, batch=b)
    buf[:, :c] = x
    return buf[:, :c]


def make_case(row, seed=0, fp64=True):
    """The row's layers (one nn.Conv2d with bias per member, CPU) and their inputs: x, residual and gate per member (CPU
    fp32), plus the fp64 linear part of every member (None without ``fp64``)."""
    _, cin, cout, k, s, d, p, h, w, B, n = row[:11]
    g = torch.Generator().manual_seed(seed + cin * 131 + cout * 7 + B)
    convs, xs, ress, gates, lins = [], [], [], [], []
    for _ in range(n):
        conv = nn.Conv2d(cin, cout, k, stride=s, dilation=d, padding=p, bias=True)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / np.sqrt(cin * k * k))
            conv.bias.copy_(torch.randn(cout, generator=g) * 0.5)
        x = torch.randn((B, cin, h, w), generator=g) * 2
        span = d * (k - 1) + 1
        shape = (B, cout, (h + 2 * p - span) // s + 1, (w + 2 * p - span) // s + 1)
        lin = F.conv2d(x.double(), conv.weight.detach().double(), conv.bias.detach().double(), stride=s, padding=p, dilation=d) if fp64 else None
        convs.append(conv); xs.append(x); lins.append(lin)
        ress.append(torch.randn(shape, generator=g))
        gates.append(torch.rand(shape, generator=g) + 0.25)  # never 0: a kept product is non-zero
    return convs, xs, ress, gates, lins


EPILOGUES = ('plain', 'res_relu', 'sigmoid_mul')


def reference(lin, res, gate, epilogue):
    if epilogue == 'plain':
        return lin
    if epilogue == 'res_relu':
        return F.relu(lin + res.double())
    return torch.sigmoid(lin) * gate.double()


def launch(ops, xs, ress, gates, epilogue):
    """One grouped launch of the members (``segconv.group``) with the given epilogue: fresh outputs."""
    from online_joint_depthfusion_and_semantic_amd import segconv
    kw = {'plain': {}, 'res_relu': {'act': 'relu', 'residuals': ress}, 'sigmoid_mul': {'act': 'sigmoid', 'muls': gates}}[epilogue]
    return segconv.group(ops, xs, **kw)


def padded(t):
    """The whole NHWC rows of an output the launch allocated: [B, round_up(c, 8), H, W]."""
    B, c, H, W = t.shape
    return t.as_strided((B, (c + 7) // 8 * 8, H, W), t.stride())


def check_member(got, lin, res, gate, epilogue, keep, what):
    """got: the dropout launch's output of one member (cuda); keep: bool NCHW mask of the restatement."""
    ref = reference(lin, res, gate, epilogue).numpy()
    out = got.cpu().numpy()
    bar = 3e-5 * np.abs(ref).max() + 1e-6
    dropped = ~keep
    assert (out[dropped] == 0).all() and not np.signbit(out[dropped]).any(), what  # dropped: exactly +0.0
    # informative elements: the undropped value is clearly non-zero (ReLU: clearly positive)
    informative = (ref > bar) if epilogue == 'res_relu' else (np.abs(ref) > bar)
    assert informative.mean() > (0.3 if epilogue == 'res_relu' else 0.95), what
    assert np.array_equal(out[informative] != 0, keep[informative]), (what, float(((out != 0) != keep)[informative].mean()))
    err = np.abs(out - 2.0 * ref)[keep].max()
    assert err <= 2 * bar, (what, err, bar)
    if got.shape[1] % 8:
        assert float(padded(got)[:, got.shape[1]:].abs().max()) == 0.0, what  # pad channels of own rows stay 0


@pytest.mark.parametrize('row', TABLE, ids=[r[0] for r in TABLE])
def test_dropout_layer_matches_restatement(row):
    from online_joint_depthfusion_and_semantic_amd.segconv import SegConv
    name, B, n, same = row[0], row[9], row[10], row[12]
    seed, frame = STATES[TABLE.index(row) % 2]
    convs, xs, ress, gates, lins = make_case(row)
    dev = torch.device('cuda:0')
    ops = [SegConv(c) for c in convs]
    xg = [to_nhwc_batch(x.to(dev)) for x in xs]
    rg = [to_nhwc_batch(r.to(dev)) for r in ress]
    gg = [to_nhwc_batch(g.to(dev)) for g in gates]
    state = torch.tensor([seed, frame], dtype=torch.int64, device=dev)
    sids = [11 + 16 * m for m in range(n)]
    keeps = [keep_mask_nchw(seed, frame, sid, *lins[0].shape) for sid in sids]
    for epilogue in EPILOGUES:
        for op in ops:
            op.set_dropout(None)
        plain = [o.clone() for o in launch(ops, xg, rg, gg, epilogue)]
        for op, sid in zip(ops, sids):
            op.set_dropout(state, sid)
        drop = launch(ops, xg, rg, gg, epilogue)
        torch.cuda.synchronize()
        assert state.tolist() == [seed, frame]  # a dropping layer reads the state, it does not advance it
        for m in range(n):
            what = (name, epilogue, m)
            check_member(drop[m], lins[m], ress[m], gates[m], epilogue, keeps[m], what)
            if same:  # same kernel form without the generator: the same sums, then v + v or +0.0
                k = torch.from_numpy(keeps[m]).to(dev)
                assert torch.equal(drop[m], torch.where(k, plain[m] + plain[m], torch.zeros_like(plain[m]))), what
        if n > 1 and epilogue != 'res_relu':  # members draw independent masks (their own stream ids)
            assert 0.4 < ((drop[0] != 0) != (drop[1] != 0)).float().mean().item() < 0.6, (name, epilogue)
    from online_joint_depthfusion_and_semantic_amd import _lib
    assert _lib.load().ojf_net_check(_lib.stream_ptr(dev)) == 0


def run_table_traced():
    """Child process body of test_table_reaches_every_drop_form: every TABLE row with and without dropout, each launch
    preceded by a marker line on stderr."""
    from online_joint_depthfusion_and_semantic_amd.segconv import SegConv
    dev = torch.device('cuda:0')
    state = torch.tensor(STATES[0], dtype=torch.int64, device=dev)
    for row in TABLE:
        convs, xs, _, _, _ = make_case(row, fp64=False)
        ops = [SegConv(c) for c in convs]
        xg = [to_nhwc_batch(x.to(dev)) for x in xs]
        for mode in ('drop', 'plain'):
            for m, op in enumerate(ops):
                op.set_dropout(state if mode == 'drop' else None, 11 + 16 * m)
            sys.stderr.write('CASE %s %s\n' % (row[0], mode))
            sys.stderr.flush()
            launch(ops, xg, None, None, 'plain')
            torch.cuda.synchronize()
    sys.stderr.write('CASE end\n')


_TRACE_SCRIPT = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tests'))
import test_segconv_dropout_gpu as t
t.run_table_traced()
print('TRACED')
'''


def test_table_reaches_every_drop_form():
    """OJF_SEG_TRACE=1 in a child process (every other OJF_SEG_* switch removed): each TABLE row's dropout launch takes the
    form the table names (gemm forms: aligned iff c_in / 8 is a multiple of 4), the rows marked bit-exact take the same
    form without dropout, and every DROP form of the default dispatcher - both tap walks of every GEMM tile - is reached."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith('OJF_SEG_')}
    env['OJF_SEG_TRACE'] = '1'
    out = subprocess.run([sys.executable, '-c', _TRACE_SCRIPT, root], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'TRACED' in out.stdout, out.stderr[-3000:]
    forms, case = {}, None
    for line in out.stderr.splitlines():
        if line.startswith('CASE '):
            case = tuple(line.split()[1:])
            continue
        m = re.match(r'segconv (.+?) +n \d+ ', line)
        if m and case is not None:
            forms.setdefault(case, []).append(m.group(1))
    reached = set()
    for row in TABLE:
        name, cin, form, same = row[0], row[1], row[11], row[12]
        got = forms.get((name, 'drop'))
        assert got == [form], (name, got)  # one launch for the whole group, in the named form
        aligned = ((cin + 7) // 8) % 4 == 0
        reached.add((form, aligned) if form.startswith('gemm') else form)
        plain = forms.get((name, 'plain'))
        assert plain is not None and len(plain) == 1, (name, plain)
        assert (plain[0] == form.replace(' drop', '')) == same, (name, plain, form)
    want = {(f, a) for f in DROP_FORMS if f.startswith('gemm') for a in (True, False)} | {f for f in DROP_FORMS if not f.startswith('gemm')}
    assert reached == want, sorted(map(str, want - reached))


# ---- the frame counter ------------------------------------------------------------------------------------------------
# (c_in, c_out, k, stride, dilation, padding, H, W, batch, members): forms without dropout - the GEMM tiles, the plain and
# split-K forms - single, grouped and batched
ADVANCE_SHAPES = [
    (512, 2048, 1, 1, 1, 0, 15, 20, 1, 2), (128, 2048, 1, 1, 1, 0, 15, 20, 3, 2), (512, 2048, 1, 1, 1, 0, 15, 20, 4, 2),
    (232, 128, 3, 1, 1, 1, 30, 40, 8, 2), (64, 512, 1, 1, 1, 0, 30, 40, 1, 2), (64, 512, 1, 1, 1, 0, 4, 6, 1, 1),
    (64, 30, 3, 1, 1, 1, 7, 9, 1, 1), (64, 6, 1, 1, 1, 0, 7, 9, 2, 1), (1024, 512, 1, 1, 1, 0, 15, 20, 1, 1),
    (512, 256, 3, 1, 8, 8, 15, 20, 1, 2), (64, 64, 3, 1, 1, 1, 240, 320, 1, 1), (256, 30, 1, 1, 1, 0, 240, 320, 1, 1),
]


def test_advancing_layer_adds_one_per_launch():
    """advance=True: every launch of the layer adds exactly 1 to frame (whatever the form, grid, batch or group size; member 0
    of a group advances), leaves the seed word alone, carries 2^32 - 1 into the high word, and drops nothing."""
    from online_joint_depthfusion_and_semantic_amd import segconv
    from online_joint_depthfusion_and_semantic_amd.segconv import SegConv, SegDeconv
    dev = torch.device('cuda:0')
    seed = -0x5a5a5a5a12345678
    frame = (7 << 32) | 0xfffffffe  # the second launch carries into the high word
    state = torch.tensor([seed, frame], dtype=torch.int64, device=dev)
    for i, shape in enumerate(ADVANCE_SHAPES):
        row = ('advance',) + shape
        convs, xs, ress, _, _ = make_case(row, seed=i, fp64=False)
        ops = [SegConv(c) for c in convs]
        xg = [to_nhwc_batch(x.to(dev)) for x in xs]
        rg = [to_nhwc_batch(r.to(dev)) for r in ress]
        plain = [o.clone() for o in segconv.group(ops, xg, act='relu', residuals=rg)]
        single = ops[0](xg[0], act='relu', residual=rg[0]).clone()  # (one member alone may take another form than the group)
        ops[0].set_dropout(state, 3, advance=True)
        got = segconv.group(ops, xg, act='relu', residuals=rg)
        torch.cuda.synchronize()
        frame += 1
        assert state.tolist() == [seed, frame], (shape, state.tolist(), frame)
        assert all(torch.equal(a, b) for a, b in zip(plain, got)), shape  # no dropout on the advancing layer
        got = ops[0](xg[0], act='relu', residual=rg[0])  # the single call advances too
        torch.cuda.synchronize()
        frame += 1
        assert state.tolist() == [seed, frame], shape
        assert torch.equal(got, single), shape
    assert frame >> 32 == 8  # the carry happened
    # the decoder's last transposed convolution is the production advancing layer
    g = torch.Generator().manual_seed(4)
    dc = nn.ConvTranspose2d(48, 12, 8, stride=4, padding=2)
    with torch.no_grad():
        dc.weight.copy_(torch.randn(dc.weight.shape, generator=g) / 8)
    de = SegDeconv(dc)
    y = to_nhwc_batch(torch.randn((3, 48, 15, 20), generator=g).to(dev))
    plain = de(y).clone()
    de.set_dropout(state, advance=True)
    for _ in range(3):
        got = de(y)
        torch.cuda.synchronize()
        frame += 1
        assert state.tolist() == [seed, frame] and torch.equal(got, plain)


@pytest.mark.parametrize('row', [TABLE[1], TABLE[11]], ids=[TABLE[1][0], TABLE[11][0]])
def test_state_is_read_at_launch_time(row):
    """A new {seed, frame} written into the state tensor between two launches - no set_dropout call - changes the masks
    (a captured graph replays with the state it finds)."""
    from online_joint_depthfusion_and_semantic_amd.segconv import SegConv
    dev = torch.device('cuda:0')
    convs, xs, ress, gates, lins = make_case(row)
    ops = [SegConv(c) for c in convs]
    xg = [to_nhwc_batch(x.to(dev)) for x in xs]
    B, (_, c, h, w) = row[9], lins[0].shape
    state = torch.tensor(STATES[0], dtype=torch.int64, device=dev)
    for m, op in enumerate(ops):
        op.set_dropout(state, 40 + m)
    for seed, frame in (STATES[0], (STATES[0][0], STATES[0][1] + 1), STATES[1], (STATES[1][0], 1 << 32)):
        state[0], state[1] = seed, frame
        out = launch(ops, xg, None, None, 'plain')
        for m in range(len(ops)):
            check_member(out[m], lins[m], ress[m], gates[m], 'plain', keep_mask_nchw(seed, frame, 40 + m, B, c, h, w), (row[0], seed, frame))
    assert state.tolist() == list(STATES[1][:1]) + [1 << 32]


def test_refusals():
    """What the C entry points refuse, each with its message - and a refused launch leaves the state alone."""
    from online_joint_depthfusion_and_semantic_amd import _lib, segconv
    from online_joint_depthfusion_and_semantic_amd.segconv import SegConv, SegDeconv
    dev = torch.device('cuda:0')
    state = torch.tensor(STATES[1], dtype=torch.int64, device=dev)
    for row in (TABLE[1], TABLE[11]):  # a GEMM-shaped layer and a plain-form one
        convs, xs, _, _, _ = make_case(row, fp64=False)
        a, b = SegConv(convs[0]), SegConv(convs[0])
        x = to_nhwc_batch(xs[0].to(dev))
        with pytest.raises(_lib.OjfError, match='advance needs the state'):
            a.set_dropout(None, advance=True)
        a.set_dropout(state, 1)
        b.set_dropout(None)
        with pytest.raises(_lib.OjfError, match='dropout on some members only'):
            segconv.group([a, b], [x, x])
        with pytest.raises(_lib.OjfError, match='dropout on some members only'):
            segconv.group([b, a], [x, x])
        a.set_dropout(None)
        b.set_dropout(state, advance=True)
        with pytest.raises(_lib.OjfError, match='only member 0 .* may advance'):
            segconv.group([a, b], [x, x])
        torch.cuda.synchronize()
        assert state.tolist() == list(STATES[1])
        segconv.group([b, a], [x, x])  # member 0 may
        torch.cuda.synchronize()
        assert state.tolist() == [STATES[1][0], STATES[1][1] + 1]
        state[1] = STATES[1][1]
    dc = nn.ConvTranspose2d(16, 8, 4, stride=2, padding=1)
    de = SegDeconv(dc)
    de.set_dropout(state, 2)
    with pytest.raises(_lib.OjfError, match='dropout on a transposed convolution'):
        de(to_nhwc_batch(torch.randn((1, 16, 6, 8), device=dev)))


def test_heterogeneous_launch_with_a_dropout_member():
    """segconv.multi with a dropout member: that member takes a launch of its own and gives the single call's bits; the
    others are unchanged.  An advancing member advances once."""
    from online_joint_depthfusion_and_semantic_amd.segconv import SegConv, multi
    dev = torch.device('cuda:0')
    seed, frame = STATES[0]
    state = torch.tensor([seed, frame], dtype=torch.int64, device=dev)
    row = TABLE[8]  # layer2's last 1x1 (64 -> 512) on 30x40
    convs, xs, ress, gates, lins = make_case(row)
    g = torch.Generator().manual_seed(8)
    other = nn.Conv2d(64, 128, 1, bias=True)
    side = nn.Conv2d(64, 24, 1, bias=True)
    with torch.no_grad():
        other.weight.copy_(torch.randn(other.weight.shape, generator=g) / 8)
        side.weight.copy_(torch.randn(side.weight.shape, generator=g) / 8)
    drop, o1, o2 = SegConv(convs[0]), SegConv(other), SegConv(side)
    x = to_nhwc_batch(xs[0].to(dev))
    r = to_nhwc_batch(ress[0].to(dev))
    drop.set_dropout(state, 9)
    got = multi([(o1, x, {'act': 'relu'}), (drop, x, {'act': 'relu', 'residual': r}), (o2, x, {})])
    single = [o1(x, act='relu'), drop(x, act='relu', residual=r), o2(x)]
    torch.cuda.synchronize()
    for a, b in zip(got, single):
        assert torch.equal(a, b)
    check_member(got[1], lins[0], ress[0], gates[0], 'res_relu', keep_mask_nchw(seed, frame, 9, 1, 512, 30, 40), 'multi')
    assert state.tolist() == [seed, frame]
    drop.set_dropout(None)
    o2.set_dropout(state, advance=True)
    got = multi([(o1, x, {'act': 'relu'}), (o2, x, {})])
    torch.cuda.synchronize()
    assert state.tolist() == [seed, frame + 1]
    assert torch.equal(got[0], single[0]) and torch.equal(got[1], single[2])
