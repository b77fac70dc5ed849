"""train_edge_cases.py without a GPU: the restated constants are the sources', the restated loops visit every pixel exactly once in the
form they name (simulated lane by lane), every row of EDGE_ROWS reaches the edges it claims and every listed edge has a row (computed,
never asserted by hand), the frames of tests/test_train_gpu.py reach what NOT_REACHED_BY_OLD_SIZES / REACHED_ONLY_AT_THE_LOOSE_BAR say,
zeroing any one sentinel pixel moves every reduced output of the float64 reference by at least ten bars, the references agree with a
second statement of the same operation (torch autograd, explicit loops), and the two C entries that expose a plan return the
restatement's sizes."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_edge_cases as ec
from test_train_gpu import REL, _net, _whole_net_inputs
from train_edge_cases import EDGE_ROWS, NEAR_ZERO, OP_ROWS, reached

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'online_joint_depthfusion_and_semantic_amd', 'csrc')


def test_restated_constants_are_the_sources():
    # the training unit: device kernels in the header, plan / launches / C entries in the .hip file
    kern = open(os.path.join(CSRC, 'ojf_train_kernels.h')).read()
    host = open(os.path.join(CSRC, 'ojf_train.hip')).read()

    def const(src, name):
        m = re.search(r'constexpr int [^;]*\b%s = (\d+)[,;]' % name, src)
        assert m, name
        return int(m.group(1))

    assert const(kern, 'kTrainSlabs') == ec.TRAIN_SLABS
    assert const(kern, 'kWgChunk') == ec.WG_CHUNK
    assert (const(kern, 'kTpW'), const(kern, 'kTpH')) == (ec.TP_W, ec.TP_H)
    assert const(kern, 'kLossThreads') == ec.LOSS_THREADS
    # the two reduction loops (statistics, BatchNorm backward): four loads 256 apart, step 1024, tail step 256
    assert len(re.findall(r'for \(; p \+ %d < p1; p \+= %d\)' % (ec.UNROLL_LAST, ec.UNROLL_STEP), kern)) == 2
    assert len(re.findall(r'for \(; p < p1; p \+= %d\)' % ec.BLOCK, kern)) == 2
    assert len(re.findall(r'\[p\], \w+\[p \+ 256\], \w+\[p \+ 512\], \w+\[p \+ %d\]\}' % ec.UNROLL_LAST, kern)) == 3
    assert len(re.findall(r'const int per = \(a?\.?npix \+ kTrainSlabs - 1\) / kTrainSlabs;', kern)) == 2
    assert len(re.findall(r'dim3\(kTrainSlabs, c_phys / 4\), dim3\(%d\)' % ec.BLOCK, host)) == 3
    # the streaming loops: bx = min(ceil(npix / 256), 128) at the two C entries and in the executor; first3, middle, tail
    # (both live in ojf_train.hip now: the C entries size the frame as h * w, the executor as t->npix)
    bx = r'const int bx = \(%s \+ 255\) / 256 < %d \? \(%s \+ 255\) / 256 : %d;'
    entry_bx, executor_bx = (bx % (n, ec.STREAM_MAX_BX, n, ec.STREAM_MAX_BX) for n in (r'h \* w', r't->npix'))
    assert len(re.findall(entry_bx, host)) == 2 and len(re.findall(executor_bx, host)) >= 1
    assert kern.count('const bool first3 = p + 2 * stride < a.npix;') == 2
    assert kern.count('for (; p + 2 * stride < a.npix; p += 3 * stride)') == 2
    assert kern.count('for (; p < a.npix; p += stride)') == 2
    # the weight gradient's plan and the kernel's slab length
    assert 'int slabs = (%d + waves - 1) / waves;' % ec.WG_WAVES in host and 'slabs = slabs > %d ? %d : slabs;' % (ec.WG_MAX_SLABS, ec.WG_MAX_SLABS) in host
    assert 'const int max_slabs = (npix + 63) / 64;' in host and ec.WG_CHUNK == 64
    assert 'p.ocp = round_up(c_out_phys, %d);' % ec.WG_TILE in host and 'p.icp = round_up(c_in_phys, %d);' % ec.WG_TILE in host
    assert 'const int per = ((a.npix + a.slabs - 1) / a.slabs + 1) & ~1;' in kern
    assert 'const int n_og = min(8, a.c4_out - ot * 8), n_ig = min(8, a.c4_in - it * 8);' in kern
    # the small launches
    assert 'const int bx = (h * w + 255) / 256 < %d ? (h * w + 255) / 256 : %d;' % (ec.POOL_MAX_BX, ec.POOL_MAX_BX) in host
    assert 'static inline dim3 px_grid(int npix, int gy) { return dim3((unsigned)((npix + 255) / 256), (unsigned)gy); }' in host
    assert 'for (int b = threadIdx.x; b < a.blocks; b += %d)' % ec.LOSS_FINISH_LANES in kern
    assert 'for (int ot0 = 0; ot0 < n_ot; ot0 += 8)' in host


@pytest.mark.parametrize('npix', [1, 2, 63, 65, 255, 257, 1023, 16448, 51200, 65536, 114700])
def test_restated_reduction_loops_visit_every_pixel_once(npix):
    """the kernel's two loops, lane by lane, against stats_pixel / lane_iterations / slab_forms"""
    per = (npix + 63) // 64
    seen = {}
    for slab in range(64):
        p0, p1 = slab * per, min(npix, slab * per + per)
        unrolled_lanes = tail_lanes = 0
        for lane in range(256):
            p, it = p0 + lane, 0
            while p + 768 < p1:
                for u in range(4):
                    assert p + 256 * u not in seen
                    seen[p + 256 * u] = (slab, lane, 'unrolled load %d' % u, it)
                p += 1024
                it += 1
            unrolled_lanes += it > 0
            it = 0
            while p < p1:
                assert p not in seen
                seen[p] = (slab, lane, 'tail', it)
                p += 256
                it += 1
            tail_lanes += it > 0
        if p0 < npix:
            f = ec.slab_forms(p1 - p0)
            assert (f['unrolled1'] + f['unrolled2plus'], f['tail']) == (unrolled_lanes, tail_lanes)
    assert sorted(seen) == list(range(npix))
    step = max(1, npix // 997)
    for p in list(range(0, npix, step)) + [npix - 1] + list(ec.reduce_sentinels(npix)):
        assert ec.stats_pixel(npix, p) == seen[p], p
    s = ec.stats_plan(npix)
    assert s['nonempty'] == len({v[0] for v in seen.values()}) and s['last_len'] == sum(v[0] == s['nonempty'] - 1 for v in seen.values())


@pytest.mark.parametrize('npix', [1, 255, 256, 257, 32768, 51200, 65536, 65792, 114700, 163840, 164096])
def test_restated_stream_loops_visit_every_pixel_once(npix):
    s = ec.stream_plan(npix)
    stride = s['stride']
    assert stride == 256 * min((npix + 255) // 256, 128)
    seen = np.zeros(npix, np.int32)
    for t in sorted(set(list(range(0, stride, 97)) + [0, 1, stride - 1, s['first3'] - 1, s['first3'], s['middle'] - 1, s['middle']])):
        if not 0 <= t < stride:
            continue
        p, forms = t, []
        f3 = p + 2 * stride < npix
        if f3:
            forms += [(p + k * stride, 'first3 load %d' % k) for k in range(3)]
            p += 3 * stride
        it = 0
        while p + 2 * stride < npix:
            forms += [(p + k * stride, 'middle loop load %d' % k) for k in range(3)]
            p += 3 * stride
            it += 1
        nt = 0
        while p < npix:
            forms.append((p, 'tail loop'))
            p += stride
            nt += 1
        assert (f3, it, nt) == ec.stream_thread(npix, stride, t)
        assert f3 == (t < s['first3']) and (it >= 1) == (t < s['middle']) and (it >= 2) == (t < s['middle2'])
        for q, form in forms:
            seen[q] += 1
            assert ec.stream_pixel(npix, q) == (t, form)
    assert int(seen.max()) <= 1
    assert ec.stream_tail_threads(npix) <= stride


def test_restated_weight_gradient_slabs_cover_the_frame():
    for row in OP_ROWS:
        if row.kind != 'wgrad':
            continue
        p = row.p
        npix = p['h'] * p['w']
        plan = ec.wgrad_plan(p['cop'], p['cip'], p['k'] ** 2, npix)
        covered = 0
        for slab in range(plan['slabs']):
            p0 = slab * plan['per']
            p1 = min(npix, p0 + plan['per'])
            assert p0 % 2 == 0
            covered += max(0, p1 - p0)
            assert (p1 > p0) == (slab < plan['nonempty'])
            if slab == plan['nonempty'] - 1:
                assert p1 - p0 == plan['last_len'] and p1 == npix
        assert covered == npix and plan['slabs'] >= 1 and plan['empty'] == plan['slabs'] - plan['nonempty']
        assert plan['slabs'] <= max(1, (npix + 63) // 64)
        for q in ec.wgrad_sentinels(plan, npix):
            slab, chunk, lane = ec.wgrad_pixel(plan, q)
            assert slab < plan['nonempty'] and 0 <= lane < 64 and chunk < plan['chunks']
    # the example of the row table: 256 slabs of 66 pixels, slabs 251..255 begin beyond the frame
    plan = ec.wgrad_plan(32, 32, 1, 128 * 129)
    assert (plan['slabs'], plan['per'], plan['nonempty'], plan['empty'], plan['last_len']) == (256, 66, 251, 5, 12)


def test_every_row_reaches_what_it_claims():
    names = [r.name for r in EDGE_ROWS]
    assert len(set(names)) == len(names)
    for r in EDGE_ROWS:
        got = reached(r)
        assert not [c for c in r.claims if c not in got], (r.name, sorted(got))
    # the unit rows go through the same computed check: none is without claims
    assert all(r.claims for r in ec.UNIT_ROWS)
    # the numbers of the row table
    assert ec.stats_plan(65)['per'] == 2 and ec.stats_plan(65)['nonempty'] == 33
    assert ec.stats_plan(200 * 256)['full']['unrolled1'] == 32 and ec.stats_plan(200 * 256)['full']['unrolled0'] == 224
    assert (ec.stats_plan(37 * 45)['per'], ec.stats_plan(37 * 45)['full']['tail']) == (27, 27)
    assert ec.stream_plan(256 * 257)['first3'] == 256 and ec.stream_plan(641 * 256)['middle'] == 256 and ec.stream_plan(639 * 256)['middle'] == 0
    assert ec.stream_plan(240 * 320)['first3'] == 11264 and ec.stream_plan(240 * 320)['middle'] == 0
    assert ec.pool_plan(257 * 256) == dict(bx=256, iterations=2, last_block=256)


def test_every_listed_edge_has_a_row():
    everywhere = set()
    for r in EDGE_ROWS:
        everywhere |= reached(r)
    assert not [e for e in ec.EDGES_ANYWHERE if e not in everywhere]
    claimed = {c for r in EDGE_ROWS for c in r.claims}
    assert not [e for e in ec.EDGES_ANYWHERE if e not in claimed]


def test_what_the_older_frame_sizes_reach():
    old = ec.old_sizes_reach()
    assert [e for e in ec.EDGES_ANYWHERE if e not in old] == [e for e in ec.EDGES_ANYWHERE if e in ec.NOT_REACHED_BY_OLD_SIZES]
    assert sorted(ec.NOT_REACHED_BY_OLD_SIZES) == sorted(set(ec.NOT_REACHED_BY_OLD_SIZES))
    assert ec.loose_only() == ec.REACHED_ONLY_AT_THE_LOOSE_BAR
    # 37 x 45, the one frame of the tight per-unit comparison: one tail iteration for 27 lanes, no first3
    tight = ec.old_tight_sizes_reach()
    assert not {ec.R_UNROLLED, ec.S_FIRST3_SOME, ec.S_MIDDLE_SOME, ec.W_EMPTY, ec.W_TAPS_OUT} & tight


# ---- one dropped sentinel pixel is visible in every reduced output (a condition on the reference alone) -----------------------------
BN_ROWS = [r for r in OP_ROWS if r.kind == 'bn']
WG_ROWS = [r for r in OP_ROWS if r.kind == 'wgrad']


@pytest.mark.parametrize('row', BN_ROWS, ids=ec.row_id)
def test_bn_sentinels_move_every_reduced_output_by_ten_bars(row):
    x = ec.bn_inputs(row)
    npix = row.p['h'] * row.p['w']
    assert len(x['sentinels']) >= min(npix, 2)
    for mode in row.p['modes']:
        training = mode == 'train'
        ref = ec.bn_reference(x, training)
        names = ['dgamma', 'dbeta', 'sums', 'squares'] + (['mean'] if training else ['dbias'])
        for q, labels in x['sentinels'].items():
            if npix == 1:
                continue  # (nothing is left of a one-pixel frame: the row is compared, not perturbed)
            z = dict(x, y=x['y'].copy(), dout=x['dout'].copy())
            z['y'][:, q] = 0
            z['dout'][:, q] = 0
            got = ec.bn_reference(z, training)
            for name in names:
                if name in ('sums', 'squares'):  # ojf_train_channel_sums: the fp64 summation bound
                    bar = npix * 2.0 ** -52 * (np.abs(x['y']) if name == 'sums' else x['y'] ** 2).sum(1).max()
                else:
                    bar = REL * np.abs(ref[name]).max()
                moved = np.abs(got[name] - ref[name])
                assert moved.min() >= 10 * bar, (row.name, mode, name, q, labels, float(moved.min() / bar))


@pytest.mark.parametrize('row', WG_ROWS, ids=ec.row_id)
def test_wgrad_sentinels_move_every_weight_gradient_that_sees_them_by_ten_bars(row):
    """dW is linear in dy and in x: without pixel q of dy every dW[oc][ic][tap] whose tap is inside the image at q loses
    dy[oc][q] * x[ic][q + offset(tap)]; without pixel q of x every tap that is inside at q - offset loses dy[oc][q - offset] * x[ic][q]"""
    p = row.p
    x = ec.wgrad_inputs(row)
    ref = ec.wgrad_reference(p, x['x'], x['dy'])
    bar = REL * np.abs(ref).max()
    h, w = p['h'], p['w']
    for q, labels in x['sentinels'].items():
        qy, qx = divmod(q, w)
        seen = 0
        for t, (oy, ox) in enumerate(ec.tap_offsets(p['k'], p['dil'])):
            for sign in (1, -1):  # the pixel as dy's (reads x at q + offset) and as x's (read from q - offset)
                yy, xx = qy + sign * oy, qx + sign * ox
                if not (0 <= yy < h and 0 <= xx < w):
                    continue
                other = yy * w + xx
                delta = np.outer(x['dy'][:, q], x['x'][:, other]) if sign == 1 else np.outer(x['dy'][:, other], x['x'][:, q])
                assert np.abs(delta).min() >= 10 * bar, (row.name, q, labels, t, float(np.abs(delta).min() / bar))
                seen += 1
        assert seen >= 2  # (the centre tap sees every pixel)


# ---- the references against a second statement ------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', [r for r in BN_ROWS if r.p['h'] * r.p['w'] <= 16512], ids=ec.row_id)
def test_bn_reference_against_torch_autograd(row):
    x = ec.bn_inputs(row)
    C, h, w = row.p['C'], row.p['h'], row.p['w']
    for mode in row.p['modes']:
        training = mode == 'train'
        ref = ec.bn_reference(x, training)
        t = lambda a: torch.from_numpy(a.copy())
        y, gamma, beta = (t(x[k]).requires_grad_(True) for k in ('y', 'gamma', 'beta'))
        rm, rv = t(x['rm']), t(x['rv'])
        out = F.batch_norm(y.view(1, C, h, w), rm, rv, gamma, beta, training, ec.MOMENTUM, ec.EPS) * ec.BN_SCALE * ec.BN_DROP
        out.backward(t(x['dout']).view(1, C, h, w))
        for name, got in (('out', out.detach().view(C, -1)), ('dy', y.grad), ('dgamma', gamma.grad), ('dbeta', beta.grad), ('running_mean', rm), ('running_var', rv)):
            scale = float(np.abs(ref[name]).max())
            assert float(np.abs(got.numpy() - ref[name]).max()) <= 1e-11 * max(scale, 1e-30), (row.name, mode, name)
        if training:  # the bias in front of batch statistics receives nothing: sum(dy) is rounding noise
            assert np.abs(ref['dbias']).max() <= 1e-12 * np.abs(x['dout']).sum(1).max()


@pytest.mark.parametrize('row', [r for r in WG_ROWS if r.p['h'] * r.p['w'] <= 200 and r.p['cip'] <= 116], ids=ec.row_id)
def test_wgrad_reference_against_autograd_and_explicit_loops(row):
    p = row.p
    x = ec.wgrad_inputs(row)
    ref = ec.wgrad_reference(p, x['x'], x['dy'])
    h, w, k, dil = p['h'], p['w'], p['k'], p['dil']
    wt = torch.zeros(p['OC'], p['IC'], k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(torch.from_numpy(x['x']).view(1, -1, h, w), wt, padding=dil * (k // 2), dilation=dil).backward(torch.from_numpy(x['dy']).view(1, -1, h, w))
    assert float((wt.grad.reshape(ref.shape) - torch.from_numpy(ref)).abs().max()) <= 1e-12 * np.abs(ref).max()
    if h * w <= 24:  # dW[oc][ic][tap] = sum_p dy[oc][p] * x[ic][p + off], written out
        loops = np.zeros_like(ref)
        for t, (oy, ox) in enumerate(ec.tap_offsets(k, dil)):
            for q in range(h * w):
                yy, xx = q // w + oy, q % w + ox
                if 0 <= yy < h and 0 <= xx < w:
                    loops[:, :, t] += np.outer(x['dy'][:, q], x['x'][:, yy * w + xx])
        assert np.abs(loops - ref).max() <= 1e-12 * np.abs(ref).max()
        inside = ec.taps_inside(k, dil, h, w)
        for t in range(k * k):
            assert (np.abs(ref[:, :, t]).max() > 0) == inside[t]


def test_bn_rows_are_well_conditioned():
    """dy = gamma invstd (dz - mean(dz) - x-hat mean(dz x-hat)) cancels when x-hat^2 is 1 everywhere (two pixels): a row whose dy is less than
    a hundredth of its terms would measure the rounding of the saved fp32 mean / invstd, not the kernel (see bn_1x2)"""
    for row in BN_ROWS:
        if 'train' in row.p['modes']:
            ref = ec.bn_reference(ec.bn_inputs(row), True)
            assert np.abs(ref['terms']).max() <= 100 * np.abs(ref['dy']).max(), row.name


def test_inputs_are_zero_mean_and_fp32_exact():
    for row in BN_ROWS + WG_ROWS:
        x = ec.bn_inputs(row) if row.kind == 'bn' else ec.wgrad_inputs(row)
        for name in ('y', 'dout') if row.kind == 'bn' else ('x', 'dy'):
            a = x[name]
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
            n = a.shape[1]
            if n >= 4096 and row.p.get('y_scale', 1.0) == 1.0:  # the mean of n values of unit size: within 6 sigma of 0, sentinels included
                assert np.abs(a.mean(1)).max() <= 6 * np.abs(a).max() / ec.SENTINEL_SCALE * (1.1 / np.sqrt(n) + 30 * ec.SENTINEL_SCALE / n), row.name


def executor_reference_instability(version, sem, h, w, seed):
    """-> the largest gradient change, in bars of _whole_net_gradient_case, that taking the other side of one near-zero ReLU / LeakyReLU
    pre-activation (|z| < NEAR_ZERO of its tensor) causes in the float64 net, and the number of such points; L1 residuals below
    NEAR_ZERO of the largest count as unstable outright (inf)."""
    x, target = _whole_net_inputs(h, w, seed)
    x, target = {k: v.double() for k, v in x.items()}, target.double()

    def grads(flip=None, found=None):
        net = _net(version, sem, h, w).double().eval()
        for name, m in net.named_modules():
            if isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU)):
                def pre(mod, inp, name=name):
                    z = inp[0]
                    if found is not None:
                        a = z.detach().abs()
                        found.extend((name, tuple(int(i) for i in at)) for at in (a < NEAR_ZERO * float(a.max())).nonzero())
                    if flip is not None and flip[0] == name:
                        z = z.clone()
                        z[flip[1]] = -z[flip[1]]
                        return (z,)
                m.register_forward_pre_hook(pre)
        e = net(x)
        ((e - target).abs().mean() + 10 * ((e - target) ** 2).mean()).backward()
        return e.detach(), {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
    found = []
    est, base = grads(found=found)
    if float((est - target).abs().min()) < NEAR_ZERO * float((est - target).abs().max()):
        return float('inf'), len(found)
    gmax = max(float(v.abs().max()) for v in base.values())
    worst = 0.0
    for point in found:
        _, other = grads(flip=point)
        worst = max(worst, max(float((base[n] - other[n]).abs().max()) / (REL * max(float(base[n].abs().max()), 1e-3 * gmax)) for n in base))
    return worst, len(found)


@pytest.mark.parametrize('row', ec.EXECUTOR_ROWS, ids=ec.row_id)
def test_executor_rows_compare_at_inputs_where_the_reference_is_stable(row):
    """see train_edge_cases.EXECUTOR_INPUT_SEEDS: the row's seed is the first of 11, 12, ... at which no near-zero ReLU pre-activation
    of the float64 net, taken on its other side, moves a gradient by more than half a bar"""
    p = row.p
    for seed in range(11, p['input_seed'] + 1):
        moved, points = executor_reference_instability(p['version'], p['sem'], p['h'], p['w'], seed)
        print('%s seed %d: %d near-zero pre-activations, the other side moves a gradient by at most %.3g bars' % (row.name, seed, points, moved))
        assert (moved <= 0.5) == (seed == p['input_seed']), (row.name, seed, moved)


# ---- the library's own statements of the plans ------------------------------------------------------------------------------------
def _library():
    from online_joint_depthfusion_and_semantic_amd import _lib
    try:
        return _lib.load()  # (a library that was never built is an error, as everywhere in the suite)
    except OSError as e:  # libojf.so links the HIP runtime; a host without it cannot load the library
        pytest.skip('libojf.so is built but cannot be loaded on this host: %s' % e)


def test_library_plan_sizes_equal_the_restatement():
    lib = _library()
    for row in EDGE_ROWS:
        p = row.p
        if row.kind == 'wgrad':
            shapes = [(p['cop'], p['cip'], p['k'], p['h'], p['w'])]
        elif row.kind == 'unit':
            s = p['shape']
            shapes = [(ec.round_up(s[1], 4), ec.round_up(ec.cdiv(s[0], s[4]) * s[5], 4), s[2], p['h'], p['w'])]
        elif row.kind == 'executor':
            shapes = [(cop, cip, k, p['h'], p['w']) for cop, cip, k, _, _ in ec.EXECUTOR_UNIT_SHAPES]
        else:
            shapes = []
        for cop, cip, k, h, w in shapes:
            assert lib.ojf_train_wgrad_partial_floats(cop, cip, k, h, w) == ec.wgrad_plan(cop, cip, k * k, h * w)['partial_floats'], (row.name, cop, cip, k)
        if row.kind == 'loss':
            assert lib.ojf_train_loss_partial_doubles(p['nv']) == 4 * ec.loss_plan(p['nv'])['blocks']
    for c in (4, 8, 20, 116, 132):
        assert lib.ojf_train_partial_doubles(c) == ec.TRAIN_SLABS * (c // 4) * 8
    for c_out in (4, 20, 116, 132):  # ojf_train_packed_floats: n_ot padded to a multiple of kNT = 2 tiles of 16 rows
        assert lib.ojf_train_packed_floats(c_out, 8, 1) == ec.conv_plan(c_out)['n_ot'] * (lib.ojf_train_packed_floats(16, 8, 1) // 2)
    assert ec.conv_plan(132)['launches'] == [(0, 8, 32), (8, 2, 1)]
