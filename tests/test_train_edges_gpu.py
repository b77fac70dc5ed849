"""-m gpu: the training kernels at their slab, chunk and stream-loop edges (tests/train_edge_cases.py::EDGE_ROWS).

 * op rows call the C ABI (ojf_train_*) one operator at a time.  Every tensor lies in a buffer wider than its window (non-zero,
   distinct *_g0), NaN outside: a read outside the window poisons the result, a write outside it changes bits that must stay.  Every
   output buffer starts NaN-filled, every row runs twice and must repeat bit for bit (the reductions claim a fixed order).
 * unit rows run LayerUnit in both `training` settings at the frames where the loops change form.
 * executor rows run HipTrainNet(executor=True) on whole nets in eval() mode at frames around one 32 x 8 pyramid tile.

References: float64 numpy / torch on the CPU from the operation's definition (tests/test_train_edges_host.py checks them against a
second statement).  Bars: REL = 1e-4 of a tensor's largest reference magnitude, per element (tests/test_train_gpu.py); padding
channels exactly 0, groups outside a window unchanged bits; ojf_train_channel_sums within the fp64 summation bound
npix * 2^-52 * sum|v|; ojf_train_fuse_output bit for bit; executor rows at _whole_net_gradient_case's bar and 2e-5 for the
split-fp16 passes, which are also held against the fp32 backward pass at the same 2e-5.  A failing row names its worst element and
where the restatement puts it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_edge_cases as ec
from test_train_gpu import REL, slotted, _guard_inputs, _net, _whole_net_gradient_case, _second_pass_case
from online_joint_depthfusion_and_semantic_amd import _lib
from online_joint_depthfusion_and_semantic_amd.train import HipTrainNet, LayerUnit, to_c4, from_c4

pytestmark = pytest.mark.gpu
NAN = float('nan')


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same_bits(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _dev(a, cuda, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(cuda)


def _window(planes, g0, after, cuda):
    """C4 planes [c4, npix, 4] inside a NaN buffer of g0 groups in front and `after` groups behind"""
    c4, npix, _ = planes.shape
    buf = torch.full((g0 + c4 + after, npix, 4), NAN, device=cuda)
    buf[g0:g0 + c4] = _dev(planes, cuda)
    return buf


def _outside_untouched(buf, g0, c4, what):
    fill = _bits(torch.full((1,), NAN))[0]
    b = _bits(buf)
    assert bool((b[:g0] == fill).all()) and bool((b[g0 + c4:] == fill).all()), '%s: a group outside the window was written' % what


def _check(got, ref, what, where=None, slack=0.0):
    """per element |got - ref| <= REL * max|ref| (+ slack); -> err / bar"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bar = REL * max(float(np.abs(ref).max()), 1e-30) + slack
    diff = np.abs(got - ref)
    diff[np.isnan(got)] = np.inf
    worst = float(diff.max())
    if worst > bar:
        at = np.unravel_index(int(diff.argmax()), diff.shape)
        pytest.fail('%s: %d of %d elements beyond the bar %.3e; worst %.3e (got %r, want %r) at %r%s'
                    % (what, int((diff > bar).sum()), diff.size, bar, worst, float(got[at]), float(ref[at]), tuple(int(i) for i in at),
                       (': ' + where(at)) if where else ''))
    return worst / bar


# ---- op rows ------------------------------------------------------------------------------------------------------------------------
def _run_bn(lib, cuda, row, x, training):
    p = row.p
    C, h, w = p['C'], p['h'], p['w']
    c_phys = ec.round_up(C, 4)
    c4 = c_phys // 4
    g = dict(y=1, out=2, dout=3, dy=4) if p['windows'] else dict(y=0, out=0, dout=0, dy=0)
    after = 1 if p['windows'] else 0
    st = _lib.stream_ptr(cuda)
    y = _window(ec.to_planes(x['y'], c_phys), g['y'], after, cuda)
    dout = _window(ec.to_planes(x['dout'], c_phys), g['dout'], after, cuda)
    npix = h * w
    out = torch.full((g['out'] + c4 + after, npix, 4), NAN, device=cuda)
    dy = torch.full((g['dy'] + c4 + after, npix, 4), NAN, device=cuda)
    gamma, beta, rm, rv = (_dev(x[k], cuda) for k in ('gamma', 'beta', 'rm', 'rv'))
    drop = torch.full((C,), ec.BN_DROP, device=cuda)
    mean, invstd = torch.full((c_phys,), NAN, device=cuda), torch.full((c_phys,), NAN, device=cuda)
    n_part = lib.ojf_train_partial_doubles(c_phys)
    part_f, part_b, part_s = (torch.full((n_part,), NAN, dtype=torch.float64, device=cuda) for _ in range(3))
    dgamma, dbeta, dbias = (torch.full((C,), NAN, device=cuda) for _ in range(3))
    _lib.check(lib.ojf_train_bn_act(y.data_ptr(), g['y'], out.data_ptr(), g['out'], c_phys, C, h, w, gamma.data_ptr(), beta.data_ptr(), drop.data_ptr(),
                                    _lib.ACT_NONE, ec.BN_SCALE, 1, int(training), ec.MOMENTUM, ec.EPS, rm.data_ptr(), rv.data_ptr(), part_f.data_ptr(),
                                    mean.data_ptr(), invstd.data_ptr(), st), 'ojf_train_bn_act')
    _lib.check(lib.ojf_train_bn_act_bwd(y.data_ptr(), g['y'], dout.data_ptr(), g['dout'], dy.data_ptr(), g['dy'], c_phys, C, h, w, mean.data_ptr(),
                                        invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), drop.data_ptr(), _lib.ACT_NONE, ec.BN_SCALE, 1, int(training),
                                        part_b.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), dbias.data_ptr(), 0, st), 'ojf_train_bn_act_bwd')
    _lib.check(lib.ojf_train_channel_sums(y.data_ptr(), g['y'], c_phys, h, w, part_s.data_ptr(), st), 'ojf_train_channel_sums')
    torch.cuda.synchronize()
    got = dict(out=out, dy=dy, dgamma=dgamma, dbeta=dbeta, dbias=dbias, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, sums=part_s)
    return {k: v.cpu() for k, v in got.items()}, g, c4


def _bn_where(x, npix):
    def where(at):
        q = int(at[-1])
        slab, lane, form, it = ec.stats_pixel(npix, q)
        t, sform = ec.stream_pixel(npix, q)
        return ('channel %d, pixel %d: reduction slab %d lane %d %s iteration %d; stream thread %d %s; %s'
                % (at[0], q, slab, lane, form, it, t, sform, 'sentinel (%s)' % ', '.join(x['sentinels'][q]) if q in x['sentinels'] else 'no sentinel'))
    return where


def _bn_row(lib, cuda, row):
    p = row.p
    C, npix = p['C'], p['h'] * p['w']
    x = ec.bn_inputs(row)
    worst = {}
    for mode in p['modes']:
        training = mode == 'train'
        ref = ec.bn_reference(x, training)
        got, g, c4 = _run_bn(lib, cuda, row, x, training)
        again, _, _ = _run_bn(lib, cuda, row, x, training)
        assert _same_bits(got, again), '%s %s: the second run differs from the first' % (row.name, mode)
        where = _bn_where(x, npix)
        e = {}
        for name in ('out', 'dy'):
            buf = got[name]
            _outside_untouched(buf, g[name], c4, '%s %s %s' % (row.name, mode, name))
            win = buf[g[name]:g[name] + c4].numpy()
            e[name] = _check(ec.from_planes(win, range(C)), ref[name], '%s %s %s' % (row.name, mode, name), where)
            pad = ec.from_planes(win, range(C, 4 * c4))
            assert pad.size == 0 or float(np.abs(pad).max()) == 0.0, '%s %s %s: padding channels are not zero' % (row.name, mode, name)
        for name in ('dgamma', 'dbeta', 'running_mean', 'running_var'):
            e[name] = _check(got[name].numpy(), ref[name], '%s %s %s' % (row.name, mode, name))
        for name in ('mean', 'invstd'):
            e[name] = _check(got[name].numpy()[:C], ref[name], '%s %s %s' % (row.name, mode, name))
            assert float(np.abs(got[name].numpy()[C:]).max()) == 0.0
        if training:  # the bias in front of batch statistics receives exactly nothing
            assert float(got['dbias'].abs().max()) == 0.0, (row.name, mode, 'dbias')
        else:
            e['dbias'] = _check(got['dbias'].numpy(), ref['dbias'], '%s %s dbias' % (row.name, mode))
        # ojf_train_channel_sums: 64 rows of fp64 sums of fp32 values and of their (exact) squares, per slab and in total
        rows = got['sums'].numpy().reshape(ec.TRAIN_SLABS, c4, 8)
        per = ec.stats_plan(npix)['per']
        for name, lo, v in (('sums', 0, x['y']), ('squares', 4, x['y'] ** 2)):
            bound = npix * 2.0 ** -52 * np.abs(v).sum(1)
            slabs = rows[:, :, lo:lo + 4].reshape(ec.TRAIN_SLABS, 4 * c4)
            for s in range(ec.TRAIN_SLABS):
                want = v[:, s * per:min(npix, (s + 1) * per)].sum(1)
                assert bool((np.abs(slabs[s, :C] - want) <= bound).all()), '%s %s: slab %d of the channel %s' % (row.name, mode, s, name)
            assert float(np.abs(slabs[:, C:]).max() if 4 * c4 > C else 0.0) == 0.0
            total = np.abs(slabs[:, :C].sum(0) - ref[name])
            assert bool((total <= bound).all()), '%s %s: channel %s off by %r, bound %r' % (row.name, mode, name, total, bound)
            e[name] = float((total / bound).max())
        worst[mode] = e
    return worst


def _run_wgrad(lib, cuda, row, x):
    p = row.p
    npix, taps = p['h'] * p['w'], p['k'] ** 2
    g = dict(x=2, dy=1) if p['windows'] else dict(x=0, dy=0)
    after = 1 if p['windows'] else 0
    xb = _window(ec.to_planes(x['x'], p['cip'], ec.slot_channels(p['IC'], p['group'], p['slot'])), g['x'], after, cuda)
    dyb = _window(ec.to_planes(x['dy'], p['cop']), g['dy'], after, cuda)
    part = torch.full((lib.ojf_train_wgrad_partial_floats(p['cop'], p['cip'], p['k'], p['h'], p['w']),), NAN, device=cuda)
    dw = _dev(x['dw0'], cuda) if p['accumulate'] else torch.full((p['OC'], p['IC'], taps), NAN, device=cuda)
    _lib.check(lib.ojf_train_wgrad(xb.data_ptr(), g['x'], p['cip'], dyb.data_ptr(), g['dy'], p['cop'], p['OC'], p['IC'], p['k'], p['dil'], p['group'], p['slot'],
                                   p['h'], p['w'], part.data_ptr(), dw.data_ptr(), p['accumulate'], _lib.stream_ptr(cuda)), 'ojf_train_wgrad')
    torch.cuda.synchronize()
    return dict(dw=dw.cpu(), partial=part.cpu())


def _wgrad_row(lib, cuda, row):
    p = row.p
    x = ec.wgrad_inputs(row)
    ref = ec.wgrad_reference(p, x['x'], x['dy']) + (x['dw0'] if p['accumulate'] else 0.0)
    got, again = _run_wgrad(lib, cuda, row, x), _run_wgrad(lib, cuda, row, x)
    assert _same_bits(got, again), '%s: the second run differs from the first' % row.name
    plan = x['plan']
    assert got['partial'].numel() == plan['partial_floats'] and bool(torch.isfinite(got['partial']).all()), '%s: partial sums not all written' % row.name
    part = got['partial'].view(plan['slabs'], -1)
    assert float(part[plan['nonempty']:].abs().max() if plan['empty'] else 0.0) == 0.0, '%s: an empty slab holds a sum' % row.name
    inside = ec.taps_inside(p['k'], p['dil'], p['h'], p['w'])

    def where(at):
        return 'oc %d (tile %d), ic %d (physical %d, tile %d), tap %d (%s the image); slabs %d of %d pixels, %d empty, last %d' % (
            at[0], at[0] // 32, at[1], ec.slot_channels(p['IC'], p['group'], p['slot'])[at[1]], ec.slot_channels(p['IC'], p['group'], p['slot'])[at[1]] // 32,
            at[2], 'inside' if inside[at[2]] else 'outside', plan['slabs'], plan['per'], plan['empty'], plan['last_len'])
    e = _check(got['dw'].numpy(), ref, row.name + ' dW', where)
    if not p['accumulate']:
        for t in range(p['k'] ** 2):
            if not inside[t]:
                assert float(got['dw'][:, :, t].abs().max()) == 0.0, '%s: tap %d is outside the image for every pixel' % (row.name, t)
    return dict(dW=e)


def _conv_row(lib, cuda, row):
    p = row.p
    h, w, k, dil, OC, IC, cop, cip = (p[n] for n in ('h', 'w', 'k', 'dil', 'OC', 'IC', 'cop', 'cip'))
    npix = h * w
    rng = np.random.default_rng(ec._seed(row.name))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    x, dy = ec.signed_unit(rng, (IC, npix)), ec.signed_unit(rng, (OC, npix)) * ec.DOUT_SCALE
    wt, bias = f32(rng.normal(0, 1, (OC, IC, k, k)) / np.sqrt(IC * k * k)), f32(rng.normal(0, 0.1, OC))
    xr = torch.from_numpy(x).view(1, IC, h, w).requires_grad_(True)
    yr = F.conv2d(xr, torch.from_numpy(wt), torch.from_numpy(bias), padding=dil * (k // 2), dilation=dil)
    yr.backward(torch.from_numpy(dy).view(1, OC, h, w))
    st = _lib.stream_ptr(cuda)
    wd, bd = _dev(wt, cuda), _dev(bias, cuda)

    def run():
        packed = torch.full((lib.ojf_train_packed_floats(cop, cip, k),), NAN, device=cuda)
        bias_packed = torch.full((ec.conv_plan(cop)['n_ot'] * 16,), NAN, device=cuda)
        packed_t = torch.full((lib.ojf_train_packed_floats(cip, cop, k),), NAN, device=cuda)
        _lib.check(lib.ojf_train_pack(wd.data_ptr(), bd.data_ptr(), OC, IC, k, IC, cip, cip, cop, 0, packed.data_ptr(), bias_packed.data_ptr(), st), 'ojf_train_pack')
        _lib.check(lib.ojf_train_pack(wd.data_ptr(), None, OC, IC, k, IC, cip, cip, cop, 1, packed_t.data_ptr(), None, st), 'ojf_train_pack (transposed)')
        xb, dyb = _window(ec.to_planes(x, cip), 3, 1, cuda), _window(ec.to_planes(dy, cop), 2, 1, cuda)
        out = torch.full((1 + cop // 4 + 8, npix, 4), NAN, device=cuda)  # (room for a whole 8-tile chunk behind the window)
        dx = torch.full((4 + cip // 4 + 8, npix, 4), NAN, device=cuda)
        _lib.check(lib.ojf_train_conv(xb.data_ptr(), 3, cip, out.data_ptr(), 1, cop, packed.data_ptr(), bias_packed.data_ptr(), k, dil, h, w, st), 'ojf_train_conv')
        _lib.check(lib.ojf_train_conv(dyb.data_ptr(), 2, cop, dx.data_ptr(), 4, cip, packed_t.data_ptr(), None, k, dil, h, w, st), 'ojf_train_conv (backward-data)')
        torch.cuda.synchronize()
        return dict(out=out.cpu(), dx=dx.cpu(), packed=packed.cpu(), packed_t=packed_t.cpu(), bias_packed=bias_packed.cpu())
    got, again = run(), run()
    assert _same_bits(got, again), '%s: the second run differs from the first' % row.name
    assert all(bool(torch.isfinite(got[n]).all()) for n in ('packed', 'packed_t', 'bias_packed')), '%s: packed weights not all written' % row.name
    e = {}
    launches = ec.conv_plan(cop)['launches']
    for name, g0, cph, C, ref in (('out', 1, cop, OC, yr.detach().view(OC, npix).numpy()), ('dx', 4, cip, IC, xr.grad.view(IC, npix).numpy())):
        _outside_untouched(got[name], g0, cph // 4, '%s %s' % (row.name, name))
        win = got[name][g0:g0 + cph // 4].numpy()
        e[name] = _check(ec.from_planes(win, range(C)), ref, '%s %s' % (row.name, name),
                         lambda at: 'channel %d (group %d; launches of (first tile, tiles, groups stored) %r), pixel (y %d, x %d)' % (at[0], at[0] // 4, launches, at[1] // w, at[1] % w))
        assert float(np.abs(ec.from_planes(win, range(C, cph))).max()) == 0.0, '%s %s: padding channels are not zero' % (row.name, name)
    return e


def _pool_row(lib, cuda, row):
    p = row.p
    h, w, c = p['h'], p['w'], p['c']
    rng = np.random.default_rng(ec._seed(row.name))
    x = ec.signed_unit(rng, (c, h * w))
    ref = F.avg_pool2d(torch.from_numpy(x).view(1, c, h, w), 3, 1, 1, count_include_pad=True).view(c, -1).numpy()
    xb = _dev(ec.to_planes(x, c), cuda)

    def run():
        out = torch.full((c // 4 + 1, h * w, 4), NAN, device=cuda)
        _lib.check(lib.ojf_train_avgpool3(xb.data_ptr(), out.data_ptr(), c, h, w, _lib.stream_ptr(cuda)), 'ojf_train_avgpool3')
        torch.cuda.synchronize()
        return dict(out=out.cpu())
    got, again = run(), run()
    assert _same_bits(got, again)
    _outside_untouched(got['out'], 0, c // 4, row.name)
    plan = ec.pool_plan(h * w)
    return dict(out=_check(ec.from_planes(got['out'][:c // 4].numpy(), range(c)), ref, row.name,
                           lambda at: 'channel %d, pixel (y %d, x %d), grid-stride iteration %d of %d' % (at[0], at[1] // w, at[1] % w, at[1] // (256 * plan['bx']), plan['iterations'])))


def _loss_row(lib, cuda, row):
    from online_joint_depthfusion_and_semantic_amd.loss import FusionLoss
    nv, P, init = row.p['nv'], 9, 0.1
    n = nv + 37
    g = torch.Generator().manual_seed(ec._seed(row.name))
    est = (torch.rand(P, n, generator=g) - 0.5) * 0.4          # beyond +-init on both sides
    fv = (torch.rand(P, n, generator=g) - 0.5) * 0.2
    fw = torch.rand(P, n, generator=g) * 3 - 0.3                # some negative weights
    valid = torch.sort(torch.randperm(n, generator=g)[:nv]).values
    target = (torch.rand(nv, P, generator=g) - 0.5) * 0.2
    target[:min(nv, 5) // 2] = 0.0                              # sign(0) rows
    d_rows = (torch.rand(nv, P, generator=g) - 0.5) * 2e-5
    fwc = torch.clamp_min(fw, 0)
    fused_ref = ((fwc * fv + torch.clamp(est, -init, init)) / (fwc + 1)).t()[valid]  # fp32: the same three roundings
    inside = ~(est.double() < -init) & ~(est.double() > init)
    d_est_ref = torch.zeros(P, n, dtype=torch.float64)
    d_est_ref[:, valid] = (d_rows.double() / (fwc.double()[:, valid].t() + 1)).t()
    d_est_ref = d_est_ref * inside
    crit = FusionLoss(w_l1=1.0, w_l2=10.0, w_cos=0.1)
    e64 = fused_ref.double().unsqueeze(0).requires_grad_(True)
    loss_ref = crit(e64, target.double().unsqueeze(0))
    loss_ref.backward()
    st = _lib.stream_ptr(cuda)
    dv = lambda t: t.contiguous().to(cuda)
    est_d, fv_d, fw_d, valid_d, target_d, d_rows_d = dv(est), dv(fv), dv(fw), dv(valid), dv(target), dv(d_rows)
    one = torch.ones((), device=cuda)

    def run():
        rows = torch.full((nv + 1, P), NAN, device=cuda)
        d_est = torch.full((P, n), NAN, device=cuda)
        partial = torch.full((lib.ojf_train_loss_partial_doubles(nv),), NAN, dtype=torch.float64, device=cuda)
        loss = torch.full((), NAN, device=cuda)
        d_loss = torch.full((nv + 1, P), NAN, device=cuda)
        _lib.check(lib.ojf_train_fuse_output(est_d.data_ptr(), fv_d.data_ptr(), fw_d.data_ptr(), valid_d.data_ptr(), n, P, nv, init, rows.data_ptr(), st), 'ojf_train_fuse_output')
        _lib.check(lib.ojf_train_fuse_output_bwd(d_rows_d.data_ptr(), est_d.data_ptr(), fw_d.data_ptr(), valid_d.data_ptr(), n, P, nv, init, d_est.data_ptr(), st),
                   'ojf_train_fuse_output_bwd')
        _lib.check(lib.ojf_train_fusion_loss(rows.data_ptr(), target_d.data_ptr(), nv, P, 1.0, 10.0, 0.1, partial.data_ptr(), loss.data_ptr(), st), 'ojf_train_fusion_loss')
        _lib.check(lib.ojf_train_fusion_loss_bwd(rows.data_ptr(), target_d.data_ptr(), nv, P, 1.0, 10.0, one.data_ptr(), d_loss.data_ptr(), st), 'ojf_train_fusion_loss_bwd')
        torch.cuda.synchronize()
        return dict(rows=rows.cpu(), d_est=d_est.cpu(), loss=loss.cpu().reshape(1), d_loss=d_loss.cpu())
    got, again = run(), run()
    assert _same_bits(got, again), '%s: the second run differs from the first' % row.name
    plan = ec.loss_plan(nv)
    blk = lambda at: 'row %d: block %d of %d, lane %d, finishing lane %d' % (at[0], at[0] // 256, plan['blocks'], at[0] % 256, (at[0] // 256) % 64)
    assert torch.equal(_bits(got['rows'][:nv]), _bits(fused_ref)), '%s: fused rows differ from the fp32 formula' % row.name
    assert bool(torch.isnan(got['rows'][nv]).all()) and bool(torch.isnan(got['d_loss'][nv]).all()), '%s: a row behind the last was written' % row.name
    e = dict(d_est=_check(got['d_est'].numpy(), d_est_ref.numpy(), row.name + ' d_est'),
             loss=_check(got['loss'].numpy(), np.array([float(loss_ref.detach())]), row.name + ' loss'),
             d_loss=_check(got['d_loss'][:nv].numpy(), e64.grad[0].numpy(), row.name + ' d_loss', blk))
    outside = torch.ones(n, dtype=torch.bool)
    outside[valid] = False
    assert float(got['d_est'][:, outside].abs().max()) == 0.0  # masked pixels receive nothing
    return e


_OP = dict(bn=_bn_row, wgrad=_wgrad_row, conv=_conv_row, pool=_pool_row, loss=_loss_row)


@pytest.mark.parametrize('row', ec.OP_ROWS, ids=ec.row_id)
def test_op_row_against_float64(cuda, row):
    worst = _OP[row.kind](_lib.load(), cuda, row)
    flat = worst if row.kind != 'bn' else {'%s %s' % (m, k): v for m, e in worst.items() for k, v in e.items()}
    print('train edges %s: err / bar %s' % (row.name, ', '.join('%s %.3g' % kv for kv in sorted(flat.items()))))


# ---- unit rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', ec.UNIT_ROWS, ids=ec.row_id)
def test_unit_row_against_float64(cuda, row):
    """test_train_gpu.py::test_layer_unit_against_torch's comparison (same reference, same bar, the drop-scale vector given) at the
    frames of UNIT_FRAMES, in both `training` settings"""
    (IC, OC, k, dil, group, slot, act, bn), H, W, training = row.p['shape'], row.p['h'], row.p['w'], row.p['training']
    g = torch.Generator().manual_seed(ec._seed(row.name))
    sign = lambda *s: (torch.randint(0, 2, s, generator=g).double() * 2 - 1) * (torch.rand(*s, generator=g, dtype=torch.float64) + 0.5)
    x = sign(1, IC, H, W).float().double()
    w = (torch.randn(OC, IC, k, k, generator=g, dtype=torch.float64) / np.sqrt(IC * k * k)).float().double()
    b = (torch.randn(OC, generator=g, dtype=torch.float64) * 0.1).float().double()
    gamma = (torch.rand(OC, generator=g, dtype=torch.float64) + 0.5).float().double()
    beta = (torch.randn(OC, generator=g, dtype=torch.float64) * 0.1).float().double()
    rm = (torch.randn(OC, generator=g, dtype=torch.float64) * 0.1).float().double()
    rv = (torch.rand(OC, generator=g, dtype=torch.float64) + 0.5).float().double()
    drop = ((torch.rand(OC, generator=g) < 0.8).double() / 0.8) if act != 'tanh' else None
    dout = (sign(1, OC, H, W) * ec.DOUT_SCALE).float().double()
    scale = 0.7 if act == 'tanh' else 1.0

    xr, wr, br, gr, ber = (t.clone().requires_grad_(True) for t in (x, w, b, gamma, beta))
    rmr, rvr = rm.clone(), rv.clone()
    y = F.conv2d(xr, wr, br, padding=dil * (k // 2), dilation=dil)
    if bn:
        y = F.batch_norm(y, rmr, rvr, gr, ber, training, 0.1, 1e-5)
    y = {'relu': F.relu, 'leaky': lambda t: F.leaky_relu(t, 0.01), 'tanh': torch.tanh, None: lambda t: t}[act](y) * scale
    if drop is not None:
        y = y * drop.view(1, -1, 1, 1)
    y.backward(dout)

    f = lambda t: t.float().to(cuda)
    xs = to_c4(f(slotted(x, group, slot))).requires_grad_(True)
    wp, bp = f(w).requires_grad_(True), f(b).requires_grad_(True)
    gp, bep = (f(gamma).requires_grad_(True), f(beta).requires_grad_(True)) if bn else (None, None)
    bnm = None
    if bn:
        bnm = torch.nn.BatchNorm2d(OC).to(cuda)
        bnm.running_mean.copy_(f(rm)); bnm.running_var.copy_(f(rv))
    meta = dict(group=group, slot=slot, dil=dil, act=act, scale=scale, bn=bnm, drop=f(drop) if drop is not None else None, training=training)
    out = LayerUnit.apply(xs, wp, bp, gp, bep, meta)
    out.backward(to_c4(f(dout)))
    npix = H * W
    c_in_phys, c_out_phys = 4 * xs.shape[0], 4 * out.shape[0]
    plan = ec.wgrad_plan(c_out_phys, c_in_phys, k * k, npix)
    inside = ec.taps_inside(k, dil, H, W)

    def pixel(at):  # (1, channel, y, x) -> where the reductions and the streaming loops put that pixel (unit rows carry no sentinels)
        q = int(at[2]) * W + int(at[3])
        slab, lane, form, it = ec.stats_pixel(npix, q)
        t, sform = ec.stream_pixel(npix, q)
        ws, chunk, wl = ec.wgrad_pixel(plan, q)
        return ('channel %d, pixel (y %d, x %d) = %d: reduction slab %d lane %d %s iteration %d; stream thread %d %s; weight-gradient slab %d '
                'chunk %d lane %d; no sentinel' % (at[1], at[2], at[3], q, slab, lane, form, it, t, sform, ws, chunk, wl))

    def weight(at):
        tap = int(at[2]) * k + int(at[3])
        return 'oc %d (tile %d), ic %d, tap %d (%s the image); %d slabs of %d pixels, %d empty, last %d' % (
            at[0], at[0] // 32, at[1], tap, 'inside' if inside[tap] else 'outside', plan['slabs'], plan['per'], plan['empty'], plan['last_len'])

    def cmp(got, want, what, where=None):  # test_train_gpu.close()'s bar, per element, with the worst element named
        return _check(got.detach().cpu().double().numpy(), want.detach().double().numpy(), '%s %s' % (row.name, what), where, slack=1e-12)
    e = dict(out=cmp(from_c4(out, OC), y, 'out', pixel))
    if out.shape[0] * 4 > OC:  # padding channels stay exactly zero
        assert float(out.detach().permute(0, 3, 1, 2).reshape(-1, H, W)[OC:].abs().max()) == 0
    e['dx'] = cmp(from_c4(xs.grad, xs.shape[0] * 4), slotted(xr.grad, group, slot), 'dx (physical channels)', pixel)
    e['dW'] = cmp(wp.grad, wr.grad, 'dW', weight)
    if bn and training:  # sum of dy vanishes under batch statistics: compare on the scale of the unnormalised sum
        assert float(bp.grad.abs().max()) <= 1e-4 * float(dout.abs().sum() / OC) + 1e-12
    else:
        e['db'] = cmp(bp.grad, br.grad, 'db')
    if bn:
        e['dgamma'] = cmp(gp.grad, gr.grad, 'dgamma')
        e['dbeta'] = cmp(bep.grad, ber.grad, 'dbeta')
        cmp(bnm.running_mean, rmr, 'running_mean')
        cmp(bnm.running_var, rvr, 'running_var')
        assert int(bnm.num_batches_tracked) == (1 if training else 0)
    print('train edges %s: err / bar %s' % (row.name, ', '.join('%s %.3g' % (n, v) for n, v in sorted(e.items()))))


# ---- executor rows ------------------------------------------------------------------------------------------------------------------
def _frame_restated(h, w):
    """what a red executor row prints next to the tensor that failed: how every launch cuts this frame"""
    npix = h * w
    wg = ['%d -> %d %dx%d dil %d x %d units: %d slabs of %d pixels, %d empty, last %d' % ((cip, cop, k, k, dil, units) + tuple(
          ec.wgrad_plan(cop, cip, k * k, npix, units)[n] for n in ('slabs', 'per', 'empty', 'last_len'))) for cop, cip, k, dil, units in ec.EXECUTOR_UNIT_SHAPES]
    s = ec.stats_plan(npix)
    return 'pyramid %r; px_grid %r; reductions: %d slabs of %d pixels, last %d; stream %r; weight gradients: %s' % (
        ec.pyramid_plan(h, w), ec.px_plan(npix), s['nonempty'], s['per'], s['last_len'], ec.stream_plan(npix), '; '.join(wg))


def _split_fp16_against_fp32_backward(cuda, version, sem, h, w):
    """The same forward pass, the backward pass once in the split-fp16 arithmetic (train_wgrad_mfma_kernel<true>, split-fp16 backward-data)
    and once on the fp32-input MFMAs: worst deviation per tensor in units of max(its scale, 1e-3 of the largest gradient), the measure
    and the 2e-5 bar of test_backward_arithmetic_f32_keeps_the_backward_convolutions_on_fp32_mfma.  (Every pass of one trainer runs the
    same arithmetic - dy's factor is derived in the pass itself - so pass 2 against pass 1 can only show non-determinism.)"""
    net = _net(version, sem, h, w).to(cuda).eval()
    x, target = _guard_inputs(cuda, h, w, sem)
    if not sem:
        x.pop('semantic_frame')
    params = [p for p in net.parameters()]
    grads = []
    for tn in (HipTrainNet(net, backward_arithmetic='f32'), HipTrainNet(net)):
        e = tn(x)
        grads.append(torch.autograd.grad((e - target).abs().mean() + 10 * ((e - target) ** 2).mean(), params, allow_unused=True))
    gmax = max(float(a.abs().max()) for a in grads[0] if a is not None)
    worst, name = 0.0, None
    for (n, _), a, b in zip(net.named_parameters(), *grads):
        if a is not None:
            d = float((a - b).abs().max()) / max(float(a.abs().max()), 1e-3 * gmax)
            worst, name = (d, n) if d > worst else (worst, name)
    print('split-fp16 against fp32 backward %s %dx%d: worst deviation %.2e of a tensor\'s scale (%s)' % (version, h, w, worst, name))
    return worst, name


@pytest.mark.parametrize('what', ['f16x3', 'f32', 'second_pass'])
@pytest.mark.parametrize('row', ec.EXECUTOR_ROWS, ids=ec.row_id)
def test_executor_row(cuda, row, what):
    """whole net, eval() mode: the first backward pass in both arithmetics against float64 autograd at _whole_net_gradient_case's bar;
    passes 2 and 3 against pass 1 within 2e-5 (_second_pass_case) and the split-fp16 backward pass against the fp32 one within 2e-5"""
    p = row.p
    try:
        if what == 'second_pass':
            assert _second_pass_case(cuda, p['version'], p['sem'], False, p['h'], p['w']) <= 2e-5
            worst, name = _split_fp16_against_fp32_backward(cuda, p['version'], p['sem'], p['h'], p['w'])
            assert worst <= 2e-5, ('split-fp16 against fp32 backward', name, worst)
        else:
            _whole_net_gradient_case(cuda, p['version'], p['sem'], False, 'executor' if what == 'f16x3' else 'executor_f32', p['h'], p['w'], input_seed=p['input_seed'])
    except AssertionError as err:
        pytest.fail('%s %s: %s\nthis frame: %s' % (row.name, what, err, _frame_restated(p['h'], p['w'])))
