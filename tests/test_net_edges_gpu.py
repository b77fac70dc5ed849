"""-m gpu: the fusion net's forward kernels at their tile, band and frame edges.  Every row of tests/net_edge_cases.py::EDGE_ROWS runs
in both arithmetics against the float64 net (copy.deepcopy(net).double() on the inputs widened to float64; computed once per row and
shared) at the project's own bar, |est - ref64| <= 1e-5; tests/test_net_edges_host.py holds the fp32 CPU net - the
reference of the older tests - within 1e-6 of it.  One engine runs input A, input B, then A again: B is the one compared, so a pixel
that a launch never wrote holds A's value and not a lucky one, and the second A must repeat the first bit for bit.  The output buffer
is NaN-filled and 12 floats wide: the columns behind the net's points keep their bits.  A failing row names its worst pixel and the
edges of the predicted launches that pixel falls into.  The OJF_NET_TRACE lines of a child process must equal predict_launches for the
device's CU count, and on a device with another CU count than 256 the rows that no longer reach their edges fail by name."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import net_edge_cases as ec
import net_plan_cases
from net_edge_cases import EDGE_ROWS, predict_launches, seeded_row_net, row_inputs, reference64
from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine

pytestmark = pytest.mark.gpu
TOL = 1e-5
SEED_A, SEED_B = 1, 7
WIDTH = 12

_CASES = {}  # row name -> (net, input A, input B, float64 reference of B): computed once, shared by both arithmetics, never changed


def _case(row):
    if row.name not in _CASES:
        net = seeded_row_net(row)
        xa, xb = row_inputs(row, SEED_A), row_inputs(row, SEED_B)
        ref = reference64(net, xb)
        assert torch.isfinite(ref).all() and int((ref.abs() > 0.99 * net.scale).sum()) == 0, row.name
        _CASES[row.name] = (net, xa, xb, ref)
    return _CASES[row.name]


def _forward(eng, row, x, cuda):
    """-> the whole [npix, WIDTH] output buffer of one forward pass, NaN-filled before"""
    n, p = row.h * row.w, row.n_points
    fv = x['tsdf_values'][0].permute(1, 2, 0).reshape(n, p).contiguous().to(cuda)
    fw = x['tsdf_weights'][0].permute(1, 2, 0).reshape(n, p).contiguous().to(cuda)
    eng.prepare_input(fv, fw, x['tsdf_frame'].reshape(row.h, row.w).contiguous().to(cuda),
                      x['sem_ids'].contiguous().to(cuda) if row.sem else None, 30)
    est = torch.full((n, WIDTH), float('nan'), device=cuda)
    eng.forward(est)
    return est.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('arith', ['f16x3', 'f32'])
@pytest.mark.parametrize('row', EDGE_ROWS, ids=ec.row_id)
def test_row_against_the_float64_net(cuda, row, arith):
    net, xa, xb, ref = _case(row)
    p = row.n_points
    eng = FusionNetEngine(net, row.h, row.w, cuda, arithmetic=arith)
    a1, b, a2 = (_forward(eng, row, x, cuda) for x in (xa, xb, xa))
    eng.check()
    eng.close()
    fill = _bits(torch.full((1,), float('nan')))[0]
    for got in (a1, b, a2):
        assert torch.all(_bits(got[:, p:]) == fill), 'columns behind the points were written'
        assert torch.isfinite(got[:, :p]).all()
    diff = (b[:, :p].double() - ref).abs()
    err = float(diff.max())
    print('net edges %s %s: max err %.2e = %.3f of the bar' % (row.name, arith, err, err / TOL))
    if err > TOL:
        at = int(diff.max(dim=1).values.argmax())
        y, x = divmod(at, row.w)
        cus = torch.cuda.get_device_properties(cuda).multi_processor_count
        items = ec.pixel_items(predict_launches(row.version, row.sem, p, row.growth, row.h, row.w, arith, cus), row.h, row.w, y, x)
        bad = int((diff.max(dim=1).values > TOL).sum())
        pytest.fail('%s %s: max err %.3e at pixel (y %d, x %d), %d of %d pixels beyond 1e-5; that pixel lies in: %s'
                    % (row.name, arith, err, y, x, bad, row.h * row.w, '; '.join(items) or 'no edge of any launch'))
    assert torch.equal(_bits(a1), _bits(a2)), 'the second pass over input A differs from the first'
    assert not torch.equal(a1[:, :p], b[:, :p])


def test_rows_reach_their_edges_on_this_device(cuda):
    """The coverage claims are computed for 256 CUs (tests/test_net_edges_host.py).  The CU count moves the persistent form's
    threshold and the chain kernel's grid: on another device the rows that no longer reach their edges are named - and fail."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    lost = {}
    for r in EDGE_ROWS:
        got = ec.reached(r.version, r.sem, r.n_points, r.growth, r.h, r.w, cus=cus)
        missing = [c for c in r.claims if c not in got]
        if missing:
            lost[r.name] = missing
    assert not lost, 'with %d CUs these rows no longer reach: %s' % (cus, lost)


_TRACE_SCRIPT = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import net_edge_cases as ec
import test_net_edges_gpu as t
dev = torch.device('cuda:0')
rows = {r.name: r for r in ec.EDGE_ROWS}
for name in sys.argv[2:]:
    row = rows[name]
    net = ec.seeded_row_net(row)
    x = ec.row_inputs(row)
    for arith in ('f16x3', 'f32'):
        eng = t.FusionNetEngine(net, row.h, row.w, dev, arithmetic=arith)
        torch.cuda.synchronize()
        os.write(2, ('BEGIN %s %s\n' % (name, arith)).encode())
        t._forward(eng, row, x, dev)
        eng.check()
        os.write(2, ('END %s %s\n' % (name, arith)).encode())
        eng.close()
"""

_CHUNKS = [EDGE_ROWS[i:i + 4] for i in range(0, len(EDGE_ROWS), 4)]  # a child process per four rows: a second or two each
_CHILD_TIMEOUT = 90  # seconds: a hang is a quick failure


@pytest.mark.parametrize('rows', _CHUNKS, ids=lambda rows: rows[0].name + '..' + rows[-1].name)
def test_trace_equals_the_prediction(cuda, rows):
    """OJF_NET_TRACE=1 is read once per process: a child process per group of rows, without the three test-only switches.  The lines
    of every forward pass equal predict_launches for this device's CU count, field by field."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in net_plan_cases.SWITCH_PLANS and k != 'OJF_NET_GRAPH'}
    env['OJF_NET_TRACE'] = '1'
    out = subprocess.run([sys.executable, '-c', _TRACE_SCRIPT, root] + [r.name for r in rows], env=env, capture_output=True, text=True, timeout=_CHILD_TIMEOUT)
    assert out.returncode == 0, out.stderr[-3000:]
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    passes, cur = {}, None
    for line in out.stderr.splitlines():
        if line.startswith('BEGIN '):
            cur = tuple(line.split()[1:])
            passes[cur] = []
        elif line.startswith('END '):
            cur = None
        elif cur is not None:
            passes[cur].append(line)
    for r in rows:
        for arith in ('f16x3', 'f32'):
            traced = ec.parse_trace('\n'.join(passes[(r.name, arith)]))
            want = predict_launches(r.version, r.sem, r.n_points, r.growth, r.h, r.w, arith, cus)
            assert len(traced) == len(want), (r.name, arith, [l['name'] for l in traced], [l['name'] for l in want])
            for i, (a, b) in enumerate(zip(traced, want)):
                assert a == b, (r.name, arith, i, a, b)


def test_trace_is_silent_when_unset(cuda):
    """With OJF_NET_TRACE unset this process prints no trace line (the variable is read once per process: checked in a child)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != 'OJF_NET_TRACE'}
    out = subprocess.run([sys.executable, '-c', _TRACE_SCRIPT, root, 'below_a_tile'], env=env, capture_output=True, text=True, timeout=_CHILD_TIMEOUT)
    assert out.returncode == 0, out.stderr[-3000:]
    assert 'BEGIN below_a_tile f32' in out.stderr and not ec.parse_trace(out.stderr)
