"""-m gpu: the row-pair form of the grouped dilated 3x3 launches (conv_f16x3_rows_kernel, csrc/ojf_net.hip) at the frame sizes where
its pairs reuse rows, straddle two dilation classes, meet band edges and run with and without the persistent walk - beside the sizes
that must keep the old form (odd h, w % 64 != 0, below the band threshold).  Nets, inputs and discipline are those of
tests/test_net_edges_gpu.py: a v3 net of 9 points and growth 5, a NaN-filled 12-wide output, input A, then B, then A again on one
engine; B is compared with the float64 net at the project's bar (|est - ref64| <= 1e-5) and the second A equals the first bit for bit,
in both arithmetics.  The fp32 arithmetic never runs this kernel, so max |est_f16x3 - est_f32| is a second bar: twice the largest
value the parent commit (old form at every size) gave on these sizes and inputs, measured on an MI355X:

    104x256 2.906e-07   98x320 2.719e-07   200x128 2.794e-07   64x192 2.533e-07   105x256 2.906e-07   104x288 2.757e-07   24x32 2.012e-07

so the bar is 5.812e-07 (the row-pair form gave 2.831e-07, 2.906e-07, 2.943e-07 and 2.310e-07 on its four sizes; the other three sizes
keep the parent's figures to the digit).
"""
import pytest
import torch

import net_edge_cases as ec
from net_edge_cases import predict_launches, seeded_row_net, row_inputs, reference64
from test_net_edges_gpu import TOL, SEED_A, SEED_B, _forward, _bits
from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine

pytestmark = pytest.mark.gpu

# max |est_f16x3 - est_f32| of input B on the parent commit, per size (MI355X; printed again by test_f16x3_stays_beside_f32)
PARENT_F16_F32 = {
    'pairs_104x256': 2.906e-07, 'pairs_98x320': 2.719e-07, 'pairs_200x128': 2.794e-07, 'pairs_64x192': 2.533e-07,
    'old_odd_h_105x256': 2.906e-07, 'old_w_288_104x288': 2.757e-07, 'old_unbanded_24x32': 2.012e-07,
}
F16_F32_BAR = 2 * max(PARENT_F16_F32.values())

Size = ec.Row  # (name, version, sem, n_points, growth, h, w, claims): claims = (row-pair form?, persistent at 256 CUs?)


def _size(name, h, w, rows_form, persistent):
    return Size(name, 3, 0, 9, 5, h, w, (rows_form, persistent))


SIZES = [
    _size('pairs_104x256', 104, 256, True, True),      # 208 positions; classes of 4 / 3 rows (r = 27) and 12 / 11 (r = 9): reusing and straddling pairs at both parities
    _size('pairs_98x320', 98, 320, True, True),        # 245 positions, five column groups, classes of 3 and 4 rows
    _size('pairs_200x128', 200, 128, True, True),      # two column groups: band edges inside a pair row
    _size('pairs_64x192', 64, 192, True, False),       # 96 positions: banded, not persistent
    _size('old_odd_h_105x256', 105, 256, False, True),
    _size('old_w_288_104x288', 104, 288, False, True),  # w % 64 != 0, w % 32 == 0
    _size('old_unbanded_24x32', 24, 32, False, False),
]

_CASES = {}    # size name -> (net, input A, input B, float64 reference of B): computed once, never changed
_RESULTS = {}  # (size name, arith) -> (first A, B, second A)


def _case(row):
    if row.name not in _CASES:
        net = seeded_row_net(row)
        xa, xb = row_inputs(row, SEED_A), row_inputs(row, SEED_B)
        ref = reference64(net, xb)
        assert torch.isfinite(ref).all()
        _CASES[row.name] = (net, xa, xb, ref)
    return _CASES[row.name]


def _result(row, arith, cuda):
    if (row.name, arith) not in _RESULTS:
        net, xa, xb, _ = _case(row)
        eng = FusionNetEngine(net, row.h, row.w, cuda, arithmetic=arith)
        out = tuple(_forward(eng, row, x, cuda) for x in (xa, xb, xa))
        eng.check()
        eng.close()
        _RESULTS[(row.name, arith)] = out
    return _RESULTS[(row.name, arith)]


def _grouped(row, arith, cus):
    return [l for l in predict_launches(row.version, row.sem, row.n_points, row.growth, row.h, row.w, arith, cus) if l['name'] == ec.GROUPED]


def rows_form(launch, h, w):
    """launch_conv_args' choice for a grouped launch of the branches' 19 -> 19 3x3 (split planes in, 9 taps, five channel groups)"""
    return bool(launch['nblocks'] and launch['mt'] == 2 and launch['nt'] == 2 and launch['lean'] and w % 64 == 0 and h % 2 == 0)


def test_sizes_get_their_forms_on_this_device(cuda):
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    wrong = {}
    for r in SIZES:
        launches = _grouped(r, 'f16x3', cus)
        assert len(launches) == 4 and not _grouped(r, 'f32', cus)
        for l in launches:
            got = (rows_form(l, r.h, r.w), bool(l['band']))
            if got != r.claims:
                wrong[r.name] = (got, r.claims)
            if got[0]:
                assert l['nblocks'] == (r.h // 2) * (r.w // 64)
    assert not wrong, 'with %d CUs (row-pair form, persistent) is not what the table claims: %s' % (cus, wrong)


@pytest.mark.parametrize('arith', ['f16x3', 'f32'])
@pytest.mark.parametrize('row', SIZES, ids=ec.row_id)
def test_size_against_the_float64_net(cuda, row, arith):
    ref = _case(row)[3]
    p = row.n_points
    a1, b, a2 = _result(row, arith, cuda)
    fill = _bits(torch.full((1,), float('nan')))[0]
    for got in (a1, b, a2):
        assert torch.all(_bits(got[:, p:]) == fill), 'columns behind the points were written'
        assert torch.isfinite(got[:, :p]).all()
    diff = (b[:, :p].double() - ref).abs()
    err = float(diff.max())
    print('grouped rows %s %s: max err %.2e = %.3f of the bar' % (row.name, arith, err, err / TOL))
    if err > TOL:
        at = int(diff.max(dim=1).values.argmax())
        y, x = divmod(at, row.w)
        pytest.fail('%s %s: max err %.3e at pixel (y %d, x %d), %d of %d pixels beyond 1e-5'
                    % (row.name, arith, err, y, x, int((diff.max(dim=1).values > TOL).sum()), row.h * row.w))
    assert torch.equal(_bits(a1), _bits(a2)), 'the second pass over input A differs from the first'
    assert not torch.equal(a1[:, :p], b[:, :p])


@pytest.mark.parametrize('row', SIZES, ids=ec.row_id)
def test_f16x3_stays_beside_f32(cuda, row):
    p = row.n_points
    d = float((_result(row, 'f16x3', cuda)[1][:, :p].double() - _result(row, 'f32', cuda)[1][:, :p].double()).abs().max())
    print('grouped rows %s: max |est_f16x3 - est_f32| = %.3e (parent %.3e, bar %.3e)' % (row.name, d, PARENT_F16_F32[row.name], F16_F32_BAR))
    assert d <= F16_F32_BAR
