"""CPU: the non-cubic box cases of box_cases.py can tell the axes apart.  Through the oracle, render_ref and track_ref
alone: the boxes are hit where they should be, and an origin component taken from the wrong axis or exchanged Y / Z
strides would change more than a tenth of the touched voxels - so the GPU tests on the same inputs (test_box_gpu.py)
cannot pass with such an error.  The conditions here are what the references alone satisfy."""
import numpy as np
import pytest

from oracle import oracle
from helpers import n_mismatch, make_stream, frame_inputs
import box_cases
from box_cases import BOXES, FRAME_SIZES, box, oracle_run, render_reference

MIN_TOUCHED = {'room': 3000, 'slab': 1000}


def _differs(a, b):
    """Voxels whose TSDF or weight bits differ."""
    bad = np.zeros(a['wgt'].shape, bool)
    for key in ('tsdf', 'wgt'):
        x, y = a[key], b[key]
        bad |= (x.view(np.uint16) != y.view(np.uint16)) & ~(np.isnan(x) & np.isnan(y))
    return bad


@pytest.mark.parametrize('h,w', FRAME_SIZES)
@pytest.mark.parametrize('name', sorted(BOXES))
def test_boxes_are_hit(name, h, w):
    origin, res, shape = box(name)
    run = oracle_run(name, h, w)
    assert [r['i'] for r in run] == list(BOXES[name]['frames'])
    touched = [r['touched'] for r in run]
    print('%s %dx%d: touched per frame %s' % (name, h, w, touched))
    assert sum(touched) >= MIN_TOUCHED[name], touched
    written = run[-1]['post']['wgt'] > 0
    assert written.shape == shape and len(set(shape)) == 3 and len(set(origin)) == 3
    if name == 'room':
        faces = [written[0], written[-1], written[:, 0], written[:, -1], written[:, :, 0], written[:, :, -1]]
        hit = [bool(f.any()) for f in faces]
        print('room %dx%d: faces x0 x1 y0 y1 z0 z1 written %s' % (h, w, hit))
        assert sum(hit) >= 4, hit
    else:
        fi = run[0]['fi']
        ex = oracle.extract(fi['depth'], fi['Ki'], fi['E'], origin, res, run[0]['pre']['tsdf'], run[0]['pre']['wgt'], debug=True)
        inside = ((ex['indices'] >= 0) & (ex['indices'] < np.array(shape))).all(axis=-1).reshape(h * w, -1)
        outside = ~inside.any(axis=1)
        partly = inside.any(axis=1) & ~inside.all(axis=1)
        print('slab %dx%d frame 0: %.0f %% of rays fully outside, %d partly inside' % (h, w, 100 * outside.mean(), partly.sum()))
        assert outside.mean() >= 0.5 and partly.sum() > 0


def test_semantics_do_not_move_the_geometry():
    """oracle_run integrates with semantics; the TSDF and weight volumes are those of a run without."""
    name, (h, w) = 'slab', FRAME_SIZES[1]
    origin, res, shape = box(name)
    run = oracle_run(name, h, w)
    vols = {k: v.copy() for k, v in run[0]['pre'].items() if k in ('tsdf', 'wgt')}
    for r in run:
        fi = r['fi']
        assert oracle.integrate(fi['fd'], fi['Ki'], fi['E'], origin, res, fi['est'], vols['tsdf'], vols['wgt']) == r['touched']
        assert n_mismatch(vols['tsdf'], r['post']['tsdf']) == 0 and n_mismatch(vols['wgt'], r['post']['wgt']) == 0


@pytest.mark.parametrize('h,w', FRAME_SIZES)
@pytest.mark.parametrize('name', sorted(BOXES))
def test_a_rotated_origin_is_seen(name, h, w):
    """The origin's components rotated to (o1, o2, o0): more than 10 % of the true run's touched voxels change."""
    origin, _, _ = box(name)
    true = oracle_run(name, h, w)[-1]['post']
    wrong = oracle_run(name, h, w, origin=(origin[1], origin[2], origin[0]))[-1]['post']
    touched = int((true['wgt'] > 0).sum())
    moved = int(_differs(true, wrong).sum())
    print('%s %dx%d: rotated origin changes %d voxels, %d touched' % (name, h, w, moved, touched))
    assert moved > 0.1 * touched


@pytest.mark.parametrize('h,w', FRAME_SIZES)
@pytest.mark.parametrize('name', sorted(BOXES))
def test_exchanged_strides_are_seen(name, h, w):
    """The true volume's flat buffer read as (X, Z, Y) and transposed back: more than 10 % of the touched voxels change."""
    X, Y, Z = box(name)[2]
    true = oracle_run(name, h, w)[-1]['post']
    wrong = {k: np.ascontiguousarray(true[k].reshape(-1).reshape(X, Z, Y).transpose(0, 2, 1)) for k in ('tsdf', 'wgt')}
    touched = int((true['wgt'] > 0).sum())
    moved = int((_differs(true, wrong) & (true['wgt'] > 0)).sum())
    print('%s %dx%d: exchanged strides change %d of %d touched voxels' % (name, h, w, moved, touched))
    assert moved > 0.1 * touched


def test_render_cases_in_the_restatement():
    box_cases.check_render_conditions(render_reference)
    d = box_cases.axis_ray_components()
    # world axes with an exactly zero ray component: view 0 x on column 26 / y on row 18, view 1 y / z, views 2 and 3 x / z
    for v, (col_axis, row_axis) in enumerate([(0, 1), (1, 2), (0, 2), (0, 2)]):
        assert not d[v, :, 26, col_axis].any() and not d[v, 18, :, row_axis].any()
        assert d[v, :, 25, col_axis].all() and d[v, 17, :, row_axis].all()
    for tag in ('gt-near0', 'gt-near1.5', 'holes-near0', 'holes-near1.5', 'axis', 'thin'):
        depth, normals, _ = render_reference(tag)
        print('render %s: hits per view %s, normals non-zero on %.0f %%' % (
            tag, np.round((depth > 0).mean(axis=(1, 2)), 2).tolist(), 100 * normals.any(axis=-1).mean()))


@pytest.mark.parametrize('h,w', box_cases.TRACK_SIZES)
def test_tracker_cases_in_the_restatement(h, w):
    from render_ref import render_ref
    origin, res, _ = box('room')
    tsdf = box_cases.room_gt(box_cases.RENDER_TRUNC)[0]

    def render(K, E, shape):
        d, n, _ = render_ref(tsdf, None, None, origin, res, K, E, shape)
        return d[0], n[0]
    case = box_cases.track_case(h, w, render)
    levels = box_cases.track_restatement(case)
    assert [lv['D'].shape for lv in levels] == [(h >> l, w >> l) for l in range(3)]
    assert (h >> 1) * 2 < h or (w >> 1) * 2 < w  # a row or a column is dropped on the way down
    inliers = [int((lv['reason'] == 0).sum()) for lv in levels]
    codes = [lv['code'] for lv in levels]
    print('track %dx%d: inliers %s, solve codes %s' % (h, w, inliers, codes))
    assert all(n >= 0.05 * lv['D'].size for n, lv in zip(inliers, levels))
    assert codes == [0, 0, 2]  # level 2 is degenerate in the restatement: the kernel must say the same
