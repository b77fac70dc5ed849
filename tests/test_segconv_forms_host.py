"""segconv_form_cases.py on the CPU: every table row predicts the kernel form it names, the rows reach every non-dropout
form of the SEGCONV dispatcher (csrc/ojf_seg.hip) at every listed edge, the restated form choice agrees with the forms the
dropout table records, and no input reached the removed ``wide<2>`` branch of the former dispatcher."""
import re
import os

import numpy as np

import segconv_form_cases as fc
from segconv_form_cases import FORM_TABLE, DECONV_TABLE, MULTI_TABLE, predict_form, predict_multi, row_edges


def test_restated_constants_are_the_dispatchers():
    """The named constants of segconv_form_cases.py are read back from ojf_seg.hip."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'online_joint_depthfusion_and_semantic_amd', 'csrc', 'ojf_seg.hip')).read()
    names = {'kMW': fc.K_MW, 'kPlainMinWaves': fc.PLAIN_MIN_WAVES, 'kSplitKMinKb': fc.SPLITK_MIN_KB, 'kSplitKMinBlocks': fc.SPLITK_MIN_BLOCKS,
             'kNw2MinKb': fc.NW2_MIN_KB, 'kNw2MaxBlocks': fc.NW2_MAX_BLOCKS, 'kPlainNw1Min': fc.PLAIN_NW1_MIN, 'kGemmMin': fc.GEMM_MIN,
             'kGemm22Min': fc.GEMM22_MIN, 'kGemmMinKb': fc.GEMM_MIN_KB, 'kMultiOwnMinKb': fc.MULTI_OWN_MIN_KB, 'kMultiOwnMinBlocks': fc.MULTI_OWN_MIN_BLOCKS}
    for name, value in names.items():
        m = re.search(r'constexpr int %s = (\d+);' % name, src)
        assert m and int(m.group(1)) == value, name
    # every segconv_kernel instantiation the dispatcher launches has kDepth 3
    depths = set(re.findall(r'segconv_kernel<\d, \d, \d, \d, (\d)', src))
    assert depths == {str(fc.K_DEPTH)}, depths
    assert 'segconv_wide' not in src and 'wide<' not in src


def test_every_row_predicts_the_form_it_names():
    names = [r[0] for r in FORM_TABLE + DECONV_TABLE] + [r[0] for r in MULTI_TABLE]
    assert len(set(names)) == len(names)
    for row in FORM_TABLE:
        assert len(row) == 12 and predict_form(*row[1:11]).form == row[11], row[0]
    for row in DECONV_TABLE:
        assert len(row) == 13 and predict_form(*row[1:11], deconv_stride=row[12]).form == row[11], row[0]
    for name, members, form in MULTI_TABLE:
        assert predict_multi(members).form == form, name


def test_tables_cover_every_form():
    assert {r[11] for r in FORM_TABLE} == set(fc.ALL_FORMS)
    assert {r[2] for r in MULTI_TABLE} == set(fc.MULTI_FORMS) | {'separate'}
    # transposed convolutions: strides 2, 4 and 8, batch 2, a plain form, a split-K form and a GEMM tile, c_out no multiple of 4
    assert {r[12] for r in DECONV_TABLE} == {2, 4, 8} and any(r[9] == 2 for r in DECONV_TABLE)
    forms = {r[11] for r in DECONV_TABLE}
    assert forms & set(fc.PLAIN_FORMS) and forms & set(fc.SPLITK_FORMS) and forms & set(fc.GEMM_FORMS)
    assert all(r[2] % 4 for r in DECONV_TABLE)
    # heterogeneous lists: members of different pixel and channel counts; the mixed list holds both kinds of member
    for name, members, form in MULTI_TABLE:
        geo = [fc.geometry(*m[:8], 1) for m in members]
        assert len({g.n_pt for g in geo}) > 1 and len({g.n_ct for g in geo}) > 1, name
        if form != 'separate':
            # blocks that must exit: the 1-D grid is larger than the members' own blocks
            own = sum(xy[0] * xy[1] for _, xy in predict_multi(members).maps)
            assert predict_multi(members).total > own, name
    mixed = predict_multi(dict((r[0], r[1]) for r in MULTI_TABLE)['multi_mixed']).groups
    assert {p.form in fc.SPLITK_FORMS for p in mixed} == {True, False}
    large = predict_multi(dict((r[0], r[1]) for r in MULTI_TABLE)['multi_large_pair']).groups
    assert [p.form in fc.GEMM_FORMS for p in large] == [True, False] and large[0].grid[2] == 2


def test_rows_carry_every_listed_edge():
    """Computed from the rows' numbers (row_edges), not asserted by hand."""
    per_form = {}
    for row in FORM_TABLE:
        per_form.setdefault(row[11], set()).update(row_edges(row))
    for form in fc.PLAIN_FORMS + fc.SPLITK_FORMS:
        assert not [e for e in fc.EDGES_PER_FORM if e not in per_form[form]], (form, [e for e in fc.EDGES_PER_FORM if e not in per_form[form]])
    for form in fc.IDLE_WAVE_FORMS:
        assert 'idle split-K wave' in per_form[form], form
    for form in fc.GEMM_FORMS:
        assert not [e for e in fc.EDGES_PER_GEMM_FORM if e not in per_form[form]], form
    # both tap walks of segconv_gemm_kernel (ALIGNED: c8 a multiple of 4) run the unaligned epilogue
    assert {fc.geometry(*r[1:10]).c8 % 4 == 0 for r in FORM_TABLE if r[11] in fc.GEMM_FORMS} == {True, False}
    everywhere = set().union(*per_form.values())
    assert not [e for e in fc.EDGES_ANYWHERE if e not in everywhere]
    # <4,2,1,4> cannot have an idle wave: it needs 32 K blocks, and with n_kb > 9 every wave owns some
    assert all(3 * fc.cdiv(n_kb, 4) < n_kb for n_kb in range(fc.NW2_MIN_KB, 4096))
    # the examples of the edges: 45 entries leave one in the last block, 9 K blocks leave wave 3 idle, 70 channels pad n_ct
    assert any(fc.geometry(*r[1:10]).entries % 4 == 1 for r in FORM_TABLE)
    assert any(fc.geometry(*r[1:10]).n_kb == 9 for r in FORM_TABLE if r[11] in fc.SPLITK_FORMS)
    assert {5, 30, 37, 70} <= {r[2] for r in FORM_TABLE}


def test_placements_clear_every_vec_store_bit():
    """Placement (b) of the GPU test: output only, residual only, gate only, all three - for every c_out of the tables;
    both kinds of misalignment occur on the output, the residual and the gate rows."""
    for kind, (lo, extra) in fc.SLICE_KINDS.items():
        for c in range(1, 80):
            first, cb = fc.slice_geometry(kind, c)
            assert cb - (first + c) >= 4 and fc.rows_aligned(kind, c) == (kind == 'aligned')
            assert (kind == 'stride') == (cb % 4 != 0)
    for c in {r[2] for r in FORM_TABLE}:
        cleared = [fc.cleared_bits(p, c) for p in fc.PLACEMENTS]
        assert {1, 2, 4, 7} <= set(cleared), (c, cleared)
    for column in (1, 2, 3):
        kinds = {p[column] for p in fc.PLACEMENTS}
        assert 'stride' in kinds and kinds & {'ptr1', 'ptr3'}, column
    assert {p[1] for p in fc.DECONV_PLACEMENTS} >= {'ptr1', 'stride'}


def test_prediction_agrees_with_the_dropout_table():
    """The forms test_segconv_dropout_gpu.py's TABLE records (and proves from its trace) for the launches WITHOUT dropout:
    where a row is marked bit-exact the plain launch takes the row's form, elsewhere another one."""
    import test_segconv_dropout_gpu as d
    for row in d.TABLE:
        form, same = row[11], row[12]
        plain = predict_form(*row[1:11]).form
        assert (plain == form.replace(' drop', '')) == same, (row[0], plain)
        if form.startswith('gemm'):
            assert plain == form


def test_hetero_cases_of_the_existing_test_predict_one_launch_each():
    import test_segconv_gpu as t
    for i, members in enumerate(t.HETERO_CASES):
        spec = [(cin, cout, k, s, 1, k // 2) + t.HETERO_INPUTS[key][1:] + ((act, gated),) for cin, cout, k, s, key, act, gated in members]
        form = predict_multi(spec).form
        assert (form == 'separate') == (i == len(t.HETERO_CASES) - 1), (i, form)


def test_no_input_reached_the_removed_wide_form():
    """The former dispatcher tried the GEMM-shaped branch first; its condition follows from the wide branch's
    (n_kb >= 6 >= 4, groups * ceil(n_pt / 4) * n >= groups * ceil(n_pt / 8) * n >= 256 >= 128).  Enumerated as well."""
    n_pt = np.arange(1, 3000, dtype=np.int64)[None, :]
    groups = np.arange(1, 40, dtype=np.int64)[:, None]
    for n in (1, 2, 8):
        for n_kb in range(1, 200):
            assert not fc.former_wide_branch_taken(n_kb, groups, n_pt, n).any(), (n_kb, n)
    # the shapes whose comments named that kernel take GEMM-shaped forms
    import test_segconv_gpu as t
    for shape in t.SHAPES[-5:]:
        assert predict_form(*shape, 1, 1).form in fc.GEMM_FORMS, shape
    assert predict_form(3, 64, 7, 2, 1, 3, 240, 320, 1, 2).form in fc.GEMM_FORMS
