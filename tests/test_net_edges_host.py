"""net_edge_cases.py without a GPU: the restated constants are the source's, every row of EDGE_ROWS reaches the edges it claims (computed
from predict_launches at 256 CUs, never asserted by hand), the frame sizes of the older net tests reach none of the listed ones,
ojf_net_plan names the launches the restatement implies, and the references of the small rows are sound: the float64 net is finite
and unsaturated, and the fp32 CPU net (the reference of the older tests) is within 1e-6 of it - the 1e-5 bar of the GPU test is more
than ten times the reference's own noise."""
import os
import re

import pytest
import torch

import net_edge_cases as ec
from net_edge_cases import EDGE_ROWS, predict_launches, reached, seeded_row_net, row_inputs, reference64
from online_joint_depthfusion_and_semantic_amd import model
from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'online_joint_depthfusion_and_semantic_amd', 'csrc')


def test_restated_constants_are_the_launch_sites():
    net = open(os.path.join(CSRC, 'ojf_net.hip')).read()
    conv = open(os.path.join(CSRC, 'ojf_net_conv.h')).read()  # what the net shares with the training unit
    chain = open(os.path.join(CSRC, 'ojf_net_chain.h')).read()
    common = open(os.path.join(CSRC, 'ojf_common.h')).read()

    def const(src, name):
        m = re.search(r'constexpr int [^;]*\b%s = (\d+)[,;]' % name, src)
        assert m, name
        return int(m.group(1))

    assert (const(net, 'kPoolTW'), const(net, 'kPoolTH')) == (ec.POOL_TW, ec.POOL_TH)
    assert const(net, 'persist_bpc') == ec.PERSIST_BPC
    assert const(net, 'kChainWaves') == ec.CHAIN_WAVES
    assert const(net, 'kSumBlocks') == ec.SUM_BLOCKS
    assert const(conv, 'kNT') == ec.K_NT
    assert (const(chain, 'kChainNG'), const(chain, 'kChainMaxLayers')) == (ec.CHAIN_NG, ec.CHAIN_MAX_LAYERS)
    assert 'kChainSyncInts = kChainFlags0 + %d;' % ec.CHAIN_MAX_TILES in net
    # the banding threshold and the superstep chunk of launch_conv_args
    assert 'arith == OJF_ARITH_F16X3 && grid.x >= %d)' % ec.BAND_MIN_BLOCKS in net
    assert 'constexpr int conv16_chunk(int nt) { return nt <= 2 ? %d : %d; }' % (ec.conv16_chunk(2), ec.conv16_chunk(4)) in net
    # one tile rule in three places: launch_chain, pair_cfg_for, chain_dense_form
    rule = r'\(\(s?\.?w \+ %d\) / %d\) \* \(\(s?\.?h \+ %d\) / %d\)' % (ec.BIG_TILE[0] - 1, ec.BIG_TILE[0], ec.BIG_TILE[1] - 1, ec.BIG_TILE[1])
    assert len(re.findall(rule, net)) == 3
    assert len(re.findall(r'>= %d\b' % ec.BIG_TILE_MIN, net)) == 3
    assert 'launch_chain_t<%d, %d, 16>' % ec.BIG_TILE in net and 'launch_chain_t<%d, %d, 8>' % ec.SMALL_TILE in net
    assert 'launch_pair_t<%d, %d>' % ec.BIG_TILE in net and 'launch_pair_t<%d, %d>' % ec.SMALL_TILE in net
    assert 's.npix < %d ? BRANCH_GROUPED' % ec.SIDE0_MIN_NPIX in net
    # the pyramid: three pooling levels = the halo; XCD bands of 8
    assert 'lv = yg < 3 ? 3 - yg : 4' in net and ec.POOL_HALO == 3
    assert '(b & 7) * (n8 >> 3) + (b >> 3)' in common and '(gridDim.x & 7) == 0' in common and ec.XCDS == 8
    assert ec.DILATIONS == tuple(model.VortexPooling.rates)


def test_every_row_reaches_what_it_claims():
    names = [r.name for r in EDGE_ROWS]
    assert len(set(names)) == len(names)
    for r in EDGE_ROWS:
        got = reached(r.version, r.sem, r.n_points, r.growth, r.h, r.w)
        missing = [c for c in r.claims if c not in got]
        assert not missing, (r.name, missing, sorted(got))
        assert r.h * r.w <= ec.MAX_ROW_PIXELS, r.name


def test_rows_reach_every_listed_edge():
    everywhere = set()
    for r in EDGE_ROWS:
        everywhere |= reached(r.version, r.sem, r.n_points, r.growth, r.h, r.w)
    assert not [e for e in ec.EDGES_ANYWHERE if e not in everywhere]
    assert not [e for e in ec.NOT_REACHED_BY_OLD_SIZES if e not in everywhere]
    # the numbers the issue's table names
    by = {r.name: predict_launches(r.version, r.sem, r.n_points, r.growth, r.h, r.w, 'f16x3', 256) for r in EDGE_ROWS}
    grouped = {k: [l for l in v if l['name'] == ec.GROUPED][0] for k, v in by.items()}
    assert (grouped['band_threshold_63']['grid_x'], grouped['band_threshold_63']['nblocks']) == (63, 0)
    assert (grouped['band_threshold_64']['grid_x'], grouped['band_threshold_64']['nblocks']) == (64, 64)
    assert grouped['band_threshold_64']['perm'] == '0:0:0,3:42:1,9:14:1,27:4:19'
    assert grouped['perm_mixed_27']['perm'] == '0:0:0,3:9:0,9:3:0,0:0:0' and grouped['perm_mixed_28']['perm'].endswith('27:1:1')
    assert (grouped['banded_ragged']['nblocks'], grouped['banded_ragged']['band'], grouped['banded_ragged']['grid16_x']) == (69, 0, 72)
    for name, nblocks in (('persist_perm_ragged', 194), ('persist_perm_193', 193), ('persist_plain_ragged_8', 196), ('persist_plain_ragged_56', 196)):
        g = grouped[name]
        assert (g['nblocks'], g['band'], g['grid16_x']) == (nblocks, 25, 192), name
    chain = {k: [l for l in v if l['name'] == ec.CHAIN] for k, v in by.items()}
    assert chain['chain_big_threshold_198'][0]['tiles'] == 2 * 198 and chain['chain_big_threshold_200'][0]['tiles'] == 200
    assert chain['chain_big_two_heads'][0]['tiles'] == 224 and len(chain['chain_big_two_heads']) == 2
    # both arithmetics of every row run the same entry, tail and pyramid launches
    shared = (ec.ENTRY, ec.PYRAMID) + ec.TAILS
    for r in EDGE_ROWS:
        f32 = predict_launches(r.version, r.sem, r.n_points, r.growth, r.h, r.w, 'f32', 256)
        assert [l for l in f32 if l['name'] in shared] == [l for l in by[r.name] if l['name'] in shared], r.name
        assert {l['name'] for l in f32} <= set(shared) | {ec.CONV32, ec.COLSUM, ec.GAVE}


def test_the_older_frame_sizes_reach_none_of_them():
    """Why the table exists: what the frame sizes of test_fusion_net_forward, the headline test and test_fusion_net_other_topologies
    reach, against the list of edges only the new rows reach."""
    old = set()
    for net in ec.OLD_NETS:
        for h, w in ec.OLD_SIZES:
            old |= reached(net[0], net[1], net[2], net[3], h, w)
    for net, (h, w) in ec.OLD_TOPOLOGIES:
        old |= reached(net[0], net[1], net[2], net[3], h, w)
    assert not [e for e in ec.NOT_REACHED_BY_OLD_SIZES if e in old]
    # what they do reach: the persistent form only with whole bands, the permutation only with whole pixel blocks
    assert {'persistent with permutation', 'row_perm with perm_rem == 0', 'row_perm with perm_rem != 0', 'chain tile 20x16',
            'chain tile 12x8', 'pair tile 12x8', 'general flow'} <= old


@pytest.mark.parametrize('arith', ['f16x3', 'f32'])
def test_plan_names_what_the_restatement_implies(arith):
    for r in EDGE_ROWS:
        plan = FusionNetEngine.plan(r.version, r.n_points, r.growth, r.sem, r.h, r.w, arith)
        assert plan == [l['name'] for l in predict_launches(r.version, r.sem, r.n_points, r.growth, r.h, r.w, arith, 256)], r.name
    import net_plan_cases
    for case, names in net_plan_cases.PLANS.items():  # and the recorded table of the plan
        version, sem, n_points, growth, h, w, a = case
        assert [l['name'] for l in predict_launches(version, sem, n_points, growth, h, w, a, 256)] == names, case


def test_trace_line_round_trip():
    launches = predict_launches(3, 1, 9, 5, 155, 160, 'f16x3', 256)
    text = ''.join('ojf_net %s | %s\n' % (l['name'], ' '.join('%s %s' % kv for kv in l.items() if kv[0] != 'name')) for l in launches)
    assert ec.parse_trace('noise\n' + text) == launches


def test_failure_message_helper_works_on_every_row():
    """pixel_items runs only when a GPU row is red: here on the corners, the centre and the last pixel block of every row, in both
    arithmetics, so that a failing row gets its diagnostic and not a traceback."""
    for r in EDGE_ROWS:
        for arith in ('f16x3', 'f32'):
            launches = predict_launches(r.version, r.sem, r.n_points, r.growth, r.h, r.w, arith, 256)
            for y, x in {(0, 0), (0, r.w - 1), (r.h - 1, 0), (r.h - 1, r.w - 1), (r.h // 2, r.w // 2)}:
                items = ec.pixel_items(launches, r.h, r.w, y, x)
                assert all(isinstance(i, str) and i for i in items), (r.name, arith, y, x)
    # what a red persistent row prints: the last position of an XCD's band, walked in a block's second step
    r = {r.name: r for r in EDGE_ROWS}['persist_perm_193']
    launches = predict_launches(r.version, r.sem, r.n_points, r.growth, r.h, r.w, 'f16x3', 256)
    text = '; '.join(ec.pixel_items(launches, r.h, r.w, 24, 127))  # pixel block 24 of the plain order (member 0)
    assert 'member 0 pixel block 24: second position of a persistent block (band 25, step 24), band end' in text
    assert 'partial last block' in '; '.join(ec.pixel_items(predict_launches(3, 0, 9, 5, 15, 32, 'f16x3', 256), 15, 32, 14, 31))


# ---- the references ---------------------------------------------------------------------------------------------------------------
SMALL_ROWS = [r for r in EDGE_ROWS if r.h * r.w < ec.CPU_REFERENCE_MAX_PIXELS]


@pytest.mark.parametrize('row', SMALL_ROWS, ids=ec.row_id)
def test_references_of_the_small_rows(row):
    net = seeded_row_net(row)
    for seed in (1, 7):  # inputs A and B of tests/test_net_edges_gpu.py
        x = row_inputs(row, seed)
        ref = reference64(net, x)
        assert torch.isfinite(ref).all()
        assert int((ref.abs() > 0.99 * net.scale).sum()) == 0  # a saturated tanh hides errors
        with torch.no_grad():
            y32 = net({k: v for k, v in x.items() if k != 'sem_ids'})[0]
        err = float((y32.permute(1, 2, 0).reshape(-1, row.n_points).double() - ref).abs().max())
        print('%s seed %d: fp32 CPU net against float64 %.2e, max |est| %.3f' % (row.name, seed, err, float(ref.abs().max())))
        assert err <= 1e-6, (row.name, err)
