"""How every launch of the fusion net's forward pass cuts its frame - restated in plain Python from csrc/ojf_net.hip (plan_forward,
launch_conv_args, launch_chain, launch_pair_t, run_vortex) - and the table of the smallest frames that reach each tile, band and
frame edge of those launches.  Shared by tests/test_net_edges_host.py (coverage computed from the table, ojf_net_plan against the
restatement, the float64 / fp32 CPU references; no GPU) and tests/test_net_edges_gpu.py (every row against the float64 net in both
arithmetics, the OJF_NET_TRACE lines of a forward pass against predict_launches).
`growth` is counted as the C ABI counts it (growth_factor - 1), as in tests/net_plan_cases.py."""
import collections

# ---- the constants of the launch sites (tests/test_net_edges_host.py reads them back from the source) ---------------------------
POOL_TW, POOL_TH, POOL_HALO = 32, 8, 3    # kPoolTW, kPoolTH; three cascaded 3x3 pools
PERSIST_BPC = 3                           # persist_bpc: persistent blocks per CU over all members of a grouped launch
BAND_MIN_BLOCKS = 64                      # launch_conv_args: split-fp16 launches of at least this many pixel blocks are XCD-banded
BIG_TILE_MIN = 200                        # launch_chain / pair_cfg_for: 20x16 tiles from this many of them
BIG_TILE, SMALL_TILE = (20, 16), (12, 8)  # (TW, TH) of dense_chain_kernel / dense_pair_kernel
CHAIN_WAVES = 4                           # kChainWaves: 16-pixel strips per block of the entry / tail kernels
SUM_BLOCKS = 32                           # kSumBlocks: pixel strips of colsum_kernel
CHAIN_NG, CHAIN_MAX_LAYERS = 5, 7         # kChainNG, kChainMaxLayers
CHAIN_MAX_TILES = 8192                    # kChainSyncInts - kChainFlags0
K_NT = 2                                  # kNT: packed output tiles are padded to a multiple of it
SIDE0_MIN_NPIX = 32768                    # plan_forward: general flow, branch 0 on the side stream from this many pixels
XCDS = 8

CHAIN, PAIR = 'dense_chain_kernel', 'dense_pair_kernel'
CONV16, GROUPED, CONV32 = 'conv_f16x3_kernel', 'conv_f16x3_kernel (grouped)', 'conv_mfma_kernel'
COLSUM, GAVE, ENTRY, PYRAMID = 'colsum_kernel', 'gave_bias_kernel', 'entry1x1_kernel', 'pool_pyramid_kernel'
TAIL, TAIL_ENTRY = 'vortex_tail_kernel', 'vortex_tail_kernel (+ next entry GEMM)'
TAIL_HALF, TAIL_HEAD = 'vortex_tail_kernel (+ half of the next entry GEMM)', 'vortex_tail_kernel (+ prediction head)'
TAILS = (TAIL, TAIL_ENTRY, TAIL_HALF, TAIL_HEAD)
CONVS = (CONV16, GROUPED, CONV32)
DILATIONS = (1, 3, 9, 27)                 # VortexPooling.rates


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(a, b):
    return cdiv(a, b) * b


def conv16_chunk(nt):
    return 6 if nt <= 2 else 3


Shape = collections.namedtuple('Shape', 'version P gf sem h w arith c cs heads pool_in os npix')


def net_shape(version, sem, n_points, growth, h, w, arith):
    sem = int(bool(sem))
    c = 2 * n_points + 1 + (sem if version == 2 else 0)
    heads = 2 if version == 3 and sem else 1
    pool_in = c * (growth + 1)
    return Shape(version, n_points, growth, sem, h, w, arith, c, round_up(c, 4), heads, pool_in, round_up(pool_in, 4), h * w)


def c_in_phys(s, k):
    return (s.gf + 1) * s.cs if k < 2 else s.heads * s.os


def entry_tiles(cin, cs):
    return (8 if cin <= 128 else 16) if cin <= 256 and 4 * cs <= 80 else 0


def fused_tail_form(cs, os):
    return cdiv(cs, 16) == 2 and cdiv(os, 16) == 8


def chain_flow_form(s, k):
    return entry_tiles(c_in_phys(s, k), s.cs) != 0 and fused_tail_form(s.cs, s.os)


def pair_form(s):
    return s.arith == 'f16x3' and s.cs <= 24


def big_tiles(h, w):
    return cdiv(w, BIG_TILE[0]) * cdiv(h, BIG_TILE[1])


def dense_tile(h, w):
    """(TW, TH) of dense_chain_kernel and of dense_pair_kernel: one rule (launch_chain, pair_cfg_for)"""
    return BIG_TILE if big_tiles(h, w) >= BIG_TILE_MIN else SMALL_TILE


def chain_dense_form(s):
    tw, th = dense_tile(s.h, s.w)
    if s.arith != 'f16x3' or cdiv(s.w, tw) * cdiv(s.h, th) > CHAIN_MAX_TILES or s.w % 8:
        return False
    return pair_form(s) and s.cs == 4 * CHAIN_NG and s.gf <= CHAIN_MAX_LAYERS and chain_flow_form(s, 0)


def chain_kind_of(s):
    return s.c if s.P == 9 and s.gf == 5 and s.c in (19, 20) else 0


Step = collections.namedtuple('Step', 'vortex chain_flow entry entry_ntin branches tail z2')


def plan_forward(s):
    """-> (dense kind, steps, head_layers): plan_forward with the test-only switch off"""
    two, fused = s.heads == 2, fused_tail_form(s.cs, s.os)
    dense = 'chain' if chain_dense_form(s) else 'pairs' if pair_form(s) else 'convs'
    kind = chain_kind_of(s)
    n_steps = 3 if two else 2
    cin2 = c_in_phys(s, 2)
    halves = two and entry_tiles(cin2, s.cs) == 16 and cin2 == 2 * s.os and chain_flow_form(s, 0)
    steps, entry_done = [], False
    for i in range(n_steps):
        last = i == n_steps - 1
        vortex = 2 if last else (1 - i if two else 0)
        flow = chain_flow_form(s, vortex)
        entry = 'generic' if not flow else 'prev_tail' if last and entry_done else 'kernel'
        branches = 'grouped' if flow or s.npix < SIDE0_MIN_NPIX else 'side0'
        if not fused:
            tail = 'unfused'
        elif last:
            tail = 'head' if kind else 'alone'
        elif halves:
            tail = 'half'
        elif not two and flow and chain_flow_form(s, 2) and cin2 == s.os:
            tail = 'entry'
        else:
            tail = 'alone'
        entry_done = entry_done or tail in ('entry', 'half')
        steps.append(Step(vortex, flow, entry, entry_tiles(c_in_phys(s, vortex), s.cs), branches, tail, last and halves))
    return dense, steps, steps[-1].tail != 'head'


# ---- one generic convolution launch (launch_conv_args) ------------------------------------------------------------------------
Member = collections.namedtuple('Member', 'c_in c_out taps dil lean_ok')


def n_ot(c_out_phys):
    return round_up(cdiv(c_out_phys, 16), K_NT)


def conv_launch(s, members, cus):
    """members of one shape; -> the launch's fields as launch_conv_args decides them"""
    f16, n = s.arith == 'f16x3', len(members)
    nt = n_ot(members[0].c_out)
    mt = (1 if nt >= 6 else 2) if f16 else 1
    grid_x = cdiv(cdiv(s.npix, mt * 16), 4)
    nblocks, grid16_x, band = 0, grid_x, 0
    if f16 and grid_x >= BAND_MIN_BLOCKS:
        nblocks, grid16_x = grid_x, round_up(grid_x, XCDS)
    perm = []
    for m in members:
        if nblocks and m.taps == 9 and 1 < m.dil < s.h and s.w % (mt * 16) == 0:
            perm.append((m.dil, s.h // m.dil, s.h % m.dil))
        else:
            perm.append((0, 0, 0))
    if nblocks:
        per = 8  # K entries per split-fp16 superstep
        single = all(cdiv(m.taps * (m.c_in // 4), per) <= conv16_chunk(nt) for m in members)
        n8 = round_up(nblocks, XCDS)
        G = (cus * PERSIST_BPC // n) // XCDS * XCDS if cus > 0 else 0
        if single and XCDS <= G < n8:
            band, grid16_x = n8 // XCDS, G
    lean = f16 and all(m.lean_ok for m in members)
    name = CONV32 if not f16 else GROUPED if n > 1 else CONV16
    return dict(name=name, n=n, mt=mt, nt=nt, grid_x=grid_x, nblocks=nblocks, grid16_x=grid16_x, band=band, lean=int(lean),
                perm=','.join('%d:%d:%d' % p for p in perm))


def predict_launches(version, sem, n_points, growth, h, w, arith, cus):
    """Every launch of a forward pass in host enqueue order, each a dict: 'name' and the fields its OJF_NET_TRACE line carries."""
    s = net_shape(version, sem, n_points, growth, h, w, arith)
    dense, steps, head_layers = plan_forward(s)
    cs, os, c4 = s.cs, s.os, s.cs // 4
    out = []
    blocks = cdiv(cdiv(s.npix, 16), CHAIN_WAVES)  # chain_blocks: entry1x1_kernel / vortex_tail_kernel
    banded = int(blocks % XCDS == 0)              # banded_block_x permutes only then
    for st in steps:
        if st.vortex < 2:
            tw, th = dense_tile(h, w)
            tx, ty = cdiv(w, tw), cdiv(h, th)
            if dense == 'chain':
                out.append(dict(name=CHAIN, tw=tw, th=th, tiles_x=tx, tiles_y=ty, tiles=tx * ty,
                                grid_x=cus if 0 < cus < tx * ty else tx * ty))
            elif dense == 'pairs':
                out += [dict(name=PAIR, tw=tw, th=th, tiles_x=tx, tiles=tx * ty, grid_x=tx * ty, banded=int(tx * ty % XCDS == 0))] * s.gf
            else:
                for i in range(s.gf):
                    out.append(conv_launch(s, [Member((i + 1) * cs, cs, 9, 1, True)], cus))
                    out.append(conv_launch(s, [Member(cs, cs, 9, 1, True)], cus))
        cin = c_in_phys(s, st.vortex)
        if st.entry == 'generic':
            out.append(dict(name=COLSUM, grid_x=SUM_BLOCKS, grid_y=cin // 4))
            out.append(dict(name=GAVE, grid_x=1, grid_y=1))
            out.append(conv_launch(s, [Member(cin, 4 * cs, 1, 1, False)], cus))  # ReLU on branch 0's channels only: not lean
        elif st.entry == 'kernel':
            out.append(dict(name=ENTRY, ntin=st.entry_ntin, blocks=blocks, banded=banded))
        tiles = cdiv(w, POOL_TW) * cdiv(h, POOL_TH)
        out.append(dict(name=PYRAMID, tiles=tiles, grid_x=round_up(tiles + (1 if st.chain_flow else 0), XCDS), grid_y=(4 if st.z2 else 3) * c4))
        branch = [Member(cs, cs, 9, d, True) for d in DILATIONS]
        if st.branches == 'grouped':
            out += [conv_launch(s, branch, cus)] * 2
        else:
            out += [conv_launch(s, branch[:1], cus)] * 2 + [conv_launch(s, branch[1:], cus)] * 2
        if st.tail == 'unfused':
            out += [conv_launch(s, [Member(cs, os, 1, 1, True)], cus)] * 4
            out.append(conv_launch(s, [Member(4 * os, os, 1, 1, True)], cus))
        else:
            out.append(dict(name={'alone': TAIL, 'entry': TAIL_ENTRY, 'half': TAIL_HALF, 'head': TAIL_HEAD}[st.tail], blocks=blocks, banded=banded))
    if head_layers:  # Pred((gf + 1 - i) c, (gf - i) c): two 1x1 each, the last one a third into the caller's rows
        prev = os
        for i in range(s.gf):
            cout = round_up((s.gf - i) * s.c, 4)
            out.append(conv_launch(s, [Member(prev, cout, 1, 1, True)], cus))
            out.append(conv_launch(s, [Member(cout, cout, 1, 1, True)], cus))
            prev = cout
        out.append(conv_launch(s, [Member(prev, round_up(s.P, 4), 1, 1, False)], cus))
    return out


def parse_trace(text):
    """The 'ojf_net <name> | <field> <value> ...' lines of a process's stderr -> launches like predict_launches'"""
    out = []
    for line in text.splitlines():
        if not line.startswith('ojf_net ') or ' | ' not in line:
            continue
        name, rest = line[len('ojf_net '):].split(' | ')
        tok = rest.split()
        d = dict(name=name)
        for k, v in zip(tok[::2], tok[1::2]):
            d[k] = v if k == 'perm' else int(v)
        out.append(d)
    return out


# ---- what a frame reaches -------------------------------------------------------------------------------------------------------
def perms(launch):
    return [tuple(int(v) for v in m.split(':')) for m in launch['perm'].split(',')]


def reached(version, sem, n_points, growth, h, w, cus=256):
    """The set of edge items the f16x3 launches of this net and frame reach (computed from predict_launches)."""
    L = predict_launches(version, sem, n_points, growth, h, w, 'f16x3', cus)
    s = net_shape(version, sem, n_points, growth, h, w, 'f16x3')
    dense, steps, head_layers = plan_forward(s)
    npix, it = h * w, set()
    names = [l['name'] for l in L]
    if npix < 16:
        it.add('npix < 16')
    if h < POOL_HALO and w < POOL_HALO:
        it.add('halo wider than the frame in both axes')
    if h < POOL_HALO:
        it.add('pyramid with h < 3')
    if w < POOL_HALO:
        it.add('pyramid and every 3x3 with w < 3')
    would_chain = chain_dense_form(s._replace(w=round_up(w, 8)))
    if PAIR in names and w % 8 and would_chain:
        it.add('chain refused (w % 8)')
    if PAIR in names:
        it.add('pair kernels')
    for l in L:
        n = l['name']
        if n == CHAIN:
            it.add('chain tile %dx%d' % (l['tw'], l['th']))
            if h < 8:
                it.add('chain kernel with h < 8')
            if l['tiles'] == 1 and (l['tw'], l['th']) == SMALL_TILE and h % l['th'] and w % l['tw']:
                it.add('one 12x8 chain tile, ragged in both axes')
            if (l['tw'], l['th']) == BIG_TILE:
                if big_tiles(h, w) == BIG_TILE_MIN:
                    it.add('exactly 200 big tiles')
                if h % l['th'] and w % l['tw'] == 4:
                    it.add('20x16 chain tiles: ragged last tile row, 4-pixel last tile column')
                if s.heads == 2:
                    it.add('20x16 chain tiles, two heads')
            elif big_tiles(h, w) == BIG_TILE_MIN - 2:
                it.add('198 big tiles -> 12x8')
        if n == PAIR:
            it.add('pair tile %dx%d' % (l['tw'], l['th']))
            it.add('pair tiles %% 8 %s 0' % ('==' if l['banded'] else '!='))
        if n == PYRAMID:
            it.add('pyramid tiles %% 8 == %d' % (l['tiles'] % 8))
            if l['grid_y'] == 4 * (s.cs // 4) and (w % POOL_TW or h % POOL_TH):
                it.add('lv == 4 row on a ragged frame')
        if n == ENTRY or n in TAILS:
            kind = 'entry' if n == ENTRY else 'tail'
            if npix % 64:
                it.add('%s %s blocks with npix %% 64 != 0' % ('banded' if l['banded'] else 'unbanded', kind))
                if l['banded']:
                    it.add('banded %s blocks, npix %% 64 == %d' % (kind, npix % 64))
            if l['banded'] and l['blocks'] == 8 and npix % 64 == 32:
                it.add('8 entry / tail blocks (banded), last block half idle')
        if n == TAIL_HALF:
            it.add('half-entry tails')
            if npix % 64 == 16:
                it.add('half-entry tails, npix % 64 == 16')
        if n == GROUPED:
            pm = perms(l)
            on = [p for p in pm if p[0]]
            it.add('grid.x == %d' % l['grid_x'] if l['grid_x'] in (63, 64) else 'grid.x other')
            if l['nblocks']:
                it.add('banded grouped launch')
                if l['nblocks'] % 8 and l['band']:
                    it.add('nblocks % 8 != 0 with band != 0')
                if l['nblocks'] % 8 and not l['band']:
                    it.add('banded, nblocks %% 8 == %d, not persistent' % (l['nblocks'] % 8))
                if npix % (l['mt'] * 64):
                    it.add('banded grouped launch, partial last pixel block')
            if l['band']:
                it.add('persistent')
                if l['band'] % (l['grid16_x'] // 8):
                    it.add('band % (grid16.x / 8) != 0')
                if l['band'] == l['grid16_x'] // 8 + 1:
                    it.add('band one above the step')
                if l['band'] * 8 > l['nblocks']:
                    it.add('last XCD band partly padding')
                it.add('persistent with permutation' if on else 'persistent without permutation')
                if on and npix % (l['mt'] * 64):
                    it.add('persistent, permutation on, npix % 128 != 0')
            if on:
                it.add('row_perm')
                it.add('row_perm with perm_rem %s 0' % ('!=' if any(p[2] for p in on) else '=='))
                if any(p[2] == 0 for p in on):
                    it.add('row_perm with perm_rem == 0')
                if any(p[2] != 0 for p in on):
                    it.add('row_perm with perm_rem != 0')
                if any(p[1] == 1 for p in on):
                    it.add('perm_q == 1')
                if any(p[1] == 1 and p[2] == 1 for p in on):
                    it.add('perm_q == 1, perm_rem == 1')
                if len(on) < sum(1 for d in DILATIONS if d > 1):
                    it.add('a group with mixed row_perm')
                if [p[2] for p in on] == [1, 1, 19]:
                    it.add('perm_rem 1, 1, 19')
                if npix % (l['mt'] * 64):
                    it.add('partial last pixel block under the permutation')
            if any(d >= h for d in DILATIONS) and on:
                it.add('dilation 27 with dil >= h beside permuted members')
    if chain_kind_of(s) == 20 and (w % POOL_TW or h % POOL_TH or npix % 64):
        it.add('chain_kind 20 on a ragged frame')
    ragged = bool(npix % 64 or w % 8)
    if COLSUM in names:
        it.add('general flow')
        if ragged:
            it.add('general flow on a ragged frame')
        if (SUM_BLOCKS - 1) * cdiv(npix, SUM_BLOCKS) >= npix:
            it.add('colsum_kernel with empty strips')
    if any(st.tail == 'unfused' for st in steps):
        it.add('unfused tail' + (' on a ragged frame' if ragged else ''))
    if TAIL in names:
        it.add('TAIL_ALONE' + (' on a ragged frame' if ragged else ''))
    if head_layers:
        it.add('layer-by-layer head' + (' on a ragged frame' if ragged else ''))
        if npix < 16:
            it.add('layer-by-layer head on a tiny frame')
    return it


def pixel_items(launches, h, w, y, x):
    """Which edges of the predicted launches the pixel (y, x) falls into: what a failing row prints beside its worst pixel."""
    p, npix, out = y * w + x, h * w, []
    seen = set()
    for l in launches:
        n = l['name']
        key = (n, tuple(sorted(l.items())))
        if key in seen:
            continue
        seen.add(key)
        if n in (CHAIN, PAIR):
            tw, th = l['tw'], l['th']
            at = []
            if x % tw in (0, tw - 1) or y % th in (0, th - 1):
                at.append('tile edge')
            if x // tw == cdiv(w, tw) - 1 and w % tw:
                at.append('ragged last tile column')
            if y // th == cdiv(h, th) - 1 and h % th:
                at.append('ragged last tile row')
            if at:
                out.append('%s %dx%d tile (%d, %d): %s' % (n, tw, th, y // th, x // tw, ', '.join(at)))
        elif n == PYRAMID:
            at = []
            if x % POOL_TW in (0, POOL_TW - 1) or y % POOL_TH in (0, POOL_TH - 1):
                at.append('tile edge')
            if min(x, y, w - 1 - x, h - 1 - y) < POOL_HALO:
                at.append('frame border inside the halo')
            tile = (y // POOL_TH) * cdiv(w, POOL_TW) + x // POOL_TW
            if tile == l['tiles'] - 1:
                at.append('last tile')
            if at:
                out.append('%s tile %d of %d: %s' % (n, tile, l['tiles'], ', '.join(at)))
        elif n == ENTRY or n in TAILS:
            if p // 64 == l['blocks'] - 1 and npix % 64:
                out.append('%s: partial last block (%d pixels)%s' % (n, npix % 64, ', banded order' if l['banded'] else ''))
        elif n in CONVS:
            per = l['mt'] * 64
            at = []
            for i, (r, q, rem) in enumerate(perms(l)):
                pos = p
                if r:  # position of row y in the order (y mod r, y div r)
                    c, k = y % r, y // r
                    pr = c * (q + 1) + k if c < rem else rem * (q + 1) + (c - rem) * q + k
                    pos = pr * w + x
                sb = pos // per
                here = []
                if sb == l['grid_x'] - 1 and npix % per:
                    here.append('partial last pixel block')
                if l['band']:
                    step = l['grid16_x'] // 8
                    if sb % l['band'] >= step:
                        here.append('second position of a persistent block (band %d, step %d)' % (l['band'], step))
                    if sb % l['band'] == l['band'] - 1:
                        here.append('band end')
                elif l['nblocks'] and sb % (l['grid16_x'] // 8) == l['grid16_x'] // 8 - 1:
                    here.append('band end')
                if r and y % r < rem and y // r == q:
                    here.append('extra row of a long class (perm %d:%d:%d)' % (r, q, rem))
                if here:
                    at.append('member %d pixel block %d: %s' % (i, sb, ', '.join(here)))
            if at:
                out.append('%s n %d nt %d: %s' % (n, l['n'], l['nt'], '; '.join(at)))
    return out


# ---- the table ----------------------------------------------------------------------------------------------------------------
# name -> (version, sem, n_points, growth, h, w), the items the row claims (keys of reached())
Row = collections.namedtuple('Row', 'name version sem n_points growth h w claims')


def _v3(name, h, w, claims, sem=0):
    return Row(name, 3, sem, 9, 5, h, w, tuple(claims))


EDGE_ROWS = [
    _v3('one_pixel', 1, 1, ['npix < 16', 'halo wider than the frame in both axes', 'chain refused (w % 8)']),
    _v3('one_row', 1, 40, ['chain kernel with h < 8', 'pyramid with h < 3']),
    _v3('one_row_sem', 1, 40, ['chain kernel with h < 8', 'pyramid with h < 3', 'lv == 4 row on a ragged frame'], sem=1),
    _v3('one_column', 40, 1, ['pyramid and every 3x3 with w < 3', 'pair kernels', 'pair tiles % 8 != 0']),
    _v3('below_a_tile', 3, 8, ['one 12x8 chain tile, ragged in both axes']),
    _v3('banded_tail_partial', 15, 32, ['8 entry / tail blocks (banded), last block half idle', 'banded entry blocks with npix % 64 != 0']),
    _v3('banded_tail_partial_sem', 15, 32, ['8 entry / tail blocks (banded), last block half idle', 'half-entry tails'], sem=1),
    _v3('band_threshold_63', 63, 128, ['grid.x == 63', 'pyramid tiles % 8 == 0']),
    _v3('band_threshold_64', 127, 64, ['grid.x == 64', 'banded grouped launch', 'row_perm', 'perm_rem 1, 1, 19', 'row_perm with perm_rem != 0']),
    _v3('perm_mixed_27', 27, 320, ['dilation 27 with dil >= h beside permuted members', 'a group with mixed row_perm', 'row_perm with perm_rem == 0']),
    _v3('perm_mixed_28', 28, 320, ['perm_q == 1', 'perm_q == 1, perm_rem == 1']),
    _v3('banded_ragged', 55, 160, ['banded, nblocks % 8 == 5, not persistent', 'banded grouped launch, partial last pixel block',
                                   'partial last pixel block under the permutation']),
    _v3('persist_perm_ragged', 155, 160, ['persistent with permutation', 'band one above the step', 'band % (grid16.x / 8) != 0',
                                          'nblocks % 8 != 0 with band != 0', 'persistent, permutation on, npix % 128 != 0',
                                          'last XCD band partly padding']),
    _v3('persist_perm_ragged_sem', 155, 160, ['persistent with permutation', 'band one above the step', 'persistent, permutation on, npix % 128 != 0',
                                              'lv == 4 row on a ragged frame'], sem=1),
    _v3('persist_perm_193', 193, 128, ['persistent with permutation', 'band one above the step', 'nblocks % 8 != 0 with band != 0',
                                       'last XCD band partly padding']),
    _v3('persist_plain_ragged_8', 149, 168, ['persistent without permutation', 'banded entry blocks, npix % 64 == 8']),
    _v3('persist_plain_ragged_56', 209, 120, ['persistent without permutation', 'banded entry blocks, npix % 64 == 56']),
    _v3('chain_big_threshold_198', 1584, 24, ['198 big tiles -> 12x8', 'chain tile 12x8']),
    _v3('chain_big_threshold_200', 1589, 24, ['exactly 200 big tiles', 'chain tile 20x16', '20x16 chain tiles: ragged last tile row, 4-pixel last tile column',
                                              'pyramid tiles % 8 == 7']),
    _v3('chain_big_two_heads', 211, 304, ['20x16 chain tiles, two heads', 'half-entry tails, npix % 64 == 16'], sem=1),
    _v3('pair_big', 211, 301, ['pair tile 20x16', 'pair tiles % 8 == 0', 'chain refused (w % 8)']),
    Row('v2_sem_ragged_15x32', 2, 1, 9, 5, 15, 32, ('chain_kind 20 on a ragged frame',)),
    Row('v2_sem_ragged_37x53', 2, 1, 9, 5, 37, 53, ('chain_kind 20 on a ragged frame', 'pair tile 12x8', 'unbanded entry blocks with npix % 64 != 0')),
    Row('general_5_4_ragged', 3, 0, 5, 4, 37, 53, ('general flow on a ragged frame', 'unfused tail on a ragged frame', 'layer-by-layer head on a ragged frame')),
    Row('general_5_4_tiny', 3, 0, 5, 4, 3, 5, ('general flow on a ragged frame', 'colsum_kernel with empty strips', 'layer-by-layer head on a tiny frame')),
    Row('general_3_3_sem_ragged', 3, 1, 3, 3, 37, 53, ('general flow on a ragged frame', 'unfused tail on a ragged frame')),
    Row('general_3_3_sem_tiny', 3, 1, 3, 3, 3, 5, ('colsum_kernel with empty strips', 'layer-by-layer head on a tiny frame')),
    Row('tail_alone_8_6_ragged', 3, 0, 8, 6, 37, 53, ('TAIL_ALONE on a ragged frame', 'layer-by-layer head on a ragged frame',
                                                       'unbanded tail blocks with npix % 64 != 0')),
]

# reached by at least one row (tests/test_net_edges_host.py::test_rows_reach_every_listed_edge)
EDGES_ANYWHERE = [
    'nblocks % 8 != 0 with band != 0', 'band % (grid16.x / 8) != 0', 'row_perm with perm_rem == 0', 'row_perm with perm_rem != 0',
    'perm_q == 1', 'a group with mixed row_perm', 'grid.x == 63', 'grid.x == 64', 'chain tile 12x8', 'chain tile 20x16',
    'pair tile 12x8', 'pair tile 20x16', 'banded entry blocks with npix % 64 != 0', 'unbanded entry blocks with npix % 64 != 0',
    'pyramid tiles % 8 == 0', 'pyramid tiles % 8 == 7', 'pair tiles % 8 == 0', 'pair tiles % 8 != 0',
]

# the frame sizes of tests/test_net_gpu.py::test_fusion_net_forward and tests/test_headline_gpu.py
OLD_SIZES = [(24, 32), (60, 80), (120, 160), (45, 77), (5, 7), (240, 320), (480, 640)]
OLD_NETS = [(3, 0, 9, 5), (3, 1, 9, 5), (2, 0, 9, 5), (2, 1, 9, 5)]
OLD_TOPOLOGIES = [((3, 0, 5, 3), (40, 56)), ((3, 1, 3, 2), (40, 56)), ((2, 1, 7, 4), (40, 56)), ((3, 0, 8, 6), (40, 56))]
# what none of them reaches (at 256 CUs): the reason for the table.  (They do reach 'band % (grid16.x / 8) != 0' - 240x320 walks a band of
# 75 in steps of 24 - and 'chain_kind 20 on a ragged frame' - v2 with semantics at 45x77 and 5x7.)
NOT_REACHED_BY_OLD_SIZES = [
    'npix < 16', 'halo wider than the frame in both axes', 'pyramid with h < 3', 'pyramid and every 3x3 with w < 3',
    'chain kernel with h < 8', 'one 12x8 chain tile, ragged in both axes', '8 entry / tail blocks (banded), last block half idle',
    'banded entry blocks with npix % 64 != 0', 'banded tail blocks with npix % 64 != 0', 'grid.x == 63', 'grid.x == 64',
    'dilation 27 with dil >= h beside permuted members', 'a group with mixed row_perm', 'perm_q == 1',
    'partial last pixel block under the permutation', 'banded grouped launch, partial last pixel block',
    'nblocks % 8 != 0 with band != 0', 'band one above the step', 'last XCD band partly padding',
    'persistent, permutation on, npix % 128 != 0', 'persistent without permutation', 'exactly 200 big tiles', '198 big tiles -> 12x8',
    '20x16 chain tiles: ragged last tile row, 4-pixel last tile column', 'pair tile 20x16', 'pair tiles % 8 == 0',
    'half-entry tails, npix % 64 == 16', 'general flow on a ragged frame',
    'colsum_kernel with empty strips', 'unfused tail on a ragged frame', 'TAIL_ALONE on a ragged frame',
    'layer-by-layer head on a ragged frame', 'layer-by-layer head on a tiny frame',
]

MAX_ROW_PIXELS = 211 * 304  # no row is larger than the largest whose float64 reference was timed (7 s)
CPU_REFERENCE_MAX_PIXELS = 10000  # rows below it get their references checked without a GPU as well


def row_id(row):
    return row.name


# ---- nets, inputs and the float64 reference of a row ----------------------------------------------------------------------------
def seeded_row_net(row, seed=0):
    """tests/test_net_gpu.py's seeded_net for the row's topology"""
    import test_net_gpu
    return test_net_gpu.seeded_net('v%d' % row.version, bool(row.sem), row.h, row.w, seed, n_points=row.n_points, growth_factor=row.growth + 1)


def row_inputs(row, seed=1):
    """tests/test_net_gpu.py's _inputs + the semantic frame of its sem_ids"""
    import test_net_gpu
    x = test_net_gpu._inputs(row.h, row.w, seed, n_points=row.n_points)
    x['semantic_frame'] = ((1 + x['sem_ids'].float()) / 30).view(1, 1, row.h, row.w)
    return x


def reference64(net, x):
    """The float64 net (copy.deepcopy(net).double()) on the inputs widened to float64 -> [h * w, n_points] float64"""
    import copy
    import torch
    net64 = copy.deepcopy(net).double()
    x64 = {k: v.double() for k, v in x.items() if k != 'sem_ids'}
    with torch.no_grad():
        y = net64(x64)[0]
    return y.permute(1, 2, 0).reshape(-1, y.shape[0])
