"""The SEGCONV kernel forms one at a time (csrc/ojf_seg.hip): a plain Python restatement of the form choice of
``seg_launch`` / ``seg_launch_multi`` from the dispatcher's named constants, and the tables of the smallest layers that
reach every form without dropout at its tile, row and K-walk edges.  No GPU import: test_segconv_forms_host.py proves on
the CPU that the tables reach what they claim, test_segconv_forms_gpu.py runs them against float64 convolutions and
proves from the launch trace that prediction == launch."""
from collections import namedtuple

# ---- the dispatcher's constants (csrc/ojf_seg.hip, in front of seg_launch) ----------------------------------------------
K_MW = 4                  # kMW: channel tiles of 16 per 64-channel group
K_DEPTH = 3               # kDepth of every segconv_kernel instantiation: K blocks in flight per wave
PLAIN_MIN_WAVES = 1024    # kPlainMinWaves
SPLITK_MIN_KB = 8         # kSplitKMinKb
SPLITK_MIN_BLOCKS = 150   # kSplitKMinBlocks
NW2_MIN_KB = 32           # kNw2MinKb
NW2_MAX_BLOCKS = 400      # kNw2MaxBlocks
PLAIN_NW1_MIN = 50        # kPlainNw1Min
GEMM_MIN = 256            # kGemmMin
GEMM22_MIN = 128          # kGemm22Min
GEMM_MIN_KB = 4           # kGemmMinKb
MULTI_OWN_MIN_KB = 6      # kMultiOwnMinKb
MULTI_OWN_MIN_BLOCKS = 256  # kMultiOwnMinBlocks

GEMM_MENU = ((4, 4, 'gemm 64x64'), (8, 8, 'gemm 128x128'), (8, 10, 'gemm 128x160'), (8, 5, 'gemm 128x80'))
GEMM_ALONE_US = (28.0, 59.5, 94.5, 51.0)

PLAIN_FORMS = ('<4,2,1,1>', '<4,1,2,1>', '<4,2,2,1>')
SPLITK_FORMS = ('<1,1,1,4>', '<2,1,1,4>', '<4,1,1,4>', '<4,2,1,4>')
GEMM_FORMS = tuple(m[2] for m in GEMM_MENU)
MULTI_FORMS = ('multi<4,2,2,1>', 'multi<1,1,1,4>', 'multi<2,1,1,4>', 'multi<4,1,1,4>')
ALL_FORMS = PLAIN_FORMS + SPLITK_FORMS + GEMM_FORMS

# form -> (channel tiles of 16, pixel tiles of 16) of a BLOCK
BLOCK_TILES = {'<4,2,1,1>': (4, 8), '<4,1,2,1>': (8, 2), '<4,2,2,1>': (8, 4), '<1,1,1,4>': (1, 1), '<2,1,1,4>': (2, 1), '<4,1,1,4>': (4, 1),
               '<4,2,1,4>': (4, 2), 'gemm 64x64': (4, 4), 'gemm 128x128': (8, 8), 'gemm 128x160': (8, 10), 'gemm 128x80': (8, 5)}


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(a, b):
    return cdiv(a, b) * b


Geometry = namedtuple('Geometry', 'c8 n_kb n_ct n_pt Ho Wo n_pix entries rows')


def geometry(c_in, c_out, k, stride, dil, pad, h, w, batch, deconv_stride=0):
    """ojf_segconv_create / seg_fill: the numbers the dispatcher sees.  A transposed convolution of stride s is a 3x3
    convolution (padding 1) to s * s phase copies of round_up(c_out, 4) rows (ojf_segdeconv_create)."""
    rows = c_out
    if deconv_stride:
        rows = deconv_stride * deconv_stride * round_up(c_out, 4)
        k, stride, dil, pad = 3, 1, 1, 1
    c8 = cdiv(c_in, 8)
    entries = k * k * c8
    span = dil * (k - 1) + 1
    Ho, Wo = (h + 2 * pad - span) // stride + 1, (w + 2 * pad - span) // stride + 1
    assert Ho >= 1 and Wo >= 1
    n_pix = batch * Ho * Wo
    return Geometry(c8, cdiv(entries, 4), round_up(cdiv(rows, 16), K_MW), cdiv(n_pix, 16), Ho, Wo, n_pix, entries, rows)


def seg_map(X, Y, Z):
    """seg_map: (S, chunk, V) of the logical grid X x Y x Z and the blocks of the 1-D launch."""
    Q = Y * Z
    S = 1
    while S < 8 and (Q * S) % 8 != 0 and cdiv(X, 2 * S) >= 2:
        S *= 2
    chunk = cdiv(X, S)
    V = Q * S
    return (S, chunk, V), round_up(V, 8) * chunk


Prediction = namedtuple('Prediction', 'form smap counts grid')  # smap (S, chunk, V), counts (n_kb, n_ct, n_pt), grid (X, Y, Z)


def _gemm_choice(n_kb, n_ct, n_pt, n):
    """The GEMM-shaped branch of seg_launch without dropout: index into GEMM_MENU, or None."""
    b44 = cdiv(n_ct, 8) * cdiv(n_pt, 8) * n
    b22 = cdiv(n_ct, 4) * cdiv(n_pt, 4) * n
    big = b44 >= GEMM_MIN and n_ct >= 8
    if not (n_kb >= GEMM_MIN_KB and (big or b22 >= GEMM22_MIN)):
        return None
    best = 1 if big else 0
    if big:
        b810 = cdiv(n_ct, 8) * cdiv(n_pt, 10) * n
        if b810 >= 200 and cdiv(b810, 256) < cdiv(b44, 256):
            best = 2
    if n_kb >= 64:
        pick, best_t = -1, 0.0
        for i, (ta, tb, _) in enumerate(GEMM_MENU):
            if ta == 8 and n_ct < 8:
                continue
            blocks = cdiv(n_ct, ta) * cdiv(n_pt, tb) * n
            if blocks < 100:
                continue
            r = cdiv(blocks, 256)
            t = GEMM_ALONE_US[i] * (1.65 * (r // 2) + (r & 1))
            if pick < 0 or t < best_t:
                pick, best_t = i, t
        if pick >= 0:
            best = pick
    return best


def predict_counts(n_kb, n_ct, n_pt, n):
    """seg_launch on the dispatcher's own numbers (no dropout): form and logical grid."""
    groups = n_ct // K_MW
    best = _gemm_choice(n_kb, n_ct, n_pt, n)
    if best is not None:
        ta, tb, name = GEMM_MENU[best]
        return name, (cdiv(n_pt, tb), cdiv(n_ct, ta), n)
    waves2 = groups * cdiv(n_pt, 2) * n
    if waves2 >= PLAIN_MIN_WAVES or n_kb < SPLITK_MIN_KB:
        if groups == 1:
            return '<4,2,1,1>', (cdiv(n_pt, 8), 1, n)
        if n_pt >= PLAIN_NW1_MIN:
            return '<4,1,2,1>', (cdiv(n_pt, 2), cdiv(groups, 2), n)
        return '<4,2,2,1>', (cdiv(n_pt, 4), cdiv(groups, 2), n)
    mw = 4
    while mw > 1 and n_pt * (n_ct // mw) * n < SPLITK_MIN_BLOCKS:
        mw //= 2
    blocks_nw2 = cdiv(n_pt, 2) * groups * n
    if mw == 1:
        return '<1,1,1,4>', (n_pt, n_ct, n)
    if mw == 2:
        return '<2,1,1,4>', (n_pt, n_ct // 2, n)
    if n_kb >= NW2_MIN_KB and SPLITK_MIN_BLOCKS <= blocks_nw2 < NW2_MAX_BLOCKS:
        return '<4,2,1,4>', (cdiv(n_pt, 2), groups, n)
    return '<4,1,1,4>', (n_pt, groups, n)


def predict_form(c_in, c_out, k, stride, dil, pad, h, w, batch, members, deconv_stride=0):
    """The launch of ``members`` convolutions of this shape without dropout (ojf_segconv_forward_group_batch -> seg_launch):
    the form as seg_trace prints it, the SegMap numbers (S, chunk, V), (n_kb, n_ct, n_pt) and the logical grid (X, Y, Z)."""
    g = geometry(c_in, c_out, k, stride, dil, pad, h, w, batch, deconv_stride)
    form, grid = predict_counts(g.n_kb, g.n_ct, g.n_pt, members)
    return Prediction(form, seg_map(*grid)[0], (g.n_kb, g.n_ct, g.n_pt), grid)


MultiPrediction = namedtuple('MultiPrediction', 'form maps total groups')


def predict_multi(members, batch=1):
    """seg_launch_multi for ``members`` = [(c_in, c_out, k, stride, dil, pad, h, w, epilogue), ...] on fresh outputs, no
    dropout.  One launch: form 'multi<...>', maps = per member ((S, chunk, V), (X, Y)), total = blocks of the 1-D grid.
    Otherwise form 'separate' and groups = the Prediction of every natural group (members of one shape), in launch order."""
    geo = [geometry(*m[:8], batch) for m in members]
    # same_shape of seg_launch_multi: with fresh outputs the row strides follow from the channel counts
    key = [(g.n_kb, g.n_ct, g.c8, m[1], m[2], m[3], g.Ho, g.Wo, m[8]) for m, g in zip(members, geo)]
    n_split = n_plain = 0
    own = False
    for g, kk in zip(geo, key):
        same = key.count(kk)
        groups = g.n_ct // K_MW
        if g.n_kb >= MULTI_OWN_MIN_KB and groups * cdiv(g.n_pt, 8) * same >= MULTI_OWN_MIN_BLOCKS:
            own = True
        if groups * cdiv(g.n_pt, 2) * same >= PLAIN_MIN_WAVES or g.n_kb < SPLITK_MIN_KB:
            n_plain += 1
        else:
            n_split += 1
    if own or (n_split and n_plain):
        out, done = [], set()
        for i, kk in enumerate(key):
            if kk in done:
                continue
            done.add(kk)
            form, grid = predict_counts(geo[i].n_kb, geo[i].n_ct, geo[i].n_pt, key.count(kk))
            out.append(Prediction(form, seg_map(*grid)[0], (geo[i].n_kb, geo[i].n_ct, geo[i].n_pt), grid))
        return MultiPrediction('separate', None, None, out)
    mw = 4
    if not n_plain:
        blocks4 = sum(g.n_pt * (g.n_ct // K_MW) for g in geo)
        while mw > 1 and blocks4 * (4 // mw) < SPLITK_MIN_BLOCKS:
            mw //= 2
    maps, total = [], 0
    for g in geo:
        X, Y = (cdiv(g.n_pt, 4), cdiv(g.n_ct // K_MW, 2)) if n_plain else (g.n_pt, g.n_ct // mw)
        smap, blocks = seg_map(X, Y, 1)
        maps.append((smap, (X, Y)))
        total += round_up(blocks, 8)
    form = 'multi<4,2,2,1>' if n_plain else 'multi<%d,1,1,4>' % mw
    return MultiPrediction(form, maps, total, None)


def former_wide_branch_taken(n_kb, groups, n_pt, n):
    """The dispatcher before segconv_wide_kernel<2> was removed: its branch (n_kb >= 6 and groups * ceil(n_pt / 8) * n >= 256)
    came AFTER the GEMM-shaped branch.  True where a launch would have reached it.  Works on numpy arrays."""
    n_ct = groups * K_MW
    b44 = -(-n_ct // 8) * -(-n_pt // 8) * n
    b22 = groups * -(-n_pt // 4) * n
    gemm = (n_kb >= GEMM_MIN_KB) & (((b44 >= GEMM_MIN) & (n_ct >= 8)) | (b22 >= GEMM22_MIN))
    wide = (n_kb >= 6) & (groups * -(-n_pt // 8) * n >= 256)
    return ~gemm & wide


# ---- the edges a row carries, computed from its numbers -------------------------------------------------------------------
def row_edges(row):
    """The set of edge names a FORM_TABLE / DECONV_TABLE row carries (see EDGES_PER_FORM / EDGES_ANYWHERE)."""
    name, c_in, c_out, k, stride, dil, pad, h, w, batch, members, form = row[:12]
    up = row[12] if len(row) > 12 else 0
    g = geometry(c_in, c_out, k, stride, dil, pad, h, w, batch, up)
    pred = predict_form(c_in, c_out, k, stride, dil, pad, h, w, batch, members, up)
    edges = set()
    if c_out % 4:
        edges.add('c_out partial group of 4')
    if g.rows % 16:
        edges.add('c_out partial 16-tile')
    if cdiv(g.rows, 16) % K_MW:
        edges.add('n_ct padded')
    if g.n_pix % 16:  # (then no multiple of the block's pixel extent either: that is a multiple of 16)
        edges.add('ragged pixel tile')
    if c_in % 8:
        edges.add('c_in not a multiple of 8')
    if g.c8 % 4:
        edges.add('c8 not a multiple of 4')
    if g.entries % 4:
        edges.add('partial last K block')
    if form in SPLITK_FORMS and 3 * cdiv(g.n_kb, 4) >= g.n_kb:
        edges.add('idle split-K wave')
    if g.n_kb < K_DEPTH:
        edges.add('n_kb < kDepth')
    if batch > 1 and any((b * g.Ho * g.Wo) % 16 for b in range(1, batch)):
        edges.add('tiles straddle images')
        if batch == 3:
            edges.add('batch 3, tiles straddle images')
    if not up and stride == 2 and h % 2 and w % 2:
        edges.add('stride 2 on odd sizes')
    if not up and k > 1 and dil >= max(h, w):
        edges.add('dilation >= image')
    edges.add('group of %d' % members)
    edges.add('S = %d' % pred.smap[0])
    if pred.smap[2] % 8:
        edges.add('V not a multiple of 8')
    return edges


# every plain and split-K form shows each of these in one of its rows ...
EDGES_PER_FORM = ('c_out partial group of 4', 'c_out partial 16-tile', 'ragged pixel tile', 'c_in not a multiple of 8', 'c8 not a multiple of 4',
                  'partial last K block', 'batch 3, tiles straddle images', 'stride 2 on odd sizes')
# ... the split-K forms whose K range allows it (<4,2,1,4> starts at 32 K blocks, where every wave owns some) an idle wave ...
IDLE_WAVE_FORMS = ('<1,1,1,4>', '<2,1,1,4>', '<4,1,1,4>')
# ... the GEMM tiles only what the dropout table does not give them (the unaligned epilogue runs on every row) ...
EDGES_PER_GEMM_FORM = ('tiles straddle images', 'ragged pixel tile', 'c_out partial group of 4')
# ... and the table as a whole these
EDGES_ANYWHERE = ('n_ct padded', 'n_kb < kDepth', 'dilation >= image', 'group of 1', 'group of 2', 'group of 3', 'group of 6', 'S = 1', 'S = 2', 'S = 4',
                  'S = 8', 'V not a multiple of 8')

# (name, c_in, c_out, k, stride, dilation, padding, H, W, batch, members, form): the smallest layers that reach each form; what
# a row carries is computed by row_edges (the name says what it was picked for)
FORM_TABLE = [
    ('p421_kb1_group6', 12, 5, 1, 1, 1, 0, 7, 9, 1, 6, '<4,2,1,1>'),            # one K block of two entries, one ragged block
    ('p421_s2_odd_batch3', 6, 30, 3, 2, 1, 1, 13, 11, 3, 1, '<4,2,1,1>'),
    ('p412_c70', 20, 70, 1, 1, 1, 0, 29, 28, 1, 1, '<4,1,2,1>'),                # 70 channels: five 16-tiles in two 64-groups
    ('p412_s2_odd_batch3_pair', 20, 70, 1, 2, 1, 0, 33, 35, 3, 2, '<4,1,2,1>'),
    ('p422_batch2_group3', 20, 70, 1, 1, 1, 0, 11, 13, 2, 3, '<4,2,2,1>'),
    ('p422_5x5_s3_d2', 8, 72, 5, 3, 2, 4, 33, 17, 1, 1, '<4,2,2,1>'),
    ('p422_s2_odd_batch3_pair', 12, 70, 3, 2, 1, 1, 13, 11, 3, 2, '<4,2,2,1>'),
    ('k1_last_block_of_one', 36, 30, 3, 1, 1, 1, 7, 9, 1, 1, '<1,1,1,4>'),      # 45 entries: the last K block holds one
    ('k1_idle_wave_pair', 32, 30, 3, 1, 1, 1, 7, 9, 1, 2, '<1,1,1,4>'),         # n_kb 9: wave 3 owns nothing
    ('k1_s2_odd_d3_batch3', 36, 5, 3, 2, 3, 3, 9, 13, 3, 1, '<1,1,1,4>'),
    ('k1_dilation_16_on_7x9_group3', 40, 30, 3, 1, 16, 16, 7, 9, 1, 3, '<1,1,1,4>'),  # only the centre tap lands
    ('k2_c70', 68, 70, 3, 1, 1, 1, 23, 27, 1, 1, '<2,1,1,4>'),
    ('k2_s2_odd_batch3', 72, 70, 3, 2, 1, 1, 29, 27, 3, 1, '<2,1,1,4>'),
    ('k2_idle_wave', 32, 70, 3, 1, 1, 1, 23, 27, 1, 1, '<2,1,1,4>'),
    ('k4_last_block_of_one', 36, 30, 3, 1, 1, 1, 41, 59, 1, 1, '<4,1,1,4>'),
    ('k4_s2_odd_pair', 72, 37, 3, 2, 1, 1, 97, 101, 1, 2, '<4,1,1,4>'),
    ('k4_idle_wave_batch3', 32, 30, 3, 1, 1, 1, 29, 28, 3, 1, '<4,1,1,4>'),
    ('k42_3x3', 116, 30, 3, 1, 1, 1, 53, 91, 1, 1, '<4,2,1,4>'),
    ('k42_1x1_s2_odd_batch3', 1000, 37, 1, 2, 1, 0, 79, 81, 3, 1, '<4,2,1,4>'),
    # the GEMM tiles: what the dropout table does not give them - the unaligned epilogue, a tile across two images
    ('gemm64_batch2_pair', 12, 30, 3, 1, 1, 1, 45, 45, 2, 2, 'gemm 64x64'),
    ('gemm64_aligned_batch2_pair', 32, 30, 3, 1, 1, 1, 45, 45, 2, 2, 'gemm 64x64'),  # c8 a multiple of 4: the scalar tap walk (ALIGNED)
    ('gemm128_batch2_pair', 12, 250, 3, 1, 1, 1, 65, 63, 2, 2, 'gemm 128x128'),
    ('gemm128x160_batch2_pair', 12, 250, 3, 1, 1, 1, 65, 65, 2, 2, 'gemm 128x160'),
    ('gemm128x80_batch2_pair', 228, 118, 3, 1, 1, 1, 65, 65, 2, 2, 'gemm 128x80'),
]

# transposed convolutions (SegDeconv: kernel 2s, stride s, padding s / 2), same layout + the stride s; k / stride / dilation /
# padding are unused.  c_out not a multiple of 4: the padded rows of every phase are skipped (co >= n_co)
DECONV_TABLE = [
    ('deconv_s2_plain', 16, 5, 0, 0, 0, 0, 5, 3, 1, 1, '<4,2,1,1>', 2),
    ('deconv_s4_splitk_batch2', 40, 6, 0, 0, 0, 0, 9, 7, 2, 1, '<1,1,1,4>', 4),
    ('deconv_s8_plain', 16, 5, 0, 0, 0, 0, 4, 6, 1, 1, '<4,2,2,1>', 8),
    ('deconv_s2_gemm_batch2', 40, 62, 0, 0, 0, 0, 30, 40, 2, 1, 'gemm 64x64', 2),
]

# segconv.multi member lists: (name, [(c_in, c_out, k, stride, dilation, padding, H, W, epilogue), ...], form).  Members of
# different pixel and channel counts: the grid holds blocks beyond a member's own channel / pixel blocks, which must exit
MULTI_TABLE = [
    ('multi_plain', [(12, 5, 1, 1, 1, 0, 7, 9, 'plain'), (20, 70, 1, 1, 1, 0, 11, 13, 'res_relu'), (6, 30, 3, 2, 1, 1, 13, 11, 'sigmoid_mul'),
                     (8, 72, 5, 3, 2, 4, 33, 17, 'plain')], 'multi<4,2,2,1>'),
    ('multi_k1', [(40, 30, 3, 1, 1, 1, 7, 9, 'res_relu'), (32, 70, 3, 1, 1, 1, 5, 7, 'plain'), (72, 5, 3, 1, 2, 2, 9, 11, 'sigmoid_mul')], 'multi<1,1,1,4>'),
    ('multi_k2', [(72, 70, 3, 1, 1, 1, 23, 27, 'plain'), (40, 30, 3, 1, 1, 1, 7, 9, 'sigmoid_mul'), (32, 37, 3, 1, 1, 1, 11, 13, 'res_relu')], 'multi<2,1,1,4>'),
    ('multi_k4', [(40, 30, 3, 1, 1, 1, 41, 59, 'sigmoid_mul'), (72, 70, 3, 1, 1, 1, 9, 11, 'res_relu'), (32, 5, 3, 1, 3, 3, 5, 7, 'plain')], 'multi<4,1,1,4>'),
    # a split-K member next to a plain one: the forms differ in what a block is - separate launches
    ('multi_mixed', [(40, 30, 3, 1, 1, 1, 7, 9, 'res_relu'), (12, 70, 1, 1, 1, 0, 11, 13, 'plain')], 'separate'),
    # members large enough for the GEMM-shaped form (kMultiOwnMinKb / kMultiOwnMinBlocks) keep a launch of their own
    ('multi_large_pair', [(20, 30, 3, 1, 1, 1, 128, 128, 'res_relu'), (20, 30, 3, 1, 1, 1, 128, 128, 'res_relu'), (12, 70, 1, 1, 1, 0, 11, 13, 'plain')], 'separate'),
]


# ---- where the caller-owned rows of placement (b) lie ---------------------------------------------------------------------
# kind -> (first channel of the slice, channels of the buffer beyond round_up(first + c, 4)): a channel slice [first, first + c)
# of a wider NHWC buffer of sentinels.  'ptr1' / 'ptr3': the row stride is a multiple of 4 and the pointer is not 16-byte
# aligned; 'stride': the row stride is no multiple of 4.  Every buffer keeps at least 4 channels behind the slice.
SLICE_KINDS = {'aligned': (4, 8), 'ptr1': (1, 4), 'ptr3': (3, 4), 'stride': (2, 5)}
SENTINEL = -7.25e11


def slice_geometry(kind, c):
    """(first channel, buffer channels) of a slice of ``c`` channels."""
    lo, extra = SLICE_KINDS[kind]
    return lo, round_up(lo + c, 4) + extra


def rows_aligned(kind, c):
    """seg_fill's test on such rows (the buffer itself is 16-byte aligned): float4 accesses allowed."""
    lo, cb = slice_geometry(kind, c)
    return cb % 4 == 0 and (lo * 4) % 16 == 0


# (epilogue, kind of the output rows, of the residual rows, of the gate rows): every vec_store bit cleared alone, and all three
PLACEMENTS = [('plain', 'ptr1', None, None), ('res_relu', 'stride', 'aligned', None), ('res_relu', 'aligned', 'ptr3', None),
              ('sigmoid_mul', 'aligned', None, 'stride'), ('res_sigmoid_mul', 'ptr3', 'stride', 'ptr1')]
DECONV_PLACEMENTS = [('plain', 'ptr1'), ('relu', 'stride'), ('relu', 'ptr3')]


def cleared_bits(placement, c):
    """The vec_store bits (1 output, 2 residual, 4 gate) the placement clears among those its epilogue uses."""
    return sum(bit for bit, kind in zip((1, 2, 4), placement[1:]) if kind is not None and not rows_aligned(kind, c))
