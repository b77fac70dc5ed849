"""The training kernels' frame-dependent decisions, restated in plain Python, and the rows that pin them.

csrc/ojf_train_kernels.h and csrc/ojf_train.hip cut a frame of npix = h * w pixels in seven ways; each is restated here without the
package (tests/test_train_edges_host.py reads the constants back from the sources and checks the two C entries that expose a plan):

  stats_plan     train_stats_partial_body, train_bn_bwd_reduce_kernel, ojf_train_channel_sums: 64 slabs of ceil(npix / 64) pixels,
                 256 lanes per slab, an unrolled loop of four loads (p + 768 < p1, step 1024) and a tail loop (step 256)
  stream_plan    train_bn_act_fwd_kernel, train_bn_bwd_apply_kernel: min(ceil(npix / 256), 128) blocks, three hoisted loads
                 ("first3"), a three-way middle loop and a tail loop
  wgrad_plan     train_wgrad_mfma_kernel: pixel slabs of even length, 64-pixel chunks, 32 x 32 (oc, ic) tiles, taps outside the image
  pool_plan      train_avgpool3_kernel: min(ceil(npix / 256), 256) blocks in a grid-stride loop
  pyramid_plan   train_pyramid_kernel: 32 x 8 tiles with LDS halos of up to three pixels
  px_plan        the one-thread-per-pixel kernels (px_grid)
  loss_plan      train_loss_partial_kernel / train_loss_finish_kernel: 256 rows per block, 64 finishing lanes

EDGE_ROWS names, per row, the edges it claims; the host test computes every claim from these functions.  The rows' inputs are zero-mean
(+-U(0.5, 1.5)) so that one dropped pixel moves a per-channel sum by ~1 / sqrt(npix) of its scale and not by 1 / npix, and the pixels
where the restatement puts a boundary (sentinels) are eight times larger."""
import collections

# ---- constants of the sources (checked by test_restated_constants_are_the_sources) -----------------------------------------------
TRAIN_SLABS = 64          # kTrainSlabs
BLOCK = 256               # threads of the reduction / streaming / per-pixel blocks
UNROLL_LAST = 768         # `p + 768 < p1`: the fourth load of an unrolled iteration
UNROLL_STEP = 1024        # `p += 1024`
STREAM_MAX_BX = 128       # bx = min(ceil(npix / 256), 128)
WG_CHUNK = 64             # kWgChunk
WG_WAVES = 2048           # wgrad_plan: slabs = ceil(2048 / waves) ...
WG_MAX_SLABS = 256        # ... at most 256 ...
WG_TILE = 32              # ... of 32 x 32 (oc, ic) tiles
POOL_MAX_BX = 256         # ojf_train_avgpool3
TP_W, TP_H = 32, 8        # kTpW, kTpH
TP_LEVELS = 3             # branch i of a VortexPooling sees i pools: halos 1..3
LOSS_THREADS = 256        # kLossThreads
LOSS_FINISH_LANES = 64    # train_loss_finish_kernel


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(a, b):
    return cdiv(a, b) * b


# ---- reductions -------------------------------------------------------------------------------------------------------------------
def lane_iterations(length, lane):
    """-> (unrolled iterations, tail iterations) of one lane over a slab of `length` pixels"""
    unrolled = 0 if lane + UNROLL_LAST >= length else (length - UNROLL_LAST - 1 - lane) // UNROLL_STEP + 1
    p = lane + UNROLL_STEP * unrolled
    return unrolled, (cdiv(length - p, BLOCK) if p < length else 0)


def slab_forms(length):
    """how the 256 lanes of a block walk a slab of `length` pixels"""
    f = dict(unrolled0=0, unrolled1=0, unrolled2plus=0, tail=0, tail2plus=0, idle=0, unrolled_without_tail=0)
    for lane in range(BLOCK):
        u, t = lane_iterations(length, lane)
        f['unrolled0' if u == 0 else 'unrolled1' if u == 1 else 'unrolled2plus'] += 1
        f['tail'] += t > 0
        f['tail2plus'] += t > 1
        f['idle'] += u == 0 and t == 0
        f['unrolled_without_tail'] += u > 0 and t == 0
    return f


def stats_plan(npix):
    per = cdiv(npix, TRAIN_SLABS)
    nonempty = min(TRAIN_SLABS, cdiv(npix, per))
    last_len = npix - (nonempty - 1) * per
    return dict(per=per, nonempty=nonempty, last_len=last_len, full=slab_forms(per), last=slab_forms(last_len))


def stats_pixel(npix, p):
    """-> (slab, lane, loop form, iteration) of pixel p: form is 'unrolled load u' or 'tail'"""
    per = cdiv(npix, TRAIN_SLABS)
    slab = p // per
    length = min(npix, (slab + 1) * per) - slab * per
    o = p - slab * per
    lane, k = o % BLOCK, o // BLOCK
    u, _ = lane_iterations(length, lane)
    if k < 4 * u:
        return slab, lane, 'unrolled load %d' % (k % 4), k // 4
    return slab, lane, 'tail', k - 4 * u


R_ONE = 'reduce: one pixel'
R_EMPTY = 'reduce: empty trailing slabs'
R_ONE_EACH = 'reduce: 64 slabs of one pixel'
R_RAGGED = 'reduce: last slab shorter than the others'
R_IDLE = 'reduce: lanes without a pixel'
R_FULL_BLOCK = 'reduce: slab of exactly 256 pixels'
R_TAIL2 = 'reduce: second tail iteration for the first lanes only'
R_UNROLLED = 'reduce: unrolled loop'
R_MIXED = 'reduce: unrolled and tail-only lanes in one block'
R_UNROLLED2 = 'reduce: two unrolled iterations'
R_UNROLLED_THEN_TAIL = 'reduce: tail iterations after an unrolled one'
REDUCE_EDGES = [R_ONE, R_EMPTY, R_ONE_EACH, R_RAGGED, R_IDLE, R_FULL_BLOCK, R_TAIL2, R_UNROLLED, R_MIXED, R_UNROLLED2, R_UNROLLED_THEN_TAIL]


def reduce_edges(npix):
    s, e = stats_plan(npix), set()
    f = s['full']
    if npix == 1: e.add(R_ONE)
    if s['nonempty'] < TRAIN_SLABS: e.add(R_EMPTY)
    if s['per'] == 1 and s['nonempty'] == TRAIN_SLABS: e.add(R_ONE_EACH)
    if s['last_len'] < s['per']: e.add(R_RAGGED)
    if f['idle']: e.add(R_IDLE)
    if s['per'] == BLOCK: e.add(R_FULL_BLOCK)
    if 0 < f['tail2plus'] < BLOCK and not f['unrolled1']: e.add(R_TAIL2)
    if f['unrolled1'] or f['unrolled2plus']: e.add(R_UNROLLED)
    if (f['unrolled1'] or f['unrolled2plus']) and f['unrolled0']: e.add(R_MIXED)
    if f['unrolled2plus']: e.add(R_UNROLLED2)
    if any(u and t for u, t in (lane_iterations(s['per'], lane) for lane in range(BLOCK))): e.add(R_UNROLLED_THEN_TAIL)
    return e


def reduce_sentinels(npix):
    """pixel -> labels: the frame's ends, the ends of the first, a middle and the last non-empty slab, and in the middle slab the
    first pixel of each loop form"""
    s = stats_plan(npix)
    per, last = s['per'], s['nonempty'] - 1
    out = collections.OrderedDict()

    def mark(p, label):
        if 0 <= p < npix:
            out.setdefault(p, []).append(label)
    mark(0, 'first pixel of the frame')
    mark(npix - 1, 'last pixel of the frame')
    for slab, name in ((0, 'first slab'), (last // 2, 'middle slab'), (last, 'last non-empty slab')):
        p0, p1 = slab * per, min(npix, (slab + 1) * per)
        mark(p0, 'first pixel of the ' + name)
        mark(p1 - 1, 'last pixel of the ' + name)
    mid = (last // 2) * per
    seen = set()
    for p in range(mid, min(npix, mid + per)):
        form = stats_pixel(npix, p)[2:]
        if form not in seen:
            seen.add(form)
            mark(p, 'first pixel of %s, iteration %d' % form)
    return out


# ---- streaming loops --------------------------------------------------------------------------------------------------------------
def stream_thread(npix, stride, t):
    """-> (first3, middle iterations, tail iterations) of the thread that starts at pixel t"""
    first3 = t + 2 * stride < npix
    p, middle = t, 0
    if first3:
        p += 3 * stride
        while p + 2 * stride < npix:
            p += 3 * stride
            middle += 1
    return first3, middle, (cdiv(npix - p, stride) if p < npix else 0)


def stream_plan(npix):
    bx = min(cdiv(npix, BLOCK), STREAM_MAX_BX)
    stride = BLOCK * bx
    first3 = max(0, min(stride, npix - 2 * stride))
    # the middle loop's first iteration needs t + 5 stride < npix, its second t + 8 stride < npix
    middle = [max(0, min(stride, npix - (2 + 3 * k) * stride)) for k in (1, 2)]
    return dict(bx=bx, stride=stride, first3=first3, middle=middle[0], middle2=middle[1], last_block=npix - BLOCK * (cdiv(npix, BLOCK) - 1))


def stream_tail_threads(npix):
    """how many threads run at least one iteration of the tail loop"""
    stride = stream_plan(npix)['stride']
    return sum(stream_thread(npix, stride, t)[2] > 0 for t in range(stride))


def stream_pixel(npix, p):
    stride = stream_plan(npix)['stride']
    t, k = p % stride, p // stride
    first3, middle, _ = stream_thread(npix, stride, t)
    if first3 and k < 3:
        return t, 'first3 load %d' % k
    if first3 and k < 3 * (1 + middle):
        return t, 'middle loop load %d' % (k % 3)
    return t, 'tail loop'


S_PARTIAL_BLOCK = 'stream: one partial block'
S_FULL_GRID = 'stream: 128 full blocks, one iteration, no first3'
S_NO_FIRST3_MAX = 'stream: the largest frame without first3'
S_FIRST3_SOME = 'stream: first3 for the first threads only'
S_FIRST3_ALL = 'stream: first3 for every thread'
S_MIDDLE_NONE = 'stream: first3 for every thread, middle loop for none'
S_MIDDLE_SOME = 'stream: middle loop for the first threads only'
S_TAIL_AFTER_FIRST3 = 'stream: tail iterations after first3'
S_GRID_STRIDE = 'stream: threads without first3 run the tail loop twice or more'
STREAM_EDGES = [S_PARTIAL_BLOCK, S_FULL_GRID, S_NO_FIRST3_MAX, S_FIRST3_SOME, S_FIRST3_ALL, S_MIDDLE_NONE, S_MIDDLE_SOME, S_TAIL_AFTER_FIRST3, S_GRID_STRIDE]


def stream_edges(npix):
    s, e = stream_plan(npix), set()
    if npix < BLOCK: e.add(S_PARTIAL_BLOCK)
    if npix == BLOCK * STREAM_MAX_BX: e.add(S_FULL_GRID)
    if npix == 2 * BLOCK * STREAM_MAX_BX: e.add(S_NO_FIRST3_MAX)
    if 0 < s['first3'] < s['stride']: e.add(S_FIRST3_SOME)
    if s['first3'] == s['stride']: e.add(S_FIRST3_ALL)
    if s['first3'] == s['stride'] and not s['middle']: e.add(S_MIDDLE_NONE)
    if 0 < s['middle'] < s['stride']: e.add(S_MIDDLE_SOME)
    if s['first3'] and stream_thread(npix, s['stride'], 0)[2]: e.add(S_TAIL_AFTER_FIRST3)
    last = stream_thread(npix, s['stride'], s['stride'] - 1)
    if not last[0] and last[2] > 1: e.add(S_GRID_STRIDE)
    return e


# ---- weight gradient --------------------------------------------------------------------------------------------------------------
def wgrad_plan(c_out_phys, c_in_phys, taps, npix, units=1):
    ocp, icp = round_up(c_out_phys, WG_TILE), round_up(c_in_phys, WG_TILE)
    waves = units * taps * (ocp // WG_TILE) * (icp // WG_TILE)
    slabs = max(1, min(cdiv(WG_WAVES, waves), WG_MAX_SLABS, cdiv(npix, WG_CHUNK)))
    per = (cdiv(npix, slabs) + 1) & ~1  # the kernel's: even, a K step of two pixels never straddles two slabs
    nonempty = min(slabs, cdiv(npix, per))
    last_len = npix - (nonempty - 1) * per
    n_ot, n_it = ocp // WG_TILE, icp // WG_TILE
    return dict(ocp=ocp, icp=icp, slabs=slabs, per=per, nonempty=nonempty, empty=slabs - nonempty, last_len=last_len,
                chunks=cdiv(per, WG_CHUNK), last_chunk=per - WG_CHUNK * (cdiv(per, WG_CHUNK) - 1),
                chunks_last_slab=cdiv(last_len, WG_CHUNK), last_chunk_last_slab=last_len - WG_CHUNK * (cdiv(last_len, WG_CHUNK) - 1),
                n_ot=n_ot, n_it=n_it, n_og_last=min(8, c_out_phys // 4 - (n_ot - 1) * 8), n_ig_last=min(8, c_in_phys // 4 - (n_it - 1) * 8),
                limited_by='pixels' if slabs == cdiv(npix, WG_CHUNK) else ('maximum' if slabs == WG_MAX_SLABS else 'waves'),
                partial_floats=slabs * taps * ocp * icp)


def tap_offsets(ksize, dil):
    return [((t // 3 - 1) * dil, (t % 3 - 1) * dil) for t in range(9)] if ksize == 3 else [(0, 0)]


def taps_inside(ksize, dil, h, w):
    """per tap: does any pixel of the frame see it inside the image"""
    return [abs(dy) < h and abs(dx) < w for dy, dx in tap_offsets(ksize, dil)]


W_ONE_SLAB = 'wgrad: one slab'
W_MAX_SLABS = 'wgrad: 256 slabs'
W_BY_PIXELS = 'wgrad: slab count limited by ceil(npix / 64)'
W_BY_WAVES = 'wgrad: slab count from the 2048-wave target'
W_EMPTY = 'wgrad: empty trailing slabs'
W_PARTIAL_CHUNK = 'wgrad: partial last chunk'
W_SHORT_SLAB = 'wgrad: slab shorter than a chunk'
W_CHUNKS = 'wgrad: several chunks per slab'
W_HALF_STEP = 'wgrad: last K step half padding'
W_ROUNDED_PER = 'wgrad: slab length rounded up to even'
W_RAGGED_SLAB = 'wgrad: last non-empty slab shorter than the others'
W_EVEN = 'wgrad: even frame, slab length needs no rounding, last K step full'
W_LAST_CHUNK_1 = 'wgrad: the third chunk of a single slab holds one pixel'
W_LAST_CHUNK_2 = 'wgrad: the third chunk of a single slab holds two pixels'
W_TAPS_OUT = 'wgrad: taps outside the image for every pixel'
W_CENTRE_ONLY = 'wgrad: every off-centre tap outside'
W_TAPS_PARTLY = 'wgrad: taps inside for some pixels only'
W_OG_SHORT = 'wgrad: fewer than 8 dy groups in the last oc tile'
W_IG_SHORT = 'wgrad: fewer than 8 x groups in the last ic tile'
W_OC_TILES = 'wgrad: several oc tiles'
W_IC_TILES = 'wgrad: several ic tiles'
W_SLOTTED = 'wgrad: several input slots with padding channels'
W_ACCUMULATE = 'wgrad: accumulate onto a non-zero dW'
WGRAD_EDGES = [W_ONE_SLAB, W_MAX_SLABS, W_BY_PIXELS, W_BY_WAVES, W_EMPTY, W_PARTIAL_CHUNK, W_SHORT_SLAB, W_CHUNKS, W_HALF_STEP, W_ROUNDED_PER,
               W_RAGGED_SLAB, W_EVEN, W_LAST_CHUNK_1, W_LAST_CHUNK_2, W_TAPS_OUT, W_CENTRE_ONLY, W_TAPS_PARTLY, W_OG_SHORT, W_IG_SHORT, W_OC_TILES, W_IC_TILES, W_SLOTTED, W_ACCUMULATE]


def wgrad_edges(c_out_phys, c_in_phys, ksize, dil, h, w, units=1, group=None, slot=None, IC=None, accumulate=0):
    npix = h * w
    p, e = wgrad_plan(c_out_phys, c_in_phys, ksize * ksize, npix, units), set()
    if p['slabs'] == 1: e.add(W_ONE_SLAB)
    if p['slabs'] == WG_MAX_SLABS: e.add(W_MAX_SLABS)
    if p['limited_by'] == 'pixels': e.add(W_BY_PIXELS)
    if p['limited_by'] == 'waves': e.add(W_BY_WAVES)
    if p['empty']: e.add(W_EMPTY)
    if p['last_chunk'] < WG_CHUNK or p['last_chunk_last_slab'] < WG_CHUNK: e.add(W_PARTIAL_CHUNK)
    if p['per'] < WG_CHUNK: e.add(W_SHORT_SLAB)
    if p['chunks'] > 1: e.add(W_CHUNKS)
    if p['last_len'] % 2: e.add(W_HALF_STEP)
    if p['per'] != cdiv(npix, p['slabs']): e.add(W_ROUNDED_PER)
    if p['last_len'] < p['per']: e.add(W_RAGGED_SLAB)
    if p['per'] == cdiv(npix, p['slabs']) and p['last_len'] % 2 == 0 and npix % 2 == 0: e.add(W_EVEN)
    if p['slabs'] == 1 and p['chunks'] == 3 and p['last_chunk_last_slab'] == 1: e.add(W_LAST_CHUNK_1)
    if p['slabs'] == 1 and p['chunks'] == 3 and p['last_chunk_last_slab'] == 2: e.add(W_LAST_CHUNK_2)
    inside = taps_inside(ksize, dil, h, w)
    if not all(inside): e.add(W_TAPS_OUT)
    if ksize == 3 and sum(inside) == 1: e.add(W_CENTRE_ONLY)
    if ksize == 3 and any(inside[t] and (dy or dx) for t, (dy, dx) in enumerate(tap_offsets(3, dil))): e.add(W_TAPS_PARTLY)
    if p['n_og_last'] < 8: e.add(W_OG_SHORT)
    if p['n_ig_last'] < 8: e.add(W_IG_SHORT)
    if p['n_ot'] > 1: e.add(W_OC_TILES)
    if p['n_it'] > 1: e.add(W_IC_TILES)
    if group and slot and slot > group and IC and IC > group: e.add(W_SLOTTED)
    if accumulate: e.add(W_ACCUMULATE)
    return e


def wgrad_pixel(plan, p):
    slab = p // plan['per']
    o = p - slab * plan['per']
    return slab, o // WG_CHUNK, o % WG_CHUNK


def wgrad_sentinels(plan, npix):
    """pixel -> labels: the frame's ends; the ends of the first, a middle and the last non-empty slab; the first pixel of a slab's
    second chunk and the last pixel of its last (partial) chunk"""
    per, last = plan['per'], plan['nonempty'] - 1
    out = collections.OrderedDict()

    def mark(p, label):
        if 0 <= p < npix:
            out.setdefault(p, []).append(label)
    mark(0, 'first pixel of the frame')
    mark(npix - 1, 'last pixel of the frame')
    for slab, name in ((0, 'first slab'), (last // 2, 'middle slab'), (last, 'last non-empty slab')):
        p0, p1 = slab * per, min(npix, (slab + 1) * per)
        mark(p0, 'first pixel of the ' + name)
        mark(p1 - 1, 'last pixel of the %s (chunk %d, lane %d)' % ((name,) + wgrad_pixel(plan, p1 - 1)[1:]))
        if p1 - p0 > WG_CHUNK:
            mark(p0 + WG_CHUNK - 1, 'last pixel of the first chunk of the ' + name)
            mark(p0 + WG_CHUNK, 'first pixel of the second chunk of the ' + name)
    return out


# ---- the small launches -----------------------------------------------------------------------------------------------------------
def pool_plan(npix):
    bx = min(cdiv(npix, BLOCK), POOL_MAX_BX)
    return dict(bx=bx, iterations=cdiv(npix, BLOCK * bx), last_block=npix - BLOCK * (cdiv(npix, BLOCK) - 1))


P_ONE_PIXEL = 'avgpool3: one pixel, every neighbour outside'
P_ONE_ROW = 'avgpool3: one row'
P_ONE_COLUMN = 'avgpool3: one column'
P_NO_INTERIOR = 'avgpool3: no pixel with all nine neighbours'
P_GRID_STRIDE = 'avgpool3: grid-stride loop iterates twice for the first threads only'
POOL_EDGES = [P_ONE_PIXEL, P_ONE_ROW, P_ONE_COLUMN, P_NO_INTERIOR, P_GRID_STRIDE]


def pool_edges(h, w):
    p, e = pool_plan(h * w), set()
    if h * w == 1: e.add(P_ONE_PIXEL)
    if h == 1 and w > 1: e.add(P_ONE_ROW)
    if w == 1 and h > 1: e.add(P_ONE_COLUMN)
    if h < 3 or w < 3: e.add(P_NO_INTERIOR)
    if p['iterations'] == 2 and h * w < 2 * BLOCK * p['bx']: e.add(P_GRID_STRIDE)
    return e


def pyramid_plan(h, w):
    tx, ty = cdiv(w, TP_W), cdiv(h, TP_H)
    return dict(tiles_x=tx, tiles_y=ty, last_w=w - TP_W * (tx - 1), last_h=h - TP_H * (ty - 1),
                halo_beyond_frame=[lv for lv in range(1, TP_LEVELS + 1) if lv >= min(h, w)])


def px_plan(npix):
    return dict(blocks=cdiv(npix, BLOCK), last_block=npix - BLOCK * (cdiv(npix, BLOCK) - 1))


X_BELOW_TILE = 'pyramid: frame inside one ragged tile'
X_ONE_TILE = 'pyramid: exactly one tile'
X_ONE_OVER = 'pyramid: one pixel over a tile each way'
X_MANY_RAGGED = 'pyramid: three tiles each way, the last one pixel wide and high'
X_HALO1 = 'pyramid: the one-pixel halo reaches beyond a one-pixel frame side'
X_HALO3 = 'pyramid: the three-pixel halo reaches beyond the frame'
X_PX_PARTIAL = 'px_grid: one partial block'
X_PX_ONE = 'px_grid: one full block'
X_PX_MANY = 'px_grid: several blocks, partial last'
X_WG_SHORT = W_SHORT_SLAB + ' (executor)'
X_WG_HALF = W_HALF_STEP + ' (executor)'
X_WG_CENTRE = W_CENTRE_ONLY + ' (executor, dilation 27)'
X_R_EMPTY = R_EMPTY + ' (executor)'
EXECUTOR_EDGES = [X_BELOW_TILE, X_ONE_TILE, X_ONE_OVER, X_MANY_RAGGED, X_HALO1, X_HALO3, X_PX_PARTIAL, X_PX_ONE, X_PX_MANY, X_WG_SHORT, X_WG_HALF,
                  X_WG_CENTRE, X_R_EMPTY]
EXECUTOR_UNIT_SHAPES = [(20, 20, 3, 27, 4), (20, 116, 1, 1, 4), (116, 20, 1, 1, 1)]  # (c_out_phys, c_in_phys, k, dil, units) of a VortexPooling


def executor_edges(h, w):
    npix, y, x, e = h * w, pyramid_plan(h, w), px_plan(h * w), set()
    if y['tiles_x'] == 1 and y['tiles_y'] == 1 and (y['last_w'] < TP_W or y['last_h'] < TP_H): e.add(X_BELOW_TILE)
    if (h, w) == (TP_H, TP_W): e.add(X_ONE_TILE)
    if (h, w) == (TP_H + 1, TP_W + 1): e.add(X_ONE_OVER)
    if (y['tiles_x'], y['tiles_y'], y['last_w'], y['last_h']) == (3, 3, 1, 1): e.add(X_MANY_RAGGED)
    if 1 in y['halo_beyond_frame']: e.add(X_HALO1)
    if 3 in y['halo_beyond_frame']: e.add(X_HALO3)
    if x['blocks'] == 1 and x['last_block'] < BLOCK: e.add(X_PX_PARTIAL)
    if x['blocks'] == 1 and x['last_block'] == BLOCK: e.add(X_PX_ONE)
    if x['blocks'] > 1 and x['last_block'] < BLOCK: e.add(X_PX_MANY)
    for cop, cip, k, dil, units in EXECUTOR_UNIT_SHAPES:
        we = wgrad_edges(cop, cip, k, dil, h, w, units)
        if W_SHORT_SLAB in we: e.add(X_WG_SHORT)
        if W_HALF_STEP in we: e.add(X_WG_HALF)
        if W_CENTRE_ONLY in we and dil == 27: e.add(X_WG_CENTRE)
    if R_EMPTY in reduce_edges(npix): e.add(X_R_EMPTY)
    return e


def loss_plan(n_valid):
    blocks = cdiv(n_valid, LOSS_THREADS)
    return dict(blocks=blocks, last_block=n_valid - LOSS_THREADS * (blocks - 1), finish_iterations=cdiv(blocks, LOSS_FINISH_LANES))


L_ONE_ROW = 'loss: one row'
L_PARTIAL = 'loss: one partial block'
L_FULL = 'loss: exactly one block'
L_ONE_OVER = 'loss: a second block of one row'
L_FINISH2 = 'loss: a finishing lane adds two blocks'
LOSS_EDGES = [L_ONE_ROW, L_PARTIAL, L_FULL, L_ONE_OVER, L_FINISH2]


def loss_edges(n_valid):
    p, e = loss_plan(n_valid), set()
    if n_valid == 1: e.add(L_ONE_ROW)
    if p['blocks'] == 1 and 1 < p['last_block'] < LOSS_THREADS: e.add(L_PARTIAL)
    if p['blocks'] == 1 and p['last_block'] == LOSS_THREADS: e.add(L_FULL)
    if p['blocks'] == 2 and p['last_block'] == 1: e.add(L_ONE_OVER)
    if p['finish_iterations'] > 1: e.add(L_FINISH2)
    return e


# ---- ojf_train_conv: chunks of 8 output tiles of 16 channels ------------------------------------------------------------------------
def conv_plan(c_out_phys):
    n_ot = round_up(cdiv(c_out_phys, 16), 2)
    og_total = cdiv(c_out_phys, 4)
    launches = [(ot0, min(8, n_ot - ot0), min(og_total - ot0 * 4, 4 * min(8, n_ot - ot0))) for ot0 in range(0, n_ot, 8)]
    return dict(n_ot=n_ot, launches=launches)  # (first tile, tiles, og_store) per launch


C_ONE_PIXEL = 'conv: one pixel, every off-centre tap outside'
C_ONE_ROW = 'conv: one row'
C_ONE_COLUMN = 'conv: one column'
C_TINY = 'conv: frame smaller than the dilation'
C_SECOND_LAUNCH = 'conv: second 8-tile chunk, og_store below its tiles'
C_TRANSPOSED = 'conv: transposed form (backward-data)'
CONV_EDGES = [C_ONE_PIXEL, C_ONE_ROW, C_ONE_COLUMN, C_TINY, C_SECOND_LAUNCH, C_TRANSPOSED]


def conv_edges(c_out_phys, ksize, dil, h, w):
    e, p = {C_TRANSPOSED}, conv_plan(c_out_phys)  # every conv row runs both forms
    if h * w == 1: e.add(C_ONE_PIXEL)
    if h == 1 and w > 1: e.add(C_ONE_ROW)
    if w == 1 and h > 1: e.add(C_ONE_COLUMN)
    if ksize == 3 and dil >= h and dil >= w and h * w > 1: e.add(C_TINY)
    if len(p['launches']) > 1 and p['launches'][-1][2] < 4 * p['launches'][-1][1]: e.add(C_SECOND_LAUNCH)
    return e


G_WINDOWS = 'windows: every *_g0 non-zero and distinct, NaN outside'
G_PLAIN = 'windows: every *_g0 zero'

# ---- the rows ---------------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple('Row', 'name kind p claims')


def _bn(name, h, w, claims, C=6, windows=True, modes=('train', 'eval'), y_scale=1.0):
    return Row(name, 'bn', dict(h=h, w=w, C=C, windows=windows, modes=modes, y_scale=y_scale), tuple(claims) + ((G_WINDOWS,) if windows else (G_PLAIN,)))


def _wg(name, h, w, cop, cip, k, dil, claims, group=None, slot=None, IC=None, accumulate=0, windows=True):
    IC = IC if IC is not None else cip - 1
    group, slot = (group, slot) if group else (IC, cip)
    return Row(name, 'wgrad', dict(h=h, w=w, cop=cop, cip=cip, OC=cop - 1, IC=IC, k=k, dil=dil, group=group, slot=slot, accumulate=accumulate, windows=windows),
               tuple(claims) + ((G_WINDOWS,) if windows else (G_PLAIN,)))


def _conv(name, h, w, cop, cip, k, dil, claims):
    return Row(name, 'conv', dict(h=h, w=w, cop=cop, cip=cip, OC=cop - 1, IC=cip - 1, k=k, dil=dil), tuple(claims) + (C_TRANSPOSED, G_WINDOWS))


OP_ROWS = [
    # reductions (train_stats_partial_body, train_bn_bwd_reduce_kernel, ojf_train_channel_sums) and the streaming loops
    _bn('bn_1x1', 1, 1, [R_ONE, R_EMPTY, R_IDLE, S_PARTIAL_BLOCK], modes=('eval',)),
    # two pixels under batch statistics: x-hat is +-1 / sqrt(1 + eps / var), so dy = gamma invstd dz (1 - x-hat^2) is eps / (var + eps) of its
    # terms.  With values of unit size that is 1e-5: the result is the rounding of the fp32 mean / invstd (torch's fp32 BatchNorm on the CPU is
    # 109 bars from float64 there, the kernel 118).  The row's y is scaled to var ~ eps, where the float64 comparison says something.
    _bn('bn_1x2', 1, 2, [R_EMPTY, R_IDLE], y_scale=2.0 ** -9),
    _bn('bn_7x9', 7, 9, [R_EMPTY, R_IDLE, S_PARTIAL_BLOCK]),
    _bn('bn_8x8_plain', 8, 8, [R_ONE_EACH], windows=False),
    _bn('bn_5x13', 5, 13, [R_EMPTY, R_RAGGED]),
    _bn('bn_128x128', 128, 128, [R_FULL_BLOCK]),
    _bn('bn_127x129', 127, 129, [R_FULL_BLOCK, R_RAGGED]),
    _bn('bn_257x64', 257, 64, [R_TAIL2]),
    _bn('bn_128x256', 128, 256, [S_FULL_GRID]),
    _bn('bn_200x256', 200, 256, [R_UNROLLED, R_MIXED]),
    _bn('bn_256x256', 256, 256, [S_NO_FIRST3_MAX, S_GRID_STRIDE, R_UNROLLED]),
    _bn('bn_256x257', 256, 257, [S_FIRST3_SOME, R_UNROLLED_THEN_TAIL]),
    _bn('bn_1x114700', 1, 114700, [R_UNROLLED2, S_FIRST3_ALL, S_MIDDLE_NONE, S_TAIL_AFTER_FIRST3]),
    _bn('bn_639x256', 639, 256, [S_MIDDLE_NONE, S_FIRST3_ALL, R_UNROLLED2]),
    _bn('bn_641x256', 641, 256, [S_MIDDLE_SOME, R_UNROLLED2]),
    # weight gradient (train_wgrad_mfma_kernel<false>, train_wgrad_reduce_kernel)
    _wg('wg_1x1_d9', 1, 1, 20, 20, 3, 9, [W_ONE_SLAB, W_CENTRE_ONLY, W_HALF_STEP, W_SHORT_SLAB, W_ROUNDED_PER]),
    _wg('wg_1x1_d27', 1, 1, 20, 20, 3, 27, [W_CENTRE_ONLY]),
    _wg('wg_1x40_d9', 1, 40, 20, 20, 3, 9, [W_TAPS_OUT, W_TAPS_PARTLY, W_SHORT_SLAB]),
    _wg('wg_1x40_d27', 1, 40, 20, 20, 3, 27, [W_TAPS_OUT, W_TAPS_PARTLY]),
    _wg('wg_40x1_d9', 40, 1, 20, 20, 3, 9, [W_TAPS_OUT, W_TAPS_PARTLY]),
    _wg('wg_40x1_d27', 40, 1, 20, 20, 3, 27, [W_TAPS_OUT, W_TAPS_PARTLY]),
    _wg('wg_3x8_d9', 3, 8, 20, 20, 3, 9, [W_CENTRE_ONLY]),
    _wg('wg_3x8_d27', 3, 8, 20, 20, 3, 27, [W_CENTRE_ONLY]),
    _wg('wg_5x13_d27', 5, 13, 20, 20, 3, 27, [W_CENTRE_ONLY, W_HALF_STEP]),
    _wg('wg_5x13_d9', 5, 13, 20, 20, 3, 9, [W_TAPS_OUT, W_TAPS_PARTLY, W_BY_PIXELS]),
    _wg('wg_7x9_d1', 7, 9, 20, 20, 3, 1, [W_PARTIAL_CHUNK, W_HALF_STEP, W_ONE_SLAB]),
    _wg('wg_8x8_plain', 8, 8, 20, 20, 1, 1, [W_ONE_SLAB], windows=False),
    _wg('wg_5x13_1x1', 5, 13, 20, 20, 1, 1, [W_BY_PIXELS, W_SHORT_SLAB, W_HALF_STEP, W_RAGGED_SLAB]),
    _wg('wg_3x43', 3, 43, 20, 20, 1, 1, [W_RAGGED_SLAB, W_HALF_STEP, W_ROUNDED_PER]),
    _wg('wg_10x13', 10, 13, 20, 20, 1, 1, [W_EVEN, W_SHORT_SLAB]),
    # 240 tiles x 9 taps = 2160 waves: one slab, so that 129 / 130 pixels put one / two pixels into a third chunk
    _wg('wg_3x43_one_slab', 3, 43, 512, 480, 3, 1, [W_ONE_SLAB, W_BY_WAVES, W_LAST_CHUNK_1, W_HALF_STEP, W_ROUNDED_PER]),
    _wg('wg_10x13_one_slab', 10, 13, 512, 480, 3, 1, [W_ONE_SLAB, W_BY_WAVES, W_LAST_CHUNK_2, W_EVEN]),
    _wg('wg_128x129_256_slabs', 128, 129, 32, 32, 1, 1, [W_MAX_SLABS, W_EMPTY, W_CHUNKS, W_PARTIAL_CHUNK, W_ROUNDED_PER]),
    _wg('wg_128x129_d9_waves', 128, 129, 20, 20, 3, 9, [W_BY_WAVES, W_CHUNKS, W_PARTIAL_CHUNK, W_TAPS_PARTLY]),
    _wg('wg_oc4_ic4', 9, 15, 4, 4, 3, 1, [W_OG_SHORT, W_IG_SHORT]),
    _wg('wg_oc36_ic36', 9, 15, 36, 36, 3, 1, [W_OG_SHORT, W_IG_SHORT, W_OC_TILES, W_IC_TILES]),
    _wg('wg_oc116_ic20', 9, 15, 116, 20, 1, 1, [W_OC_TILES, W_OG_SHORT]),
    _wg('wg_oc20_ic116_slotted', 9, 15, 20, 116, 1, 1, [W_IC_TILES, W_IG_SHORT, W_SLOTTED], group=19, slot=20, IC=110),
    _wg('wg_oc20_ic232_slotted', 9, 15, 20, 232, 1, 1, [W_SLOTTED, W_IC_TILES], group=114, slot=116, IC=228),
    _wg('wg_oc116_ic572', 5, 13, 116, 572, 1, 1, [W_IC_TILES, W_IG_SHORT, W_OC_TILES]),
    _wg('wg_accumulate', 9, 15, 20, 20, 3, 9, [W_ACCUMULATE, W_TAPS_PARTLY], accumulate=1),
    # ojf_train_pack + ojf_train_conv, forward and transposed
    _conv('conv_1x1', 1, 1, 20, 20, 3, 9, [C_ONE_PIXEL]),
    _conv('conv_1x40', 1, 40, 20, 20, 3, 27, [C_ONE_ROW]),
    _conv('conv_40x1', 40, 1, 20, 20, 3, 9, [C_ONE_COLUMN]),
    _conv('conv_3x8', 3, 8, 20, 20, 3, 9, [C_TINY]),
    _conv('conv_oc132', 7, 9, 132, 8, 1, 1, [C_SECOND_LAUNCH]),
    _conv('conv_oc132_3x3', 7, 9, 132, 8, 3, 1, [C_SECOND_LAUNCH]),
    # ojf_train_avgpool3
    Row('pool_1x1', 'pool', dict(h=1, w=1, c=4), (P_ONE_PIXEL, P_NO_INTERIOR)),
    Row('pool_1x5', 'pool', dict(h=1, w=5, c=4), (P_ONE_ROW,)),
    Row('pool_5x1', 'pool', dict(h=5, w=1, c=20), (P_ONE_COLUMN,)),
    Row('pool_2x2', 'pool', dict(h=2, w=2, c=20), (P_NO_INTERIOR,)),
    Row('pool_7x9', 'pool', dict(h=7, w=9, c=4), ()),
    Row('pool_257x256', 'pool', dict(h=257, w=256, c=4), (P_GRID_STRIDE,)),
    # ojf_train_fuse_output(_bwd), ojf_train_fusion_loss(_bwd)
    Row('loss_1', 'loss', dict(nv=1), (L_ONE_ROW,)),
    Row('loss_255', 'loss', dict(nv=255), (L_PARTIAL,)),
    Row('loss_256', 'loss', dict(nv=256), (L_FULL,)),
    Row('loss_257', 'loss', dict(nv=257), (L_ONE_OVER,)),
    Row('loss_16385', 'loss', dict(nv=64 * 256 + 1), (L_FINISH2,)),
]

# LayerUnit in both `training` settings: (IC, OC, k, dil, group, slot, act, bn) x frames
UNIT_SHAPES = [(19, 19, 3, 27, 19, 20, 'relu', True), (114, 19, 1, 1, 19, 20, 'relu', True), (19, 9, 1, 1, 19, 20, 'tanh', False)]
UNIT_FRAMES = [(1, 40), (40, 1), (3, 8), (200, 256), (256, 257)]
UNIT_FRAME_CLAIMS = {(1, 40): (R_EMPTY, S_PARTIAL_BLOCK, W_SHORT_SLAB), (40, 1): (R_EMPTY, S_PARTIAL_BLOCK, W_SHORT_SLAB), (3, 8): (R_EMPTY, R_IDLE, W_ONE_SLAB),
                     (200, 256): (R_UNROLLED, R_MIXED, W_CHUNKS), (256, 257): (S_FIRST3_SOME, R_UNROLLED_THEN_TAIL, W_CHUNKS)}
UNIT_DILATED_CLAIMS = {(1, 40): (W_TAPS_OUT, W_TAPS_PARTLY), (40, 1): (W_TAPS_OUT, W_TAPS_PARTLY), (3, 8): (W_CENTRE_ONLY,), (200, 256): (W_TAPS_PARTLY,),
                       (256, 257): (W_TAPS_PARTLY,)}
UNIT_ROWS = [Row('unit_%d_%d_k%d_d%d_%s_%dx%d_%s' % (s[0], s[1], s[2], s[3], s[6], h, w, 'train' if training else 'eval'), 'unit',
                 dict(shape=s, h=h, w=w, training=training), UNIT_FRAME_CLAIMS[(h, w)] + (UNIT_DILATED_CLAIMS[(h, w)] if s[2] == 3 else ()))
             for s in UNIT_SHAPES for h, w in UNIT_FRAMES for training in (True, False)]

EXECUTOR_FRAMES = collections.OrderedDict([
    ((1, 1), (X_BELOW_TILE, X_HALO1, X_HALO3, X_PX_PARTIAL, X_WG_SHORT, X_WG_HALF, X_WG_CENTRE, X_R_EMPTY)),
    ((1, 40), (X_HALO1, X_HALO3, X_WG_SHORT, X_R_EMPTY)),
    ((40, 1), (X_HALO1, X_HALO3, X_R_EMPTY)),
    ((3, 8), (X_BELOW_TILE, X_HALO3, X_WG_CENTRE, X_PX_PARTIAL)),
    ((8, 32), (X_ONE_TILE, X_PX_ONE)),
    ((9, 33), (X_ONE_OVER, X_PX_MANY, X_WG_HALF)),
    ((17, 65), (X_MANY_RAGGED, X_PX_MANY, X_WG_HALF)),
])
EXECUTOR_NETS = [('v3', True), ('v2', True)]
# The whole-net gradient is discontinuous where a ReLU's pre-activation or an L1 residual crosses zero.  An input at which the float64
# reference sits within one fp32 ulp of such a point, and where the other side moves a gradient by more than half a bar, compares which
# side an fp32 evaluation happens to take, not the kernels.  With _whole_net_gradient_case's input seed 11 that holds for three rows,
# measured on the float64 net alone: v3 17 x 65 11.5 bars; v2 17 x 65 2.4 bars and, at seed 12, 3.2 bars; v2 9 x 33 127 bars (one
# pre-activation of 3.5e-8 beside values of 0.53; its other side moves block.0.block.0.weight by 1.081e-6, 1.07e-4 of its scale - the
# split-fp16 forward pass took it and sat 1.0806e-6 from the reference).  Those rows use the first seed 12, 13, ... at which the
# reference is stable; tests/test_train_edges_host.py evaluates the rule (executor_reference_instability there) for every row: seed 11
# wherever it is stable, and every skipped seed unstable.
NEAR_ZERO = 2.0 ** -23           # of a tensor's largest magnitude: one fp32 ulp of it - no fp32 evaluation can tell the sides apart
EXECUTOR_INPUT_SEEDS = {('v2', 9, 33): 12, ('v3', 17, 65): 12, ('v2', 17, 65): 13}
EXECUTOR_ROWS = [Row('executor_%s_%dx%d' % (v, h, w), 'executor', dict(version=v, sem=sem, h=h, w=w, input_seed=EXECUTOR_INPUT_SEEDS.get((v, h, w), 11)), claims)
                 for v, sem in EXECUTOR_NETS for (h, w), claims in EXECUTOR_FRAMES.items()]
EDGE_ROWS = OP_ROWS + UNIT_ROWS + EXECUTOR_ROWS

EDGES_ANYWHERE = REDUCE_EDGES + STREAM_EDGES + WGRAD_EDGES + POOL_EDGES + LOSS_EDGES + CONV_EDGES + EXECUTOR_EDGES + [G_WINDOWS, G_PLAIN]


def row_id(row):
    return row.name


def reached(row):
    """the set of edges a row reaches, computed from the restatement"""
    p = row.p
    if row.kind == 'bn':
        return reduce_edges(p['h'] * p['w']) | stream_edges(p['h'] * p['w']) | {G_WINDOWS if p['windows'] else G_PLAIN}
    if row.kind == 'wgrad':
        return wgrad_edges(p['cop'], p['cip'], p['k'], p['dil'], p['h'], p['w'], 1, p['group'], p['slot'], p['IC'], p['accumulate']) | {G_WINDOWS if p['windows'] else G_PLAIN}
    if row.kind == 'conv':
        return conv_edges(p['cop'], p['k'], p['dil'], p['h'], p['w']) | {G_WINDOWS}
    if row.kind == 'pool':
        return pool_edges(p['h'], p['w'])
    if row.kind == 'loss':
        return loss_edges(p['nv'])
    if row.kind == 'executor':
        return executor_edges(p['h'], p['w'])
    if row.kind == 'unit':
        c_in = round_up(cdiv(p['shape'][0], p['shape'][4]) * p['shape'][5], 4)
        return reduce_edges(p['h'] * p['w']) | stream_edges(p['h'] * p['w']) | wgrad_edges(round_up(p['shape'][1], 4), c_in, p['shape'][2], p['shape'][3], p['h'], p['w'])
    raise KeyError(row.kind)


# ---- what the frames of tests/test_train_gpu.py reach -------------------------------------------------------------------------------
OLD_FRAMES = [(37, 45), (40, 56), (13, 15), (23, 37), (24, 40), (240, 320)]
# (c_out_phys, c_in_phys, ksize, dil, units) of test_layer_unit_against_torch's list ("every layer geometry of the net"); the executor
# groups the four branches of a VortexPooling into one launch (units = 4)
OLD_UNIT_SHAPES = [(20, 20, 3, 1, 1), (20, 60, 3, 1, 1), (20, 100, 3, 1, 1), (20, 20, 3, 27, 1), (20, 20, 3, 9, 1), (20, 120, 1, 1, 1), (20, 116, 1, 1, 1),
                   (116, 20, 1, 1, 1), (116, 580, 1, 1, 1), (96, 116, 1, 1, 1), (20, 20, 1, 1, 1), (12, 20, 1, 1, 1), (20, 232, 1, 1, 1),
                   (20, 20, 3, 27, 4), (20, 20, 3, 9, 4), (20, 20, 3, 3, 4), (20, 20, 3, 1, 4), (20, 116, 1, 1, 4)]


def old_sizes_reach():
    got = set()
    for h, w in OLD_FRAMES:
        got |= reduce_edges(h * w) | stream_edges(h * w) | executor_edges(h, w) | pool_edges(h, w)
        for cop, cip, k, dil, units in OLD_UNIT_SHAPES:
            got |= wgrad_edges(cop, cip, k, dil, h, w, units)
        got |= conv_edges(116, 3, 27, h, w) - {C_TRANSPOSED}
    got |= loss_edges(int(0.8 * 56 * 40))  # test_fuse_output_and_fusion_loss_kernels_match_the_tensor_formulas
    return got | {G_PLAIN, C_TRANSPOSED, W_ACCUMULATE, W_SLOTTED}


# the listed edges that no frame of the older tests reaches at any bar (computed by old_sizes_reach; asserted by the host test)
NOT_REACHED_BY_OLD_SIZES = [
    R_ONE, R_ONE_EACH, R_FULL_BLOCK, R_TAIL2, R_MIXED, R_UNROLLED2,
    S_FULL_GRID, S_NO_FIRST3_MAX, S_FIRST3_ALL, S_MIDDLE_NONE, S_MIDDLE_SOME, S_TAIL_AFTER_FIRST3,
    W_ONE_SLAB, W_EMPTY, W_LAST_CHUNK_1, W_LAST_CHUNK_2,
    P_ONE_PIXEL, P_ONE_ROW, P_ONE_COLUMN, P_NO_INTERIOR,
    L_ONE_ROW, L_PARTIAL, L_FULL, L_ONE_OVER, L_FINISH2,
    C_ONE_PIXEL, C_ONE_ROW, C_ONE_COLUMN, C_SECOND_LAUNCH,
    X_BELOW_TILE, X_ONE_TILE, X_ONE_OVER, X_MANY_RAGGED, X_HALO1, X_HALO3, X_PX_ONE,
    G_WINDOWS,
]
# ... and those they reach only on whole-net frames (240 x 320; 13 x 15 for the partial block and the taps outside), under the whole-net
# bar max(1e-4, 2.5 x torch fp32's error, 2 x the net's noise)
REACHED_ONLY_AT_THE_LOOSE_BAR = [R_UNROLLED, R_UNROLLED_THEN_TAIL, S_PARTIAL_BLOCK, S_FIRST3_SOME, S_GRID_STRIDE, W_MAX_SLABS, W_BY_WAVES, W_CHUNKS, W_ROUNDED_PER,
                                 W_EVEN, W_TAPS_OUT, W_CENTRE_ONLY, W_ACCUMULATE]


def old_tight_sizes_reach():
    """the same for the one frame a per-unit float64 comparison at 1e-4 runs on (37 x 45)"""
    h, w = OLD_FRAMES[0]
    got = reduce_edges(h * w) | stream_edges(h * w)
    for cop, cip, k, dil, units in OLD_UNIT_SHAPES:
        if units == 1:
            got |= wgrad_edges(cop, cip, k, dil, h, w, units)
    return got | {W_SLOTTED}


def loose_only():
    old, tight = old_sizes_reach(), old_tight_sizes_reach()
    return [e for e in REDUCE_EDGES + STREAM_EDGES + WGRAD_EDGES if e in old and e not in tight]


# ---- inputs and float64 references ------------------------------------------------------------------------------------------------
SENTINEL_SCALE = 8.0
EPS, MOMENTUM = 1e-5, 0.1
BN_SCALE, BN_DROP = 0.75, 1.25
DOUT_SCALE = 2.0 ** -17  # loss gradients are tiny


def signed_unit(rng, shape):
    """zero-mean, no small magnitudes: +-U(0.5, 1.5), exactly representable in fp32"""
    import numpy as np
    return (rng.choice([-1.0, 1.0], size=shape) * rng.uniform(0.5, 1.5, size=shape)).astype(np.float32).astype(np.float64)


def _seed(name):
    import zlib
    return zlib.crc32(name.encode())


def bn_inputs(row):
    import numpy as np
    p = row.p
    npix, C = p['h'] * p['w'], p['C']
    rng = np.random.default_rng(_seed(row.name))
    y, dout = signed_unit(rng, (C, npix)) * p['y_scale'], signed_unit(rng, (C, npix)) * DOUT_SCALE
    sent = reduce_sentinels(npix)
    for q in sent:
        y[:, q] *= SENTINEL_SCALE
        dout[:, q] *= SENTINEL_SCALE
    f = lambda a: a.astype(np.float32).astype(np.float64)
    return dict(y=y, dout=dout, gamma=f(rng.uniform(0.5, 1.5, C)), beta=f(rng.normal(0, 0.1, C)), rm=f(rng.normal(0, 0.1, C)),
                rv=f(rng.uniform(0.5, 1.5, C)), sentinels=sent)


def bn_reference(x, training):
    """conv output y -> BatchNorm2d (batch or running statistics) -> * scale * drop, and its backward pass, from the definitions"""
    import numpy as np
    y, dout, gamma, beta = x['y'], x['dout'], x['gamma'][:, None], x['beta'][:, None]
    n = y.shape[1]
    if training:
        mean, var = y.mean(1), y.var(1)
    else:
        mean, var = x['rm'], x['rv']
    invstd = 1.0 / np.sqrt(var + EPS)
    xhat = (y - mean[:, None]) * invstd[:, None]
    out = (xhat * gamma + beta) * BN_SCALE * BN_DROP
    dz = dout * BN_SCALE * BN_DROP
    dbeta, dgamma = dz.sum(1), (dz * xhat).sum(1)
    gi = gamma * invstd[:, None]
    if training:
        dy = gi * (dz - dz.mean(1, keepdims=True) - xhat * (dz * xhat).mean(1, keepdims=True))
        rm = (1 - MOMENTUM) * x['rm'] + MOMENTUM * mean
        rv = (1 - MOMENTUM) * x['rv'] + MOMENTUM * (var * n / (n - 1) if n > 1 else var)
    else:
        dy = gi * dz
        rm, rv = x['rm'], x['rv']
    return dict(out=out, dy=dy, terms=gi * dz, dgamma=dgamma, dbeta=dbeta, dbias=dy.sum(1), mean=mean, invstd=invstd, running_mean=rm, running_var=rv,
                sums=y.sum(1), squares=(y * y).sum(1))


def wgrad_inputs(row):
    import numpy as np
    p = row.p
    npix = p['h'] * p['w']
    rng = np.random.default_rng(_seed(row.name))
    x, dy = signed_unit(rng, (p['IC'], npix)), signed_unit(rng, (p['OC'], npix)) * DOUT_SCALE
    plan = wgrad_plan(p['cop'], p['cip'], p['k'] ** 2, npix)
    sent = wgrad_sentinels(plan, npix)
    for q in sent:
        x[:, q] *= SENTINEL_SCALE
        dy[:, q] *= SENTINEL_SCALE
    dw0 = signed_unit(rng, (p['OC'], p['IC'], p['k'] ** 2)) * DOUT_SCALE if p['accumulate'] else None
    return dict(x=x, dy=dy, dw0=dw0, sentinels=sent, plan=plan)


def wgrad_reference(p, x, dy):
    """dW[oc][ic][tap] = sum_p dy[oc][p] * x[ic][p + offset(tap)], zero outside the image: shifted planes and one matrix product per tap"""
    import numpy as np
    h, w = p['h'], p['w']
    xi = x.reshape(-1, h, w)
    dw = np.zeros((dy.shape[0], x.shape[0], p['k'] ** 2))
    for t, (oy, ox) in enumerate(tap_offsets(p['k'], p['dil'])):
        sh = np.zeros_like(xi)
        ys, xs = slice(max(0, -oy), min(h, h - oy)), slice(max(0, -ox), min(w, w - ox))
        if ys.start < ys.stop and xs.start < xs.stop:
            sh[:, ys, xs] = xi[:, ys.start + oy:ys.stop + oy, xs.start + ox:xs.stop + ox]
        dw[:, :, t] = dy @ sh.reshape(x.shape[0], -1).T
    return dw


def slot_channels(IC, group, slot):
    """physical channel of every logical input channel: `group`-wide tensors in `slot`-wide slots"""
    return [(l // group) * slot + l % group for l in range(IC)]


def to_planes(a, c_phys, channels=None):
    """[C, npix] -> C4 planes [c_phys / 4, npix, 4] with zero padding channels (channels: physical index per row)"""
    import numpy as np
    full = np.zeros((c_phys, a.shape[1]), a.dtype)
    full[list(channels) if channels is not None else slice(0, a.shape[0])] = a
    return np.ascontiguousarray(full.reshape(c_phys // 4, 4, -1).transpose(0, 2, 1))


def from_planes(pl, channels):
    """C4 planes [c4, npix, 4] -> [len(channels), npix]"""
    c4, npix, _ = pl.shape
    return pl.transpose(0, 2, 1).reshape(4 * c4, npix)[list(channels)]
