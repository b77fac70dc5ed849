"""Profiling helper (not a test): the life of the pool pyramid launch's blocks, from a libojf.so built with -DOJF_POOL_STAMPS
(OJF_LIB_PATH=.../libojf_stamps.so python tools/pool_stamps.py [h w [sem]]): every block's thread 0 stamps the 100-MHz wall clock at its
start and end; the stamps of the LAST pyramid launch of a forward pass remain.  Prints, per repeat, the launch's span (first start to
last end), when the block that folds the global-average branch started and ended, and when the last pooling block ended."""
import ctypes, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_joint_depthfusion_and_semantic_amd import _lib, model
from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine
import types

SLOTS, TW, TH = 8192, 32, 8


def main():
    h, w = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (240, 320)
    sem = len(sys.argv) > 3 and sys.argv[3] == 'sem'
    dev = torch.device('cuda:0')
    raw = ctypes.CDLL(_lib.LIB_PATH)
    if not hasattr(raw, 'ojf_debug_pool_stamps'):
        sys.exit('this libojf.so was not built with -DOJF_POOL_STAMPS')
    for name in list(_lib.SIGNATURES):  # (an older library patched with the stamps lacks newer entry points)
        if not hasattr(raw, name):
            del _lib.SIGNATURES[name]
    raw.ojf_debug_pool_stamps.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    cfg = types.SimpleNamespace(n_points=9, growth_factor=6, use_semantics=sem, output_scale=1.0, resx=w, resy=h)
    torch.manual_seed(0)
    net = model.FusionNet_v3(cfg)
    eng = FusionNetEngine(net.eval(), h, w, dev, arithmetic='f16x3')
    g = torch.Generator(device=dev); g.manual_seed(1)
    fv = (torch.rand(9, h * w, device=dev, generator=g) * 0.2 - 0.1).contiguous()
    fw = torch.rand(9, h * w, device=dev, generator=g).contiguous()
    d = (torch.rand(h, w, device=dev, generator=g) * 3).contiguous()
    ids = (torch.rand(h * w, device=dev, generator=g) * 30).to(torch.uint8)
    est = torch.empty(h * w, 9, device=dev)
    eng.prepare_input(fv, fw, d, ids if sem else None, 30 if sem else 0, planes=True)
    tiles = ((w + TW - 1) // TW) * ((h + TH - 1) // TH)
    gx = (tiles + 1 + 7) // 8 * 8
    fold = next(b for b in range(gx) if (b & 7) * (gx >> 3) + (b >> 3) == tiles)  # blockIdx.x of the fold block (block row 0)
    stamps = np.zeros((SLOTS, 2), np.uint64)
    rows = []
    for rep in range(12):
        eng.forward(est)
        torch.cuda.synchronize()
        assert raw.ojf_debug_pool_stamps(stamps.ctypes.data, stamps.nbytes) == 0
        s = stamps.astype(np.int64)
        ph = s[SLOTS - 8:SLOTS - 4, 0]  # the fold block's phases (0 start, 1 mean formed, 2 first mat-vec done, 3 end), where the build has them
        used = s[:, 0] != 0
        used[SLOTS - 8:] = False
        t0 = s[used, 0].min()
        pools = used.copy(); pools[fold] = False
        rows.append(((s[used, 1].max() - t0) / 100.0, (s[fold, 0] - t0) / 100.0, (s[fold, 1] - t0) / 100.0,
                     (s[pools, 1].max() - t0) / 100.0, int(used.sum()), [(p - ph[0]) / 100.0 for p in ph] if ph.all() else None))
    eng.close()
    print('%dx%d%s: grid_x %d, fold block %d, %d blocks stamped; microseconds from the first block start (warm repeats 2..)' % (
        h, w, ' sem' if sem else '', gx, fold, rows[-1][4]))
    for span, f0, f1, p1, _, ph in rows[2:]:
        print('   launch span %5.2f | fold block %5.2f -> %5.2f (life %5.2f) | last pool block ends %5.2f%s' % (
            span, f0, f1, f1 - f0, p1, '' if ph is None else ' | fold phases: mean %.2f, first mat-vec %.2f, end %.2f' % tuple(ph[1:])))
    rows_y = (int(used.sum()) + gx - 1) // gx  # block rows of the last repeat; a fifth of the three pooled branches' rows each
    life = (s[:rows_y * gx, 1] - s[:rows_y * gx, 0]).reshape(rows_y, gx) / 100.0
    st, en = (s[:rows_y * gx, 0].reshape(rows_y, gx) - t0) / 100.0, (s[:rows_y * gx, 1].reshape(rows_y, gx) - t0) / 100.0
    for y in range(rows_y):
        print('   block row %2d: life median %5.2f max %5.2f | starts %5.2f .. %5.2f | ends %5.2f .. %5.2f' % (
            y, np.median(life[y]), life[y].max(), st[y].min(), st[y].max(), en[y].min(), en[y].max()))
    med = np.median(np.array([r[:4] for r in rows[2:]]), axis=0)
    print('   median: span %.2f, fold life %.2f, fold end %.2f, pools end %.2f' % (med[0], med[2] - med[1], med[2], med[3]))


if __name__ == '__main__':
    main()
