"""Profiling helper (not a test): the life of the stand-alone entry GEMM's blocks (entry1x1_kernel, both forms), from a libojf.so built
with -DOJF_ENTRY_STAMPS (OJF_LIB_PATH=.../libojf_stamps.so python tools/entry_stamps.py [h w]): thread 0 of every block stamps clock64 at
the phases of each strip of its walk (the first four strips) and the 100-MHz wall clock at the strip's start and end; the stamps of the
LAST stamped launch of a forward pass remain.  Prints, per position in the walk, when each phase was reached after the strip's start
(medians over the blocks, microseconds), the blocks' lives and the launch's span."""
import ctypes, os, sys, types
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_joint_depthfusion_and_semantic_amd import _lib, model
from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine

BLOCKS, STRIPS, SLOTS = 8192, 4, 10
PHASES = ['inputs landed', 'channel sums done', 'weight part 0 landed', 'weight part 1 landed', 'MFMAs issued', 'stores issued']


def report(s):
    """s: int64 [BLOCKS][STRIPS][SLOTS] of one launch"""
    used = s[:, 0, 9] != 0
    first, last_end = s[used, 0, 7].min(), s[used][:, :, 8].max()
    life = (s[used][:, :, 8].max(axis=1) - s[used, 0, 7]) / 100.0
    walked = (s[used][:, :, 9] != 0).sum(axis=1)
    d = s[used, 0, :]
    ok = (d[:, 8] - d[:, 7]) > 50
    rate = float(np.median((d[ok, 6] - d[ok, 0]) / ((d[ok, 8] - d[ok, 7]) / 100.0))) if ok.any() else 2400.0  # clock64 per us
    print('   %d blocks stamped, strips per block %s; launch span %.2f us (first start to last end); block life median %.2f, max %.2f; '
          'starts median %.2f, max %.2f after the first; clock64 %.0f per us' % (
              int(used.sum()), dict(zip(*[a.tolist() for a in np.unique(walked, return_counts=True)])), (last_end - first) / 100.0,
              np.median(life), life.max(), np.median((s[used, 0, 7] - first) / 100.0), ((s[used, 0, 7] - first) / 100.0).max(), rate))
    for k in range(STRIPS):
        on = used & (s[:, k, 9] != 0)
        if not on.any():
            continue
        r = s[on, k, :]
        line = '   strip %d of the walk (%4d blocks): wall %5.2f us |' % (k, int(on.sum()), np.median((r[:, 8] - r[:, 7]) / 100.0))
        for i, nm in enumerate(PHASES):
            have = r[:, i + 1] != 0
            if have.any():
                line += ' %s %.2f |' % (nm, np.median((r[have, i + 1] - r[have, 0]) / rate))
        print(line)


def main():
    h, w = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (240, 320)
    dev = torch.device('cuda:0')
    raw = ctypes.CDLL(_lib.LIB_PATH)
    if not hasattr(raw, 'ojf_debug_entry_stamps'):
        sys.exit('this libojf.so was not built with -DOJF_ENTRY_STAMPS')
    for name in list(_lib.SIGNATURES):  # (an older library patched with the stamps lacks newer entry points)
        if not hasattr(raw, name):
            del _lib.SIGNATURES[name]
    raw.ojf_debug_entry_stamps.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    cfg = types.SimpleNamespace(n_points=9, growth_factor=6, use_semantics=False, output_scale=1.0, resx=w, resy=h)
    torch.manual_seed(0)
    eng = FusionNetEngine(model.FusionNet_v3(cfg).eval(), h, w, dev, arithmetic='f16x3')
    g = torch.Generator(device=dev); g.manual_seed(1)
    fv = (torch.rand(9, h * w, device=dev, generator=g) * 0.2 - 0.1).contiguous()
    fw = torch.rand(9, h * w, device=dev, generator=g).contiguous()
    d = (torch.rand(h, w, device=dev, generator=g) * 3).contiguous()
    est = torch.empty(h * w, 9, device=dev)
    eng.prepare_input(fv, fw, d, None, 0, planes=True)
    stamps = np.zeros((BLOCKS, STRIPS, SLOTS), np.uint64)
    print('%dx%d, geometry-only split-fp16 net, warm forwards 10 and 11 (times after each strip\'s start, medians over the blocks):' % (w, h))
    for rep in range(12):
        eng.forward(est)
        torch.cuda.synchronize()
        if rep >= 10:
            assert raw.ojf_debug_entry_stamps(stamps.ctypes.data, stamps.nbytes) == 0
            report(stamps.astype(np.int64))
    eng.close()


if __name__ == '__main__':
    main()
