"""Profiling helper (not a test): the life of the fused VortexPooling tails' blocks (vortex_tail_kernel: tail + next entry GEMM, tail +
prediction head), from a libojf.so built with -DOJF_TAIL_STAMPS (OJF_LIB_PATH=.../libojf_stamps.so python tools/tail_stamps.py [h w [form]]):
thread 0 of every block stamps clock64 at the phases of its life and the 100-MHz wall clock at its start and end; the stamps of the last
launch of each kind remain.  form: 1 = the product kernel (branch b + 1's planes requested during branch b), 0 = requested at each
branch's head.  Prints, for two warm forwards and both tails, how long each phase took (medians over the blocks,
microseconds; h0..h10 = the prediction head's layers), the blocks' lives, the launch's span from the first start to the last end, and when the second round of blocks starts.

"inputs landed" is the profiling build's own `s_waitcnt vmcnt(0)` in front of each branch's closing 1x1: it covers the wave's planes and
its chunks of the weight part requested one part earlier - the wait chain_layer would make a few instructions later anyway."""
import ctypes, os, sys, types
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_joint_depthfusion_and_semantic_amd import _lib, model
from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine

KINDS, BLOCKS, SLOTS = 2, 8192, 32
NAMES = ['tail + next entry GEMM', 'tail + prediction head']
SLOTS_PER_CU = 3 * 256  # resident blocks of the launch: three per CU


def phases(kind):
    """(name, slot it ends at, slot it starts at)"""
    out = []
    for b in range(4):
        out.append(('b%d inputs landed' % b, 1 + 3 * b, 3 * b))
        out.append(('b%d closing 1x1' % b, 2 + 3 * b, 1 + 3 * b))
        out.append(('b%d accumulation' % b, 3 + 3 * b, 2 + 3 * b))
    out.append(('final epilogue', 13, 12))
    if kind == 0:
        out.append(('channel sums', 14, 13))
        out.append(('entry layer', 15, 14))
    else:
        out.append(('head', 15, 13))
    return out


def head_layers(r, rate):
    """[blocks, 11] us: the head's 11 pointwise layers, each from the end of the one before (slots 20..30 hold the 100-MHz wall clock;
    the first layer starts at the final epilogue's end, a clock64 stamp: block start + its clock64 distance from there)"""
    wall = (r[:, 20:31] - r[:, 16:17]) / 100.0
    begin = (r[:, 13] - r[:, 0]) / rate
    return np.diff(np.concatenate([begin[:, None], wall], axis=1), axis=1)


def report(s, kind):
    """s: int64 [BLOCKS][SLOTS] of one launch"""
    used = s[:, 18] != 0
    if not used.any():
        print('   %s: no stamps' % NAMES[kind])
        return
    r = s[used]
    first = r[:, 16].min()
    start, life = (r[:, 16] - first) / 100.0, (r[:, 17] - r[:, 16]) / 100.0
    ok = life > 0.5
    rate = float(np.median((r[ok, 15] - r[ok, 0]) / life[ok]))  # clock64 per us
    order = np.sort(start)
    second = order[SLOTS_PER_CU] if len(order) > SLOTS_PER_CU else float('nan')
    print('   %s: %d blocks; launch span %.2f us (first start to last end); block life median %.2f, p10 %.2f, p90 %.2f, max %.2f; '
          'block %d (the second round) starts at %.2f; clock64 %.0f per us' % (
              NAMES[kind], int(used.sum()), (r[:, 17].max() - first) / 100.0, np.median(life), np.percentile(life, 10),
              np.percentile(life, 90), life.max(), SLOTS_PER_CU, second, rate))
    rounds = [('all blocks', np.ones(len(r), bool))]
    if len(order) > SLOTS_PER_CU:
        rounds += [('first round', start < second), ('later rounds', start >= second)]
    for label, sel in rounds:
        line = '      %-12s (%4d) life %5.2f |' % (label, int(sel.sum()), np.median(life[sel]))
        waits = 0.0
        for name, end, begin in phases(kind):
            d = float(np.median((r[sel, end] - r[sel, begin]) / rate))
            line += ' %s %.2f |' % (name, d)
            if name.endswith('inputs landed') and not name.startswith('b0'):
                waits += d
        print(line + ' b1..b3 input waits together %.2f' % waits)
        if kind == 1:
            h = np.median(head_layers(r[sel], rate), axis=0)
            print('      %-12s head layers (8-6-6-5-5-4-4-3-3-2-2-1 tiles):' % '' + ''.join(' h%d %.2f |' % (l, h[l]) for l in range(11)) +
                  ' the six small ones together %.2f' % h[5:].sum())


def main():
    h, w = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (240, 320)
    form = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    dev = torch.device('cuda:0')
    raw = ctypes.CDLL(_lib.LIB_PATH)
    if not hasattr(raw, 'ojf_debug_tail_stamps'):
        sys.exit('this libojf.so was not built with -DOJF_TAIL_STAMPS')
    raw.ojf_debug_tail_stamps.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    assert raw.ojf_debug_tail_form(form) == 0
    cfg = types.SimpleNamespace(n_points=9, growth_factor=6, use_semantics=False, output_scale=1.0, resx=w, resy=h)
    torch.manual_seed(0)
    eng = FusionNetEngine(model.FusionNet_v3(cfg).eval(), h, w, dev, arithmetic='f16x3')
    g = torch.Generator(device=dev); g.manual_seed(1)
    fv = (torch.rand(9, h * w, device=dev, generator=g) * 0.2 - 0.1).contiguous()
    fw = torch.rand(9, h * w, device=dev, generator=g).contiguous()
    d = (torch.rand(h, w, device=dev, generator=g) * 3).contiguous()
    est = torch.empty(h * w, 9, device=dev)
    eng.prepare_input(fv, fw, d, None, 0, planes=True)
    stamps = np.zeros((KINDS, BLOCKS, SLOTS), np.uint64)
    print('%dx%d, geometry-only split-fp16 net, form %d, warm forwards 10 and 11 (phase durations, medians over the blocks, us):' % (w, h, form))
    for rep in range(12):
        eng.forward(est)
        torch.cuda.synchronize()
        if rep >= 10:
            assert raw.ojf_debug_tail_stamps(stamps.ctypes.data, stamps.nbytes) == 0
            for kind in range(KINDS):
                report(stamps[kind].astype(np.int64), kind)
    eng.close()


if __name__ == '__main__':
    main()
