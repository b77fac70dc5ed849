"""Times of the multi-label TV kernels (csrc/ojf_label_tv.hip) for DESIGN.md 23: the label images of 8 frames of the synthetic
room at 320x240 fused into a 256^3 box of 30 classes (S = 32: 64 B per voxel, 1 GiB) within a band of 0.1 m.  Device events
around `--iters` calls after `--warmup`, `--repeats` batches per case, the cases taking turns; the median is reported with the
smallest and the largest batch.  Reported: a restart with 0 iterations (the set-up pass, the read-back of the brick count - the
call's one synchronisation - and the start values); an iteration (a continued call of 30 over 30: a dual and a primal launch
each); a 30-iteration solve from a restart; the write, without and with the second record volume.  Beside each: the bytes the
pass must touch (counted from the volume: the records and the 5·C state floats of the observed voxels, the flag bytes of the
listed bricks) and the time of a device copy that moves as many bytes (half read, half written) - the yardstick of DESIGN.md
15-19 -, the observed voxels, the listed bricks and the bytes of the state.  One JSON line per case; `--out FILE` also writes
them as one JSON document (profiles/label_tv_bench.json).

    python tools/label_tv_bench.py [--iters 10] [--warmup 2] [--repeats 5] [--out profiles/label_tv_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from online_joint_depthfusion_and_semantic_amd import label_probs, label_tv, synthetic  # noqa: E402
from tvl1_bench import time_calls, copy_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--grid', type=int, default=256)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('label_tv_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    h, w, grid, band, C, views, K_IT = 240, 320, args.grid, 0.1, 30, 8, 30
    S = label_probs.record_size(C)
    shape = (grid,) * 3
    N = grid ** 3
    origin, res, _ = synthetic.grid_spec(grid)
    st = synthetic.SyntheticStream(h, w, grid, 40, n_classes=C)
    fr = [st.frame(i) for i in range(views)]
    depth = torch.from_numpy(np.stack([f['tof_depth'] for f in fr])).to(dev)
    mask = torch.from_numpy(np.stack([f['mask'] for f in fr]).astype(np.uint8)).to(dev)
    labels = torch.from_numpy(np.stack([np.asarray(f['semantic_gt']) for f in fr]).astype(np.uint8)).to(dev)
    E = np.stack([f['extrinsics'] for f in fr])
    vol = label_probs.new_volume(shape, C, dev)
    label_probs.integrate_label_probs(vol, C, origin=origin, resolution=res, depth=depth, intrinsics=st.K, extrinsics=E, mask=mask,
                                      labels=labels, band=band)
    observed = int((vol[..., C] > 0).sum())
    t = dict(iters=args.iters, warmup=args.warmup, repeats=args.repeats)
    cases = []

    def emit(row):
        print(json.dumps(row), flush=True)
        cases.append(row)

    solver = label_tv.Solver(shape, C, dev)
    solver.solve(vol, iterations=0)
    bricks, L = solver.count, solver.layout
    base = {'grid': grid, 'h': h, 'w': w, 'views': views, 'n_classes': C, 'record_bytes': 2 * S, 'observed_voxels': observed,
            'observed_fraction': round(observed / N, 5), 'listed_bricks': bricks, 'bricks_of_the_box': L['n_bricks'],
            'state_bytes': 20 * L['plane'], 'dense_state_bytes': 20 * C * N}
    ids = torch.zeros(shape, dtype=torch.uint8, device=dev)
    scores = torch.zeros(shape, dtype=torch.float16, device=dev)
    out = label_probs.new_volume(shape, C, dev)
    fns = {'restart': lambda: solver.solve(vol, iterations=0),
           'solve30': lambda: solver.solve(vol, iterations=K_IT),
           'iterate30': lambda: solver.solve(vol, iterations=K_IT, restart=False),
           'write': lambda: solver.write(ids, scores),
           'write_probs': lambda: solver.write(ids, scores, out)}
    times = time_calls(fns, **t)
    flags = bricks * label_tv.BRICK_VOXELS

    def row(case, key, nbytes, per=1, unit='us_per_call'):
        med, lo, hi = times[key]
        emit(dict(base, case=case, bytes_touched=nbytes, **{unit: round(med / per, 2), unit + '_min_max': [round(lo / per, 2), round(hi / per, 2)]},
                  copy_of_those_bytes_us=round(copy_us(nbytes, dev, **t), 2)))
    # set-up: W of every voxel (and of its six neighbours, from the cache), a flag byte per voxel of the padded box; the start
    # values: the record of every observed voxel, the five state arrays of the listed bricks
    row('label_tv_restart', 'restart', N * 2 + L['n_bricks'] * label_tv.BRICK_VOXELS + observed * 2 * S + flags * (1 + 20 * C))
    # dual: flags, ub read, p read + written;  primal: flags, the record, p read, u read + written, ub written
    row('label_tv_iteration', 'iterate30', 2 * flags + observed * (4 * C * (1 + 3 + 3) + 2 * S + 4 * C * (3 + 1 + 1 + 1)), per=K_IT,
        unit='us_per_iteration')
    med, lo, hi = times['solve30']
    emit(dict(base, case='label_tv_solve_30_from_restart', us_per_call=round(med, 2), us_per_call_min_max=[round(lo, 2), round(hi, 2)]))
    row('label_tv_write', 'write', flags + observed * (4 * C + 3))
    row('label_tv_write_with_distribution', 'write_probs', flags + observed * (4 * C + 3 + 2 + 2 * (C + 1)))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/label_tv_bench.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
