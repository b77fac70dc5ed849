"""Times of the TV-L1 fusion kernels (csrc/ojf_tvl1.hip) for DESIGN.md 22: frames of the synthetic room at 320x240 into a 256^3
box, 9 bins (S = 16: 32 B per voxel, 512 MiB), carve on.  Device events around `--iters` calls after `--warmup`, `--repeats`
batches per case, the cases taking turns; the median is reported with the smallest and the largest batch.  Reported: the
histogram sweep per call and per view at 1 and 8 views per call; the set-up pass (a restart with 0 iterations); an iteration
(a continued call of 25 over 25) on the listed bricks and on every brick of the box; a 25-iteration solve from a restart; the
write.  Beside each: the bytes the pass must touch (counted from the volume: records of voting (voxel, view) pairs, the arrays
of the listed bricks) and the time of a device copy that moves as many bytes (half read, half written) - the yardstick of
DESIGN.md 15-19 -, the observed voxels and the listed bricks.  One JSON line per case; `--out FILE` also writes them as one
JSON document (profiles/tvl1_bench.json).

    python tools/tvl1_bench.py [--iters 20] [--warmup 3] [--repeats 5] [--out profiles/tvl1_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from online_joint_depthfusion_and_semantic_amd import synthetic, tvl1  # noqa: E402

BRICK = 4 * 8 * 32  # voxels of a brick (csrc/ojf_tvl1.hip kTvX·kTvY·kTvZ)


def time_calls(fns, iters, warmup, repeats):
    """{name: (median, min, max)} in us per call over `repeats` batches of `iters` calls per function, the functions taking turns."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / iters)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in out.items()}


def copy_us(nbytes, dev, iters, warmup, repeats):
    """us of a device copy that touches ``nbytes`` (half read, half written)."""
    n = max(int(nbytes) // 2, 256)
    src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    return time_calls({'copy': lambda: dst.copy_(src)}, iters, warmup, repeats)['copy'][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--grid', type=int, default=256)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tvl1_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    h, w, grid, trunc, B, lam, K_IT = 240, 320, args.grid, 0.1, 9, 2.0, 25
    S = tvl1.record_size(B)
    shape = (grid,) * 3
    N = grid ** 3
    origin, res, _ = synthetic.grid_spec(grid)
    st = synthetic.SyntheticStream(h, w, grid, 40)
    fr = [st.frame(i) for i in range(8)]
    depth = torch.from_numpy(np.stack([f['tof_depth'] for f in fr])).to(dev)
    mask = torch.from_numpy(np.stack([f['mask'] for f in fr]).astype(np.uint8)).to(dev)
    E = np.stack([f['extrinsics'] for f in fr])
    t = dict(iters=args.iters, warmup=args.warmup, repeats=args.repeats)
    cases = []

    def emit(row):
        print(json.dumps(row), flush=True)
        cases.append(row)

    hist = None
    for n in (1, 8):
        hist = tvl1.new_volume(shape, B, dev)

        def fuse(hist=hist, n=n):
            tvl1.integrate_depth_hist(hist, B, origin=origin, resolution=res, depth=depth[:n], intrinsics=st.K, extrinsics=E[:n],
                                      mask=mask[:n], truncation=trunc, max_weight=2048.0)
        fuse()
        votes = int(hist[..., B].float().sum())  # voting (voxel, view) pairs of one call: one read and one write of a record each
        nbytes = 2 * votes * 2 * S
        med, lo, hi = time_calls({'fuse': fuse}, **t)['fuse']
        emit({'case': 'fuse_depth_hist', 'grid': grid, 'h': h, 'w': w, 'n_bins': B, 'record_bytes': 2 * S, 'n': n, 'carve': True,
              'observed_voxels': int((hist[..., B] > 0).sum()), 'voting_voxel_views': votes, 'bytes_touched': nbytes,
              'us_per_call': round(med, 2), 'us_per_view': round(med / n, 2), 'us_per_call_min_max': [round(lo, 2), round(hi, 2)],
              'copy_of_those_bytes_us': round(copy_us(nbytes, dev, **t), 2)})
        if n == 1:
            del hist
    # the solver, on the histograms of the eight views
    hist.zero_()
    tvl1.integrate_depth_hist(hist, B, origin=origin, resolution=res, depth=depth, intrinsics=st.K, extrinsics=E, mask=mask, truncation=trunc)
    observed = int((hist[..., B] > 0).sum())
    solver = tvl1.Solver(shape, dev)

    def listed():
        torch.cuda.synchronize()
        off = solver._ws_ptr - solver.workspace.data_ptr()
        return int(solver.workspace[off:off + 4].cpu().numpy().view(np.uint32)[0])
    solver.solve(hist, B, lam, 0)
    bricks = listed()
    total_bricks = -(-grid // 4) * -(-grid // 8) * -(-grid // 32)
    per_voxel = 1 + 8 + 24  # flags, ub read + written, p read + written
    per_observed = 2 * S + 8  # the record, u read + written
    base = {'grid': grid, 'n_bins': B, 'record_bytes': 2 * S, 'observed_voxels': observed, 'observed_fraction': round(observed / N, 5),
            'listed_bricks': bricks, 'bricks_of_the_box': total_bricks}
    fns = {'setup': lambda: solver.solve(hist, B, lam, 0),
           'solve25': lambda: solver.solve(hist, B, lam, K_IT),
           'iterate25': lambda: solver.solve(hist, B, lam, K_IT, restart=False)}
    times = time_calls(fns, **t)
    setup_bytes = N * (2 + 1 + 24 + 4) + observed * (2 * S + 4)
    emit(dict(base, case='tvl1_setup', bytes_touched=setup_bytes, us_per_call=round(times['setup'][0], 2),
              us_per_call_min_max=[round(v, 2) for v in times['setup'][1:]], copy_of_those_bytes_us=round(copy_us(setup_bytes, dev, **t), 2)))
    it_bytes = bricks * BRICK * per_voxel + observed * per_observed
    emit(dict(base, case='tvl1_iteration', bytes_touched=it_bytes, us_per_iteration=round(times['iterate25'][0] / K_IT, 2),
              us_per_iteration_min_max=[round(v / K_IT, 2) for v in times['iterate25'][1:]],
              copy_of_those_bytes_us=round(copy_us(it_bytes, dev, **t), 2)))
    emit(dict(base, case='tvl1_solve_25_from_restart', us_per_call=round(times['solve25'][0], 2),
              us_per_call_min_max=[round(v, 2) for v in times['solve25'][1:]]))
    # the same iteration over every brick of the box
    solver.solve(hist, B, lam, 0, all_bricks=True)
    assert listed() == total_bricks
    med, lo, hi = time_calls({'all': lambda: solver.solve(hist, B, lam, K_IT, restart=False)}, **t)['all']
    all_bytes = total_bricks * BRICK * per_voxel + observed * per_observed
    emit(dict(base, case='tvl1_iteration_all_bricks', listed_bricks=total_bricks, bytes_touched=all_bytes, us_per_iteration=round(med / K_IT, 2),
              us_per_iteration_min_max=[round(lo / K_IT, 2), round(hi / K_IT, 2)], copy_of_those_bytes_us=round(copy_us(all_bytes, dev, **t), 2)))
    tsdf = torch.full(shape, trunc, dtype=torch.float16, device=dev)
    wgt = torch.zeros(shape, dtype=torch.float16, device=dev)
    med, lo, hi = time_calls({'write': lambda: solver.write(tsdf, wgt, trunc)}, **t)['write']
    write_bytes = 2 * N + observed * 8
    emit(dict(base, case='tvl1_write', bytes_touched=write_bytes, us_per_call=round(med, 2), us_per_call_min_max=[round(lo, 2), round(hi, 2)],
              copy_of_those_bytes_us=round(copy_us(write_bytes, dev, **t), 2)))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/tvl1_bench.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
