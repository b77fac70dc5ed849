"""Time of a frame tracked with colour (tracking.track_frame_rgbd: three ray casts, three colour renders and one
ojf_track_rgbd call of 1 + 2·19 launches) against the depth-only tracker (tracking.track_frame) for DESIGN.md §25, both at
320x240 against the 256^3 ground-truth room with a colour volume fused from twelve frames of the stream, tracking frame
i+1 from the pose of frame i, both from this tree's library.

Host time: wall clock of each call after a synchronise (the call ends with its one copy back), after `--warmup` calls, the
two trackers alternating.  The per-launch kernel times come from a separate run under the profiler, summarised by
--summarize, which adds them (and the ratio of the two associate launches) to the same JSON file:

    python tools/track_rgbd_bench.py [--iters 50] [--warmup 10] --out profiles/track_rgbd_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/track_rgbd_bench.py --iters 20 --out ''
    python tools/track_rgbd_bench.py --summarize OUT/.../kt_kernel_trace.csv --out profiles/track_rgbd_bench.json
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time
from collections import defaultdict

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

KERNELS = ('track_rgbd_prepare_kernel', 'track_rgbd_associate_kernel', 'track_pyramid_kernel', 'track_associate_kernel',
           'track_solve_kernel', 'color_render', 'render_kernel')


def summarize(path, out_path):
    """Median / min / max dispatch time per kernel and grid size, and the rgbd associate over the depth-only associate at
    the level-0 grid (75 blocks at 320x240)."""
    acc = defaultdict(list)
    for r in csv.DictReader(open(path)):
        name = r['Kernel_Name'].split('(')[0].replace('void ', '').replace('ojf::', '').replace('rgbd::', '')
        if any(k in name for k in KERNELS):
            acc[(name, int(r.get('Grid_Size_X') or r.get('Grid_Size') or 0))].append(
                (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    kernels = [{'kernel': n, 'grid_threads': g, 'calls': len(v), 'median_us': round(statistics.median(v), 2),
                'min_us': round(min(v), 2), 'max_us': round(max(v), 2)}
               for (n, g), v in sorted(acc.items(), key=lambda kv: (kv[0][0], -kv[0][1]))]

    def level0(name):
        rows = [k for k in kernels if k['kernel'] == name]
        return max(rows, key=lambda k: k['grid_threads']) if rows else None
    a, b = level0('track_rgbd_associate_kernel'), level0('track_associate_kernel')
    result = {'kernels': kernels}
    if a and b:
        result['associate_level0_us'] = {'rgbd': a['median_us'], 'depth_only': b['median_us'],
                                         'ratio': round(a['median_us'] / b['median_us'], 3)}
    print(json.dumps(result))
    if out_path:
        merged = json.load(open(out_path)) if os.path.exists(out_path) else {}
        merged.update(result)
        with open(out_path, 'w') as f:
            json.dump(merged, f, indent=1)
            f.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_rgbd_bench.json'))
    ap.add_argument('--summarize', metavar='KERNEL_TRACE_CSV')
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.out)
    import numpy as np
    import torch
    from online_joint_depthfusion_and_semantic_amd import color, synthetic
    from online_joint_depthfusion_and_semantic_amd.tracking import track_frame, track_frame_rgbd
    if not torch.cuda.is_available():
        raise SystemExit('track_rgbd_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    h, w, grid = 240, 320, 256
    origin, res, _ = synthetic.grid_spec(grid)
    tsdf = torch.from_numpy(synthetic.gt_volumes(grid)[0]).to(dev)
    st = synthetic.SyntheticStream(h, w, grid, 400)
    colors = color.new_volume(tsdf.shape, dev)

    def image_of(f):  # the stream's float [3,h,w] image on the 0..255 scale
        im = np.asarray(f['image'], np.float32)
        return torch.from_numpy(im * (255.0 if im.max() <= 1.0 else 1.0)).to(dev)
    for i in range(140, 152):
        f = st.frame(i)
        color.integrate_color(colors, origin=origin, resolution=res, image=image_of(f),
                              depth=torch.from_numpy(f['depth_gt']).to(dev), intrinsics=st.K, extrinsics=f['extrinsics'],
                              band=3 * res)
    f0, f1 = st.frame(150), st.frame(151)
    kw = dict(origin=origin, resolution=res, depth=torch.from_numpy(f1['tof_depth']).to(dev),
              mask=torch.from_numpy(f1['mask']).to(dev), intrinsics=st.K, extrinsics=f0['extrinsics'])
    image = color.pack_image(image_of(f1), 1, h, w, dev)[0]
    last = {}

    def depth_only():
        last['depth'] = track_frame(tsdf, None, **kw)

    def rgbd():
        last['rgbd'] = track_frame_rgbd(tsdf, None, colors, image=image, **kw)
    for _ in range(args.warmup):
        depth_only()
        rgbd()
    ts = {'depth': [], 'rgbd': []}
    for _ in range(args.iters):  # alternating: both see the same neighbours on the machine
        for name, fn in (('depth', depth_only), ('rgbd', rgbd)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t0) * 1e3)

    def err(r):
        return round(1e3 * float(np.linalg.norm(r['extrinsics'][:3, 3] - f1['extrinsics'][:, 3])), 3)
    result = {'case': 'track_frame_rgbd vs track_frame', 'h': h, 'w': w, 'grid': grid, 'levels': 3, 'iterations': [10, 5, 4],
              'iters': args.iters, 'warmup': args.warmup,
              'launches': {'track_frame': 3 + 1 + 2 * 19, 'track_frame_rgbd': 3 + 3 + 1 + 2 * 19},
              'track_frame_ms': {'median': round(statistics.median(ts['depth']), 4), 'min': round(min(ts['depth']), 4)},
              'track_frame_rgbd_ms': {'median': round(statistics.median(ts['rgbd']), 4), 'min': round(min(ts['rgbd']), 4)},
              'host_ratio': round(statistics.median(ts['rgbd']) / statistics.median(ts['depth']), 3),
              'ok': [bool(last['depth']['ok']), bool(last['rgbd']['ok'])],
              'translation_error_mm': {'track_frame': err(last['depth']), 'track_frame_rgbd': err(last['rgbd'])},
              'rows_last_step': {'track_frame': int(last['depth']['stats'][-1, 0]),
                                 'track_frame_rgbd': int(last['rgbd']['stats'][-1, 0])}}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
