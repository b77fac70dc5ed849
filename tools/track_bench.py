"""Time of a tracked frame (tracking.track_frame: three ray casts of the model + one ojf_track call of 1 + 2·19 launches)
for DESIGN.md §9, at 320x240 against the 256^3 ground-truth room, tracking frame i+1 from the pose of frame i.

Host time: wall clock of each track_frame call after a synchronise (the call ends with its one copy back), after
`--warmup` calls; "raw" is the bare ojf_track call with its inputs prepared once (model images, buffers), timed the same
way.  One JSON line.  The kernel times come from a separate run under the profiler, summarised by --summarize:

    python tools/track_bench.py [--iters 50] [--warmup 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/track_bench.py --iters 20
    python tools/track_bench.py --summarize OUT/.../kt_kernel_trace.csv
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


def summarize(path):
    """Per-kernel dispatch times of a kernel trace, and per tracked frame the span from its first ray cast to its last
    solve (a frame = the render_kernel launches in front of a track_pyramid_kernel and what follows up to the next)."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    rows = [r for r in rows if any(k in r['Kernel_Name'] for k in ('render_kernel', 'track_'))]
    acc = defaultdict(list)
    for r in rows:
        name = r['Kernel_Name'].split('(')[0].replace('void ', '').replace('ojf::', '')
        acc[(name, r.get('Grid_Size_X', ''))].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    frames, pending = [], []  # a frame: the ray casts in front of a pyramid launch, the pyramid and its steps
    for r in rows:
        if 'render_kernel' in r['Kernel_Name']:
            pending.append(r)
        elif 'track_pyramid' in r['Kernel_Name']:
            frames.append(pending + [r])
            pending = []
        elif frames:
            frames[-1].append(r)
    out = ['kernel                          grid threads   calls   median us   min us   max us']
    for (name, grid), v in sorted(acc.items(), key=lambda kv: -sum(kv[1])):
        out.append('%-30s %12s %7d %11.2f %8.2f %8.2f' % (name[:30], grid, len(v), statistics.median(v), min(v), max(v)))
    for what, sel in (('track_frame (3 ray casts + ojf_track)', [f for f in frames if 'render' in f[0]['Kernel_Name']]),
                      ('bare ojf_track', [f for f in frames if 'render' not in f[0]['Kernel_Name']])):
        if not sel:
            continue
        span = [(int(f[-1]['End_Timestamp']) - int(f[0]['Start_Timestamp'])) / 1e3 for f in sel]
        busy = [sum(int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in f) / 1e3 for f in sel]
        out.append('%s: %d calls, %s launches each; first start -> last end median %.1f us (min %.1f); sum of kernel '
                   'times median %.1f us' % (what, len(sel), sorted(set(len(f) for f in sel)), statistics.median(span),
                                             min(span), statistics.median(busy)))
    print('\n'.join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--summarize', metavar='KERNEL_TRACE_CSV')
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import numpy as np
    import torch
    from online_joint_depthfusion_and_semantic_amd import _lib, synthetic
    from online_joint_depthfusion_and_semantic_amd.ops import camera_arrays
    from online_joint_depthfusion_and_semantic_amd.render import render_views
    from online_joint_depthfusion_and_semantic_amd.tracking import level_intrinsics, pose12, track_frame
    if not torch.cuda.is_available():
        raise SystemExit('track_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    h, w, grid = 240, 320, 256
    origin, res, _ = synthetic.grid_spec(grid)
    tsdf = torch.from_numpy(synthetic.gt_volumes(grid)[0]).to(dev)
    st = synthetic.SyntheticStream(h, w, grid, 400)
    f0, f1 = st.frame(150), st.frame(151)
    kw = dict(origin=origin, resolution=res, depth=torch.from_numpy(f1['tof_depth']).to(dev),
              mask=torch.from_numpy(f1['mask']).to(dev), intrinsics=st.K, extrinsics=f0['extrinsics'])

    def wall(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    last = {}

    def full():
        last['out'] = track_frame(tsdf, None, **kw)
    t_full = wall(full)

    # the bare ojf_track call: model images, buffers and host arrays prepared once
    lib = _lib.load()
    E = pose12(f0['extrinsics'])
    K0 = np.ascontiguousarray(st.K.reshape(9))
    Kinv = np.stack([camera_arrays(level_intrinsics(st.K, l), E.reshape(3, 4))[0] for l in range(3)])
    model = [render_views(tsdf, None, origin=origin, resolution=res, intrinsics=level_intrinsics(st.K, l),
                          extrinsics=E.reshape(3, 4), shape=(h >> l, w >> l)) for l in range(3)]
    md = np.array([_lib.ptr(m['depth']) for m in model], dtype=np.uint64)
    mn = np.array([_lib.ptr(m['normals']) for m in model], dtype=np.uint64)
    its = np.array([10, 5, 4], np.int32)
    ws = torch.empty(lib.ojf_track_workspace_bytes(h, w, 3), dtype=torch.uint8, device=dev)
    out = torch.empty(12 + 4 * 19 + 1, dtype=torch.float64, device=dev)
    m8 = kw['mask'].to(torch.uint8)

    def raw():
        _lib.check(lib.ojf_track(_lib.ptr(kw['depth']), _lib.ptr(m8), h, w, 3, K0.ctypes.data, Kinv.ctypes.data,
                                 md.ctypes.data, mn.ctypes.data, E.ctypes.data, E.ctypes.data, its.ctypes.data, 0.1, 20.0,
                                 0.03, 0.05, _lib.ptr(ws), ws.numel(), out.data_ptr(), out.data_ptr() + 96,
                                 out.data_ptr() + 8 * (12 + 76), _lib.stream_ptr(dev)), 'ojf_track')
        torch.cuda.synchronize()
    t_raw = wall(raw)
    r = last['out']
    dt = float(np.linalg.norm(r['extrinsics'][:3, 3] - f1['extrinsics'][:, 3]))
    print(json.dumps({'case': 'track_frame', 'h': h, 'w': w, 'grid': grid, 'levels': 3, 'iterations': [10, 5, 4],
                      'launches': 3 + 1 + 2 * 19, 'iters': args.iters, 'warmup': args.warmup,
                      'host_ms_median': round(statistics.median(t_full), 4), 'host_ms_min': round(min(t_full), 4),
                      'raw_ms_median': round(statistics.median(t_raw), 4), 'raw_ms_min': round(min(t_raw), 4),
                      'ok': bool(r['ok']), 'inliers_last': int(r['stats'][-1, 0]), 'translation_error_mm': round(1e3 * dt, 3)}),
          flush=True)


if __name__ == '__main__':
    main()
