"""Time of the distance transform (distance.esdf: ojf_volume_surface_mask, ojf_volume_edt pass by pass, ojf_volume_esdf) beside
a byte floor and beside scipy.ndimage.distance_transform_edt on the host of the same node, for DESIGN.md 18.

Cases `room_256` and `room_512`: the surface mask of a volume fused from `--frames` frames (240 x 320) of the synthetic room by
projective.integrate_depth (truncation of three voxels, no carving), transformed without a limit and with a limit of
`--limit` metres (0.24), as Database.esdf does.

Every timed iteration runs surface mask, the z, y and x passes as three calls, and the finishing pass, with device events
between them, after `--warmup` iterations; medians over `--iters` iterations, and the smallest and largest total.  The floor
is a device-to-device copy, timed in the same run, of half the bytes the passes must read and write with V voxels (a copy of
n bytes reads n and writes n): surface 5 V (the two fp16 volumes in, the mask out; what it reads of the neighbours is not
counted), z 9 V (seeds in, d² and index out), y and x 16 V each (d² in and out, the index gathered and written), finish 12 V
(d² and the two fp16 volumes in, fp32 out): 58 V bytes.  scipy's transform gets the same mask on the host (`--scipy-repeats`
runs, the fastest is reported); rint of its squared distances is checked against the device's d².  One JSON line per case;
`--out FILE` writes them as one document (profiles/distance_bench.json).

    python tools/distance_bench.py [--iters 10] [--warmup 2] [--frames 40] [--sizes 256 512] [--limit 0.24] [--out profiles/distance_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from online_joint_depthfusion_and_semantic_amd import _lib, distance, projective, synthetic  # noqa: E402

STEPS = ('surface', 'z', 'y', 'x', 'finish')
BYTES_PER_VOXEL = 58


def room_volumes(grid, frames, dev):
    st = synthetic.SyntheticStream(240, 320, grid, frames)
    origin, res, _ = synthetic.grid_spec(grid)
    trunc = 3.0 * res
    tsdf = torch.full((grid,) * 3, trunc, dtype=torch.float16, device=dev)
    wgt = torch.zeros((grid,) * 3, dtype=torch.float16, device=dev)
    for v0 in range(0, frames, 8):
        fr = [st.frame(i) for i in range(v0, min(frames, v0 + 8))]
        projective.integrate_depth(tsdf, wgt, origin=origin, resolution=res, depth=torch.from_numpy(np.stack([f['tof_depth'] for f in fr])).to(dev),
                                   intrinsics=st.K, extrinsics=np.stack([f['extrinsics'] for f in fr]),
                                   mask=torch.from_numpy(np.stack([f['mask'] for f in fr])).to(dev), truncation=trunc)
    return tsdf, wgt, float(res)


def time_steps(tsdf, wgt, res, max_dist2, far, iters, warmup):
    """({step: median us}, [total us per iteration], mask, dist2) of the five steps."""
    lib = _lib.load()
    dev, (X, Y, Z) = tsdf.device, tsdf.shape
    st = _lib.stream_ptr(dev)
    n = tsdf.numel()
    ws_bytes = lib.ojf_volume_edt_workspace_bytes(X, Y, Z)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    mask = torch.empty((X, Y, Z), dtype=torch.uint8, device=dev)
    dist2 = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
    nearest = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
    out = torch.empty((X, Y, Z), dtype=torch.float32, device=dev)
    t16, w16 = tsdf.view(torch.int16), wgt.view(torch.int16)

    def edt(bit):
        _lib.check(lib.ojf_volume_edt(mask.data_ptr(), X, Y, Z, max_dist2, bit, ws.data_ptr(), ws_bytes, dist2.data_ptr(), nearest.data_ptr(), st),
                   'ojf_volume_edt')

    calls = (lambda: _lib.check(lib.ojf_volume_surface_mask(t16.data_ptr(), w16.data_ptr(), X, Y, Z, mask.data_ptr(), st), 'ojf_volume_surface_mask'),
             lambda: edt(_lib.EDT_Z), lambda: edt(_lib.EDT_Y), lambda: edt(_lib.EDT_X),
             lambda: _lib.check(lib.ojf_volume_esdf(dist2.data_ptr(), t16.data_ptr(), w16.data_ptr(), n, res, far, out.data_ptr(), st),
                                'ojf_volume_esdf'))
    per = {name: [] for name in STEPS}
    totals = []
    for it in range(warmup + iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STEPS) + 1)]
        torch.cuda.synchronize()
        ev[0].record()
        for i, call in enumerate(calls):
            call()
            ev[i + 1].record()
        ev[-1].synchronize()
        if it >= warmup:
            for i, name in enumerate(STEPS):
                per[name].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)
            totals.append(ev[0].elapsed_time(ev[-1]) * 1e3)
    return {k: statistics.median(v) for k, v in per.items()}, totals, mask, dist2


def time_copy(nbytes, dev, iters, warmup):
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    out = []
    for it in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def scipy_edt(mask_host, repeats):
    from scipy import ndimage
    best, d = None, None
    for _ in range(repeats):
        t0 = time.perf_counter()
        d = ndimage.distance_transform_edt(mask_host == 0)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--sizes', type=int, nargs='*', default=[256, 512])
    ap.add_argument('--limit', type=float, default=0.24)
    ap.add_argument('--scipy-repeats', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('distance_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    rows = []
    for grid in args.sizes:
        tsdf, wgt, res = room_volumes(grid, args.frames, dev)
        V = tsdf.numel()
        copy_us = time_copy(BYTES_PER_VOXEL * V // 2, dev, args.iters, args.warmup)
        scipy_s = None
        for limit in (None, args.limit):
            max_dist2 = -1 if limit is None else distance._radius2('distance_bench', 'limit', limit, res)
            per, totals, mask, dist2 = time_steps(tsdf, wgt, res, max_dist2, float('inf') if limit is None else limit, args.iters, args.warmup)
            d2 = dist2.cpu().numpy()
            if scipy_s is None:  # (once per size: the unlimited transform)
                host = mask.cpu().numpy()
                scipy_s, d = scipy_edt(host, args.scipy_repeats)
                want = np.rint(d * d).astype(np.int64)
                del d
                if not (d2 == want).all():
                    raise SystemExit('distance_bench: {} voxels differ from scipy'.format(int((d2 != want).sum())))
            else:
                if not (d2 == np.where(want > max_dist2, distance.NONE, want)).all():
                    raise SystemExit('distance_bench: the limited transform is not the unlimited one masked')
            total = statistics.median(totals)
            row = {'case': 'room_%d' % grid + ('' if limit is None else '_limit'), 'grid': grid, 'resolution': res, 'limit_m': limit,
                   'max_dist2': max_dist2, 'voxels': V, 'surface_voxels': int((host != 0).sum()),
                   'largest_distance_voxels': round(math.sqrt(float(want.max())), 2), 'iters': args.iters,
                   'pass_us': {k: round(v, 1) for k, v in per.items()}, 'total_us': round(total, 1),
                   'total_us_min_max': [round(min(totals), 1), round(max(totals), 1)],
                   'bytes_touched': BYTES_PER_VOXEL * V, 'copy_floor_us': round(copy_us, 1), 'total_over_floor': round(total / copy_us, 2),
                   'scipy_edt_ms': round(scipy_s * 1e3, 1), 'scipy_over_device_edt': round(scipy_s * 1e6 / (per['z'] + per['y'] + per['x']), 1),
                   'scipy_dist2_equal': True}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del mask, dist2, d2
        del tsdf, wgt, want, host
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/distance_bench.py', 'device': torch.cuda.get_device_name(0), 'frames': args.frames, 'cases': rows}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
