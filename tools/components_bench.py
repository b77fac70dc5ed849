"""Time of ojf_volume_components (components.label_components) pass by pass, beside a byte floor and beside
scipy.ndimage.label on the host of the same node, for DESIGN.md 17.

Case 1, `room_256` and `room_512`: the observed mask of a volume fused from `--frames` frames (240 x 320) of the synthetic
room by projective.integrate_depth (truncation of three voxels, no carving), connectivity 26 - what Database.filter_components
labels.  Case 2, `serpentine_256`: a path one voxel wide through every brick of 256^3 (every even x-layer holds the even
y-rows, bridged at alternating ends; the layers are bridged at alternating ends of the layer path): one component whose unions
form the longest chain the seam pass can be given, connectivity 6.

Every timed iteration runs the five phases (brick, seam, flatten, rank, list) as five calls on the same buffers with device
events between them - a phase on its own would find the work of the earlier iteration done (a seam pass over labels that are
united already hooks nothing) - after `--warmup` iterations; medians over `--iters` iterations, and the smallest and largest
total.  The floor is a device-to-device copy, timed in the same run, of half the bytes the passes must read and write with V
voxels (a copy of n bytes reads n and writes n): brick 9 V (mask in, labels and brick figures out), seam V (the mask; what
it reads of the labels on brick shells is not counted), flatten 8 V, rank 16 V (count 4, rank 4, gather 8), list 4 V:
38 V bytes.  scipy.ndimage.label gets the same mask on the host (`--scipy-repeats` runs, the fastest is reported); its
labels are checked against the device's partition.  One JSON line per case; `--out FILE` writes them as one document
(profiles/components_bench.json).

    python tools/components_bench.py [--iters 10] [--warmup 2] [--frames 40] [--sizes 256 512] [--out profiles/components_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from online_joint_depthfusion_and_semantic_amd import _lib, components, projective, synthetic  # noqa: E402

PHASES = (('brick', _lib.COMPONENTS_BRICK), ('seam', _lib.COMPONENTS_SEAM), ('flatten', _lib.COMPONENTS_FLATTEN),
          ('rank', _lib.COMPONENTS_RANK), ('list', _lib.COMPONENTS_LIST))
BYTES_PER_VOXEL = 38


def room_mask(grid, frames, dev):
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
    return components.observed_mask(tsdf, wgt)


def serpentine_mask(n, dev):
    m = torch.zeros((n, n, n), dtype=torch.uint8, device=dev)
    rows = (n + 1) // 2
    m[0::2, 0::2, :] = 1
    for r in range(rows - 1):
        m[0::2, 2 * r + 1, n - 1 if r % 2 == 0 else 0] = 1
    end = (2 * (rows - 1), n - 1 if rows % 2 == 1 else 0)
    for k in range(rows - 1):
        y, z = end if k % 2 == 0 else (0, 0)
        m[2 * k + 1, y, z] = 1
    return m, rows * (rows * n + rows - 1) + (rows - 1)


def time_passes(mask, connectivity, iters, warmup):
    """({phase: median us}, [total us per iteration], n) of the five phases on ``mask``."""
    lib = _lib.load()
    dev, (X, Y, Z) = mask.device, mask.shape
    st = _lib.stream_ptr(dev)
    ws_bytes = lib.ojf_volume_components_workspace_bytes(X, Y, Z)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    labels = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
    ids = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(phases, lists, cap):
        rc = lib.ojf_volume_components(mask.data_ptr(), None, X, Y, Z, connectivity, phases, ws.data_ptr(), ws_bytes, labels.data_ptr(),
                                       ids.data_ptr(), *(None if a is None else a.data_ptr() for a in lists), cap, count.data_ptr(), st)
        _lib.check(rc, 'ojf_volume_components')

    run(_lib.COMPONENTS_ALL, [None] * 4, 0)
    n = int(count.item())
    cap = max(n, 1)
    lists = [torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
             torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty((cap, 6), dtype=torch.int32, device=dev)]
    per = {name: [] for name, _ in PHASES}
    totals = []
    for it in range(warmup + iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 1)]
        torch.cuda.synchronize()
        ev[0].record()
        for i, (_, bit) in enumerate(PHASES):
            run(bit, lists, cap)
            ev[i + 1].record()
        ev[-1].synchronize()
        if it >= warmup:
            for i, (name, _) in enumerate(PHASES):
                per[name].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)
            totals.append(ev[0].elapsed_time(ev[-1]) * 1e3)
    return {k: statistics.median(v) for k, v in per.items()}, totals, n, labels, lists


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


def scipy_label(mask_host, connectivity, repeats):
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    best, lab, n = None, None, 0
    for _ in range(repeats):
        t0 = time.perf_counter()
        lab, n = ndimage.label(mask_host, structure=structure)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, lab, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--sizes', type=int, nargs='*', default=[256, 512])
    ap.add_argument('--scipy-repeats', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('components_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    rows = []
    cases = [('room_%d' % g, g, 26) for g in args.sizes] + [('serpentine_256', 256, 6)]
    for case, grid, connectivity in cases:
        if case.startswith('room'):
            mask, expect_size = room_mask(grid, args.frames, dev), None
        else:
            mask, expect_size = serpentine_mask(grid, dev)
        V = mask.numel()
        per, totals, n, labels, lists = time_passes(mask, connectivity, args.iters, args.warmup)
        sizes = lists[1][:n].cpu().numpy()
        if expect_size is not None and (n != 1 or int(sizes[0]) != expect_size):
            raise SystemExit('components_bench: the serpentine came out as {} components, largest {}'.format(n, sizes.max(initial=0)))
        copy_us = time_copy(BYTES_PER_VOXEL * V // 2, dev, args.iters, args.warmup)
        host = mask.cpu().numpy()
        scipy_s, lab, scipy_n = scipy_label(host, connectivity, args.scipy_repeats)
        got = labels.cpu().numpy()
        fg = host != 0
        pairs = np.unique(np.stack([got[fg].astype(np.int64), lab[fg].astype(np.int64)]), axis=1).shape[1]
        if not (scipy_n == n == pairs):
            raise SystemExit('components_bench: {} components on the device, {} by scipy, {} label pairs'.format(n, scipy_n, pairs))
        total = statistics.median(totals)
        row = {'case': case, 'grid': grid, 'connectivity': connectivity, 'voxels': V, 'foreground': int(fg.sum()), 'components': n,
               'largest_component': int(sizes.max(initial=0)), 'iters': args.iters,
               'pass_us': {k: round(v, 1) for k, v in per.items()}, 'total_us': round(total, 1),
               'total_us_min_max': [round(min(totals), 1), round(max(totals), 1)],
               'bytes_touched': BYTES_PER_VOXEL * V, 'copy_floor_us': round(copy_us, 1), 'total_over_floor': round(total / copy_us, 2),
               'scipy_label_ms': round(scipy_s * 1e3, 1), 'scipy_over_device': round(scipy_s * 1e6 / total, 1),
               'scipy_partition_equal': True}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del mask, labels, lists
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/components_bench.py', 'device': torch.cuda.get_device_name(0), 'frames': args.frames, 'cases': rows}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
