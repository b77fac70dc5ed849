"""Time of ojf_resample_volumes / ojf_resample_records (resample.resample_scene) beside the byte floor, for DESIGN.md 15: device
events around `--iters` calls after `--warmup`, the volumes prepared once.  Cases: a 256^3 scene (TSDF, weights, ids, scores:
7 B per voxel), the same with a 30-class record volume (S = 32: 64 B per voxel more), 512^3 -> 256^3 at twice the voxel size,
and a merge of two 256^3 scenes; each under a whole-voxel shift (3, -2, 5) and under a rotation of 17 degrees about the axis
(1, 2, 3) through the centre of the box.  The volumes hold random fp16 values with a third of the voxels unobserved at random
(the worst case for the "observed" branches; a fused room is sparser and more coherent).

The floor is not a figure fixed in advance: it is a device-to-device copy, timed in the same run, of as many bytes as the call
must touch - every source volume read once, every destination volume written once (and, in a merge, read once): a copy of n
bytes reads n and writes n, so the floor copies half of that sum.  For the same-size replace that is exactly a copy of the
volumes.  `--repeats` timed batches per case, call and copy taking turns; the median is reported with the smallest and the
largest batch.  One JSON line per case; `--out FILE` also writes the cases as one JSON document (profiles/resample_bench.json).

    python tools/resample_bench.py [--iters 20] [--warmup 3] [--repeats 5] [--out profiles/resample_bench.json]
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

from online_joint_depthfusion_and_semantic_amd import resample  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.label_probs import record_size  # noqa: E402

SHIFT = (3, -2, 5)
AXIS, ANGLE = (1.0, 2.0, 3.0), 17.0
C = 30


def random_scene(n, dev, records, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    shape = (n, n, n)
    s = {'tsdf': (torch.rand(shape, generator=g, device=dev) * 0.2 - 0.1).half()}
    w = (torch.rand(shape, generator=g, device=dev) * 40 + 0.5).half()
    w[torch.rand(shape, generator=g, device=dev) < 1.0 / 3.0] = 0
    s['weights'] = w
    s['ids'] = torch.randint(0, 40, shape, generator=g, device=dev, dtype=torch.uint8)
    s['scores'] = torch.rand(shape, generator=g, device=dev).half()
    if records:
        S = record_size(C)
        v = torch.rand(shape + (S,), generator=g, device=dev).half()
        v[..., C] = torch.randint(1, 9, shape, generator=g, device=dev).half()
        v[..., C][torch.rand(shape, generator=g, device=dev) < 1.0 / 3.0] = 0
        v[..., C + 1:] = 0
        s['label_probs'], s['n_classes'] = v, C
    return s


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def boxes(n_src, n_dst, res_src):
    """{name: resample_scene keywords} for a source box of n_src^3 at the origin and a destination of n_dst^3 over the same extent."""
    res_dst = res_src * n_src / n_dst
    centre = np.full(3, 0.5 * n_src * res_src)
    R = rotation(AXIS, ANGLE)
    T = np.concatenate([R, (centre - R @ centre)[:, None]], axis=1)
    base = dict(src_origin=np.zeros(3), src_resolution=res_src, dst_shape=(n_dst,) * 3, dst_resolution=res_dst)
    return {'shift': dict(base, dst_origin=res_src * np.array(SHIFT, np.float64)),
            'rotation': dict(base, dst_origin=np.zeros(3), transform=T)}


def nbytes(scene):
    return sum(v.numel() * v.element_size() for k, v in scene.items() if k != 'n_classes')


def time_pair(call, copy, iters, warmup, repeats):
    out = {'call': [], 'copy': []}
    for fn in (call, copy):
        for _ in range(warmup):
            fn()
    for _ in range(repeats):
        for name, fn in (('call', call), ('copy', copy)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('resample_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    rows = []
    for case, n_src, n_dst, records, merge in (('scene_256', 256, 256, False, False), ('scene_256_records', 256, 256, True, False),
                                               ('down_512_to_256', 512, 256, False, False), ('merge_256', 256, 256, False, True)):
        src = random_scene(n_src, dev, records, 1)
        dst = random_scene(n_dst, dev, records, 2)  # (replace mode overwrites every voxel of it; a merge updates it)
        touched = nbytes(src) + nbytes(dst) * (2 if merge else 1)
        a = torch.empty(touched // 2, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        for name, kw in boxes(n_src, n_dst, 0.02).items():
            if merge:
                def call(kw=kw):
                    resample.resample_scene(src, into=dst, init_value=0.1, **kw)
            else:
                # replace mode through the merge-free path of the public call: fresh volumes come from torch's caching allocator
                def call(kw=kw):
                    resample.resample_scene(src, init_value=0.1, **kw)
            out = resample.resample_scene(src, init_value=0.1, **kw)
            covered = float((out['weights'] > 0).float().mean())
            del out
            t = time_pair(call, lambda: b.copy_(a), args.iters, args.warmup, args.repeats)
            row = {'case': case, 'map': name, 'source': n_src, 'destination': n_dst, 'mode': 'merge' if merge else 'replace',
                   'record_classes': C if records else 0, 'covered_fraction': round(covered, 4), 'bytes_touched': touched,
                   'iters': args.iters, 'repeats': args.repeats,
                   'resample_us': round(t['call'][0], 1), 'resample_us_min_max': [round(t['call'][1], 1), round(t['call'][2], 1)],
                   'copy_floor_us': round(t['copy'][0], 1), 'copy_floor_us_min_max': [round(t['copy'][1], 1), round(t['copy'][2], 1)],
                   'resample_over_floor': round(t['call'][0] / t['copy'][0], 3),
                   'resample_gb_per_s': round(touched / t['call'][0] * 1e-3, 1), 'copy_gb_per_s': round(touched / t['copy'][0] * 1e-3, 1)}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del src, dst, a, b
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/resample_bench.py', 'device': torch.cuda.get_device_name(0), 'cases': rows}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
