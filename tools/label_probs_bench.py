"""Time of ojf_fuse_label_probs (both observation forms) beside ojf_fuse_color, and of ojf_label_decide, for DESIGN.md 14:
device events around `--iters` bare ABI calls after `--warmup`, with the inputs prepared once, per call and per view, for
frames of the synthetic room at 320x240 into a 256^3 volume with C = 30 classes (S = 32: 64 B per voxel, 1 GiB), n = 1 and
n = 8 views per call.  All kernels see the same depth, masks and poses in the same process and repeat on the same volumes
(the work of a call does not depend on what the voxels hold); the band of the label calls is the band of the colour call, so
all update the same voxels.  `--repeats` timed batches per kernel and case, the kernels taking turns; the median is reported,
with the smallest and the largest batch.  One JSON line per case, with the ratios to the colour call and the bytes a call
must move (2·S bytes each way per band voxel and view, C gathered floats per band voxel and view in the probability form);
`--out FILE` also writes the cases as one JSON document (profiles/label_probs_bench.json).

    python tools/label_probs_bench.py [--iters 100] [--warmup 5] [--repeats 5] [--out profiles/label_probs_bench.json]
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

from online_joint_depthfusion_and_semantic_amd import synthetic  # noqa: E402
from online_joint_depthfusion_and_semantic_amd import _lib  # noqa: E402
from online_joint_depthfusion_and_semantic_amd import color, label_probs  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.views import cameras  # noqa: E402


def raw_calls(colors, vol_l, vol_p, C, shape, origin, res, K, E, depth, mask, image, labels, probs, band):
    """(ojf_fuse_color, ojf_fuse_label_probs with labels, ojf_fuse_label_probs with probabilities) closures with the cameras
    and images prepared once."""
    lib = _lib.load()
    n, h, w = depth.shape
    _, Kh, Eh = cameras('label_probs_bench', K, E, n)
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float64))
    st = _lib.stream_ptr(colors.device)
    cargs = (_lib.ptr(colors), *shape, org.ctypes.data, float(res), n, Kh.ctypes.data, Eh.ctypes.data, _lib.ptr(depth),
             _lib.ptr(mask), _lib.ptr(image), h, w, float(band), 64.0, 0.0, st)
    head = (*shape, org.ctypes.data, float(res), n, Kh.ctypes.data, Eh.ctypes.data, _lib.ptr(depth), _lib.ptr(mask))
    largs = (_lib.ptr(vol_l), C, *head, None, 0, _lib.ptr(labels), h, w, float(band), 64.0, 0.0, st)
    pargs = (_lib.ptr(vol_p), C, *head, _lib.ptr(probs), probs.shape[-1], None, h, w, float(band), 64.0, 0.0, st)

    def fuse_color(keep=(Kh, Eh, org)):
        _lib.check(lib.ojf_fuse_color(*cargs), 'ojf_fuse_color')

    def fuse_labels(keep=(Kh, Eh, org)):
        _lib.check(lib.ojf_fuse_label_probs(*largs), 'ojf_fuse_label_probs')

    def fuse_probs(keep=(Kh, Eh, org)):
        _lib.check(lib.ojf_fuse_label_probs(*pargs), 'ojf_fuse_label_probs')
    return fuse_color, fuse_labels, fuse_probs


def time_calls(fns, iters, warmup, repeats):
    """{name: (median, min, max)} in us per call over `repeats` batches of `iters` calls per function, the functions taking turns
    batch by batch (what else runs on the machine then falls on all alike)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('label_probs_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    h, w, grid, band, C = 240, 320, 256, 0.1, 30
    S = label_probs.record_size(C)
    shape = (grid,) * 3
    origin, res, _ = synthetic.grid_spec(grid)
    st = synthetic.SyntheticStream(h, w, grid, 40, n_classes=C)
    fr = [st.frame(i) for i in range(8)]
    depth = torch.from_numpy(np.stack([f['tof_depth'] for f in fr])).to(dev)
    mask = torch.from_numpy(np.stack([f['mask'] for f in fr]).astype(np.uint8)).to(dev)
    labels = torch.from_numpy(np.stack([f['semantic_gt'] for f in fr]).astype(np.uint8)).to(dev)
    rng = np.random.default_rng(0)
    image = color.pack_image(torch.from_numpy(rng.integers(0, 256, (8, h, w, 3)).astype(np.uint8)).to(dev), 8, h, w, dev)
    probs = torch.softmax(torch.from_numpy(rng.normal(0.0, 2.0, (8, h, w, C)).astype(np.float32)), dim=-1)
    probs = torch.nn.functional.pad(probs, (0, 32 - C)).contiguous().to(dev)  # rows of 32 floats, as SegEngine.predict_probs gives them
    E = np.stack([f['extrinsics'] for f in fr])
    ids = torch.zeros(shape, dtype=torch.uint8, device=dev)
    scores = torch.zeros(shape, dtype=torch.float16, device=dev)
    lib = _lib.load()
    cases = []
    for n in (1, 8):
        colors = color.new_volume(shape, dev)
        vol_l, vol_p = label_probs.new_volume(shape, C, dev), label_probs.new_volume(shape, C, dev)
        fns = raw_calls(colors, vol_l, vol_p, C, shape, origin, res, st.K, E[:n], depth[:n].contiguous(), mask[:n].contiguous(),
                        image[:n].contiguous(), labels[:n].contiguous(), probs[:n].contiguous(), band)
        for fn in fns:
            fn()
        voted = int((vol_l[..., C] > 0).sum())
        assert voted == int((colors[..., 3] > 0).sum()) == int((vol_p[..., C] > 0).sum())  # the same voxels
        updates = int(vol_l[..., C].float().sum())  # (voxel, view) pairs inside the band: one read and one write of a record each
        row = {'case': 'label_probs_vs_color', 'grid': grid, 'h': h, 'w': w, 'n_classes': C, 'record_bytes': 2 * S, 'n': n,
               'iters': args.iters, 'repeats': args.repeats, 'updated_fraction': round(voted / grid ** 3, 5),
               'band_voxel_views': updates, 'record_bytes_read_and_written': 2 * updates * 2 * S,
               'probability_bytes_gathered': updates * 4 * C}
        times = time_calls({'color': fns[0], 'labels': fns[1], 'probs': fns[2]}, args.iters, args.warmup, args.repeats)
        for name, (med, lo, hi) in times.items():
            row[name + '_us_per_call'] = round(med, 2)
            row[name + '_us_per_view'] = round(med / n, 2)
            row[name + '_us_per_call_min_max'] = [round(lo, 2), round(hi, 2)]
        row['labels_over_color'] = round(row['labels_us_per_call'] / row['color_us_per_call'], 3)
        row['probs_over_color'] = round(row['probs_us_per_call'] / row['color_us_per_call'], 3)
        print(json.dumps(row), flush=True)
        cases.append(row)
        if n == 8:  # the decision over the volume the eight views voted in
            args_d = (_lib.ptr(vol_l), C, *shape, _lib.ptr(ids), _lib.ptr(scores), _lib.stream_ptr(dev))

            def decide():
                _lib.check(lib.ojf_label_decide(*args_d), 'ojf_label_decide')
            med, lo, hi = time_calls({'decide': decide}, args.iters, args.warmup, args.repeats)['decide']
            row = {'case': 'label_decide', 'grid': grid, 'n_classes': C, 'record_bytes': 2 * S, 'decided_fraction': round(voted / grid ** 3, 5),
                   'iters': args.iters, 'repeats': args.repeats, 'decide_us_per_call': round(med, 2),
                   'decide_us_per_call_min_max': [round(lo, 2), round(hi, 2)],
                   'bytes_read': 2 * grid ** 3 + 2 * C * voted, 'bytes_written': 3 * voted}
            print(json.dumps(row), flush=True)
            cases.append(row)
        del colors, vol_l, vol_p
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/label_probs_bench.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
