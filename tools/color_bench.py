"""Time of ojf_fuse_color beside ojf_fuse_projective for DESIGN.md 11: device events around `--iters` bare ABI calls after
`--warmup`, with the inputs prepared once, per call and per view, for frames of the synthetic room at 320x240 into a 256^3
volume, n = 1 and n = 8 views per call.  Both kernels see the same depth, masks and poses in the same process and repeat on
the same volumes (the work of a call does not depend on what the voxels hold); the band of the colour call is the truncation
of the depth call (carve off), so both update the same voxels.  `--repeats` timed batches per kernel and case, the two
kernels taking turns; the median is reported, with the smallest and the largest batch.  One JSON line per case, with the
ratio colour / projective; `--out FILE` also writes the cases as one JSON document (profiles/color_bench.json).

    python tools/color_bench.py [--iters 300] [--warmup 10] [--repeats 7] [--out profiles/color_bench.json]
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
from online_joint_depthfusion_and_semantic_amd.color import new_volume, pack_image  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.views import cameras  # noqa: E402


def raw_calls(tsdf, wgt, colors, origin, res, K, E, depth, mask, image, band):
    """(ojf_fuse_projective, ojf_fuse_color) closures with the cameras and images prepared once."""
    lib = _lib.load()
    n, h, w = depth.shape
    _, Kh, Eh = cameras('color_bench', K, E, n)
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float64))
    st = _lib.stream_ptr(tsdf.device)
    pargs = (_lib.ptr(tsdf), _lib.ptr(wgt), None, None, *tsdf.shape, org.ctypes.data, float(res), n, Kh.ctypes.data, Eh.ctypes.data,
             _lib.ptr(depth), _lib.ptr(mask), None, None, h, w, float(band), 128.0, 0.0, 0, st)
    cargs = (_lib.ptr(colors), *tsdf.shape, org.ctypes.data, float(res), n, Kh.ctypes.data, Eh.ctypes.data, _lib.ptr(depth),
             _lib.ptr(mask), _lib.ptr(image), h, w, float(band), 64.0, 0.0, st)

    def projective(keep=(Kh, Eh, org)):
        _lib.check(lib.ojf_fuse_projective(*pargs), 'ojf_fuse_projective')

    def color(keep=(Kh, Eh, org)):
        _lib.check(lib.ojf_fuse_color(*cargs), 'ojf_fuse_color')
    return projective, color


def time_calls(fns, iters, warmup, repeats):
    """{name: (median, min, max)} in us per call over `repeats` batches of `iters` calls per function, the functions taking turns
    batch by batch (what else runs on the machine then falls on both alike)."""
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
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('color_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    h, w, grid, band = 240, 320, 256, 0.1
    origin, res, _ = synthetic.grid_spec(grid)
    st = synthetic.SyntheticStream(h, w, grid, 40)
    fr = [st.frame(i) for i in range(8)]
    depth = torch.from_numpy(np.stack([f['tof_depth'] for f in fr])).to(dev)
    mask = torch.from_numpy(np.stack([f['mask'] for f in fr]).astype(np.uint8)).to(dev)
    rng = np.random.default_rng(0)
    image = pack_image(torch.from_numpy(rng.integers(0, 256, (8, h, w, 3)).astype(np.uint8)).to(dev), 8, h, w, dev)
    E = np.stack([f['extrinsics'] for f in fr])
    cases = []
    for n in (1, 8):
        tsdf = torch.full((grid,) * 3, band, dtype=torch.float16, device=dev)
        wgt = torch.zeros((grid,) * 3, dtype=torch.float16, device=dev)
        colors = new_volume((grid,) * 3, dev)
        projective, color = raw_calls(tsdf, wgt, colors, origin, res, st.K, E[:n], depth[:n].contiguous(), mask[:n].contiguous(),
                                      image[:n].contiguous(), band)
        projective()
        color()
        updated = float((wgt > 0).float().mean())
        assert int((wgt > 0).sum()) == int((colors[..., 3] > 0).sum())  # the same voxels
        row = {'case': 'color_vs_projective', 'grid': grid, 'h': h, 'w': w, 'n': n, 'iters': args.iters, 'repeats': args.repeats,
               'updated_fraction': round(updated, 5)}
        times = time_calls({'projective': projective, 'color': color}, args.iters, args.warmup, args.repeats)
        for name, (med, lo, hi) in times.items():
            row[name + '_us_per_call'] = round(med, 2)
            row[name + '_us_per_view'] = round(med / n, 2)
            row[name + '_us_per_call_min_max'] = [round(lo, 2), round(hi, 2)]
        row['color_over_projective'] = round(row['color_us_per_call'] / row['projective_us_per_call'], 3)
        print(json.dumps(row), flush=True)
        cases.append(row)
        del tsdf, wgt, colors
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'tool': 'tools/color_bench.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
