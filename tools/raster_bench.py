"""Time of ojf_rasterize for DESIGN.md 12: device events around `--iters` bare ABI calls after `--warmup`, with the mesh,
the cameras and the outputs prepared once.  Two meshes of the synthetic room - the one `mesh.extract_mesh` makes of its
256^3 ground-truth volume (marching tetrahedra: small triangles, many of them) and the box room itself (a few triangles
that fill the screen) - at 320x240 and 640x480, n = 1 and n = 8 orbit views per call.  In the same process ojf_render
ray-casts the 256^3 volume at the same views (depth only), for scale; the two calls take turns batch by batch.  `--repeats`
timed batches per call and case; the median is reported with the smallest and the largest batch.  One JSON line per case;
`--out FILE` also writes the cases as one JSON document (profiles/raster_bench.json).  The rasterised depth of the
extracted mesh is compared with the ray-cast depth on the way (median absolute difference, in the JSON).

    python tools/raster_bench.py [--iters 50] [--warmup 5] [--repeats 5] [--out profiles/raster_bench.json]
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

from online_joint_depthfusion_and_semantic_amd import _lib, mesh, synthetic  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.views import cameras, inverse_cameras  # noqa: E402


def box_room():
    """The room and its three solids as closed boxes, two triangles per side (the mesh of tests/raster_ref.room_mesh)."""
    verts, faces = [], []
    for s, (lo, hi) in enumerate([(synthetic.ROOM_MIN, synthetic.ROOM_MAX)] + list(synthetic._SOLIDS)):
        c = (lo, hi)
        verts += [[c[i][0], c[j][1], c[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
        for q in ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)):
            faces += [[8 * s + q[0], 8 * s + q[1], 8 * s + q[2]], [8 * s + q[0], 8 * s + q[2], 8 * s + q[3]]]
    return np.array(verts, np.float32), np.array(faces, np.int32)


def time_calls(fns, iters, warmup, repeats):
    """{name: (median, min, max)} in us per call over `repeats` batches of `iters` calls per function, the functions taking
    turns batch by batch."""
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
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--grid', type=int, default=256)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('raster_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    stream = _lib.stream_ptr(dev)
    grid, trunc = args.grid, 0.1
    origin, res, _ = synthetic.grid_spec(grid)
    tsdf = torch.from_numpy(synthetic.gt_volumes(grid, trunc)[0]).to(dev)
    m = mesh.extract_mesh(tsdf, origin=origin + 0.5 * res, resolution=res)  # (voxel (i,j,k) has its centre at origin + (i + 0.5)·res)
    meshes = {'extracted_{}'.format(grid): (m['vertices'].astype(np.float32), m['faces'].astype(np.int32)), 'box_room': box_room()}
    org = np.ascontiguousarray(origin, dtype=np.float64)
    cases = []
    for name, (verts, faces) in meshes.items():
        v, f = torch.from_numpy(verts).to(dev).contiguous(), torch.from_numpy(faces).to(dev).contiguous()
        for h, w in ((240, 320), (480, 640)):
            K = synthetic.intrinsics(h, w)
            for n in (1, 8):
                E = np.stack([synthetic.camera_pose(2.0 * np.pi * i / 8) for i in range(n)])
                _, Kh, Eh = cameras('raster_bench', K, E, n)
                _, Ki, Ef = inverse_cameras('raster_bench', K, E)
                keys = torch.empty((n, h, w), dtype=torch.int64, device=dev)
                depth = torch.empty((n, h, w), dtype=torch.float32, device=dev)
                face = torch.empty((n, h, w), dtype=torch.int32, device=dev)
                cast = torch.empty((n, h, w), dtype=torch.float32, device=dev)
                rargs = (_lib.ptr(v), len(verts), _lib.ptr(f), len(faces), n, Kh.ctypes.data, Eh.ctypes.data, h, w, 0.0, _lib.ptr(keys),
                         _lib.ptr(depth), _lib.ptr(face), stream)
                cargs = (_lib.ptr(tsdf), None, None, grid, grid, grid, org.ctypes.data, float(res), n, Ki.ctypes.data, Ef.ctypes.data, h, w,
                         0.0, _lib.ptr(cast), None, None, stream)

                def rasterize():
                    _lib.check(lib.ojf_rasterize(*rargs), 'ojf_rasterize')

                def render():
                    _lib.check(lib.ojf_render(*cargs), 'ojf_render')
                rasterize()
                render()
                both = (depth > 0) & (cast > 0)
                row = {'case': 'rasterize_vs_render', 'mesh': name, 'vertices': len(verts), 'triangles': len(faces), 'h': h, 'w': w, 'n': n,
                       'grid': grid, 'iters': args.iters, 'repeats': args.repeats,
                       'covered_fraction': round(float((depth > 0).float().mean()), 5),
                       'median_abs_depth_difference_to_render_m': round(float((depth - cast)[both].abs().median()), 6)}
                for key, (med, lo, hi) in time_calls({'rasterize': rasterize, 'render': render}, args.iters, args.warmup, args.repeats).items():
                    row[key + '_us_per_call'] = round(med, 2)
                    row[key + '_us_per_view'] = round(med / n, 2)
                    row[key + '_us_per_call_min_max'] = [round(lo, 2), round(hi, 2)]
                row['rasterize_over_render'] = round(row['rasterize_us_per_call'] / row['render_us_per_call'], 3)
                print(json.dumps(row), flush=True)
                cases.append(row)
    if args.out:
        with open(args.out, 'w') as fo:
            json.dump({'tool': 'tools/raster_bench.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, fo, indent=1)
            fo.write('\n')


if __name__ == '__main__':
    main()
