"""Time of ojf_mesh_distance / ojf_mesh_distance_sign for DESIGN.md 16: device events around bare ABI calls after a
warm-up, with the mesh, the workspace, the lists and the outputs prepared once.  Two meshes of the synthetic room - the one
`mesh.extract_mesh` makes of its 256^3 ground-truth volume (about 2 M small triangles) and the box room itself (48
triangles, walls that span every brick) - into 256^3 and 512^3 voxels over the room's box, with a band of one voxel and of
the truncation distance (0.24 m).  Each phase of the call (bin = count, scan, fill, gather = the distance kernel) is timed
on its own through the `phases` argument, then the whole call, then the sign kernel; `--repeats` timed batches each, the
median reported with the smallest and the largest batch; a batch holds as many calls as fit `--batch-ms` (at least one).
With them the number of (triangle, brick) pairs and the lengths of the bricks' lists (median and maximum over the
non-empty bricks).  In the same process `rasterize.ground_truth_grid` fuses 20 views of 240 x 320 of the box room into the
same volume, for scale (host time of the whole Python call, synchronised).  One JSON line per case; `--out FILE` also writes
the cases as one JSON document (profiles/mesh_distance_bench.json).

    python tools/mesh_distance_bench.py [--grids 256 512] [--repeats 5] [--batch-ms 300] [--out profiles/mesh_distance_bench.json]
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

from online_joint_depthfusion_and_semantic_amd import _lib, mesh, synthetic  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.mesh_distance import pseudonormals  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.rasterize import ground_truth_grid  # noqa: E402

TRUNC = 0.24


def box_room():
    """The room and its three solids as closed boxes, two triangles per side (the mesh of tests/raster_ref.room_mesh)."""
    verts, faces = [], []
    for s, (lo, hi) in enumerate([(synthetic.ROOM_MIN, synthetic.ROOM_MAX)] + list(synthetic._SOLIDS)):
        c = (lo, hi)
        verts += [[c[i][0], c[j][1], c[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
        for q in ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)):
            faces += [[8 * s + q[0], 8 * s + q[1], 8 * s + q[2]], [8 * s + q[0], 8 * s + q[2], 8 * s + q[3]]]
    return np.array(verts, np.float32), np.array(faces, np.int32)


def time_call(fn, warmup, repeats, batch_ms):
    """(median, min, max, calls per batch) in us per call over `repeats` batches."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    iters = int(max(1, min(200, batch_ms / max(a.elapsed_time(b), 1e-3))))
    for _ in range(warmup if iters > 1 else 0):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(out), min(out), max(out), iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grids', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--mesh-grid', type=int, default=256)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch-ms', type=float, default=300.0)
    ap.add_argument('--views', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mesh_distance_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    stream = _lib.stream_ptr(dev)
    mg = args.mesh_grid
    m_origin, m_res, _ = synthetic.grid_spec(mg)
    tsdf = torch.from_numpy(synthetic.gt_volumes(mg, 0.1)[0]).to(dev)
    m = mesh.extract_mesh(tsdf, origin=m_origin + 0.5 * m_res, resolution=m_res)
    del tsdf
    meshes = {'box_room': box_room(), 'extracted_{}'.format(mg): (m['vertices'].astype(np.float32), m['faces'].astype(np.int32))}
    normals = {name: pseudonormals(*vf) for name, vf in meshes.items()}
    cases = []
    for grid in args.grids:
        origin, res, _ = synthetic.grid_spec(grid)
        org = np.ascontiguousarray(origin, dtype=np.float64)
        X = Y = Z = grid
        ws_bytes = lib.ojf_mesh_distance_workspace_bytes(X, Y, Z)
        nb = ((grid + 7) // 8) ** 3
        dist = torch.empty((X, Y, Z), dtype=torch.float32, device=dev)
        face = torch.empty((X, Y, Z), dtype=torch.int32, device=dev)
        sgn = torch.empty((X, Y, Z), dtype=torch.float32, device=dev)
        # ground_truth_grid, for scale
        verts, faces = meshes['box_room']
        K = synthetic.intrinsics(240, 320)
        E = np.stack([synthetic.camera_pose(2.0 * np.pi * i / 40) for i in range(args.views)])
        gv = torch.from_numpy(verts).to(dev)
        gt_ms = {}
        for mode in ('projective', 'euclidean'):
            times = []
            for _ in range(1 + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ground_truth_grid(gv, faces, origin=org, resolution=res, shape=(X, Y, Z), truncation=TRUNC, intrinsics=K, extrinsics=E,
                                  image_shape=(240, 320), distance=mode)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            gt_ms[mode] = round(statistics.median(times[1:]), 3)
        for name, (verts, faces) in meshes.items():
            v, f = torch.from_numpy(verts).to(dev).contiguous(), torch.from_numpy(faces).to(dev).contiguous()
            vn, en, fe = (torch.from_numpy(a).to(dev) for a in normals[name])
            for band_name, band in (('one_voxel', float(res)), ('truncation', TRUNC)):
                ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
                count = torch.zeros(1, dtype=torch.int64, device=dev)
                head = (_lib.ptr(v), len(verts), _lib.ptr(f), len(faces), org.ctypes.data, float(res), X, Y, Z, band)
                _lib.check(lib.ojf_mesh_distance(*head, _lib.MESH_DISTANCE_ALL, _lib.ptr(ws), ws_bytes, None, 0, _lib.ptr(count), None, None,
                                                 stream), 'ojf_mesh_distance')
                n_pairs = int(count.item())
                if n_pairs >= 2 ** 31:
                    print(json.dumps({'case': 'mesh_distance', 'mesh': name, 'grid': grid, 'band': band_name, 'pairs': n_pairs, 'skipped': 'too many pairs'}))
                    continue
                pairs = torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)
                counts = ws[:4 * nb].view(torch.int32).cpu().numpy().astype(np.int64)
                filled = counts[counts > 0]

                def call(phases):
                    _lib.check(lib.ojf_mesh_distance(*head, phases, _lib.ptr(ws), ws_bytes, _lib.ptr(pairs), pairs.numel(), _lib.ptr(count),
                                                     _lib.ptr(dist), _lib.ptr(face), stream), 'ojf_mesh_distance')

                def sign():
                    _lib.check(lib.ojf_mesh_distance_sign(*head[:9], _lib.ptr(dist), _lib.ptr(face), _lib.ptr(vn), _lib.ptr(en), en.shape[0],
                                                          _lib.ptr(fe), _lib.ptr(sgn), stream), 'ojf_mesh_distance_sign')
                call(_lib.MESH_DISTANCE_ALL)
                row = {'case': 'mesh_distance', 'mesh': name, 'vertices': len(verts), 'triangles': len(faces), 'grid': grid, 'band': band_name,
                       'band_m': round(band, 5), 'bricks': nb, 'pairs': n_pairs, 'non_empty_bricks': int(len(filled)),
                       'list_length_median': float(np.median(filled)) if len(filled) else 0.0,
                       'list_length_mean': round(float(filled.mean()), 1) if len(filled) else 0.0,
                       'list_length_max': int(filled.max()) if len(filled) else 0,
                       'voxels_in_band_fraction': round(float(torch.isfinite(dist).float().mean()), 5), 'repeats': args.repeats}
                steps = (('bin', _lib.MESH_DISTANCE_BIN), ('scan', _lib.MESH_DISTANCE_SCAN), ('fill', _lib.MESH_DISTANCE_FILL),
                         ('distance', _lib.MESH_DISTANCE_GATHER), ('all_phases', _lib.MESH_DISTANCE_ALL))
                for key, phases in steps:
                    med, lo, hi, iters = time_call(lambda: call(phases), args.warmup, args.repeats, args.batch_ms)
                    row[key + '_us'] = round(med, 2)
                    row[key + '_us_min_max'] = [round(lo, 2), round(hi, 2)]
                    row[key + '_calls_per_batch'] = iters
                med, lo, hi, iters = time_call(sign, args.warmup, args.repeats, args.batch_ms)
                row['sign_us'], row['sign_us_min_max'] = round(med, 2), [round(lo, 2), round(hi, 2)]
                row['ground_truth_grid_{}_views_ms'.format(args.views)] = gt_ms
                print(json.dumps(row), flush=True)
                cases.append(row)
                if args.out:  # (after every case: a long run that is cut short keeps what it measured)
                    with open(args.out, 'w') as fo:
                        json.dump({'tool': 'tools/mesh_distance_bench.py', 'device': torch.cuda.get_device_name(0), 'cases': cases}, fo, indent=1)
                        fo.write('\n')
                del pairs


if __name__ == '__main__':
    main()
