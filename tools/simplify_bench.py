"""Time of the mesh simplification (ojf_mesh_simplify phase by phase) beside a byte floor and beside the numpy restatement on the
host of the same node, for DESIGN.md 19.

Cases `room_256` and `room_512`: the synthetic room's ground-truth volume at that size, extracted and welded on the device
(mesh.extract_triangles + mesh.weld, what mesh.extract_mesh does), simplified with cells of `--cells` voxels (1, 2, 4) on the grid
mesh_simplify.cluster chooses.

Every timed iteration runs the seven phases as seven calls with device events between them, after `--warmup` iterations; medians
over `--iters` iterations, and the smallest and largest total.  The floor is a device-to-device copy, timed in the same run, of half
the bytes the phases must read and write (a copy of n bytes reads n and writes n), counted by `bytes_touched` from nv vertices, nf
faces, W bitmap words, nc clusters and nk kept faces; an atomic counts as the bytes it adds (8 per 64-bit integer).  The numpy
restatement (tests/simplify_ref.py) gets the same mesh on the host for the sizes in `--ref-sizes`, once per cell size; all four of
its outputs are checked bit for bit against the device's.  One JSON line per case; `--out FILE` appends this run, labelled
`--label`, to the document's list of runs (profiles/simplify_bench.json).

    python tools/simplify_bench.py [--iters 10] [--warmup 2] [--sizes 256 512] [--cells 1 2 4] [--ref-sizes 256] [--label NAME] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from online_joint_depthfusion_and_semantic_amd import _lib, mesh, mesh_simplify, synthetic  # noqa: E402

PHASES = (('mark', _lib.SIMPLIFY_MARK), ('scan', _lib.SIMPLIFY_SCAN), ('count', _lib.SIMPLIFY_COUNT), ('accumulate', _lib.SIMPLIFY_ACCUMULATE),
          ('solve', _lib.SIMPLIFY_SOLVE), ('nearest', _lib.SIMPLIFY_NEAREST), ('faces', _lib.SIMPLIFY_FACES))


def bytes_touched(nv, nf, W, nc, nk):
    """Bytes each phase must read and write (gathers counted once per use, atomics as the bytes they add)."""
    face_in = 12 * nf + 3 * 4 * nf + 3 * 12 * nf  # indices, the corners' clusters, the corners' positions
    return {'mark': 12 * nv + 8 * nv + 4 * W + 4 * nv,          # vertices in, cell and position out, the bitmap cleared, one atomicOr each
            'scan': 3 * 4 * W + 4 * nv + 8 * nv + 4 * nv,        # words read twice, prefix out; rank: cell in, word and prefix gathered, out
            'count': face_in + 4 * (nf // 256 + 1) * 3,
            'accumulate': 128 * nc + 8 * W + 4 * nc + 8 * nv + 32 * nv + face_in + 3 * 4 * nf + 27 * 8 * nf,
            'solve': 128 * nc + 12 * nc + 20 * nc,
            'nearest': 12 * nv + 4 * nv + 12 * nv + 8 * nv + 8 * nc + 4 * nc,
            'faces': face_in + 16 * nk}


def room_mesh(grid, dev):
    origin, res, _ = synthetic.grid_spec(grid)
    tsdf = torch.from_numpy(synthetic.gt_volumes(grid, 0.1)[0]).to(dev)
    tri, _, keys = mesh.extract_triangles(tsdf, origin=origin + 0.5 * res, resolution=res, keys=True)
    verts, faces, _ = mesh.weld(tri, None, keys, n_voxels=tsdf.numel())
    return verts.contiguous(), faces.to(torch.int32).contiguous(), float(res)


def time_phases(verts, faces, cell, iters, warmup):
    """({phase: median us}, [total us per iteration], outputs, (W, nc, nk, grid))."""
    lib = _lib.load()
    dev = verts.device
    st = _lib.stream_ptr(dev)
    nv, nf = verts.shape[0], faces.shape[0]
    cell = float(np.float32(cell))
    lo, grid = mesh_simplify.default_grid(verts.min(dim=0).values.tolist(), verts.max(dim=0).values.tolist(), cell)
    ws_bytes = lib.ojf_mesh_simplify_workspace_bytes(nv, nf, *grid)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    buf = {'rows': None, 'v': None, 's': None, 'f': None, 'fs': None}

    def call(phases):
        cap_v = 0 if buf['v'] is None else buf['v'].shape[0]
        cap_f = 0 if buf['f'] is None else buf['f'].shape[0]
        _lib.check(lib.ojf_mesh_simplify(_lib.ptr(verts), nv, _lib.ptr(faces), nf, lo.ctypes.data, cell, grid[0], grid[1], grid[2], phases,
                                         _lib.ptr(ws), ws_bytes, _lib.ptr(buf['rows']), 0 if buf['rows'] is None else buf['rows'].numel(),
                                         _lib.ptr(buf['v']), _lib.ptr(buf['s']), cap_v, _lib.ptr(buf['f']), _lib.ptr(buf['fs']), cap_f,
                                         _lib.ptr(counts), st), 'ojf_mesh_simplify')

    call(_lib.SIMPLIFY_MARK | _lib.SIMPLIFY_SCAN | _lib.SIMPLIFY_COUNT)
    nc, nk = counts.tolist()
    buf['rows'] = torch.empty(lib.ojf_mesh_simplify_cluster_bytes(nc), dtype=torch.uint8, device=dev)
    buf['v'] = torch.empty((nc, 3), dtype=torch.float32, device=dev)
    buf['s'] = torch.empty(nc, dtype=torch.int32, device=dev)
    buf['f'] = torch.empty((max(nk, 1), 3), dtype=torch.int32, device=dev)
    buf['fs'] = torch.empty(max(nk, 1), dtype=torch.int32, device=dev)
    per = {name: [] for name, _ in PHASES}
    totals = []
    for it in range(warmup + iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 1)]
        torch.cuda.synchronize()
        ev[0].record()
        for i, (_, bit) in enumerate(PHASES):
            call(bit)
            ev[i + 1].record()
        ev[-1].synchronize()
        if it >= warmup:
            for i, (name, _) in enumerate(PHASES):
                per[name].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)
            totals.append(ev[0].elapsed_time(ev[-1]) * 1e3)
    assert counts.tolist() == [nc, nk]
    out = (buf['v'], buf['f'][:nk], buf['s'], buf['fs'][:nk])
    return {k: statistics.median(v) for k, v in per.items()}, totals, out, ((grid[0] * grid[1] * grid[2] + 31) // 32, nc, nk, grid, lo)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sizes', type=int, nargs='*', default=[256, 512])
    ap.add_argument('--cells', type=float, nargs='*', default=[1, 2, 4])
    ap.add_argument('--ref-sizes', type=int, nargs='*', default=[256])
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('simplify_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    rows = []
    for grid in args.sizes:
        verts, faces, res = room_mesh(grid, dev)
        nv, nf = verts.shape[0], faces.shape[0]
        host = (verts.cpu().numpy(), faces.cpu().numpy()) if grid in args.ref_sizes else None
        for cells in args.cells:
            per, totals, out, (W, nc, nk, G, lo) = time_phases(verts, faces, cells * res, args.iters, args.warmup)
            touched = bytes_touched(nv, nf, W, nc, nk)
            n_bytes = sum(touched.values())
            copy_us = time_copy(n_bytes // 2, dev, args.iters, args.warmup)
            total = statistics.median(totals)
            row = {'case': 'room_%d_cell_%g' % (grid, cells), 'grid': grid, 'resolution': res, 'cell_voxels': cells, 'vertices': nv, 'faces': nf,
                   'cell_grid': list(G), 'bitmap_words': W, 'clusters': nc, 'kept_faces': nk, 'iters': args.iters,
                   'phase_us': {k: round(v, 1) for k, v in per.items()}, 'total_us': round(total, 1),
                   'total_us_min_max': [round(min(totals), 1), round(max(totals), 1)], 'bytes_touched': n_bytes,
                   'phase_bytes': touched, 'copy_floor_us': round(copy_us, 1), 'total_over_floor': round(total / copy_us, 2)}
            if host is not None:
                import simplify_ref
                t0 = time.perf_counter()
                want = simplify_ref.cluster(host[0], host[1], lo, np.float32(cells * res), G)
                row['numpy_restatement_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
                got = [t.cpu().numpy() for t in out]
                same = (np.array_equal(got[0].view(np.uint32), want.vertices.view(np.uint32)) and np.array_equal(got[1], want.faces) and
                        np.array_equal(got[2], want.source) and np.array_equal(got[3], want.face_source))
                if not same:
                    raise SystemExit('simplify_bench: the device differs from the restatement at {}'.format(row['case']))
                row['restatement_equal'] = True
                row['numpy_over_device'] = round(row['numpy_restatement_ms'] * 1e3 / total, 1)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del out
        del verts, faces
        torch.cuda.empty_cache()
    if args.out:
        doc = {'tool': 'tools/simplify_bench.py', 'runs': []}
        if os.path.exists(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc['runs'].append({'label': args.label, 'device': torch.cuda.get_device_name(0), 'cases': rows})
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
