"""Time of the registration (registration.register_volumes: ojf_register_select, signed_distance_field, ojf_register stage by
stage) beside a byte floor, for DESIGN.md 21.

Case `room_256`: the synthetic room sampled analytically on the 256^3 grid (2 cm voxels, truncation 10 cm, voxels more than the
truncation behind the surface unobserved) against the same room in a world turned by 17 degrees about (1,2,3), in a box of
another shape and origin; band 6 cm, the default two stages (coarse: signed distance field, stride 2; fine: TSDF, stride 1; 10
iterations each; the coarse field up to registration.coarse_reach, 0.64 m).

Timed with device events after `--warmup` runs, medians over `--iters`: the selection (count + fill, per stride), the signed
distance field, every iteration of each stage as its own one-iteration ojf_register call (one associate and one solve launch;
`rocprofv3 --kernel-trace --stats` on this tool splits the pair into its two kernels), each stage as one call, and the whole
register_volumes call (host work and both copies back included, wall clock).  The floor is a device-to-device copy, timed in
the same run, of half the bytes one iteration of a stage touches (a copy of n bytes reads n and writes n), counted per point:
the list entry (4), the moving TSDF (2) and eight corners of the field (8 x 4: fp16 TSDF + fp16 weight, or one f32) - 38 bytes.
One JSON document; `--out FILE` writes it (profiles/register_bench.json).

    python tools/register_bench.py [--iters 10] [--warmup 2] [--grid 256] [--degrees 17] [--out profiles/register_bench.json]
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

from online_joint_depthfusion_and_semantic_amd import _lib, registration, synthetic  # noqa: E402

BYTES_PER_POINT = 38


def scene_sdf(p):
    """synthetic.scene_sdf in torch (f64), for points [...,3] on the device."""
    lo = torch.tensor(synthetic.ROOM_MIN, dtype=torch.float64, device=p.device)
    hi = torch.tensor(synthetic.ROOM_MAX, dtype=torch.float64, device=p.device)
    sdf = torch.minimum(p - lo, hi - p).min(dim=-1).values
    for a, b in synthetic._SOLIDS:
        c = torch.tensor(0.5 * (a + b), dtype=torch.float64, device=p.device)
        e = torch.tensor(0.5 * (b - a), dtype=torch.float64, device=p.device)
        q = (p - c).abs() - e
        box = q.clamp(min=0.0).norm(dim=-1) + q.max(dim=-1).values.clamp(max=0.0)
        sdf = torch.minimum(sdf, box)
    return sdf


def sampled_scene(shape, origin, res, trunc, world_from_room, dev):
    tsdf = torch.empty(shape, dtype=torch.float16, device=dev)
    wgt = torch.empty(shape, dtype=torch.float16, device=dev)
    R = torch.tensor(world_from_room[:, :3], dtype=torch.float64, device=dev)
    t = torch.tensor(world_from_room[:, 3], dtype=torch.float64, device=dev)
    ay = origin[1] + (torch.arange(shape[1], dtype=torch.float64, device=dev) + 0.5) * res
    az = origin[2] + (torch.arange(shape[2], dtype=torch.float64, device=dev) + 0.5) * res
    yy, zz = torch.meshgrid(ay, az, indexing='ij')
    for i in range(shape[0]):  # slab by slab keeps the peak memory small
        pts = torch.stack([torch.full_like(yy, origin[0] + (i + 0.5) * res), yy, zz], dim=-1)
        sd = scene_sdf((pts - t) @ R)
        tsdf[i] = sd.clamp(-trunc, trunc).to(torch.float16)
        wgt[i] = (sd > -trunc).to(torch.float16)
    return dict(tsdf=tsdf, weights=wgt, origin=np.asarray(origin, np.float64), resolution=float(res))


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = np.radians(degrees)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def timed(fn, iters, warmup):
    """Median device time of fn() in microseconds."""
    out = []
    for it in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--grid', type=int, default=256)
    ap.add_argument('--degrees', type=float, default=17.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('register_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    grid = args.grid
    origin, res, _ = synthetic.grid_spec(grid)
    trunc, band = 5.0 * res, 3.0 * res
    W = np.concatenate([rotation((1, 2, 3), args.degrees), np.array([[0.30], [-0.20], [0.15]])], axis=1)
    fshape = (grid * 21 // 16, grid * 5 // 4, grid)
    forigin = W[:, 3] - 0.5 * res * np.array(fshape) + np.array([0.013, 0.021, -0.017])
    moving = sampled_scene((grid,) * 3, origin, res, trunc, np.eye(4)[:3], dev)
    fixed = sampled_scene(fshape, forigin, res, trunc, W, dev)
    corners = np.array([[x, y, z] for x in (-2.4, 2.4) for y in (-2.4, 2.4) for z in (-1.4, 1.4)])

    def error(P):
        d = corners @ (P[:, :3] - W[:, :3]).T + (P[:, 3] - W[:, 3])
        return float(np.linalg.norm(d, axis=1).max())

    # the whole call, wall clock (it reads the counts back and copies the result back)
    whole = []
    for it in range(args.warmup + args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = registration.register_volumes(moving, fixed, band=band)
        whole.append((time.perf_counter() - t0) * 1e6)
    whole = whole[args.warmup:]
    stages = registration.default_stages(band)
    m_t, m_w, f_t, f_w = moving['tsdf'], moving['weights'], fixed['tsdf'], fixed['weights']

    # the pieces, with device events
    ws_sel = registration._select_workspace(lib, m_t)
    lists, select_us = {}, {}
    for stride in (2, 1):
        n = int(registration._select('register_bench', lib, m_t, m_w, band, stride, ws_sel).cpu()[0])
        lists[stride] = torch.empty(n, dtype=torch.int32, device=dev)

        def select(stride=stride):
            registration._select('register_bench', lib, m_t, m_w, band, stride, ws_sel)
            registration._select('register_bench', lib, m_t, m_w, band, stride, ws_sel, lists[stride])
        select_us[stride] = timed(select, args.iters, args.warmup)
    reach = registration.coarse_reach(stages, band, res)
    field_us = timed(lambda: registration.signed_distance_field(f_t, f_w, res, reach=reach), args.iters, args.warmup)
    field_unlimited_us = timed(lambda: registration.signed_distance_field(f_t, f_w, res), args.iters, args.warmup)
    field = registration.signed_distance_field(f_t, f_w, res, reach=reach)

    c_m, c_f = registration.condition(m_t.shape, moving['origin'], res, np.eye(3), np.zeros(3))
    o_m, o_f = np.ascontiguousarray(moving['origin'] - c_m), np.ascontiguousarray(fixed['origin'] - c_f)
    E0 = np.ascontiguousarray(np.eye(4)[:3].reshape(12))
    rows = _lib.REGISTER_MAX_ITERATIONS
    state = torch.zeros(12 + 4 * rows + 1, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.ojf_register_workspace_bytes(max(l.numel() for l in lists.values()))), dtype=torch.uint8, device=dev)
    fband = float(np.nextafter(np.float32(trunc), np.float32(0)))
    st = _lib.stream_ptr(dev)

    def stage_call(k, iterations, first, cont):
        s = stages[k]
        lst, sdf = lists[s['stride']], s['field'] == 'sdf'
        rc = lib.ojf_register(m_t.data_ptr(), *m_t.shape, o_m.ctypes.data, res, lst.data_ptr(), lst.numel(),
                              None if sdf else f_t.data_ptr(), None if sdf else f_w.data_ptr(), field.data_ptr() if sdf else None,
                              *f_t.shape, o_f.ctypes.data, res, float('inf') if sdf else fband, s['dist'], iterations, first, 0.05,
                              E0.ctypes.data, int(cont), ws.data_ptr(), ws.numel(), state.data_ptr(), state.data_ptr() + 96,
                              state.data_ptr() + 8 * (12 + 4 * rows), st)
        _lib.check(rc, 'ojf_register')

    # every iteration as a call of its own, in the order of the whole call, so that each sees the pose its turn would see
    per_iter = [[] for _ in range(20)]
    stage_us = [[], []]
    for it in range(args.warmup + args.iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
        torch.cuda.synchronize()
        ev[0].record()
        for i in range(20):
            stage_call(i // 10, 1, i, i > 0)
            ev[i + 1].record()
        ev[-1].synchronize()
        if it >= args.warmup:
            for i in range(20):
                per_iter[i].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        stage_call(0, 10, 0, False)
        e[1].record()
        stage_call(1, 10, 10, True)
        e[2].record()
        e[2].synchronize()
        if it >= args.warmup:
            stage_us[0].append(e[0].elapsed_time(e[1]) * 1e3)
            stage_us[1].append(e[1].elapsed_time(e[2]) * 1e3)
    host = state.cpu().numpy()
    P = host[:12].reshape(3, 4).copy()
    P[:, 3] = P[:, 3] + c_f - P[:, :3] @ c_m
    status = host[12 + 4 * rows:].view(np.int32)

    def copy_us(nbytes):
        a = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        return timed(lambda: b.copy_(a), args.iters, args.warmup)

    doc = {'tool': 'tools/register_bench.py', 'device': torch.cuda.get_device_name(0), 'case': 'room_%d' % grid, 'grid': grid,
           'fixed_shape': list(fshape), 'resolution': res, 'truncation': trunc, 'band': band, 'degrees': args.degrees,
           'iters': args.iters, 'warmup': args.warmup,
           'start_error_m': round(error(np.eye(4)[:3]), 4), 'end_error_m': round(error(out['transform']), 6),
           'end_error_staged_calls_m': round(error(P), 6), 'status': int(status[0]), 'n_points': out['n_points'],
           'select_us': {'stride_%d' % k: round(v, 1) for k, v in select_us.items()}, 'signed_field_us': round(field_us, 1),
           'signed_field_reach_m': round(reach, 4), 'signed_field_unlimited_us': round(field_unlimited_us, 1),
           'stages': []}
    for k, s in enumerate(stages):
        n = lists[s['stride']].numel()
        its = [statistics.median(v) for v in per_iter[10 * k:10 * k + 10]]
        floor = copy_us(BYTES_PER_POINT * n // 2)
        doc['stages'].append({'field': s['field'], 'stride': s['stride'], 'points': n, 'blocks': (n + 1023) // 1024,
                              'iteration_us': [round(v, 1) for v in its], 'iteration_us_median': round(statistics.median(its), 1),
                              'stage_call_us': round(statistics.median(stage_us[k]), 1), 'bytes_touched': BYTES_PER_POINT * n,
                              'copy_floor_us': round(floor, 1), 'iteration_over_floor': round(statistics.median(its) / floor, 2)})
    doc['whole_call_wall_us'] = round(statistics.median(whole), 1)
    doc['whole_call_wall_us_min_max'] = [round(min(whole), 1), round(max(whole), 1)]
    print(json.dumps(doc), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
