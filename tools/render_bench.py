"""Time of ojf_render (render.render_views) for DESIGN.md: device events around `--iters` calls after `--warmup`, per
call and per view, at 320x240 over a 256^3 volume and 640x480 over 512^3, on the synthetic ground-truth room and on a
volume fused by Pipeline.fuse (with its weights, so unobserved space is transparent), at n = 1 and n = 8 views per call.
"raw" times the bare ojf_render call with the cameras prepared and the outputs allocated once.  Gathers per ray come
from the fp32 restatement (tests/render_ref.py) on a sub-sampled image: 8 fp16 voxels per march sample, 8 fp16 weights
per sample checked at a candidate crossing (an upper bound: the kernel skips the second check when the first fails),
48 voxels for the normal.  One JSON line per case.

    python tools/render_bench.py [--iters 50] [--warmup 5] [--quick] [--no-counts]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from online_joint_depthfusion_and_semantic_amd import synthetic  # noqa: E402
from online_joint_depthfusion_and_semantic_amd import _lib  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.render import render_views  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.views import inverse_cameras  # noqa: E402


def raw_call(tsdf, wgt, ids, origin, res, K, E, h, w):
    """ojf_render with the cameras prepared and the outputs allocated once: the kernel without render_views' host work."""
    lib = _lib.load()
    n, Ki, Ew = inverse_cameras('render_bench', K, E)
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float64))
    depth = torch.empty((n, h, w), dtype=torch.float32, device=tsdf.device)
    nrm = torch.empty((n, h, w, 3), dtype=torch.float32, device=tsdf.device)
    lab = torch.empty((n, h, w), dtype=torch.uint8, device=tsdf.device)
    args = (_lib.ptr(tsdf), _lib.ptr(wgt), _lib.ptr(ids), *tsdf.shape, org.ctypes.data, float(res), n, Ki.ctypes.data,
            Ew.ctypes.data, h, w, 0.0, _lib.ptr(depth), _lib.ptr(nrm), _lib.ptr(lab), _lib.stream_ptr(tsdf.device))

    def fn():
        _lib.check(lib.ojf_render(*args), 'ojf_render')
    return fn


def fused_volume(h, w, grid, frames, dev):
    from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
    from online_joint_depthfusion_and_semantic_amd.database import Database
    from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
    cfg = default_config(h, w, semantics=True, use_semantics=True)
    cfg.SETTINGS.device = str(dev)
    st = synthetic.SyntheticStream(h, w, grid, frames)
    db = Database(st, database_config(cfg))
    torch.manual_seed(3)
    pipe = Pipeline(cfg)
    for m in pipe._fusion_network.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.xavier_normal_(m.weight)
    pipe = pipe.to(dev).eval()
    with torch.no_grad():
        for i in range(frames):
            pipe.fuse({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in st.batch(i).items()}, db, dev)
    torch.cuda.synchronize()
    s = st.scene
    return db.scenes_est[s].volume, db.fusion_weights[s], db.ids_est[s].volume


def time_calls(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def gathers(tsdf, wgt, ids, origin, res, K, E, h, w, stride=8):
    """Restatement's counts on every stride-th pixel of every stride-th row of view 0."""
    from render_ref import render_ref
    Ks = K.copy()
    Ks[0, 0] /= stride
    Ks[1, 1] /= stride
    Ks[0, 2] /= stride
    Ks[1, 2] /= stride
    c = {}
    render_ref(tsdf.cpu().numpy(), None if wgt is None else wgt.cpu().numpy(), ids.cpu().numpy(), origin, res, Ks, E[0],
               (h // stride, w // stride), counts=c)
    rays = max(c['rays'], 1)
    per_ray = (8 * c['samples'] + 8 * c['valid_checks'] + 48 * c['hits']) / rays
    return {'samples_per_ray': c['samples'] / rays, 'max_samples': c['max_samples'], 'ref_hit_fraction': c['hits'] / rays,
            'voxel_gathers_per_ray': per_ray, 'gathered_bytes_per_ray': 2 * per_ray + (c['hits'] / rays) * 1,
            'written_bytes_per_ray': 4 + 12 + 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='the 320x240 / 256^3 cases only')
    ap.add_argument('--no-counts', action='store_true', help='skip the CPU restatement counts')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('render_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    sizes = [(240, 320, 256)] if args.quick else [(240, 320, 256), (480, 640, 512)]
    for h, w, grid in sizes:
        origin, res, _ = synthetic.grid_spec(grid)
        K = synthetic.intrinsics(h, w)
        E8 = np.stack([synthetic.camera_pose(t) for t in np.linspace(0.2, 6.0, 8)])
        t, ids = synthetic.gt_volumes(grid)
        volumes = {'gt': (torch.from_numpy(t).to(dev), None, torch.from_numpy(ids).to(dev))}
        del t, ids
        volumes['fused'] = fused_volume(h, w, grid, 10, dev)
        for name, (tsdf, wgt, ids) in volumes.items():
            counts = None if args.no_counts else gathers(tsdf, wgt, ids, origin, res, K, E8, h, w)
            for n in (1, 8):
                kw = dict(origin=origin, resolution=res, intrinsics=K, extrinsics=E8[:n], shape=(h, w))
                us = time_calls(lambda: render_views(tsdf, wgt, ids, **kw), args.iters, args.warmup)
                us_raw = time_calls(raw_call(tsdf, wgt, ids, origin, res, K, E8[:n], h, w), args.iters, args.warmup)
                hit = float((render_views(tsdf, wgt, ids, **kw)['depth'] > 0).float().mean())
                rec = {'case': 'render', 'volume': name, 'grid': grid, 'h': h, 'w': w, 'n': n, 'weights': wgt is not None,
                       'us_per_call': round(us, 2), 'us_per_view': round(us / n, 2), 'raw_us_per_call': round(us_raw, 2),
                       'raw_us_per_view': round(us_raw / n, 2), 'hit_fraction': round(hit, 5)}
                if counts:
                    rec.update({k: (round(v, 2) if isinstance(v, float) else v) for k, v in counts.items()})
                print(json.dumps(rec), flush=True)
        del volumes
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
