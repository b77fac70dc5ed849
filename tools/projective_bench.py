"""Time of ojf_fuse_projective (projective.integrate_depth) for DESIGN.md: device events around `--iters` bare ABI calls
after `--warmup`, with the inputs prepared once, per call and per view, for frames of the synthetic room at 320x240 into a
256^3 volume and 640x480 into 512^3, n = 1 and n = 8 views per call, carve off and on.  The calls repeat on the same
volumes (the work of a call does not depend on what the voxels hold).  "updated_fraction": the share of the voxels the
first call of a fresh volume updates.  One JSON line per case; --pipeline adds the frames/s of a Pipeline.fuse loop with
FUSION_MODEL.name 'tsdf' at 320x240 into 256^3 (host work included).

    python tools/projective_bench.py [--iters 50] [--warmup 5] [--quick] [--pipeline]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from online_joint_depthfusion_and_semantic_amd import synthetic  # noqa: E402
from online_joint_depthfusion_and_semantic_amd import _lib  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.projective import integrate_depth  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.views import cameras  # noqa: E402


def raw_call(tsdf, wgt, origin, res, K, E, depth, mask, trunc, carve):
    """ojf_fuse_projective with the cameras and images prepared once: the kernel without integrate_depth's host work."""
    lib = _lib.load()
    n, h, w = depth.shape
    _, Kh, Eh = cameras('projective_bench', K, E, n)
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float64))
    args = (_lib.ptr(tsdf), _lib.ptr(wgt), None, None, *tsdf.shape, org.ctypes.data, float(res), n, Kh.ctypes.data, Eh.ctypes.data,
            _lib.ptr(depth), _lib.ptr(mask), None, None, h, w, float(trunc), 128.0, 0.0, int(carve), _lib.stream_ptr(tsdf.device))

    def fn(keep=(Kh, Eh, org)):
        _lib.check(lib.ojf_fuse_projective(*args), 'ojf_fuse_projective')
    return fn


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


def pipeline_fps(h, w, grid, frames, dev):
    from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config
    from online_joint_depthfusion_and_semantic_amd.database import Database
    from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
    cfg = default_config(h, w, model='tsdf')
    cfg.SETTINGS.device = str(dev)
    st = synthetic.SyntheticStream(h, w, grid, 40)
    db = Database(st, database_config(cfg))
    pipe = Pipeline(cfg).to(dev).eval()
    batches = [{k: (v.to(dev) if torch.is_tensor(v) and k not in ('extrinsics', 'intrinsics') else v) for k, v in st.batch(i).items()}
               for i in range(8)]
    with torch.no_grad():
        for i in range(16):
            pipe.fuse(batches[i % 8], db, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(frames):
            pipe.fuse(batches[i % 8], db, dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return frames / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='the 320x240 / 256^3 cases only')
    ap.add_argument('--pipeline', action='store_true', help='also time a Pipeline.fuse loop in the classical mode')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('projective_bench: no HIP device visible (there is no CPU path to time)')
    dev = torch.device('cuda:0')
    sizes = [(240, 320, 256)] if args.quick else [(240, 320, 256), (480, 640, 512)]
    for h, w, grid in sizes:
        origin, res, _ = synthetic.grid_spec(grid)
        st = synthetic.SyntheticStream(h, w, grid, 40)
        fr = [st.frame(i) for i in range(8)]
        depth = torch.from_numpy(np.stack([f['tof_depth'] for f in fr])).to(dev)
        mask = torch.from_numpy(np.stack([f['mask'] for f in fr]).astype(np.uint8)).to(dev)
        E = np.stack([f['extrinsics'] for f in fr])
        trunc = 0.1
        for n in (1, 8):
            for carve in (False, True):
                tsdf = torch.full((grid,) * 3, trunc, dtype=torch.float16, device=dev)
                wgt = torch.zeros((grid,) * 3, dtype=torch.float16, device=dev)
                fn = raw_call(tsdf, wgt, origin, res, st.K, E[:n], depth[:n].contiguous(), mask[:n].contiguous(), trunc, carve)
                fn()
                updated = float((wgt > 0).float().mean())
                us_raw = time_calls(fn, args.iters, args.warmup)
                kw = dict(origin=origin, resolution=res, depth=depth[:n], intrinsics=st.K, extrinsics=E[:n], mask=mask[:n],
                          truncation=trunc, carve=carve)
                us = time_calls(lambda: integrate_depth(tsdf, wgt, **kw), args.iters, args.warmup)
                print(json.dumps({'case': 'projective', 'grid': grid, 'h': h, 'w': w, 'n': n, 'carve': carve,
                                  'raw_us_per_call': round(us_raw, 2), 'raw_us_per_view': round(us_raw / n, 2),
                                  'us_per_call': round(us, 2), 'us_per_view': round(us / n, 2),
                                  'updated_fraction': round(updated, 5)}), flush=True)
                del tsdf, wgt
        torch.cuda.empty_cache()
    if args.pipeline:
        fps = pipeline_fps(240, 320, 256, 400, dev)
        print(json.dumps({'case': 'pipeline_fuse_tsdf', 'grid': 256, 'h': 240, 'w': 320, 'frames_per_s': round(fps, 1),
                          'ms_per_frame': round(1e3 / fps, 4)}), flush=True)


if __name__ == '__main__':
    main()
