"""Time and effect of ojf_depth_prepare (frames.py) for DESIGN.md 24.  Four steps, each in a child process of its own under
a time limit (a step that fails or runs out of time ends the run; what was measured until then is kept):

  time        device events around `--iters` bare ABI calls after `--warmup`, at 320x240 and 640x480, n = 1 and n = 8 frames
              per call, with the stages off (validity + copy), the filter alone, edge test + filter, and everything on - each
              beside a device copy (torch copy_) that reads and writes as many bytes as the call touches; `--repeats` batches,
              the median with the smallest and the largest.
  quality     frames 0, 7, 13 of the noisy synthetic room (2 cm depth noise) at 48x64 and 240x320: mean absolute depth error
              against depth_gt over the kept pixels, raw and filtered, the share of valid pixels kept, and the mean angle of
              the normals against those of the clean frame, raw and filtered.
  track       Database.track of frames 1..9 against a model fused from frames 0..9, each started at the previous frame's true
              pose, with and without `filter`: mean translation (m) and rotation (degrees) error.
  components  the voxels Database.filter_components removes after 20 fused frames, with and without edge rejection.

One JSON line per result; `--out FILE` also writes them as one JSON document (profiles/frames_bench.json).

    python tools/frames_bench.py [--iters 300] [--warmup 10] [--repeats 7] [--out profiles/frames_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from online_joint_depthfusion_and_semantic_amd import _lib, frames, synthetic  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.config import default_config, database_config  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.database import Database  # noqa: E402

STEP_LIMITS = {'time': 240, 'quality': 120, 'track': 180, 'components': 180}  # seconds
FILTER = dict(radius=2, sigma_space=1.5, range0=0.06, edge_abs=0.12)
VARIANTS = {  # name -> (prepare_depth options, normals)
    'stages off': (dict(radius=0, range0=0.06), False),
    'filter r2': (dict(radius=2, sigma_space=1.5, range0=0.06), False),
    'edge + filter r2': (dict(FILTER), False),
    'all on r2': (dict(FILTER, max_angle=75.0), True),
    'all on r4': (dict(FILTER, radius=4, sigma_space=2.5, max_angle=75.0), True),
}


def emit(row):
    print(json.dumps(row, default=float), flush=True)  # (numpy scalars)


def timed(fn, iters, warmup, repeats):
    """(median, min, max) us per call over `repeats` batches of `iters` calls."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def step_time(args, dev):
    lib = _lib.load()
    for h, w in ((240, 320), (480, 640)):
        st = synthetic.SyntheticStream(h, w, 64, 40, noise_sigma=0.02)
        fr = [st.frame(i) for i in range(8)]
        for n in (1, 8):
            depth = torch.from_numpy(np.stack([f['tof_depth'] for f in fr[:n]])).to(dev)
            mask = torch.from_numpy(np.stack([f['mask'] for f in fr[:n]]).astype(np.uint8)).to(dev)
            out, valid = torch.empty_like(depth), torch.empty_like(mask)
            nrm = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
            K = frames.frame_intrinsics(np.repeat(st.K.reshape(1, 9), n, axis=0))
            for name, (opts, normals) in VARIANTS.items():
                o = frames.options(**opts)
                call_args = (_lib.ptr(depth), _lib.ptr(mask), n, h, w, K.ctypes.data, o['radius'], _lib.ptr(o['spatial']), o['range0'],
                             o['range2'], o['edge_abs'], o['edge_rel'], o['near'], o['far'], o['cos_min'], _lib.ptr(out), _lib.ptr(valid),
                             _lib.ptr(nrm) if normals else None, _lib.stream_ptr(dev))

                def call(keep=(K, o)):
                    _lib.check(lib.ojf_depth_prepare(*call_args), 'ojf_depth_prepare')
                touched = n * h * w * (4 + 1 + 4 + 1 + (12 if normals else 0))  # depth, mask in; depth, valid(, normals) out
                src = torch.empty(touched // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                med, lo, hi = timed(call, args.iters, args.warmup, args.repeats)
                cmed, clo, chi = timed(lambda: dst.copy_(src), args.iters, args.warmup, args.repeats)
                emit({'case': 'time', 'device': torch.cuda.get_device_name(0), 'h': h, 'w': w, 'n': n, 'variant': name, 'iters': args.iters, 'repeats': args.repeats,
                      'us_per_call': round(med, 2), 'us_per_call_min_max': [round(lo, 2), round(hi, 2)], 'us_per_frame': round(med / n, 2),
                      'bytes_touched': touched, 'copy_us_per_call': round(cmed, 2), 'copy_us_per_call_min_max': [round(clo, 2), round(chi, 2)],
                      'over_copy': round(med / cmed, 3)})


def _angles(a, b):
    return np.degrees(np.arccos(np.clip((a.astype(np.float64) * b.astype(np.float64)).sum(-1), -1.0, 1.0)))


def step_quality(args, dev):
    for h, w in ((48, 64), (240, 320)):
        st = synthetic.SyntheticStream(h, w, 64, 40, noise_sigma=0.02)
        raw = fil = kept = valid = ang_raw = ang_fil = cnt = 0.0
        for i in (0, 7, 13):
            f = st.frame(i)
            d, gt, m = (torch.from_numpy(f[k]).to(dev) for k in ('tof_depth', 'depth_gt', 'mask'))
            o = frames.prepare_depth(d, intrinsics=st.K, mask=m, normals=True, **FILTER)
            plain = frames.prepare_depth(d, intrinsics=st.K, mask=m, normals=True, radius=0, range0=0.06)
            clean = frames.prepare_depth(gt, intrinsics=st.K, normals=True, radius=0, range0=0.06)
            k = o['valid'][0].cpu().numpy()
            raw += np.abs(f['tof_depth'][k] - f['depth_gt'][k]).sum()
            fil += np.abs(o['depth'][0].cpu().numpy()[k] - f['depth_gt'][k]).sum()
            kept += k.sum()
            valid += f['mask'].sum()
            no, np_, nc = (x['normals'][0].cpu().numpy() for x in (o, plain, clean))
            both = k & (np.abs(no).sum(-1) > 0) & (np.abs(np_).sum(-1) > 0) & (np.abs(nc).sum(-1) > 0)
            ang_raw += _angles(np_[both], nc[both]).sum()
            ang_fil += _angles(no[both], nc[both]).sum()
            cnt += both.sum()
        emit({'case': 'quality', 'h': h, 'w': w, 'frames': [0, 7, 13], 'noise_sigma': 0.02, 'options': FILTER,
              'depth_error_raw_m': round(raw / kept, 5), 'depth_error_filtered_m': round(fil / kept, 5), 'ratio': round(float(fil / raw), 4),
              'kept_fraction': round(kept / valid, 4), 'normal_error_raw_deg': round(ang_raw / cnt, 2),
              'normal_error_filtered_deg': round(ang_fil / cnt, 2)})


def _scene(dev, h, w, grid, frames_):
    cfg = default_config(h, w, model='tsdf')
    cfg.SETTINGS.device = str(dev)
    ds = synthetic.SyntheticDataset(h, w, grid, frames_)
    st = synthetic.SyntheticStream(h, w, grid, frames_, noise_sigma=0.02)
    return st, Database(ds, database_config(cfg))


def step_track(args, dev):
    h, w, grid = 120, 160, 128
    for name, filt in (('raw', None), ('filtered', dict(FILTER))):
        st, db = _scene(dev, h, w, grid, 160)  # (160 frames per orbit: 2.25 degrees and about 4 cm from one frame to the next)
        fr = [st.frame(i) for i in range(10)]
        for f in fr:
            db.integrate_depth(st.scene, f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'], filter=filt)
        dt, dr, ok = [], [], 0
        for i in range(1, 10):
            f = fr[i]
            out = db.track(st.scene, f['tof_depth'], f['intrinsics'], fr[i - 1]['extrinsics'], mask=f['mask'], filter=filt)
            ok += bool(out['ok'])
            E, T = out['extrinsics'], f['extrinsics']
            dt.append(float(np.linalg.norm(E[:3, 3] - T[:3, 3])))
            c = (np.trace(E[:3, :3].T @ T[:3, :3]) - 1.0) / 2.0
            dr.append(float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))))
        step = float(np.mean([np.linalg.norm(fr[i]['extrinsics'][:3, 3] - fr[i - 1]['extrinsics'][:3, 3]) for i in range(1, 10)]))
        emit({'case': 'track', 'frames': name, 'h': h, 'w': w, 'grid': grid, 'tracked': 9, 'ok': ok, 'mean_start_offset_m': round(step, 4),
              'translation_error_m': round(float(np.mean(dt)), 5), 'rotation_error_deg': round(float(np.mean(dr)), 4)})


def step_components(args, dev):
    h, w, grid = 120, 160, 128
    for name, filt in (('raw', None), ('edge rejection', dict(radius=0, range0=0.06, edge_abs=0.12))):
        st, db = _scene(dev, h, w, grid, 40)
        for i in range(20):
            f = st.frame(i)
            db.integrate_depth(st.scene, f['tof_depth'], f['intrinsics'], f['extrinsics'], mask=f['mask'], filter=filt)
        before = int((db.fusion_weights[st.scene] > 0).sum())
        db.filter_components(keep_largest=1)
        after = int((db.fusion_weights[st.scene] > 0).sum())
        emit({'case': 'components', 'frames': name, 'h': h, 'w': w, 'grid': grid, 'fused_frames': 20, 'observed_voxels': before,
              'removed_voxels': before - after})


STEPS = {'time': step_time, 'quality': step_quality, 'track': step_track, 'components': step_components}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--step', choices=sorted(STEPS), default=None, help='run this step in this process (what the parent starts)')
    args = ap.parse_args()
    if args.step:
        if not torch.cuda.is_available():
            raise SystemExit('frames_bench: no HIP device visible (there is no CPU path to time)')
        STEPS[args.step](args, torch.device('cuda:0'))
        return
    cases, failed = [], None
    for name in ('time', 'quality', 'track', 'components'):
        cmd = [sys.executable, os.path.abspath(__file__), '--step', name, '--iters', str(args.iters), '--warmup', str(args.warmup),
               '--repeats', str(args.repeats)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=STEP_LIMITS[name])
            rc = p.returncode
            lines = p.stdout.decode().splitlines()
        except subprocess.TimeoutExpired as e:
            rc, lines = 124, (e.stdout or b'').decode().splitlines()
        for line in lines:
            if line.startswith('{'):
                print(line, flush=True)
                cases.append(json.loads(line))
        if rc != 0:  # nothing more is started on the device after a step that failed or hung
            failed = {'step': name, 'exit_status': rc}
            print(json.dumps({'case': 'failed', **failed}), flush=True)
            break
    if args.out and cases:
        doc = {'tool': 'tools/frames_bench.py', 'cases': cases}
        if failed:
            doc['failed'] = failed
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')
    if failed:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
