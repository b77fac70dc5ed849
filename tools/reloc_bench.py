"""Time of the relocalisation kernels (relocalize.py, csrc/ojf_reloc.hip) for DESIGN.md 26.  Two steps, each in a child process
of its own under a time limit (a step that fails or runs out of time ends the run; what was measured until then is kept):

  time        device events around `--iters` bare ABI calls after `--warmup`, at 320x240 with 512 ferns: ojf_reloc_encode for 1
              and 8 frames per call, with and without an image; ojf_reloc_query (k = 4) against stores of 256, 4 096 and 65 536
              keyframes, all of them filled; one ojf_reloc_insert into a store of 4 096 that holds 2 048 - each beside a device
              copy (torch copy_) that reads and writes as many bytes as the call touches; `--repeats` batches, the median with
              the smallest and the largest.
  relocalize  host clock around relocalize.relocalize_frame (k = 4, which ends in a copy back) of three held-out frames of
              the synthetic orbit against the 256^3 ground-truth room with keyframes 0, 4, ..., 76, beside one
              tracking.track_frame from the true neighbouring pose; the pose errors of the results.

Retrieval on real data is not measured: only the synthetic room is at hand (tests/test_reloc_host.py has its figures).
One JSON line per result; `--out FILE` also writes them as one JSON document (profiles/reloc_bench.json).

    python tools/reloc_bench.py [--iters 300] [--warmup 10] [--repeats 7] [--out profiles/reloc_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from online_joint_depthfusion_and_semantic_amd import _lib, synthetic  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.relocalize import Relocalizer, relocalize_frame  # noqa: E402
from online_joint_depthfusion_and_semantic_amd.tracking import track_frame  # noqa: E402

STEP_LIMITS = {'time': 240, 'relocalize': 240}  # seconds
H, W, M = 240, 320, 512


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


def report(args, dev, case, call, touched, **extra):
    src = torch.empty(max(touched // 2, 1), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    med, lo, hi = timed(call, args.iters, args.warmup, args.repeats)
    cmed, clo, chi = timed(lambda: dst.copy_(src), args.iters, args.warmup, args.repeats)
    emit(dict({'case': case, 'device': torch.cuda.get_device_name(0), 'h': H, 'w': W, 'n_ferns': M, 'iters': args.iters,
               'repeats': args.repeats}, **extra, us_per_call=round(med, 2), us_per_call_min_max=[round(lo, 2), round(hi, 2)],
              bytes_touched=touched, copy_us_per_call=round(cmed, 2), copy_us_per_call_min_max=[round(clo, 2), round(chi, 2)],
              over_copy=round(med / cmed, 3)))


def step_time(args, dev):
    lib = _lib.load()
    stream = _lib.stream_ptr(dev)
    st = synthetic.SyntheticStream(H, W, 64, 400)
    fr = [st.frame(i) for i in range(8)]
    rng = np.random.default_rng(1)
    for color in (False, True):
        r = Relocalizer(H, W, device=dev, n_ferns=M, color=color)
        t = r._table_dev
        for n in (1, 8):
            depth = torch.from_numpy(np.stack([f['tof_depth'] for f in fr[:n]])).to(dev)
            mask = torch.from_numpy(np.stack([f['mask'] for f in fr[:n]]).astype(np.uint8)).to(dev)
            image = torch.from_numpy(rng.integers(0, 256, (n, H, W, 4), dtype=np.uint8)).to(dev) if color else None
            codes = torch.empty((n, r.words), dtype=torch.int32, device=dev)
            enc = (_lib.ptr(depth), _lib.ptr(mask), _lib.ptr(image), n, H, W, r.cell, M, _lib.ptr(t['cell']), _lib.ptr(t['channel']),
                   _lib.ptr(t['threshold']), _lib.ptr(codes), None, stream)

            def call(enc=enc, keep=(depth, mask, image, codes)):
                _lib.check(lib.ojf_reloc_encode(*enc), 'ojf_reloc_encode')
            touched = n * H * W * (4 + 1 + (4 if color else 0)) + M * 4 * 9 + n * r.words * 4  # frames in, the table, codes out
            report(args, dev, 'encode', call, touched, n=n, image=color, cell=r.cell, us_per_frame_note='us_per_call / n')
    # query and insert: stores filled with random codes
    query = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (1, M // 8), dtype=np.int64).astype(np.int32)).to(dev)
    pose = torch.zeros((1, 12), dtype=torch.float64, device=dev)
    for capacity in (256, 4096, 65536):
        db = torch.randint(-2 ** 31, 2 ** 31 - 1, (capacity, M // 8), dtype=torch.int64, device=dev).to(torch.int32)
        count = torch.tensor([capacity], dtype=torch.int32, device=dev)
        keys = torch.empty((1, 4), dtype=torch.int64, device=dev)
        q = (_lib.ptr(query), 1, M, _lib.ptr(db), _lib.ptr(count), capacity, 4, _lib.ptr(keys), stream)

        def call(q=q, keep=(db, count, keys)):
            _lib.check(lib.ojf_reloc_query(*q), 'ojf_reloc_query')
        report(args, dev, 'query', call, capacity * (M // 8) * 4 + (M // 8) * 4 + 32, keyframes=capacity, k=4)
    capacity, held = 4096, 2048
    db = torch.randint(-2 ** 31, 2 ** 31 - 1, (capacity, M // 8), dtype=torch.int64, device=dev).to(torch.int32)
    poses = torch.zeros((capacity, 12), dtype=torch.float64, device=dev)
    count = torch.tensor([held], dtype=torch.int32, device=dev)
    best = torch.empty(1, dtype=torch.int64, device=dev)
    added = torch.empty(1, dtype=torch.int32, device=dev)
    ins = (_lib.ptr(query), _lib.ptr(pose), 1, M, M, 0, _lib.ptr(db), _lib.ptr(poses), _lib.ptr(count), capacity, _lib.ptr(best),
           _lib.ptr(added), stream)  # (min_differ = M: the frame is searched for and never added, so the store stays at `held`)

    def call():
        _lib.check(lib.ojf_reloc_insert(*ins), 'ojf_reloc_insert')
    report(args, dev, 'insert', call, held * (M // 8) * 4 + (M // 8) * 4 + 12, keyframes=held, capacity=capacity)
    assert int(count.item()) == held


def _pose_error(E, T):
    c = (np.trace(E[:3, :3].T @ T[:3, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(E[:3, 3] - T[:3, 3])), float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def step_relocalize(args, dev):
    grid = 256
    tsdf = torch.from_numpy(synthetic.gt_volumes(grid, 0.1)[0]).to(dev)
    origin, res, _ = synthetic.grid_spec(grid)
    st = synthetic.SyntheticStream(H, W, grid, 400)
    r = Relocalizer(H, W, device=dev, n_ferns=M)
    key_frames = list(range(0, 80, 4))
    fr = [st.frame(i) for i in key_frames]
    r.add(torch.from_numpy(np.stack([f['tof_depth'] for f in fr])).to(dev), np.stack([f['extrinsics'] for f in fr]),
          mask=torch.from_numpy(np.stack([f['mask'] for f in fr])).to(dev), force=True)
    for q in (30, 45, 62):
        f = st.frame(q)
        d, m = torch.from_numpy(f['tof_depth']).to(dev), torch.from_numpy(f['mask']).to(dev)
        kw = dict(origin=origin, resolution=res, depth=d, intrinsics=st.K, mask=m)

        def host_ms(fn, reps=20):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                out = fn()
            return 1e3 * (time.perf_counter() - t0) / reps, out  # (every call ends in a copy back: the device is idle here)
        ms4, out4 = host_ms(lambda: relocalize_frame(tsdf, None, r, k=4, **kw))
        ms1, out1 = host_ms(lambda: relocalize_frame(tsdf, None, r, k=1, **kw))
        E_prev = st.frame(q - 1)['extrinsics']
        mst, outt = host_ms(lambda: track_frame(tsdf, None, extrinsics=E_prev, **kw))
        msq, near = host_ms(lambda: r.query(d, mask=m, k=4))
        e4, e1, et = (_pose_error(o['extrinsics'], f['extrinsics']) for o in (out4, out1, outt))
        emit({'case': 'relocalize', 'device': torch.cuda.get_device_name(0), 'h': H, 'w': W, 'grid': grid, 'frame': q, 'keyframes': len(key_frames),
              'candidates': [key_frames[c['index']] for c in out4['candidates']],
              'dissimilarity': [round(c['dissimilarity'], 4) for c in out4['candidates']], 'chosen': key_frames[out4['candidate']],
              'ok': bool(out4['ok']), 'relocalize_k4_ms': round(ms4, 3), 'relocalize_k1_ms': round(ms1, 3), 'query_ms': round(msq, 3),
              'track_frame_ms': round(mst, 3), 'error_k4_mm_deg': [round(1e3 * e4[0], 3), round(e4[1], 4)],
              'error_k1_mm_deg': [round(1e3 * e1[0], 3), round(e1[1], 4)], 'error_track_mm_deg': [round(1e3 * et[0], 3), round(et[1], 4)]})
    emit({'case': 'retrieval on real data', 'status': 'not measured', 'why': 'only the synthetic room is available'})


STEPS = {'time': step_time, 'relocalize': step_relocalize}


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
            raise SystemExit('reloc_bench: no HIP device visible (there is no CPU path to time)')
        STEPS[args.step](args, torch.device('cuda:0'))
        return
    cases, failed = [], None
    for name in ('time', 'relocalize'):
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
        doc = {'tool': 'tools/reloc_bench.py', 'cases': cases}
        if failed:
            doc['failed'] = failed
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')
    if failed:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
