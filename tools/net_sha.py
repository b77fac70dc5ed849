"""Profiling helper (not a test): sha256 of the HIP fusion net's output at a frame size + its time per forward pass, the per-kernel
profile and the launch-name sequence in host enqueue order
(python tools/net_sha.py [h w [sem]] [--version v3] [--n-points 9] [--growth 5] [--arith f16x3] [--reps 200]; growth as the C ABI
counts it = growth_factor - 1): A/B of two builds (or of a test-only switch) that must not change a bit or a launch."""
import argparse, hashlib, os, sys, time, types, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_joint_depthfusion_and_semantic_amd import model
from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine


def run(h=240, w=320, sem=False, version='v3', n_points=9, growth=5, arith='f16x3', reps=200):
    """-> dict(sha, us, names (launch names of one profiled forward, in order), launches, prof {name: [us]})"""
    dev = torch.device('cuda:0')
    cfg = types.SimpleNamespace(n_points=n_points, growth_factor=growth + 1, use_semantics=sem, output_scale=1.0, resx=w, resy=h)
    torch.manual_seed(0)
    net = getattr(model, 'FusionNet_' + version)(cfg)
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d): torch.nn.init.xavier_normal_(m.weight)
    eng = FusionNetEngine(net.eval(), h, w, dev, arithmetic=arith)
    g = torch.Generator(device=dev); g.manual_seed(1)
    fv = (torch.rand(n_points, h * w, device=dev, generator=g) * 0.2 - 0.1).contiguous()
    fw = torch.rand(n_points, h * w, device=dev, generator=g).contiguous()
    d = (torch.rand(h, w, device=dev, generator=g) * 3).contiguous()
    ids = (torch.rand(h * w, device=dev, generator=g) * 30).to(torch.uint8)
    est = torch.empty(h * w, n_points, device=dev)
    for _ in range(5):
        eng.prepare_input(fv, fw, d, ids if sem else None, 30 if sem else 0, planes=True)
        eng.forward(est)
    eng.check()
    launches = eng.launches
    sha = hashlib.sha256(est.cpu().numpy().tobytes()).hexdigest()[:16]
    t0 = time.perf_counter()
    for _ in range(reps): eng.forward(est)
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / max(reps, 1) * 1e6
    prof, names = {}, None
    for _ in range(5):
        p = eng.profile(est)
        names = [name for name, _ in p]
        for name, t in p:
            prof.setdefault(name, []).append(t)
    eng.close()
    return dict(sha=sha, us=us, names=names, launches=launches, prof=prof)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('size', nargs='*', help='h w [sem]')
    ap.add_argument('--version', default='v3', choices=['v2', 'v3'])
    ap.add_argument('--n-points', type=int, default=9)
    ap.add_argument('--growth', type=int, default=5)
    ap.add_argument('--arith', default='f16x3', choices=['f16x3', 'f32'])
    ap.add_argument('--reps', type=int, default=200)
    a = ap.parse_args()
    h, w = (int(a.size[0]), int(a.size[1])) if len(a.size) > 1 else (240, 320)
    sem = len(a.size) > 2 and a.size[2] == 'sem'
    r = run(h, w, sem, a.version, a.n_points, a.growth, a.arith, a.reps)
    print('%dx%d%s %s P=%d growth=%d %s: est sha %s  %.1f us per forward  %d launches  %s' % (
        h, w, ' sem' if sem else '', a.version, a.n_points, a.growth, a.arith, r['sha'], r['us'], r['launches'],
        ' '.join('%s=%s' % (k, v) for k, v in sorted(os.environ.items()) if k.startswith('OJF_'))))
    n = 5
    print('   ' + ' | '.join('%s %.1f' % (k[:34], sum(v) / n) for k, v in sorted(r['prof'].items(), key=lambda kv: -sum(kv[1]))))
    print('   sequence: ' + '; '.join(r['names']))


if __name__ == '__main__':
    main()
