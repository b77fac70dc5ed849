"""SegEngine (adapnet_engine.py: AdapNet++ inference on the SEGCONV HIP kernels) against the torch module tree it
was built from (adapnet.py, itself pinned block by block on the reference in tests/test_adapnet.py).

The default initialisation makes a 50-layer ReLU network forget its input (activations shrink layer by layer and
the output is set by the last biases), which would make an end-to-end comparison vacuous - so the nets here are
re-initialised to keep the signal alive, and the test checks that the output really depends on the input.
Tolerance: split-fp16 products + another summation order, ~80 layers deep: max|err| <= 5e-4 * max|logit|."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def lively(net, seed=0, dropout=False):
    from online_joint_depthfusion_and_semantic_amd import adapnet
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / m.weight[0].numel()))
            elif isinstance(m, nn.ConvTranspose2d):
                fan = m.weight.shape[0] * (m.kernel_size[0] / m.stride[0]) ** 2
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / fan))
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.5 + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
        for m in net.modules():
            if isinstance(m, (adapnet.Bottleneck, adapnet.BottleneckSSMA)):
                m.bn3.weight.mul_(0.4)  # keeps the residual stream from growing 16 units deep
            if isinstance(m, adapnet.BottleneckSSMA):
                m.dropout = dropout
    return net


def build(stage, n_classes, seed=0, dropout=False):
    from online_joint_depthfusion_and_semantic_amd.adapnet import AdapNet
    from online_joint_depthfusion_and_semantic_amd.config import AttrDict
    torch.manual_seed(seed)
    return lively(AdapNet(AttrDict({'stage': stage, 'n_classes': n_classes})), seed, dropout).cuda().eval()


@pytest.mark.parametrize('stage,n_classes,h,w', [(2, 30, 64, 96), (1, 12, 48, 64), (2, 40, 240, 320), (2, 40, 480, 640), (1, 5, 16, 16)])
def test_engine_matches_module(stage, n_classes, h, w):
    from online_joint_depthfusion_and_semantic_amd import _lib
    from online_joint_depthfusion_and_semantic_amd.adapnet_engine import SegEngine
    net = build(stage, n_classes)
    g = torch.Generator().manual_seed(5)
    img = torch.randn((1, 3, h, w), generator=g).cuda()
    dep = (torch.rand((1, 3, h, w), generator=g) * 3).cuda()
    args = (img, dep) if stage != 1 else (img,)
    with torch.no_grad():
        want = net(*args)[0]
        other = net(*[torch.flip(a, dims=(3,)) for a in args])[0]
        eng = SegEngine(net)
        got = eng(*args)
    top = want.abs().max().item()
    assert tuple(got.shape) == tuple(want.shape) == (1, n_classes, h, w)
    assert (want - torch.flip(other, dims=(3,))).abs().max().item() > 0.05 * top  # the output depends on the input
    assert 1e-2 < top < 1e4
    err = (got - want).abs().max().item()
    assert err <= 5e-4 * top, (err, top)
    assert (got.argmax(1) == want.argmax(1)).float().mean().item() > 0.999
    assert _lib.load().ojf_net_check(_lib.stream_ptr(img.device)) == 0


def test_dropout_quirk_is_kept():
    """adapnet.py:80-82: units built with drop_out=True drop activations at inference too."""
    from online_joint_depthfusion_and_semantic_amd.adapnet_engine import SegEngine
    net = build(2, 12)
    for m in net.modules():
        if hasattr(m, 'dropout') and isinstance(m.dropout, bool):
            m.dropout = True
    net.no_resn50_dropout()
    img, dep = torch.randn(1, 3, 32, 48).cuda(), torch.rand(1, 3, 32, 48).cuda()
    with torch.no_grad():
        eng = SegEngine(net)
        a, b = eng(img, dep), eng(img, dep)
        assert (a - b).abs().max().item() > 1e-3 * a.abs().max().item()  # two draws of the masks
        for m in net.modules():
            if hasattr(m, 'dropout') and isinstance(m.dropout, bool):
                m.dropout = False  # the flags are read at call time, like the module does
        a, b = eng(img, dep), eng(img, dep)
        assert torch.equal(a, b)  # every kernel of the engine sums in a fixed order


def test_pipeline_uses_the_engine_and_follows_weight_updates(cuda):
    from online_joint_depthfusion_and_semantic_amd.config import default_config
    from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline
    h, w = 64, 96
    cfg = default_config(h, w, semantics=True, use_semantics=True, n_classes=12)
    cfg.SETTINGS.device = str(cuda)
    cfg.DATA.semantic_strategy = 'predict'
    torch.manual_seed(0)
    pipe = Pipeline(cfg).to(cuda).eval()
    pipe.device = torch.device(cuda)
    lively(pipe._semantic_2d_network, 3)
    batch = {'image': torch.randn(1, 3, h, w, device=cuda) * 50 + 120, cfg.DATA.input: torch.rand(1, 1, h, w, device=cuda) * 3}
    with torch.no_grad():
        hip = pipe._labels2d.segmentation(batch, cuda)
        assert pipe._labels2d.seg_cache['engine'] is not None
        first = pipe._labels2d.seg_cache['engine']
        cfg.SEMANTIC_2D_MODEL.engine = 'torch'
        ref = pipe._labels2d.segmentation(batch, cuda)
        assert (hip - ref).abs().max().item() < 2e-4 and (hip.argmax(-1) == ref.argmax(-1)).float().mean().item() > 0.999
        cfg.SEMANTIC_2D_MODEL.engine = 'hip'
        for p in pipe._semantic_2d_network.decoder.parameters():
            p.mul_(1.5)  # in-place update: version counters move, the engine is rebuilt
        ref2 = pipe._labels2d.segmentation(dict(batch), cuda)
        cfg.SEMANTIC_2D_MODEL.engine = 'torch'
        want2 = pipe._labels2d.segmentation(batch, cuda)
        cfg.SEMANTIC_2D_MODEL.engine = 'hip'
        assert pipe._labels2d.seg_cache['engine'] is not first
        assert (ref2 - want2).abs().max().item() < 2e-4 and (ref2 - hip).abs().max().item() > 1e-3
        # graph replay of the engine == eager engine, before and after another update
        for _ in range(2):
            s, i = pipe._labels2d.segmentation_graph(batch, cuda)
            assert pipe._labels2d.seg_graph['graph'] is not None
            es, ei = pipe._labels2d.segment_max(batch, cuda)  # the eager chain of the same libojf launches (SegEngine.predict)
            assert torch.equal(s, es) and torch.equal(i, ei)  # same kernels, fixed summation order
            # torch's image / 255 (a multiplication by 1/255 on the GPU, a true division here and on the reference's CPU
            # path), softmax and max around the same engine: one input ulp through 50 layers of a lively net
            ts, ti = pipe._labels2d.segmentation(batch, cuda).max(dim=-1)
            assert torch.allclose(s, ts, rtol=0, atol=2e-3) and float((i.long() == ti).float().mean()) > 0.995
            for p in pipe._semantic_2d_network.decoder.parameters():
                p.mul_(0.9)
    with pytest.raises(Exception):  # training mode never routes through the inference engine silently
        pipe._semantic_2d_network.train()
        assert pipe._labels2d.seg_engine((1, 3, h, w), cuda) is None
        raise RuntimeError('ok')


@pytest.mark.parametrize('stage', [2, 1])
def test_engine_matches_reference_whole_network_golden(stage):
    """SegEngine against the REFERENCE's whole-network output (tests/golden/adapnet_net.npz, generated by importing
    modules/adapnet.py): main head within 5e-4 of the logit range, same arg-max."""
    from adapnet_golden_util import golden_net
    from online_joint_depthfusion_and_semantic_amd.adapnet_engine import SegEngine
    net, ins, outs = golden_net(stage)
    net = net.cuda()
    with torch.no_grad():
        got = SegEngine(net)(*[x.cuda() for x in ins]).cpu()
    want = outs[0]
    err, top = float((got - want).abs().max()), float(want.abs().max())
    assert err <= 5e-4 * top, (err, top)
    assert float((got.argmax(1) == want.argmax(1)).float().mean()) > 0.995


def test_predict_many_equals_predict_per_frame():
    """SegEngine.predict_many: B frames as one [B, H, W, C] pass == B single-frame passes (scores to 1e-6: a layer's kernel
    form - and with it the order its K blocks are added - may differ with the number of pixel tiles; arg-max identical apart
    from exact near-ties)."""
    from online_joint_depthfusion_and_semantic_amd.adapnet_engine import SegEngine
    net = build(2, 30)
    net.no_resn50_dropout()
    for m in net.modules():
        if hasattr(m, 'dropout') and isinstance(m.dropout, bool):
            m.dropout = False
    g = torch.Generator().manual_seed(9)
    B, h, w = 3, 64, 96
    images = [(torch.rand((1, 3, h, w), generator=g) * 255).cuda() for _ in range(B)]
    depths = [(torch.rand((1, h, w), generator=g) * 3).cuda() for _ in range(B)]
    with torch.no_grad():
        eng = SegEngine(net)
        scores, ids = eng.predict_many(images, depths)
        for b in range(B):
            s1, i1 = eng.predict(images[b], depths[b])
            assert (scores[b] - s1).abs().max().item() <= 1e-6
            assert (ids[b] == i1).float().mean().item() >= 0.9995
    assert scores.shape == (B, h * w) and ids.dtype == torch.uint8


# ---- the always-on dropout against the module with the restatement's masks (tests/dropout_ref.py) ------------------------
def unit_pairs(net, eng):
    """(module, engine unit) of every residual unit of every encoder."""
    encs = [(net.encoder_mod1, eng.enc1)] + ([(net.encoder_mod2, eng.enc2)] if eng.fusion else [])
    pairs = []
    for mod, enc in encs:
        r = mod.res_n50_enc
        for li, layer in enumerate((r.layer1, r.layer2, r.layer3, r.layer4)):
            assert len(layer) == len(enc.layers[li])
            pairs += [(m, enc.layers[li][ui]) for ui, m in enumerate(layer)]
    return pairs


def module_with_masks(net, eng, args, seed, frame):
    """net(*args)[0] with every dropping unit's F.dropout replaced by the restatement's masks for (seed, frame, the engine
    unit's stream id): output x 2 x mask."""
    from dropout_ref import keep_mask_nchw
    hooks, units = [], []
    for m, u in unit_pairs(net, eng):
        if getattr(m, 'dropout', False) is True:
            units.append(m)
            m.dropout = False

            def hook(module, inputs, out, sid=u.drop_id):
                keep = keep_mask_nchw(seed, frame, sid, *out.shape)
                return out * torch.from_numpy(2.0 * keep).to(out.device, out.dtype)
            hooks.append(m.register_forward_hook(hook))
    try:
        with torch.no_grad():
            return net(*args)[0]
    finally:
        for h in hooks:
            h.remove()
        for m in units:
            m.dropout = True


def lively_inputs(stage, h, w, batch=1, seed=5):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn((batch, 3, h, w), generator=g).cuda()
    dep = (torch.rand((batch, 3, h, w), generator=g) * 3).cuda()
    return (img, dep) if stage != 1 else (img,)


@pytest.mark.parametrize('stage,n_classes,h,w,state', [(2, 30, 64, 96, (0x0123456789abcdef, (3 << 32) | 0xfffffffe)),
                                                       (2, 40, 240, 320, (-0x1234567890abcdef, (1 << 32) | 7)),
                                                       (1, 12, 48, 64, (0x7edcba9876543210, 0xffffffff))])
def test_engine_dropout_matches_module_with_restated_masks(stage, n_classes, h, w, state):
    """SegEngine with every multi-scale unit dropping == the module forward with each unit's dropout replaced by the
    restatement's masks for the engine's (seed, frame, stream id); one counter step per pass.  The masks of the next frame
    miss by far more than the bar."""
    from online_joint_depthfusion_and_semantic_amd.adapnet_engine import SegEngine
    net = build(stage, n_classes, dropout=True)
    args = lively_inputs(stage, h, w)
    with torch.no_grad():
        eng = SegEngine(net)
        pairs = unit_pairs(net, eng)
        ids = [u.drop_id for _, u in pairs]
        assert len(set(ids)) == len(ids)  # a stream per unit and encoder
        dropping = [m for m, _ in pairs if getattr(m, 'dropout', False) is True]
        assert len(dropping) == 8 * (2 if stage != 1 else 1)  # layer2[-1], layer3[2..5], layer4[0..2] per encoder
        eng.rng.copy_(torch.tensor(state, dtype=torch.int64))
        seed, frame = eng.rng.tolist()
        got = eng(*args)
        torch.cuda.synchronize()
        assert eng.rng.tolist() == [seed, frame + 1]
    want = module_with_masks(net, eng, args, seed, frame)
    top = want.abs().max().item()
    assert 1e-2 < top < 1e4
    err = (got - want).abs().max().item()
    assert err <= 5e-4 * top, (err, top)
    assert (got.argmax(1) == want.argmax(1)).float().mean().item() > 0.999
    wrong = module_with_masks(net, eng, args, seed, frame + 1)
    assert (got - wrong).abs().max().item() > 40 * 5e-4 * top  # the comparison sees the masks


def test_engine_dropout_batch_is_one_pass_numbered_batch_major():
    """eng.forward on 3 images: one pass, one counter step, masks over the batch-major pixel index."""
    from online_joint_depthfusion_and_semantic_amd import segconv
    from online_joint_depthfusion_and_semantic_amd.adapnet_engine import SegEngine
    net = build(2, 30, dropout=True)
    args = lively_inputs(2, 64, 96, batch=3, seed=6)

    def packed(x):  # the stem's rows of every image: [B, 8, H, W] NHWC
        out = segconv.nhwc(8, x.shape[2], x.shape[3], x.device, batch=x.shape[0])
        for b in range(x.shape[0]):
            segconv.pack_input(x[b:b + 1].contiguous(), 1.0, out=out[b:b + 1])
        return out
    with torch.no_grad():
        eng = SegEngine(net)
        eng.rng.copy_(torch.tensor([0x5eed0000cafe1234, (9 << 32) | 1], dtype=torch.int64))
        seed, frame = eng.rng.tolist()
        got = eng(*[packed(a) for a in args])
        torch.cuda.synchronize()
        assert eng.rng.tolist() == [seed, frame + 1]
    want = module_with_masks(net, eng, args, seed, frame)
    top = want.abs().max().item()
    assert (got - want).abs().max().item() <= 5e-4 * top
    assert (got.argmax(1) == want.argmax(1)).float().mean().item() > 0.999
    # image 1 alone draws the masks of pixels 0.. (not H*W..): it differs from its slice of the batch
    alone = module_with_masks(net, eng, [a[1:2] for a in args], seed, frame)
    assert (got[1:2] - alone).abs().max().item() > 40 * 5e-4 * top


def test_engine_dropout_graph_replay_advances_and_matches_eager():
    """A captured forward pass: each replay adds one to the counter and equals, bit for bit, an eager pass run after
    resetting the counter to the replay's frame; consecutive replays draw different masks."""
    from online_joint_depthfusion_and_semantic_amd.adapnet_engine import SegEngine
    net = build(2, 30, dropout=True)
    args = lively_inputs(2, 64, 96, seed=7)
    with torch.no_grad():
        eng = SegEngine(net)
        eng.rng.copy_(torch.tensor([-0x0fedcba987654321, (2 << 32) | 0xfffffffc], dtype=torch.int64))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                eng(*args)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = eng(*args)
        torch.cuda.synchronize()
        seed, frame = eng.rng.tolist()
        prev = None
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            assert eng.rng.tolist() == [seed, frame + 1]
            rep = out.clone()
            eng.rng[1] = frame
            eager = eng(*args)
            torch.cuda.synchronize()
            assert eng.rng.tolist() == [seed, frame + 1]
            assert torch.equal(rep, eager)
            if prev is not None:
                assert not torch.equal(rep, prev)
            prev, frame = rep, frame + 1
    assert frame >> 32 == 3  # the replays carried into the high word
