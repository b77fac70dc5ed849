"""CPU: the host front end of the view operators (views.py) - for every helper the forms it accepts, what it makes of them,
and its refusals, each a ValueError that starts with the caller's name.  No device, no library."""
import numpy as np
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import ops, views

WHO = 'some_operator'
K0 = np.array([[500.0, 0.0, 319.5], [0.0, 480.0, 239.5], [0.0, 0.0, 1.0]])


def _pose(i, rows=4):
    a = 0.3 * i
    E = np.eye(4)
    E[:3, :3] = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
    E[:3, 3] = [0.1 * i, -0.2, 1.0 + i]
    return E[:rows]


def _refused(call, *args, **kw):
    with pytest.raises(ValueError) as err:
        call(WHO, *args, **kw)
    assert str(err.value).startswith(WHO + ': '), str(err.value)


# ---- cameras ----------------------------------------------------------------------------------------------------------
CAMERA_FORMS = {
    '3x3+3x4': (K0, _pose(1, 3), None, 1),
    '3x3+4x4': (K0, _pose(1), None, 1),
    'nx3x3+nx4x4': (np.stack([K0, 2 * K0 - np.diag([0, 0, 1.0]), K0]), np.stack([_pose(i) for i in range(3)]), None, 3),
    'one K for n poses': (K0, np.stack([_pose(i, 3) for i in range(3)]), None, 3),
    'one K and one pose for n frames': (K0, _pose(2), 4, 4),
}


@pytest.mark.parametrize('form', sorted(CAMERA_FORMS))
@pytest.mark.parametrize('container', ['numpy', 'torch'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_cameras_accepts(form, container, dtype):
    K, E, n_in, n = CAMERA_FORMS[form]
    K, E = K.astype(dtype), E.astype(dtype)
    wrap = torch.from_numpy if container == 'torch' else (lambda a: a)
    got_n, Kh, Eh = views.cameras(WHO, wrap(K), wrap(E), n_in)
    assert got_n == n
    for a, cols in ((Kh, 9), (Eh, 12)):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (n, cols) and a.flags['C_CONTIGUOUS']
    want_K = np.broadcast_to(K.reshape(-1, 3, 3), (n, 3, 3)).astype(np.float64).reshape(n, 9)
    want_E = np.broadcast_to(E.reshape(-1, E.shape[-2], 4)[:, :3], (n, 3, 4)).astype(np.float64).reshape(n, 12)
    assert np.array_equal(Kh, want_K) and np.array_equal(Eh, want_E)


def test_cameras_refuses():
    poses = np.stack([_pose(i) for i in range(2)])
    _refused(views.cameras, np.stack([K0] * 3), poses)  # 3 intrinsics for 2 views
    _refused(views.cameras, np.stack([K0] * 3), poses, 2)
    _refused(views.cameras, K0, np.stack([_pose(i) for i in range(3)]), 2)  # 3 poses for 2 frames
    skew = K0.copy()
    skew[0, 1] = 1e-3
    _refused(views.cameras, np.stack([K0, skew]), poses)  # the second view only
    nan = poses.copy()
    nan[1, 2, 3] = np.nan
    _refused(views.cameras, K0, nan)
    inf = K0.copy()
    inf[0, 2] = np.inf
    _refused(views.cameras, inf, poses)
    scaled = K0.copy()
    scaled[2, 2] = 2.0
    _refused(views.cameras, scaled, poses)  # K[8] != 1
    flat = K0.copy()
    flat[0, 0] = 0.0
    assert views.cameras(WHO, flat, poses)[0] == 2  # fx == 0 is a pinhole matrix ...
    _refused(views.cameras, flat, poses, nonzero_focal=True)  # ... that rasterize cannot divide by
    _refused(views.cameras, K0[:2], poses)  # shapes
    _refused(views.cameras, K0, poses[:, :2])
    _refused(views.cameras, K0, poses[None])
    _refused(views.cameras, K0, poses[:0])  # no view


# ---- inverse_cameras --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3])
def test_inverse_cameras_is_camera_arrays_view_by_view(n):
    K = torch.from_numpy(K0.astype(np.float32))
    E = torch.from_numpy(np.stack([_pose(i) for i in range(n)]))
    got_n, Ki, Ew = views.inverse_cameras(WHO, K, E if n > 1 else E[0])
    assert got_n == n and Ki.dtype == Ew.dtype == np.float32 and Ki.shape == (n, 9) and Ew.shape == (n, 12)
    for i in range(n):
        ki, ew = ops.camera_arrays(K, E[i])
        assert ki.tobytes() == Ki[i].tobytes() and ew.tobytes() == Ew[i].tobytes()
    _refused(views.inverse_cameras, np.stack([K0] * 2), np.stack([_pose(i) for i in range(3)]))
    _refused(views.inverse_cameras, K0, E[..., :3])


# ---- depth_frames, images ---------------------------------------------------------------------------------------------
def test_depth_frames():
    cpu = torch.device('cpu')
    d = torch.arange(2 * 5 * 7, dtype=torch.float64).reshape(2, 5, 7)
    one = views.depth_frames(WHO, d[0], cpu)
    assert one.dtype == torch.float32 and one.shape == (1, 5, 7) and one.is_contiguous() and torch.equal(one[0], d[0].float())
    both = views.depth_frames(WHO, d, cpu)
    assert both.dtype == torch.float32 and both.shape == (2, 5, 7) and torch.equal(both, d.float())
    strided = d.float()[:, ::2, 1::3]
    assert not strided.is_contiguous()
    got = views.depth_frames(WHO, strided, cpu)
    assert got.is_contiguous() and got.shape == (2, 3, 2) and torch.equal(got, strided)
    ready = d.float()
    assert views.depth_frames(WHO, ready, cpu).data_ptr() == ready.data_ptr()  # nothing to do: no copy
    _refused(views.depth_frames, d[:0], cpu)  # n = 0
    _refused(views.depth_frames, d[None], cpu)  # 4-D
    _refused(views.depth_frames, d[0, 0], cpu)  # 1-D
    _refused(views.depth_frames, d, 'meta')  # a tensor that lives elsewhere
    _refused(views.depth_frames, d.numpy(), cpu)


def test_images():
    cpu = torch.device('cpu')
    assert views.images(WHO, None, 'mask', torch.uint8, 2, 3, 4, cpu) is None
    mask = torch.rand(2, 3, 4) > 0.5
    got = views.images(WHO, mask, 'mask', torch.uint8, 2, 3, 4, cpu)
    assert got.dtype == torch.uint8 and got.shape == (2, 3, 4) and got.data_ptr() == mask.data_ptr()  # reinterpreted in place
    assert torch.equal(got, mask.to(torch.uint8))
    flat = views.images(WHO, mask[0].reshape(-1), 'mask', torch.uint8, 1, 3, 4, cpu)  # any shape with the element count
    assert flat.shape == (1, 3, 4) and torch.equal(flat[0], mask[0].to(torch.uint8))
    scores = views.images(WHO, torch.ones(2, 3, 4, dtype=torch.float64), 'label_scores', torch.float32, 2, 3, 4, cpu)
    assert scores.dtype == torch.float32 and scores.is_contiguous()
    _refused(views.images, mask, 'mask', torch.uint8, 2, 3, 5, cpu)  # a wrong element count
    _refused(views.images, mask, 'mask', torch.uint8, 2, 3, 4, 'meta')
    _refused(views.images, mask.numpy(), 'mask', torch.uint8, 2, 3, 4, cpu)


# ---- running_mean_options ---------------------------------------------------------------------------------------------
def test_running_mean_options():
    assert views.running_mean_options(WHO, 'band', 0.04, 1, 0) == (0.04, 1.0, 0.0)
    assert views.running_mean_options(WHO, 'truncation', np.float32(0.5), 2048, 0.25) == (0.5, 2048.0, 0.25)
    nan, inf = float('nan'), float('inf')
    for width in (0, -0.01, inf, nan):
        _refused(views.running_mean_options, 'band', width, 64.0, 0.0)
    for max_weight in (0.5, 2049, nan, inf):
        _refused(views.running_mean_options, 'band', 0.04, max_weight, 0.0)
    for near in (-0.01, inf, nan):
        _refused(views.running_mean_options, 'band', 0.04, 64.0, near)
    with pytest.raises(ValueError, match='truncation > 0'):
        views.running_mean_options(WHO, 'truncation', 0, 64.0, 0.0)


# ---- volume3 ----------------------------------------------------------------------------------------------------------
def test_volume3():
    cpu = torch.device('cpu')
    ids = torch.zeros(3, 4, 5, dtype=torch.uint8)
    assert views.volume3(WHO, ids, 'ids', torch.uint8, (3, 4, 5), cpu) is ids
    _refused(views.volume3, ids, 'ids', torch.uint8)  # a volume on its own must be on a cuda device
    _refused(views.volume3, ids, 'ids', torch.float16, (3, 4, 5), cpu)
    _refused(views.volume3, ids, 'ids', torch.uint8, (3, 4, 6), cpu)
    _refused(views.volume3, ids[0], 'ids', torch.uint8, (4, 5), cpu)
    _refused(views.volume3, ids, 'ids', torch.uint8, (3, 4, 5), 'meta')
    _refused(views.volume3, ids.numpy(), 'ids', torch.uint8, (3, 4, 5), cpu)
    _refused(views.volume3, None, 'weights', torch.float16, (3, 4, 5), cpu)
    strided = torch.zeros(3, 4, 10, dtype=torch.uint8)[:, :, ::2]
    _refused(views.volume3, strided, 'ids', torch.uint8, (3, 4, 5), cpu)
    got = views.volume3(WHO, strided, 'ids', torch.uint8, (3, 4, 5), cpu, copy=True)
    assert got.is_contiguous() and got.shape == (3, 4, 5)


# ---- the volume operators' half ------------------------------------------------------------------------------------------
def test_mask_volume_tsdf_pair_and_on_device():
    mask = torch.zeros(3, 4, 5, dtype=torch.bool)
    as_u8 = views.mask_volume(WHO, mask, 'mask', torch.uint8)  # a volume on its own: wherever it lives; bool is reinterpreted
    assert as_u8.dtype == torch.uint8 and as_u8.data_ptr() == mask.data_ptr()
    keys = torch.zeros(3, 4, 5, dtype=torch.uint8)
    assert views.mask_volume(WHO, keys, 'keys', torch.uint8, like=as_u8) is keys
    _refused(views.mask_volume, keys[:2], 'keys', torch.uint8, like=as_u8)
    _refused(views.mask_volume, keys.numpy(), 'keys', torch.uint8)
    _refused(views.mask_volume, keys.float(), 'keys', torch.uint8)
    tsdf, wgt = torch.zeros(3, 4, 5, dtype=torch.float16), torch.ones(3, 4, 5, dtype=torch.float16)
    got = views.tsdf_pair(WHO, tsdf, wgt)
    assert got[0] is tsdf and got[1] is wgt
    _refused(views.tsdf_pair, tsdf, wgt[:, :, :4])
    _refused(views.tsdf_pair, tsdf, wgt.float())
    with pytest.raises(ValueError, match=WHO + ': the volumes must be cuda tensors'):  # the device check comes first
        views.on_device(WHO, tsdf)
    with pytest.raises(ValueError, match=WHO + ': the volumes must be cuda tensors'):
        views.on_device(WHO, tsdf, 2048)


# ---- chunks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, spans', [(1, [(0, 1)]), (32, [(0, 32)]), (33, [(0, 32), (32, 33)]), (64, [(0, 32), (32, 64)]),
                                      (65, [(0, 32), (32, 64), (64, 65)])])
def test_chunks(n, spans):
    K = np.arange(9.0 * n).reshape(n, 9)
    E = np.asfortranarray(np.arange(12.0 * n).reshape(n, 12))  # (slices of it are not C-contiguous)
    got = list(views.chunks(n, 32, K, E))
    assert [(v0, v1) for v0, v1, _, _ in got] == spans
    for v0, v1, Kc, Ec in got:
        assert Kc.flags['C_CONTIGUOUS'] and Ec.flags['C_CONTIGUOUS']
        assert np.array_equal(Kc, K[v0:v1]) and np.array_equal(Ec, E[v0:v1])
    assert views.part(None, 0, 1) is None and np.array_equal(views.part(K, 0, 1), K[:1])
