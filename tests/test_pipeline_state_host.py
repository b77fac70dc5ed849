"""CPU: the host state around Pipeline's frame steps, each in the object that owns it - guard_records.GuardRecords (the ring of
remembered frames, its event marks and latch records), announce.TrainingAnnouncements (held announcements, counters, counts) - and
the module tree of Pipeline itself, which none of these objects may join."""
import pytest
import torch

from online_joint_depthfusion_and_semantic_amd import _lib
from online_joint_depthfusion_and_semantic_amd.announce import TrainingAnnouncements
from online_joint_depthfusion_and_semantic_amd.config import default_config
from online_joint_depthfusion_and_semantic_amd.guard_records import GuardRecords
from online_joint_depthfusion_and_semantic_amd.pipeline import Pipeline


# ---- Pipeline's module tree ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('strategy', ['gt', 'predict'])
@pytest.mark.parametrize('name', ['v3', 'v2', 'tsdf'])
def test_the_module_tree_is_the_two_networks(name, strategy):
    """An owner object that held a module (or was one) would add state_dict keys and children silently: checkpoints of the parent
    would stop loading strictly."""
    cfg = default_config(32, 48, semantics=True, use_semantics=True, n_classes=5, model=name)
    cfg.DATA.semantic_strategy = strategy
    pipe = Pipeline(cfg)
    nets = [('_fusion_network', pipe._fusion_network)]
    if strategy == 'predict':
        nets.append(('_semantic_2d_network', pipe._semantic_2d_network))
    else:
        assert pipe._semantic_2d_network is None
    assert set(pipe.state_dict()) == {prefix + '.' + k for prefix, net in nets for k in net.state_dict()}
    # the children are those networks and, as before the owner objects existed, the two stateless stage modules of the reference's API
    children = dict(pipe.named_children())
    assert list(children) == [n for n, _ in nets] + ['_extractor', '_integrator']
    assert all(children[n] is net for n, net in nets)
    for n in ('_extractor', '_integrator'):
        assert not children[n].state_dict() and not list(children[n].children())


def test_a_deep_copy_owns_its_own_state():
    """The owners hold the pipeline's sub-module dict and config, no closure over the pipeline: a copy reads the copy's."""
    import copy
    cfg = default_config(32, 48, semantics=True, use_semantics=True, n_classes=5)
    cfg.DATA.semantic_strategy = 'predict'
    pipe = Pipeline(cfg)
    twin = copy.deepcopy(pipe)
    assert pipe._labels2d.network() is pipe._semantic_2d_network
    assert twin._labels2d.network() is twin._semantic_2d_network is not pipe._semantic_2d_network
    assert twin._guard.config is twin.config is not pipe.config and twin._labels2d.config is twin.config
    replaced = torch.nn.Identity()
    twin._semantic_2d_network = replaced
    assert twin._labels2d.network() is replaced and pipe._labels2d.network() is pipe._semantic_2d_network


# ---- GuardRecords with stand-ins for the event and the flag read ---------------------------------------------------------------
class _Event:
    def __init__(self, log):
        self.log = log

    def synchronize(self):
        self.log.append('sync')


class _Workspace:
    def __init__(self, skipped):
        self.skipped = skipped

    def guard_latch(self):  # (ops.IntegrateWorkspace.guard_latch: the four bytes of the latch word)
        return torch.tensor([int(self.skipped), 0, 0, 0], dtype=torch.uint8)


def _records(flag_set=False, policy='f32'):
    log = []
    cfg = default_config(24, 32)
    cfg.FUSION_MODEL.guard_policy = policy
    return GuardRecords(cfg, record_event=lambda device: _Event(log), guard_is_set=lambda: flag_set), log


def _frame(i):
    return {'frame_id': ['scene/%d' % i]}


def _ids(rec):
    return [r[0]['frame_id'][0] for r in rec.ring]


def test_a_silent_guard_forgets_the_frames_in_front_of_the_oldest_mark():
    rec, log = _records()
    for i in range(49):
        rec.remember(_frame(i), 'db')
        assert len(rec.ring) <= GuardRecords.KEEP
    assert _ids(rec) == ['scene/%d' % i for i in range(16, 49)] and [m[0] for m in rec.marks] == [16, 32]
    assert log == ['sync']  # (the one completed mark was awaited before the flag was read)
    for i in range(49, 64):
        rec.remember(_frame(i), 'db')
    assert _ids(rec) == ['scene/%d' % i for i in range(16, 64)] and [m[0] for m in rec.marks] == [16, 32, 48]
    rec.remember(_frame(64), 'db')
    assert _ids(rec) == ['scene/%d' % i for i in range(32, 65)] and [m[0] for m in rec.marks] == [16, 32]
    assert all(r[1] == 'db' for r in rec.ring)


def test_a_set_guard_forgets_nothing():
    rec, _ = _records(flag_set=True)
    for i in range(49):
        rec.remember(_frame(i), 'db')
    assert _ids(rec) == ['scene/%d' % i for i in range(49)]


@pytest.mark.parametrize('policy,arithmetic', [('raise', 'f16x3'), ('off', 'f16x3'), ('f32', 'f32')])
def test_another_policy_remembers_nothing(policy, arithmetic):
    """(with the fp32 arithmetic there is nothing to switch to: guard_policy 'f32' does not hold then)"""
    rec, log = _records(policy=policy)
    rec.config.FUSION_MODEL.arithmetic = arithmetic
    rec.note(0, _Workspace(True))
    for i in range(20):
        rec.remember(_frame(i), 'db')
    assert rec.ring == [] and rec.marks == [] and rec.latches == {} and log == []


def test_a_slots_latch_goes_to_the_frame_remembered_for_that_slot():
    rec, _ = _records()
    rec.note(1, _Workspace(True))
    rec.note(0, _Workspace(False))
    b = _frame(7)
    rec.remember(b, 'db', slot=1)
    assert rec.ring[0][0] is b and rec.ring[0][2].tolist() == [1, 0, 0, 0]
    assert list(rec.latches) == [0]  # slot 1 handed its latch over, slot 0 still holds its own


def test_a_frame_without_a_noted_integrate_call_has_no_record():
    rec, _ = _records()
    rec.remember(_frame(0), 'db')
    assert rec.ring[0][2] is None
    with pytest.raises(_lib.OjfError, match='no record of its integrate call'):
        rec.take(0)


def test_take_returns_the_skipped_frames_in_ring_order_and_empties_the_records():
    rec, _ = _records()
    skipped = [False, False, True, False, True, True, False]
    frames = [_frame(i) for i in range(len(skipped))]
    for i, (f, s) in enumerate(zip(frames, skipped)):
        rec.note(i % 3, _Workspace(s))
        rec.remember(f, 'db%d' % i, slot=i % 3)
    rec.note(2, _Workspace(True))  # (an integrate call whose frame was never remembered: its latch is dropped with the rest)
    with pytest.raises(_lib.OjfError, match='range guard: the device counted 2 skipped frames'):
        rec.take(2)
    assert len(rec.ring) == len(frames)  # a refused take keeps the records
    redo, skips = rec.take(3)
    assert len(redo) == 3 and all(got[0] is frames[i] and got[1] == 'db%d' % i for got, i in zip(redo, (2, 4, 5)))
    assert skips == [('scene/%d' % i, s) for i, s in enumerate(skipped)]
    assert rec.ring == [] and rec.marks == [] and rec.latches == {}
    assert rec.take(0) == ([], [])


def test_take_clears_the_marks_too():
    rec, _ = _records()
    for i in range(20):
        rec.note(0, _Workspace(False))
        rec.remember(_frame(i), 'db')
    assert [m[0] for m in rec.marks] == [16]
    assert rec.take(0)[0] == [] and rec.marks == [] and rec.ring == []


# ---- TrainingAnnouncements on CPU tensors ---------------------------------------------------------------------------------------
def _announce(ann, batch, device='cpu'):
    frame = torch.arange(12, dtype=torch.float32, device=device).reshape(1, 3, 4)
    filtered = torch.where(frame % 3 != 0, frame, torch.zeros(()))
    frame, filtered = frame[0], filtered[0]
    ann.announce(batch, frame, filtered)
    return frame, filtered


def test_announcements_are_matched_by_identity_and_outlive_one_foreign_frame_step():
    ann = TrainingAnnouncements()
    b0, b1, b2, stranger = ({'frame_id': ['s/%d' % i]} for i in range(4))
    frame, filtered = _announce(ann, b1)
    assert ann.take(b0, 'cpu') is None  # a miss; b1 survives it
    assert (ann.hits, ann.misses) == (0, 1) and [a[0] for a in ann.held] == [b1]
    _announce(ann, stranger)  # announced between two frames, never brought
    assert [a[0] for a in ann.held] == [b1, stranger]
    hit = ann.take(b1, 'cpu')
    assert hit[0] is b1 and hit[1] is frame and hit[2] is filtered and (ann.hits, ann.misses) == (1, 1)
    assert [a[0] for a in ann.held] == [stranger]  # held through one frame step of another batch ...
    assert ann.take(dict(b1), 'cpu') is None  # (an equal dict is another object)
    assert ann.held == [] and (ann.hits, ann.misses) == (1, 2)  # ... and dropped by the second
    for b in (b0, b1, b2):
        _announce(ann, b)
        assert len(ann.held) <= 2
    assert [a[0] for a in ann.held] == [b1, b2]
    ann.announce(None)
    assert ann.held == []
    assert ann.take(b2, 'cpu') is None and (ann.hits, ann.misses) == (1, 3)


def test_an_announcement_for_another_device_is_dropped():
    ann = TrainingAnnouncements()
    b = {'frame_id': ['s/0']}
    _announce(ann, b)
    assert ann.take(b, 'meta') is None and ann.held == [] and (ann.hits, ann.misses) == (0, 1)
    _announce(ann, b)
    assert ann.take(b, 'cpu')[0] is b and (ann.hits, ann.misses) == (1, 1)


def test_the_count_of_a_host_mask_is_an_int_and_the_index_is_nonzero():
    ann = TrainingAnnouncements()
    b = {'frame_id': ['s/0']}
    frame, filtered = _announce(ann, b)
    _, _, _, valid_mask, count, seen = ann.take(b, 'cpu')
    want = (filtered.reshape(-1) != 0)
    assert isinstance(count, int) and count == int(want.sum()) == 8 and seen == 0 and torch.equal(valid_mask, want)
    assert torch.equal(ann.valid_index(valid_mask, count), want.nonzero()[:, 0])
    assert ann.async_count(torch.zeros(5, dtype=torch.bool)) == 0
