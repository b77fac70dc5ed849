"""CPU: which remembered frames a range-guard recovery (FUSION_MODEL.guard_policy 'f32') fuses again -
guard_records.guard_frames_to_fuse_again on hand-made rings.  The rule it replaces was "the last n of the ring"."""
import os
import re

import pytest

from online_joint_depthfusion_and_semantic_amd import _lib, ops
from online_joint_depthfusion_and_semantic_amd.guard_records import guard_frames_to_fuse_again as select

HERE = os.path.dirname(os.path.abspath(__file__))


def _ring(*names):
    return [(name, 'db') for name in names]


def _tail_rule(ring, n):
    """what _guard_recover did before the per-frame records: the last n remembered frames"""
    return ring[len(ring) - n:] if n else []


def test_the_skipped_frames_are_the_tail():
    ring = _ring('a0', 'b0', 'c0', 'a1', 'b1', 'c1')
    records = [False, False, False, True, True, True]
    assert select(ring, records, 3) == ring[3:] == _tail_rule(ring, 3)


def test_only_the_middle_scene_of_three_skipped():
    """Per-slot fuse_many: scene c's stream latched "not set" before scene b's net raised the flag, scene a ran in front of it.
    The recovery must fuse b1 again and nothing else.  The earlier ``ring[-n:]`` rule picks c1 - fused twice, b1 lost -
    which the last assertion shows: with that rule in place of the selection this test fails."""
    ring = _ring('a0', 'b0', 'c0', 'a1', 'b1', 'c1')
    records = [False, False, False, False, True, False]
    assert select(ring, records, 1) == [('b1', 'db')]
    assert _tail_rule(ring, 1) == [('c1', 'db')] != select(ring, records, 1)


def test_the_skipped_set_spans_two_calls_and_keeps_ring_order():
    """The event is noticed one call late: b1 tripped, c1 went through, then every frame of the next call skipped."""
    ring = _ring('a0', 'b0', 'c0', 'a1', 'b1', 'c1', 'a2', 'b2', 'c2')
    records = [False] * 4 + [True, False, True, True, True]
    assert select(ring, records, 4) == _ring('b1', 'a2', 'b2', 'c2')
    assert _tail_rule(ring, 4) == _ring('c1', 'a2', 'b2', 'c2')


def test_nothing_skipped():
    """The flag was raised behind the last integrate call: the arithmetic switches, no frame is fused again."""
    ring = _ring('a0', 'b0', 'c0')
    assert select(ring, [False] * 3, 0) == []
    assert select([], [], 0) == []


@pytest.mark.parametrize('records,count', [([False, True, False], 2), ([False, True, False], 0), ([True, True, True], 4),
                                           ([False, False, False], 1), ([False, True], 1)])
def test_records_and_device_count_must_agree(records, count):
    """A frame skipped that nobody remembers (a frame step outside the ring, a pruned ring), a record without its skip, or a ring
    and records of different lengths: OjfError, not a guess."""
    with pytest.raises(_lib.OjfError, match='range guard'):
        select(_ring('a', 'b', 'c'), records, count)


def test_the_latch_word_is_the_kernels():
    """ops.IntegrateWorkspace.guard_latch copies header word kGuardLatch of csrc/ojf_integrate.h, inside the header."""
    with open(os.path.join(HERE, '..', 'online_joint_depthfusion_and_semantic_amd', 'csrc', 'ojf_integrate.h')) as f:
        src = f.read()
    word = int(re.search(r'constexpr int kGuardLatch = (\d+);', src).group(1))
    header = int(re.search(r'kHeaderBytes = (\d+)', src).group(1))
    assert ops.IntegrateWorkspace.GUARD_LATCH_WORD == word and 4 * word + 4 <= header
