"""CPU: the fusion net's forward plan (ojf_net_plan: the planner ojf_net_create runs, on a bare shape - no device) against the launch
sequences recorded from the commit before the plan existed (net_plan_cases.py), its refusals, the test-only switch (read once per
process: child processes) and the retired switches, which change nothing."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from online_joint_depthfusion_and_semantic_amd import _lib
from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine
import net_plan_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in cases.SWITCH_PLANS:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize('case', list(cases.PLANS), ids=lambda c: 'v%d-sem%d-%dx%d-%dx%d-%s' % c)
def test_plan_equals_the_recorded_pass(case):
    version, sem, n_points, growth, h, w, arith = case
    assert FusionNetEngine.plan(version, n_points, growth, sem, h, w, arith) == cases.PLANS[case]


def test_sanity_anchor():
    """The reference topology in split-fp16 at 24x32 is the ten launches the header comment of ojf_net.hip lists; at 45x77
    (w % 8 != 0) the first becomes one dense_pair_kernel launch per Block."""
    ten = ['dense_chain_kernel', 'entry1x1_kernel', 'pool_pyramid_kernel', 'conv_f16x3_kernel (grouped)', 'conv_f16x3_kernel (grouped)',
           'vortex_tail_kernel (+ next entry GEMM)', 'pool_pyramid_kernel', 'conv_f16x3_kernel (grouped)', 'conv_f16x3_kernel (grouped)',
           'vortex_tail_kernel (+ prediction head)']
    assert FusionNetEngine.plan(3, 9, 5, False, 24, 32) == ten
    assert FusionNetEngine.plan(3, 9, 5, False, 45, 77) == ['dense_pair_kernel'] * 5 + ten[1:]


_SWITCH_SCRIPT = """
import sys
sys.path.insert(0, sys.argv[1])
from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine
print('\\n'.join(FusionNetEngine.plan(3, 9, 5, False, 24, 32, 'f16x3')))
"""


@pytest.mark.parametrize('switch', list(cases.SWITCH_PLANS))
def test_switches_change_the_plan_as_they_change_the_run(switch):
    env = {k: v for k, v in os.environ.items() if k not in cases.SWITCH_PLANS}
    env[switch] = '1'
    out = subprocess.run([sys.executable, '-c', _SWITCH_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.split('\n')[:-1]
    assert got == cases.SWITCH_PLANS[switch]
    assert got != cases.PLANS[(3, 0, 9, 5, 24, 32, 'f16x3')]


_ALL_ROWS_SCRIPT = """
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from online_joint_depthfusion_and_semantic_amd.engine import FusionNetEngine
import net_plan_cases as cases
print(json.dumps([FusionNetEngine.plan(v, p, g, s, h, w, a) for v, s, p, g, h, w, a in cases.PLANS]))
"""


def test_retired_switches_are_inert():
    """OJF_BRANCH_KERNEL=1 and OJF_SUBCONV=1 once selected vortex_branch_kernel / subconv_kernel (removed).  With both
    set, every row of the table and the row of the remaining switch still plan what the table records."""
    env = {k: v for k, v in os.environ.items() if k not in cases.SWITCH_PLANS}
    env.update(OJF_BRANCH_KERNEL='1', OJF_SUBCONV='1')
    out = subprocess.run([sys.executable, '-c', _ALL_ROWS_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert dict(zip(cases.PLANS, json.loads(out.stdout))) == cases.PLANS
    for switch, plan in cases.SWITCH_PLANS.items():
        out = subprocess.run([sys.executable, '-c', _SWITCH_SCRIPT, ROOT], env=dict(env, **{switch: '1'}), capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split('\n')[:-1] == plan


def _refused(*args):
    lib = _lib.load()
    rc = lib.ojf_net_plan(*args)
    return rc, lib.ojf_last_error().decode()


def test_refusals():
    buf = ctypes.create_string_buffer(8192)
    good = (3, 9, 5, 0, 24, 32, _lib.ARITH_F16X3)
    assert _lib.load().ojf_net_plan(*good, buf, 8192) == 10
    for args, what in [
            (good + (None, 8192), 'bad argument'),
            (good + (buf, 0), 'bad argument'),
            ((4,) + good[1:] + (buf, 8192), 'version must be 2 or 3'),
            ((3, 0, 5, 0, 24, 32, _lib.ARITH_F16X3, buf, 8192), 'bad sizes'),
            ((3, 9, 0, 0, 24, 32, _lib.ARITH_F16X3, buf, 8192), 'bad sizes'),
            ((3, 9, 5, 0, 0, 32, _lib.ARITH_F16X3, buf, 8192), 'bad sizes'),
            ((3, 9, 5, 0, 24, -1, _lib.ARITH_F16X3, buf, 8192), 'bad sizes'),
            ((3, 9, 5, 0, 24, 32, 7, buf, 8192), 'unknown arithmetic'),
            ((3, 9, 5, 1, 24, 32, _lib.ARITH_F16X3, buf, 8192), None),  # (two heads of 116 channels: 232 <= 256, planned)
            ((3, 12, 5, 1, 24, 32, _lib.ARITH_F16X3, buf, 8192), 'topology too wide'),
    ]:
        rc, err = _refused(*args)
        if what is None:
            assert rc > 0
            continue
        assert rc < 0 and err.startswith('ojf_net_plan: ') and what in err, (args[:7], rc, err)
    # a buffer one byte short of the names and their terminator is refused, the exact size is not
    need = sum(len(n) + 1 for n in cases.PLANS[(3, 0, 9, 5, 24, 32, 'f16x3')]) + 1
    rc, err = _refused(*good, buf, need - 1)
    assert rc < 0 and 'names buffer too small' in err
    assert _lib.load().ojf_net_plan(*good, buf, need) == 10
