"""The plans the library makes report what tests/golden/osm_plan_info.json records (see
tests/test_osm_geo.py: `OsmPlan.info()` on an MI355X before the planning moved to csrc/osm_geo.hpp),
for the blocks of up to 2^22 samples: powers of two in this process, lengths that are not with the
mode of plan-time compilation the process runs in, and with BBT_RTC=0 in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import baseband_tasks_amd as bt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'osm_plan_info.json')) as f:
    RECORDS = [r for r in json.load(f) if r['n_fft'] <= 2**22]


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not bt.hip.available():
        pytest.fail("no GPU / libbbt_hip.so: the -m gpu suite must run on an MI355X")


def check(records):
    """Every plan of `records`, one after the other; returns how many."""
    for r in records:
        plan = bt.hip.OsmPlan(r['n_fft'], r['n_stream'], np.ones((1, r['n_fft']), np.complex64))
        try:
            info = plan.info()
        finally:
            plan.close()
        print('CASE', r['n_fft'], r['n_stream'], info, flush=True)
        assert info == r['info'], (r, info)
    return len(records)


def generic(mode):
    return [r for r in RECORDS if r['n_fft'] & (r['n_fft'] - 1) and r['mode'] == mode]


def child():
    assert bt.hip.rtc_info()['mode'] == 'off'
    assert check(generic('off')) == 6


def test_power_of_two_plans_report_the_recorded_geometry():
    assert check([r for r in RECORDS if not r['n_fft'] & (r['n_fft'] - 1)]) == 13


def test_generic_plans_report_the_recorded_geometry():
    mode = bt.hip.rtc_info()['mode']
    assert check(generic('off' if mode == 'off' else 'on')) == 6


def test_generic_plans_without_compilation_report_the_recorded_geometry():
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_osm_geo_gpu as t; t.child()"
            % (ROOT, os.path.join(ROOT, 'tests')))
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, BBT_RTC='0'), capture_output=True,
                         text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.count('CASE ') == 6
