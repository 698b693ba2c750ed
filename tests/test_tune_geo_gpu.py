"""The plans that time candidate kernels compare what tests/golden/tune_candidates.json records
(see tests/test_tune_geo.py: the lines BBT_RTC_VERBOSE=1 printed on an MI355X before the rules
moved to csrc/chan_geo.hpp and csrc/pfb_geo.hpp), in the recorded order.  One fresh child process
per shape (tools/tune_candidates.py: child), since a process remembers its choices: the child
checks the output of the chosen kernel against the oracle on 11 spectra and makes the same plan
again, which must compare nothing and compile nothing."""
import json
import os
import subprocess
import sys

import pytest

import baseband_tasks_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import tune_candidates  # noqa: E402

pytestmark = pytest.mark.gpu

with open(tune_candidates.GOLDEN) as f:
    GOLDEN = json.load(f)
CASES = [(kind, r) for kind in tune_candidates.SHAPES for r in GOLDEN[kind]]
abnormal = []          # the first child that ended abnormally: nothing more is started on the device


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not bt.hip.available():
        pytest.fail("no GPU / libbbt_hip.so: the -m gpu suite must run on an MI355X")


def test_the_record_covers_the_shapes():
    assert [(kind, tuple(r['shape'])) for kind, r in CASES] == [(kind, s) for kind, shapes in tune_candidates.SHAPES.items()
                                                                 for s in shapes]


@pytest.mark.parametrize('kind, record', CASES, ids=lambda v: v if isinstance(v, str) else 'x'.join(str(n) for n in v['shape']))
def test_timed_plans_compare_the_recorded_candidates(kind, record):
    if bt.hip.rtc_info()['mode'] == 'off' and kind == 'channelize':
        pytest.skip('BBT_RTC=0: no channelizer plan times candidates')
    assert not abnormal, f'an earlier child ended abnormally: {abnormal[0]}'
    try:
        done = tune_candidates.run_child(kind, record['shape'])
    except subprocess.TimeoutExpired as e:
        abnormal.append((kind, record['shape'], 'timeout'))
        pytest.fail(f'the child did not end: {e}')
    print(done.stdout)
    if done.returncode < 0 or done.returncode > 1:
        abnormal.append((kind, record['shape'], done.returncode))
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-3000:])
    first, mark, second = done.stderr.partition(tune_candidates.MARK)
    assert mark
    assert tune_candidates.candidates(first, kind, record['shape']) == record['candidates']
    assert tune_candidates.parse(second) == ([], [])                     # remembered: no candidate is timed again
    before, after = (int(v) for v in done.stdout.split()[-2:])
    assert after == before, done.stdout                                  # ... and nothing compiled
