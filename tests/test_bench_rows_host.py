"""The parent loop of the row-by-row bench tools (tools/bench_rows.py) without a GPU and without the library:
a child script written for the test stands in for a tool.  What a visit to a shared GPU relies on is pinned
here: a row is a process of its own with the tool's own command line, and after the first row that fails or
runs out of time nothing more is started."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bench_rows                                                    # noqa: E402

#: stands in for a tool: leaves `<row>.started` beside itself, then does what the row's name says
CHILD = '''
import json, os, sys, time
row = sys.argv[-1]
open(os.path.join(os.path.dirname(os.path.abspath(__file__)), row + '.started'), 'w').close()
if row.startswith('fail'):
    sys.exit(3)
if row.startswith('sleep'):
    time.sleep(60)
print('something a library says on the way')
print(json.dumps(dict(row=row, argv=sys.argv[1:])), flush=True)
'''


def _tool(tmp_path):
    script = tmp_path / 'tool.py'
    script.write_text(CHILD)
    return str(script), str(tmp_path / 'out' / 'rows.jsonl')


def _started(tmp_path):
    return sorted(name[:-len('.started')] for name in os.listdir(tmp_path) if name.endswith('.started'))


def test_every_row_is_printed_and_appended(tmp_path, capsys):
    script, out = _tool(tmp_path)
    os.makedirs(os.path.dirname(out))
    with open(out, 'w') as f:
        f.write('{"row": "from an earlier run"}\n')
    assert bench_rows.run_rows(script, ['ok_a', 'ok_b'], 3, 30, out) == 0
    want = [dict(row=row, argv=['--child', '--reps', '3', row]) for row in ('ok_a', 'ok_b')]
    printed = capsys.readouterr()
    assert [json.loads(line) for line in printed.out.splitlines()] == want and printed.err == ''
    with open(out) as f:
        assert [json.loads(line) for line in f] == [dict(row='from an earlier run')] + want
    assert _started(tmp_path) == ['ok_a', 'ok_b']


def test_a_failed_row_ends_the_run(tmp_path, capsys):
    script, out = _tool(tmp_path)
    assert bench_rows.run_rows(script, ['ok_a', 'fail', 'ok_b'], 1, 30, out) == 1
    printed = capsys.readouterr()
    assert printed.err == 'fail: exit status 3; stopping\n'
    assert _started(tmp_path) == ['fail', 'ok_a']                    # ok_b was never started
    with open(out) as f:
        assert [json.loads(line)['row'] for line in f] == ['ok_a'] == [json.loads(line)['row'] for line in printed.out.splitlines()]


def test_a_row_beyond_its_time_limit_ends_the_run(tmp_path, capsys):
    script, out = _tool(tmp_path)
    assert bench_rows.run_rows(script, ['ok_a', 'sleep', 'ok_b'], 1, 1, out) == 1
    printed = capsys.readouterr()
    assert printed.err == 'sleep: no result within 1 s; stopping\n'
    assert _started(tmp_path) == ['ok_a', 'sleep']                   # ok_b was never started
    with open(out) as f:
        assert [json.loads(line)['row'] for line in f] == ['ok_a'] == [json.loads(line)['row'] for line in printed.out.splitlines()]
