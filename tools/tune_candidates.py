"""Which candidates the timed plans compare (csrc/chan_geo.hpp, csrc/pfb_geo.hpp; timed through
csrc/tune.hpp), as the library itself reports them with BBT_RTC_VERBOSE=1.

  python tools/tune_candidates.py record [out.json]   one fresh child process per shape of SHAPES;
                                                      writes tests/golden/tune_candidates.json
  python tools/tune_candidates.py child <kind> <shape...>   what each child runs (also the children
                                                      of tests/test_tune_geo_gpu.py)

A child makes the plan through the task (Channelize / PolyphaseFilterBank on 11 spectra, checked
against the oracle), prints MARK on stderr, and makes the same plan twice more: through a new task
and through the plan class.  `parse` turns the verbose lines into lists of small integers, the
times stripped: Channelize [points per thread, pairs, transforms per workgroup], filter bank
[pairs per workgroup (0: two passes, 1: one pair), order of the workgroups]."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'tune_candidates.json')
# (n_chan, n_stream) and (n_tap, n_chan, n_stream)
SHAPES = {'channelize': [(14, 2), (360, 16), (1000, 2)],
          'filter_bank': [(4, 1024, 32), (12, 256, 8), (8, 2048, 16)]}
MARK = 'tune_candidates: second time'
CHILD_TIMEOUT = 120
REL_L2_TOL, MAX_TOL = 1e-6, 1e-5         # (the suite's: tests/test_gpu_parity.py)

CHAN_LINE = re.compile(r'bbt: Channelize\((\d+)\) x (\d+) streams, (\d+) points per thread, '
                       r'(\d+) pairs x (\d+) transforms per workgroup: ')
PFB_LINE = re.compile(r'bbt: PolyphaseFilterBank (\d+) x (\d+) on (\d+) streams, (two passes|one pass) '
                      r'\(pairs (\d+), order (\d+)\): ')


def parse(text):
    """(channelize, filter_bank): for every candidate line of `text`, in order, the shape it names
    and the candidate, as ((n_chan, n_stream), [points, pairs, transforms]) and
    ((n_tap, n_chan, n_stream), [pairs, order]).  Lines are matched by their prefix: the stderr of
    a verbose run also carries generated source."""
    chan, pfb = [], []
    for line in text.splitlines():
        m = CHAN_LINE.match(line)
        if m:
            v = [int(g) for g in m.groups()]
            chan.append((tuple(v[:2]), v[2:]))
        m = PFB_LINE.match(line)
        if m:
            assert (m.group(4) == 'two passes') == (int(m.group(5)) == 0), line
            pfb.append((tuple(int(m.group(i)) for i in (1, 2, 3)), [int(m.group(5)), int(m.group(6))]))
    return chan, pfb


def candidates(text, kind, shape):
    """The candidates `text` lists, every line being of `kind` and `shape`."""
    chan, pfb = parse(text)
    lines, other = (chan, pfb) if kind == 'channelize' else (pfb, chan)
    assert not other and all(s == tuple(shape) for s, _ in lines), (kind, shape, chan, pfb)
    return [c for _, c in lines]


def child(kind, shape):
    import numpy as np
    sys.path.insert(0, ROOT)
    import baseband_tasks_amd as bt
    from baseband_tasks_amd import units as u
    from oracle import bbt_oracle as orc
    t0 = '2020-01-01T00:00:00'
    n_spec = 11
    n_stream = shape[-1]
    rng = np.random.default_rng(sum(shape))

    def parity(got, want):
        assert got.shape == want.shape and got.dtype == np.complex64, (got.shape, want.shape, got.dtype)
        d = np.asarray(got, np.complex128) - want
        e2 = np.linalg.norm(d.ravel()) / np.linalg.norm(want.ravel())
        em = np.abs(d).max() / np.sqrt(np.mean(np.abs(want) ** 2))
        print(f'parity: rel-L2 {e2:.2e}, max / rms {em:.2e}', flush=True)
        assert e2 <= REL_L2_TOL and em <= MAX_TOL, (kind, shape, e2, em)

    if kind == 'channelize':
        n_chan = shape[0]
        x = rng.standard_normal((n_spec * n_chan, n_stream, 2), dtype=np.float32).view(np.complex64)[..., 0]

        def task():
            return bt.Channelize(bt.DeviceStream(x, t0, 1 * u.MHz), n_chan).read()

        def plan():
            bt.hip.ChanPlan(n_chan, n_stream, -1).close()
        want = orc.channelize(x, n_chan)
    else:
        n_tap, n_chan = shape[:2]
        n_in = (n_spec + n_tap - 1) * n_chan
        x = rng.standard_normal((n_in, n_stream, 2), dtype=np.float32).view(np.complex64)[..., 0]

        def task():
            ds = bt.DeviceStream(x, t0, 1 * u.MHz, samples_per_frame=n_in)
            return bt.PolyphaseFilterBank(ds, bt.sinc_hamming(n_tap, n_chan), samples_per_frame=n_spec).read()

        def plan():
            bt.hip.PfbPlan(bt.sinc_hamming(n_tap, n_chan), n_stream).close()
        want, _ = orc.polyphase_filter_bank(x, orc.sinc_hamming(n_tap, n_chan), n_in, samples_per_frame=n_spec)
    first = task()
    parity(first, want)
    modules = bt.hip.rtc_info()['modules']
    print(MARK, file=sys.stderr, flush=True)
    again = task()
    plan()
    assert np.array_equal(first, again)
    print(f'modules {modules} {bt.hip.rtc_info()["modules"]}', flush=True)


def run_child(kind, shape):
    """The child of one shape in a fresh process: its CompletedProcess."""
    cmd = [sys.executable, os.path.abspath(__file__), 'child', kind] + [str(v) for v in shape]
    return subprocess.run(cmd, env=dict(os.environ, BBT_RTC_VERBOSE='1'), capture_output=True, text=True,
                          timeout=CHILD_TIMEOUT)


def record(path):
    sys.path.insert(0, ROOT)
    import baseband_tasks_amd as bt
    out = {'source': 'tools/tune_candidates.py record: the candidate lines BBT_RTC_VERBOSE=1 printed on an %s, one '
                     'fresh process per shape, with the library before the rules moved to csrc/chan_geo.hpp and '
                     'csrc/pfb_geo.hpp (a candidate equal to an earlier one was then compiled, not timed, and not '
                     'printed); times stripped' % bt.hip.device_name(),
           'channelize': [], 'filter_bank': []}
    for kind, shapes in SHAPES.items():
        for shape in shapes:
            done = run_child(kind, shape)
            print(kind, shape, 'exit', done.returncode, done.stdout.strip().splitlines()[-2:], flush=True)
            if done.returncode != 0:        # (nothing more on the device after a child that ended abnormally)
                sys.stderr.write(done.stderr[-3000:])
                return 1
            before, _, after = done.stderr.partition(MARK)
            assert parse(after) == ([], []), after[-2000:]
            out[kind].append({'shape': list(shape), 'candidates': candidates(before, kind, shape)})
    write(out, path)
    print(json.dumps(out))
    return 0


def write(out, path):
    """One line per shape."""
    kinds = [' "%s": [\n%s\n ]' % (kind, ',\n'.join('  ' + json.dumps(entry) for entry in out[kind])) for kind in SHAPES]
    with open(path, 'w') as f:
        f.write('{\n "source": %s,\n%s\n}\n' % (json.dumps(out['source']), ',\n'.join(kinds)))


if __name__ == '__main__':
    if sys.argv[1:2] == ['child']:
        child(sys.argv[2], tuple(int(v) for v in sys.argv[3:]))
    elif sys.argv[1:2] == ['record']:
        sys.exit(record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN))
    else:
        sys.exit(__doc__)
