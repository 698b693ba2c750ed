"""What an overlap-save plan decides every time it runs a chunk (csrc/osm_launch.hpp: the kernel launches,
their instantiations, grids, workgroup sizes, dynamic LDS and timing marks), without a GPU:
tests/gen2_plan_dump.cpp prints the list.  tests/golden/osm_launches.json holds the launches of one
execute call per case as `rocprofv3 --kernel-trace` saw them on an MI355X for the library before the
launch code moved out of bbt_hip.hip (tools/osm_launch_cases.py retakes it)."""
import json
import os
import subprocess

import pytest

from geo_check import PIPES, compile_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'osm_launches.json')) as f:
    RECORDS = json.load(f)
KIB = 1024


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    exe = compile_check('gen2_plan_dump', tmp_path_factory.mktemp('osm_launches'))

    def run(*args):
        out = subprocess.run([exe] + [str(int(a)) if isinstance(a, bool) else str(a) for a in args], **PIPES)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        return [json.loads(line) for line in out.stdout.splitlines()]
    return run


def words(n_fft, n_stream, nblk, reg_count=0, n_chan=0, det=0, in_plane=0, timing=0, mid_mib=128):
    return [n_fft, n_stream, nblk, reg_count, n_chan, det, in_plane, timing, mid_mib]


def marks(launches):
    """After which launches (counted from 1) timing events 1 and 2 fall."""
    return [[i + 1 for i, l in enumerate(launches) if l['mark'] & bit] for bit in (1, 2)]


def test_the_recorded_launches_are_reproduced(dump):
    assert len(RECORDS) == 49
    seen = set()
    for r in RECORDS:
        rtc = 0 if r['setting'] == 'rtc0' else 1
        mid = 32 if r['setting'] == 'mid32' else 128
        got = dump('launches', rtc, *sum((words(r['n_fft'], r['n_stream'], nblk, reg, r['n_chan'], r['det'], r['in_plane'],
                                                r['timing'], mid) for nblk, reg in r['chunks']), []))
        assert len(got) == len(r['chunks']) and not any('error' in g for g in got), (r, got)
        launches = sum((g['launches'] for g in got), [])
        assert [{k: l[k] for k in ('kernel', 'targs', 'grid', 'threads', 'lds')} for l in launches] == r['launches'], r
        if r['marks']:
            assert [[a, b] for (a,), (b,) in map(marks, (g['launches'] for g in got))] == r['marks'], r
        seen |= {(l['kernel'],) + tuple(l['targs']) for l in launches}
    # every route was taken: each family, and the arms of the column passes
    assert {s[0] for s in seen} == {'k_osm_col16', 'k_osm_col256', 'k_osm_rowpass', 'k_osm_mid16', 'k_osm_small',
                                    'k_osm_small_big', 'k_gen_osm_small', 'k_gen_col', 'k_gen_row', 'k_small',
                                    'k_first', 'k_row', 'k_last'}
    assert len({s for s in seen if s[0] == 'k_osm_col256'}) >= 16 and len({s for s in seen if s[0] == 'k_osm_col16'}) == 9


def test_every_power_of_two_plan_launches_within_bounds(dump):
    plans = [(1 << e, s) for e in range(8, 25) for s in (1, 2, 4, 16, 128, 510, 2048)]
    geo = dump('osm', 1, *sum((list(c) for c in plans), []))
    cases = [(n, s, nblk, n_chan, timing)
             for (n, s), g in zip(plans, geo) if 'error' not in g
             for nblk in sorted({1, g['chunk']}) for n_chan in [0] + [2 << i for i in range(12)] for timing in (0, 1)]
    got = dump('launches', 1, *sum((words(n, s, nblk, n_chan=n_chan, timing=timing) for n, s, nblk, n_chan, timing in cases), []))
    assert len(got) == len(cases) > 3000
    fused = pieces = 0
    for (n, s, nblk, n_chan, timing), g in zip(cases, got):
        if n_chan and not g.get('fusable'):
            continue
        what = (n, s, nblk, n_chan, timing)
        assert 'error' not in g, (what, g)
        fused += n_chan != 0
        ls = g['launches']
        pairs = (nblk + 1) // 2 if s == 1 else nblk          # one stream: the work buffer holds pairs of blocks
        for l in ls:
            assert 1 <= l['grid'][0] < 2**31 and 1 <= l['grid'][1] <= 65535 and 16 <= l['threads'] <= 1024, (what, l)
            assert l['lds'] <= 160 * KIB and (l['raise_lds'] or l['lds'] <= 64 * KIB), (what, l)
        mids = [l for l in ls if l['kernel'] == 'k_osm_mid16' and l['targs'] == ['true']]
        if len(mids) <= 1:          # (as under timing: the passes one after the other)
            (a,), (b,) = marks(ls)
            assert a <= b and (a < b) == (g['n1'] > 1), (what, ls)
        else:
            assert not timing
            pieces += 1
        rows = [l for l in ls if l['kernel'] == 'k_osm_rowpass']
        if g['outer'] > 1:
            assert [l['kernel'] for l in ls] == ['k_osm_col256'] + ['k_osm_mid16', 'k_osm_rowpass', 'k_osm_mid16'] * len(mids) + ['k_osm_col256']
            for part in (mids, rows, [l for l in ls if l['kernel'] == 'k_osm_mid16' and l['targs'] == ['false']]):
                assert [l['y0'] for l in part] == [sum(m['ny'] for m in part[:i]) for i in range(len(part))], (what, part)
                assert sum(l['ny'] for l in part) == pairs * g['npair'] * 256, (what, part)
                assert all(l['grid'][1] == l['ny'] for l in part)
        elif g['n1'] > 1:
            row, = rows
            assert row['grid'] in ([g['n1'] * pairs * g['npair'], 1], [g['n1'], pairs * g['npair']]), (what, row)
    assert fused > 1000 and pieces > 20


def test_refusals_keep_their_texts(dump):
    generic = 'osm: the fused channelizer needs a power-of-two block length'
    cases = [(1, words(2**21, 2, 1, n_chan=256, det=1), 'osm: fused detection needs 256-point columns'),
             (1, words(2**22, 2, 1, n_chan=256, det=1), 'osm: fused detection needs 256-point columns'),
             (1, words(2**17, 1, 1, n_chan=256, det=1), 'osm: one-stream plans have no fused detection'),
             (1, words(2**23, 1, 1, n_chan=256, det=1), 'osm: one-stream plans have no fused detection'),
             (1, words(6174, 2, 1, n_chan=256), generic), (0, words(6174, 2, 1, n_chan=256), generic),
             (1, words(1666980, 2, 1, n_chan=16), generic), (0, words(1666980, 2, 1, n_chan=16), generic)]
    for rtc, case, text in cases:
        got, = dump('launches', rtc, *case)
        assert got == dict(error=text), (case, got)
    # ... and the same plans without what was refused
    for rtc, case, _ in cases:
        got, = dump('launches', rtc, *(case[:4] + [0, 0] + case[6:]))
        assert 'error' not in got and got['launches']
