"""What the two kinds of plan that time candidate kernels decide without a device: channelizer
plans of channel counts that are not powers of two (csrc/chan_geo.hpp) and filter-bank plans on
many streams (csrc/pfb_geo.hpp) -- argument checks, candidate lists, forced routes, tap permutation.
tests/gen2_plan_dump.cpp prints them; the tool is built a second time with the address and
undefined-behaviour sanitizers and every case here runs through both builds.
tests/golden/tune_candidates.json holds the candidates the library itself listed on an MI355X
before these rules moved out of bbt_hip.hip (tools/tune_candidates.py);
tests/test_tune_geo_gpu.py holds the library to the same record."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gen2_planner import dump, CSRC  # noqa: F401  (the fixture that builds the tool)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import tune_candidates  # noqa: E402

with open(tune_candidates.GOLDEN) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope='module')
def dumps(dump, tmp_path_factory):
    """The tool as the other tests use it, and built with sanitizers: both answer every call."""
    exe = str(tmp_path_factory.mktemp('gen2_san') / 'gen2_plan_dump')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I', CSRC, os.path.join(ROOT, 'tests', 'gen2_plan_dump.cpp'), '-o', exe])

    def run(*args):
        plain = dump(*args)
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr[-3000:]
        assert [json.loads(line) for line in out.stdout.splitlines()] == plain
        return plain
    run.exe = dump.exe
    return run


def listed(g):
    """code: pairs x transforms per workgroup, threads"""
    return [(c['code'], c['cp'], c['plan']['ct'] // c['cp'], c['plan']['threads']) for c in g['candidates']]


# -- channelizer ----------------------------------------------------------------------------------
CHAN = {(6, 2): [(10, 1, 64, 64)],
        (14, 2): [(10, 1, 32, 64), (16, 1, 64, 64)],
        (30, 2): [(10, 1, 16, 64), (16, 1, 16, 64), (20, 1, 32, 64)],
        (360, 16): [(10, 4, 1, 192), (16, 8, 1, 256), (20, 8, 1, 192), (110, 8, 1, 384)],
        (1000, 2): [(10, 1, 1, 128), (20, 1, 1, 64)],
        (1000, 24): [(10, 2, 1, 256), (20, 4, 1, 256), (110, 4, 1, 448)],
        (3000, 8): [(10, 1, 1, 384), (16, 1, 1, 256), (20, 1, 1, 192), (110, 2, 1, 704), (116, 4, 1, 832), (120, 4, 1, 704)],
        (6174, 2): [(10, 1, 1, 896), (16, 1, 1, 704), (20, 1, 1, 448)],
        # (what the rule lists on its own: the product runs 8192 channels on the `big` kernels)
        (8192, 2): [(10, 1, 1, 1024), (16, 1, 1, 512)]}


def test_channelizer_candidates(dumps):
    got = dumps('chan', *sum((list(k) for k in CHAN), []))
    assert len(got) == len(CHAN)
    for (key, want), g in zip(CHAN.items(), got):
        assert (g['n_chan'], g['n_stream']) == key and listed(g) == want, (key, listed(g))
        assert g['kind'] == ('big' if key[0] == 8192 else 'generic')
        assert not g['single'] and not g['split_real'] and g['direction'] == -1
        # timed by default; BBT_G2_TUNE=0: 10 points, wide only with BBT_G2_CHAN_WIDE; a remembered choice as it is
        assert g['untimed'] == [-1, 10, 110, 116]


def test_channelizer_candidates_are_the_recorded_ones(dumps):
    recs = GOLDEN['channelize']
    assert [tuple(r['shape']) for r in recs] == tune_candidates.SHAPES['channelize']
    got = dumps('chan', *sum((r['shape'] for r in recs), []))
    for r, g in zip(recs, got):
        # (the library prints points per thread, pairs and transforms per workgroup)
        assert [[code % 100, cp, bt] for code, cp, bt, _ in listed(g)] == r['candidates'], (r, listed(g))


def smooth7(limit):
    return sorted(a * b * c * d for a in (2**i for i in range(14)) for b in (3**i for i in range(9))
                  for c in (5**i for i in range(6)) for d in (7**i for i in range(5)) if 2 <= a * b * c * d <= limit)


def test_every_channelizer_candidate_list_is_consistent(dumps):
    lengths = smooth7(8192)
    assert len(lengths) > 300 and lengths[-1] == 8192
    for n_stream in (2, 8, 16):
        got = dumps('chan', *sum(([n, n_stream] for n in lengths), []))
        assert len(got) == len(lengths)
        for n, g in zip(lengths, got):
            power_of_two = n & (n - 1) == 0
            assert g['kind'] == ('generic' if not power_of_two else 'big' if n == 8192 else 'rows' if n >= 256 else 'short')
            assert bool(g['candidates']) == (not power_of_two or n == 8192), (n, n_stream, g)
            npair = n_stream // 2
            plans = []
            for c in g['candidates']:
                q = c['plan']
                assert q['n'] == n and q['threads'] <= 1024 and q['tj'] * q['ct'] <= q['threads'], (n, n_stream, c)
                assert npair % c['cp'] == 0 and c['cp'] <= 8 and q['ct'] % c['cp'] == 0, (n, n_stream, c)
                assert (c['code'] >= 100) <= (npair >= 4) and c['code'] % 100 in (10, 16, 20)
                assert max(q['fac']) <= c['code'] % 100 and int(np.prod(q['fac'])) == n
                plans.append((q['fac'], q['tj'], q['ct']))
            assert all(a != b for i, a in enumerate(plans) for b in plans[:i]), (n, n_stream, plans)
            assert [c['code'] for c in g['candidates']] == sorted(c['code'] for c in g['candidates'])


def test_channelizer_candidate_source(dumps):
    """A candidate of one transform per workgroup and 20 points per thread is the overlap-save
    plan's row transform of that length: the same traits, the same entry point."""
    for n, hint in ((1000, 0), (3000, 0), (6174, 4)):
        g, = dumps('chan', n, 2)
        c, = [c for c in g['candidates'] if c['code'] == 20]
        assert c['plan']['ct'] == 1 and (c['plan']['threads'] >= 448) == (hint == 4)
        osm = subprocess.check_output([dumps.exe, 'source', str(n)], text=True).splitlines()
        trait, = [line for line in osm if line.startswith('BBT_G2_TRAIT(GA, ')]
        rows, = [line for line in osm if line.startswith('BBT_G2_KERNEL_FFT_ROWS(k_rows, ')]
        assert rows == 'BBT_G2_KERNEL_FFT_ROWS(k_rows, GA, -1, 0)'
        assert c['source'].splitlines() == [osm[0], trait, rows.replace(', 0)', ', %d)' % hint)]
        assert osm[0] == '#include "gen2_kernels.hpp"' and c['source'].endswith('\n')
    # the inverse
    back, = dumps('chan', 'dir=1', 1000, 2)
    assert [c['source'].splitlines()[-1] for c in back['candidates']] == ['BBT_G2_KERNEL_FFT_ROWS(k_rows, GA, +1, 0)'] * 2


def test_channelizer_refusals_keep_their_texts(dumps):
    def n_chan_text(n):
        return (f'bbt_chan_plan_create: n_chan={n} must be a power of two in [2, 16384] (above 4096: stream '
                'pairs, directions -1 / +1) or a product of 2, 3, 5, 7 up to 8192')

    def n_stream_text(s):
        return (f'bbt_chan_plan_create: n_stream={s} must be even and >= 2 (or 1 for a power-of-two n_chan '
                'in [256, 4096])')
    cases = [((n, 2), n_chan_text(n)) for n in (1, 0, -8, 11, 8192 * 3, 32768, 8400)]
    cases += [((n, s), n_stream_text(s)) for n in (14, 1024) for s in (3, 5, 0, -2, 131072)]
    cases += [((n, 1), n_stream_text(1)) for n in (14, 128, 6174, 8192)]
    cases += [((16384, 1), n_chan_text(16384)), ((16384, 3), n_chan_text(16384))]
    got = dumps('chan', *sum((list(c) for c, _ in cases), []))
    assert [g.get('error') for g in got] == [text for _, text in cases]
    # ... and what lies just inside
    got = dumps('chan', 2, 2, 128, 2, 256, 1, 4096, 1, 4096, 131070, 8192, 2, 16384, 2, 8100, 2)
    assert [g.get('error') for g in got] == [None] * 8
    assert [g['kind'] for g in got] == ['short', 'short', 'rows', 'rows', 'rows', 'big', 'big', 'generic']
    assert [g['single'] for g in got] == [False, False, True, True, False, False, False, False]


def test_channelizer_directions(dumps):
    split = 'bbt_chan_plan_create: direction -2 / +2 needs a power-of-two n_chan in [256, 4096]'
    for d in (-2, 2):
        got = dumps('chan', f'dir={d}', 1000, 2, 6174, 2, 128, 2, 256, 2, 4096, 1, 8192, 2, 16384, 2)
        assert [g.get('error') for g in got[:3]] == [split] * 3
        assert [(g['kind'], g['split_real'], g['direction'], g['single']) for g in got[3:5]] == [
            ('rows', True, d // 2, False), ('rows', True, d // 2, True)]
        # (the `big` kernels take the plain directions only: 8192 is then a generic length, 16384 none at all)
        assert got[5].get('error') == split
        assert got[6].get('error', '').startswith('bbt_chan_plan_create: n_chan=16384 must be a power of two in [2, 16384]')
    for d in (0, 3, -3):
        got = dumps('chan', f'dir={d}', 1000, 2, 1024, 2)
        assert [g.get('error') for g in got] == ['bbt_chan_plan_create: direction must be -1, +1, -2 or +2'] * 2
    got = dumps('chan', 'dir=1', 8192, 2, 16384, 2, 8192, 1, 16384, 1)
    assert [g.get('kind') for g in got] == ['big', 'big', None, None] and got[0]['direction'] == 1


# -- filter bank ----------------------------------------------------------------------------------
TWO, ONE = [0, 0], [1, 0]
PFB = {(4, 1024, 32): (True, TWO, [TWO, [4, 0], [4, 4], [8, 0], [8, 1]]),
       (12, 256, 8): (True, ONE, [TWO, ONE, [4, 0]]),
       (8, 2048, 16): (True, TWO, [TWO, [4, 0]]),             # (geometry 4096: no eights)
       (16, 4096, 16): (False, TWO, []),                      # no window kernel; the rule
       (5, 1024, 32): (False, ONE, []),                       # k_pfb: two passes need 4, 8, 12 or 16 taps
       (4, 1024, 6): (False, ONE, []),                        # fewer than 8 streams
       (8, 4096, 2): (False, TWO, [])}                        # no window kernel, 8 taps


def route(g):
    return g['timed'], g['fixed'], g['candidates']


def test_filter_bank_routes(dumps):
    got = dumps('pfb', '-', *sum((list(k) for k in PFB), []))
    for (key, want), g in zip(PFB.items(), got):
        assert route(g) == want, (key, g)
    assert [g['gn'] for g in got] == [2048, 2048, 4096, 4096, 4096, 4096, 4096]
    assert [g['window'] for g in got] == [True, True, True, False, False, True, False]
    assert [g['pp_ok'] for g in got] == [True, True, True, False, False, False, False]


def test_filter_bank_routes_are_the_recorded_ones(dumps):
    recs = GOLDEN['filter_bank']
    assert [tuple(r['shape']) for r in recs] == tune_candidates.SHAPES['filter_bank']
    got = dumps('pfb', '-', *sum((r['shape'] for r in recs), []))
    for r, g in zip(recs, got):
        assert g['timed'] and g['candidates'] == r['candidates'], (r, g)


def test_filter_bank_switches(dumps):
    def one(knobs, *shape):
        g, = dumps('pfb', knobs, *shape)
        return route(g)
    timed = PFB[4, 1024, 32]
    for knobs, want in (('tune=0', (False, TWO, [])), ('two=1', (False, TWO, [])), ('two=0', (False, ONE, [])),
                        ('pp=4', (False, [4, 0], [])), ('pp=4,gl=4', (False, [4, 4], [])), ('pp=4,gl=2', (False, [4, 2], [])),
                        ('pp=4,gl=3', (False, [4, 0], [])),       # 4 pair groups: an order of 3 is order 0
                        ('pp=4,gl=-1', (False, [4, 0], [])),
                        ('pp=8', (False, [8, 0], [])), ('pp=8,gl=1', (False, [8, 1], [])), ('pp=8,gl=2', (False, [8, 2], [])),
                        ('pp=8,gl=4', (False, [8, 0], [])), ('pp=8,two=1,tune=0', (False, [8, 0], [])),
                        ('pp=2', timed), ('pp=16', timed), ('pp=0', timed), ('gl=4', timed),
                        ('pp=2,two=0', (False, ONE, [])), ('pp=2,tune=0', (False, TWO, []))):
        assert one(knobs, 4, 1024, 32) == want, knobs
    # eight pairs per workgroup only on the geometry of 2048 and where they divide the pairs: ignored, timed as ever
    assert one('pp=8', 8, 2048, 16) == PFB[8, 2048, 16]
    assert one('pp=8', 4, 1024, 24) == (True, TWO, [TWO, [4, 0]])
    assert one('pp=4', 8, 2048, 16) == (False, [4, 0], [])
    # no several-pairs form: the switch is ignored and the rule decides
    assert one('pp=4', 4, 1024, 6) == (False, ONE, []) and one('pp=4', 16, 4096, 16) == (False, TWO, [])
    # two passes cannot be forced where they do not exist
    assert one('two=1', 5, 1024, 32) == (False, ONE, []) and one('two=1', 4, 1024, -2) == (False, ONE, [])
    assert one('two=1', 4, 1024, 2) == (False, TWO, []) and one('two=0', 16, 4096, 16) == (False, ONE, [])
    # the rule: two passes from 16 streams on, or without a window kernel from 8 taps on
    assert [one('tune=0', 4, 1024, s)[1] for s in (2, 8, 14, 16, 64)] == [ONE, ONE, ONE, TWO, TWO]
    assert [one('-', t, 4096, 2)[1] for t in (4, 8, 12, 16, 20)] == [ONE, TWO, TWO, TWO, ONE]
    # one pair per workgroup is a candidate below 16 streams only; the orders where they divide the pair groups
    assert one('-', 4, 512, 8) == (True, ONE, [TWO, ONE, [4, 0]])
    assert one('-', 4, 512, 16) == (True, TWO, [TWO, [4, 0], [8, 0]])
    assert one('-', 16, 256, 128) == (True, TWO, [TWO, [4, 0], [4, 4], [8, 0], [8, 1]])
    assert one('-', 4, 1024, -32) == (False, ONE, [])          # (pairs of real streams: the window kernel, one pair)


def test_filter_bank_refusals_keep_their_texts(dumps):
    def one_stream(n_tap, n_chan):
        return ('bbt_pfb_plan_create: one stream needs n_chan in 256..2048 and 4, 8, 12 or 16 taps '
                f'(got {n_tap} x {n_chan}); pad to two streams otherwise')
    cases = [((4, n, 2), f'bbt_pfb_plan_create: n_chan={n} must be a power of two in [256, 4096]') for n in (128, 1000, 8192, 0)]
    cases += [((t, 1024, 2), f'bbt_pfb_plan_create: n_tap={t} must be in [1, 64]') for t in (0, -4, 65)]
    # (a negative even count is so many streams made of two real ones each; -1: one)
    cases += [((4, 1024, s), f'bbt_pfb_plan_create: n_stream={s} must be even and >= 2') for s in (0, 3, -3, 131072)]
    cases += [((4, 1024, -131072), 'bbt_pfb_plan_create: n_stream=131072 must be even and >= 2')]
    cases += [((t, n, s), one_stream(t, n)) for t, n in ((4, 4096), (5, 1024), (20, 256)) for s in (1, -1, -2, -16)]
    got = dumps('pfb', '-', *sum((list(c) for c, _ in cases), []))
    assert [g.get('error') for g in got] == [text for _, text in cases]
    got = dumps('pfb', '-', 1, 256, 2, 64, 4096, 131070, 16, 2048, 1, 4, 256, -1, 12, 512, -131070)
    assert [g.get('error') for g in got] == [None] * 5
    assert [(g['streams'], g['split_real']) for g in got] == [(2, False), (131070, False), (1, False), (1, True), (131070, True)]


@pytest.mark.parametrize('n_tap, n_chan, T', [(4, 256, 256), (12, 1024, 256), (8, 2048, 256), (16, 512, 128), (4, 1024, 128)])
def test_tap_quads(dumps, n_tap, n_chan, T):
    """quads[((c * n_tap / 4) + q) * T + tau][k] = h[4 q + k][tau + T c]"""
    got, = dumps('quads', n_tap, n_chan, T)
    h = np.arange(n_tap * n_chan).reshape(n_tap // 4, 4, n_chan // T, T)        # [q][k][c][tau]
    assert np.array_equal(np.array(got), h.transpose(2, 0, 3, 1).ravel())
    assert sorted(got) == list(range(n_tap * n_chan))
