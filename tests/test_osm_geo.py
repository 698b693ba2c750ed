"""What an overlap-save plan decides from the block length and the stream count (csrc/osm_geo.hpp:
levels, lanes, chunk, work buffers, how a regular run is cut into launches), without a GPU:
tests/gen2_plan_dump.cpp prints it with the default knobs.  tests/golden/osm_plan_info.json holds
what `OsmPlan.info()` reported on an MI355X for the library before these rules moved out of
bbt_osm_plan_create (response: ones, one column), with plan-time compilation on and with BBT_RTC=0;
tests/test_osm_geo_gpu.py holds the library to the same records."""
import json
import os

import pytest

from test_gen2_planner import dump  # noqa: F401  (the fixture that builds the tool)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'osm_plan_info.json')) as f:
    RECORDS = json.load(f)
MIB = 1 << 20


def test_the_recorded_plans_are_reproduced(dump):
    assert len(RECORDS) == 29
    for mode, rtc_ok in (('on', 1), ('off', 0)):
        recs = [r for r in RECORDS if r['mode'] == mode]
        got = dump('osm', rtc_ok, *sum(([r['n_fft'], r['n_stream']] for r in recs), []))
        assert len(got) == len(recs) >= 7
        for r, g in zip(recs, got):
            assert dict(workspace_bytes=g['workspace_bytes'], chunk_blocks=g['chunk'], n1=g['n1'], n2=g['n2']) == r['info'], (r, g)


# n_fft, n_stream: outer, n1, n2, lanes, chunk, cap, work_bytes per lane -- by hand from the rules:
# 192 MiB over the lanes, at most 16 descriptors, grid.y <= 65535, twice the blocks for one stream
ANCHORS = {(4096, 2): (1, 1, 4096, 1, 16, 1048576, 0),
           (8192, 16): (1, 16, 512, 2, 16, 96, 96 * MIB),
           (16384, 16): (1, 16, 1024, 2, 16, 48, 96 * MIB),
           (65536, 2): (1, 16, 4096, 2, 16, 96, 96 * MIB),
           (2**20, 2): (1, 256, 4096, 2, 6, 6, 96 * MIB),
           (2**20, 1): (1, 256, 4096, 2, 12, 12, 96 * MIB),
           (2**20, 16): (1, 256, 4096, 2, 1, 1, 128 * MIB),
           (2**21, 2): (1, 512, 4096, 2, 3, 3, 96 * MIB),
           (2**22, 2): (1, 1024, 4096, 2, 1, 1, 64 * MIB),
           (2**22, 16): (256, 16, 1024, 2, 1, 1, 512 * MIB),
           (2**23, 2): (256, 16, 2048, 2, 1, 1, 128 * MIB),
           (2**24, 2): (256, 16, 4096, 2, 1, 1, 256 * MIB),
           (2**24, 16): (256, 16, 4096, 2, 1, 1, 2048 * MIB)}


def test_anchors_of_the_power_of_two_ladder(dump):
    got = dump('osm', 1, *sum((list(k) for k in ANCHORS), []))
    for (key, want), g in zip(ANCHORS.items(), got):
        assert (g['outer'], g['n1'], g['n2'], g['lanes'], g['chunk'], g['cap'], g['work_bytes']) == want, (key, g)
        assert g['workspace_bytes'] == g['work_bytes'] * g['lanes']


TOO_MANY = 'bbt_osm_plan_create: blocks longer than 2^20 support at most 510 streams'


def test_every_power_of_two_plan_is_consistent(dump):
    cases = [(1 << e, s) for e in range(8, 25) for s in (1, 2, 4, 16, 128, 510, 2048)]
    got = dump('osm', 1, *sum((list(c) for c in cases), []))
    assert len(got) == len(cases)
    refused = 0
    for (n, s), g in zip(cases, got):
        npair = 1 if s == 1 else s // 2
        three_level = n > 2**22 or (n == 2**22 and s > 1 and npair % 8 == 0)
        if three_level and s // 2 > 255:
            assert g.get('error') == TOO_MANY, (n, s, g)
            refused += 1
            continue
        assert 'error' not in g, (n, s, g)
        assert g['outer'] * g['n1'] * g['n2'] == n and g['outer'] == (256 if three_level else 1), (n, s, g)
        assert 1 <= g['chunk'] <= 16 and g['cap'] >= g['chunk'], (n, s, g)
        assert 1 <= g['lanes'] <= 8 and g['n2p'] == g['n2']
        assert (g['work_bytes'] == 0 and g['lanes'] == 1) == (g['n1'] == 1), (n, s, g)
        if g['n1'] > 1:
            assert g['chunk'] * npair * g['outer'] <= 65535, (n, s, g)
            # the work buffer holds `cap` blocks of every pair; one stream: cap / 2 pairs of blocks
            assert g['work_bytes'] == (g['cap'] // 2 if s == 1 else g['cap']) * npair * n * 16, (n, s, g)
    assert refused == 3         # 2048 streams on 2^22 (pairs in eights: three levels), 2^23 and 2^24 samples


def test_refusals_keep_their_texts(dump):
    def n_fft_text(n):
        return (f'bbt_osm_plan_create: n_fft={n} must be a power of two in [256, 2^24] or a product of '
                '2, 3, 5, 7 that is <= 8192 or splits into two such factors')

    def n_stream_text(s):
        return (f'bbt_osm_plan_create: n_stream={s} must be even and >= 2 (or 1 with a power-of-two block '
                'length)')
    cases = [((n, 2), n_fft_text(n)) for n in (0, 1, -4, 11, 8192 * 11, 2**27, 20588575)]
    cases += [((4096, s), n_stream_text(s)) for s in (0, -2, 3, 131072)]
    cases += [((6174, 1), n_stream_text(1)), ((1666980, 1), n_stream_text(1))]
    cases += [((n, s), TOO_MANY) for n, s in ((2**22, 512), (2**23, 512), (2**24, 1024), (2**24, 131070))]
    for mode in (0, 1):
        got = dump('osm', mode, *sum((list(c) for c, _ in cases), []))
        assert [g.get('error') for g in got] == [text for _, text in cases]
    # ... and what lies just inside
    got = dump('osm', 1, 2**22, 514, 2**23, 510, 4096, 131070, 2**25, 2, 2, 2)
    assert [g.get('error') for g in got] == [None] * 5
    assert (got[0]['outer'], got[0]['n1']) == (1, 1024) and got[1]['outer'] == 256
    assert (got[3]['n1'], got[3]['n2']) == (4096, 8192)           # (2^25: a generic two-level block)


def test_generic_plans_pad_their_rows_only_on_the_compiled_kernels(dump):
    for n in (6174, 10206, 1666980):
        on, = dump('osm', 1, n, 2)
        failed, = dump('osm', 'failed', n, 2)
        off, = dump('osm', 0, n, 2)
        assert on['n2p'] == -(-on['n2'] // 8) * 8 and failed['n2p'] == failed['n2'] and off['n2p'] == off['n2']
        # (a failed compilation keeps the split and the tile chosen for the compiled kernels)
        assert (failed['n1'], failed['n2'], failed['gen_ct']) == (on['n1'], on['n2'], on['gen_ct'])
        if on['n1'] > 1:
            assert on['work_bytes'] == on['cap'] * on['n1'] * on['n2p'] * 16
            assert failed['work_bytes'] == failed['cap'] * n * 16


def test_regular_runs_are_cut_into_equal_launches(dump):
    assert dump('parts', 1000, 16, 96, 2, 1, 64, 16, 96, 2, 1, 40, 16, 96, 2, 1) == [
        dict(parts=11, per=91), dict(parts=2, per=32), dict(parts=1, per=40)]
    cases = [(run, chunk, cap, lanes, fork)
             for chunk, cap, lanes in ((16, 96, 2), (16, 48, 2), (6, 7, 2), (12, 12, 2), (3, 5, 4), (16, 202, 1), (1, 2, 8))
             for fork in (0, 1) for run in list(range(chunk + 1, 6 * cap + 2)) + [4096, 65535]]
    got = dump('parts', *sum((list(c) for c in cases), []))
    assert len(got) == len(cases)
    for (run, chunk, cap, lanes, fork), g in zip(cases, got):
        parts, per = g['parts'], g['per']
        assert parts * per >= run > (parts - 1) * per and 1 <= per <= cap, (run, chunk, cap, lanes, fork, g)
        fewest = -(-run // cap)
        if fork and fewest < lanes and run >= 2 * lanes * chunk:
            assert parts == lanes
        else:
            assert parts == fewest
