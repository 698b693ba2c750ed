"""The kernel launches of one execute call of an overlap-save plan, case by case: the record
tests/golden/osm_launches.json, which tests/test_osm_launches.py holds csrc/osm_launch.hpp to (dev tool).

    python tools/osm_launch_cases.py record <dir> <out.json>   trace every setting and write the record
    python tools/osm_launch_cases.py read <dir> <out.json>     the record from the databases already in <dir>
    python tools/osm_launch_cases.py run <setting>             the cases of one setting (what `record` traces)

`record` starts one `rocprofv3 --kernel-trace` child per environment setting (this process never touches
the GPU) and reads their rocpd databases with tools/rocprof_db.py's name rule.  Before every case the
child launches one k_chirp of (case number + 1) workgroups: the delimiter the launches are cut at.  A trace
does not show events: after which launches of a chunk the timing events 1 and 2 fall (`marks`) is read
from the code path, as are the chunks (blocks, regular count) a call is cut into.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]

#: setting -> the environment of its child
SETTINGS = {'default': {}, 'rtc0': {'BBT_RTC': '0'}, 'mid32': {'BBT_OSM_MID_MIB': '32'}}
#: the kernels of a chunk (everything else -- the delimiter, the seam pass -- is left out)
FAMILIES = ('k_osm_col16', 'k_osm_col256', 'k_osm_rowpass', 'k_osm_mid16', 'k_osm_small', 'k_osm_small_big',
            'k_gen_osm_small', 'k_gen_col', 'k_gen_row', 'k_small', 'k_first', 'k_row', 'k_last')


def case(n_fft, n_stream, chunks=((1, 0),), how='execute', n_chan=0, det=0, in_plane=0, timing=0, marks=None,
         setting='default'):
    """chunks: (blocks, regular count) of every chunk launch of the call; marks: per chunk, after which
    of its launches (counted from 1) timing events 1 and 2 are recorded."""
    return dict(n_fft=n_fft, n_stream=n_stream, chunks=[list(c) for c in chunks], how=how, n_chan=n_chan,
                det=det, in_plane=in_plane, timing=timing, marks=marks, setting=setting)


CASES = (
    # one kernel
    [case(256, s) for s in (1, 2, 4, 8, 16)]
    + [case(1024, 16), case(4096, 6), case(4096, 16), case(8192, 1), case(8192, 2), case(16384, 2),
       case(4096, 2, chunks=[(1, 40)], how='regular')]
    # two levels, 16 columns
    + [case(8192, 16), case(32768, 1), case(32768, 2), case(32768, 16),
       case(32768, 2, n_chan=4), case(32768, 2, n_chan=256), case(32768, 16, n_chan=256),
       case(32768, 1, n_chan=256), case(8192, 16, chunks=[(40, 40)])]
    # two levels, 256 columns
    + [case(2**17, s) for s in (1, 2, 8, 16, 24)]
    + [case(2**17, 4, in_plane=1), case(2**17, 2, n_chan=4), case(2**17, 2, n_chan=16),
       case(2**17, 2, n_chan=256), case(2**17, 2, n_chan=256, det=16), case(2**20, 2, chunks=[(6, 0), (1, 0)])]
    # 512 / 1024 columns
    + [case(2**21, 1), case(2**21, 2), case(2**22, 2)]
    # three levels
    + [case(2**22, 16), case(2**23, 2), case(2**23, 2, n_chan=16), case(2**23, 2, n_chan=256),
       case(2**23, 2, setting='mid32')]
    # generic: compiled, and on the general kernels
    + [case(n, 2, setting=s) for s in ('default', 'rtc0') for n in (6174, 10206, 1666980)]
    # timing on (mode 1)
    + [case(4096, 2, timing=1, marks=[[1, 1]]), case(2**20, 2, timing=1, marks=[[1, 2]]),
       case(2**23, 2, timing=1, marks=[[2, 3]])])


def run(setting):
    import numpy as np
    import baseband_tasks_amd as bt
    hip = bt.hip
    hip.set_device(0)
    for number, c in enumerate(CASES):
        if c['setting'] != setting:
            continue
        n, S = c['n_fft'], c['n_stream']
        nblk = sum(max(b, r) for b, r in c['chunks'])
        pad = n // 8
        keep = n - 2 * pad
        n_in = (nblk - 1) * keep + n
        plan = hip.OsmPlan(n, S, np.ones((1, n), np.complex64))
        x = hip.DeviceArray((n_in, S), np.complex64)
        x.fill_bytes(0)
        y = hip.DeviceArray((n_in, S), np.complex64)
        if c['in_plane']:
            plan.set_layout(in_plane=n_in)
        if c['timing']:
            plan.timing_enable(c['timing'])
        off = np.arange(nblk) * keep
        desc = (off, off, np.full(nblk, pad), np.full(nblk, keep))
        hip.synchronize()
        hip.chirp(256 * (number + 1), [1e9], [1.], [1e9], 1e6, 1.)          # the delimiter
        if c['how'] == 'regular':
            plan.execute_regular(x, y, nblk, 0, 0, keep, pad)
        elif c['det']:
            n_bins = nblk * keep // c['n_chan'] // c['det']
            plan.execute_channelized_detect(x, y, *desc, c['n_chan'], 0, n_bins, c['det'], 1)
        elif c['n_chan']:
            plan.execute_channelized(x, y, *desc, c['n_chan'], 0, nblk * keep // c['n_chan'])
        else:
            plan.execute(x, y, *desc)
        hip.synchronize()
        print('CASE', number, n, S, flush=True)
        plan.close()
        del x, y


def launches_of(db):
    """[(case number of a delimiter or None, launch)] in the order the kernels were enqueued."""
    import sqlite3
    from rocprof_db import short
    con = sqlite3.connect(db)
    con.row_factory = sqlite3.Row
    rows = con.execute('select S.display_name as name, S.group_segment_size as lds_static, K.* '
                       'from rocpd_kernel_dispatch K join rocpd_info_kernel_symbol S '
                       'on S.id = K.kernel_id and S.guid = K.guid order by K.dispatch_id').fetchall()
    out = []
    for r in rows:
        s = short(r['name'])
        if not s:
            continue
        base, _, targs = s.partition('<')
        wg = [r['workgroup_size_x'], r['workgroup_size_y'], r['workgroup_size_z']]
        grid = [r['grid_size_x'] // wg[0], r['grid_size_y'] // wg[1], r['grid_size_z'] // wg[2]]
        if base == 'k_chirp':
            out.append((grid[0] - 1, None))
        elif base in FAMILIES:
            out.append((None, dict(kernel=base, targs=[a.strip() for a in targs.rstrip('>').split(',')] if targs else [],
                                   grid=grid[:2], threads=wg[0], lds=r['group_segment_size'] - r['lds_static'])))
    return out


def read(where, out_json):
    import glob
    record = []
    for setting in SETTINGS:
        dbs = sorted(glob.glob(os.path.join(where, setting, '**', '*.db'), recursive=True))
        assert len(dbs) == 1, (setting, dbs)
        cut = {}
        number = None
        for delim, launch in launches_of(dbs[0]):
            if delim is not None:
                number = delim
                cut[number] = []
            else:
                cut[number].append(launch)
        assert sorted(cut) == [i for i, c in enumerate(CASES) if c['setting'] == setting], (setting, sorted(cut))
        record += [(i, dict(CASES[i], launches=launches)) for i, launches in cut.items()]
    record = [r for _, r in sorted(record, key=lambda ir: ir[0])]
    with open(out_json, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(r) for r in record) + '\n]\n')
    print(len(record), 'cases,', sum(len(r['launches']) for r in record), 'launches ->', out_json)


def record(where, out_json):
    for setting, env in SETTINGS.items():
        cmd = ['rocprofv3', '--kernel-trace', '-f', 'rocpd', '-d', os.path.join(where, setting), '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), 'run', setting]
        print(' '.join(cmd), flush=True)
        subprocess.run(cmd, env=dict(os.environ, **env), check=True, timeout=300)
    read(where, out_json)


if __name__ == '__main__':
    {'run': run, 'read': read, 'record': record}[sys.argv[1]](*sys.argv[2:])
