"""`FFASearch` on a resident standardized (time, DM) plane against two yardsticks from the same run, one JSON
line per row (dev tool; needs a GPU).

    python tools/bench_ffa.py [--out FILE] [--reps N] [--no-cpu] [row ...]

Rows: float32 noise planes of (2^18, 512) and (2^20, 64), resident in HBM, each searched as one block at the
base periods 256 ... 511 with 6 widths.  The `*_fuse1`, `*_fuse2` and `*_fuse3` rows are the same search under
BBT_FFA_FUSE = 1, 2, 3, taking turns (the row list interleaves them `--turns` times; every run is a line of its
own).  Every row runs in a child process of its own under a time limit, and the first row that fails ends the
run.

Timed with device events around ``read_device()`` of the whole result (the cache dropped before every
repeat): 2 warm-up reads, then ``--reps`` timed ones; the minimum and the median are reported.

  `copy_ms`: a device-to-device copy of the plane's bytes.
  `cpu_s`: `ffa.ffa_search_samples` on `cpu_columns` columns of the same plane, every base period, the base
      periods dealt to 16 worker processes; `cpu_plane_s` is that scaled to all columns.  Measured by the
      parent, which never opens the GPU, before the rows run.
  `adds`: float32 adds of the rule, per base period and column M p log2(M) for the fold stages plus M p (K - 1)
      for the boxcar levels; `gadds_per_s` is that over the best read.

The split between the fold passes and the S/N pass is not taken here: `bash tools/gpu_job.sh ffa` runs one row
under a kernel trace and tools/rocprof_db.py sums the kernels."""
import json
import os
import sys
import time

import bench_rows
from bench_rows import events_ms, reread

sys.path.insert(0, bench_rows.ROOT)

PERIODS, K = (256, 512), 6
SHAPES = {'n18_d512': dict(n=1 << 18, ndm=512), 'n20_d64': dict(n=1 << 20, ndm=64)}
ROWS = {}
for _name, _shape in SHAPES.items():
    ROWS[_name] = dict(_shape, yardsticks=True)
    for _f in (1, 2, 3):
        ROWS[f'{_name}_fuse{_f}'] = dict(_shape, env=dict(BBT_FFA_FUSE=_f))
ROW_LIMIT = 300          # seconds a row may take
RATE = 1e4
BUDGET = 1 << 32         # bytes: every column and base period of a block in one launch
CPU_COLUMNS, CPU_WORKERS = 2, 16


def plane(n, ndm):
    import numpy as np
    return np.random.default_rng(7).standard_normal((n, ndm), dtype=np.float32)


def adds(n, ndm):
    from baseband_tasks_amd import ffa
    total = 0
    for p in range(*PERIODS):
        m, M = ffa.ffa_rows(n, p)
        total += M * p * ((M.bit_length() - 1) + K - 1)
    return total * ndm


def _cpu_part(args):
    from baseband_tasks_amd import ffa
    n, ndm, pa, pb = args
    x = plane(n, CPU_COLUMNS)                                   # (noise like the plane's; only the time matters)
    t0 = time.perf_counter()
    ffa.ffa_search_samples(x, n, (pa, pb), K)
    return time.perf_counter() - t0


def cpu_seconds(n, ndm):
    """Wall seconds of the twin on CPU_COLUMNS columns with the base periods dealt to CPU_WORKERS processes."""
    import multiprocessing
    edges = [PERIODS[0] + (PERIODS[1] - PERIODS[0]) * i // CPU_WORKERS for i in range(CPU_WORKERS + 1)]
    parts = [(n, ndm, a, b) for a, b in zip(edges[:-1], edges[1:]) if a < b]
    with multiprocessing.get_context('spawn').Pool(CPU_WORKERS) as pool:
        pool.map(_cpu_part, parts[:1])                          # (start the workers, import the package)
        t0 = time.perf_counter()
        pool.map(_cpu_part, parts, chunksize=1)
        return time.perf_counter() - t0


def run_row(name, reps):
    import numpy as np
    import baseband_tasks_amd as bt
    from baseband_tasks_amd import hip
    row = ROWS[name]
    n, ndm = row['n'], row['ndm']
    for key, value in row.get('env', {}).items():
        os.environ[key] = str(value)
    bt.hip.set_device(0)
    stream = bt.DeviceStream(plane(n, ndm), bt.Time('2020-01-01T00:00:00'), RATE, samples_per_frame=n)
    info = hip.ffa_info()
    line = dict(row=name, device=hip.device_name(), n=n, ndm=ndm, periods=list(PERIODS), n_widths=K, reps=reps,
                plane_bytes=n * ndm * 4, fuse=info['fuse'], width=info['width'], budget=BUDGET, adds=adds(n, ndm))
    fs = bt.FFASearch(stream, n, PERIODS, K)
    fs.ffa_budget = BUDGET
    line['launches'] = len(fs._chunks())
    times = events_ms(lambda: reread(fs), 2, reps)
    line['ffa_ms_min'], line['ffa_ms_med'] = round(min(times), 3), round(float(np.median(times)), 3)
    line['gadds_per_s'] = round(line['adds'] / min(times) / 1e6, 1)
    line['scratch_bytes'] = fs._plan.info()['scratch_bytes']
    fs.close()
    if row.get('yardsticks'):
        words = n * ndm
        src, dst = hip.DeviceArray((words,), np.float32), hip.DeviceArray((words,), np.float32)
        hip.check(hip.lib().bbt_memset(src.ptr, 0, src.nbytes, None))
        c = events_ms(lambda: dst.copy_from_device(src), 2, reps)
        line.update(copy_ms=round(min(c), 3), copy_ms_med=round(float(np.median(c)), 3))
        line['ffa_over_copy'] = round(line['ffa_ms_min'] / line['copy_ms'], 1)
    return line


def main():
    ap = bench_rows.parser(__doc__, 'ffa_bench.jsonl', [])
    ap.add_argument('--turns', type=int, default=2, help='how often the fuse rows of a shape take turns')
    ap.add_argument('--no-cpu', action='store_true', help='skip the NumPy twin on the CPU')
    args = ap.parse_args()
    if args.child:
        print(json.dumps(run_row(args.rows[0], args.reps)), flush=True)
        return 0
    rows = args.rows
    if not rows:
        for shape in SHAPES:
            rows += [shape] + [f'{shape}_fuse{f}' for _ in range(args.turns) for f in (1, 2, 3)]
    bench_rows.check_rows(ap, rows, ROWS)
    cpu = {}
    if not args.no_cpu:
        for name in rows:
            if ROWS[name].get('yardsticks') and name not in cpu:
                n, ndm = ROWS[name]['n'], ROWS[name]['ndm']
                seconds = cpu_seconds(n, ndm)
                cpu[name] = dict(cpu_s=round(seconds, 2), cpu_columns=CPU_COLUMNS, cpu_workers=CPU_WORKERS,
                                 cpu_plane_s=round(seconds * ndm / CPU_COLUMNS, 1))
                print(f'{name}: twin on {CPU_COLUMNS} columns: {seconds:.2f} s', file=sys.stderr, flush=True)

    def with_twin(name, line):
        if name in cpu:
            line.update(cpu[name])
            line['cpu_plane_over_ffa'] = round(line['cpu_plane_s'] * 1e3 / line['ffa_ms_min'], 1)
        return line

    return bench_rows.run_rows(__file__, rows, args.reps, ROW_LIMIT, args.out, edit=with_twin)


if __name__ == '__main__':
    sys.exit(main())
