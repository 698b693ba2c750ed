"""What the row-by-row bench tools share (a module, not a tool): the timers, and the parent loop that
gives every row a child process of its own under a time limit and starts nothing more after the first
row that fails or runs out of time.

A tool keeps its docstring, its ``ROWS``, its ``run_row(name, reps)`` and its ``ROW_LIMIT``, and ends in

    if __name__ == '__main__':
        sys.exit(bench_rows.main(__file__, __doc__, ROWS, run_row, ROW_LIMIT, 'x_bench.jsonl'))

`timed` and `copy_rate` are the timers of the older one-process tools (tools/bench_real2complex.py,
tools/bench_gather.py and those that follow their method).  The package is imported only inside the
functions that time something, so that the loop can be driven without the library."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- timers --------------------------------------------------------------------------------------------
def events_ms(step, warm, reps):
    from baseband_tasks_amd import hip
    for _ in range(warm):
        step()
    hip.synchronize()
    times = []
    for _ in range(reps):
        a = hip.Event().record()
        step()
        b = hip.Event().record()
        b.synchronize()
        times.append(a.elapsed_ms(b))
    return times


def take_turns(candidates, warm, reps):
    """name -> ms of each timed turn: the steps of `candidates` (name -> step) one after the other, turn by
    turn, `warm` untimed turns and then `reps` timed ones."""
    from baseband_tasks_amd import hip
    times = {key: [] for key in candidates}
    for turn in range(warm + reps):
        for key, step in candidates.items():
            hip.synchronize()
            a = hip.Event().record()
            step()
            b = hip.Event().record()
            b.synchronize()
            if turn >= warm:
                times[key].append(a.elapsed_ms(b))
    return times


def reread(task):
    """Read the whole result of `task` again: the cache dropped, from sample 0."""
    task.invalidate_cache()
    task.seek(0)
    task.read_device()


def timed(fn, reps):
    """Device time per call (s) of ``fn()`` on the package's stream, after one warm-up call."""
    import ctypes as C
    from baseband_tasks_amd import hip
    lib = hip.lib()
    fn()
    hip.synchronize()
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.check(lib.bbt_event_create(C.byref(e0)))
    hip.check(lib.bbt_event_create(C.byref(e1)))
    st = hip._stream
    hip.check(lib.bbt_event_record(e0, st))
    for _ in range(reps):
        fn()
    hip.check(lib.bbt_event_record(e1, st))
    hip.check(lib.bbt_event_sync(e1))
    ms = C.c_float()
    hip.check(lib.bbt_event_elapsed_ms(e0, e1, C.byref(ms)))
    lib.bbt_event_destroy(e0)
    lib.bbt_event_destroy(e1)
    return ms.value / 1e3 / reps


def copy_rate(nbytes, reps):
    import numpy as np
    from baseband_tasks_amd import hip
    a = hip.DeviceArray((nbytes,), np.uint8)
    b = hip.DeviceArray((nbytes,), np.uint8)
    a.fill_bytes(1)
    t = timed(lambda: b.copy_from_device(a), reps)
    return 2 * nbytes / t


# -- one child process per row -------------------------------------------------------------------------
def parser(doc, out_name, rows):
    """``[--out FILE] [--reps N] [row ...]`` and the hidden ``--child``."""
    ap = argparse.ArgumentParser(description=doc.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', out_name))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('rows', nargs='*', default=list(rows))
    return ap


def check_rows(ap, names, rows):
    for name in names:
        if name not in rows:
            ap.error(f'unknown row {name}; one of {", ".join(rows)}')


def run_rows(script, names, reps, limit, out_path, edit=None):
    """Each row of `names` as ``python script --child --reps N row`` with `limit` seconds to finish; the
    last line it prints is a JSON object (passed through ``edit(name, line)``, a dict for a dict, if given),
    printed and appended to `out_path` row by row.  The first row that fails or runs out of time ends the
    run: 1 is returned and no further row is started."""
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as out:
        for name in names:
            try:
                done = subprocess.run([sys.executable, os.path.abspath(script), '--child', '--reps', str(reps), name],
                                      stdout=subprocess.PIPE, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                print(f'{name}: no result within {limit} s; stopping', file=sys.stderr)
                return 1
            if done.returncode != 0:
                print(f'{name}: exit status {done.returncode}; stopping', file=sys.stderr)
                return 1
            line = done.stdout.strip().splitlines()[-1]
            if edit:
                line = json.dumps(edit(name, json.loads(line)))
            else:
                json.loads(line)
            print(line, flush=True)
            out.write(line + '\n')
            out.flush()
    return 0


def main(script, doc, rows, run_row, limit, out_name):
    """The whole command line of a tool that has nothing of its own to add to it."""
    ap = parser(doc, out_name, rows)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(run_row(args.rows[0], args.reps)), flush=True)
        return 0
    check_rows(ap, args.rows, rows)
    return run_rows(script, args.rows, args.reps, limit, args.out)
