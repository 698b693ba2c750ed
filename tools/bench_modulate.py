"""Rates of `Modulate`, one JSON line per case (dev tool).

    python tools/bench_modulate.py [--log2 26] [--wide-log2 16] [--reps 10] [--task-log2 22]
                                   [--out profiles/modulate_bench.jsonl]

Every case reads a stream that is resident in HBM through ``Modulate(...).read_device`` and reports
two times beside a device-to-device copy of the same bytes timed in the same run (the yardstick of
tools/bench_psrfits_search.py): ``s_read_device``, wall time of the whole read, best of three, with
the host's share in it (run tables, pieces, launches), and ``s_kernel``, device time per launch of
the entry point alone on tables that are in HBM already (events, the method of
tools/bench_real2complex.py).  Bytes moved: the stream read once and written once.

Cases: (2^log2, 2) complex64 with a `PolycoPhase` on tests/golden/B1937_polyco.dat and 1024 bins on
both table routes; the same stream with a linear host callable; (2^wide_log2, 1024, 2) complex64
with a gain per bin and element; and the host alternative for the narrow stream, the generic `Task`
with a NumPy multiply per frame read through ``read()`` (on 2^task_log2 samples).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import baseband_tasks_amd as bt                                     # noqa: E402
from baseband_tasks_amd import hip                                  # noqa: E402
from baseband_tasks_amd.fold_table import plan_pieces               # noqa: E402
from bench_rows import copy_rate, timed                             # noqa: E402

POLYCO = os.path.join(ROOT, 'tests', 'golden', 'B1937_polyco.dat')
T0 = bt.Time('2018-05-06T22:20:00')
RATE = 16e6


def stream(n, sample_shape):
    x = hip.DeviceArray((n,) + sample_shape, np.complex64)
    x.fill_bytes(0x3c)                                  # (every float 0.0115: the product does not care)
    return bt.DeviceStream(x, T0, RATE, samples_per_frame=min(n, (1 << 24) // int(np.prod(sample_shape))))


def wall(mh, n):
    best = None
    for _ in range(3):
        mh.seek(0)
        mh.invalidate_cache()
        hip.synchronize()
        t0 = time.perf_counter()
        mh.read_device(n)
        hip.synchronize()
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return best


def kernel(mh, reps):
    """Device time of one launch over the first chunk of the stream, tables uploaded before."""
    n = min(mh.shape[0], max(1, mh.modulate_budget // (mh._n_elem * 8)))
    x = hip.DeviceArray((n,) + mh.sample_shape, np.complex64).fill_bytes(0x3c)
    y = hip.DeviceArray((n,) + mh.sample_shape, np.complex64)
    gain = hip.DeviceArray.from_host(mh._gain_host)
    stride = mh._n_elem if mh._gain_host.ndim == 2 else 0
    lib, st = hip.lib(), hip.get_stream()
    if hasattr(mh.phase, 'fold_pieces') and mh._route() == 'device':
        edges = mh._frame_edges(0, n)
        plan = plan_pieces(edges, mh._row_pieces(edges), mh.n_phase, 0, n)[2]
        pieces = hip.DeviceArray.from_host(hip._piece_words(plan))
        n_piece, n_coeff = len(plan['row']), plan['coeff'].shape[1]
        t = timed(lambda: hip.check(lib.bbt_modulate_pieces(x.ptr, y.ptr, n, 2 * mh._n_elem, gain.ptr, mh.n_phase,
                                                            stride, pieces.ptr, n_piece, n_coeff, st)), reps)
        return n, t, dict(pieces=n_piece, coefficients=n_coeff)
    begin, bins = mh._runs(0, n)
    table = hip.DeviceArray.from_host(np.concatenate([begin, bins]))
    t = timed(lambda: hip.check(lib.bbt_modulate_runs(x.ptr, y.ptr, n, 2 * mh._n_elem, gain.ptr, mh.n_phase, stride,
                                                      table.ptr, table.ptr + 8 * len(begin), len(begin), st)), reps)
    return n, t, dict(runs=len(begin))


def case(name, mh, reps, copy):
    n = mh.shape[0]
    sample_bytes = mh._n_elem * 8
    t_wall = wall(mh, n)
    n_k, t_k, extra = kernel(mh, reps)
    return dict(what='modulate', case=name, shape=list(mh.shape), n_phase=mh.n_phase,
                gain_per_element=mh._gain_host.ndim == 2, route=mh._route() if hasattr(mh.phase, 'fold_pieces') else 'runs',
                mib=n * sample_bytes / 2**20, s_read_device=t_wall, read_gb_per_s=2 * n * sample_bytes / t_wall / 1e9,
                read_copy_fraction=2 * n * sample_bytes / t_wall / copy, kernel_samples=n_k, s_kernel=t_k,
                kernel_gb_per_s=2 * n_k * sample_bytes / t_k / 1e9, kernel_copy_fraction=2 * n_k * sample_bytes / t_k / copy,
                copy_gb_per_s=copy / 1e9, **extra)


def host_task(n, profile, copy):
    """The reference's way: a host `Task` whose callable multiplies each frame (NumPy), read()."""
    sh = stream(n, (2,))
    f0 = 641.9

    def modulate(fh, data):
        t = fh.tell() + np.arange(data.shape[0])
        b = (((t / RATE * f0) % 1.) * len(profile)).astype(np.int64)
        return data * profile[b][:, np.newaxis]
    th = bt.Task(sh, modulate, samples_per_frame=1 << 16)
    best = None
    for _ in range(2):
        th.seek(0)
        t0 = time.perf_counter()
        th.read()
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return dict(what='host_task', shape=[n, 2], mib=n * 16 / 2**20, s_read=best, gb_per_s=2 * n * 16 / best / 1e9,
                copy_fraction=2 * n * 16 / best / copy, copy_gb_per_s=copy / 1e9,
                note='Task(DeviceStream, NumPy multiply per frame of 65536 samples).read(): down, multiply, result on the host')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--log2', type=int, default=26)
    ap.add_argument('--wide-log2', type=int, default=16)
    ap.add_argument('--task-log2', type=int, default=22)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    hip.set_device(0)
    n = 1 << args.log2
    copy = copy_rate(n * 16, args.reps)
    lines = [json.dumps(dict(what='copy', mib=n * 16 / 2**20, gb_per_s=copy / 1e9,
                             source='hipMemcpyAsync device to device', device=hip.device_name()))]
    print(lines[0], flush=True)

    def keep(result):
        lines.append(json.dumps(result))
        print(lines[-1], flush=True)

    rng = np.random.default_rng(1)
    profile = np.sqrt(1. + 20. * np.exp(-0.5 * ((np.arange(1024) - 512) / 20.) ** 2)).astype(np.float32)
    pp = bt.phases.PolycoPhase(POLYCO)
    narrow = stream(n, (2,))
    for route in ('device', 'host'):
        mh = bt.Modulate(narrow, profile, pp)
        mh.table_route = route
        keep(case('polyco', mh, args.reps, copy))
        mh.close()
    mh = bt.Modulate(narrow, profile, lambda t: 0.25 + 641.9 * (t - T0))
    keep(case('linear_callable', mh, args.reps, copy))
    mh.close()
    del narrow
    wide = stream(1 << args.wide_log2, (1024, 2))
    gains = (profile[:, np.newaxis, np.newaxis] * rng.uniform(0.5, 1.5, (1024, 2))).astype(np.float32)
    mh = bt.Modulate(wide, gains, lambda t: 0.25 + 641.9 * (t - T0))
    keep(case('wide_per_element', mh, args.reps, copy))
    mh.close()
    mh = bt.Modulate(wide, profile, lambda t: 0.25 + 641.9 * (t - T0))
    keep(case('wide_shared', mh, args.reps, copy))
    mh.close()
    del wide
    keep(host_task(1 << args.task_log2, profile, copy))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
