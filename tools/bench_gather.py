"""Rates of the shaping and combining kernels, HBM-resident, one JSON line per case (dev tool;
results under profiles/gather_bench.jsonl).

    python tools/bench_gather.py [--mib 128] [--reps 20] [--copy-tb-s 6.2] [--out profiles/gather_bench.jsonl]

For each case: one bbt_gather_execute that writes about ``--mib`` MiB, timed with device events after
a warm-up call (the method of tools/bench_real2complex.py).  Reported: bytes read that are used plus
bytes written per second, the route, and the fraction of the plain copy rate: a device-to-device
hipMemcpyAsync of the same output size, timed the same way in the same run (``copy_gb_per_s``;
``--copy-tb-s`` overrides it with the rate tools/membench.hip gave in the same visit).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from baseband_tasks_amd import hip                                  # noqa: E402
from baseband_tasks_amd.shaping import index_map                    # noqa: E402
from bench_rows import copy_rate, timed                             # noqa: E402

CF = 8          # complex64

CASES = [
    # name, input sample shapes, element bytes, task, combine, forced route
    ('stack2_last', [()] * 2, CF, lambda d: np.stack(d, -1), True, 'auto'),
    ('stack8_last', [()] * 8, CF, lambda d: np.stack(d, -1), True, 'auto'),
    ('concatenate_2x(1024,2)', [(1024, 2)] * 2, CF, lambda d: np.concatenate(d, 1), True, 'auto'),
    ('transpose_(1024,2)', [(1024, 2)], CF, lambda d: d.transpose(0, 2, 1), False, 'auto'),
    ('getitem_256_of_1024', [(1024, 2)], CF, lambda d: d[:, 384:640], False, 'auto'),
    ('getitem_stride2', [(1024,)], CF, lambda d: d[:, ::2], False, 'auto'),
    ('getitem_stride2_pairs', [(1024, 2)], CF, lambda d: d[:, ::2], False, 'auto'),
    ('transpose_(1024,2)_direct', [(1024, 2)], CF, lambda d: d.transpose(0, 2, 1), False, 'direct'),
    ('stack2_last_direct', [()] * 2, CF, lambda d: np.stack(d, -1), True, 'direct'),
]


def case(name, shapes, eb, task, combine, route, mib, reps, copy):
    out_shape, src, elem = index_map(task, shapes, combine=combine)
    rows = [int(np.prod(s, dtype=np.int64)) for s in shapes]
    r_out = len(src)
    n = max(1, (mib << 20) // (r_out * eb))
    xs = [hip.DeviceArray((n, r * eb), np.uint8).fill_bytes(k + 1) for k, r in enumerate(rows)]
    y = hip.DeviceArray((n, r_out * eb), np.uint8)
    plan = hip.GatherPlan(rows, src, elem, eb, route=route)
    info = plan.info()
    t = timed(lambda: plan.execute(xs, y, n), reps)
    moved = 2 * n * r_out * eb
    plan.close()
    return dict(what='gather', case=name, sample_shapes=[list(s) for s in shapes], out_shape=list(out_shape),
                elem_bytes=eb, n_samples=n, out_mib=n * r_out * eb / 2**20, s_per_call=t,
                gb_per_s=moved / t / 1e9, copy_gb_per_s=copy / 1e9, copy_fraction=moved / t / copy, **info)


def host_roundtrip(mib):
    """What `Stack` replaces: two single-pol complex64 streams in HBM read to the host, stacked with
    NumPy and uploaded again (wall time, best of three)."""
    import time
    import baseband_tasks_amd as bt
    n = (mib << 20) // 16
    rng = np.random.default_rng(1)
    xs = [bt.DeviceStream(rng.standard_normal((n, 2)).astype(np.float32).view(np.complex64)[:, 0],
                          '2020-01-01T00:00:00', 16e6) for _ in range(2)]
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        for x in xs:
            x.seek(0)
        both = np.stack([x.read() for x in xs], axis=-1)
        up = bt.DeviceStream(both, '2020-01-01T00:00:00', 16e6)
        hip.synchronize()
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
        del up
    return dict(what='stack2_host_roundtrip', out_mib=mib, s_host_roundtrip=best,
                gb_per_s_host=2 * (mib << 20) / best / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mib', type=int, default=128)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--copy-tb-s', type=float, default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    hip.set_device(0)
    copy = args.copy_tb_s * 1e12 if args.copy_tb_s else copy_rate(args.mib << 20, args.reps)
    lines = [json.dumps(dict(what='copy', mib=args.mib, gb_per_s=copy / 1e9,
                             source='--copy-tb-s' if args.copy_tb_s else 'hipMemcpyAsync device to device'))]
    print(lines[0], flush=True)
    for c in CASES:
        lines.append(json.dumps(case(*c, args.mib, args.reps, copy)))
        print(lines[-1], flush=True)
    lines.append(json.dumps(host_roundtrip(args.mib)))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
