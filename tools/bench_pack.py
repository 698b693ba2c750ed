"""Rates of the encoders of the compact HDF5 payloads, one JSON line per case (dev tool).

    python tools/bench_pack.py [--mib 128] [--reps 20] [--copy-tb-s 6.2] [--dir /tmp] [--out profiles/pack_bench.jsonl]

Kernels, HBM-resident: bbt_pack at 1, 2, 4, 8 and 16 bits, bbt_to_half and bbt_from_half on
``--mib`` MiB of float32, each timed with device events after a warm-up call (the method of
tools/bench_real2complex.py).  Reported: bytes read plus bytes written per second, and the fraction
of the plain copy rate (a device-to-device hipMemcpyAsync of the same input size, same run;
``--copy-tb-s`` overrides it, e.g. with the rate tools/membench.hip gives on the same device).

Files: ``read(out=writer)`` of a 2-pol complex64 `Dedisperse` over ``--mib`` MiB of input into a raw
file, a '<c4' file and an 8-bit coded file under ``--dir`` (wall time, best of three, the file closed
inside the timed region), and ``raw_host_pieces``: a stand-in for the raw write before writers took
device pieces -- the same code with `accepts_device` off, so that the task copies every piece down
as complex64 itself.  It is this commit emulating its parent, not a run of the parent.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import baseband_tasks_amd as bt                                     # noqa: E402
from baseband_tasks_amd import hdf5, hip                            # noqa: E402
from baseband_tasks_amd import units as u                           # noqa: E402
from bench_rows import copy_rate, timed                             # noqa: E402


def kernels(mib, reps, copy):
    n = (mib << 20) // 4
    rng = np.random.default_rng(1)
    x = hip.DeviceArray.from_host(rng.standard_normal(n).astype(np.float32))
    for bits in hip.PACK_BITS:
        out = hip.DeviceArray((n * bits // 32,), np.uint32)
        t = timed(lambda: hip.pack(x, bits, out=out), reps)
        moved = x.nbytes + out.nbytes
        yield dict(what='pack', bits=bits, in_mib=mib, s_per_call=t, gb_per_s=moved / t / 1e9,
                   in_gb_per_s=x.nbytes / t / 1e9, copy_gb_per_s=copy / 1e9, copy_fraction=moved / t / copy)
    h = hip.DeviceArray((n,), np.float16)
    t = timed(lambda: hip.to_half(x, out=h), reps)
    moved = x.nbytes + h.nbytes
    yield dict(what='to_half', in_mib=mib, s_per_call=t, gb_per_s=moved / t / 1e9, copy_gb_per_s=copy / 1e9,
               copy_fraction=moved / t / copy)
    t = timed(lambda: hip.from_half(h, np.float32, out=x), reps)
    yield dict(what='from_half', out_mib=mib, s_per_call=t, gb_per_s=moved / t / 1e9, copy_gb_per_s=copy / 1e9,
               copy_fraction=moved / t / copy)


class HostPiecesWriter(hdf5.HDF5StreamWriter):
    """The writer as tasks saw it before it took device pieces."""
    accepts_device = False


def files(mib, where):
    n = (mib << 20) // 16
    rng = np.random.default_rng(2)
    x = rng.standard_normal((n, 2, 2)).astype(np.float32).view(np.complex64)[..., 0]
    ds = bt.DeviceStream(x, '2020-01-01T00:00:00', 16 * u.MHz, frequency=1400 * u.MHz, sideband=1)
    dd = bt.Dedisperse(ds, 30.)
    dd.read_device(dd.samples_per_frame)                                 # (plans made, buffers allocated)
    hip.synchronize()
    cases = [('raw_host_pieces', HostPiecesWriter, {}), ('raw', hdf5.HDF5StreamWriter, {}),
             ('c4', hdf5.HDF5StreamWriter, dict(encoded_dtype='c4')), ('bps8', hdf5.HDF5StreamWriter, dict(bps=8))]
    for name, cls, how in cases:
        path = os.path.join(where, f'bench_pack_{name}.h5')
        best = None
        for _ in range(3):
            dd.seek(0)
            t0 = time.perf_counter()
            with cls(path, template=dd, **how) as fw:
                dd.read(out=fw)
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        size = os.path.getsize(path)
        os.remove(path)
        yield dict(what='read_out_writer', file=name, in_mib=mib, n_samples=int(dd.shape[0]), file_mib=size / 2**20,
                   s_best_of_3=best, gsamples_per_s=dd.shape[0] / best / 1e9,
                   stream_gb_per_s=dd.shape[0] * 16 / best / 1e9, directory=where)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mib', type=int, default=128)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--copy-tb-s', type=float, default=None)
    ap.add_argument('--dir', default=tempfile.gettempdir())
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    hip.set_device(0)
    copy = args.copy_tb_s * 1e12 if args.copy_tb_s else copy_rate(args.mib << 20, args.reps)
    lines = [json.dumps(dict(what='copy', mib=args.mib, gb_per_s=copy / 1e9,
                             source='--copy-tb-s' if args.copy_tb_s else 'hipMemcpyAsync device to device'))]
    print(lines[0], flush=True)
    for result in list(kernels(args.mib, args.reps, copy)) + list(files(args.mib, args.dir)):
        lines.append(json.dumps(result))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
