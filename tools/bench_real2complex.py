"""Real2Complex rates, HBM-resident, one JSON line per case (dev tool; results under profiles/).

    python tools/bench_real2complex.py [--mib 128] [--reps 20] [--m 1024,4096,...] [--s 1,2,8]

For each output frame length M and number S of float32 streams: one bbt_r2c_execute over as many
frames as make about ``--mib`` MiB of input, timed with device events after a warm-up call.
Reported: output complete samples per second, bytes moved (16 S per output complete sample: the
input read once, the output written once), the fraction of 8 TB/s, and the route.  Yardsticks on
the same bytes: the overlap-save plan with n_fft = M on S complex64 streams (max(S, 2)), one block
per frame (hop M, nothing dropped: the same transforms per pair), and Channelize(M) where it runs.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from baseband_tasks_amd import hip          # noqa: E402
from bench_rows import timed                # noqa: E402

HBM = 8e12


def case(m, s, mib, reps):
    frames = max(1, (mib << 20) // (2 * m * s * 4))
    x = hip.DeviceArray((frames * 2 * m, s), np.float32)
    hip.check(hip.lib().bbt_memset(x.ptr, 0, x.nbytes, hip._stream))
    y = hip.DeviceArray((frames * m, s), np.complex64)
    plan = hip.R2CPlan(m, s)
    info = plan.info()
    t = timed(lambda: plan.execute(x, y, frames), reps)
    n_out = frames * m
    nbytes = 16 * s * n_out
    row = dict(what='real2complex', M=m, S=s, frames=frames, one_pass=info['one_pass'],
               workspace_bytes=info['workspace_bytes'], s_per_call=t, samples_per_s=n_out / t,
               gb_per_s=nbytes / t / 1e9, hbm_fraction=nbytes / t / HBM, us_per_frame=t / frames * 1e6)
    # yardstick: the overlap-save plan, n_fft = M, on the same bytes as S complex64 streams
    sc = max(s, 2)
    xz = hip.DeviceArray((frames * m, sc), np.complex64)
    yz = hip.DeviceArray((frames * m, sc), np.complex64)
    hip.check(hip.lib().bbt_memset(xz.ptr, 0, xz.nbytes, None))
    osm = hip.OsmPlan(m, sc, np.ones((1, m), np.complex64))
    lib = hip.lib()
    t_osm = timed(lambda: hip.check(lib.bbt_osm_execute_regular(osm._h, xz.ptr, yz.ptr, frames, 0, 0, m, 0,
                                                                 hip._stream)),
                  reps)
    row.update(osm_s_per_call=t_osm, osm_us_per_block=t_osm / frames * 1e6, vs_osm=t / t_osm * sc / s)
    try:
        chan = hip.ChanPlan(m, sc, -1)
        t_ch = timed(lambda: chan.execute(xz, yz, frames), reps)
        row.update(chan_s_per_call=t_ch, vs_chan=t / t_ch * sc / s)
        chan.close()
    except Exception as e:            # (Channelize takes n <= 8192 and 16384 only)
        row.update(chan_s_per_call=None, chan_note=str(e).splitlines()[0][:80])
    osm.close()
    plan.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mib', type=int, default=128)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--m', default='1024,4096,6174,8192,10000,16384,1048576')
    ap.add_argument('--s', default='1,2,8')
    args = ap.parse_args()
    hip.set_device(0)
    for m in [int(v) for v in args.m.split(',')]:
        for s in [int(v) for v in args.s.split(',')]:
            print(json.dumps(case(m, s, args.mib, args.reps)), flush=True)


if __name__ == '__main__':
    main()
