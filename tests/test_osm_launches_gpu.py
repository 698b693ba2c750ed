"""Arms of the overlap-save launch list (csrc/osm_launch.hpp) that the parity suite reaches thinly, each as
one plan and one execute call on seeded input against overlap-save with numpy.fft in double: pair-planar
input, 1024-point columns, the middle passes of three levels in pieces, and a regular run as one launch.
Tolerances: those of tests/test_gpu_parity.py, which holds every block length to the same two."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from conftest import rel_l2, max_over_rms
from test_gpu_parity import MAX_TOL, REL_L2_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not bt.hip.available():
        pytest.fail("no GPU / libbbt_hip.so: the -m gpu suite must run on an MI355X")


def run_and_compare(n_fft, n_stream, nblk, planar=False, regular=False):
    hip = bt.hip
    rng = np.random.default_rng(n_fft + n_stream)
    pad = n_fft // 8
    keep = n_fft - 2 * pad
    n_in = (nblk - 1) * keep + n_fft
    x = rng.standard_normal((n_in, 2 * n_stream), dtype=np.float32).view(np.complex64)
    resp = np.exp(2j * np.pi * rng.random(n_fft)) * (0.5 + rng.random(n_fft))
    plan = hip.OsmPlan(n_fft, n_stream, resp[np.newaxis].astype(np.complex64))
    try:
        info = plan.info()
        if planar:          # pair p as its own array of two-stream samples
            given = np.ascontiguousarray(x.reshape(n_in, n_stream // 2, 2).transpose(1, 0, 2))
            plan.set_layout(in_plane=n_in)
        else:
            given = x
        x_dev = hip.DeviceArray.from_host(given.reshape(n_in, n_stream))
        y_dev = hip.DeviceArray((n_in, n_stream), np.complex64)
        y_dev.fill_bytes(0)
        off = np.arange(nblk) * keep
        if regular:
            plan.execute_regular(x_dev, y_dev, nblk, 0, 0, keep, pad)
        else:
            plan.execute(x_dev, y_dev, off, off, np.full(nblk, pad), np.full(nblk, keep))
        got = y_dev.to_host()[:nblk * keep]
    finally:
        plan.close()
    want = np.empty((nblk * keep, n_stream), np.complex128)
    resp64 = resp.astype(np.complex64).astype(np.complex128)[:, np.newaxis]
    for b in range(nblk):
        block = np.fft.ifft(np.fft.fft(x[b * keep:b * keep + n_fft].astype(np.complex128), axis=0) * resp64, axis=0)
        want[b * keep:(b + 1) * keep] = block[pad:pad + keep]
    e2, em = rel_l2(got, want), max_over_rms(got, want)
    print(f'n_fft {n_fft}  streams {n_stream}  blocks {nblk}  plan {info}  rel-L2 {e2:.2e}  max/rms {em:.2e}')
    assert got.dtype == np.complex64 and e2 <= REL_L2_TOL and em <= MAX_TOL, (e2, em)
    return info


def test_pair_planar_input_of_256_point_columns():
    info = run_and_compare(2**17, 4, 3, planar=True)
    assert (info['n1'], info['n2']) == (256, 512)


def test_1024_point_columns():
    info = run_and_compare(2**22, 2, 1)
    assert (info['n1'], info['n2']) == (1024, 4096)


def test_three_levels_with_the_middle_passes_in_pieces():
    # two stream pairs of 2^23 samples: 512 outer rows of 512 KiB, two pieces of the default 128 MiB
    info = run_and_compare(2**23, 4, 1)
    assert (info['n1'], info['n2']) == (16, 2048)


def test_a_regular_run_as_one_launch():
    # 40 blocks in steps: one launch of 16-point column passes with pairs in eights, and of the one kernel
    info = run_and_compare(8192, 16, 40)
    assert (info['n1'], info['n2'], info['chunk_blocks']) == (16, 512, 16)
    info = run_and_compare(4096, 2, 40, regular=True)
    assert (info['n1'], info['n2']) == (1, 4096)
