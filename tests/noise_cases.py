"""Inputs shared by test_noise_model.py (which proves, with the CPU model, what paths of the
sampler they exercise) and test_noise_gpu.py (which runs them on the device)."""
import numpy as np

START = '2020-01-01T00:00:00'

#: (seed, samples_per_frame, sample_shape, dtype, samples in the stream)
CASES = [
    (0, 4096, (), np.float32, 4 * 4096 - 1000),       # frame 0 ends on a wedge acceptance; cut last frame
    (1, 1001, (3,), np.complex64, 5 * 1001 + 17),     # n = 6006 per frame: no multiple of 4; rejected tail pairs
    (12345, 4099, (2,), np.float32, 3 * 4099),        # n = 8198: nine tiles of words, no multiple of 4
    (7, 3000, (), np.complex64, 4 * 3000),            # a wedge pair across a tile boundary, a rejected tail pair
]

#: what the model finds in the whole frames of each case (tools/noise_model.py: `frame`'s tally)
EXPECTED_PATHS = [
    dict(direct=16247, wedge_accept=131, wedge_reject=119, tail=6, tail_reject=0, wedge_straddle=1),
    dict(direct=35719, wedge_accept=310, wedge_reject=254, tail=7, tail_reject=2, wedge_straddle=0),
    dict(direct=24395, wedge_accept=196, wedge_reject=176, tail=3, tail_reject=0, wedge_straddle=0),
    dict(direct=23795, wedge_accept=195, wedge_reject=176, tail=10, tail_reject=1, wedge_straddle=1),
]
#: how the last normal of each whole frame of case 0 is made
EXPECTED_LAST_KINDS_CASE0 = ['wedge', 'direct', 'direct', 'direct']


def make(cls, case, **kwargs):
    from baseband_tasks_amd import units as u
    seed, spf, sample_shape, dtype, length = case
    return cls((length,) + tuple(sample_shape), START, 1. * u.MHz, spf, dtype=dtype, seed=seed, **kwargs)
