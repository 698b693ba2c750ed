"""Inputs shared by test_noise_model.py (which proves, with the CPU model, what paths of the
sampler and which seams of the three passes they exercise) and test_noise_gpu.py (which runs them
on the device)."""
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

# Frames with an explicit counter, and a batch of frames under a finite guard, that reach what a
# stream from counter 0 all but never does.  Everything from here to the end marker is what
# `python tools/noise_find_cases.py` prints (test_noise_model.py runs the finder and compares):
# `stats` is what the model's `frame` reports for the frame, `flags` what it raises per frame of
# NoiseGenerator(seed=seed, samples_per_frame=..., float32) under a guard of 2**guard_log2.
# --- found by tools/noise_find_cases.py ---
KEY = (5514401882974304769, 18299549282331608904)

COUNTER_CASES = [
    dict(name='entry_tail1_pos', key=KEY, counter=(3664, 0, 0, 0), n=1500, n_words=None,
         stats=dict(direct=1493, wedge_accept=6, wedge_reject=14, tail=1, tail_reject=0, wedge_straddle=0, total=1761,
                    n_tile=2, last_kind='direct', tile_entry=[0, 0, 1, 0, 0, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 0}, tail_reject_runs=0,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='entry_tail1_neg', key=KEY, counter=(25049, 0, 0, 0), n=1500, n_words=None,
         stats=dict(direct=1486, wedge_accept=13, wedge_reject=8, tail=1, tail_reject=0, wedge_straddle=0, total=1765,
                    n_tile=2, last_kind='direct', tile_entry=[0, 0, 0, 1, 0, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 0}, tail_reject_runs=0,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='entry_tail2_pos', key=KEY, counter=(13083, 0, 0, 0), n=1500, n_words=None,
         stats=dict(direct=1488, wedge_accept=11, wedge_reject=11, tail=1, tail_reject=0, wedge_straddle=0, total=1766,
                    n_tile=2, last_kind='direct', tile_entry=[0, 0, 0, 0, 1, 0],
                    tail_pair_across_tiles={'accepted': 1, 'rejected': 0}, tail_reject_runs=0,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='entry_tail2_neg', key=KEY, counter=(4910, 0, 0, 0), n=1500, n_words=None,
         stats=dict(direct=1488, wedge_accept=11, wedge_reject=8, tail=1, tail_reject=0, wedge_straddle=0, total=1769,
                    n_tile=2, last_kind='direct', tile_entry=[0, 0, 0, 0, 0, 1],
                    tail_pair_across_tiles={'accepted': 1, 'rejected': 0}, tail_reject_runs=0,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='entry_tail1_pos_rejected', key=KEY, counter=(823, 0, 0, 0), n=1500, n_words=None,
         stats=dict(direct=1491, wedge_accept=8, wedge_reject=7, tail=1, tail_reject=1, wedge_straddle=0, total=1773,
                    n_tile=2, last_kind='direct', tile_entry=[0, 0, 1, 0, 0, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 0}, tail_reject_runs=1,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='entry_tail1_neg_rejected', key=KEY, counter=(89525, 0, 0, 0), n=1500, n_words=None,
         stats=dict(direct=1490, wedge_accept=9, wedge_reject=10, tail=1, tail_reject=1, wedge_straddle=0, total=1765,
                    n_tile=2, last_kind='direct', tile_entry=[0, 0, 0, 1, 0, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 0}, tail_reject_runs=1,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='entry_tail2_pos_rejected', key=KEY, counter=(71647, 0, 0, 0), n=1500, n_words=None,
         stats=dict(direct=1491, wedge_accept=8, wedge_reject=5, tail=1, tail_reject=1, wedge_straddle=0, total=1780,
                    n_tile=2, last_kind='direct', tile_entry=[0, 0, 0, 0, 1, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 1}, tail_reject_runs=1,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='entry_tail2_neg_rejected', key=KEY, counter=(432455, 0, 0, 0), n=1500, n_words=None,
         stats=dict(direct=1484, wedge_accept=15, wedge_reject=12, tail=1, tail_reject=1, wedge_straddle=0, total=1759,
                    n_tile=2, last_kind='direct', tile_entry=[0, 0, 0, 0, 0, 1],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 1}, tail_reject_runs=1,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='reject_run', key=KEY, counter=(125309, 0, 0, 0), n=1500, n_words=None,
         stats=dict(direct=1490, wedge_accept=9, wedge_reject=5, tail=1, tail_reject=2, wedge_straddle=0, total=1769,
                    n_tile=2, last_kind='direct', tile_entry=[1, 0, 0, 0, 0, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 0}, tail_reject_runs=2,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='last_is_tail', key=KEY, counter=(3438, 0, 0, 0), n=396, n_words=None,
         stats=dict(direct=394, wedge_accept=1, wedge_reject=2, tail=1, tail_reject=0, wedge_straddle=0, total=651,
                    n_tile=1, last_kind='tail', tile_entry=[0, 0, 0, 0, 0, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 0}, tail_reject_runs=0,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='last_is_straddled_tail', key=KEY, counter=(4910, 0, 0, 0), n=1007, n_words=None,
         stats=dict(direct=1002, wedge_accept=4, wedge_reject=6, tail=1, tail_reject=0, wedge_straddle=0, total=1270,
                    n_tile=2, last_kind='tail_straddled', tile_entry=[0, 0, 0, 0, 0, 1],
                    tail_pair_across_tiles={'accepted': 1, 'rejected': 0}, tail_reject_runs=0,
                    round_entry=[], host_carry=0, wrap_block=None)),
    dict(name='round_entry_wedge', key=KEY, counter=(103, 0, 0, 0), n=260000, n_words=None,
         stats=dict(direct=257856, wedge_accept=2068, wedge_reject=1687, tail=76, tail_reject=4, wedge_straddle=4,
                    total=262408, n_tile=262, last_kind='direct', tile_entry=[255, 4, 0, 0, 0, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 0}, tail_reject_runs=1,
                    round_entry=[1], host_carry=0, wrap_block=None)),
    dict(name='round_entry_tail', key=KEY, counter=(13287, 0, 0, 0), n=260000, n_words=None,
         stats=dict(direct=257800, wedge_accept=2124, wedge_reject=1689, tail=76, tail_reject=5, wedge_straddle=3,
                    total=262328, n_tile=262, last_kind='direct', tile_entry=[255, 3, 0, 0, 0, 1],
                    tail_pair_across_tiles={'accepted': 1, 'rejected': 0}, tail_reject_runs=1,
                    round_entry=[5], host_carry=0, wrap_block=None)),
    dict(name='carry_host', key=KEY, counter=(18446744073709551615, 18446744073709551615,
         18446744073709551615, 7), n=1500, n_words=None,
         stats=dict(direct=1482, wedge_accept=18, wedge_reject=10, tail=0, tail_reject=0, wedge_straddle=0, total=1756,
                    n_tile=2, last_kind='direct', tile_entry=[1, 0, 0, 0, 0, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 0}, tail_reject_runs=0,
                    round_entry=[], host_carry=3, wrap_block=None)),
    dict(name='carry_mid_tile', key=KEY, counter=(18446744073709551515, 18446744073709551615,
         18446744073709551615, 7), n=1500, n_words=None,
         stats=dict(direct=1481, wedge_accept=19, wedge_reject=7, tail=0, tail_reject=0, wedge_straddle=0, total=1763,
                    n_tile=2, last_kind='direct', tile_entry=[1, 0, 0, 0, 0, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 0}, tail_reject_runs=0,
                    round_entry=[], host_carry=0, wrap_block=100)),
    dict(name='carry_at_tile', key=KEY, counter=(18446744073709551359, 18446744073709551615,
         18446744073709551615, 7), n=1500, n_words=None,
         stats=dict(direct=1482, wedge_accept=17, wedge_reject=10, tail=1, tail_reject=0, wedge_straddle=0, total=1754,
                    n_tile=2, last_kind='direct', tile_entry=[1, 0, 0, 0, 0, 0],
                    tail_pair_across_tiles={'accepted': 0, 'rejected': 0}, tail_reject_runs=0,
                    round_entry=[], host_carry=0, wrap_block=256)),
]

GUARD_CASE = dict(seed=2024, samples_per_frame=3000, n_frame=64, guard_log2=-22,
                  flags=[0, 1, 1, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 1, 1, 1, 1, 1,
                         0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 0,
                         1])
# --- end of what tools/noise_find_cases.py found ---


def counter_case(name):
    return next(c for c in COUNTER_CASES if c['name'] == name)


def make(cls, case, **kwargs):
    from baseband_tasks_amd import units as u
    seed, spf, sample_shape, dtype, length = case
    return cls((length,) + tuple(sample_shape), START, 1. * u.MHz, spf, dtype=dtype, seed=seed, **kwargs)
