"""Finds the frames of tests/noise_cases.py that drive csrc/noise_kernels.hpp through the paths a
stream from counter 0 all but never takes: tiles entered in a tail state, tail pairs across a tile
boundary (accepted, rejected, rejected twice), a frame that ends on a tail, scan rounds entered in
another state than START, counter carries, and a batch of frames under a finite guard.

A frame's counter is free, so nothing has to be searched for by brute force: the first 2^20 blocks
of one key are classified word by word (NumPy, a second or two), and a word of block B that is
wanted in block j of a frame gets there with counter[0] = B - j.  Every candidate is then run
through the model (tools/noise_model.py) and kept only if the model's stats show the path, its
values are NumPy's bit for bit, no flag is raised and the default number of words suffices.

    python tools/noise_find_cases.py          # prints COUNTER_CASES and GUARD_CASE as literals

Deterministic: tests/test_noise_model.py runs `find()` and compares with what is committed.
"""
import pprint
import textwrap

import numpy as np

import noise_model as nm

SEED = 2024                      # the key is that of Philox(SEED)
N_BLOCKS = 1 << 20               # blocks classified
N = 1500                         # normals per frame unless the case says otherwise: two tiles of words
N_ROUNDS = 260000                # 262 tiles: a second round of the scan over a frame's tiles
PER_TILE = nm.TILE // 4          # blocks per tile
FULL = 2**64 - 1
#: stats that are not recorded (they serve the finder only)
NOT_RECORDED = ('tail_ranks', 'walk')
#: tests/noise_cases.py holds what `render` makes between these two lines
BEGIN = '# --- found by tools/noise_find_cases.py ---\n'
END = '# --- end of what tools/noise_find_cases.py found ---\n'


def key_of(seed=SEED):
    return tuple(int(k) for k in np.random.Philox(seed).state['state']['key'])


def run(key, counter, n):
    """The model's stats of a frame, or None unless the frame is a sound test input: NumPy's values
    bit for bit, no flag at the default guard, enough normals in the default number of words."""
    stats = {}
    got, total, flag = nm.frame(key, counter, n, stats=stats)
    if flag or total < n or got.tobytes() != nm.numpy_frame(key, counter, n).tobytes():
        return None
    return stats


def entry(name, key, counter, n, stats):
    return dict(name=name, key=key, counter=tuple(int(c) for c in counter), n=n, n_words=None,
                stats={k: v for k, v in stats.items() if k not in NOT_RECORDED})


def first_that(key, candidates, word_in_frame, n, shows):
    """The first candidate word (an index into the classified stream) that, moved to
    `word_in_frame` of a frame, makes a sound input whose stats satisfy `shows`."""
    for i in candidates:
        block = int(i) // 4 - word_in_frame // 4
        if block < 0:
            continue
        counter = (block, 0, 0, 0)
        stats = run(key, counter, n)
        if stats is not None and shows(stats):
            return counter, stats
    raise RuntimeError('no frame found: classify more blocks')


def one_tail(stats, rejected):
    """The frame's only tail is accepted at once, or after at least one rejected pair."""
    return stats['tail'] == 1 and (stats['tail_reject'] >= 1 if rejected else stats['tail_reject'] == 0)


def find_counter_cases():
    key = key_of()
    W = nm.Words(nm.philox_words(key, (0, 0, 0, 0), 4 * N_BLOCKS), nm.GUARD)
    where = np.arange(4 * N_BLOCKS)
    # the first pair of a tail opened by word i is (i + 1, i + 2)
    first_ok = np.concatenate((W.tail_ok[2:], [False, False]))
    second_ok = np.concatenate((W.tail_ok[4:], [False] * 4))
    inside = where < 4 * N_BLOCKS - 8
    cases = []
    found = {}
    # tiles entered in a tail state: the opener is word 1023 (TAIL1) or 1022 (TAIL2) of the frame
    for rejected in (False, True):
        for depth, opener in ((1, nm.TILE - 1), (2, nm.TILE - 2)):
            for sign, sign_name in ((0, 'pos'), (1, 'neg')):
                state = (nm.TAIL1 if depth == 1 else nm.TAIL2) + sign
                across = 'rejected' if rejected else 'accepted'

                def shows(s, state=state, depth=depth, across=across, rejected=rejected):
                    return (s['tile_entry'][state] == 1 and sum(s['tile_entry']) == 1 and one_tail(s, rejected) and
                            (depth == 1 or s['tail_pair_across_tiles'][across] == 1))

                cand = np.nonzero(W.tail_init & inside & (where % 4 == opener % 4) & (W.tail_sign == sign) &
                                  (first_ok != rejected))[0]
                name = f'entry_tail{depth}_{sign_name}' + ('_rejected' if rejected else '')
                counter, stats = first_that(key, cand, opener, N, shows)
                found[name] = (counter, stats)
                cases.append(entry(name, key, counter, N, stats))
    # two rejected pairs in a row: with the opener at word 1021 the second one lies across the tiles
    cand = np.nonzero(W.tail_init & inside & ~first_ok & ~second_ok)[0]
    try:
        counter, stats = first_that(
            key, cand[cand % 4 == (nm.TILE - 3) % 4], nm.TILE - 3, N,
            lambda s: s['tail_reject_runs'] >= 2 and s['tail_pair_across_tiles']['rejected'] == 1)
    except RuntimeError:
        counter, stats = first_that(key, cand, 400, N, lambda s: s['tail_reject_runs'] >= 2)
    cases.append(entry('reject_run', key, counter, N, stats))
    # the last normal of the frame is made by a tail: n is that tail's rank plus one
    cand = np.nonzero(W.tail_init & inside & first_ok & (where % 4 == 0))[0]
    counter, stats = first_that(key, cand, 400, N, lambda s: one_tail(s, False) and sum(s['tile_entry'][2:]) == 0)
    n = stats['tail_ranks'][0] + 1
    stats = run(key, counter, n)
    assert stats is not None and stats['last_kind'] == 'tail'
    cases.append(entry('last_is_tail', key, counter, n, stats))
    counter, stats = found['entry_tail2_neg']
    n = stats['tail_ranks'][0] + 1
    stats = run(key, counter, n)
    assert stats is not None and stats['last_kind'] == 'tail_straddled'
    cases.append(entry('last_is_straddled_tail', key, counter, n, stats))
    # the scan's second round of 256 tiles starts in WEDGE, or in a tail state
    last_of_round = 256 * nm.TILE - 1
    cand = np.nonzero(W.wedge_init & inside & (where % 4 == 3))[0]
    counter, stats = first_that(key, cand, last_of_round, N_ROUNDS, lambda s: s['round_entry'] == [nm.WEDGE])
    cases.append(entry('round_entry_wedge', key, counter, N_ROUNDS, stats))
    cand = np.nonzero(W.tail_init & inside & (where % 4 == 2) & (W.tail_sign == 1))[0]
    counter, stats = first_that(key, cand, last_of_round - 1, N_ROUNDS, lambda s: s['round_entry'] == [nm.TAIL2 + 1])
    cases.append(entry('round_entry_tail', key, counter, N_ROUNDS, stats))
    # counter carries: the host's + 1 through three words; word 0 wrapping inside tile 0; and
    # between the block that thread 0 of tile 1 computes again (255) and its own (256)
    for name, counter in (('carry_host', (FULL, FULL, FULL, 7)),
                          ('carry_mid_tile', (FULL - 100, FULL, FULL, 7)),
                          ('carry_at_tile', (FULL - PER_TILE, FULL, FULL, 7))):
        stats = run(key, counter, N)
        assert stats is not None
        cases.append(entry(name, key, counter, N, stats))
    assert cases[-3]['stats']['host_carry'] == 3
    assert cases[-2]['stats']['wrap_block'] == 100 and cases[-1]['stats']['wrap_block'] == PER_TILE
    return cases


def guard_walks(seed, spf, n_frame):
    """What the walk of each frame of a float32 stream met (it does not depend on the guard)."""
    stats = {}
    nm.stream_frames(seed, spf, (), np.float32, list(range(n_frame)), stats=stats)
    return [s['walk'] for s in stats['per_frame']]


def off_the_doorstep(walks, guard):
    """No comparison that bears on these frames has its sides within a relative [guard / 4, 4 guard]
    of each other, and no tail value's float32 rounding turns safe or unsafe in that range: what is
    ambiguous at a guard is so at every larger one, so this holds when every frame has as many
    ambiguous decisions at guard / 4 as at 4 guard."""
    return all(nm.ambiguous_at(w, guard / 4) == nm.ambiguous_at(w, 4 * guard) for w in walks)


def find_guard_case(seed=SEED, spf=3000, n_frame=64, walks=None):
    """The largest guard 2^-k, k >= 10, under which some of the frames are flagged and some are not,
    with every decision at least a factor of 4 away from it."""
    if walks is None:
        walks = guard_walks(seed, spf, n_frame)
    for k in range(10, 40):
        guard = 2.0 ** -k
        flags = [int(nm.ambiguous_at(w, guard) > 0) for w in walks]
        if any(flags) and not all(flags) and off_the_doorstep(walks, guard):
            return dict(seed=seed, samples_per_frame=spf, n_frame=n_frame, guard_log2=-k, flags=flags)
    raise RuntimeError('no guard found')


def render(counter_cases, guard_case):
    """The literals as they stand in tests/noise_cases.py."""
    lines = [f'KEY = {counter_cases[0]["key"]!r}', '', 'COUNTER_CASES = [']
    for c in counter_cases:
        assert c['key'] == counter_cases[0]['key']
        stats = 'dict(' + ', '.join(f'{k}={v!r}' for k, v in c['stats'].items()) + ')'
        stats = textwrap.fill(stats, 104, subsequent_indent=' ' * 20, break_long_words=False)
        head = f"dict(name={c['name']!r}, key=KEY, counter={c['counter']!r}, n={c['n']!r}, n_words={c['n_words']!r},"
        lines.append(textwrap.fill(head, 108, initial_indent=' ' * 4, subsequent_indent=' ' * 9))
        lines.append(f'         stats={stats}),')
    lines += [']', '']
    flags = pprint.pformat(guard_case['flags'], width=96, compact=True).replace('\n', '\n' + ' ' * 24)
    head = ', '.join(f'{k}={v!r}' for k, v in guard_case.items() if k != 'flags')
    lines += [f'GUARD_CASE = dict({head},', f'                  flags={flags})']
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    print(render(find_counter_cases(), find_guard_case()), end='')
