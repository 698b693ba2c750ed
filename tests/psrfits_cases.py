"""Cases shared by the host and GPU tests of the two PSRFITS coders: test_psrfits_gpu.py and
test_psrfits_search_gpu.py run them on the device against the NumPy twins; test_psrfits_host.py and
test_psrfits_search_host.py feed every one of them, without a GPU, through the launchers' own rule
(csrc/psrfits_geo.hpp, csrc/psrsearch_geo.hpp, compiled into tests/psrfits_geo_check.cpp and
tests/psrsearch_geo_check.cpp) and prove with the ledgers below that together they launch every
template instantiation of the kernels and reach every ragged edge of the tiling.  A case list that
stops covering a path fails there, on any machine, and the ledger names the path."""

# -- search mode -----------------------------------------------------------------------------------
#: ((nrow, nsblk, nchan, npol), nbits): one tile of 64 columns at every width (the 1-bit rows leave as
#: bytes, the others as dwords); a byte a spectrum; 48 columns, not a power of two, nsblk neither;
#: one sample a row; few columns, time across the lanes, more samples than a coding tile; 16 tiles
SEARCH_OLD = [((3, 64, 16, 4), 8), ((3, 64, 16, 4), 4), ((3, 64, 16, 4), 2), ((3, 64, 16, 4), 1),
              ((2, 32, 8, 1), 1), ((2, 48, 24, 2), 4), ((2, 48, 24, 2), 8), ((1, 1, 16, 2), 8),
              ((2, 8192, 8, 2), 8), ((2, 64, 1024, 4), 8)]
#: the smallest shapes that reach the rest of the family: dword stores at 1 bit and a ragged last
#: channel tile behind a full one of 64 channels (so codes beyond the LDS skew at channel 32) at
#: every width; byte stores because of the shape (9, 18, 33 bytes a polarization), the last with a
#: tile of one byte; three polarizations (ct 84: 252 busy threads, pitch 97) with dwords and with
#: bytes; 24 columns (ny = 10 threads a column); three coding tiles on the few-column route
SEARCH_NEW = [((2, 40, 96, 4), 1), ((2, 40, 96, 4), 2), ((2, 40, 80, 4), 4), ((2, 40, 80, 4), 8),
              ((2, 40, 72, 4), 1), ((2, 40, 72, 4), 2), ((2, 40, 66, 4), 4),
              ((2, 50, 100, 3), 8), ((2, 50, 100, 3), 2), ((2, 50, 8, 3), 8), ((1, 600, 8, 2), 8)]
SEARCH_CASES = SEARCH_OLD + SEARCH_NEW
#: codes 1 byte into their allocation: byte accesses whatever the shape (the first with the input 4
#: bytes into its own, too)
SEARCH_SHIFTED_OLD = ((2, 64, 16, 4), 8)
SEARCH_SHIFTED_NEW = [((2, 40, 96, 4), 1), ((2, 40, 96, 4), 2), ((2, 40, 80, 4), 4)]
SEARCH_SHIFTED = [SEARCH_SHIFTED_OLD] + SEARCH_SHIFTED_NEW


def search_id(case, shifted=False):
    (n_row, nsblk, n_chan, n_pol), nbits = case
    # (the first shifted case had this name before there were others)
    tail = '-codes+1' if shifted and case != SEARCH_SHIFTED_OLD else ''
    return f'{n_row}x{nsblk}x{n_chan}x{n_pol}-{nbits}bit{tail}'


def search_runs(cases=None, shifted=None):
    """[(name, (nsblk, nchan, npol, nbits, codes 4-byte aligned))] of what the GPU tests launch."""
    cases = SEARCH_CASES if cases is None else cases
    shifted = SEARCH_SHIFTED if shifted is None else shifted
    return ([(search_id(c), c[0][1:] + (c[1], 1)) for c in cases]
            + [(search_id(c, True) + ' (shifted)', c[0][1:] + (c[1], 0)) for c in shifted])


def _pow2(n):
    return n & (n - 1) == 0


def search_ledger(runs, geo):
    """path of the search-mode kernels -> the names of the runs that take it.  ``geo(shape)`` is
    psrsearch_geo_check's line for (nsblk, nchan, npol, nbits, aligned)."""
    took = {}
    for nbits in (1, 2, 4, 8):
        for how in ('vec', 'scalar'):
            took[f'<{nbits},{how}> is launched'] = []
    for nbits in (1, 2, 4):
        for how in ('vec', 'scalar by shape'):
            took[f'{nbits} bit, {how}: ragged last tile on the 32 / n_pol pitch'] = []
            took[f'{nbits} bit, {how}: a tile beyond the skew (ct > 32)'] = []
        took[f'{nbits} bit: scalar by the codes pointer alone, ragged last tile, ct > 32'] = []
    took['8 bit: ragged last tile on the 32 / n_pol pitch'] = []
    for n_pol in (1, 2, 3, 4):
        took[f'n_pol = {n_pol}'] = []
    took['3 polarizations (pitch of want = 1, idle threads), vec'] = []
    took['3 polarizations (pitch of want = 1, idle threads), scalar'] = []
    took['few-column route with ny not a power of two'] = []
    took['few-column route with 3 polarizations (pitch of want = 1)'] = []
    took['nsblk below ts'] = []
    took['nsblk an exact multiple of ts'] = []
    took['nsblk = k ts + r, k >= 2'] = []
    took['few-column route: nsblk = k ts + r, k >= 2'] = []
    for name, shape in runs:
        nsblk, n_chan, n_pol, nbits, aligned = shape
        g = geo(shape)
        how = 'vec' if g['vec'] else 'scalar'
        took[f'<{nbits},{how}> is launched'].append(name)
        ragged, skew = n_chan % g['ct'] != 0, g['ct'] > 32
        by_pointer = not aligned and bool(geo(shape[:4] + (1,))['vec'])
        mode = 'vec' if g['vec'] else 'scalar by shape' if aligned else None
        if nbits < 8 and mode and _pow2(n_pol):
            if ragged:
                took[f'{nbits} bit, {mode}: ragged last tile on the 32 / n_pol pitch'].append(name)
            if skew:
                took[f'{nbits} bit, {mode}: a tile beyond the skew (ct > 32)'].append(name)
        if nbits < 8 and by_pointer and ragged and skew:
            took[f'{nbits} bit: scalar by the codes pointer alone, ragged last tile, ct > 32'].append(name)
        if nbits == 8 and ragged and _pow2(n_pol):
            took['8 bit: ragged last tile on the 32 / n_pol pitch'].append(name)
        if n_pol in (1, 2, 3, 4):
            took[f'n_pol = {n_pol}'].append(name)
        if n_pol == 3 and g['ny'] == 1 and g['ct'] * n_pol < 256:
            took[f'3 polarizations (pitch of want = 1, idle threads), {how}'].append(name)
        if g['ny'] > 1 and not _pow2(g['ny']):
            took['few-column route with ny not a power of two'].append(name)
        if g['ny'] > 1 and n_pol == 3:
            took['few-column route with 3 polarizations (pitch of want = 1)'].append(name)
        k, r = divmod(nsblk, g['ts'])
        if k == 0:
            took['nsblk below ts'].append(name)
        if k >= 1 and r == 0:
            took['nsblk an exact multiple of ts'].append(name)
        if k >= 2 and r:
            took['nsblk = k ts + r, k >= 2'].append(name)
            if g['ny'] > 1:
                took['few-column route: nsblk = k ts + r, k >= 2'].append(name)
    return took


# -- fold mode -------------------------------------------------------------------------------------
#: (rows, bins, chan, pol): the fixture's shape; odd bins and a minor axis smaller than any tile;
#: ragged in both directions; one bin; many tiles (16 MiB)
FOLD_OLD = [(1, 2048, 1, 1), (2, 5, 3, 4), (3, 33, 70, 2), (1, 1, 7, 1), (2, 1024, 512, 4)]
#: <4,vec> (a thread owns the tile's four columns) on one column tile with bins 1024 + 2, and on five
#: with fewer bins than a tile; <32,vec> with ragged tiles both ways (columns 32 + 4, bins 128 + 2),
#: again on two rows with more of each (4 x 32 + 12, 2 x 128 + 2), and on a single pair of bins;
#: <4,scalar> with bins 1024 + 1: the half pair falls in the second bin tile
FOLD_NEW = [(2, 1026, 1, 4), (2, 64, 5, 4), (1, 130, 9, 4), (2, 258, 35, 4), (3, 2, 8, 4), (1, 1025, 2, 1)]
FOLD_SHAPES = FOLD_OLD + FOLD_NEW
FOLD_SHIFTED = (1, 64, 16, 4)        # the floats as a view 4 bytes into an allocation: scalar by x / out
FOLD_SHIFTED_CODES = (1, 64, 16, 4)  # the codes 2 bytes into theirs, the floats aligned: scalar by codes


def fold_id(shape):
    return '-'.join(str(v) for v in shape)


def fold_runs(shapes=None, shifted=True, shifted_codes=True):
    """[(name, (rows, bins, chan, pol), floats 16-byte aligned, codes 4-byte aligned)] of what the
    GPU tests launch, encoder and decoder alike."""
    shapes = FOLD_SHAPES if shapes is None else shapes
    runs = [(fold_id(s), s, 1, 1) for s in shapes]
    if shifted:
        runs.append((fold_id(FOLD_SHIFTED) + ' (floats shifted)', FOLD_SHIFTED, 0, 1))
    if shifted_codes:
        runs.append((fold_id(FOLD_SHIFTED_CODES) + ' (codes shifted)', FOLD_SHIFTED_CODES, 1, 0))
    return runs


def fold_ledger(runs, geo):
    """path of the fold-mode kernels -> the names of the runs that take it.  ``geo(shape)`` is
    psrfits_geo_check's line for (bins, chan, pol, floats aligned, codes aligned)."""
    took = {}
    for tc in (32, 4):
        for how in ('vec', 'scalar'):
            took[f'<{tc},{how}> is launched'] = []
    took['<4,vec>: bins = k TB + r'] = []
    took['<4,vec>: several column tiles'] = []
    took['<4,scalar>: odd bins beyond one bin tile (the half pair in a later tile)'] = []
    took['<32,vec>: ragged last column tile'] = []
    took['<32,vec>: a last column tile of one float4'] = []
    took['<32,vec>: bins = k TB + r, k >= 2'] = []
    took['<32,scalar>: ragged last column tile'] = []
    took['bins = 1'] = []
    took['bins = 2, vec'] = []
    took['odd bins'] = []
    took['bins below TB, vec'] = []
    took['bins = k TB, vec'] = []
    took['bins = k TB + r, vec'] = []
    took['scalar by the pointer to the floats alone'] = []
    took['scalar by the pointer to the codes alone'] = []
    for name, (_, n_bin, n_chan, n_pol), x_aligned, codes_aligned in runs:
        g = geo((n_bin, n_chan, n_pol, x_aligned, codes_aligned))
        tc, vec, n_col = g['tc'], bool(g['vec']), n_chan * n_pol
        how = 'vec' if vec else 'scalar'
        took[f'<{tc},{how}> is launched'].append(name)
        k, r = divmod(n_bin, g['tb'])
        ragged = n_col % tc != 0
        if tc == 4 and vec and k >= 1 and r:
            took['<4,vec>: bins = k TB + r'].append(name)
        if tc == 4 and vec and g['n_tile'] > 1:
            took['<4,vec>: several column tiles'].append(name)
        if tc == 4 and not vec and n_bin % 2 and k >= 1:
            took['<4,scalar>: odd bins beyond one bin tile (the half pair in a later tile)'].append(name)
        if tc == 32 and ragged:
            took[f'<32,{how}>: ragged last column tile'].append(name)
        if tc == 32 and vec and n_col % 32 == 4:
            took['<32,vec>: a last column tile of one float4'].append(name)
        if tc == 32 and vec and k >= 2 and r:
            took['<32,vec>: bins = k TB + r, k >= 2'].append(name)
        if n_bin == 1:
            took['bins = 1'].append(name)
        if n_bin == 2 and vec:
            took['bins = 2, vec'].append(name)
        if n_bin % 2:
            took['odd bins'].append(name)
        if vec and k == 0:
            took['bins below TB, vec'].append(name)
        if vec and k >= 1 and r == 0:
            took['bins = k TB, vec'].append(name)
        if vec and k >= 1 and r:
            took['bins = k TB + r, vec'].append(name)
        if not vec and geo((n_bin, n_chan, n_pol, 1, 1))['vec']:
            if not x_aligned and codes_aligned:
                took['scalar by the pointer to the floats alone'].append(name)
            if x_aligned and not codes_aligned:
                took['scalar by the pointer to the codes alone'].append(name)
    return took


def uncovered(took):
    return [path for path, names in took.items() if not names]
